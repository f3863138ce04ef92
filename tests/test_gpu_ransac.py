"""dsir_ransac_correspondence and dsir_feature_correspondences (csrc/ransac.hip) through the C ABI, against the host restatement
deepsir_amd/ransac.py.  Everything integer is compared exactly: the draws, the inlier counts given the DEVICE's own transforms, the
pick.  The fits are compared to the float64 fit of the same sample, the refit to the restatement's refit started from the device's
winner (2e-6 rad / 2e-6 m, the bar of the Kabsch tests).

Shapes: H = 300 (no multiple of 64, 128 or 256: partial fitting and scoring workgroups), ragged counts, M on both sides of the
wave (63/64/65) and of the scoring chunk (255/256/257, DSIR_RANSAC_CHUNK), M = 5000 (several slices of several chunks), stride 3 and 6."""
import numpy as np
import pytest
import torch

from deepsir_amd import ransac as R

pytestmark = pytest.mark.gpu
EXTENT = 3.0          # make_problem's cube
THR = 0.05


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), max_points=5120, max_pairs=4)
    yield e
    e.close()


def _cuda(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def _run(eng, probs, counts=None, stride=3, T_init=None, **kw):
    """probs: list of make_problem dicts of one M -> numpy outputs of one device call (diag on)."""
    def pad(a):
        return np.concatenate([a, np.full((a.shape[0], stride - 3), 7.0, np.float32)], 1) if stride > 3 else a
    src = np.stack([pad(p["src"]) for p in probs])
    ref = np.stack([pad(p["ref"]) for p in probs])
    corr = np.stack([p["corr"] for p in probs]).astype(np.int32)
    kw.setdefault("hypotheses", 300)
    T, stats, invalid, d = eng.ransac_correspondence(_cuda(src), _cuda(ref), _cuda(corr), THR,
                                                     counts=None if counts is None else _cuda(np.asarray(counts, np.int32)),
                                                     T_init=None if T_init is None else _cuda(T_init), diag=True, **kw)
    out = {k: v.cpu().numpy() for k, v in d.items()}
    out.update(T=T.cpu().numpy(), stats=stats.cpu().numpy(), invalid=invalid.cpu().numpy())
    return out


def _rot_angle(A, B):
    """Angle between two rotations from |A - B|_F = 2 sqrt(2) sin(angle / 2): well conditioned at small angles, where the arccos of
    the trace of fp32-rounded matrices resolves no better than sqrt(2 x 1e-7) = 4e-4 rad."""
    d = np.linalg.norm(A[:, :3].astype(np.float64) - B[:, :3].astype(np.float64))
    return float(2.0 * np.arcsin(min(1.0, d / (2.0 * np.sqrt(2.0)))))


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("n", [3, 4])
def test_samples_fits_and_verdicts(eng, n):
    probs = [R.make_problem(512, 0.5, 0.005, 20 + p) for p in range(3)]
    counts, H, seed = [37, 512, 2], 300, 77
    out = _run(eng, probs, counts, ransac_n=n, seed=seed)
    thr2 = R.thr2_of(THR)
    for p in range(3):
        cs, cq, count, _ = R.gather(probs[p]["src"], probs[p]["ref"], probs[p]["corr"], counts[p])
        rows = R.sample_rows(seed, p, np.arange(H), n, count)
        assert np.array_equal(out["hyp_sample"][p], rows)                                   # the draws, exactly
        repeat = np.array([len(set(r[:n])) < n for r in rows])
        assert not out["hyp_valid"][p][repeat].any()
        if count < n:
            assert not out["hyp_valid"][p].any() and out["stats"][p][2] == -1
            continue
        hyp = R.hypotheses(cs, cq, count, rows, n, thr2, 0.9)
        valid = out["hyp_valid"][p].astype(bool)
        sure = hyp["margin"] > 1e-4
        assert np.array_equal(valid[sure], hyp["valid"][sure])                              # verdicts away from the thresholds
        assert not valid[~hyp["fitted"]].any()
        well = valid & hyp["valid"] & (hyp["sigma"][:, 1] > 1e-2 * hyp["sigma"][:, 0])
        assert valid.sum() > 0 and well.sum() >= 0.9 * valid.sum(), (valid.sum(), well.sum())
        worst = [0.0, 0.0]
        for h in np.nonzero(well)[0]:
            worst[0] = max(worst[0], _rot_angle(out["hyp_T"][p][h], hyp["T"][h]))
            worst[1] = max(worst[1], float(np.abs(out["hyp_T"][p][h][:, 3].astype(np.float64) - hyp["T"][h][:, 3]).max()))
        print(f"FITS n={n} pair {p}: {int(valid.sum())} valid, {int(well.sum())} compared, worst {worst[0]:.1e} rad {worst[1]:.1e} m")
        assert worst[0] < 1e-5 and worst[1] < 1e-5 * EXTENT


@pytest.mark.parametrize("M,stride", [(1, 3), (63, 6), (64, 3), (65, 6), (255, 3), (256, 6), (257, 3), (512, 6), (5000, 3)])
def test_counts_and_pick_are_exact(eng, M, stride):
    probs = [R.make_problem(M, 0.3, 0.005, 40 + p) for p in range(3)]
    counts = [M, max(1, (2 * M) // 3), max(1, M // 2 + 1)]
    out = _run(eng, probs, counts, stride=stride, seed=5)
    thr2 = R.thr2_of(THR)
    for p in range(3):
        cs, cq, count, _ = R.gather(probs[p]["src"], probs[p]["ref"], probs[p]["corr"], counts[p])
        valid = out["hyp_valid"][p].astype(bool)
        want = np.zeros(300, np.int64)
        if valid.any():
            want[valid] = R.count_inliers(out["hyp_T"][p][valid], cs, cq, count, thr2)      # the device's own T bits
        assert np.array_equal(out["hyp_count"][p], want), (M, p)
        h = R.pick(valid, out["hyp_count"][p])
        assert out["stats"][p][2] == h and out["stats"][p][3] == valid.sum()
        if M >= 63:
            assert valid.any()


def test_ties_go_to_the_lower_hypothesis(eng):
    # two copies of one noise-free structure: every hypothesis drawn from inliers counts all of them
    a = R.make_problem(100, 0.3, 0.0, 60)
    pr = {"src": np.concatenate([a["src"], a["src"]]), "ref": np.concatenate([a["ref"], a["ref"]]),
          "corr": np.stack([np.arange(200), np.arange(200)], 1).astype(np.int32)}
    out = _run(eng, [pr], seed=9)
    valid, cnt = out["hyp_valid"][0].astype(bool), out["hyp_count"][0]
    top = cnt[valid].max()
    tied = np.nonzero(valid & (cnt == top))[0]
    assert top == 2 * int(a["inlier"].sum()) and len(tied) >= 2
    assert out["stats"][0][2] == tied[0] == R.pick(valid, cnt)


@pytest.mark.parametrize("case,n", [("A", 3), ("B", 3), ("C", 3), ("A", 4), ("B", 4), ("C", 4)])
def test_recovery_and_refit(eng, case, n):
    M, frac, H = {"A": (512, 0.6, 2048), "B": (512, 0.8, 4096), "C": (37, 0.5, 512)}[case]
    pr = R.make_problem(M, frac, 0.005, seed={"A": 11, "B": 12, "C": 13}[case])
    out = _run(eng, [pr], hypotheses=H, ransac_n=n, seed=2024)
    rot, tr = R.pose_error(out["T"][0], pr["T_gt"])
    print(f"RECOVERY case {case} n={n}: winner {int(out['stats'][0][2])}, {int(out['stats'][0][3])} valid, inliers {int(out['stats'][0][4])} "
          f"of {int(pr['inlier'].sum())} true, pose error {rot:.1e} rad {tr:.1e} m")
    assert rot < 0.01 and tr < 0.01
    # the refit, restated from the device's winning transform
    cs, cq, count, _ = R.gather(pr["src"], pr["ref"], pr["corr"])
    thr2 = R.thr2_of(THR)
    h = int(out["stats"][0][2])
    Ts, cnts = R.refit_sequence(out["hyp_T"][0][h], cs, cq, count, thr2, 2)
    T_want, st_want = R.finish(Ts, cnts, cs, cq, count, thr2, h, int(out["hyp_valid"][0].sum()))
    assert _rot_angle(out["T"][0], T_want) < 2e-6 and np.abs(out["T"][0][:, 3] - T_want[:, 3]).max() < 2e-6
    d_inl = abs(out["stats"][0][4] - st_want[4])
    if d_inl:
        d2 = R.residual2(out["T"][0], cs, cq).astype(np.float64)
        k = int(np.argmin(np.abs(d2 - float(thr2))))
        print(f"REFIT one off: residual {d2[k]!r} against thr^2 {float(thr2)!r}")
        assert d_inl == 1 and abs(d2[k] - float(thr2)) <= 1e-6 * float(thr2)
    else:
        assert out["stats"][0][0] == out["stats"][0][4] / count
        assert abs(out["stats"][0][1] - st_want[1]) < 2e-6
    assert out["stats"][0][4] == R.count_inliers(out["T"][0], cs, cq, count, thr2)          # exact given the device's T_out


def test_pairs_are_independent_and_runs_repeat(eng):
    probs = [R.make_problem(512, 0.5, 0.005, 70 + p) for p in range(4)]
    counts, seed = [512, 300, 2, 37], 31
    keys = ("T", "stats", "invalid", "hyp_sample", "hyp_T", "hyp_valid", "hyp_count")
    a = _run(eng, probs, counts, seed=seed)
    b = _run(eng, probs, counts, seed=seed)
    for k in keys:
        assert _same_bits(a[k], b[k]), k
    for p in range(4):                                       # pair p of a call is pair 0 of a call with seed ^ (p << 40)
        one = _run(eng, [probs[p]], [counts[p]], seed=seed ^ (p << 40))
        for k in keys:
            assert _same_bits(a[k][p], one[k][0]), (k, p)
    big = _run(eng, probs, counts, seed=seed, hypotheses=1000)
    for k in ("hyp_sample", "hyp_T", "hyp_valid", "hyp_count"):
        assert _same_bits(a[k], big[k][:, :300]), k


def test_edge_cases(eng):
    from deepsir_amd.engine import EngineError
    rng = np.random.default_rng(3)
    good = R.make_problem(128, 0.3, 0.005, 80)
    junk = dict(good, ref=rng.uniform(-50, 50, (128, 3)).astype(np.float32))               # no structure: nothing survives the checks
    nan = R.make_problem(128, 0.3, 0.005, 81)
    nan["src"][[3, 50]] = np.nan
    nan["ref"][9, 2] = np.inf
    oob = R.make_problem(128, 0.3, 0.005, 82)
    oob["corr"] = oob["corr"].copy()
    oob["corr"][5] = (-3, 1 << 20)
    T_init = np.tile(np.array([[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3]], np.float32), (4, 1, 1))
    out = _run(eng, [good, junk, nan, oob], [2, 128, 128, 128], T_init=T_init, seed=4)
    for p in (0, 1):                                         # count < n; all outliers
        assert not out["hyp_valid"][p].any() and _same_bits(out["T"][p], T_init[p])
        assert np.array_equal(out["stats"][p], [0, 0, -1, 0, 0])
    assert np.array_equal(out["invalid"], [0, 0, 0, 2])
    # the NaN pair: never sampled, never counted, finite result equal to the restatement's count
    bad = np.isin(out["hyp_sample"][2][:, :3], [3, 9, 50]).any(1)
    assert bad.any() and not out["hyp_valid"][2][bad].any()
    assert np.isfinite(out["T"]).all() and np.isfinite(out["stats"]).all()
    cs, cq, count, _ = R.gather(nan["src"], nan["ref"], nan["corr"])
    assert out["stats"][2][4] == R.count_inliers(out["T"][2], cs, cq, count, R.thr2_of(THR)) > 0
    rot, tr = R.pose_error(out["T"][2], nan["T_gt"])
    assert rot < 0.01 and tr < 0.01
    # the out-of-range row was clamped as the restatement clamps it
    cs, cq, count, inv = R.gather(oob["src"], oob["ref"], oob["corr"])
    assert inv == 2 and out["stats"][3][4] == R.count_inliers(out["T"][3], cs, cq, count, R.thr2_of(THR))
    # the neighbours of the NaN pair keep their bits
    ref_run = _run(eng, [good, junk, good, oob], [2, 128, 128, 128], T_init=T_init, seed=4)
    for k in ("T", "stats", "hyp_T", "hyp_count"):
        for p in (0, 1, 3):
            assert _same_bits(out[k][p], ref_run[k][p]), (k, p)
    # bad arguments are errors, never aborts
    x, c = _cuda(good["src"][None]), _cuda(good["corr"][None].astype(np.int32))
    for kw in (dict(ransac_n=2), dict(ransac_n=5), dict(hypotheses=0), dict(hypotheses=eng.RANSAC_MAX_HYPOTHESES + 1),
               dict(refine_iters=-1), dict(refine_iters=9)):
        with pytest.raises(EngineError, match="ransac"):
            eng.ransac_correspondence(x, x, c, THR, **kw)
    with pytest.raises(EngineError, match="bad arguments"):
        eng.ransac_correspondence(x, x, c, 0.0)
    big = torch.zeros(1, eng.max_points + 1, 2, dtype=torch.int32, device="cuda")
    with pytest.raises(EngineError, match="max_points"):
        eng.ransac_correspondence(x, x, big, THR)
    T, stats, _ = eng.ransac_correspondence(x, x, c, THR, hypotheses=64)                   # and the context still works
    assert stats[0, 4] == 128


@pytest.mark.parametrize("mutual", [True, False])
@pytest.mark.parametrize("J,K", [(1, 1), (65, 300), (512, 512)])
def test_feature_correspondences(eng, J, K, mutual):
    rng = np.random.default_rng(J + K)
    a = rng.normal(size=(2, J, 64)).astype(np.float32)
    a /= np.linalg.norm(a, axis=2, keepdims=True)
    b = rng.normal(size=(2, K, 64)).astype(np.float32)
    b /= np.linalg.norm(b, axis=2, keepdims=True)
    if K >= 65:                                              # duplicated descriptors: exact ties, which go to the lower index
        b[:, 10] = a[:, 5]
        b[:, 40] = a[:, 5]
        b[:, 41] = a[:, 7]
        a[:, 60] = a[:, 7]
    corr, counts = eng.feature_correspondences(_cuda(a), _cuda(b), mutual=mutual)
    corr, counts = corr.cpu().numpy(), counts.cpu().numpy()
    for p in range(2):
        want, n = R.feature_correspondences(a[p], b[p], mutual)
        assert counts[p] == n and np.array_equal(corr[p], want), (p, counts[p], n)
        assert (corr[p][n:] == -1).all()
    if K >= 65:
        row = corr[0][corr[0][:, 0] == 5]
        assert len(row) == 1 and row[0, 1] == 10


def test_descriptors_to_pose(eng):
    # ground-truth-consistent descriptors: desc_ref is desc_src permuted, the ref points are the moved src points permuted
    rng = np.random.default_rng(5)
    P, N = 2, 2048
    desc = rng.normal(size=(P, N, 64)).astype(np.float32)
    desc /= np.linalg.norm(desc, axis=2, keepdims=True)
    probs = [R.make_problem(N, 0.0, 0.0, 90 + p) for p in range(P)]
    perm = [rng.permutation(N) for _ in range(P)]
    src = np.stack([p["src"] for p in probs])
    ref = np.stack([p["ref"][q] for p, q in zip(probs, perm)])
    dref = np.stack([desc[p][perm[p]] for p in range(P)])
    corr, counts = eng.feature_correspondences(_cuda(desc), _cuda(dref), mutual=True)
    assert counts.cpu().tolist() == [N, N]
    T, stats, invalid = eng.ransac_correspondence(_cuda(src), _cuda(ref), corr, THR, counts=counts, hypotheses=256)
    for p in range(P):
        rot, tr = R.pose_error(T[p].cpu().numpy(), probs[p]["T_gt"])
        assert rot < 1e-3 and tr < 1e-3 and stats[p, 0] == 1.0


def _network(pipeline, num_sub):
    from types import SimpleNamespace
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.model import Network
    from deepsir_amd.weights import generate_state_dict, to_torch_state_dict
    args = SimpleNamespace(pipeline=pipeline, num_sub=num_sub, feat_len=3, num_knn=16, out_feat_dim=64, d_out=[16, 64, 128, 256],
                           sub_sampling_ratio=[4, 4, 4, 4], clip_weight_thresh=0.0, use_ppf=False, num_points=2048)
    net = Network(args)
    net.load_state_dict(to_torch_state_dict(generate_state_dict(NetConfig(feat_len=3, pipeline=pipeline, num_sub=num_sub), 0)), strict=True)
    return net.cuda().eval()


def test_register_feat_end_to_end():
    from deepsir_amd.harness import evaluate_align, register_feat
    from deepsir_amd.synth import make_pair
    net = _network("feat", 512)
    pairs = [make_pair(2048, s, 3) for s in (51, 52)]
    pred, stats = register_feat(pairs, net, voxel_size=0.05, hypotheses=1024, mutual=True, num_reg=2, batch=2)
    assert pred.shape == (2, 2, 3, 4) and stats.shape == (2, 5) and np.isfinite(pred).all() and np.isfinite(stats).all()
    for T in pred[:, 0]:
        assert np.abs(T[:, :3] @ T[:, :3].T - np.eye(3)).max() < 1e-5 and np.linalg.det(T[:, :3]) > 0.999
    assert np.array_equal(pred[:, 0], pred[:, 1]) and (stats[:, 3] > 0).all()
    metrics, _ = evaluate_align(pred, pairs, net._ensure_engine(2048, 2))
    assert len(metrics) == 2 and all(np.isfinite(v).all() for v in metrics[-1].values())


def test_inference_align_ransac_safeguard():
    from deepsir_amd.harness import inference_align
    from deepsir_amd.synth import make_pair
    net = _network("align", -1)
    pairs = [make_pair(2048, s, 3) for s in (41, 42)]
    plain, _ = inference_align(pairs, net, 3, batch=2)
    safe, stats = inference_align(pairs, net, 3, batch=2, pose_opt="ransac", voxel_size=0.05, ransac_hypotheses=1024)
    assert plain.shape == safe.shape == (2, 4, 3, 4) and np.array_equal(plain[:, :3], safe[:, :3]) and np.isfinite(safe).all()
    for T in safe[:, 3]:
        assert np.abs(T[:, :3] @ T[:, :3].T - np.eye(3)).max() < 1e-5
    kept, _ = inference_align(pairs, net, 3, batch=2, pose_opt="ransac", voxel_size=0.05, ransac_hypotheses=1024, safeguard_wsum=0.0)
    assert _same_bits(kept[:, 3], plain[:, 2]) and _same_bits(kept, plain)
    with pytest.raises(ValueError):
        inference_align(pairs, net, 3, batch=2, pose_opt="nope")
