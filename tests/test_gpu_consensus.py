"""dsir_consensus_correspondence (csrc/consensus.hip) through the C ABI with diag on, against the host restatement
deepsir_amd/consensus.py.  Compared exactly: the bit matrix outside the restatement's band, the scores, the seed list, the member
lists, seed validity, the inlier counts given the DEVICE's own seed poses, the pick.  The fits are compared to the float64 Kabsch of
the same members (1e-5 rad / 1e-5 x extent, the bar of test_gpu_ransac.py), the final pose to the restatement's refit started from
the device's winner (2e-6 rad / 2e-6 m).

Shapes: M on both sides of a word (63/64/65), of two words (127/128/129) and of the RANSAC scoring chunk and the scoring
workgroup's 256 rows (255/256/257); M = 1 and 2 (no seed); ragged counts; strides 3 and 6; M = 2000 at 0.97 outliers (8 row
blocks x 4 word chunks of the scoring kernel, 32 column words).  The inputs are random; their bands were checked empty on the host."""
import numpy as np
import pytest
import torch

from deepsir_amd import consensus as Cn
from deepsir_amd import ransac as R

pytestmark = pytest.mark.gpu
EXTENT = 3.0
THR = 0.05
DIAG = ("bits", "score", "seed", "seed_members", "seed_T", "seed_valid", "seed_count")


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
    def pad(a):
        return np.concatenate([a, np.full((a.shape[0], stride - 3), 7.0, np.float32)], 1) if stride > 3 else a
    src = np.stack([pad(p["src"]) for p in probs])
    ref = np.stack([pad(p["ref"]) for p in probs])
    corr = np.stack([p["corr"] for p in probs]).astype(np.int32)
    T, stats, invalid, d = eng.consensus_correspondence(_cuda(src), _cuda(ref), _cuda(corr), THR,
                                                        counts=None if counts is None else _cuda(np.asarray(counts, np.int32)),
                                                        T_init=None if T_init is None else _cuda(T_init), diag=True, **kw)
    out = {k: v.cpu().numpy() for k, v in d.items()}
    out["bits"] = out["bits"].view(np.uint64)
    out.update(T=T.cpu().numpy(), stats=stats.cpu().numpy(), invalid=invalid.cpu().numpy())
    return out


def _rot_angle(A, B):
    d = np.linalg.norm(A[:, :3].astype(np.float64) - B[:, :3].astype(np.float64))
    return float(2.0 * np.arcsin(min(1.0, d / (2.0 * np.sqrt(2.0)))))


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _check_pair(out, p, prob, count, seeds=64, members=32, refine_iters=2, T_init=None):
    """Every comparison of one pair of a device call against the restatement."""
    want = Cn.consensus_pair(prob["src"], prob["ref"], prob["corr"], count, max_dist=THR, seeds=seeds, members=members,
                             refine_iters=refine_iters, T_init=T_init)
    M, cs, cq, n = want["M"], want["cs"], want["cq"], want["count"]
    thr2 = R.thr2_of(THR)
    band = want["band"]
    assert band.sum() <= 1e-4 * M * M
    got_C = Cn.unpack_bits(out["bits"][p], M)
    assert np.array_equal(got_C[~band], want["C"][~band])
    pad = Cn.unpack_bits(out["bits"][p], out["bits"][p].shape[1] * 64)[:, M:]
    assert not pad.any()                                                            # the bits beyond M are 0
    if band.any():                                                                  # downstream of a bit that may differ: not compared
        return want
    assert np.array_equal(out["score"][p], want["score"])
    assert np.array_equal(out["seed"][p], want["seed"])
    assert np.array_equal(out["seed_members"][p], want["seed_members"])
    valid = out["seed_valid"][p].astype(bool)
    assert np.array_equal(valid, want["seed_valid"])
    worst = [0.0, 0.0]
    well = valid & (want["sigma"][:, 1] > 1e-2 * want["sigma"][:, 0])
    for r in np.nonzero(well)[0]:
        worst[0] = max(worst[0], _rot_angle(out["seed_T"][p][r], want["seed_T"][r]))
        worst[1] = max(worst[1], float(np.abs(out["seed_T"][p][r][:, 3].astype(np.float64) - want["seed_T"][r][:, 3]).max()))
    print(f"FITS M={M} pair {p}: {int(valid.sum())} valid seeds, {int(well.sum())} compared, worst {worst[0]:.1e} rad {worst[1]:.1e} m")
    assert worst[0] < 1e-5 and worst[1] < 1e-5 * EXTENT
    assert (out["seed_T"][p][~valid] == 0).all()
    cnt = np.zeros(seeds, np.int64)
    if valid.any():
        cnt[valid] = R.count_inliers(out["seed_T"][p][valid], cs, cq, n, thr2)      # the device's own T bits
    assert np.array_equal(out["seed_count"][p], cnt)
    h = R.pick(valid, out["seed_count"][p])
    assert out["stats"][p][2] == h and out["stats"][p][3] == valid.sum()
    if h < 0:
        T0 = R.IDENTITY if T_init is None else T_init
        assert _same_bits(out["T"][p], np.asarray(T0, np.float32)) and np.array_equal(out["stats"][p], [0, 0, -1, 0, 0])
        return want
    Ts, cnts = R.refit_sequence(out["seed_T"][p][h], cs, cq, n, thr2, refine_iters)
    T_want, st_want = R.finish(Ts, cnts, cs, cq, n, thr2, h, int(valid.sum()))
    assert _rot_angle(out["T"][p], T_want) < 2e-6 and np.abs(out["T"][p][:, 3] - T_want[:, 3]).max() < 2e-6
    assert out["stats"][p][4] == R.count_inliers(out["T"][p], cs, cq, n, thr2)      # exact given the device's T_out
    return want


@pytest.mark.parametrize("M,stride", [(1, 3), (2, 6), (63, 3), (64, 6), (65, 3), (127, 6), (128, 3), (129, 6), (255, 3), (256, 6),
                                      (257, 3)])
def test_every_stage_against_the_restatement(eng, M, stride):
    probs = [R.make_problem(M, 0.5, 0.005, 300 + p) for p in range(2)]
    counts = [M, max(1, (2 * M) // 3)]
    out = _run(eng, probs, counts, stride=stride)
    for p in range(2):
        want = _check_pair(out, p, probs[p], counts[p])
        if M >= 63:
            assert want["seed_valid"].any() and out["stats"][p][2] >= 0
        if M <= 2:
            assert out["stats"][p][2] == -1


def test_ragged_batch(eng):
    probs = [R.make_problem(512, 0.5, 0.005, 320 + p) for p in range(3)]
    counts = [37, 512, 2]
    T_init = np.tile(np.array([[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3]], np.float32), (3, 1, 1))
    out = _run(eng, probs, counts, T_init=T_init)
    for p in range(3):
        _check_pair(out, p, probs[p], counts[p], T_init=T_init[p])
    assert out["stats"][2][2] == -1 and _same_bits(out["T"][2], T_init[2])          # two live rows: no seed, T_init back
    assert (out["score"][0][37:] == 0).all() and not out["bits"][0][37:].any()      # rows beyond count are compatible with nothing


@pytest.mark.parametrize("seeds,members", [(1, 32), (7, 3), (64, 128), (64, 32)])
def test_seeds_and_members(eng, seeds, members):
    assert eng.CONSENSUS_MAX_MEMBERS == Cn.MAX_MEMBERS == 128
    pr = R.make_problem(300, 0.6, 0.005, 330)
    out = _run(eng, [pr], seeds=seeds, members=members)
    assert out["seed"].shape == (1, seeds) and out["seed_members"].shape == (1, seeds, members)
    _check_pair(out, 0, pr, 300, seeds=seeds, members=members)
    assert (out["seed_members"][0] >= 0).sum(1).max() == min(members, 128)


def test_many_outliers_several_tiles(eng):
    pr = R.make_problem(2000, 0.97, 0.005, 340)
    out = _run(eng, [pr])
    _check_pair(out, 0, pr, 2000)
    rot, tr = R.pose_error(out["T"][0], pr["T_gt"])
    print(f"RECOVERY M=2000 at 0.97 outliers: inliers {int(out['stats'][0][4])} of {int(pr['inlier'].sum())} true, {rot:.1e} rad {tr:.1e} m")
    assert rot < 5e-3 and tr < 5e-3


def test_ties_go_to_the_lower_index(eng):
    # two copies of one structure: scores and S2 values tie in pairs, every seed pose counts the same inliers
    a = R.make_problem(100, 0.3, 0.0, 60)
    pr = {"src": np.concatenate([a["src"], a["src"]]), "ref": np.concatenate([a["ref"], a["ref"]]),
          "corr": np.stack([np.arange(200), np.arange(200)], 1).astype(np.int32)}
    out = _run(eng, [pr], seeds=8, members=9)
    want = _check_pair(out, 0, pr, 200, seeds=8, members=9)
    sc = want["score"]
    assert sc[out["seed"][0][0]] == sc[out["seed"][0][0] + 100] and out["seed"][0][0] < 100     # the copy ties and loses
    assert out["stats"][0][2] == 0                                                              # equal counts: the lower rank


def test_pairs_are_independent_and_runs_repeat(eng):
    probs = [R.make_problem(512, 0.8, 0.005, 350 + p) for p in range(4)]
    counts = [512, 300, 2, 37]
    keys = ("T", "stats", "invalid") + DIAG
    a = _run(eng, probs, counts)
    b = _run(eng, probs, counts)
    for k in keys:
        assert _same_bits(a[k], b[k]), k
    for p in range(4):
        one = _run(eng, [probs[p]], [counts[p]])
        for k in keys:
            assert _same_bits(a[k][p], one[k][0]), (k, p)


def test_edge_cases(eng):
    from deepsir_amd.engine import EngineError
    good = R.make_problem(128, 0.3, 0.005, 80)
    nan = R.make_problem(128, 0.3, 0.005, 81)
    nan["src"][[3, 50]] = np.nan
    nan["ref"][9, 2] = np.inf
    oob = R.make_problem(128, 0.3, 0.005, 82)
    oob["corr"] = oob["corr"].copy()
    oob["corr"][5] = (-3, 1 << 20)
    out = _run(eng, [good, nan, oob], [128, 128, 128])
    assert np.array_equal(out["invalid"], [0, 0, 2])                                # a clamped index raises bit 2
    for p, pr in enumerate((good, nan, oob)):
        _check_pair(out, p, pr, 128)
    for row in (3, 9, 50):                                                          # parked rows: compatible with nothing, never members
        assert not out["bits"][1][row].any() and out["score"][1][row] == 0
    assert not np.isin(out["seed_members"][1], [3, 9, 50]).any()
    assert np.isfinite(out["T"]).all() and np.isfinite(out["stats"]).all()
    ref_run = _run(eng, [good, good, oob], [128, 128, 128])                         # the neighbours of the NaN pair keep their bits
    for k in ("T", "stats") + DIAG:
        for p in (0, 2):
            assert _same_bits(out[k][p], ref_run[k][p]), (k, p)
    # bad arguments and a problem the arena cannot hold are errors before any launch, never faults
    x, c = _cuda(good["src"][None]), _cuda(good["corr"][None].astype(np.int32))
    for kw in (dict(seeds=0), dict(seeds=eng.CONSENSUS_MAX_SEEDS + 1), dict(members=2), dict(members=eng.CONSENSUS_MAX_MEMBERS + 1),
               dict(refine_iters=-1), dict(refine_iters=9)):
        with pytest.raises(EngineError, match="consensus"):
            eng.consensus_correspondence(x, x, c, THR, **kw)
    with pytest.raises(EngineError, match="bad arguments"):
        eng.consensus_correspondence(x, x, c, 0.0)
    big = torch.zeros(1, eng.max_points + 1, 2, dtype=torch.int32, device="cuda")
    with pytest.raises(EngineError, match="max_points"):
        eng.consensus_correspondence(x, x, big, THR)
    T, stats, _ = eng.consensus_correspondence(x, x, c, THR)                        # and the context still works
    assert stats[0, 4] == 128


def test_too_large_for_the_arena_is_refused():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine, EngineError
    e = Engine(NetConfig(), max_points=32768, max_pairs=1)                          # an arena of about 0.8 GB
    try:
        M = e.CONSENSUS_MAX_M                                                       # 75 MB of bit matrix a pair: 16 pairs need 1.2 GB
        x = torch.zeros(16, 4, 3, device="cuda")
        c = torch.zeros(16, M + 1, 2, dtype=torch.int32, device="cuda")
        with pytest.raises(EngineError, match=r"needs \d+ bytes .* holds \d+"):
            e.consensus_correspondence(x, x, c[:, :M].contiguous(), THR)
        with pytest.raises(EngineError, match="DSIR_CONSENSUS_MAX_M"):
            e.consensus_correspondence(x[:1], x[:1], c[:1], THR)
    finally:
        e.close()


def test_register_fpfh_pose_routes():
    from deepsir_amd import fpfh as F
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    from deepsir_amd.harness import evaluate_align, register_fpfh
    from deepsir_amd.metrics import THRESHOLDS, rte_rre
    from deepsir_amd.weights import generate_state_dict
    cfg = NetConfig()
    e = Engine(cfg, max_points=2048, max_pairs=2)
    try:
        e.load_state_dict(generate_state_dict(cfg, 0))
        pairs = [F.bumpy_pair(1), F.bumpy_pair(2)]
        kw = dict(voxel_size=0.05, batch=2, num_reg=2)
        plain, _ = register_fpfh(pairs, e, hypotheses=1024, **kw)
        named, _ = register_fpfh(pairs, e, hypotheses=1024, pose="ransac", **kw)
        assert _same_bits(plain, named)                                             # the default route is untouched
        pred, stats = register_fpfh(pairs, e, pose="consensus", **kw)
        assert pred.shape == (2, 2, 3, 4) and stats.shape == (2, 5) and np.isfinite(pred).all() and np.isfinite(stats).all()
        assert np.array_equal(pred[:, 0], pred[:, 1])
        for T, pr in zip(pred[:, 0], pairs):
            assert np.abs(T[:, :3] @ T[:, :3].T - np.eye(3)).max() < 1e-5 and np.linalg.det(T[:, :3]) > 0.999
            assert rte_rre(T, pr["transform_gt"][0], *THRESHOLDS["3DMatch"])[0] == 1.0
        again, _ = register_fpfh(pairs, e, pose="consensus", **kw)
        assert _same_bits(pred, again)
        metrics, _ = evaluate_align(pred, pairs, e)
        assert len(metrics) == 2 and all(np.isfinite(v).all() for v in metrics[-1].values())
        with pytest.raises(ValueError):
            register_fpfh(pairs, e, pose="nope", **kw)
    finally:
        e.close()
