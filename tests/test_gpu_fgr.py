"""dsir_fgr_correspondence (csrc/fgr.hip) through the C ABI with diag on, against the host restatement deepsir_amd/fgr.py.

Exact: the row list, n_rows, trials, the invalid bits, iter_mu, iters_run, the inlier count given the device's own T_out.
Normalisation: a sum of n float64 terms carries at most (n - 1) 2^-53 sum|x| whatever the order, so two orders differ by at most twice
that; the mean adds one rounding: |d mean| <= (2 n + 2) 2^-53 max|x|.  The scale inherits the mean's error plus a handful of roundings:
|d scale| <= (2 n + 8) 2^-53 (max|x| + scale).  Both are asserted as stated.
Trajectory and pose: the device adds the 29 sums of an iteration in another order than numpy, so the two trajectories agree to
rounding, amplified by the optimisation.  The yardstick is the restatement's own sensitivity: over the cases of this file (CASES
below) the fp32 inputs were moved by +-1 ulp at random, 4 draws a case, on the CPU, and the restatement re-run on the same row list.
Measured spread (the largest over all cases and draws): last iter_T 3.9e-08 (normalised frame, max abs entry), T_out rotation
6.7e-08 rad, T_out translation 1.2e-07 m (one fp32 ulp of a 1 - 2 m translation).  Allowed: 4 x that, the margin of test_gpu_icp_plane.py and for the same reason (the
device's summation order is one more perturbation of the size of an input rounding, not a different computation).
The tail: T_out against ransac.refit_sequence / finish started from the device's own candidate pose (its last iter_T un-normalised
with its own norm), 2e-6 rad / 2e-6 m - the bar of test_gpu_consensus.py for its final pose.

Shapes: live counts 3, 4, 63/64/65, 255/256/257 (the selection's block of 256 trials, the optimise workgroup's 256 rows), 1023/1024/
1025, 2000; ragged over the 4 pairs of a call; strides 3 and 6."""
import numpy as np
import pytest
import torch

from deepsir_amd import fgr as F
from deepsir_amd import ransac as R

pytestmark = pytest.mark.gpu
THR = 0.05
DIAG = ("rows", "n_rows", "trials", "norm", "iter_T", "iter_mu", "iter_energy", "iters_run")
SPREAD_ITER_T, SPREAD_ROT, SPREAD_TR = 3.9e-08, 6.7e-08, 1.2e-07      # measured on the CPU (docstring); allowed: 4 x
# (counts of the 4 pairs, stride): M is the largest count
CASES = [((3, 4, 63, 64), 3), ((65, 255, 256, 257), 6), ((1023, 1024, 1025, 2000), 3)]
# seeds found on the host for which, on _cap_problem(), the max_tuples-th accepted trial is the last of a block of 256 (asserted below)
CAP_SEEDS = {1: 1208, 5: 196}


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), max_points=5120, max_pairs=4)
    yield e
    e.close()


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def case_problems(counts):
    return [R.make_problem(max(counts), 0.5, 0.005, 500 + 7 * p + max(counts)) for p in range(len(counts))]


def _cap_problem():
    return R.make_problem(512, 0.8, 0.005, 411)


def _run(eng, probs, counts=None, stride=3, T_init=None, **kw):
    def pad(a):
        return np.concatenate([a, np.full((a.shape[0], stride - 3), 7.0, np.float32)], 1) if stride > 3 else a
    src = np.stack([pad(p["src"]) for p in probs])
    ref = np.stack([pad(p["ref"]) for p in probs])
    corr = np.stack([p["corr"] for p in probs]).astype(np.int32)
    T, stats, invalid, d = eng.fgr_correspondence(_cuda(src), _cuda(ref), _cuda(corr), THR,
                                                  counts=None if counts is None else _cuda(np.asarray(counts, np.int32)),
                                                  T_init=None if T_init is None else _cuda(T_init), diag=True, **kw)
    out = {k: v.cpu().numpy() for k, v in d.items()}
    out.update(T=T.cpu().numpy(), stats=stats.cpu().numpy(), invalid=invalid.cpu().numpy())
    return out


def _rot_angle(A, B):
    d = np.linalg.norm(np.asarray(A)[:, :3].astype(np.float64) - np.asarray(B)[:, :3].astype(np.float64))
    return float(2.0 * np.arcsin(min(1.0, d / (2.0 * np.sqrt(2.0)))))


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _check_pair(out, p, prob, count, T_init=None, **kw):
    """Every comparison of one pair of a device call against the restatement."""
    refine_iters = kw.get("refine_iters", 2)
    want = F.fgr_pair(prob["src"], prob["ref"], prob["corr"], count, max_dist=THR, p=p, T_init=T_init, **kw)
    cs, cq, cnt = want["cs"], want["cq"], want["count"]
    n = want["n_rows"]
    # the list
    assert out["n_rows"][p] == n and out["trials"][p] == want["trials"] and out["invalid"][p] == want["invalid"]
    assert np.array_equal(out["rows"][p][:n], want["rows"]) and (out["rows"][p][n:] == -1).all()
    # the normalisation
    if n >= 3:
        x = np.abs(np.concatenate([cs[want["rows"]], cq[want["rows"]]]).astype(np.float64)).max()
        dn = np.abs(out["norm"][p] - want["norm"])
        print(f"NORM pair {p} n={n}: mean {dn[:6].max():.1e} (bound {(2 * n + 2) * 2.0 ** -53 * x:.1e}), scale {dn[6]:.1e}")
        assert dn[:6].max() <= (2 * n + 2) * 2.0 ** -53 * x
        assert dn[6] <= (2 * n + 8) * 2.0 ** -53 * (x + want["norm"][6])
    else:
        assert (out["norm"][p] == 0).all()
    # the trajectory
    assert out["iters_run"][p] == want["iters_run"]
    assert np.array_equal(out["iter_mu"][p], want["iter_mu"])
    run = int(want["iters_run"]) if want["iters_run"] >= 0 else -int(want["iters_run"]) - 1                # iterations that moved T
    if run > 0:
        dT = np.abs(out["iter_T"][p][run - 1] - want["iter_T"][run - 1]).max()
        de = np.abs(out["iter_energy"][p][:run] - want["iter_energy"][:run]).max()
        print(f"TRAJ pair {p} n={n}: {run} iterations, last iter_T differs by {dT:.1e}, energy by {de:.1e}")
        assert dT <= 4 * SPREAD_ITER_T
    assert (out["iter_T"][p][run:] == 0).all()
    # no pose: T_init and the siblings' stats
    if want["T_candidate"] is None:
        T0 = R.IDENTITY if T_init is None else T_init
        assert _same_bits(out["T"][p], np.asarray(T0, np.float32)) and np.array_equal(out["stats"][p], [0, 0, -1, 0, 0])
        return want
    # the pose
    rot, tr = _rot_angle(out["T"][p], want["T"]), float(np.abs(out["T"][p].astype(np.float64) - want["T"])[:, 3].max())
    print(f"POSE pair {p} n={n}: T_out differs by {rot:.1e} rad, {tr:.1e} m")
    assert rot <= 4 * SPREAD_ROT and tr <= 4 * SPREAD_TR
    assert out["stats"][p][2] == 0 and out["stats"][p][3] == 1
    # the tail, from the device's own candidate
    T_norm = out["iter_T"][p][run - 1] if run > 0 else np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    cand = F.unnormalise(T_norm, out["norm"][p][0:3], out["norm"][p][3:6], out["norm"][p][6]).astype(np.float32)
    thr2 = R.thr2_of(THR)
    Ts, cnts = R.refit_sequence(cand, cs, cq, cnt, thr2, refine_iters)
    T_want, _ = R.finish(Ts, cnts, cs, cq, cnt, thr2, 0, 1)
    assert _rot_angle(out["T"][p], T_want) < 2e-6 and np.abs(out["T"][p][:, 3] - T_want[:, 3]).max() < 2e-6
    assert out["stats"][p][4] == R.count_inliers(out["T"][p], cs, cq, cnt, thr2)    # exact given the device's T_out
    return want


@pytest.mark.parametrize("counts,stride", CASES)
def test_every_stage_against_the_restatement(eng, counts, stride):
    probs = case_problems(counts)
    out = _run(eng, probs, counts, stride=stride, seed=11)
    for p, prob in enumerate(probs):
        want = _check_pair(out, p, prob, counts[p], seed=11)
        if counts[p] >= 63:
            rot, tr = R.pose_error(out["T"][p], prob["T_gt"])
            assert rot < np.radians(1.0) and tr < THR and want["iters_run"] == 64 and want["iter_mu"][-1] < 1.0


@pytest.mark.parametrize("counts,stride", [((64, 257, 1025, 2000), 6)])
def test_without_the_tuple_test(eng, counts, stride):
    probs = case_problems(counts)
    out = _run(eng, probs, counts, stride=stride, tuple_test=False)
    assert out["rows"].shape[1] == max(counts) and (out["trials"] == 0).all()
    for p, prob in enumerate(probs):
        want = _check_pair(out, p, prob, counts[p], tuple_test=False)
        assert np.array_equal(want["rows"], np.arange(counts[p]))


@pytest.mark.parametrize("max_tuples", [1, 5, 1000])
def test_cap_on_the_last_trial_of_a_block_and_never(eng, max_tuples):
    prob = _cap_problem()
    cs, cq, count, _ = R.gather(prob["src"], prob["ref"], prob["corr"])
    if max_tuples in CAP_SEEDS:
        seed = CAP_SEEDS[max_tuples]
        _, ok = F.tuple_trials(cs, cq, count, seed, 0, 0.95, np.arange(F.trials_of(count, 1 << 20)))
        t_cap = int(np.nonzero(ok)[0][max_tuples - 1])
        assert t_cap % 256 == 255                                                   # the cap is reached by a block's last trial
        kw = dict(seed=seed, max_tuples=max_tuples)
    else:
        kw = dict(seed=5, max_tuples=max_tuples, max_trials=2048)                   # 2048 trials at 0.8 outliers: far fewer accepted
    out = _run(eng, [prob], **kw)
    want = _check_pair(out, 0, prob, None, **kw)
    assert (want["n_rows"] == 3 * max_tuples) == (max_tuples in CAP_SEEDS)


def test_max_trials_cuts_the_run_short(eng):
    probs = case_problems((64, 64))
    out = _run(eng, probs, max_trials=300, seed=2)
    assert (out["trials"] == 300).all()
    for p, prob in enumerate(probs):
        full = F.fgr_pair(prob["src"], prob["ref"], prob["corr"], None, max_dist=THR, p=p, seed=2)
        want = _check_pair(out, p, prob, None, max_trials=300, seed=2)
        assert want["n_rows"] < full["n_rows"]


def test_bad_indices_non_finite_points_and_duplicates(eng):
    probs = case_problems((300, 300, 300))
    M = 300
    probs[0]["corr"] = probs[0]["corr"].copy()
    probs[0]["corr"][5] = (-1, 7)
    probs[0]["corr"][77] = (3, M + 9)
    probs[1]["src"] = probs[1]["src"].copy()
    probs[1]["ref"] = probs[1]["ref"].copy()
    probs[1]["src"][::7, 1] = np.nan
    probs[1]["ref"][3::11, 2] = np.inf
    probs[2]["corr"] = probs[2]["corr"].copy()
    probs[2]["corr"][100:200] = probs[2]["corr"][0:100]
    for tt in (True, False):
        out = _run(eng, probs, tuple_test=tt, seed=9)
        assert out["invalid"].tolist() == [2, 0, 0]
        for p, prob in enumerate(probs):
            want = _check_pair(out, p, prob, None, tuple_test=tt, seed=9)
            if p == 1:
                dead = R.is_parked(want["cs"], want["cq"])
                assert dead.sum() > 40 and not dead[want["rows"]].any()


@pytest.mark.parametrize("kw", [dict(division_factor=1.0), dict(division_factor=0.5), dict(iterations=1), dict(refine_iters=0),
                                dict(iterations=7, refine_iters=0, tuple_test=False)])
def test_schedule(eng, kw):
    probs = case_problems((257, 257))
    out = _run(eng, probs, (257, 100), **kw)
    for p, prob in enumerate(probs):
        want = _check_pair(out, p, prob, (257, 100)[p], **kw)
        if kw.get("division_factor", 1.4) <= 1.0:
            assert (want["iter_mu"] == 1.0).all()


def test_exact_rigid_copy(eng):
    probs = [R.make_problem(200, 0.0, 0.0, 77), R.make_problem(200, 0.0, 0.0, 78)]
    out = _run(eng, probs, seed=1)
    for p, prob in enumerate(probs):
        _check_pair(out, p, prob, None, seed=1)
        tr = np.abs(out["T"][p][:, 3] - prob["T_gt"][:, 3]).max()
        assert _rot_angle(out["T"][p], prob["T_gt"]) < 1e-6 and tr < 1e-6 and out["stats"][p][0] == 1.0


def test_solve_refusal_keeps_the_pose(eng):
    """Every listed row on a line parallel to x, the ref side a translated copy: the rotation about x has a zero diagonal entry, the
    solve refuses at iteration 0 and the identity of the normalised frame (a translation by mq - ms) is the candidate."""
    x = np.linspace(-1.0, 1.0, 40, dtype=np.float32)
    src = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)
    ref = (src + np.float32([0.5, 0.25, -0.125])).astype(np.float32)
    prob = {"src": src, "ref": ref, "corr": np.stack([np.arange(40), np.arange(40)], 1).astype(np.int32)}
    out = _run(eng, [prob], tuple_test=False, refine_iters=0)    # no refit: a Kabsch of collinear points has a free rotation about the line
    want = _check_pair(out, 0, prob, None, tuple_test=False, refine_iters=0)
    assert out["iters_run"][0] == -1 and want["iters_run"] == -1
    assert np.abs(out["T"][0] - np.float32([[1, 0, 0, 0.5], [0, 1, 0, 0.25], [0, 0, 1, -0.125]])).max() < 1e-6
    assert out["stats"][0][2] == 0 and out["stats"][0][4] == 40


def test_no_pose_returns_T_init(eng):
    rng = np.random.default_rng(3)
    T_init = rng.normal(size=(4, 3, 4)).astype(np.float32)
    probs = case_problems((64, 64, 64, 64))
    probs[1] = R.make_problem(64, 0.0, 0.005, 31)
    probs[1]["ref"] = (2.0 * probs[1]["ref"]).astype(np.float32)                    # every edge is twice as long: every tuple fails
    probs[2]["src"] = np.full_like(probs[2]["src"], 0.5)                            # all coincident
    probs[2]["ref"] = np.full_like(probs[2]["ref"], -0.25)
    counts = (2, 64, 64, 64)                                                        # pair 0: fewer than 3 rows
    out = _run(eng, probs, counts, T_init=T_init, seed=4)
    for p, prob in enumerate(probs):
        want = _check_pair(out, p, prob, counts[p], T_init=T_init[p], seed=4)
        assert (want["T_candidate"] is None) == (p < 3)
    out = _run(eng, probs[2:3], tuple_test=False)                                   # coincident without the tuple test: scale == 0
    want = _check_pair(out, 0, probs[2], None, tuple_test=False)
    assert want["T_candidate"] is None and want["n_rows"] == 64 and out["norm"][0][6] == 0.0


def test_two_runs_same_bytes_and_pairs_are_independent(eng):
    counts = (64, 257, 1025, 700)
    probs = case_problems(counts)
    seed = 0x1234567
    a = _run(eng, probs, counts, seed=seed)
    b = _run(eng, probs, counts, seed=seed)
    for k in DIAG + ("T", "stats", "invalid"):
        assert _same_bits(a[k], b[k]), k
    for p in range(4):
        one = _run(eng, probs[p:p + 1], counts[p:p + 1], seed=seed ^ (p << 40))
        for k in DIAG + ("T", "stats", "invalid"):
            assert _same_bits(a[k][p], one[k][0]), (k, p)


def test_refusals(eng):
    from deepsir_amd.engine import EngineError
    x = torch.zeros(1, 8, 3, device="cuda")
    c = torch.zeros(1, 8, 2, dtype=torch.int32, device="cuda")
    bad = [dict(tuple_scale=0.0), dict(tuple_scale=1.5), dict(tuple_scale=float("nan")), dict(max_tuples=0),
           dict(max_tuples=eng.FGR_MAX_TUPLES + 1), dict(max_trials=0), dict(max_trials=eng.FGR_MAX_TRIALS + 1), dict(iterations=0),
           dict(iterations=eng.FGR_MAX_ITERS + 1), dict(division_factor=float("nan")), dict(division_factor=float("inf")),
           dict(refine_iters=-1), dict(refine_iters=9)]
    for kw in bad:
        with pytest.raises(EngineError, match="dsir_fgr_correspondence"):
            eng.fgr_correspondence(x, x, c, THR, **kw)
    for md in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(EngineError, match="dsir_fgr_correspondence"):
            eng.fgr_correspondence(x, x, c, md)
    big = torch.zeros(1, eng.max_points + 1, 2, dtype=torch.int32, device="cuda")
    with pytest.raises(EngineError, match="beyond max_points"):
        eng.fgr_correspondence(x, x, big, THR)
    xs = torch.zeros(512, 4, 3, device="cuda")
    cc = torch.zeros(512, 4, 2, dtype=torch.int32, device="cuda")
    with pytest.raises(EngineError, match=r"needs \d+ bytes .* holds \d+"):          # 512 lists of 3 x 65536 rows: 5 GB
        eng.fgr_correspondence(xs, xs, cc, THR, max_tuples=eng.FGR_MAX_TUPLES)
    with pytest.raises(EngineError, match="unsupported"):
        eng.fgr_correspondence(xs, xs, cc, THR, max_trials=eng.FGR_MAX_TRIALS)
    T, stats, invalid = eng.fgr_correspondence(x, x, c, THR)                        # the engine is usable afterwards
    assert np.array_equal(stats.cpu().numpy()[0], [0, 0, -1, 0, 0]) and int(invalid[0]) == 0
