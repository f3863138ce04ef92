"""The host restatement of the RANSAC pose rule (deepsir_amd/ransac.py; the device side is csrc/ransac.hip): draws, the exact
fp32 residual, recovery on synthetic problems with fixed seeds, and the edge cases.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from deepsir_amd import ransac as R
from deepsir_amd.augment import MASK, splitmix64

# (M, outlier fraction, hypotheses); noise sigma 5 mm, threshold 0.05 m
CASES = {"A": (512, 0.6, 2048), "B": (512, 0.8, 4096), "C": (37, 0.5, 512)}


def test_draws_follow_the_formula_and_nothing_else():
    seed, count = 0x1234ABCD, 37
    for p, h, k in [(0, 0, 0), (2, 299, 2), (7, 79999, 3), (1000, 1 << 19, 1)]:
        d = splitmix64(splitmix64((seed ^ (p << 40)) & MASK) ^ ((h << 8) & MASK) ^ k)
        assert R.sample_rows(seed, p, [h], 4, count)[0, k] == ((d >> 32) * count) >> 32
    # the rows of (seed, p, h, k) do not depend on how many hypotheses or pairs are drawn
    small, large = R.sample_rows(seed, 3, np.arange(300), 3, count), R.sample_rows(seed, 3, np.arange(5000), 3, count)
    assert np.array_equal(small, large[:300]) and (small[:, 3] == -1).all() and (small[:, :3] >= 0).all() and (small[:, :3] < count).all()
    one = [R.ransac_pair(pr["src"], pr["ref"], pr["corr"], hypotheses_n=64, seed=5, p=p)["hyp_sample"]
           for p, pr in enumerate([R.make_problem(37, 0.5, 0.005, 1)] * 3)]
    batch = R.ransac([R.make_problem(37, 0.5, 0.005, 1)["src"]] * 3, [R.make_problem(37, 0.5, 0.005, 1)["ref"]] * 3,
                     [R.make_problem(37, 0.5, 0.005, 1)["corr"]] * 3, hypotheses_n=200, seed=5)
    for p in range(3):
        assert np.array_equal(one[p], batch[p]["hyp_sample"][:64])
    assert not np.array_equal(one[0], one[1])            # the pair index does enter


def test_draws_are_uniform():
    count, n_draws = 37, 100000
    rows = R.sample_rows(99, 0, np.arange(n_draws // 4), 4, count).reshape(-1)[:n_draws]
    obs = np.bincount(rows, minlength=count).astype(np.float64)
    chi2 = float(((obs - n_draws / count) ** 2 / (n_draws / count)).sum())
    dof = count - 1
    print(f"chi2 = {chi2:.1f} at {dof} degrees of freedom")
    assert chi2 < dof + 5.0 * np.sqrt(2.0 * dof)         # five standard deviations of a chi-square variable


def _round_f32(v: Fraction) -> np.float32:
    f = np.float32(float(v))
    cands = {float(f), float(np.nextafter(f, np.float32(np.inf))), float(np.nextafter(f, np.float32(-np.inf)))}
    best = sorted(cands, key=lambda c: (abs(Fraction(c) - v), np.float32(c).view(np.uint32) & 1))
    return np.float32(best[0])


def test_fma32_is_the_correctly_rounded_fused_multiply_add():
    rng = np.random.default_rng(3)
    a = rng.normal(size=400).astype(np.float32)
    b = rng.normal(size=400).astype(np.float32) * np.float32(10)
    c = (-(a.astype(np.float64) * b)).astype(np.float32) * (1 + rng.integers(-2, 3, 400).astype(np.float32) * np.float32(2.0 ** -20))
    # products whose sum with c sits next to an fp32 rounding boundary: where rounding twice (float64, then fp32) goes wrong
    a[:50], b[:50], c[:50] = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23), (rng.integers(1, 1 << 20, 50) * 2.0 ** -1).astype(np.float32)
    got = R.fma32(a, b, c)
    for i in range(400):
        want = _round_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i] == want, (i, a[i], b[i], c[i], got[i], want)


@pytest.mark.parametrize("n", [3, 4])
@pytest.mark.parametrize("case", sorted(CASES))
def test_recovery(case, n):
    M, frac, H = CASES[case]
    pr = R.make_problem(M, frac, 0.005, seed={"A": 11, "B": 12, "C": 13}[case])
    res = R.ransac_pair(pr["src"], pr["ref"], pr["corr"], max_dist=0.05, ransac_n=n, edge_sim=0.9, hypotheses_n=H, refine_iters=2,
                        seed=2024)
    truth = int(pr["inlier"].sum())
    h = res["h"]
    print(f"case {case} n={n}: {int(res['hyp_valid'].sum())} valid hypotheses, winner {h} count {res['hyp_count'][h]} "
          f"(true inliers {truth}), pose error before / after refit {R.pose_error(res['T_winner'], pr['T_gt'])} / {R.pose_error(res['T'], pr['T_gt'])}")
    assert h >= 0 and res["hyp_valid"][h]
    assert abs(int(res["hyp_count"][h]) - truth) <= 0.02 * truth
    assert h == R.pick(res["hyp_valid"], res["hyp_count"])
    # every valid hypothesis counts at least its own sample
    assert (res["hyp_count"][res["hyp_valid"]] >= n).all() and (res["hyp_count"][~res["hyp_valid"]] == 0).all()
    rot, tr = R.pose_error(res["T"], pr["T_gt"])
    assert rot < 0.01 and tr < 0.01
    assert res["stats"][4] >= res["hyp_count"][h] and res["stats"][0] == res["stats"][4] / M and res["stats"][2] == h


def test_count_below_n_has_no_valid_hypothesis():
    pr = R.make_problem(37, 0.0, 0.0, 4)
    T_init = np.array([[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3]], np.float32)
    for n, count in [(3, 2), (4, 3), (3, 0)]:
        res = R.ransac_pair(pr["src"], pr["ref"], pr["corr"], count=count, ransac_n=n, hypotheses_n=128, T_init=T_init)
        assert not res["hyp_valid"].any() and res["h"] == -1
        assert np.array_equal(res["T"], T_init) and np.array_equal(res["stats"], [0, 0, -1, 0, 0])
    res = R.ransac_pair(pr["src"], pr["ref"], pr["corr"], count=2, hypotheses_n=16)
    assert np.array_equal(res["T"], R.IDENTITY)


def test_identical_points_give_a_finite_pose():
    # every sample is degenerate (zero covariance): the fit falls back to R = I and the translation between the two points,
    # which maps every row exactly - a valid hypothesis under the rule, finite, and nothing divides by zero
    src = np.tile(np.float32([1.0, 2.0, 3.0]), (20, 1))
    ref = np.tile(np.float32([1.5, 2.0, 2.0]), (20, 1))
    corr = np.stack([np.arange(20), np.arange(20)], 1)
    res = R.ransac_pair(src, ref, corr, hypotheses_n=64)
    assert np.isfinite(res["T"]).all() and np.isfinite(res["stats"]).all()
    assert np.abs(R.transform_points(res["T"], src) - ref).max() < 1e-5 and res["stats"][0] == 1.0


def test_nan_points_are_never_inliers_and_never_sampled():
    pr = R.make_problem(64, 0.25, 0.002, 5)
    src, ref = pr["src"].copy(), pr["ref"].copy()
    src[[3, 10]] = np.nan
    ref[17, 1] = np.inf
    res = R.ransac_pair(src, ref, pr["corr"], hypotheses_n=512, seed=8)
    bad = np.isin(res["hyp_sample"][:, :3], [3, 10, 17]).any(1)
    assert bad.any() and not res["hyp_valid"][bad].any()
    assert np.isfinite(res["T"]).all() and np.isfinite(res["stats"]).all()
    truth = int(pr["inlier"].sum() - pr["inlier"][[3, 10, 17]].sum())
    assert res["stats"][4] == truth
    rot, tr = R.pose_error(res["T"], pr["T_gt"])
    assert rot < 0.01 and tr < 0.01
    # a pair of nothing but NaN: no valid hypothesis, T_init back, fitness 0
    res = R.ransac_pair(np.full((8, 3), np.nan, np.float32), ref[:8], pr["corr"][:8], hypotheses_n=32)
    assert res["h"] == -1 and np.array_equal(res["T"], R.IDENTITY) and res["stats"][0] == 0.0


def test_out_of_range_indices_are_clamped_and_flagged():
    pr = R.make_problem(37, 0.0, 0.0, 6)
    corr = pr["corr"].copy()
    corr[5] = (-4, 1000)
    cs, cq, count, invalid = R.gather(pr["src"], pr["ref"], corr)
    assert invalid == 2 and np.array_equal(cs[5], pr["src"][0]) and np.array_equal(cq[5], pr["ref"][36])
    assert R.gather(pr["src"], pr["ref"], corr, count=5)[3] == 0       # the bad row is not live


def test_feature_correspondences_restatement():
    rng = np.random.default_rng(0)
    a = rng.normal(size=(6, 64))
    b = np.concatenate([a[[4, 2, 0]], a[[2]], rng.normal(size=(2, 64))])   # ref rows 1 and 3 are the same descriptor
    corr, n = R.feature_correspondences(a, b, mutual=False)
    assert n == 6 and corr[0, 1] == 2 and corr[2, 1] == 1 and corr[4, 1] == 0   # the tie goes to the lower index
    corr, n = R.feature_correspondences(a, b, mutual=True)
    assert [tuple(r) for r in corr[:n] if r[0] in (0, 2, 4)] == [(0, 2), (2, 1), (4, 0)] and (corr[n:] == -1).all()
    assert (np.diff(corr[:n, 0]) > 0).all()
