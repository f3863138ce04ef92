"""dsir_icp_refine (csrc/icp.hip and the skip / T_prev / T_cum / src_out branches of csrc/kabsch.hip that only ICP uses) at
ragged, edge and large shapes, against oracle/icp.py.  CPU tests (no mark) pin what the cases rely on; GPU tests carry the
``gpu`` mark.

Which test covers which branch
  test_gpu_icp_search_exact          icp_nn_kernel: the slice split ceil(K/4) with K % 4 != 0 and K < 4 (empty slices), the
                                     256-point tiles and their partial last tile, the 64-lane staging rows, q >= J lanes,
                                     ref_stride > 3, the `bd <= r2` admission; icp_apply_kernel with stride > 3;
                                     icp_stats_kernel count / sse; max_iter == 0 (no update, T_out = T_init)
  test_gpu_icp_ties_take_the_lower_index
                                     the strict `<` in the tile loop and in the four-slice merge
  test_gpu_icp_batch_is_bitwise_independent
                                     the frozen pair: `skip` early exits of icp_nn_kernel / kabsch_reg_kernel, the carry-over
                                     of T_prev into T_cum for both parities of the Ta / Tb ping-pong, `st[2] != 0` in
                                     icp_stats_kernel
  test_gpu_icp_batch_is_bitwise_independent_large
                                     the same carry-over in kabsch_reg_kernel<8> (J = 6000) and kabsch_kernel (J = 9000); the
                                     chunked path (kabsch_part / final / apply) is not reachable from ICP, which passes no
                                     partial-sum buffer
  test_gpu_icp_max_iter_cap          converged == 0, the iteration counter, the pose after exactly n - 1 updates
  test_gpu_icp_degenerate_correspondence_sets
                                     0 / 1 / 2 / 3 / collinear correspondences into kabsch_solve (rank 0, 1, 2 covariance)
  test_gpu_icp_non_finite_point_stays_in_its_pair
                                     NaN / inf coordinates: the pair takes identity updates (init returned bit for bit), its
                                     neighbours keep their bits
  test_gpu_icp_partial_overlap_5000  the whole loop at fitness ~ 0.65, ragged convergence inside one batch

Tolerance classes (every assertion is one of these)
  exact      counts, `fitness == count / J` in fp64, converged / iteration flags, every bitwise comparison
  existing   tests/test_icp.py: fitness 2e-3, rmse 1e-5, rotation 2e-5 rad, translation 2e-5 m; test_finetune.py's
             R^T R = I (here 1e-6 as the issue states) and det > 0.999
  derived    rmse of one search: 1e-12 relative (an fp64 sum of identical fp32 terms in another order: <= J * 2^-53);
             objective of an under-determined fit: 1e-10 x squared cloud extent; partial overlap: 4 x the oracle's own
             spread under +-1 ulp moves of the updated points where that exceeds the existing tolerance
             (test_oracle_partial_overlap_spread records the figures)

Measured on an MI355X (the tagged lines the tests print)
  SEARCH    all 16 shapes x 3 radii x 3 pairs: counts equal, worst rmse relative error 0.0e+00
  TIES      K=2399: pose error 0.0e+00 rad 0.0e+00 m, fitness 1.0
  FROZEN    iterations device == oracle == [1, 3, 25, 1] at max_iter 30 and 29; worst pose error 1.2e-07 rad 2.9e-07 m,
            worst rmse difference 7.7e-08, fitness equal; batch == single bit for bit at max_iter 30, 29, 2
  CAP       n=10: max_iter 9 -> converged 0, 9 iterations; 10 -> converged 1; 1 -> converged 0; worst pose error 3.7e-08 rad
            1.7e-07 m
  DEGEN     objective excess / extent^2: one 0.0e+00, two 8.3e-16, three 1.0e-14, collinear 1.8e-14; |R^T R - I| <= 4.6e-08;
            one / three: pose vs oracle <= 2.6e-08 rad 1.5e-07 m (two / collinear differ from the oracle's minimiser by 2.8 /
            1.0 rad, as they may)
  FROZENL   J=6000: device iterations [1, 8, 4, 1], J=9000: [1, 12, 4, 1], all converged; batch == single bit for bit at
            max_iter 30 and 29
  NONFINITE both pairs: T_out == T_init bit for bit, converged after 1 iteration, fitness 0.5214 / 0.4557, finite stats
  PARTIAL   pair 201: fitness diff 0.0e+00 rmse diff 7.1e-09 pose 1.1e-07 rad 1.8e-07 m, iterations 19 == 19
            pair 202: fitness diff 0.0e+00 rmse diff 1.2e-08 pose 4.2e-08 rad 3.0e-07 m, iterations 8 == 8
Every iteration count of this file equals the oracle's; no kernel fault was found.
"""
import numpy as np
import pytest

from deepsir_amd.synth import make_batch, make_pair
from oracle.icp import _nearest, icp, search_stats

POSE_TOL = 2e-5        # rad and m, tests/test_icp.py
FIT_TOL, RMSE_TOL = 2e-3, 1e-5

IDENT = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)


def _rot_err(Ra, Rb):
    D = np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)
    v = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(np.linalg.norm(v), 0.5 * (np.trace(D) - 1.0)))


def _pose_err(Ta, Tb):
    return _rot_err(Ta[:, :3], Tb[:, :3]), float(np.linalg.norm(np.asarray(Ta, np.float64)[:, 3] - np.asarray(Tb, np.float64)[:, 3]))


def _perturb_pose(T_gt, rng, ang_deg, shift):
    ax = rng.standard_normal(3); ax /= np.linalg.norm(ax)
    a = np.deg2rad(ang_deg)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    dR = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
    return np.hstack([dR @ T_gt[:, :3], (dR @ T_gt[:, 3] + rng.uniform(-shift, shift, 3))[:, None]]).astype(np.float32)


def _widen(xyz, stride, rng):
    """[n,3] -> [n,stride]: extra columns are large distractors (a kernel that read them as coordinates would be far off)"""
    extra = rng.uniform(1e5, 1e6, (len(xyz), stride - 3)) * rng.choice([-1.0, 1.0], (len(xyz), stride - 3))
    return np.ascontiguousarray(np.concatenate([xyz, extra], 1), np.float32)


def _engine(max_points, max_pairs):
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    return Engine(NetConfig(), 0, max_points=max(max_points, 1024), max_pairs=max_pairs)


def _run(eng, src, ref, T0, r, **kw):
    """numpy in, numpy out: src [P,J,s], ref [P,K,s], T0 [P,3,4]"""
    import torch
    T, st = eng.icp_refine(torch.from_numpy(np.ascontiguousarray(src)).cuda(), torch.from_numpy(np.ascontiguousarray(ref)).cuda(),
                           torch.from_numpy(np.ascontiguousarray(T0, np.float32)).cuda(), r, **kw)
    return T.cpu().numpy(), st.cpu().numpy()


# ------------------------------------------------------------------ 1. the search kernel in isolation
# (J, K, stride): every J and K the issue lists, ragged pairings, three strides
SEARCH_SHAPES = [(1, 1, 3), (1, 5, 4), (63, 2, 3), (64, 3, 7), (65, 4, 3), (63, 255, 4), (64, 256, 3), (65, 257, 7),
                 (1000, 1023, 3), (1000, 1024, 4), (1000, 1025, 3), (5000, 1029, 7), (1000, 5000, 3), (5000, 5000, 4),
                 (5000, 16387, 3), (1, 16387, 7)]
LATTICE = 16.0      # coordinates are integers / 16 in [0, 4): exact in fp32, squared distances exact multiples of 1/256


def _search_case(J, K, stride):
    """Three pairs of lattice clouds and three radii m / 16 (r^2 exact in fp32) with fitness near 0, near 0.5 and 1.  At the
    middle radius a source point of every pair is hand-placed at exactly r from a reference point, next to the lattice's own
    exact hits: `<=` against `<` changes the count."""
    rng = np.random.default_rng(1000 * J + K + stride)
    src = rng.integers(0, 64, (3, J, 3)).astype(np.float64) / LATTICE
    ref = rng.integers(0, 64, (3, K, 3)).astype(np.float64) / LATTICE
    d2 = np.concatenate([_nearest(src[k].astype(np.float32), ref[k].astype(np.float32))[1] for k in range(3)])
    m = max(1, int(round(LATTICE * float(np.sqrt(np.median(d2))))))
    for k in range(3):
        off = np.zeros(3); off[k] = m / LATTICE
        src[k, 0] = ref[k, K - 1] + off                      # at exactly r from the last reference point
    radii = (1.0 / 1024.0, m / LATTICE, 64.0)
    return (np.stack([_widen(s, stride, rng) for s in src]), np.stack([_widen(t, stride, rng) for t in ref]), radii)


def test_search_cases_pin_the_radius_and_span_the_fitness():
    """CPU: in every case some nearest neighbour sits at exactly r (so `<=` is pinned), and the three radii give a fitness
    near 0, in the middle and 1."""
    for J, K, stride in SEARCH_SHAPES:
        if J * K > 6_000_000:
            continue                                         # the two largest shapes: same construction, kept for the GPU test
        src, ref, radii = _search_case(J, K, stride)
        at_r, fit = 0, np.zeros(3)
        for k in range(3):
            nn = _nearest(src[k, :, :3], ref[k, :, :3])
            at_r += int((nn[1] == np.float32(radii[1]) ** 2).sum())
            fit += [search_stats(src[k, :, :3], ref[k, :, :3], r, nn)[0] / J / 3 for r in radii]
        assert at_r >= 1, (J, K, at_r)
        assert fit[0] <= 0.1 and fit[2] == 1.0, (J, K, fit)
        if J >= 63:
            assert 0.25 <= fit[1] <= 0.8, (J, K, fit)


@pytest.mark.gpu
@pytest.mark.parametrize("J,K,stride", SEARCH_SHAPES)
def test_gpu_icp_search_exact(J, K, stride):
    """max_iter = 0, identity init: the first search alone.  exact: count, flags, T_out bits.  derived: rmse 1e-12 relative.
    Prints one SEARCH line per shape."""
    src, ref, radii = _search_case(J, K, stride)
    eng = _engine(J, 3)
    T0 = np.stack([IDENT] * 3)
    worst = 0.0
    for r in radii:
        T, st = _run(eng, src, ref, T0, r, max_iter=0)
        for k in range(3):
            n, rmse = search_stats(src[k, :, :3], ref[k, :, :3], r)
            assert st[k, 0] == n / J and round(st[k, 0] * J) == n, (r, k, st[k], n)
            rel = abs(st[k, 1] - rmse) / rmse if rmse else abs(st[k, 1])
            worst = max(worst, rel)
            assert rel <= 1e-12, (r, k, st[k, 1], rmse)
            assert st[k, 2] == 0.0 and st[k, 3] == 0.0
        assert T.tobytes() == T0.tobytes()
    print(f"SEARCH J={J} K={K} stride={stride}: counts equal, worst rmse relative error {worst:.1e}")
    eng.close()


# ------------------------------------------------------------------ 2. ties and the slice merge
TIE_K = 2399            # slice = 600: tiles [0,256) [256,512) [512,600) per slice, the last slice one point short
TIE_KINDS = ("other slice", "far slice", "other tile", "other tile of slice 2", "other staging row", "same row", "triple")


def _tie_case():
    """96 queries on a coarse lattice (spacing 4), each with two reference points at exactly the same fp32 distance:
    q + (0.5, 0, 0) at the LOWER index, q - (0.5, 0, 0) at the higher one ('triple': a third at q + (0, 0.5, 0), higher still).
    Where the partners sit in the reference decides which comparison of the kernel breaks the tie.  Everything else in the
    reference is far away.  Returns src [1,J,3], ref [1,K,3], kind index per query."""
    J = 96
    g = np.stack(np.meshgrid(np.arange(6), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)[:J]
    src = 4.0 * g.astype(np.float64) + 1.0
    ref = np.stack([1000.0 + np.arange(TIE_K), np.full(TIE_K, -500.0), np.zeros(TIE_K)], 1)
    kind = np.arange(J) % len(TIE_KINDS)
    # i = j // 7 = 0..13 counts the queries of one kind, so every offset stays inside the tile / row its comment names
    slots = {
        0: lambda i: (10 + i, 600 + 300 + i),                # slice 0 / slice 1
        1: lambda i: (600 + 10 + i, 1800 + 590 - i),         # slice 1 / slice 3 (its short tail)
        2: lambda i: (130 + i, 256 + 100 + i),               # slice 0: tile 0 / tile 1
        3: lambda i: (1200 + 200 + i, 1200 + 512 + 40 + i),  # slice 2: tile 0 / tile 2 (the partial tile)
        4: lambda i: (1800 + 20 + i, 1800 + 64 + 30 + i),    # slice 3, tile 0: staging row 0 / row 1
        5: lambda i: (2 * i + 700, 2 * i + 701),             # neighbours in one row (slice 1, tile 0, row 1)
        6: lambda i: (300 + i, 1500 + i, 2250 + i),          # slices 0, 2, 3
    }
    where = lambda x: (x // 600, (x % 600) // 256, ((x % 600) % 256) // 64)       # (slice, tile, staging row) of an index
    want = {0: ((0, 0, 0), (1, 1, 0)), 1: ((1, 0, 0), (3, 2, 1)), 2: ((0, 0, 2), (0, 1, 1)), 3: ((2, 0, 3), (2, 2, 0)),
            4: ((3, 0, 0), (3, 0, 1)), 5: ((1, 0, 1), (1, 0, 1)), 6: ((0, 1, 0), (2, 1, 0), (3, 1, 3))}
    used = set()
    for j in range(J):
        idx = slots[int(kind[j])](j // len(TIE_KINDS))
        assert tuple(where(x) for x in idx) == want[int(kind[j])], (j, idx)
        assert all(a < b for a, b in zip(idx, idx[1:])) and not used.intersection(idx) and idx[-1] < TIE_K
        used.update(idx)
        for i, off in zip(idx, ((0.5, 0, 0), (-0.5, 0, 0), (0, 0.5, 0))):
            ref[i] = src[j] + np.array(off)
    return src.astype(np.float32)[None], ref.astype(np.float32)[None], kind


def test_tie_lattice_has_teeth():
    """CPU: every query has an exact fp32 tie, and breaking the ties of ANY one kind of placement to the higher index moves
    the oracle's single step by more than 100 x the pose tolerance."""
    src, ref, kind = _tie_case()
    s, t = src[0], ref[0]
    d = ((t[None, :, 0] - s[:, None, 0]) ** 2 + (t[None, :, 1] - s[:, None, 1]) ** 2) + (t[None, :, 2] - s[:, None, 2]) ** 2
    ties = (d == d.min(1, keepdims=True)).sum(1)
    assert (ties[kind != 6] == 2).all() and (ties[kind == 6] == 3).all()
    T_low = icp(s, t, IDENT, 1.0, max_iter=1)[0]
    np.testing.assert_allclose(T_low, np.hstack([np.eye(3), [[0.5], [0], [0]]]), atol=1e-12)
    for k in list(range(len(TIE_KINDS))) + [None]:
        T_high = icp(s, t, IDENT, 1.0, max_iter=1, tie_high=(kind == k) if k is not None else True)[0]
        er, et = _pose_err(T_high, T_low)
        assert max(er, et) > 100 * POSE_TOL, (k, er, et)


@pytest.mark.gpu
def test_gpu_icp_ties_take_the_lower_index():
    """One update from the identity on the tie lattice.  existing: pose 2e-5 / 2e-5.  exact: fitness 1, one iteration.
    Prints the TIES line."""
    src, ref, _ = _tie_case()
    eng = _engine(96, 1)
    T, st = _run(eng, src, ref, IDENT[None], 1.0, max_iter=1)
    To, fitness, rmse, converged, iters = icp(src[0], ref[0], IDENT, 1.0, max_iter=1)
    er, et = _pose_err(T[0], To)
    print(f"TIES K={TIE_K}: pose error {er:.1e} rad {et:.1e} m, fitness {st[0, 0]}, rmse {st[0, 1]:.3e} (oracle {rmse:.3e})")
    assert er < POSE_TOL and et < POSE_TOL
    assert st[0, 0] == fitness == 1.0 and abs(st[0, 1] - rmse) < RMSE_TOL and st[0, 3] == 1.0 and st[0, 2] == float(converged)
    eng.close()


# ------------------------------------------------------------------ 3. frozen pairs, the cap, degenerate sets
def _ragged_pair(seed, ang_deg, shift, noise, J=1500, K=1800, stride=4, away=0.0):
    p = make_pair(K, seed, stride)
    rng = np.random.default_rng(seed)
    src, ref = p["points_src"][0][:J].copy(), p["points_ref"][0].copy()
    if noise:
        ref[:, :3] += rng.normal(0, noise, (K, 3)).astype(np.float32)
    ref[:, :3] += np.float32(away)
    T_gt = p["transform_gt"][0].astype(np.float64)
    T0 = _perturb_pose(T_gt, rng, ang_deg, shift) if ang_deg else T_gt.astype(np.float32)
    return src, ref, T0


def _frozen_batch():
    """at the optimum / small perturbation / large perturbation with noise / nothing in reach"""
    return [_ragged_pair(103, 0, 0, 0), _ragged_pair(103, 1, 0.02, 0), _ragged_pair(103, 12, 0.15, 0.006),
            _ragged_pair(104, 1, 0.02, 0, away=100.0)]


CAP_PAIR = dict(seed=103, ang_deg=8, shift=0.1, noise=0.004)


def test_frozen_batch_iteration_counts_span_1_to_10():
    """CPU: the batch of test_gpu_icp_batch_is_bitwise_independent freezes its pairs many iterations apart."""
    its = [icp(s, r, t0, 0.1)[4] for s, r, t0 in _frozen_batch()]
    assert min(its) == 1 and max(its) >= 10 and len(set(its)) >= 3, its
    assert its[3] == 1 and icp(*_frozen_batch()[3], 0.1)[1] == 0.0


def test_cap_pair_converges_with_margin():
    """CPU: the pair of test_gpu_icp_max_iter_cap stops at iteration n >= 5 for a reason that does not hang on the last bit:
    the rmse change of iteration n - 1 is above 1e-5 and that of iteration n below 1e-7 (the criterion is 1e-6)."""
    s, r, t0 = _ragged_pair(**CAP_PAIR)
    tr = []
    n = icp(s, r, t0, 0.1, trace=tr)[4]
    assert n >= 5 and len(tr) == n + 1
    assert abs(tr[n - 1][1] - tr[n - 2][1]) > 1e-5 and abs(tr[n][1] - tr[n - 1][1]) < 1e-7 and tr[n][0] == tr[n - 1][0]


@pytest.mark.gpu
def test_gpu_icp_batch_is_bitwise_independent():
    """exact: T_out[k] and stats[k] of the batch == the single-pair call, for max_iter 30 and 29 (both parities of the
    ping-pong at the final copy); iteration counts == the oracle's.  existing: pose / fitness / rmse against the oracle.
    Oracle iteration counts of the batch: [1, 3, 25, 1].  Prints FROZEN lines."""
    cases = _frozen_batch()
    eng = _engine(1500, 4)
    src, ref, T0 = (np.stack([c[i] for c in cases]) for i in range(3))
    for max_iter in (30, 29, 2):
        Tb, sb = _run(eng, src, ref, T0, 0.1, max_iter=max_iter)
        for k in range(4):
            T1, s1 = _run(eng, src[k:k + 1], ref[k:k + 1], T0[k:k + 1], 0.1, max_iter=max_iter)
            assert T1[0].tobytes() == Tb[k].tobytes() and s1[0].tobytes() == sb[k].tobytes(), (max_iter, k, T1[0], Tb[k], s1, sb[k])
        if max_iter == 2:
            continue
        for k, (s, r, t0) in enumerate(cases):
            To, fitness, rmse, converged, iters = icp(s, r, t0, 0.1, max_iter=max_iter)
            er, et = _pose_err(Tb[k], To)
            print(f"FROZEN max_iter={max_iter} pair {k}: iterations device {int(sb[k, 3])} oracle {iters}, pose error {er:.1e} rad "
                  f"{et:.1e} m, fitness {sb[k, 0]:.4f}/{fitness:.4f}, rmse diff {abs(sb[k, 1] - rmse):.1e}")
            assert sb[k, 3] == iters and sb[k, 2] == float(converged)
            assert er < POSE_TOL and et < POSE_TOL and abs(sb[k, 0] - fitness) < FIT_TOL and abs(sb[k, 1] - rmse) < RMSE_TOL
    assert Tb[3].tobytes() == T0[3].tobytes() and sb[3, 0] == 0.0 and sb[3, 1] == 0.0     # nothing in reach: the init, bit for bit
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("J,K", [(6000, 6100), (9000, 9300)])
def test_gpu_icp_batch_is_bitwise_independent_large(J, K):
    """The same frozen-pair carry-over in the other Kabsch kernels ICP reaches: kabsch_reg_kernel<8> (5120 < J <= 8192) and the
    streaming kabsch_kernel (J > 8192, the 16384- and 65536-point pose_opt use).  exact: batch == single bit for bit at
    max_iter 30 and 29; the pairs freeze at different iterations (asserted on the device's own counts); no oracle.
    Prints FROZENL lines."""
    cases = [_ragged_pair(120, 0, 0, 0, J=J, K=K, stride=3), _ragged_pair(121, 3, 0.05, 0.002, J=J, K=K, stride=3),
             _ragged_pair(122, 1, 0.02, 0, J=J, K=K, stride=3), _ragged_pair(123, 1, 0.02, 0, J=J, K=K, stride=3, away=100.0)]
    eng = _engine(J, 4)
    src, ref, T0 = (np.stack([c[i] for c in cases]) for i in range(3))
    for max_iter in (30, 29):
        Tb, sb = _run(eng, src, ref, T0, 0.1, max_iter=max_iter)
        for k in range(4):
            T1, s1 = _run(eng, src[k:k + 1], ref[k:k + 1], T0[k:k + 1], 0.1, max_iter=max_iter)
            assert T1[0].tobytes() == Tb[k].tobytes() and s1[0].tobytes() == sb[k].tobytes(), (max_iter, k, T1[0], Tb[k], s1, sb[k])
        print(f"FROZENL J={J} max_iter={max_iter}: device iterations {sb[:, 3].astype(int).tolist()} converged {sb[:, 2].astype(int).tolist()}")
        assert sb[0, 3] == 1.0 and sb[3, 3] == 1.0 and sb[1, 3] >= sb[2, 3] + 2 and sb[2, 3] >= 2 and (sb[:, 2] == 1.0).all()
    assert Tb[3].tobytes() == T0[3].tobytes()
    eng.close()


@pytest.mark.gpu
def test_gpu_icp_max_iter_cap():
    """exact: converged / iterations at max_iter = n - 1, n, 1.  existing: the pose after exactly that many updates.
    The oracle's n is 10.  Prints CAP lines."""
    s, r, t0 = _ragged_pair(**CAP_PAIR)
    n = icp(s, r, t0, 0.1)[4]
    eng = _engine(1500, 1)
    for max_iter, conv in ((n - 1, 0.0), (n, 1.0), (1, 0.0)):
        T, st = _run(eng, s[None], r[None], t0[None], 0.1, max_iter=max_iter)
        To, fitness, rmse, converged, iters = icp(s, r, t0, 0.1, max_iter=max_iter)
        er, et = _pose_err(T[0], To)
        print(f"CAP n={n} max_iter={max_iter}: device converged {st[0, 2]} iterations {st[0, 3]}, pose error {er:.1e} rad {et:.1e} m")
        assert converged == bool(conv) and iters == max_iter
        assert st[0, 2] == conv and st[0, 3] == max_iter
        assert er < POSE_TOL and et < POSE_TOL and abs(st[0, 0] - fitness) < FIT_TOL and abs(st[0, 1] - rmse) < RMSE_TOL
    eng.close()


DEGEN = ("none", "one", "two", "three", "collinear")
DEGEN_R = 0.01


def _degenerate_batch():
    """Five pairs, J = 6, K = 9, radius 0.01: the first c source points have a reference point within reach (a small rigid
    motion of them, rounded to fp32), everything else is metres away."""
    rng = np.random.default_rng(5)
    a = 1e-3
    dR = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    dt = np.array([0.003, -0.002, 0.001])
    src, ref, cnt = [], [], []
    for name in DEGEN:
        s = np.array([[1.0, 2.0, 0.5], [1.75, 1.5, 1.0], [0.5, 1.0, 2.0], [2.5, 0.25, 1.5], [0.25, 2.75, 2.5], [2.0, 2.5, 0.25]])
        if name == "collinear":
            s[:4] = s[0] + np.outer([0.0, 0.5, 1.25, 2.0], [0.6, -0.48, 0.64])
        c = {"none": 0, "one": 1, "two": 2, "three": 3, "collinear": 4}[name]
        t = np.stack([20.0 + np.arange(9.0), np.full(9, -7.0), np.full(9, 3.0)], 1)
        order = rng.permutation(9)[:c]
        t[order] = s[:c] @ dR.T + dt
        src.append(s); ref.append(t); cnt.append(c)
    return np.stack(src).astype(np.float32), np.stack(ref).astype(np.float32), cnt


def _objective(T, s, t):
    return float((((s.astype(np.float64) @ np.asarray(T, np.float64)[:, :3].T + np.asarray(T, np.float64)[:, 3]) - t) ** 2).sum())


def test_degenerate_batch_has_the_intended_counts():
    src, ref, cnt = _degenerate_batch()
    for k, c in enumerate(cnt):
        assert search_stats(src[k], ref[k], DEGEN_R)[0] == c
        if DEGEN[k] == "collinear":
            assert np.linalg.matrix_rank(src[k, :4].astype(np.float64) - src[k, 0], tol=1e-6) == 1


@pytest.mark.gpu
def test_gpu_icp_degenerate_correspondence_sets():
    """exact: counts, the init returned bit for bit when nothing corresponds.  existing: pose for 1 and 3 correspondences,
    R^T R = I to 1e-6, det > 0.999.  derived: where the minimiser is not unique (2, collinear) the OBJECTIVE after one step is
    within 1e-10 x squared extent of the oracle's optimum.
    Prints DEGEN lines."""
    src, ref, cnt = _degenerate_batch()
    eng = _engine(6, 5)
    T0 = np.stack([IDENT] * 5)
    for max_iter in (1, 30):
        T, st = _run(eng, src, ref, T0, DEGEN_R, max_iter=max_iter)
        assert np.isfinite(T).all() and np.isfinite(st).all()
        for k, c in enumerate(cnt):
            R = T[k][:, :3].astype(np.float64)
            orth = float(np.abs(R.T @ R - np.eye(3)).max())
            assert orth < 1e-6 and np.linalg.det(R) > 0.999, (DEGEN[k], R)
            if c == 0:
                assert T[k].tobytes() == T0[k].tobytes() and st[k, 0] == 0.0 and st[k, 1] == 0.0
                continue
            if max_iter != 1:
                continue
            nn = _nearest(src[k], ref[k])
            ok = nn[1] <= np.float32(DEGEN_R) ** 2
            s_in, t_in = src[k][ok], ref[k][nn[0][ok]]
            To = icp(src[k], ref[k], IDENT, DEGEN_R, max_iter=1)[0]
            ext2 = float(np.ptp(np.concatenate([src[k], ref[k][nn[0][ok]]]), axis=0).max()) ** 2
            excess = (_objective(T[k], s_in, t_in) - _objective(To, s_in, t_in)) / ext2
            er, et = _pose_err(T[k], To)
            print(f"DEGEN {DEGEN[k]} ({c} correspondences): objective excess {excess:.1e} x extent^2, pose vs oracle {er:.1e} rad "
                  f"{et:.1e} m, |R^T R - I| {orth:.1e}, fitness {st[k, 0]:.4f}")
            assert excess <= 1e-10
            if DEGEN[k] == "one":
                assert et < POSE_TOL and er < POSE_TOL            # a pure translation
            if DEGEN[k] == "three":
                assert et < POSE_TOL and er < POSE_TOL
    eng.close()


@pytest.mark.gpu
def test_gpu_icp_non_finite_point_stays_in_its_pair():
    """A NaN source coordinate in pair 0, an inf reference coordinate (at index 0, where unmatched points gather) in pair 2.
    exact: pairs 1 and 3 keep their single-pair bits.  Pairs 0 and 2: as include/dsir.h documents, every update is the
    identity: T_out == T_init bit for bit, converged after one iteration, finite stats."""
    cases = [_ragged_pair(110 + k, 2, 0.03, 0.002, J=700, K=900, stride=3) for k in range(4)]
    src, ref, T0 = (np.stack([c[i] for c in cases]) for i in range(3))
    src[0, 5, 1] = np.nan
    ref[2, 0, 2] = np.inf
    src[2, 11, :3] = 50.0                                    # an unmatched source point, so the clamped index 0 is gathered
    eng = _engine(700, 4)
    Tb, sb = _run(eng, src, ref, T0, 0.1)
    for k in (1, 3):
        T1, s1 = _run(eng, src[k:k + 1], ref[k:k + 1], T0[k:k + 1], 0.1)
        assert T1[0].tobytes() == Tb[k].tobytes() and s1[0].tobytes() == sb[k].tobytes()
        To, fitness, rmse, converged, iters = icp(*cases[k], 0.1)
        er, et = _pose_err(Tb[k], To)
        assert er < POSE_TOL and et < POSE_TOL and sb[k, 3] == iters
    for k in (0, 2):
        print(f"NONFINITE pair {k}: stats {sb[k].tolist()}, moved from the init by {np.abs(Tb[k] - T0[k]).max():.1e}")
        # the documented outcome: identity updates, so the init comes back bit for bit, 'converged' after one iteration
        assert Tb[k].tobytes() == T0[k].tobytes() and sb[k, 2] == 1.0 and sb[k, 3] == 1.0
        assert np.isfinite(sb[k]).all() and 0.0 < sb[k, 0] < 1.0
    eng.close()


# ------------------------------------------------------------------ partial overlap at 5000 points
PARTIAL_SEEDS = (201, 202)
ULP_SEEDS = (1, 2, 3, 4)
# bounds = max(existing tolerance, 4 x the oracle's spread under +-1 ulp moves), per pair: fitness, rmse, rot, trans, iterations
# spreads measured by test_oracle_partial_overlap_spread (its docstring has the figures)
PARTIAL_BOUND = {201: (2e-3, 1e-5, 2e-5, 2e-5, 0), 202: (2e-3, 1e-5, 2e-5, 2e-5, 0)}


def _partial_case(k):
    b = make_batch(5000, PARTIAL_SEEDS, 3, partial_overlap=True)
    T0 = _perturb_pose(b["transform_gt"][k].astype(np.float64), np.random.default_rng(k), 3.0, 0.05)
    return b["points_src"][k], b["points_ref"][k], T0


@pytest.mark.parametrize("k", range(len(PARTIAL_SEEDS)))
def test_oracle_partial_overlap_spread(k):
    """CPU: the oracle's own spread at 5000 partially overlapping points when every updated point moves by -1 / 0 / +1 fp32
    ulp (4 seeds): worst |fitness|, |rmse|, rotation, translation and iteration difference from the unperturbed run.
    Measured  pair 201: fitness 0.0e+00 rmse 1.0e-08 rot 1.3e-08 trans 3.9e-08 iterations 0 (oracle: 19 iterations)
              pair 202: fitness 0.0e+00 rmse 3.5e-09 rot 1.5e-08 trans 2.6e-08 iterations 0 (oracle: 8 iterations)
    4 x these is below the existing tolerances throughout, so PARTIAL_BOUND keeps the existing ones and an exact count."""
    s, r, t0 = _partial_case(k)
    To, f, e, c, it = icp(s, r, t0, 0.1)
    assert c and 0.3 < f < 0.9
    sp = np.zeros(5)
    for seed in ULP_SEEDS:
        Tp, fp, ep, cp, itp = icp(s, r, t0, 0.1, perturb_ulps=seed)
        sp = np.maximum(sp, [abs(fp - f), abs(ep - e), *_pose_err(Tp, To), abs(itp - it)])
    print(f"SPREAD pair {PARTIAL_SEEDS[k]}: fitness {sp[0]:.1e} rmse {sp[1]:.1e} rot {sp[2]:.1e} trans {sp[3]:.1e} iterations {int(sp[4])}"
          f" (oracle: fitness {f:.4f}, {it} iterations)")
    existing = (FIT_TOL, RMSE_TOL, POSE_TOL, POSE_TOL, 0)
    bound = PARTIAL_BOUND[PARTIAL_SEEDS[k]]
    for i in range(5):
        assert bound[i] == max(existing[i], bound[i]) and 4 * sp[i] <= bound[i], (i, sp, bound)


@pytest.mark.gpu
def test_gpu_icp_partial_overlap_5000():
    """The whole loop at 5000 partially overlapping points, two pairs that stop 11 iterations apart, against the full oracle
    loop.  existing tolerances (PARTIAL_BOUND: the oracle's 4 x ulp spread is below them), iterations exact.
    Prints PARTIAL lines."""
    cases = [_partial_case(k) for k in range(len(PARTIAL_SEEDS))]
    src, ref, T0 = (np.stack([c[i] for c in cases]) for i in range(3))
    eng = _engine(5000, len(cases))
    T, st = _run(eng, src, ref, T0, 0.1)
    bad = []
    for k, (s, r, t0) in enumerate(cases):
        To, fitness, rmse, converged, iters = icp(s, r, t0, 0.1)
        er, et = _pose_err(T[k], To)
        b = PARTIAL_BOUND[PARTIAL_SEEDS[k]]
        err = (abs(st[k, 0] - fitness), abs(st[k, 1] - rmse), er, et, abs(st[k, 3] - iters))
        print(f"PARTIAL pair {PARTIAL_SEEDS[k]}: fitness diff {err[0]:.1e} rmse diff {err[1]:.1e} pose {er:.1e} rad {et:.1e} m, "
              f"iterations device {int(st[k, 3])} oracle {iters}, fitness {fitness:.4f}")
        if not (all(e <= bb for e, bb in zip(err, b)) and st[k, 2] == float(converged)):
            bad.append((k, err, b))
    assert not bad, bad
    eng.close()
