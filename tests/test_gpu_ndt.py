"""dsir_ndt_refine / dsir_ndt_map (csrc/ndt.hip) against the host restatement deepsir_amd/ndt.py.  Every test carries the ``gpu`` mark.

Tolerances
  exact      lattice, sorted keys, index, which positions hold a record, n; `converged`, the identity-update count, the matched
             fraction given the device's own final pose, every bitwise comparison
  bound      a cell's mean: the fp64 summation bound (2n + 2) 2^-53 max |x|.  The six sums of C are not part of a record (mu, B, n),
             so they are held through B alone
  measured   B: 4 x B_SENSITIVITY of tests/test_ndt_host.py (the restatement's change of B when C moves by its summation bound);
             pose and mean likelihood: 4 x the host rule's largest deviation under +-1 ulp moves (POSE_TOL, LIKELIHOOD_TOL there)
  iterations equal to the host's.  The capped runs (6 iterations) are clear of their thresholds by a factor 10 at every iteration
             (asserted), so equality is owed.  A run to convergence cannot have that margin - the step shrinks by about 0.45 per
             iteration - and the host rule's own count did not move under the +-1 ulp draws (0 in 96 runs), so equality is asserted
             there too; both counts are printed.

Measured on an MI355X (the tagged lines the tests print)
  NDT MAP    up to 250 valid cells a pair: every exact comparison held, the means bit for bit, B within 8.4e-15 of the host's
             (allowed 1.2e-12)
  NDT        48 pairs x 2 runs: iterations device == host everywhere (6 capped; 11 .. 22 to convergence), worst pose difference
             3.6e-07 rad 7.0e-07 (allowed 6.8e-06), worst mean-likelihood difference 1.5e-07 (allowed 3.0e-06), matched fraction equal
  OUTSIDE    matched 0.5333 / 0.3000 (neighbors 7 / 1) on both sides, likelihood equal
Every bitwise comparison (two runs, batch of 3 against single pairs, stride 3 against 6, ragged against dense, harness) held.
"""
import numpy as np
import pytest

from deepsir_amd.ndt import KEY_NONE, matched_fraction_host, ndt_map_host, ndt_refine_host
from ndt_cases import CAP_ITERS, NEIGHBORS, REFINE_CASES, RES, STEP_TOL, clear_of_thresholds, host_refine, map_cloud
from test_icp_plane import pose_err, surface_case
from test_ndt_host import B_SENSITIVITY, LIKELIHOOD_TOL, MAP_RES, MAP_SHAPES, POSE_TOL

pytestmark = pytest.mark.gpu


def _engine(max_points, max_pairs):
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    return Engine(NetConfig(), 0, max_points=max(max_points, 1024), max_pairs=max_pairs)


def _dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _run(eng, src, ref, T0, res=RES, **kw):
    T, st = eng.ndt_refine(_dev(src), _dev(ref), _dev(T0), res, **kw)
    return T.cpu().numpy(), st.cpu().numpy()


def _batch(J, K, noise, seeds):
    cases = [surface_case(J, K, s, noise) for s in seeds]
    return tuple(np.stack([c[k] for c in cases]) for k in ("src", "ref", "T0"))


def _pad6(a):
    """rows of 6 columns: xyz and three columns the engine must not read"""
    return np.concatenate([a, np.full(a.shape[:-1] + (3,), np.nan, np.float32)], -1)


# ------------------------------------------------------------------ 1. the map
@pytest.mark.parametrize("stride", [3, 6])
@pytest.mark.parametrize("K", MAP_SHAPES)
def test_gpu_map_matches_host(K, stride):
    refs = np.stack([map_cloud(K, 10 * K + s, MAP_RES) for s in (1, 2, 3)])
    counts = np.array([K, 0, max(K - 3, 0)], np.int32)                   # one pair ragged to Kp = 0, one short of the capacity
    refs[1] = np.nan
    refs[2, counts[2]:] = np.nan
    eng = _engine(K, 3)
    lat, keys, index, rec = (t.cpu().numpy() for t in eng.ndt_map(_dev(_pad6(refs) if stride == 6 else refs), MAP_RES, counts_ref=counts))
    eng.close()
    worst_mu, worst_B, cells = 0.0, 0.0, 0
    for p in range(3):
        Kp = int(counts[p])
        m = ndt_map_host(refs[p, :Kp], MAP_RES)
        assert np.array_equal(lat[p], np.r_[m["origin"], m["h"]])
        assert np.array_equal(keys[p, :Kp].view(np.uint64), m["keys"]) and np.array_equal(index[p, :Kp], m["index"])
        assert (keys[p, Kp:].view(np.uint64) == KEY_NONE).all() and np.array_equal(index[p, Kp:], np.arange(Kp, K))
        held = rec[p, :, 9] != 0
        assert np.array_equal(held[:Kp], m["records"][:, 9] != 0) and not held[Kp:].any() and not rec[p][~held].any()
        assert np.array_equal(rec[p, :Kp, 9], m["records"][:, 9])
        for q in np.flatnonzero(held):
            n = int(rec[p, q, 9])
            x = refs[p, m["index"][q:q + n]].astype(np.float64)
            bound = (2 * n + 2) * 2.0 ** -53 * float(np.abs(x).max())
            dmu = float(np.abs(rec[p, q, :3] - m["records"][q, :3]).max())
            dB = float(np.abs(rec[p, q, 3:9] - m["records"][q, 3:9]).max() / np.abs(m["records"][q, 3:9]).max())
            worst_mu, worst_B, cells = max(worst_mu, dmu / bound), max(worst_B, dB), cells + 1
            assert dmu <= bound, (p, q, dmu, bound)
            assert dB <= 4 * B_SENSITIVITY, (p, q, dB)
    print(f"NDT MAP K={K} stride={stride}: {cells} valid cells, mean within {worst_mu:.2f} of its bound, B within {worst_B:.1e} (allowed {4 * B_SENSITIVITY:.1e})")
    assert cells > 0 or K < 6 or K == 6


# ------------------------------------------------------------------ 2. refine against the host rule
def _check(tag, c, T, st, host, nb, exact_iters_owed):
    To, so, trace = host
    er, et = pose_err(T, To)
    mf = matched_fraction_host(c["src"], c["ref"], T, RES, nb)
    print(f"{tag}: iterations device {int(st[3])} host {int(so[3])}, pose {er:.2e} rad {et:.2e} (allowed {POSE_TOL:.1e}), likelihood diff "
          f"{abs(float(st[0]) - float(so[0])):.1e} (allowed {LIKELIHOOD_TOL:.1e}), matched {st[1]:.4f} host at the device's pose {mf:.4f}, "
          f"identity updates {int(st[4])}/{int(so[4])}")
    if exact_iters_owed:
        assert clear_of_thresholds(trace, 10.0), trace
    assert st[2] == so[2] and st[4] == so[4]
    assert st[3] == so[3]
    assert st[1] == np.float32(mf)
    assert er < POSE_TOL and et < POSE_TOL, (er, et, POSE_TOL)
    assert abs(float(st[0]) - float(so[0])) < LIKELIHOOD_TOL


@pytest.mark.parametrize("neighbors", NEIGHBORS)
@pytest.mark.parametrize("J,K,noise,seeds", REFINE_CASES)
def test_gpu_refine_matches_host_rule(J, K, noise, seeds, neighbors):
    src, ref, T0 = _batch(J, K, noise, seeds)
    eng = _engine(max(J, K), 3)
    for max_iter in (CAP_ITERS, 30):
        T, st = _run(eng, src, ref, T0, neighbors=neighbors, max_iter=max_iter, step_tol=STEP_TOL)
        assert st.shape == (3, 5) and np.isfinite(T).all() and np.isfinite(st).all()
        for k, seed in enumerate(seeds):
            _check(f"NDT J={J} K={K} nb={neighbors} max_iter={max_iter} seed={seed}", surface_case(J, K, seed, noise), T[k], st[k],
                   host_refine(J, K, seed, noise, neighbors, max_iter), neighbors, max_iter == CAP_ITERS)
    eng.close()


# ------------------------------------------------------------------ 3. edges
def test_gpu_refine_edges():
    J = K = 300
    seeds = (4, 14, 24)
    src, ref, T0 = _batch(J, K, 0.0, seeds)
    eng = _engine(1024, 3)
    T_ok, st_ok = _run(eng, src, ref, T0)
    # max_iter = 0: T_init back bit for bit, nothing converged, statistics of the first pose
    T, st = _run(eng, src, ref, T0, max_iter=0)
    assert np.array_equal(T, T0) and not st[:, 2:].any() and (st[:, 0] > 0).all()
    # a non-finite source row: identity update, T_init back bit for bit, the bystanders untouched
    s2 = src.copy(); s2[1, 7, 1] = np.nan
    T, st = _run(eng, s2, ref, T0)
    assert np.array_equal(T[1], T0[1]) and list(st[1, 2:]) == [1, 1, 1]
    assert np.array_equal(T[[0, 2]], T_ok[[0, 2]]) and np.array_equal(st[[0, 2]], st_ok[[0, 2]])
    # a non-finite reference row is ignored: the same bytes as without it
    r2 = ref.copy(); r2[0, 3] = np.nan
    T, st = _run(eng, src, r2, T0)
    Th, sh, _ = ndt_refine_host(src[0], r2[0], T0[0], RES)
    assert st[0, 3] == sh[3] and pose_err(T[0], Th)[0] < POSE_TOL and pose_err(T[0], Th)[1] < POSE_TOL
    Td, sd = _run(eng, src[:1], np.delete(ref[:1], 3, 1), T0[:1])
    assert np.array_equal(T[0], Td[0]) and np.array_equal(st[0], sd[0])
    # a reference with no valid cell (5 points), and Jp = 0: identity, converged after one iteration
    T, st = _run(eng, src, ref, T0, counts_ref=[K, 5, K], counts_src=[J, J, 0])
    for p in (1, 2):
        assert np.array_equal(T[p], T0[p]) and list(st[p]) == [0, 0, 1, 1, 1]
    assert np.array_equal(T[0], T_ok[0]) and np.array_equal(st[0], st_ok[0])
    # source rows outside the lattice on each side: no own cell, the in-range face neighbours still visited - as the host counts
    c = surface_case(J, K, 4)
    m = ndt_map_host(c["ref"], RES)
    lo, h = m["origin"], m["h"]
    hi = c["ref"].astype(np.float64).max(0)
    cur = (c["src"].astype(np.float64) @ c["T_gt"][:, :3].T + c["T_gt"][:, 3]).astype(np.float32)
    out = cur.copy()
    for a in range(3):
        out[10 + a, a] = np.float32(lo[a] - 0.3 * h)                     # cell -1 on axis a
        out[20 + a, a] = np.float32(hi[a] + 1.2 * h)                     # beyond the last cell
        out[30 + a, a] = np.float32(-1e30 if a % 2 else 1e30)            # clamped by cell_of
    eye = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)
    for nb in NEIGHBORS:
        T, st = _run(eng, out[None], c["ref"][None], eye[None], neighbors=nb, max_iter=0)
        Th, sh, _ = ndt_refine_host(out, c["ref"], eye, RES, neighbors=nb, max_iter=0, m=m)
        print(f"NDT OUTSIDE nb={nb}: matched device {st[0, 1]:.4f} host {sh[1]:.4f}, likelihood diff {abs(float(st[0, 0]) - float(sh[0])):.1e}")
        assert st[0, 1] == sh[1] and abs(float(st[0, 0]) - float(sh[0])) < LIKELIHOOD_TOL
    eng.close()


# ------------------------------------------------------------------ 4. bitwise
def test_gpu_refine_bitwise_runs_batch_stride():
    J, K, noise, seeds = REFINE_CASES[2]
    src, ref, T0 = _batch(J, K, noise, seeds)
    eng = _engine(2048, 4)
    a = _run(eng, src, ref, T0)
    b = _run(eng, src, ref, T0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])                       # two runs
    for p in range(3):                                                                     # a batch of 3 against the pairs alone
        T, st = _run(eng, src[p:p + 1], ref[p:p + 1], T0[p:p + 1])
        assert np.array_equal(T[0], a[0][p]) and np.array_equal(st[0], a[1][p])
    T, st = _run(eng, _pad6(src), _pad6(ref), T0)                                          # stride 6 against 3
    assert np.array_equal(T, a[0]) and np.array_equal(st, a[1])
    eng.close()


def test_gpu_refine_ragged_equals_dense():
    cap = 2048
    counts = [(37, 300), (300, 300), (1025, 1024), (2000, 2048)]
    cases = [surface_case(2048, 2048, 40 + i) for i in range(4)]
    src = np.full((4, cap, 3), np.nan, np.float32)
    ref = np.full((4, cap, 3), np.nan, np.float32)
    for i, ((j, k), c) in enumerate(zip(counts, cases)):
        src[i, :j], ref[i, :k] = c["src"][:j], c["ref"][:k]
    src[0, 40:60], ref[1, 400:500] = cases[0]["src"][40:60], cases[1]["ref"][400:500]      # finite padding that would match well
    T0 = np.stack([c["T0"] for c in cases])
    eng = _engine(cap, 4)
    for nb in NEIGHBORS:
        T, st = _run(eng, src, ref, T0, neighbors=nb, counts_src=[c[0] for c in counts], counts_ref=[c[1] for c in counts])
        for i, (j, k) in enumerate(counts):
            Td, sd = _run(eng, src[i:i + 1, :j], ref[i:i + 1, :k], T0[i:i + 1], neighbors=nb)
            assert np.array_equal(T[i], Td[0]) and np.array_equal(st[i], sd[0]), (nb, i)
        assert (st[:, 3] >= 1).all()
    eng.close()


# ------------------------------------------------------------------ 5. harness
def test_gpu_ndt_multiscale_equals_chained_calls():
    import torch
    from deepsir_amd import harness
    cases = [surface_case(1357, 1024, 9), surface_case(300, 300, 4)]
    eng = _engine(2048, 2)
    T0 = np.stack([c["T0"] for c in cases])
    T, stats = harness.ndt_multiscale([c["src"] for c in cases], [c["ref"] for c in cases], T0, [0.4, RES], [10, 30], engine=eng)
    src, ns = harness.pad_clouds([_dev(c["src"]) for c in cases])
    ref, nr = harness.pad_clouds([_dev(c["ref"]) for c in cases])
    Ta, sa = eng.ndt_refine(src, ref, _dev(T0), 0.4, max_iter=10, counts_src=ns, counts_ref=nr)
    Tb, sb = eng.ndt_refine(src, ref, Ta, RES, max_iter=30, counts_src=ns, counts_ref=nr)
    assert torch.equal(T, Tb) and torch.equal(stats[0], sa) and torch.equal(stats[1], sb) and len(stats) == 2
    eng.close()


def test_gpu_inference_align_ndt_equals_call_by_hand():
    """inference_align(pose_opt='ndt') on two 2048-point surface pairs (the pairs of tests/test_gpu_icp_plane.py's harness test): the
    appended pose is Engine.ndt_refine's, called by hand from the network's last pose, bit for bit; the earlier entries are the
    plain run's."""
    import argparse
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.harness import inference_align
    from deepsir_amd.model import Network
    from deepsir_amd.weights import generate_state_dict, to_torch_state_dict
    args = argparse.Namespace(pipeline="align", num_sub=-1, num_knn=16, out_feat_dim=64, clip_weight_thresh=0.0, feat_len=3,
                              d_out=[16, 64, 128, 256], num_points=2048, sub_sampling_ratio=[4, 4, 4, 4], use_ppf=False)
    net = Network(args)
    net.load_state_dict(to_torch_state_dict(generate_state_dict(NetConfig(), 0)))
    net = net.cuda().eval()
    cases = [surface_case(2048, 2048, s) for s in (41, 42)]
    pairs = [dict(points_src=c["src"][None], points_ref=c["ref"][None], transform_gt=c["T_gt"][None].astype(np.float32)) for c in cases]
    plain, _ = inference_align(pairs, net, 3, batch=2)
    ndt, _ = inference_align(pairs, net, 3, batch=2, pose_opt="ndt", voxel_size=0.05)          # default resolution 4 x voxel = 0.2
    ndt2, _ = inference_align(pairs, net, 3, batch=2, pose_opt="ndt", ndt_resolution=0.4)
    assert plain.shape == ndt.shape == (2, 4, 3, 4) and np.isfinite(ndt).all()
    assert plain[:, :3].tobytes() == ndt[:, :3].tobytes() == ndt2[:, :3].tobytes()
    with pytest.raises(ValueError, match="'ndt'"):
        inference_align(pairs, net, 3, batch=2, pose_opt="nope")
    eng = net._ensure_engine(2048, 2)
    src, ref = _dev(np.stack([c["src"] for c in cases])), _dev(np.stack([c["ref"] for c in cases]))
    for res, got in ((4 * 0.05, ndt), (0.4, ndt2)):
        T, st = eng.ndt_refine(src, ref, _dev(plain[:, 2]), res)
        assert np.array_equal(got[:, 3], T.cpu().numpy()) and (st[:, 3] >= 1).all()


# ------------------------------------------------------------------ 6. arguments
def test_gpu_bad_arguments_return_errors_and_leave_the_context_usable():
    from deepsir_amd.engine import EngineError
    src, ref, T0 = _batch(300, 300, 0.0, (4, 14, 24))
    eng = _engine(1024, 3)
    good = _run(eng, src, ref, T0)
    bad = [dict(res=0.0), dict(res=-1.0), dict(res=float("nan")), dict(res=float("inf")), dict(step_tol=0.0), dict(step_tol=float("nan")),
           dict(step_tol=float("inf")), dict(outlier_ratio=0.0), dict(outlier_ratio=1.0), dict(outlier_ratio=float("nan")),
           dict(neighbors=0), dict(neighbors=27), dict(max_iter=-1)]
    for kw in bad:
        with pytest.raises(EngineError, match="dsir_ndt_refine"):
            _run(eng, src, ref, T0, **kw)
        again = _run(eng, src, ref, T0)
        assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1]), kw
    with pytest.raises(EngineError, match="dsir_ndt_map"):
        eng.ndt_map(_dev(ref), 0.0)
    big = np.zeros((3, 4_000_000, 3), np.float32)                        # beyond the context's workspace
    with pytest.raises(EngineError, match="workspace too small"):
        eng.ndt_map(_dev(big), RES)
    again = _run(eng, src, ref, T0)
    assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1])
    eng.close()
