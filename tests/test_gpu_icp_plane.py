"""dsir_icp_refine_ex with the point-to-plane estimator (csrc/icp.hip: icp_plane_accum_kernel, icp_plane_step_kernel) against
the host rule tests/icp_plane_host.py, on the surface clouds of tests/test_icp_plane.py.  Every test carries the ``gpu`` mark.

Shapes (J, K): (37, 300) J below one wave and K != J; (300, 300); (1357, 1024) two chunks of the sums, six workgroups of the step,
J > K; (2500, 2500) with noise 0.004: three chunks.  Three pairs per call with different seeds.

Tolerances
  exact      `converged`, the counter of identity updates, every bitwise comparison
  existing   fitness 2e-3, rmse 1e-5 (tests/test_icp.py)
  measured   pose: POSE_TOL of tests/test_icp_plane.py = 4 x the host rule's largest deviation under +-1 ulp moves of the updated
             points (figures next to the constant there)
  iterations equal to the host's (the issue allows 1; both printed)

Measured on an MI355X (the tagged lines the tests print)
  PLANE      12 pairs: iterations device == host (3 .. 6), worst pose difference 7.6e-08 rad 7.4e-08, fitness equal, worst rmse
             difference 4.7e-08, no identity update
  FLAT       stats [1.0, 0.0275, 1, 1, 1] at max_iter 30 and 3: T_init back bit for bit, one iteration, one identity update
  NONFINITE  normals: 4 == 4 iterations, pose 5.9e-08 rad 4.1e-08; source: stats [0.9967, 0.0494, 1, 1, 1]; bystander 4 == 4
  HARNESS    host 6 / 13 iterations from the network's pose, pose difference 2.0e-08 rad 3.2e-08 / 5.4e-08 rad 1.3e-07
Every bitwise comparison (three normal routes, two runs, batch of 3 against single pairs, estimator 0 against dsir_icp_refine) held.
"""

import numpy as np
import pytest

from icp_plane_host import icp_plane
from test_icp_plane import CASES, POSE_TOL, RADIUS, flat_case, host_result, pose_err, surface_case

pytestmark = pytest.mark.gpu

FIT_TOL, RMSE_TOL = 2e-3, 1e-5


def _engine(max_points, max_pairs):
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    return Engine(NetConfig(), 0, max_points=max(max_points, 1024), max_pairs=max_pairs)


def _dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _run(eng, src, ref, T0, normals=None, r=RADIUS, **kw):
    """numpy in, numpy out: src [P,J,s], ref [P,K,s], T0 [P,3,4], normals [P,K,3] or None -> (T, stats [P,5])"""
    T, st = eng.icp_refine(_dev(src), _dev(ref), _dev(T0), r, estimator="plane", normals_ref=None if normals is None else _dev(normals),
                           **kw)
    return T.cpu().numpy(), st.cpu().numpy()


def _batch(J, K, noise, seeds):
    cases = [surface_case(J, K, s, noise) for s in seeds]
    return tuple(np.stack([c[k] for c in cases]) for k in ("src", "ref", "T0", "normals"))


def _check_against_host(tag, T, st, host):
    To, fitness, rmse, converged, iters, singular = host
    er, et = pose_err(T, To)
    print(f"{tag}: iterations device {int(st[3])} host {iters}, pose {er:.2e} rad {et:.2e}, fitness diff {abs(st[0] - fitness):.1e}, "
          f"rmse diff {abs(st[1] - rmse):.1e}, identity updates {int(st[4])}/{singular}")
    assert abs(st[0] - fitness) < FIT_TOL and abs(st[1] - rmse) < RMSE_TOL
    # iterations: the issue allows a difference of 1; the MI355X run showed the host's count in every case of this file
    # (3 .. 6 updates, the non-finite and bystander pairs included), so equality is asserted
    assert st[2] == float(converged) and st[3] == iters and st[4] == singular
    assert er < POSE_TOL and et < POSE_TOL, (er, et, POSE_TOL)


# ------------------------------------------------------------------ 1. device against the host rule
@pytest.mark.parametrize("J,K,noise,seeds", CASES)
def test_gpu_plane_matches_host_rule(J, K, noise, seeds):
    src, ref, T0, normals = _batch(J, K, noise, seeds)
    eng = _engine(max(J, K), 3)
    T, st = _run(eng, src, ref, T0, normals)
    assert st.shape == (3, 5) and np.isfinite(T).all() and np.isfinite(st).all()
    for k, seed in enumerate(seeds):
        _check_against_host(f"PLANE J={J} K={K} seed={seed}", T[k], st[k], host_result(J, K, seed, noise))
    eng.close()


# ------------------------------------------------------------------ 2. three input routes, same bytes
@pytest.mark.parametrize("J,K,noise,seeds", [c for c in CASES if c[1] >= 1024])
def test_gpu_plane_three_normal_routes_same_bytes(J, K, noise, seeds):
    import torch
    src, ref, T0, _ = _batch(J, K, noise, seeds)
    eng = _engine(max(J, K), 3)
    _, neigh, _, _ = eng.knn_pyramid(_dev(ref))
    normals, flags = eng.estimate_normals(_dev(ref), neigh)
    assert int(flags.sum()) == 0
    normals = normals.cpu().numpy()
    T_a, st_a = _run(eng, src, ref, T0, normals)                                  # normals_ref
    rows_ref = np.concatenate([ref, normals], 2)
    rows_src = np.concatenate([src, np.full_like(src, 7.0)], 2)                   # the source rows' own columns 3..5 are not read
    T_b, st_b = _run(eng, rows_src, rows_ref, T0)                                 # columns 3..5 of 6-column rows
    T_c, st_c = _run(eng, src, ref, T0)                                           # estimated by icp_refine itself
    assert T_a.tobytes() == T_b.tobytes() == T_c.tobytes() and st_a.tobytes() == st_b.tobytes() == st_c.tobytes()
    assert (st_a[:, 3] >= 1).all() and (st_a[:, 4] == 0).all()
    # separately: what the call estimates for itself is Engine.estimate_normals on the same pyramid
    assert torch.equal(eng.icp_normals(_dev(ref)).cpu(), torch.from_numpy(normals))
    eng.close()


def test_gpu_plane_estimating_route_refuses_small_and_large_clouds():
    c = surface_case(300, 300, 4)
    eng = _engine(1024, 1)
    with pytest.raises(ValueError, match="pass normals_ref"):
        _run(eng, c["src"][None], c["ref"][None], c["T0"][None])
    big = surface_case(37, 300, 3)
    ref = np.tile(big["ref"], (4, 1))[None]                                       # 1200 points > max_points = 1024
    with pytest.raises(ValueError, match="pass normals_ref"):
        _run(eng, big["src"][None], ref, big["T0"][None])
    eng.close()


# ------------------------------------------------------------------ 3. determinism and pair independence
@pytest.mark.parametrize("J,K,noise,seeds", CASES)
def test_gpu_plane_deterministic_and_pairs_independent(J, K, noise, seeds):
    src, ref, T0, normals = _batch(J, K, noise, seeds)
    eng = _engine(max(J, K), 3)
    for max_iter in (30, 3):                                                      # both parities of the transform ping-pong
        T, st = _run(eng, src, ref, T0, normals, max_iter=max_iter)
        T2, st2 = _run(eng, src, ref, T0, normals, max_iter=max_iter)
        assert T.tobytes() == T2.tobytes() and st.tobytes() == st2.tobytes()
        for k in range(3):
            T1, s1 = _run(eng, src[k:k + 1], ref[k:k + 1], T0[k:k + 1], normals[k:k + 1], max_iter=max_iter)
            assert T1[0].tobytes() == T[k].tobytes() and s1[0].tobytes() == st[k].tobytes(), (max_iter, k, s1, st[k])
    eng.close()


# ------------------------------------------------------------------ 4. estimator 0 equals the old entry
def _refine_ex(eng, src, ref, T0, estimator, normals, r=RADIUS, max_iter=30):
    """dsir_icp_refine_ex called directly -> (return code, T, stats [P,5])"""
    import torch
    s, t, t0 = _dev(src), _dev(ref), _dev(T0)
    n = None if normals is None else _dev(normals)
    P, J, stride = s.shape
    T = torch.zeros((P, 3, 4), dtype=torch.float32, device="cuda")
    st = torch.full((P, 5), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = eng.lib.dsir_icp_refine_ex(eng.h, s.data_ptr(), t.data_ptr(), P, J, t.shape[1], stride, float(r), int(max_iter), 1e-6, 1e-6,
                                    t0.data_ptr(), T.data_ptr(), int(estimator), None if n is None else n.data_ptr(), st.data_ptr())
    eng.sync()
    return rc, T.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("J,K,noise,seeds", [CASES[0], CASES[3]])
def test_gpu_estimator_point_equals_icp_refine(J, K, noise, seeds):
    src, ref, T0, normals = _batch(J, K, noise, seeds)
    eng = _engine(max(J, K), 3)
    import torch
    s, t, t0 = _dev(src), _dev(ref), _dev(T0)                                     # the old entry itself: dsir_icp_refine
    T_old = torch.zeros((3, 3, 4), dtype=torch.float32, device="cuda")
    st_old = torch.full((3, 4), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert eng.lib.dsir_icp_refine(eng.h, s.data_ptr(), t.data_ptr(), 3, J, K, s.shape[2], float(RADIUS), 30, 1e-6, 1e-6, t0.data_ptr(),
                                   T_old.data_ptr(), st_old.data_ptr()) == 0
    eng.sync()
    T_old, st_old = T_old.cpu().numpy(), st_old.cpu().numpy()
    T_def, st_def = eng.icp_refine(s, t, t0, RADIUS)                              # and the default Python call
    assert tuple(st_def.shape) == (3, 4)
    assert T_def.cpu().numpy().tobytes() == T_old.tobytes() and st_def.cpu().numpy().tobytes() == st_old.tobytes()
    for nrm in (None, normals):                                                   # estimator 0 does not read the normals
        rc, T, st = _refine_ex(eng, src, ref, T0, 0, nrm)
        assert rc == 0
        assert T.tobytes() == T_old.tobytes() and st[:, :4].tobytes() == st_old.tobytes() and (st[:, 4] == 0.0).all()
    eng.close()


# ------------------------------------------------------------------ 5. corner cases
def test_gpu_plane_flat_target_is_singular():
    """pair 1 is a planar target: T_init comes back, the counter equals the iterations; pairs 0 and 2 keep their bytes"""
    J = K = 300
    cases = [surface_case(J, K, 4), flat_case(J, K), surface_case(J, K, 24)]
    src, ref, T0, normals = (np.stack([c[k] for c in cases]) for k in ("src", "ref", "T0", "normals"))
    eng = _engine(K, 3)
    for max_iter in (30, 3):
        T, st = _run(eng, src, ref, T0, normals, max_iter=max_iter)
        c = cases[1]
        To, fitness, rmse, converged, iters, singular = icp_plane(c["src"], c["ref"], c["normals"], c["T0"], RADIUS, max_iter=max_iter)
        print(f"FLAT max_iter={max_iter}: stats {st[1].tolist()} host iterations {iters} singular {singular}")
        assert T[1].tobytes() == T0[1].tobytes()
        assert st[1, 4] == st[1, 3] == iters == singular and st[1, 2] == float(converged) and st[1, 0] == fitness > 0.5
        for k in (0, 2):
            T1, s1 = _run(eng, src[k:k + 1], ref[k:k + 1], T0[k:k + 1], normals[k:k + 1], max_iter=max_iter)
            assert T1[0].tobytes() == T[k].tobytes() and s1[0].tobytes() == st[k].tobytes() and st[k, 4] == 0.0
    eng.close()


def test_gpu_plane_non_finite_values_stay_where_they_are():
    """pair 0: NaN / inf / zero normals on 40 reference points - only those correspondences leave the update (the host rule with
    the same normals agrees within the tolerances).  pair 1: a NaN source coordinate - identity updates, T_init back, T finite with
    det R = 1.  pair 2: untouched, its single-pair bytes."""
    J, K = 300, 300
    cases = [surface_case(J, K, s) for s in (4, 14, 24)]
    src, ref, T0, normals = (np.stack([c[k] for c in cases]).copy() for k in ("src", "ref", "T0", "normals"))
    normals[0, 0:20, 1] = np.nan
    normals[0, 20:30, 0] = np.inf
    normals[0, 30:40] = 0.0
    src[1, 7, 2] = np.nan
    eng = _engine(K, 3)
    T, st = _run(eng, src, ref, T0, normals)
    assert np.isfinite(T).all() and np.isfinite(st).all()
    _check_against_host("NONFINITE normals", T[0], st[0], icp_plane(src[0], ref[0], normals[0], T0[0], RADIUS))
    er, et = pose_err(T[0], cases[0]["T_gt"])
    assert er < 1e-5 and et < 1e-5                                                # 260 good rows: still the truth
    print(f"NONFINITE source: stats {st[1].tolist()}")
    assert T[1].tobytes() == T0[1].tobytes() and st[1, 2] == 1.0 and st[1, 3] == 1.0 and st[1, 4] == 1.0 and 0.0 < st[1, 0] < 1.0
    assert abs(np.linalg.det(T[1][:, :3].astype(np.float64)) - 1.0) < 1e-5
    T1, s1 = _run(eng, src[2:3], ref[2:3], T0[2:3], normals[2:3])
    assert T1[0].tobytes() == T[2].tobytes() and s1[0].tobytes() == st[2].tobytes()
    _check_against_host("NONFINITE bystander", T[2], st[2], host_result(J, K, 24))
    eng.close()


def test_gpu_plane_nothing_in_reach_max_iter_zero_and_bad_arguments():
    from deepsir_amd.engine import EngineError
    J, K, noise, seeds = CASES[1]
    src, ref, T0, normals = _batch(J, K, noise, seeds)
    eng = _engine(K, 3)
    # a radius that admits nothing: T_init comes back (fewer than 6 rows: identity updates, counted), fitness 0
    T, st = _run(eng, src, ref + np.float32(100.0), T0, normals)
    assert T.tobytes() == T0.tobytes() and (st[:, 0] == 0.0).all() and (st[:, 1] == 0.0).all()
    assert (st[:, 2] == 1.0).all() and (st[:, 3] == 1.0).all() and (st[:, 4] == 1.0).all()
    # max_iter = 0: the first search's statistics, T_out = T_init
    T, st = _run(eng, src, ref, T0, normals, max_iter=0)
    T_p, st_p = eng.icp_refine(_dev(src), _dev(ref), _dev(T0), RADIUS, max_iter=0)
    assert T.tobytes() == T0.tobytes() and st[:, :4].tobytes() == st_p.cpu().numpy().tobytes()
    assert (st[:, 0] > 0.5).all() and (st[:, 2:] == 0.0).all()
    # estimator 1, no normals, rows of 3 columns: an error string, not an abort; the context still works afterwards
    rc, _, _ = _refine_ex(eng, src, ref, T0, 1, None)
    assert rc != 0 and b"stride" in eng.lib.dsir_last_error(eng.h) and b"bad arguments" in eng.lib.dsir_last_error(eng.h)
    rc, _, _ = _refine_ex(eng, src, ref, T0, 2, normals)
    assert rc != 0 and b"bad arguments" in eng.lib.dsir_last_error(eng.h)
    with pytest.raises(ValueError):
        eng.icp_refine(_dev(src), _dev(ref), _dev(T0), RADIUS, estimator="nope")
    with pytest.raises((ValueError, EngineError)):
        eng.icp_refine(_dev(src), _dev(ref), _dev(T0), RADIUS, estimator="plane", normals_ref=_dev(normals[:, :10]))
    rc, T2, st2 = _refine_ex(eng, src, ref, T0, 1, normals)
    T3, st3 = _run(eng, src, ref, T0, normals)
    assert rc == 0 and T2.tobytes() == T3.tobytes() and st2.tobytes() == st3.tobytes()
    eng.close()


# ------------------------------------------------------------------ 6. harness
def test_gpu_harness_pose_opt_icp_plane():
    """inference_align(pose_opt='icp_plane') on two 2048-point surface pairs: the appended pose is the host rule's, started from
    the network's last pose (normals: the engine's own estimate, as the harness takes them); the earlier entries are the plain
    run's, bit for bit."""
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
    plane, _ = inference_align(pairs, net, 3, batch=2, pose_opt="icp_plane", voxel_size=0.05)
    assert plain.shape == plane.shape == (2, 4, 3, 4)
    assert plain[:, :3].tobytes() == plane[:, :3].tobytes() and np.array_equal(plain[:, 3], plain[:, 2])
    with pytest.raises(ValueError, match="icp_plane"):
        inference_align(pairs, net, 3, batch=2, pose_opt="nope")
    eng = net._ensure_engine(2048, 2)
    ref = _dev(np.stack([c["ref"] for c in cases]))
    normals = eng.estimate_normals(ref, eng.knn_pyramid(ref)[1])[0].cpu().numpy()
    for k, c in enumerate(cases):
        To, fitness, rmse, converged, iters, singular = icp_plane(c["src"], c["ref"], normals[k], plain[k, 2], 0.1)
        er, et = pose_err(plane[k, 3], To)
        print(f"HARNESS pair {k}: host {iters} iterations fitness {fitness:.3f} singular {singular}, pose {er:.2e} rad {et:.2e}")
        assert er < POSE_TOL and et < POSE_TOL
