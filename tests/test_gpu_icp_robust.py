"""dsir_icp_refine_ex4: the robust loss kernels of both ICP estimators (csrc/icp.hip: icp_stats_kernel<true>,
icp_plane_accum_kernel<true>, the Kabsch kernels' zero_freeze) against the host rule tests/icp_robust_host.py, their plumbing up to
``register_scene``, and ``harness.icp_multiscale``.  Every test carries the ``gpu`` mark.

Cases, scales and tolerances are those of tests/test_icp_robust_host.py (chosen and measured there on the CPU): shapes (37, 300),
(300, 300), (1357, 1024), three pairs per call, clean and with 20 % of the source points displaced by (0, 0, 0.095).
  exact      `converged`, the identity-update counter, every bitwise comparison
  existing   fitness 2e-3, rmse 1e-5, point-estimator pose 2e-5 (tests/test_icp.py)
  measured   plane-estimator pose: PLANE_POSE_TOL = 4 x the robust host rule's largest deviation under +-1 ulp moves (5.0e-07)
  iterations equal to the host's; a difference of 1 is allowed and printed, as the issue sets it (the host rule itself moves by one
             under the ulp hook in one (1357, 1024) run)
"""
import numpy as np
import pytest

import icp_robust_host as H
from test_icp_plane import RADIUS, pose_err, surface_case
from test_icp_robust_host import PLANE_POSE_TOL, POINT_POSE_TOL, SCALES, SHAPES, host_result, robust_case

pytestmark = pytest.mark.gpu

FIT_TOL, RMSE_TOL = 2e-3, 1e-5
ESTIMATORS = ("point", "plane")


def _engine(max_points, max_pairs):
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    return Engine(NetConfig(), 0, max_points=max(max_points, 1024), max_pairs=max_pairs)


def _dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _batch(J, K, seeds, outliers):
    cases = [robust_case(J, K, s, outliers) for s in seeds]
    return tuple(np.stack([c[k] for c in cases]) for k in ("src", "ref", "T0", "normals"))


def _run(eng, est, src, ref, T0, normals, r=RADIUS, **kw):
    """numpy (or device tensors) in, numpy out -> (T [P,3,4], stats [P,4|5])"""
    import torch
    d = lambda a: a if isinstance(a, torch.Tensor) else _dev(a)
    T, st = eng.icp_refine(d(src), d(ref), d(T0), r, estimator=est, normals_ref=d(normals) if est == "plane" else None, **kw)
    return T.cpu().numpy(), st.cpu().numpy()


def _same(a, b):
    return all(x.tobytes() == y.tobytes() and x.shape == y.shape for x, y in zip(a, b))


def _check_against_host(tag, est, T, st, host, max_iter=30):
    To, fitness, rmse, converged, iters, identity = host
    er, et = pose_err(T, To)
    tol = PLANE_POSE_TOL if est == "plane" else POINT_POSE_TOL
    print(f"{tag}: iterations device {int(st[3])} host {iters}, pose {er:.2e} rad {et:.2e} (tol {tol:.1e}), fitness diff "
          f"{abs(st[0] - fitness):.1e}, rmse diff {abs(st[1] - rmse):.1e}, identity updates host {identity}")
    assert abs(st[0] - fitness) < FIT_TOL and abs(st[1] - rmse) < RMSE_TOL
    assert st[2] == float(converged)
    if st[3] != iters:
        print(f"{tag}: ITERATIONS DIFFER device {int(st[3])} host {iters}")
    assert abs(st[3] - iters) <= 1
    if est == "plane":
        assert st[4] == identity
    else:
        assert identity == 0
    assert er < tol and et < tol, (er, et, tol)


# ------------------------------------------------------------------ 1. device against the host rule
@pytest.mark.parametrize("outliers", (False, True))
@pytest.mark.parametrize("J,K,seeds", SHAPES)
def test_gpu_robust_matches_host_rule(J, K, seeds, outliers):
    src, ref, T0, normals = (_dev(a) for a in _batch(J, K, seeds, outliers))
    eng = _engine(max(J, K), 3)
    for est in ESTIMATORS:
        for kernel, k in SCALES.items():
            T, st = _run(eng, est, src, ref, T0, normals, kernel=kernel, kernel_scale=k)
            assert st.shape == (3, 5 if est == "plane" else 4) and np.isfinite(T).all() and np.isfinite(st).all()
            T1, st1 = _run(eng, est, src, ref, T0, normals, kernel=kernel, kernel_scale=k, max_iter=1)
            for p, seed in enumerate(seeds):
                tag = f"ROBUST J={J} K={K} seed={seed} outliers={int(outliers)} {est} {kernel}"
                _check_against_host(tag, est, T[p], st[p], host_result(J, K, seed, outliers, est, kernel))
                _check_against_host(tag + " max_iter=1", est, T1[p], st1[p], host_result(J, K, seed, outliers, est, kernel, max_iter=1))
    eng.close()


def test_gpu_tukey_holds_the_truth_where_l2_does_not():
    """the device on the outlier cases: under tukey at least 5 times closer to T_gt than under l2 (the host rule's margin is 7.4)"""
    J, K, seeds = SHAPES[1]
    src, ref, T0, normals = (_dev(a) for a in _batch(J, K, seeds, True))
    eng = _engine(K, 3)
    for est in ESTIMATORS:
        T_l2, _ = _run(eng, est, src, ref, T0, normals)
        T_tk, _ = _run(eng, est, src, ref, T0, normals, kernel="tukey", kernel_scale=SCALES["tukey"])
        for p, seed in enumerate(seeds):
            gt = robust_case(J, K, seed, True)["T_gt"]
            e_l2, e_tk = max(pose_err(T_l2[p], gt)), max(pose_err(T_tk[p], gt))
            print(f"DEVICE OUTLIERS seed={seed} {est}: l2 {e_l2:.2e} tukey {e_tk:.2e}")
            assert e_l2 >= 5.0 * e_tk
    eng.close()


# ------------------------------------------------------------------ 2. l2 keeps its bytes
def _refine_abi(eng, entry, est, src, ref, T0, normals, search=0, counts=(None, None), tail=(), r=RADIUS, max_iter=30):
    """dsir_icp_refine_ex3 / _ex4 called directly -> (return code, T, stats [P,5])"""
    import ctypes
    import torch
    P, J, stride = src.shape
    T = torch.zeros((P, 3, 4), dtype=torch.float32, device="cuda")
    st = torch.full((P, 5), -1.0, dtype=torch.float64, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()
    torch.cuda.synchronize()
    rc = getattr(eng.lib, entry)(eng.h, src.data_ptr(), ref.data_ptr(), P, J, ref.shape[1], stride, float(r), int(max_iter), 1e-6, 1e-6,
                                 T0.data_ptr(), T.data_ptr(), int(est == "plane"), ptr(normals) if est == "plane" else None, int(search),
                                 st.data_ptr(), ptr(counts[0]), ptr(counts[1]), *[ctypes.c_float(x) if isinstance(x, float) else x for x in tail])
    eng.sync()
    return rc, T.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("est", ESTIMATORS)
def test_gpu_l2_is_byte_for_byte_icp_refine_ex3(est):
    J, K, seeds = SHAPES[2]
    src, ref, T0, normals = (_dev(a) for a in _batch(J, K, seeds, True))
    eng = _engine(max(J, K), 3)
    rc, T3, st3 = _refine_abi(eng, "dsir_icp_refine_ex3", est, src, ref, T0, normals)
    assert rc == 0 and (st3[:, 3] >= 2).all()
    cols = 5 if est == "plane" else 4
    want = (T3, np.ascontiguousarray(st3[:, :cols]))
    assert _same(_run(eng, est, src, ref, T0, normals), want)
    assert _same(_run(eng, est, src, ref, T0, normals, kernel="l2"), want)
    assert _same(_run(eng, est, src, ref, T0, normals, kernel="l2", kernel_scale=float("nan")), want)       # ignored with l2
    for scale in (0.0, float("nan"), -1.0, 0.05):                                                            # and in the C entry
        rc, T4, st4 = _refine_abi(eng, "dsir_icp_refine_ex4", est, src, ref, T0, normals, tail=(0, scale))
        assert rc == 0 and _same((T4, st4), (T3, st3)), scale
    eng.close()


# ------------------------------------------------------------------ 3. huber beyond the radius: the weighted path, all weights 1
@pytest.mark.parametrize("search", ("brute", "grid"))
@pytest.mark.parametrize("est", ESTIMATORS)
def test_gpu_huber_beyond_the_radius_is_l2_byte_for_byte(est, search):
    from deepsir_amd.harness import pad_clouds
    J, K, seeds = SHAPES[2]
    src, ref, T0, normals = (_dev(a) for a in _batch(J, K, seeds, True))
    eng = _engine(max(J, K), 3)
    kw = dict(kernel="huber", kernel_scale=2 * RADIUS)
    a = _run(eng, est, src, ref, T0, normals, search=search)
    assert (a[1][:, 3] >= 2).all() and (a[1][:, 0] > 0.5).all()
    assert _same(_run(eng, est, src, ref, T0, normals, search=search, **kw), a)
    # with counts: unequal sizes, NaN padding
    n_s, n_t = (1357, 900, 37), (1024, 1000, 300)
    ps, cs = pad_clouds([src[p, :n] for p, n in enumerate(n_s)])
    pr, cr = pad_clouds([ref[p, :n] for p, n in enumerate(n_t)])
    pn, _ = pad_clouds([normals[p, :n] for p, n in enumerate(n_t)])
    b = _run(eng, est, ps, pr, T0, pn, search=search, counts_src=cs, counts_ref=cr)
    assert _same(_run(eng, est, ps, pr, T0, pn, search=search, counts_src=cs, counts_ref=cr, **kw), b)
    assert b[0][0].tobytes() == a[0][0].tobytes() and b[0][1].tobytes() != a[0][1].tobytes()
    eng.close()


# ------------------------------------------------------------------ 4. same bytes under a robust kernel
@pytest.mark.parametrize("kernel", ("tukey", "cauchy"))
@pytest.mark.parametrize("est", ESTIMATORS)
def test_gpu_robust_same_bytes(est, kernel):
    from deepsir_amd.harness import pad_clouds
    J, K, seeds = SHAPES[2]
    src, ref, T0, normals = (_dev(a) for a in _batch(J, K, seeds, True))
    eng = _engine(max(J, K), 3)
    kw = dict(kernel=kernel, kernel_scale=SCALES[kernel])
    a = _run(eng, est, src, ref, T0, normals, **kw)
    assert _same(_run(eng, est, src, ref, T0, normals, **kw), a)                                             # two runs
    assert _same(_run(eng, est, src, ref, T0, normals, search="grid", **kw), a)                             # grid = brute
    assert not _same(_run(eng, est, src, ref, T0, normals), a)                                               # and it is not l2
    for p in range(3):                                                                                       # a batch of 3 = single pairs
        one = _run(eng, est, src[p:p + 1], ref[p:p + 1], T0[p:p + 1], normals[p:p + 1], **kw)
        assert one[0][0].tobytes() == a[0][p].tobytes() and one[1][0].tobytes() == a[1][p].tobytes(), p
    # a pair in a ragged batch (NaN padding) = the pair alone
    n_s, n_t = (1357, 900, 37), (1024, 1000, 300)
    ps, cs = pad_clouds([src[p, :n] for p, n in enumerate(n_s)])
    pr, cr = pad_clouds([ref[p, :n] for p, n in enumerate(n_t)])
    pn, _ = pad_clouds([normals[p, :n] for p, n in enumerate(n_t)])
    for search in ("brute", "grid"):
        b = _run(eng, est, ps, pr, T0, pn, search=search, counts_src=cs, counts_ref=cr, **kw)
        assert np.isfinite(b[0]).all() and np.isfinite(b[1]).all()
        for p in range(3):
            one = _run(eng, est, src[p:p + 1, :n_s[p]].contiguous(), ref[p:p + 1, :n_t[p]].contiguous(), T0[p:p + 1],
                       normals[p:p + 1, :n_t[p]].contiguous(), **kw)
            assert one[0][0].tobytes() == b[0][p].tobytes() and one[1][0].tobytes() == b[1][p].tobytes(), (search, p)
    eng.close()


# ------------------------------------------------------------------ 5. all weights zero
@pytest.mark.parametrize("est", ESTIMATORS)
def test_gpu_all_zero_weights_carry_the_pose_over(est):
    """tukey with k = 1e-6 on noisy clouds: every weight is 0, every update the identity; T_init comes back bit for bit - its -0.0
    entries included, which composing with an identity transform would turn into +0.0"""
    J = K = 300
    cases = [surface_case(J, K, s, 0.004) for s in (4, 14, 24)]
    src, ref, T0, normals = (np.stack([c[k] for c in cases]) for k in ("src", "ref", "T0", "normals"))
    T0 = T0.copy()
    T0[1, 0, 3] = np.float32(-0.0)                                      # pair 1: a pose with a -0.0 entry (and so a worse start)
    eng = _engine(K, 3)
    for max_iter in (30, 3):
        T, st = _run(eng, est, src, ref, T0, normals, kernel="tukey", kernel_scale=1e-6, max_iter=max_iter)
        print(f"ZERO WEIGHTS {est} max_iter={max_iter}: stats {st.tolist()}")
        assert np.isfinite(T).all() and np.isfinite(st).all()
        assert T.tobytes() == T0.tobytes()
        assert (st[[0, 2], 0] > 0.5).all() and (st[:, 2] == 1.0).all() and (st[:, 3] == 1.0).all()
        if est == "plane":
            assert (st[:, 4] == st[:, 3]).all()
        for p in (0, 2):                                                 # the host rule says the same
            c = cases[p]
            To, fitness, rmse, converged, iters, identity = (H.icp_point(c["src"], c["ref"], c["T0"], RADIUS, "tukey", 1e-6, max_iter=max_iter)
                                                             if est == "point" else
                                                             H.icp_plane(c["src"], c["ref"], c["normals"], c["T0"], RADIUS, "tukey", 1e-6, max_iter=max_iter))
            assert st[p, 3] == iters == identity and st[p, 0] == fitness and abs(st[p, 1] - rmse) < RMSE_TOL
    eng.close()


# ------------------------------------------------------------------ 6. refusals and the symbol
def test_gpu_robust_refusals():
    J, K, seeds = SHAPES[0]
    src, ref, T0, normals = (_dev(a) for a in _batch(J, K, seeds, False))
    eng = _engine(K, 3)
    assert hasattr(eng.lib, "dsir_icp_refine_ex4")
    for kernel, scale in (("l1", 0.05), ("TUKEY", 0.05), (None, 0.05), ("tukey", 0.0), ("huber", -0.05), ("cauchy", float("nan")),
                          ("gm", float("inf")), ("tukey", None)):
        with pytest.raises(ValueError):
            eng.icp_refine(src, ref, T0, RADIUS, kernel=kernel, kernel_scale=scale)
    for tail in ((5, 0.05), (-1, 0.05), (4, 0.0), (1, -0.05), (2, float("nan")), (3, float("inf")), (4, float("-inf"))):
        rc, _, _ = _refine_abi(eng, "dsir_icp_refine_ex4", "point", src, ref, T0, normals, tail=tail)
        err = eng.lib.dsir_last_error(eng.h)
        assert rc != 0 and b"dsir_icp_refine_ex4" in err and b"bad arguments" in err and b"kernel" in err, (tail, err)
    # the scale is ignored with l2, and the context still works
    rc, T4, st4 = _refine_abi(eng, "dsir_icp_refine_ex4", "point", src, ref, T0, normals, tail=(0, float("inf")))
    T, st = _run(eng, "point", src, ref, T0, normals)
    assert rc == 0 and T4.tobytes() == T.tobytes() and st4[:, :4].tobytes() == st.tobytes()
    rc, T4, st4 = _refine_abi(eng, "dsir_icp_refine_ex4", "plane", src, ref, T0, normals, tail=(4, 0.08))
    assert rc == 0 and _same((T4, st4), _run(eng, "plane", src, ref, T0, normals, kernel="tukey", kernel_scale=0.08))
    eng.close()


# ------------------------------------------------------------------ 7. register_scene forwards
def test_gpu_register_scene_forwards_the_kernel():
    import torch
    from deepsir_amd import harness as HN
    from test_gpu_icp_ragged import _scene
    frags, edges = _scene()
    eng = _engine(2304, 4)
    kw = dict(icp_kernel="tukey", icp_kernel_scale=0.05)
    res = {name: HN.register_scene(frags, eng, edges, voxel_size=0.05, batch=4, **k) for name, k in (("l2", {}), ("tukey", kw))}
    differ = 0
    for name, k in (("l2", {}), ("tukey", dict(kernel="tukey", kernel_scale=0.05))):
        for row, (s, t, T_init, _) in zip(res[name]["edges"], edges):
            src, ref = _dev(frags[s])[None], _dev(frags[t])[None]
            T, _ = eng.icp_refine(src, ref, _dev(np.asarray(T_init, np.float32)[None, :3]), 0.1, search="auto", **k)
            assert T[0].cpu().numpy().astype(np.float64).tobytes() == np.asarray(row["T"]).tobytes(), (name, s, t)
            info, count = eng.information_matrix(src, ref, T, 0.1, search="auto")                   # the information matrix: unweighted
            assert info[0].cpu().numpy().tobytes() == np.asarray(row["info"]).tobytes() and int(count[0]) == row["count"]
    for a, b in zip(res["l2"]["edges"], res["tukey"]["edges"]):
        differ += np.asarray(a["T"]).tobytes() != np.asarray(b["T"]).tobytes()
    assert differ >= 1
    with pytest.raises(ValueError):
        HN.register_scene(frags, eng, edges, voxel_size=0.05, icp_kernel="tukey")
    torch.cuda.synchronize()
    eng.close()


# ------------------------------------------------------------------ 8. coarse to fine
@pytest.mark.parametrize("est", ESTIMATORS)
def test_gpu_icp_multiscale_is_its_engine_calls(est):
    """two scales on one pair of unequal sizes (1357 and 1024 points) plus a smaller pair: byte-identical to the calls written out"""
    from deepsir_amd.harness import icp_multiscale, pad_clouds
    cases = [robust_case(1357, 1024, 9, True), robust_case(300, 300, 4, True)]
    srcs, refs = [_dev(c["src"]) for c in cases], [_dev(c["ref"]) for c in cases]
    T0 = np.stack([c["T0"] for c in cases])
    eng = _engine(2048, 2)
    voxels, iters, scales = (0.08, 0.03), (20, 30), (0.2, 0.08)
    T, stats = icp_multiscale(srcs, refs, T0, voxels, iters, estimator=est, kernel="tukey", kernel_scales=scales, search="grid", engine=eng)
    # by hand
    Th = _dev(T0)
    for voxel, it, k in zip(voxels, iters, scales):
        vs, ns = eng.voxel_downsample(srcs, voxel)
        vr, nr = eng.voxel_downsample(refs, voxel)
        eng.sync()
        ns, nr = ns.cpu().tolist(), nr.cpu().tolist()
        s_list, r_list = [vs[i, :ns[i]].contiguous() for i in range(2)], [vr[i, :nr[i]].contiguous() for i in range(2)]
        assert ns[0] != nr[0] and min(ns + nr) >= 6
        ps, cs = pad_clouds(s_list)
        pr, cr = pad_clouds(r_list)
        nrm = None
        if est == "plane":
            nrm = pad_clouds([eng.estimate_normals(c[None], csr=eng.radius_neighbors(c[None], 2 * voxel, max_nn=30))[0][0] for c in r_list])[0]
        Th, sth = eng.icp_refine(ps, pr, Th, 2 * voxel, max_iter=it, estimator=est, normals_ref=nrm, search="grid", counts_src=cs, counts_ref=cr,
                                 kernel="tukey", kernel_scale=k)
        print(f"MULTISCALE {est} voxel {voxel}: sizes {ns} {nr}, stats {sth.cpu().numpy().tolist()}")
    assert len(stats) == 2 and T.cpu().numpy().tobytes() == Th.cpu().numpy().tobytes()
    assert stats[1].cpu().numpy().tobytes() == sth.cpu().numpy().tobytes()
    with pytest.raises(ValueError):
        icp_multiscale(srcs, refs, T0, (None,), (5,), engine=eng)                                            # no voxel size, no radius
    with pytest.raises(ValueError):
        icp_multiscale(srcs, refs, T0, voxels, (5,), engine=eng)
    eng.close()


def test_gpu_icp_multiscale_reaches_what_the_fine_radius_alone_does_not():
    """a start outside the fine radius's basin (chosen on the host rule: fine alone ends 0.79 from T_gt, coarse then fine 3.6e-08)"""
    from deepsir_amd.harness import icp_multiscale
    from test_icp_robust_host import C2F_RADII, c2f_case
    c, T_start = c2f_case()
    eng = _engine(1357, 1)
    T, stats = icp_multiscale([c["src"]], [c["ref"]], T_start[None], (None, None), (30, 30), radii=C2F_RADII, engine=eng)
    er, et = pose_err(T[0].cpu().numpy(), c["T_gt"])
    print(f"COARSE TO FINE: device error {er:.2e} rad {et:.2e}, stats {[s.cpu().numpy().tolist() for s in stats]}")
    assert er < POINT_POSE_TOL and et < POINT_POSE_TOL
    Tf, stf = icp_multiscale([c["src"]], [c["ref"]], T_start[None], (None,), (30,), radii=C2F_RADII[1:], engine=eng)
    print(f"FINE ONLY: device error {pose_err(Tf[0].cpu().numpy(), c['T_gt'])}, stats {stf[0].cpu().numpy().tolist()}")   # not asserted
    eng.close()
