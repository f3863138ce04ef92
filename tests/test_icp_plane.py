"""The point-to-plane ICP rule on the host (tests/icp_plane_host.py restates csrc/icp.hip's header) and the C-ABI declaration of
dsir_icp_refine_ex.  No GPU.  The surface clouds and the pose tolerance of tests/test_gpu_icp_plane.py are built and measured here.

synth.make_pair fills a volume, so its neighbourhoods have no planes; the clouds here are a surface: three quarters of the points
on z = 0.15 sin(3x) cos(2.5y) over [0, 1.5]^2, one quarter on the wall x = 0.02 sin(4u), y = 1.5u, z = 0.8v - 0.15.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from icp_plane_host import IDENTITY, icp_plane, normal_sums, solve, vec6_to_T
from oracle.icp import icp

RADIUS = 0.1

# (J, K, noise on ref, seeds of the three pairs of a call): the shapes of tests/test_gpu_icp_plane.py
CASES = [(37, 300, 0.0, (3, 13, 23)), (300, 300, 0.0, (4, 14, 24)), (1357, 1024, 0.0, (9, 19, 29)), (2500, 2500, 0.004, (8, 18, 28))]
ULP_SEEDS = (1, 2, 3, 4)


def rot_err(Ra, Rb):
    D = np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)
    v = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(np.linalg.norm(v), 0.5 * (np.trace(D) - 1.0)))


def pose_err(Ta, Tb):
    return rot_err(Ta[:, :3], Tb[:, :3]), float(np.linalg.norm(np.asarray(Ta, np.float64)[:, 3] - np.asarray(Tb, np.float64)[:, 3]))


def _rodrigues(ax, a):
    ax = np.asarray(ax, np.float64) / np.linalg.norm(ax)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def surface(n, rng):
    m = n * 3 // 4
    xy = rng.uniform(0, 1.5, (m, 2))
    a = np.c_[xy, 0.15 * np.sin(3.0 * xy[:, 0]) * np.cos(2.5 * xy[:, 1])]
    uv = rng.uniform(0, 1.0, (n - m, 2))
    b = np.c_[0.02 * np.sin(4.0 * uv[:, 0]), 1.5 * uv[:, 0], 0.8 * uv[:, 1] - 0.15]
    return np.r_[a, b][rng.permutation(n)]


def knn16(p):
    """exact 16 nearest neighbours (self first), float64, ties to the lower index"""
    p = np.asarray(p, np.float64)
    d = ((p[:, None, :] - p[None]) ** 2).sum(-1) if len(p) <= 1500 else np.stack([((q - p) ** 2).sum(-1) for q in p])
    return np.argsort(d, 1, kind="stable")[:, :16].astype(np.int32)


_CASE_CACHE = {}


def surface_case(J, K, seed, noise=0.0):
    """-> dict(src [J,3] f32, ref [K,3] f32, normals [K,3] f32 of ref (deepsir_amd.ppf.estimate_normals on exact 16-NN lists), flags,
    T_gt [3,4] f64 (ref = T_gt src), T0 [3,4] f32: 3 degrees about a seeded axis and up to 0.05 per axis off T_gt).  The surface has
    K points; src is its rigid copy, permuted independently: the first J of it, or (J > K) all of it and J - K points a second
    time, so that every source point has its exact partner and the truth is the minimiser."""
    key = (J, K, seed, noise)
    if key in _CASE_CACHE:
        return _CASE_CACHE[key]
    from deepsir_amd.ppf import estimate_normals
    rng = np.random.default_rng(seed)
    base = surface(K, rng).astype(np.float32).astype(np.float64)
    R, t = _rodrigues(rng.standard_normal(3), rng.uniform(0.3, 1.0)), rng.uniform(-0.5, 0.5, 3)
    ref = base.astype(np.float32)
    pick = np.concatenate([rng.permutation(K), rng.integers(0, K, max(J - K, 0))])[:J]
    src = ((base[pick] - t) @ R).astype(np.float32)                                        # R^T (p - t)
    if noise:
        ref = (ref + rng.normal(0, noise, ref.shape)).astype(np.float32)
    dR = _rodrigues(rng.standard_normal(3), np.deg2rad(3.0))
    T0 = np.hstack([dR @ R, (dR @ t + rng.uniform(-0.05, 0.05, 3))[:, None]]).astype(np.float32)
    normals, flags = estimate_normals(ref[None], knn16(ref)[None])
    c = dict(src=src, ref=ref, normals=np.ascontiguousarray(normals[0], np.float32), flags=flags[0], T_gt=np.hstack([R, t[:, None]]), T0=T0)
    _CASE_CACHE[key] = c
    return c


_HOST_CACHE = {}


def host_result(J, K, seed, noise=0.0, **kw):
    """icp_plane_host.icp_plane on a surface case, computed once per (case, arguments)"""
    key = (J, K, seed, noise, tuple(sorted(kw.items())))
    if key not in _HOST_CACHE:
        c = surface_case(J, K, seed, noise)
        _HOST_CACHE[key] = icp_plane(c["src"], c["ref"], c["normals"], c["T0"], RADIUS, **kw)
    return _HOST_CACHE[key]


def flat_case(J=300, K=400, seed=5):
    """a planar target z = 0 with normals (0, 0, 1): the system of every update is singular (rotation about z, translation in
    x and y are free)"""
    rng = np.random.default_rng(seed)
    ref = np.c_[rng.uniform(0, 1, (K, 2)), np.zeros(K)].astype(np.float32)
    src = (ref[rng.permutation(K)[:J]] + np.array([0.01, -0.02, 0.03])).astype(np.float32)
    normals = np.tile(np.array([0, 0, 1], np.float32), (K, 1))
    T0 = np.hstack([_rodrigues([0.2, -0.1, 1.0], 0.02), [[0.01], [0.0], [-0.01]]]).astype(np.float32)
    return dict(src=src, ref=ref, normals=normals, T0=T0)


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("J,K,noise,seeds", CASES)
def test_surface_normals_are_not_degenerate(J, K, noise, seeds):
    for seed in seeds:
        c = surface_case(J, K, seed, noise)
        assert int(c["flags"].sum()) == 0
        assert np.allclose(np.linalg.norm(c["normals"].astype(np.float64), axis=1), 1.0, atol=1e-6)


@pytest.mark.parametrize("J,K,noise,seeds", [c for c in CASES if c[2] == 0.0])
def test_host_rule_recovers_the_truth(J, K, noise, seeds):
    """noise-free: rotation and translation error below 1e-5 (the CPU prototype reached 1e-7), converged within max_iter"""
    for seed in seeds:
        c = surface_case(J, K, seed)
        T, fitness, rmse, converged, iters, singular = host_result(J, K, seed)
        er, et = pose_err(T, c["T_gt"])
        print(f"HOST J={J} K={K} seed={seed}: {iters} updates, fitness {fitness:.3f} rmse {rmse:.2e}, error {er:.1e} rad {et:.1e}")
        assert converged and iters <= 30 and singular == 0
        assert er < 1e-5 and et < 1e-5


def test_host_rule_converges_with_noise():
    J, K, noise, seeds = CASES[3]
    for seed in seeds:
        T, fitness, rmse, converged, iters, singular = host_result(J, K, seed, noise)
        er, et = pose_err(T, surface_case(J, K, seed, noise)["T_gt"])
        assert converged and iters <= 30 and singular == 0 and er < 5e-3 and et < 5e-3, (seed, iters, er, et)


def test_plane_needs_no_more_updates_than_point():
    """1024 points, seed 7: the prototype took 4 updates against point-to-point's 10"""
    c = surface_case(1024, 1024, 7)
    it_plane = host_result(1024, 1024, 7)[4]
    it_point = icp(c["src"], c["ref"], c["T0"], RADIUS)[4]
    print(f"UPDATES plane {it_plane} point {it_point}")
    assert it_plane <= it_point


def test_flat_target_is_singular():
    c = flat_case()
    for max_iter in (30, 3):
        T, fitness, rmse, converged, iters, singular = icp_plane(c["src"], c["ref"], c["normals"], c["T0"], RADIUS, max_iter=max_iter)
        assert fitness > 0.5 and iters >= 1
        assert np.array_equal(T, c["T0"].astype(np.float64))          # every update the identity: T_init comes back
        assert singular == iters
    A, b, rows = normal_sums(c["src"], c["ref"][:len(c["src"])], c["normals"][:len(c["src"])])
    assert rows == len(c["src"]) and (np.diag(A)[2:5] == 0).all() and solve(A, b, rows) is None


def test_singular_test_is_explicit():
    rng = np.random.default_rng(0)
    Jm = rng.standard_normal((40, 6))
    x_true = np.array([0.01, -0.02, 0.03, 0.1, -0.2, 0.05])
    A = Jm.T @ Jm
    x = solve(A, -A @ x_true, 40)
    assert x is not None and np.abs(x - x_true).max() < 1e-12
    assert solve(A, -A @ x_true, 5) is None                            # fewer than 6 correspondences
    u = np.array([1e3, 1e3, 1e3, 1e-3, 1e-3, 1e-3])                   # units do not matter: the matrix is scaled first
    xs = solve(A * u[:, None] * u[None], -(A @ x_true) * u, 40)
    assert xs is not None and np.abs(xs * u - x_true).max() < 1e-11
    Jd = Jm.copy(); Jd[:, 5] = Jd[:, 4]                               # rank 5, no zero on the diagonal
    assert solve(Jd.T @ Jd, np.ones(6), 40) is None
    Jz = Jm.copy(); Jz[:, 2] = 0.0                                    # a zero diagonal entry
    assert solve(Jz.T @ Jz, np.ones(6), 40) is None
    An = A.copy(); An[0, 3] = An[3, 0] = np.nan
    assert solve(An, np.ones(6), 40) is None
    R = vec6_to_T(x_true)[:, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15


def test_zero_and_non_finite_normals_contribute_nothing():
    c = surface_case(300, 300, 4)
    s = c["src"].astype(np.float64) @ c["T0"][:, :3].astype(np.float64).T + c["T0"][:, 3]
    t, n = c["ref"].astype(np.float64), c["normals"].astype(np.float64)
    A0, b0, rows0 = normal_sums(s[5:], t[5:], n[5:])
    n2, t2 = n.copy(), t.copy()
    n2[0] = 0.0
    n2[1, 1] = np.nan
    n2[2, 0] = np.inf
    t2[3, 2] = np.nan
    n2[4] = -0.0
    A, b, rows = normal_sums(s, t2, n2)
    assert rows == rows0 == 295 and np.array_equal(A, A0) and np.array_equal(b, b0)


def test_non_finite_source_point_gives_identity_updates():
    c = surface_case(300, 300, 4)
    src = c["src"].copy()
    src[7, 1] = np.nan
    T, fitness, rmse, converged, iters, singular = icp_plane(src, c["ref"], c["normals"], c["T0"], RADIUS)
    assert np.array_equal(T, c["T0"].astype(np.float64)) and singular == iters == 1 and converged and 0 < fitness < 1


# ------------------------------------------------------------------ the pose tolerance of the GPU test, measured
# MEASURED (this test prints the figures): the host rule's own deviation from its unperturbed run when every coordinate of the
# moved points is shifted by -1 / 0 / +1 fp32 ulp after each update, worst over the 3 pairs of a case and 4 hook seeds:
#   (37, 300):          rot 5.024e-08 rad  trans 1.023e-07   fitness 0   rmse 1.9e-07   iterations 0
#   (300, 300):         rot 1.402e-08 rad  trans 2.162e-08   fitness 0   rmse 1.1e-07   iterations 0
#   (1357, 1024):       rot 1.114e-08 rad  trans 1.628e-08   fitness 0   rmse 1.2e-07   iterations 0
#   (2500, 2500) noisy: rot 5.581e-09 rad  trans 1.472e-08   fitness 0   rmse 3.7e-09   iterations 0
# POSE_TOL (rad and length units alike) = 4 x the largest pose deviation, as the issue sets it: 4.1e-07.  The factor covers the
# device's fp32 transform application, which the hook models only in the last bit.
ULP_DEVIATION = {(37, 300): (5.03e-08, 1.024e-07), (300, 300): (1.41e-08, 2.17e-08), (1357, 1024): (1.12e-08, 1.63e-08),
                 (2500, 2500): (5.59e-09, 1.48e-08)}
POSE_TOL = 4 * max(max(v) for v in ULP_DEVIATION.values())


@pytest.mark.parametrize("J,K,noise,seeds", CASES)
def test_host_rule_spread_under_ulp_moves(J, K, noise, seeds):
    """Measures the figures above; asserts that they are not exceeded (so POSE_TOL stays 4 x the worst deviation)."""
    sp = np.zeros(5)
    for seed in seeds:
        c = surface_case(J, K, seed, noise)
        T, f, e, conv, it, _ = host_result(J, K, seed, noise)
        for u in ULP_SEEDS:
            Tp, fp, ep, cp, itp, _ = icp_plane(c["src"], c["ref"], c["normals"], c["T0"], RADIUS, perturb_ulps=u)
            sp = np.maximum(sp, [*pose_err(Tp, T), abs(fp - f), abs(ep - e), abs(itp - it)])
    print(f"SPREAD J={J} K={K}: rot {sp[0]:.3e} trans {sp[1]:.3e} fitness {sp[2]:.1e} rmse {sp[3]:.1e} iterations {int(sp[4])}")
    rot, trans = ULP_DEVIATION[(J, K)]
    assert sp[0] <= rot and sp[1] <= trans, sp


# ------------------------------------------------------------------ the C ABI
def test_header_declares_and_library_exports_icp_refine_ex():
    from deepsir_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsir.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+dsir_icp_refine_ex\s*\(([^)]*)\)", txt)
    assert m, "include/dsir.h does not declare dsir_icp_refine_ex"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 16 and args[13] == "int estimator" and args[14] == "const float* normals_ref" and args[15] == "double* stats"
    assert "dsir_icp_refine_ex" in _lib.SYMBOLS and len(_lib.SYMBOLS["dsir_icp_refine_ex"][1]) == 16
    assert os.path.exists(_lib.LIB_PATH), "build it first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = _lib.load()
    assert hasattr(lib, "dsir_icp_refine_ex") and hasattr(lib, "dsir_icp_refine")
    # no context: an error code, not an abort
    assert lib.dsir_icp_refine_ex(None, None, None, 1, 1, 1, 3, ctypes.c_float(0.1), 1, ctypes.c_float(1e-6), ctypes.c_float(1e-6),
                                  None, None, 1, None, None) != 0


def test_host_only_icp_plane_check(tmp_path):
    """csrc/icp_plane.h (the LDL^T solve, the singularity test, the scratch sizes) compiles as plain host C++; its stand-alone
    check (tools/icp_plane_check.cpp; the sanitizer command is in its header) passes."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "icp_plane_check")
    r = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "deepsir_amd", "csrc"),
                        os.path.join(ROOT, "tools", "icp_plane_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "icp_plane: " in r.stdout, r.stdout + r.stderr
