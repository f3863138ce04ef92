"""The robust loss kernels of the ICP estimators on the host (tests/icp_robust_host.py restates csrc/icp_robust.h and the head of
csrc/icp.hip), the C-ABI declaration of dsir_icp_refine_ex4 and the stand-alone check of the header.  No GPU.  The outlier cases,
the kernel scales and the plane pose tolerance of tests/test_gpu_icp_robust.py are chosen and measured here.

The outlier case: a ``test_icp_plane.surface_case`` with SHARE = 20 % of its source points displaced by ONE common offset
OFFSET = (0, 0, 0.095) (in the reference frame; inside the radius 0.1).  The least-squares minimum is then shifted by about
SHARE x |OFFSET| = 0.019; under tukey with k = 0.08 < |OFFSET| the displaced points weigh nothing at the truth, which stays the
minimum.  The offset is along z because three quarters of the surface have normals close to z: the plane residual of a displaced
point is then about |OFFSET| too, so the same k serves both estimators.
Seeds: (300, 300) and (1357, 1024) keep the seeds of tests/test_icp_plane.py.  (37, 300) - 37 source points, 7 of them displaced, on
a reference of 300 whose spacing is about the radius - takes (13, 53, 63): of the seeds 3, 13, .. 93 the first three on which the
HOST rule converges within max_iter under every kernel and estimator (on the others the 30 host updates do not settle, and a pose
that has not settled cannot be compared within a rounding tolerance).  The device played no part in the choice.

MEASURED on the host rule (test_outliers_shift_l2_and_not_tukey prints them): pose error against T_gt, max(rad, length), l2 / tukey
  point  (37, 300): 1.99e-02 / 9.45e-04, 2.10e-02 / 2.84e-03, 2.01e-02 / 9.70e-04   (300, 300): 1.47e-02 / 4.39e-04, 1.55e-02 / 9.65e-04,
         1.84e-02 / 5.29e-04   (1357, 1024): 9.19e-03 / 2.17e-04, 1.07e-02 / 3.77e-04, 1.07e-02 / 4.54e-04
  plane  (37, 300): 1.09e-01 / 6.43e-03, 1.02e-02 / 4.27e-04, 3.88e-02 / 3.89e-04   (300, 300): 1.56e-02 / 9.63e-04, 3.40e-02 / 2.28e-03,
         3.18e-02 / 6.09e-04   (1357, 1024): 1.49e-02 / 3.29e-04, 1.73e-02 / 7.78e-04, 1.66e-02 / 4.62e-04
The smallest ratio is 7.4 (asserted: at least 5).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import icp_plane_host
import icp_robust_host as H
from oracle.icp import icp as oracle_icp
from test_icp_plane import RADIUS, pose_err, surface_case

SHARE, OFFSET = 0.2, (0.0, 0.0, 0.095)
# the scales of the GPU tests.  tukey: below |OFFSET| (above); huber and cauchy: a third of the radius, so both branches of huber
# occur from T0 on; gm: open3d's GMLoss weighs k / (k + q)^2 with q a SQUARED length, so its k is one too - (0.07)^2 rounded
SCALES = {"huber": 0.03, "cauchy": 0.03, "gm": 0.005, "tukey": 0.08}
SHAPES = [(37, 300, (13, 53, 63)), (300, 300, (4, 14, 24)), (1357, 1024, (9, 19, 29))]
ULP_SEEDS = (1, 2, 3, 4)

_CASES, _HOST = {}, {}


def robust_case(J, K, seed, outliers):
    key = (J, K, seed, outliers)
    if key not in _CASES:
        c = surface_case(J, K, seed)
        _CASES[key] = H.outlier_case(c, SHARE, OFFSET, seed) if outliers else c
    return _CASES[key]


def host_result(J, K, seed, outliers, estimator, kernel, **kw):
    """the host rule on a case, computed once per (case, arguments) -> (T, fitness, rmse, converged, iterations, identity updates)"""
    key = (J, K, seed, outliers, estimator, kernel, tuple(sorted(kw.items())))
    if key not in _HOST:
        c = robust_case(J, K, seed, outliers)
        k = SCALES.get(kernel)
        if estimator == "point":
            _HOST[key] = H.icp_point(c["src"], c["ref"], c["T0"], RADIUS, kernel, k, **kw)
        else:
            _HOST[key] = H.icp_plane(c["src"], c["ref"], c["normals"], c["T0"], RADIUS, kernel, k, **kw)
    return _HOST[key]


# ------------------------------------------------------------------ the weights
def test_weights_at_their_corners():
    for k in (1e-6, 0.03, 0.08, 1.0):
        k = float(np.float32(k))
        kk = k * k
        q = np.array([0.0, np.nextafter(kk, 0.0), kk, np.nextafter(kk, np.inf), 4 * kk, 5e-324, 1e300, np.inf])   # ascending but [5]
        hu, ca, gm, tu = (H.weight(n, q, k) for n in ("huber", "cauchy", "gm", "tukey"))
        assert hu[0] == hu[1] == hu[2] == 1.0 and 1.0 - 1e-15 < hu[3] <= 1.0 and abs(hu[4] - 0.5) < 1e-15 and hu[7] == 0.0
        assert tu[0] == 1.0 and 0.0 <= tu[1] < 1e-30 and tu[2] == tu[3] == tu[4] == tu[6] == tu[7] == 0.0
        assert ca[0] == 1.0 and ca[2] == 0.5 and ca[7] == 0.0 and gm[0] == k / (k * k) and gm[6] == 0.0
        for w in (hu, ca, gm, tu):
            assert (np.diff(w[[5, 0, 1, 2, 3, 4, 6, 7]]) <= 0).all() and (w >= 0).all() and np.isfinite(w).all() and w[5] == w[0]
        assert (H.weight("l2", q, k) == 1.0).all()
        assert not (H.weight("huber", np.nan, k) > 0) and not (H.weight("tukey", np.nan, k) > 0)


def test_l2_of_this_file_is_the_existing_host_rules():
    """kernel l2 here against oracle.icp.icp and icp_plane_host.icp_plane: the same iterations and statistics; the poses agree to
    float64 rounding (the weighted Kabsch normalises by the sum, the oracle takes means)"""
    J, K, seed = 300, 300, 4
    c = surface_case(J, K, seed)
    a, b = host_result(J, K, seed, False, "point", "l2"), oracle_icp(c["src"], c["ref"], c["T0"], RADIUS)
    assert a[1:5] == b[1:5] and a[5] == 0 and max(pose_err(a[0], b[0])) < 1e-12
    a, b = host_result(J, K, seed, False, "plane", "l2"), icp_plane_host.icp_plane(c["src"], c["ref"], c["normals"], c["T0"], RADIUS)
    assert a[1:] == b[1:] and max(pose_err(a[0], b[0])) < 1e-12


# ------------------------------------------------------------------ the feature does something
@pytest.mark.parametrize("J,K,seeds", SHAPES)
def test_outliers_shift_l2_and_not_tukey(J, K, seeds):
    """both estimators: the host rule's pose error against T_gt under l2 is at least 5 times its error under tukey"""
    for seed in seeds:
        c = robust_case(J, K, seed, True)
        for est in ("point", "plane"):
            e_l2 = max(pose_err(host_result(J, K, seed, True, est, "l2")[0], c["T_gt"]))
            r = host_result(J, K, seed, True, est, "tukey")
            e_tk = max(pose_err(r[0], c["T_gt"]))
            print(f"OUTLIERS J={J} K={K} seed={seed} {est}: l2 {e_l2:.2e} tukey {e_tk:.2e} ratio {e_l2 / e_tk:.1f} ({r[4]} updates)")
            assert r[3] and r[5] == 0
            assert e_l2 >= 5.0 * e_tk, (est, seed, e_l2, e_tk)


@pytest.mark.parametrize("J,K,seeds", SHAPES)
def test_host_rule_settles_under_every_kernel(J, K, seeds):
    """what the choice of the seeds rests on: converged before max_iter, no identity update, clean and outlier variant alike"""
    for seed in seeds:
        for outliers in (False, True):
            for est in ("point", "plane"):
                for kernel in SCALES:
                    r = host_result(J, K, seed, outliers, est, kernel)
                    assert r[3] and r[4] < 30 and r[5] == 0, (seed, outliers, est, kernel, r[1:])


# ------------------------------------------------------------------ exact identities
def test_huber_beyond_the_radius_is_l2():
    """k = 2 x max_corr_dist: every weight is exactly 1.0, so T and the stats are l2's, bit for bit"""
    J, K, seed = 300, 300, 14
    c = robust_case(J, K, seed, True)
    ws = []
    a = H.icp_point(c["src"], c["ref"], c["T0"], RADIUS, "huber", 2 * RADIUS, weights=ws)
    b = host_result(J, K, seed, True, "point", "l2")
    assert all((w == np.float32(1.0)).all() for w in ws) and len(ws) == a[4]
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    a = H.icp_plane(c["src"], c["ref"], c["normals"], c["T0"], RADIUS, "huber", 2 * RADIUS)
    b = host_result(J, K, seed, True, "plane", "l2")
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def test_tukey_with_a_tiny_scale_is_the_identity_update():
    """k = 1e-6 on a noisy case: every weight is 0, every update the identity (counted), T_init comes back"""
    c = surface_case(300, 300, 4, 0.004)
    for max_iter in (30, 3):
        ws = []
        T, fitness, rmse, converged, iters, identity = H.icp_point(c["src"], c["ref"], c["T0"], RADIUS, "tukey", 1e-6, max_iter=max_iter, weights=ws)
        assert all((w == 0).all() for w in ws) and fitness > 0.5
        assert np.array_equal(T, c["T0"].astype(np.float64)) and identity == iters == 1 and converged
        T, fitness, rmse, converged, iters, identity = H.icp_plane(c["src"], c["ref"], c["normals"], c["T0"], RADIUS, "tukey", 1e-6, max_iter=max_iter)
        assert np.array_equal(T, c["T0"].astype(np.float64)) and identity == iters == 1 and converged and fitness > 0.5


def test_weight_zero_rows_are_not_counted():
    c = robust_case(300, 300, 4, True)
    s = c["src"].astype(np.float64) @ c["T_gt"][:, :3].T + c["T_gt"][:, 3]
    idx, _ = H._nearest(s.astype(np.float32), c["ref"])
    t, n = c["ref"].astype(np.float64)[idx], c["normals"].astype(np.float64)[idx]
    A, b, rows = H.weighted_normal_sums(s, t, n, "tukey", 0.08)
    A2, b2, rows2 = icp_plane_host.normal_sums(s, t, n)
    assert rows2 == 300 and 200 <= rows < 300                          # the displaced points (60) weigh nothing at the truth
    A1, b1, rows1 = H.weighted_normal_sums(s, t, n, "huber", 10.0)     # all weights 1: the unweighted sums
    assert rows1 == 300 and np.array_equal(A1, A2) and np.array_equal(b1, b2)


# ------------------------------------------------------------------ the plane pose tolerance of the GPU test, measured
# MEASURED (this test prints the figures): the robust host rule's own deviation from its unperturbed run when every coordinate of
# the moved points is shifted by -1 / 0 / +1 fp32 ulp after each update - worst over the 3 pairs of a shape, clean and outlier
# variant, the four kernels at SCALES and 4 hook seeds, plane estimator:
#   (37, 300):     rot 6.325e-08 rad  trans 1.246e-07   fitness 0   rmse 2.0e-07   iterations 0   (seed 13, outliers, huber)
#   (300, 300):    rot 2.603e-08 rad  trans 3.769e-08   fitness 0   rmse 1.2e-07   iterations 0   (seed 24, outliers, gm)
#   (1357, 1024):  rot 1.793e-08 rad  trans 3.248e-08   fitness 0   rmse 1.3e-07   iterations 1   (seed 19, outliers, gm)
# The iteration count moves by one under the hook in one (1357, 1024) run: the GPU test allows that one there, and prints both.
ULP_DEVIATION = {(37, 300): (6.33e-08, 1.247e-07), (300, 300): (2.61e-08, 3.77e-08), (1357, 1024): (1.80e-08, 3.25e-08)}
# PLANE_POSE_TOL (rad and length units alike) = 4 x the largest deviation, as the issue sets it: 5.0e-07.  The point estimator keeps
# the 2e-5 of tests/test_icp.py.
PLANE_POSE_TOL = 4 * max(max(v) for v in ULP_DEVIATION.values())
POINT_POSE_TOL = 2e-5


@pytest.mark.parametrize("J,K,seeds", SHAPES)
def test_robust_plane_rule_spread_under_ulp_moves(J, K, seeds):
    """Measures the figures above; asserts that they are not exceeded (so PLANE_POSE_TOL stays 4 x the worst deviation)."""
    sp = np.zeros(5)
    worst = None
    for seed in seeds:
        for outliers in (False, True):
            c = robust_case(J, K, seed, outliers)
            for kernel, k in SCALES.items():
                T, f, e, conv, it, _ = host_result(J, K, seed, outliers, "plane", kernel)
                for u in ULP_SEEDS:
                    Tp, fp, ep, cp, itp, _ = H.icp_plane(c["src"], c["ref"], c["normals"], c["T0"], RADIUS, kernel, k, perturb_ulps=u)
                    d = [*pose_err(Tp, T), abs(fp - f), abs(ep - e), abs(itp - it)]
                    if max(d[:2]) > max(sp[:2]):
                        worst = (seed, outliers, kernel, u)
                    sp = np.maximum(sp, d)
    print(f"SPREAD J={J} K={K}: rot {sp[0]:.3e} trans {sp[1]:.3e} fitness {sp[2]:.1e} rmse {sp[3]:.1e} iterations {int(sp[4])} at {worst}")
    rot, trans = ULP_DEVIATION[(J, K)]
    assert sp[0] <= rot and sp[1] <= trans, sp


# ------------------------------------------------------------------ coarse to fine: a start outside the fine radius's basin
C2F_RADII = (0.4, 0.05)
C2F_SHIFT = (0.12, 0.1, -0.1)


def c2f_case():
    """surface_case(1357, 1024, 9) started C2F_SHIFT further off than its T0 -> (case, T_start [3,4] f32).  MEASURED on the host
    point-to-point rule: the fine radius alone ends 0.79 from T_gt (17 updates, fitness 0.08), coarse then fine 3.6e-08."""
    c = surface_case(1357, 1024, 9)
    T = c["T0"].astype(np.float64).copy()
    T[:, 3] += C2F_SHIFT
    return c, T.astype(np.float32)


def test_coarse_to_fine_start_is_outside_the_fine_basin():
    c, T_start = c2f_case()
    fine = H.icp_point(c["src"], c["ref"], T_start, C2F_RADII[1])
    coarse = H.icp_point(c["src"], c["ref"], T_start, C2F_RADII[0])
    both = H.icp_point(c["src"], c["ref"], coarse[0].astype(np.float32), C2F_RADII[1])
    e_fine, e_both = max(pose_err(fine[0], c["T_gt"])), max(pose_err(both[0], c["T_gt"]))
    print(f"C2F host: fine alone {e_fine:.2e} ({fine[4]} updates, fitness {fine[1]:.2f}), coarse then fine {e_both:.2e}")
    assert e_fine > 10 * POINT_POSE_TOL and e_both < POINT_POSE_TOL


# ------------------------------------------------------------------ the C ABI and the header
def test_header_declares_and_library_exports_icp_refine_ex4():
    from deepsir_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsir.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+dsir_icp_refine_ex4\s*\(([^)]*)\)", txt)
    assert m, "include/dsir.h does not declare dsir_icp_refine_ex4"
    args = [a.strip() for a in m.group(1).split(",")]
    m3 = re.search(r"\bint\s+dsir_icp_refine_ex3\s*\(([^)]*)\)", txt)
    assert args[:-2] == [a.strip() for a in m3.group(1).split(",")] and args[-2:] == ["int kernel", "float kernel_scale"]
    assert len(_lib.SYMBOLS["dsir_icp_refine_ex4"][1]) == len(args) == 21
    for name, value in (("L2", 0), ("HUBER", 1), ("CAUCHY", 2), ("GM", 3), ("TUKEY", 4)):
        assert re.search(rf"#define\s+DSIR_ICP_{name}\s+{value}\b", txt)
    from deepsir_amd.engine import ICP_KERNELS
    assert ICP_KERNELS == H.KERNELS == {"l2": 0, "huber": 1, "cauchy": 2, "gm": 3, "tukey": 4}
    assert os.path.exists(_lib.LIB_PATH), "build it first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = _lib.load()
    assert hasattr(lib, "dsir_icp_refine_ex4")
    # no context: an error code, not an abort
    assert lib.dsir_icp_refine_ex4(None, None, None, 1, 1, 1, 3, ctypes.c_float(0.1), 1, ctypes.c_float(1e-6), ctypes.c_float(1e-6),
                                   None, None, 0, None, 0, None, None, None, 4, ctypes.c_float(0.05)) != 0


def test_python_refuses_bad_kernel_arguments():
    from deepsir_amd.engine import icp_kernel_args
    assert icp_kernel_args("l2", None) == (0, 0.0) and icp_kernel_args("l2", float("nan")) == (0, 0.0)
    assert icp_kernel_args("tukey", 0.08) == (4, float(np.float32(0.08))) and icp_kernel_args("huber", 1) == (1, 1.0)
    for kernel, scale in (("l1", 0.1), (None, 0.1), (4, 0.1), ("tukey", None), ("tukey", 0.0), ("huber", -1.0), ("cauchy", float("nan")),
                          ("gm", float("inf")), ("gm", 1e39), ("tukey", 1e-50), ("huber", "wide")):
        with pytest.raises(ValueError):
            icp_kernel_args(kernel, scale)


def test_host_only_icp_robust_check(tmp_path):
    """csrc/icp_robust.h compiles as plain host C++; its stand-alone check (tools/icp_robust_check.cpp; the sanitizer command is in
    its header) passes."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "icp_robust_check")
    r = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "deepsir_amd", "csrc"),
                        os.path.join(ROOT, "tools", "icp_robust_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "icp_robust: " in r.stdout, r.stdout + r.stderr
