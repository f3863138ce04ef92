"""The NDT rule on the host (deepsir_amd/ndt.py restates csrc/ndt.hip's header), the C-ABI declarations of dsir_ndt_refine /
dsir_ndt_map and the host-only check of csrc/ndt.h.  No GPU.  The tolerances of tests/test_gpu_ndt.py are measured here.

Pose bar.  tests/test_icp_plane.py holds its own host rule to 1e-5 on noise-free clouds and to 5e-3 on noisy ones.  NDT fits
Gaussians of cell size, not points: on these clouds the truth is not a stationary point of its score (a cell's points are weighted
by their own likelihood), and the rule ends 1e-4 .. 2e-3 from it at a cell edge of 0.2 whether the cloud is noisy or not.  The bar
asserted here is that file's 5e-3, on the shapes with enough points per cell (1357 / 1024 and 2500 / 2500); the 1e-5 bar is NOT met
and is not claimed.  The sparse shapes (37 / 300, 300 / 300: 10 .. 15 valid cells) serve the device-against-host tests only.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from deepsir_amd.ndt import (KEY_NONE, MAXC, cell_key, inverse_covariance, ndt_constants, ndt_lattice_host, ndt_map_host, ndt_refine_host,
                             ndt_step_host)
from icp_plane_host import icp_plane
from ndt_cases import CAP_ITERS, NEIGHBORS, REFINE_CASES, RES, STEP_TOL, ULP_SEEDS, clear_of_thresholds, host_refine, map_cloud
from test_icp_plane import RADIUS, _rodrigues, pose_err, surface_case

POSE_BAR = 5e-3            # tests/test_icp_plane.py test_host_rule_converges_with_noise


# ------------------------------------------------------------------ constants
@pytest.mark.parametrize("res", [1.0, 0.3])
def test_constants_closed_form(res):
    d1, d2, d3 = ndt_constants(0.55, res)
    r = float(np.float32(res))
    c1, c2 = 4.5, 0.55 / r ** 3
    assert abs(d3 + np.log(c2)) < 1e-15 and abs(d1 - (np.log(c2) - np.log(c1 + c2))) < 1e-14
    # what defines them: the Gaussian d1 exp(-d2 q / 2) + d3 meets -log(c1 exp(-q / 2) + c2) at q = 0 and q = 1
    assert abs(d1 + d3 + np.log(c1 + c2)) < 1e-14
    assert abs(d1 * np.exp(-d2 / 2) + d3 + np.log(c1 * np.exp(-0.5) + c2)) < 1e-13
    assert d1 < 0 < d2
    if res == 1.0:
        assert abs(d3 - 0.5978370007556204) < 1e-15 and abs(d1 - np.log(0.55 / 5.05)) < 1e-14      # -log(0.55), log(0.55 / 5.05)


# ------------------------------------------------------------------ the map of a hand-made cloud
def _hand_cloud():
    rng = np.random.default_rng(0)
    blob = lambda cell, n: (np.array(cell) + 0.5) + rng.uniform(-0.3, 0.3, (n, 3))
    five, six, seven = blob((0, 0, 0), 5), blob((2, 0, 0), 6), blob((0, 2, 0), 7)
    flat = blob((0, 0, 2), 9)
    flat[:, 2] = 2.5                                                     # coplanar: the smallest eigenvalue is 0
    same = np.tile(np.array([[2.5, 2.5, 0.5]]), (6, 1))                  # six identical points
    bad = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5]])
    corner = np.array([[0.0, 0.0, 0.0], [3.0, 3.0, 3.0]])                # fix the origin at 0
    return np.concatenate([five, six, seven, flat, same, bad, corner]).astype(np.float32)


def _record_of(m, cell):
    k = cell_key(np.array(cell))
    p = int(np.searchsorted(m["keys"], k))
    assert m["keys"][p] == k
    return p, m["records"][p]


def test_map_of_hand_made_cloud():
    ref = _hand_cloud()
    m = ndt_map_host(ref, 1.0)
    assert np.array_equal(m["origin"], np.zeros(3)) and m["h"] == 1.0
    assert (m["keys"][-2:] == KEY_NONE).all() and (m["keys"][:-2] != KEY_NONE).all()      # the two non-finite rows: last, in no cell
    assert sorted(m["index"][-2:].tolist()) == [33, 34] and np.array_equal(np.sort(m["index"]), np.arange(len(ref)))
    assert (np.diff(m["keys"].astype(np.float64)) >= 0).all()
    p5, r5 = _record_of(m, (0, 0, 0))
    assert m["runs"][p5] == 6 and r5[9] == 6                             # 5 points and the corner point at the origin: valid
    _, r6 = _record_of(m, (2, 0, 0))
    _, r7 = _record_of(m, (0, 2, 0))
    assert r6[9] == 6 and r7[9] == 7
    pf, rf = _record_of(m, (0, 0, 2))
    assert rf[9] == 9 and m["lam"][pf][2] == 0.01 * m["lam"][pf][0] and m["lam"][pf][1] > m["lam"][pf][2]   # the floor, exactly
    ps, rs = _record_of(m, (2, 2, 0))
    assert m["runs"][ps] == 6 and not rs.any()                           # six identical points: lambda_1 = 0, invalid
    # a run's rows stand in ascending original index, records stand at run heads only
    for p in np.flatnonzero(m["runs"]):
        idx = m["index"][p:p + m["runs"][p]]
        assert (np.diff(idx) > 0).all()
    assert not m["records"][m["runs"] == 0].any()
    # the mean and B of a valid cell against a plain statement
    x = ref[m["index"][pf:pf + 9]].astype(np.float64)
    assert np.allclose(rf[:3], x.mean(0), rtol=0, atol=1e-15)
    lam, V = np.linalg.eigh(np.cov(x.T))
    Bfull = (V / np.maximum(lam, 0.01 * lam.max())) @ V.T
    assert np.allclose([rf[3], rf[4], rf[5], rf[6], rf[7], rf[8]], Bfull[np.triu_indices(3)], rtol=1e-9)


def test_cells_of_5_6_7_points():
    rng = np.random.default_rng(1)
    for n, valid in ((5, False), (6, True), (7, True)):
        ref = np.concatenate([rng.uniform(0.1, 0.9, (n, 3)), [[0, 0, 0]], [[5.5, 5.5, 5.5]]]).astype(np.float32)
        ref[n] = [-1.0, -1.0, -1.0]                                      # the origin's own cell holds one point
        m = ndt_map_host(ref, 1.0)
        p, r = _record_of(m, (1, 1, 1))
        assert m["runs"][p] == n and (r[9] == n) == valid and r.any() == valid
    assert inverse_covariance(np.zeros(6)) == (None, None)
    assert inverse_covariance(np.array([np.inf, 0, 0, 1, 0, 1]))[0] is None


def test_far_point_coarsens_the_edge():
    ref = np.concatenate([np.random.default_rng(2).uniform(0, 1, (20, 3)), [[3.0e6, 0.5, 0.5]]]).astype(np.float32)
    o, h = ndt_lattice_host(ref, 1.0)
    ext = float(ref[:, 0].max()) - float(ref[:, 0].min())
    assert ext / 2 ** 20 > 1.0 and h == ext / 1048576.0
    m = ndt_map_host(ref, 1.0)
    assert m["h"] == h and int(m["keys"][-1] & np.uint64(MAXC)) == 2 ** 20 and m["keys"][-1] != KEY_NONE
    assert m["runs"][0] == 20 and m["records"][0, 9] == 20               # the unit cube is one cell now
    o0, h0 = ndt_lattice_host(np.full((3, 3), np.nan, np.float32), 0.25)
    assert not o0.any() and h0 == 0.25 and not ndt_map_host(np.full((3, 3), np.nan, np.float32), 0.25)["runs"].any()


def test_map_cloud_generator_keeps_the_condition_number():
    for K in (300, 2500):
        m = ndt_map_host(map_cloud(K, 7), 0.25)
        lam = m["lam"][m["records"][:, 9] > 0]
        assert len(lam) > 5 and (lam[:, 0] / lam[:, 2] <= 100.0 * (1 + 1e-12)).all()
        n = m["runs"][m["runs"] > 0]
        assert (n < 6).any() and (n == 6).any() and (n > 6).any()


# ------------------------------------------------------------------ one step
def test_step_identity_cases_and_out_of_lattice_points():
    c = surface_case(300, 300, 4)
    m = ndt_map_host(c["ref"], RES)
    d2 = ndt_constants(0.55, RES)[1]
    cur = (c["src"].astype(np.float64) @ c["T_gt"][:, :3].T + c["T_gt"][:, 3]).astype(np.float32)
    st = ndt_step_host(cur, m, d2)
    assert st["x"] is not None and st["bad"] == 0 and st["matched"] > 100 and st["rows"] >= st["matched"]
    assert np.abs(st["A"] - st["A"].T).max() == 0 and np.linalg.eigvalsh(st["A"]).min() > -1e-9 * np.abs(st["A"]).max()
    assert ndt_step_host(cur, m, d2, neighbors=1)["rows"] <= st["rows"]
    bad = cur.copy(); bad[7, 1] = np.nan
    sb = ndt_step_host(bad, m, d2)
    assert sb["bad"] == 1 and sb["x"] is None                           # a non-finite moved point: the identity update
    assert ndt_step_host(cur[:0], m, d2)["x"] is None and ndt_step_host(cur, ndt_map_host(c["ref"][:0], RES), d2)["x"] is None
    # a point one cell outside the lattice has no own cell and still visits its in-range face neighbour
    o, h = m["origin"], m["h"]
    inside = cur[np.flatnonzero(np.floor((cur[:, 0].astype(np.float64) - o[0]) / h) == 0)[:1]]
    if len(inside):
        out = inside.copy(); out[0, 0] = np.float32(o[0] - 0.25 * h)
        s7, s1 = ndt_step_host(out, m, d2, 7), ndt_step_host(out, m, d2, 1)
        assert s1["rows"] == 0 and s7["rows"] <= 1
    far = np.array([[1e30, 0, 0], [-1e30, 0, 0], [0, 1e30, 0], [0, 0, -1e30]], np.float32)
    assert ndt_step_host(far, m, d2)["rows"] == 0 and ndt_step_host(far, m, d2)["bad"] == 0


# ------------------------------------------------------------------ the loop
@pytest.mark.parametrize("J,K,noise,seeds", [c for c in REFINE_CASES if c[0] >= 1000])
def test_host_rule_recovers_the_pose(J, K, noise, seeds):
    """from the 3 degrees / 0.05 per axis offset of surface_case, to the 5e-3 bar (the module's docstring says why not 1e-5)"""
    for seed in seeds:
        c = surface_case(J, K, seed, noise)
        T, st, trace = host_refine(J, K, seed, noise, 7, 30)
        er, et = pose_err(T, c["T_gt"])
        e0 = pose_err(c["T0"], c["T_gt"])
        print(f"NDT HOST J={J} K={K} seed={seed}: {int(st[3])} iterations, likelihood {st[0]:.3f} matched {st[1]:.3f}, error {er:.1e} rad "
              f"{et:.1e} (from {e0[0]:.1e} rad {e0[1]:.1e})")
        assert st[2] == 1 and st[3] <= 30 and st[4] == 0
        assert er < POSE_BAR and et < POSE_BAR


def test_refine_edge_rules():
    c = surface_case(300, 300, 4)
    T0 = c["T0"]
    T, st, _ = ndt_refine_host(c["src"], c["ref"], T0, RES, max_iter=0)
    assert np.array_equal(T, T0) and st[2] == 0 and st[3] == 0 and st[4] == 0 and st[0] > 0
    src = c["src"].copy(); src[7, 1] = np.nan
    T, st, tr = ndt_refine_host(src, c["ref"], T0, RES)
    assert np.array_equal(T, T0) and list(st[2:]) == [1, 1, 1] and tr == [None]
    T, st, _ = ndt_refine_host(c["src"], c["ref"][:5], T0, RES)          # no valid cell
    assert np.array_equal(T, T0) and list(st) == [0, 0, 1, 1, 1]
    T, st, _ = ndt_refine_host(c["src"][:0], c["ref"], T0, RES)          # Jp = 0
    assert np.array_equal(T, T0) and list(st) == [0, 0, 1, 1, 1]
    ref = c["ref"].copy(); ref[3] = np.nan
    Ta, sa, _ = ndt_refine_host(c["src"], ref, T0, RES)
    Tb, sb, _ = ndt_refine_host(c["src"], np.delete(c["ref"], 3, 0), T0, RES)
    assert np.array_equal(Ta, Tb) and np.array_equal(sa, sb)             # a non-finite reference row is ignored


# MEASURED (printed by test_ndt_wider_basin_than_point_to_plane): surface_case(1357, 1024, seed 101) from 30 degrees about a seeded axis
# and 0.40 off the truth - point-to-plane (radius 0.1) ends 1.7e+00 rad 3.0e+00 from the truth, NDT coarse to fine (0.6 then 0.2)
# 8.2e-04 rad 2.0e-03.  Single-scale NDT at 0.2 fails from there too (2.7e-02 rad 3.0e-01): the basin table is in profiles/README.md.
BASIN_SEED, BASIN_DEG, BASIN_SHIFT = 101, 30.0, 0.40


def basin_T0(c, seed, deg, shift):
    rng = np.random.default_rng(1000 + seed)
    R, t = c["T_gt"][:, :3], c["T_gt"][:, 3]
    dR = _rodrigues(rng.standard_normal(3), np.deg2rad(deg))
    dt = rng.standard_normal(3)
    dt *= shift / np.linalg.norm(dt)
    return np.hstack([dR @ R, (dR @ t + dt)[:, None]]).astype(np.float32)


def test_ndt_wider_basin_than_point_to_plane():
    """an offset at which the host point-to-plane rule ends further from the truth than NDT does: both printed, NDT's asserted"""
    c = surface_case(1357, 1024, BASIN_SEED)
    T0 = basin_T0(c, BASIN_SEED, BASIN_DEG, BASIN_SHIFT)
    Ta, _, _ = ndt_refine_host(c["src"], c["ref"], T0, 0.6)
    Tn, st, _ = ndt_refine_host(c["src"], c["ref"], Ta, 0.2)
    Tp = icp_plane(c["src"], c["ref"], c["normals"], T0, RADIUS)[0]
    en, ep = pose_err(Tn, c["T_gt"]), pose_err(Tp, c["T_gt"])
    print(f"BASIN seed {BASIN_SEED} from {BASIN_DEG} deg {BASIN_SHIFT}: point-to-plane {ep[0]:.1e} rad {ep[1]:.1e}, NDT 0.6 -> 0.2 {en[0]:.1e} rad {en[1]:.1e}")
    assert en[0] < POSE_BAR and en[1] < POSE_BAR


# ------------------------------------------------------------------ the tolerances of the GPU test, measured
# MEASURED (test_host_rule_spread_under_ulp_moves prints the figures): the host rule's own deviation from its unperturbed run when
# every coordinate of the moved points is shifted by -1 / 0 / +1 fp32 ulp after T_init is applied and after each update; worst over
# the 3 pairs of a case, neighbors 7 and 1, the capped (6 iterations) and the converged run, and 4 draws:
#   (37, 300):     rot 1.354e-06 rad  trans 1.684e-06   likelihood 7.5e-07   iterations 0
#   (300, 300):    rot 3.314e-07 rad  trans 4.064e-07   likelihood 2.4e-07   iterations 0
#   (1357, 1024):  rot 1.445e-07 rad  trans 8.429e-08   likelihood 1.5e-07   iterations 0
#   (2500, 2500):  rot 3.213e-08 rad  trans 1.229e-07   likelihood 8.9e-08   iterations 0
# POSE_TOL (rad and length units alike) and LIKELIHOOD_TOL = 4 x the largest deviation, the convention of tests/test_icp_plane.py.
ULP_DEVIATION = {(37, 300): (1.36e-06, 1.69e-06, 7.6e-07), (300, 300): (3.32e-07, 4.07e-07, 2.4e-07), (1357, 1024): (1.45e-07, 8.5e-08, 1.5e-07),
                 (2500, 2500): (3.3e-08, 1.23e-07, 9.0e-08)}
POSE_TOL = 4 * max(max(v[:2]) for v in ULP_DEVIATION.values())
LIKELIHOOD_TOL = 4 * max(v[2] for v in ULP_DEVIATION.values())


@pytest.mark.parametrize("J,K,noise,seeds", REFINE_CASES)
def test_host_rule_spread_under_ulp_moves(J, K, noise, seeds):
    """Measures the figures above; asserts that they are not exceeded.  Also asserts what the GPU test's equality of iterations
    rests on: every capped run is clear of its thresholds by a factor 10 at every iteration."""
    sp = np.zeros(4)
    for max_iter in (CAP_ITERS, 30):
        for nb in NEIGHBORS:
            for seed in seeds:
                T, st, trace = host_refine(J, K, seed, noise, nb, max_iter)
                if max_iter == CAP_ITERS:
                    assert clear_of_thresholds(trace, 10.0) and st[2] == 0 and st[3] == CAP_ITERS, (seed, nb, trace)
                for u in ULP_SEEDS:
                    Tp, sp_, _ = host_refine(J, K, seed, noise, nb, max_iter, perturb_ulps=u)
                    sp = np.maximum(sp, [*pose_err(Tp, T), abs(float(sp_[0]) - float(st[0])), abs(float(sp_[3]) - float(st[3]))])
    print(f"NDT SPREAD J={J} K={K}: rot {sp[0]:.3e} trans {sp[1]:.3e} likelihood {sp[2]:.1e} iterations {int(sp[3])}")
    rot, trans, lik = ULP_DEVIATION[(J, K)]
    assert sp[0] <= rot and sp[1] <= trans and sp[2] <= lik and sp[3] == 0, sp


# MEASURED (test_inverse_covariance_sensitivity prints it): the largest change of B, relative to max |B|, over the valid cells of the
# GPU test's map clouds when every entry of a cell's C moves by the fp64 summation bound (2n + 2) 2^-53 max |x - mu|^2 in the worst
# of 8 sign patterns: 2.86e-13 (the constant is that figure rounded up).  The GPU test allows 4 x that between svd3's B and eigh's.
B_SENSITIVITY = 3.0e-13
MAP_SHAPES = (5, 6, 300, 1024, 2500)
MAP_RES = 0.25


def test_inverse_covariance_sensitivity():
    worst = 0.0
    rng = np.random.default_rng(0)
    for K in MAP_SHAPES:
        for seed in (1, 2, 3):
            ref = map_cloud(K, 10 * K + seed, MAP_RES)
            m = ndt_map_host(ref, MAP_RES)
            for p in np.flatnonzero(m["records"][:, 9] > 0):
                n = int(m["runs"][p])
                x = ref[m["index"][p:p + n]].astype(np.float64)
                dmax = float(((x - m["records"][p, :3]) ** 2).sum(1).max())
                bound = (2 * n + 2) * 2.0 ** -53 * dmax
                c = m["sums"][p, 3:] / (n - 1)
                B0 = m["records"][p, 3:9]
                for _ in range(8):
                    B1, _ = inverse_covariance(c + rng.choice([-1.0, 1.0], 6) * bound / (n - 1))
                    worst = max(worst, float(np.abs(B1 - B0).max() / np.abs(B0).max()))
    print(f"NDT B SENSITIVITY: {worst:.2e} relative to max |B|")
    assert worst <= B_SENSITIVITY


# ------------------------------------------------------------------ the C ABI and the host-only check
def test_header_declares_and_library_exports_ndt():
    from deepsir_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsir.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+dsir_ndt_refine\s*\(([^)]*)\)", txt)
    assert m, "include/dsir.h does not declare dsir_ndt_refine"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 17 and args[10] == "float resolution" and args[11] == "int neighbors" and args[16] == "float* stats"
    m = re.search(r"\bint\s+dsir_ndt_map\s*\(([^)]*)\)", txt)
    assert m and len(m.group(1).split(",")) == 11
    assert len(_lib.SYMBOLS["dsir_ndt_refine"][1]) == 17 and len(_lib.SYMBOLS["dsir_ndt_map"][1]) == 11
    assert os.path.exists(_lib.LIB_PATH), "build it first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = _lib.load()
    # no context: an error code, not an abort
    assert lib.dsir_ndt_refine(None, None, None, 1, 1, 1, 3, None, None, None, ctypes.c_float(0.3), 7, 1, ctypes.c_float(1e-4),
                               ctypes.c_float(0.55), None, None) != 0
    assert lib.dsir_ndt_map(None, None, 1, 1, 3, None, ctypes.c_float(0.3), None, None, None, None) != 0
    from deepsir_amd.engine import Engine
    assert callable(Engine.ndt_refine) and callable(Engine.ndt_map)


def test_host_only_ndt_check(tmp_path):
    """csrc/ndt.h (lattice, constants, argument checks, layout, the key interval of the x triple) compiles as plain host C++; its
    stand-alone check (tools/ndt_check.cpp; the sanitizer command is in its header) passes."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "ndt_check")
    r = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "deepsir_amd", "csrc"),
                        os.path.join(ROOT, "tools", "ndt_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ndt: " in r.stdout, r.stdout + r.stderr
