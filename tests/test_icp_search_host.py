"""The ICP search rule and the per-pair lattice of the cell index on the host (deepsir_amd/icp.py, csrc/icp_grid.h).  No GPU.
tests/test_gpu_icp_grid.py compares both kernels with `icp_search_host` bit for bit; this file pins `icp_search_host` itself."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from deepsir_amd import icp as I

R = 0.03
BAND = 1e-3          # relative band around r^2 inside which fp32 and fp64 may disagree (tests/test_overlap_host.py)


def surface(n, seed, side=1.7):
    """random samples of a wavy surface: about one point per r x r at n = 3000, so matches and misses mix"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, side, (n, 2))
    return np.c_[xy, 0.1 * np.sin(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1])].astype(np.float32)


def brute64(a, b):
    """float64 brute force -> (nearest index with ties to the lower one, its d2, the second smallest d2)"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    d2 = ((a[:, None, :] - b[None]) ** 2).sum(-1)
    k = np.argmin(d2, 1)
    part = np.partition(d2, 1, axis=1) if d2.shape[1] > 1 else np.c_[d2, np.full(len(a), np.inf)]
    return k, d2[np.arange(len(a)), k], part[:, 1]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_search_host_against_float64(seed):
    a, b = surface(3000, seed), surface(3000, 100 + seed)
    idx, d2 = I.icp_search_host(a, b, R)
    k, best, second = brute64(a, b)
    r2 = R * R
    m64 = best <= r2
    band = np.abs(best - r2) <= BAND * r2
    print(f"seed {seed}: fp64 matches {m64.sum()} of {len(a)}, fp32 {(idx >= 0).sum()}, in band {band.sum()} ({100 * band.mean():.3f} %)")
    assert band.mean() < 0.005                                 # the band cannot hide a wrong rule
    assert 0.2 * len(a) < m64.sum() < 0.95 * len(a)            # both outcomes are exercised
    assert np.array_equal((idx >= 0)[~band], m64[~band])
    sure = m64 & ~band & (second - best > BAND * r2)
    assert sure.sum() > 0.9 * (m64 & ~band).sum()
    assert np.array_equal(idx[sure], k[sure])
    assert np.allclose(d2[sure], best[sure], rtol=1e-4, atol=1e-9) and (d2[idx < 0] == 0).all()
    assert idx.dtype == np.int32 and d2.dtype == np.float32


def test_ties_go_to_the_lower_index():
    rng = np.random.default_rng(7)
    base = rng.uniform(0, 1, (50, 3)).astype(np.float32)
    ref = np.concatenate([base, base[::-1], base])             # every point three times
    idx, d2 = I.icp_search_host(base, ref, 0.1)
    assert np.array_equal(idx, np.arange(50)) and (d2 == 0).all()
    idx, _ = I.icp_search_host(base, ref[50:], 0.1)            # the reversed copy first: its positions win over the third copy's
    assert np.array_equal(idx, 49 - np.arange(50))
    # distinct points at the same distance, exactly (integer coordinates)
    ref = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, 0, -1]], np.float32)
    idx, d2 = I.icp_search_host(np.zeros((1, 3), np.float32), ref, 1.5)
    assert idx[0] == 0 and d2[0] == 1.0
    idx, _ = I.icp_search_host(np.zeros((1, 3), np.float32), ref[::-1].copy(), 1.5)
    assert idx[0] == 0


def test_inclusion_at_exactly_r():
    """points at offset 0.5 along an axis with r = 0.5: d2 == r2 == 0.25 is accepted (`<=`; overlap.py's strict rule refuses it)"""
    q = np.array([[0, 0, 0], [10, 0, 0], [0, 20, 0], [0, 0, 30], [40, 40, 40]], np.float32)
    ref = q + np.array([[0.5, 0, 0], [-0.5, 0, 0], [0, 0.5, 0], [0, 0, -0.5], [0.5, 0.5, 0]], np.float32)
    idx, d2 = I.icp_search_host(q, ref, 0.5)
    assert np.array_equal(idx, [0, 1, 2, 3, -1]) and np.array_equal(d2, np.float32([0.25, 0.25, 0.25, 0.25, 0]))
    from deepsir_amd.overlap import nn_pair_host
    assert (nn_pair_host(q, ref, 0.5) == -1).all()
    idx, _ = I.icp_search_host(q, ref, np.nextafter(np.float32(0.5), np.float32(0)))
    assert (idx == -1).all()


def test_non_finite_rows_match_nothing():
    ref = np.array([[0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [0.01, 0, 0]], np.float32)
    q = np.array([[0.009, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, -np.inf, 0]], np.float32)
    idx, d2 = I.icp_search_host(q, ref, 0.1)
    assert np.array_equal(idx, [3, -1, -1, -1]) and (d2[1:] == 0).all()
    idx, d2 = I.icp_search_host(q, ref[1:3], 0.1)              # no finite reference point
    assert (idx == -1).all() and (d2 == 0).all()


def test_move_and_stats_host():
    rng = np.random.default_rng(3)
    p = rng.uniform(-2, 2, (777, 3)).astype(np.float32)
    eye = np.eye(3, 4, dtype=np.float32)
    assert I.icp_move_host(eye, p).tobytes() == p.tobytes()
    T = eye.copy()
    T[:, 3] = [0.25, -1.5, 3.0]
    assert I.icp_move_host(T, p).tobytes() == (p + T[:, 3]).astype(np.float32).tobytes()
    c, s = np.cos(0.3), np.sin(0.3)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    want = p.astype(np.float64) @ T[:, :3].astype(np.float64).T + T[:, 3]
    assert np.abs(I.icp_move_host(T, p) - want).max() < 1e-6
    idx = np.where(rng.uniform(size=777) < 0.6, 1, -1)
    d2 = np.where(idx >= 0, rng.uniform(0, 1e-2, 777), 0).astype(np.float32)
    st = I.icp_stats_host(idx, d2)
    n = (idx >= 0).sum()
    assert st[0] == n / 777 and abs(st[1] - np.sqrt(d2.astype(np.float64).sum() / n)) < 1e-15
    assert np.array_equal(I.icp_stats_host(np.full(5, -1), np.zeros(5, np.float32)), [0.0, 0.0])


# ---------------------------------------------------------------------- the lattice
def _contained(cur, ref, r):
    """every neighbour the brute rule accepts lies in the 27 cells of its query; -> the number of accepted neighbours"""
    idx, _ = I.icp_search_host(cur, ref, r)
    o, h = I.grid_lattice(ref, r)
    assert h >= float(np.float32(r)) * I.GRID_MARGIN
    fin = np.isfinite(ref).all(1)
    cr = I.grid_cells(ref[fin], o, h)
    assert cr.min() >= 0 and cr.max() <= 1 << 20               # c + 1 fits the 21 bits of a key axis
    keys = I.grid_key(cr)
    assert keys.max() < I.KEY_NONE
    hit = idx >= 0
    cq = I.grid_cells(cur[hit], o, h)
    cn = I.grid_cells(ref[idx[hit]], o, h)
    assert np.abs(cq - cn).max(initial=0) <= 1
    return int(hit.sum())


@pytest.mark.parametrize("seed", [11, 12])
def test_lattice_contains_every_accepted_neighbour_random(seed):
    rng = np.random.default_rng(seed)
    ref = surface(2500, seed)
    cur = (surface(2500, 50 + seed) + rng.normal(0, 0.01, (2500, 3))).astype(np.float32)
    assert _contained(cur, ref, R) > 500
    assert _contained(cur, ref, 0.2) > 2000
    assert _contained(cur, ref, 5.0) == 2500                   # r larger than the cloud: one cell


def test_lattice_contains_points_on_cell_faces():
    r = 0.5
    h = float(np.float32(r)) * I.GRID_MARGIN
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    ref = (g * h).astype(np.float32)                            # on the faces of the cells, up to the rounding to fp32
    cur = np.concatenate([ref + np.float32([r, 0, 0]), ref - np.float32([0, r, 0]), ref + np.float32([0, 0, 1e-7]), ref])
    assert _contained(cur, ref, r) > len(ref)
    ref = (g * 0.25).astype(np.float32)                         # a lattice of r / 2: many pairs at exactly d2 == r2
    cur = np.concatenate([ref + np.float32([r, 0, 0]), ref + np.float32([0, -r, 0])])
    idx, d2 = I.icp_search_host(cur, ref, r)
    assert (d2[idx >= 0] == 0).sum() > 100
    assert _contained(cur, ref, r) > len(ref)
    cur = ref + np.float32([0.375, 0, 0])                       # the next lattice point at exactly 0.125 = r, but for the last x layer
    assert _contained(cur, ref, 0.125) == len(ref) - 32


def test_lattice_coarse_edge_when_the_extent_is_huge():
    rng = np.random.default_rng(5)
    r = 1e-5
    cl = [np.float32(rng.uniform(0, 1000, 3)) + rng.uniform(0, 3e-4, (80, 3)).astype(np.float32) for _ in range(6)]
    ref = np.concatenate(cl + [np.float32([[0, 0, 0], [1000, 1000, 10]])]).astype(np.float32)
    o, h = I.grid_lattice(ref, r)
    assert h == 1000.0 / 2 ** 20 and h > 50 * r                 # the third term of the edge rule, not the radius
    cur = ref[rng.permutation(len(ref))]
    assert _contained(cur, ref, r) == len(ref)
    assert I.grid_cell_edge(1e-30, 0.0) == 2.0 ** -60 and I.grid_cell_edge(0.2, 10.0) == float(np.float32(0.2)) * (1 + 2.0 ** -10)


def test_lattice_coordinates_near_1e5():
    ref = (surface(2000, 21) + np.float32(1e5)).astype(np.float32)
    cur = (surface(2000, 22) + np.float32(1e5)).astype(np.float32)
    assert _contained(cur, ref, 0.05) > 500
    far = (cur - np.float32(3e5)).astype(np.float32)            # moved far outside: clamped cells, no neighbour
    idx, _ = I.icp_search_host(far, ref, 0.05)
    o, h = I.grid_lattice(ref, 0.05)
    assert (idx == -1).all() and (I.grid_cells(far, o, h) == -2).all()


def test_lattice_without_a_finite_reference_point():
    ref = np.full((4, 3), np.nan, np.float32)
    o, h = I.grid_lattice(ref, 0.1)
    assert (o == 0).all() and h == float(np.float32(0.1)) * I.GRID_MARGIN


def test_header_declares_and_library_exports_the_search():
    import re
    from deepsir_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsir.h")).read(), flags=re.S)
    for name, nargs in (("dsir_icp_refine_ex2", 17), ("dsir_icp_correspondences", 13)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert len(_lib.SYMBOLS[name][1]) == nargs and hasattr(_lib.load(), name)
    assert "int search" in re.search(r"dsir_icp_refine_ex2\s*\(([^)]*)\)", txt).group(1)


def test_host_only_icp_grid_check(tmp_path):
    """csrc/icp_grid.h and csrc/cell_index.h compile as plain host C++ and their stand-alone check passes (tools/icp_grid_check.cpp;
    the sanitizer command is in its header)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "icp_grid_check")
    r = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "deepsir_amd", "csrc"),
                        os.path.join(ROOT, "tools", "icp_grid_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "icp_grid: " in r.stdout, r.stdout + r.stderr


def test_host_only_scratch_layout_check(tmp_path):
    """csrc/scratch.h and csrc/op_layouts.h compile as plain host C++ and their stand-alone check passes (tools/scratch_layout_check.cpp:
    every layout's parts in order, on 256 bytes, inside `bytes`, and `bytes` equal to the sums the size functions used to spell out)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "scratch_layout_check")
    r = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "deepsir_amd", "csrc"),
                        os.path.join(ROOT, "tools", "scratch_layout_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "scratch_layout: " in r.stdout, r.stdout + r.stderr
