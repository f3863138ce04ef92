"""Neighbour lists on the host (no GPU): the float32 restatement of the radius / hybrid rule (deepsir_amd/overlap.py::
radius_neighbors_host; the rule: csrc/radius_nn.hip) against a float64 KD-tree, its selection and order, the corner cases, and the
stand-alone sanitizer build of tools/radius_nn_check.cpp."""
import os
import subprocess

import numpy as np
import pytest

from deepsir_amd import overlap as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0.1
BAND = 1e-3          # relative band around r^2 inside which fp32 and fp64 may disagree (tests/test_overlap_host.py)


def rows_of(off, cols):
    return [cols[off[i]:off[i + 1]] for i in range(len(off) - 1)]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_rule_against_a_float64_kdtree(seed):
    """Uniform clouds of 2000 points: outside a relative band of 1e-3 around r^2 the float32 sets equal the float64 ball; at most
    1 % of the float64 entries lie in the band (on these clouds: 0.11 - 0.16 %, float64 side alone)."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    a, b = rng.random((2000, 3)).astype(np.float32), rng.random((2000, 3)).astype(np.float32)
    off, cols, d2 = O.radius_neighbors_host(np.concatenate([a, b]), [0, 2000, 4000], [(0, 1)], R)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    ball = cKDTree(b64).query_ball_point(a64, R * (1.0 + BAND))           # a superset of ball and band
    r2 = R * R
    n64 = in_band = 0
    for i, got in enumerate(rows_of(off, cols)):
        k = np.array(sorted(ball[i]), np.int64)
        e = ((b64[k] - a64[i]) ** 2).sum(1)
        band = np.abs(e - r2) <= BAND * r2
        m64 = e < r2
        n64 += int(m64.sum())
        in_band += int((m64 & band).sum())
        sure = set(k[m64 & ~band].tolist())
        maybe = set(k[band].tolist())
        g = set(got.tolist())
        assert sure <= g and g <= sure | maybe, i
    print(f"seed {seed}: fp64 entries {n64}, fp32 {len(cols)}, in band {in_band} ({100.0 * in_band / n64:.3f} %)")
    assert n64 > 4 * 2000                                                   # rows hold several entries
    assert in_band <= 0.01 * n64
    assert off[0] == 0 and off[-1] == len(cols) == len(d2)


def test_hybrid_selection_ties_go_to_the_lower_index():
    rng = np.random.default_rng(5)
    base = rng.random((40, 3)).astype(np.float32) * np.float32(0.05)       # all within 0.1 of each other
    b = np.concatenate([base, base, base])                                 # every point three times: indices i, 40 + i, 80 + i
    a = base[:10]
    pts = np.concatenate([a, b])
    offs = [0, 10, 10 + len(b)]
    off0, cols0, d0 = O.radius_neighbors_host(pts, offs, [(0, 1)], R)
    assert np.array_equal(np.diff(off0), np.full(10, 120))                 # the whole ball
    for max_nn in (1, 2, 3, 4, 16, 100, 119, 120, 121, 500):
        off, cols, d2 = O.radius_neighbors_host(pts, offs, [(0, 1)], R, max_nn=max_nn)
        assert np.array_equal(np.diff(off), np.full(10, min(120, max_nn)))
        for i, (row, dist) in enumerate(zip(rows_of(off, cols), rows_of(off, d2))):
            assert np.all(np.diff(row) > 0)                                # ascending index
            full, fd = cols0[off0[i]:off0[i + 1]], d0[off0[i]:off0[i + 1]]
            order = sorted(range(120), key=lambda t: (fd[t], full[t]))[:max_nn]
            assert np.array_equal(row, np.sort(full[order]))
            assert np.array_equal(dist, fd[np.isin(full, row)])
    # rank 1 and 2: the twin at distance 0 three times - the lower indices win, in index order
    off, cols, _ = O.radius_neighbors_host(pts, offs, [(0, 1)], R, max_nn=2)
    assert np.array_equal(cols.reshape(10, 2), np.stack([np.arange(10), 40 + np.arange(10)], 1))
    off, cols, _ = O.radius_neighbors_host(pts, offs, [(0, 1)], R, max_nn=500)        # larger than the count: the ball
    assert np.array_equal(cols, cols0) and np.array_equal(off, off0)


def test_row_order_self_match_and_non_finite_rows():
    rng = np.random.default_rng(6)
    x = rng.random((300, 3)).astype(np.float32) * np.float32(0.4)
    x[7] = [np.nan, 0.0, 0.0]
    x[8] = [0.1, np.inf, 0.0]
    off, cols, d2 = O.radius_neighbors_host(x, [0, 300], [(0, 0)], R)
    rows = rows_of(off, cols)
    assert len(rows[7]) == 0 and len(rows[8]) == 0                          # a non-finite query has an empty row
    assert 7 not in cols and 8 not in cols                                  # a non-finite b is in no row
    for i, (row, dist) in enumerate(zip(rows, rows_of(off, d2))):
        assert np.all(np.diff(row) > 0)
        if i not in (7, 8):
            assert i in row and dist[list(row).index(i)] == 0.0              # a query of the target finds itself
    assert (d2 < np.float32(R) * np.float32(R)).all()
    # d2 == fl(r r) exactly is excluded: 3-4-5 on a grid of 1/64 with r = 5/64
    g = np.array([[0, 0, 0], [3, 4, 0], [0, 0, 5], [3, 0, 3.9]], np.float32) / np.float32(64.0)
    off, cols, _ = O.radius_neighbors_host(g, [0, 4], [(0, 0)], 5.0 / 64.0)
    assert list(rows_of(off, cols)[0]) == [0, 3]
    e0 = O.radius_neighbors_host(x, [0, 0, 300], [(0, 1), (1, 0)], R)       # an empty side, either way
    assert np.array_equal(e0[0], np.zeros(301, np.int32)) and len(e0[1]) == 0


def test_pose_is_applied_in_float32_before_the_search():
    rng = np.random.default_rng(4)
    a, b = (rng.random((300, 3)) * 0.5).astype(np.float32), (rng.random((300, 3)) * 0.5).astype(np.float32)
    T = np.array([[0.0, -1.0, 0.0, 0.5], [1.0, 0.0, 0.0, -0.25], [0.0, 0.0, 1.0, 0.125]], np.float32)
    pts = np.concatenate([a, b])
    got = O.radius_neighbors_host(pts, [0, 300, 600], [(0, 1)], R, poses=T[None], max_nn=5)
    moved = np.stack([-a[:, 1] + np.float32(0.5), a[:, 0] - np.float32(0.25), a[:, 2] + np.float32(0.125)], 1)
    want = O.radius_neighbors_host(np.concatenate([moved, b]), [0, 300, 600], [(0, 1)], R, max_nn=5)
    assert len(got[1]) > 300
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.int32), w.view(np.int32))
    # rows follow the job list: two jobs are the two single-job results, one after the other
    both = O.radius_neighbors_host(pts, [0, 300, 600], [(0, 1), (1, 1)], R, poses=np.stack([T, np.eye(4, dtype=np.float32)[:3]]), max_nn=5)
    self1 = O.radius_neighbors_host(pts, [0, 300, 600], [(1, 1)], R, max_nn=5)
    assert np.array_equal(both[1], np.concatenate([got[1], self1[1]]))
    assert np.array_equal(both[0], np.concatenate([got[0], got[0][-1] + self1[0][1:]]))


def test_sanitizer_build_of_the_host_check(tmp_path):
    """csrc/radius_nn.h compiles as plain host C++ under AddressSanitizer + UndefinedBehaviorSanitizer and its stand-alone check
    (tools/radius_nn_check.cpp: scratch and offset arithmetic, refusals) passes on the CPU."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "radius_nn_check")
    # host code only: -x c++ compiles no device code, and -fno-gpu-sanitize keeps the sanitizers off any offload part
    san = ["-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + san + ["-I" + os.path.join(ROOT, "deepsir_amd", "csrc"),
                        os.path.join(ROOT, "tools", "radius_nn_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "radius_nn: " in r.stdout, r.stdout + r.stderr
