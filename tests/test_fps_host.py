"""The farthest-point-sampling rule on the host (deepsir_amd/fps.py, the restatement of csrc/fps.hip): against a float64 restatement
where fp32 is exact, against the reference's own sampler with the start fixed, the corner cases of the rule, and the stand-alone check
of csrc/fps.h (key, row-to-lane map, tiers, scratch layout)."""
import os
import subprocess

import numpy as np
import pytest

import fps_cases as K
from conftest import ROOT
from deepsir_amd.fps import farthest_point_sample_host as fps_host


def _fps64(p, k, start=0):
    """the rule in float64 on one cloud of finite rows: selection order and the chosen distances"""
    p = np.asarray(p, np.float64)
    n = len(p)
    dist = np.full(n, np.inf)
    left = np.ones(n, bool)
    idx, dd = [start], [np.inf]
    left[start] = False
    for _ in range(1, min(k, n)):
        d = p - p[idx[-1]]
        dist = np.minimum(dist, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        s = int(np.argmax(np.where(left, dist, -1.0)))
        idx.append(s); dd.append(dist[s])
        left[s] = False
    return np.array(idx), np.array(dd)


def _reference_sampler(pts, k, start):
    """dataloader/data_base.py:328 farthest_point_sampler with the random first row fixed to `start`; returns rows, not points"""
    calc = lambda p0, points: ((p0 - points) ** 2).sum(axis=1)
    rows = [start]
    distances = calc(pts[start], pts)
    for _ in range(1, k):
        rows.append(int(np.argmax(distances)))
        distances = np.minimum(distances, calc(pts[rows[-1]], pts))
    return np.array(rows)


@pytest.mark.parametrize("n,k,start", [(1, 1, 0), (2, 2, 1), (65, 65, 0), (300, 300, 7), (1025, 200, 1024), (5000, 64, 0)])
def test_against_float64_where_fp32_is_exact(n, k, start):
    """coordinates = small integers x 2^-4: differences, squares and sums are exact in fp32, so the sequences are identical"""
    rng = np.random.Generator(np.random.Philox(key=n))
    p = (rng.integers(-64, 65, (n, 3)) * 0.0625).astype(np.float32)
    index, counts, min_d2 = fps_host(p[None], k, start=start)
    n_distinct = len(np.unique(p, axis=0))
    i64, d64 = _fps64(p, k, start)
    assert counts[0] == k and np.array_equal(index[0], i64)
    assert np.array_equal(min_d2[0].astype(np.float64), d64)
    assert (min_d2[0, :min(k, n_distinct)][1:] > 0).all()          # twins come only after every distinct point


def test_against_the_reference_sampler_on_a_cloud_without_ties():
    p = K.random_cloud(700, 3)
    for start, k in ((0, 1), (0, 128), (699, 128), (123, 400)):
        index, counts, _ = fps_host(p[None], k, start=start)
        ref = _reference_sampler(p.astype(np.float64), k, start)    # the reference's loader works on float64 arrays
        assert counts[0] == k and np.array_equal(index[0], ref), (start, k)


def test_k_one_and_k_n():
    p = K.random_cloud(257, 1)
    index, counts, min_d2 = fps_host(p[None], 1, start=5)
    assert index.tolist() == [[5]] and counts.tolist() == [1] and np.isposinf(min_d2[0, 0])
    index, counts, min_d2 = fps_host(p[None], 257)
    assert counts[0] == 257 and sorted(index[0].tolist()) == list(range(257))
    q = K.nonfinite_cloud(257, 1)
    index, counts, min_d2 = fps_host(q[None], 257)
    finite = np.nonzero(np.isfinite(q).all(1))[0]
    assert counts[0] == len(finite) < 257 and sorted(index[0, :counts[0]].tolist()) == finite.tolist()
    assert (index[0, counts[0]:] == -1).all() and (min_d2[0, counts[0]:] == 0).all()


def test_duplicates_lower_index_first_twin_last():
    n = 41
    p = K.duplicate_cloud(n)
    h = n // 2
    index, counts, min_d2 = fps_host(p[None], n)
    order = index[0].tolist()
    assert counts[0] == n and sorted(order) == list(range(n))
    first = order[:h + 1]                                           # the h distinct rows of the first half and the row without a twin
    assert sorted(first) == list(range(h)) + [n - 1]
    assert (min_d2[0, 1:h + 1] > 0).all() and (min_d2[0, h + 1:] == 0).all()
    assert order[h + 1:] == list(range(h, 2 * h))                   # all dist 0: the twins in ascending index


def test_lattice_ties_go_to_the_lower_index():
    p = K.lattice(4)
    index, counts, min_d2 = fps_host(p[None], 64)
    i64, d64 = _fps64(p, 64)
    assert counts[0] == 64 and np.array_equal(index[0], i64) and np.array_equal(min_d2[0].astype(np.float64), d64)
    assert index[0, :2].tolist() == [0, 63] and min_d2[0, 1] == 27.0          # the far corner
    # step 2: min(|p|^2, |p - (3,3,3)|^2) peaks at 10, on the twelve permutations of (0,1,3) and (0,2,3); the lowest row is (0,1,3) = 7
    assert min_d2[0, 2] == 10.0 and index[0, 2] == 7
    # every step, from the definition: the chosen row is the lowest among the candidates of largest dist; most steps do tie
    q = p.astype(np.float64)
    dist, left, tied = np.full(64, np.inf), np.ones(64, bool), 0
    left[0] = False
    for t in range(1, 64):
        dist = np.minimum(dist, ((q - q[index[0, t - 1]]) ** 2).sum(1))
        top = np.nonzero(left & (dist == dist[left].max()))[0]
        assert index[0, t] == top[0], t
        tied += len(top) > 1
        left[index[0, t]] = False
    assert tied >= 32


def test_nonfinite_rows_and_start():
    n = 300
    p = K.nonfinite_cloud(n)
    bad = K.nonfinite_rows(n)
    finite = np.setdiff1d(np.arange(n), bad)
    index, counts, _ = fps_host(p[None], 100, start=int(bad[1]))    # start on a non-finite row: the lowest finite row instead
    assert counts[0] == 100 and index[0, 0] == finite[0] and not np.isin(index[0], bad).any()
    index2, _, _ = fps_host(p[None], 100, start=int(finite[0]))
    assert np.array_equal(index, index2)
    index3, _, _ = fps_host(p[None], 100, start=n + 5)              # a row that does not exist
    assert np.array_equal(index, index3)
    k = len(finite) + 10                                            # k above the finite count
    index, counts, min_d2 = fps_host(p[None], k)
    assert counts[0] == len(finite) and (index[0, len(finite):] == -1).all() and (min_d2[0, len(finite):] == 0).all()
    allbad = np.full((1, 5, 3), np.nan, np.float32)
    index, counts, min_d2 = fps_host(allbad, 3)
    assert counts[0] == 0 and (index == -1).all() and (min_d2 == 0).all()


@pytest.mark.parametrize("kind", sorted(K.KINDS))
def test_min_d2_is_non_increasing(kind):
    p = K.cloud(kind, 500)
    _, counts, min_d2 = fps_host(p[None], 500)
    d = min_d2[0, :counts[0]]
    assert np.isposinf(d[0]) and (np.diff(d[1:].astype(np.float64)) <= 0).all() and (d >= 0).all()


def test_ragged_counts():
    sizes = (65, 300, 1)
    clouds = [K.random_cloud(n, 10 + i) for i, n in enumerate(sizes)]
    pad = np.full((3, 300, 3), np.nan, np.float32)
    for i, c in enumerate(clouds):
        pad[i, :len(c)] = c
    index, counts, min_d2 = fps_host(pad, 100, counts=np.array(sizes, np.int32), start=64)
    assert counts.tolist() == [65, 100, 1]
    for i, c in enumerate(clouds):
        k = min(100, len(c))
        a, b, d = fps_host(c[None], k, start=64)
        assert np.array_equal(index[i, :k], a[0]) and (index[i, k:] == -1).all()
        assert np.array_equal(min_d2[i, :k].view(np.uint32), d[0].view(np.uint32)) and (min_d2[i, k:] == 0).all()
    assert index[0, 0] == 64 and index[1, 0] == 64 and index[2, 0] == 0
    with pytest.raises(ValueError):
        fps_host(pad, 301)
    with pytest.raises(ValueError):
        fps_host(pad, 0)


def test_fps_check_tool(tmp_path):
    """csrc/fps.h (the candidate key, the row-to-lane map, the tiers, the scratch layout) holds no device code: its stand-alone check
    (tools/fps_check.cpp; the sanitizer command is in the file's header) builds as plain host C++ and passes."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "fps_check")
    r = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "deepsir_amd", "csrc"),
                        os.path.join(ROOT, "tools", "fps_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "fps: " in r.stdout and "checks passed" in r.stdout, r.stdout + r.stderr
