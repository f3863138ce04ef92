"""Radius and hybrid neighbour lists on the device (csrc/radius_nn.hip, ``NNIndex.neighbors`` / ``Engine.radius_neighbors``): the CSR
and d2 bit for bit against the float32 restatement (deepsir_amd/overlap.py::radius_neighbors_host) and, for max_nn = 0, against
``Engine.radius_matches``, on the smallest shapes that can break the kernels: rows from 0 to above 512 entries (the fill kernel ranks
512 entries per chunk, 64 candidates per walk step)."""
import os
import re

import numpy as np
import pytest
import torch

from deepsir_amd import overlap as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0.1
H = float(np.float32(R)) * (1.0 + 1.0 / 1024.0)      # the lattice's cell edge
MAX_NN = [0, 1, 16, 100]


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), 0, max_points=8192, max_pairs=2)
    yield e
    e.close()


def pack(frags):
    off = np.concatenate([[0], np.cumsum([len(f) for f in frags])]).astype(np.int64)
    return np.concatenate([np.asarray(f, np.float32).reshape(-1, 3) for f in frags]), off


def device(eng, frags, jobs, r=R, poses=None, max_nn=0):
    pts, off = pack(frags)
    T = None if poses is None else torch.from_numpy(np.ascontiguousarray(poses, np.float32)).cuda()
    index = eng.nn_index(torch.from_numpy(pts).cuda(), off, r)
    out = index.neighbors(np.asarray(jobs, np.int32).reshape(-1, 2), T, max_nn, with_dist=True)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def same(got, want, tag=""):
    for name, g, w in zip(("offsets", "cols", "d2"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), (tag, name, np.nonzero(g.view(np.int32) != w.view(np.int32))[0][:5])


def check(eng, frags, jobs, r=R, poses=None, max_nn=0):
    """Device == host, bit for bit: offsets, cols and d2; -> the device's."""
    pts, off = pack(frags)
    got = device(eng, frags, jobs, r, poses, max_nn)
    same(got, O.radius_neighbors_host(pts, off, jobs, r, poses, max_nn), f"max_nn={max_nn}")
    return got


def clusters(seed, sizes=(1, 15, 16, 17, 99, 100, 101), spread=0.02):
    """Isolated clusters, 1 apart: every point of a cluster of size s has exactly s neighbours - max_nn below, at and above a count."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.random((s, 3)) * spread + [float(i), 0.0, 0.0] for i, s in enumerate(sizes)]).astype(np.float32)


@pytest.fixture(scope="module")
def ragged():
    """Fragments of 0, 1, 257 and 1500 points.  The 1500: 700 inside a cube of 0.04 (rows above 512 entries: a second chunk), 451 thin
    over a 3 x 3 sheet (rows of 1 and 2), and the clusters of 1 .. 101.  The 257 straddle the cube; the single point sits in it."""
    rng = np.random.default_rng(11)
    blob = rng.random((700, 3)) * 0.04 + [5.0, 5.0, 0.0]
    sheet = np.concatenate([rng.random((451, 2)) * 3.0, np.zeros((451, 1))], 1) + [0.0, 2.0, 0.0]
    big = np.concatenate([blob, sheet, clusters(12)])[rng.permutation(1500)].astype(np.float32)
    mid = (rng.random((257, 3)) * [0.3, 0.3, 0.05] + [4.9, 4.9, 0.0]).astype(np.float32)
    one = np.array([[5.02, 5.02, 0.02]], np.float32)
    return [np.zeros((0, 3), np.float32), one, mid, big]


@pytest.fixture(scope="module")
def ragged_host(ragged):
    """The host rule on every ordered pair of the ragged fragments, once per max_nn."""
    pts, off = pack(ragged)
    jobs = [(q, t) for q in range(4) for t in range(4)]
    return jobs, {m: O.radius_neighbors_host(pts, off, jobs, R, None, m) for m in MAX_NN}


@pytest.mark.parametrize("max_nn", MAX_NN)
def test_ragged_all_ordered_pairs(eng, ragged, ragged_host, max_nn):
    jobs, want = ragged_host
    got = device(eng, ragged, jobs, max_nn=max_nn)
    same(got, want[max_nn], f"max_nn={max_nn}")
    lens = np.diff(got[0].astype(np.int64))
    full = np.diff(want[0][0].astype(np.int64))
    assert np.array_equal(lens, np.minimum(full, max_nn) if max_nn else full)
    if max_nn:
        assert (full < max_nn).any() and (full == max_nn).any() and (full > max_nn).any()       # below, at and above a row's count
    else:
        assert (full == 1).any() and (full > 64).any() and (full > 512).any()


def test_determinism_and_independence_of_the_job_list(eng, ragged, ragged_host):
    jobs, want = ragged_host
    for max_nn in (0, 16):
        a = device(eng, ragged, jobs, max_nn=max_nn)
        b = device(eng, ragged, jobs, max_nn=max_nn)
        same(a, b, "two runs")
        rows = np.concatenate([[0], np.cumsum([len(ragged[q]) for q, _ in jobs])])
        for j in (6, 11, 14, 15):                                   # (1, 2), (2, 3), (3, 2), (3, 3) alone
            off, cols, d2 = device(eng, ragged, [jobs[j]], max_nn=max_nn)
            lo, hi = a[0][rows[j]], a[0][rows[j + 1]]
            assert np.array_equal(off, a[0][rows[j]:rows[j + 1] + 1] - lo)
            assert cols.tobytes() == a[1][lo:hi].tobytes() and d2.tobytes() == a[2][lo:hi].tobytes()


@pytest.mark.parametrize("posed", [False, True])
def test_whole_ball_equals_radius_matches(eng, ragged, posed):
    from deepsir_amd import augment as A
    src, ref = ragged[2], ragged[3]
    T = np.eye(4, dtype=np.float32)[:3]
    if posed:
        T = np.concatenate([A.rodrigues(np.array([0.1, 0.9, -0.2]), 0.7), [[0.21], [-0.43], [0.01]]], 1).astype(np.float32)
        src = ((src.astype(np.float64) - T[:, 3]) @ T[:, :3].astype(np.float64)).astype(np.float32)      # T brings it back onto ref
    dT = torch.from_numpy(T[None].copy()).cuda()
    off_b, cols_b = eng.radius_matches(torch.from_numpy(src[None]).cuda(), torch.from_numpy(ref[None]).cuda(), dT, R)
    got = check(eng, [src, ref], [(0, 1)], poses=T[None])
    assert got[0].tobytes() == off_b.cpu().numpy().tobytes() and got[1].tobytes() == cols_b.cpu().numpy().tobytes()
    assert len(got[1]) > 1000
    if not posed:                                                   # poses == NULL reads the unmoved bits: the identity gives the same
        same(device(eng, [src, ref], [(0, 1)]), got, "identity vs none")
    # the dense form: one fragment and one job (i, i) per cloud, cloud-local columns
    x = torch.from_numpy(np.stack([ref[:257], src])).cuda()
    eye = torch.eye(4)[:3].repeat(2, 1, 1).contiguous().cuda()
    off_b, cols_b = eng.radius_matches(x, x, eye, R)
    off_g, cols_g = eng.radius_neighbors(x, R)
    assert torch.equal(off_g, off_b) and torch.equal(cols_g, cols_b) and cols_g.numel() > 514


@pytest.mark.parametrize("max_nn", MAX_NN)
def test_cell_faces_exact_radius_and_ties(eng, max_nn):
    # integer multiples of the cell edge from the origin (rounded to fp32), and half steps: points on faces, edges and corners
    g = np.array([[i, j, k] for i in range(7) for j in range(7) for k in range(3)], np.float64) * (0.5 * H)
    check(eng, [g.astype(np.float32), g.astype(np.float32)[::-1].copy()], [(0, 0), (0, 1), (1, 0)], max_nn=max_nn)
    # a lattice of step r / 2 with r = 0.5: d2 == fl(r r) exactly two steps along an axis (excluded), and every d2 tied many times
    q = np.array([[i, j, k] for i in range(6) for j in range(6) for k in range(4)], np.float32) * np.float32(0.25)
    off, cols, d2 = check(eng, [q], [(0, 0)], r=0.5, max_nn=max_nn)
    assert (d2 < np.float32(0.25)).all()
    if max_nn == 0:
        inner = np.nonzero((q[:, 0] == 0.5) & (q[:, 1] == 0.5) & (q[:, 2] == 0.25))[0][0]
        assert off[inner + 1] - off[inner] == 27                    # the 3 x 3 x 3 block (corners at 0.1875 < 0.25), not the six at exactly r
    # 3-4-5 on a grid of 1/64: d2 == 25 / 4096 == fl(r r)
    t = np.array([[0, 0, 0], [3, 4, 0], [0, 0, 5], [3, 0, 3.9]], np.float32) / np.float32(64.0)
    off, cols, _ = check(eng, [t], [(0, 0)], r=5.0 / 64.0, max_nn=max_nn)
    assert list(cols[off[0]:off[1]]) == ([0] if max_nn == 1 else [0, 3])


@pytest.mark.parametrize("max_nn", [0, 1, 2, 3, 16, 100, 119, 120, 121])
def test_duplicates_tie_across_the_boundary_by_index(eng, max_nn):
    rng = np.random.default_rng(5)
    base = (rng.random((40, 3)) * 0.05).astype(np.float32)
    b = np.concatenate([base, base, base])                          # indices i, 40 + i, 80 + i coincide
    off, cols, d2 = check(eng, [base[:10], b], [(0, 1), (1, 1)], max_nn=max_nn)
    if max_nn == 2:
        assert np.array_equal(cols[:20].reshape(10, 2), np.stack([np.arange(10), 40 + np.arange(10)], 1))


@pytest.mark.parametrize("max_nn", [0, 16])
def test_non_finite_rows_disjoint_boxes_one_cell_and_large_offsets(eng, max_nn):
    rng = np.random.default_rng(7)
    a = (rng.random((300, 3)) * 0.4).astype(np.float32)
    b = a.copy()
    a[7] = [np.nan, 0.0, 0.0]; a[8] = [0.1, np.inf, 0.0]; a[299] = [-np.inf, np.nan, 0.0]
    b[3] = np.nan; b[150] = [0.0, 0.0, np.inf]
    off, cols, _ = check(eng, [a, b], [(0, 1), (1, 0), (0, 0), (1, 1)], max_nn=max_nn)
    assert off[8] - off[7] == 0 and off[9] - off[8] == 0 and 3 not in cols[:off[300]] and 150 not in cols[:off[300]]
    far = a[:100] + np.float32(50.0)                                # disjoint boxes: empty rows either way, with and without a pose
    far[7:9] = 50.0
    off, cols, _ = check(eng, [b, far], [(0, 1), (1, 0)], max_nn=max_nn)
    assert off[-1] == 0
    back = np.array([[1, 0, 0, -50], [0, 1, 0, -50], [0, 0, 1, -50]], np.float32)
    off, cols, _ = check(eng, [b, far], [(1, 0)], poses=back[None], max_nn=max_nn)          # the pose brings them together
    assert off[-1] > 100
    cell = (rng.random((600, 3)) * 0.05).astype(np.float32)         # every point in one cell: rows of 600
    off, cols, _ = check(eng, [cell, cell[:257]], [(0, 0), (1, 0), (0, 1)], max_nn=max_nn)
    assert (np.diff(off)[:600] == (max_nn or 600)).all()
    big = (rng.random((500, 3)) * 0.5).astype(np.float32) + np.float32(1e5)                 # 1e5: an ulp is 0.0078, ties everywhere
    off, cols, _ = check(eng, [big, big[::-1].copy()], [(0, 0), (0, 1)], max_nn=max_nn)
    assert off[-1] > 1000


def test_refusals_raise_before_any_launch(eng, ragged):
    from deepsir_amd import _lib
    lib = _lib.load()
    pts, off = pack(ragged)
    d = torch.from_numpy(pts).cuda()
    index = eng.nn_index(d, off, R)
    with pytest.raises(ValueError, match="max_nn"):
        index.neighbors([(2, 3)], max_nn=-1)
    for bad in ([(0, 4)], [(-1, 0)], [(2, 3), (4, 0)]):
        with pytest.raises(ValueError, match="job index out of range"):
            index.neighbors(bad)
    with pytest.raises(ValueError, match="poses"):
        index.neighbors([(2, 3)], poses=torch.zeros(2, 3, 4, device="cuda"))
    for r in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="radius"):
            eng.radius_neighbors(d[None], r)
    built = []
    real = eng.nn_index
    eng.nn_index = lambda *a, **k: built.append(1) or real(*a, **k)
    try:
        with pytest.raises(ValueError, match="max_nn"):
            eng.radius_neighbors(d[None], R, max_nn=-3)             # refused before the index is built
    finally:
        del eng.nn_index
    assert not built
    assert lib.dsir_t_nn_radius_scratch(1, 2 ** 26 - 1) > 0 and lib.dsir_t_nn_radius_scratch(1, 2 ** 26) == 0      # one workgroup per row
    # the C entries themselves: an error code, and the buffers they would have written are untouched
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda x: x.ctypes.data
    ok, bad = np.array([[2, 3]], np.int32), np.array([[2, 4]], np.int32)
    b_ok = index.bounds
    b_wide = np.array([0, 0, 0, 2, 7e5, 2], np.float32)
    assert lib.dsir_t_nn_radius_scratch(1, 257) > 0 and lib.dsir_t_nn_radius_scratch(-1, 0) == 0 and lib.dsir_t_nn_radius_scratch(1, 2 ** 31) == 0
    counts = torch.full((257,), -7, dtype=torch.int32, device="cuda")
    offs = torch.full((258,), -7, dtype=torch.int32, device="cuda")
    cols = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    scratch = torch.full((int(lib.dsir_t_nn_radius_scratch(1, 257)),), 0x5a, dtype=torch.uint8, device="cuda")
    for r, b, jb, m in ((R, b_ok, ok, -1), (0.0, b_ok, ok, 0), (R, b_wide, ok, 0), (R, b_ok, bad, 0)):
        assert lib.dsir_t_nn_radius_count(stream, index.index.data_ptr(), p(off), 4, p(jb), 1, None, r, p(b), m, counts.data_ptr(),
                                          offs.data_ptr(), scratch.data_ptr()) != 0
        assert lib.dsir_t_nn_radius_fill(stream, index.index.data_ptr(), p(off), 4, p(jb), 1, None, r, p(b), m, offs.data_ptr(),
                                         scratch.data_ptr(), cols.data_ptr(), None, 64) != 0
    torch.cuda.synchronize()
    assert (counts == -7).all() and (offs == -7).all() and (cols == -7).all() and (scratch == 0x5a).all()


def test_header_declares_and_library_exports_the_entries():
    from deepsir_amd import _lib
    lib = _lib.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsir_train.h")).read(), flags=re.S)
    for name, nargs in (("dsir_t_nn_radius_scratch", 2), ("dsir_t_nn_radius_count", 13), ("dsir_t_nn_radius_fill", 15)):
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert len(_lib.SYMBOLS[name][1]) == nargs and hasattr(lib, name)
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsir.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+dsir_estimate_normals_csr\s*\(([^)]*)\)", txt)
    assert m and len(m.group(1).split(",")) == 10 and hasattr(lib, "dsir_estimate_normals_csr")
