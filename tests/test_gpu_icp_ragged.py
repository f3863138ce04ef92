"""ICP and the edge information matrix on batches of clouds of unequal sizes (dsir_icp_refine_ex3, dsir_icp_correspondences_ex,
dsir_information_matrix_ex; `Engine.icp_refine / icp_correspondences / information_matrix(counts_src=, counts_ref=)`) on the MI355X.

The oracle everywhere is the existing dense call on the pair alone - `icp_refine(src[p:p+1, :Jp], ref[p:p+1, :Kp], ...)` without
counts - and every comparison is an equality of bytes (`torch.equal` on the uint8 view): T, all stats columns, idx, d2, info, count.
No tolerance appears anywhere.  The clouds are `test_icp_plane.surface`, the start poses 0.05 rad / 0.03 m off as in
tests/test_gpu_icp_grid.py, so that pairs freeze at different iterations.  The dense results are computed once per
(estimator, search, max_iter) and shared by the tests."""
import numpy as np
import pytest

from test_icp_plane import RADIUS, surface

pytestmark = pytest.mark.gpu

CAP = 4608
# (Jp, Kp): either side of the 64-query block of the brute search, of the 1024-row chunk of the plane and information sums and of
# the 4095 / 4096 switch between the segmented and the device-wide sort of the index; the first pairs are also the largest gap
# between a pair's own size and the capacity.  launch_kabsch's thresholds between its register and streaming kernels (5120 and 8192
# points) lie above this capacity: test_gpu_ragged_kabsch_kernel_choice below puts a pair on each side of both.
SIZES = [(1, 1), (63, 65), (64, 4095), (1023, 4096), (1024, 1337), (1025, 2049), (4608, 4607), (4607, 4608)]
ESTIMATORS = ("point", "plane")
SEARCHES = ("brute", "grid")


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), 0, max_points=4608, max_pairs=8)
    yield e
    e.close()


def _pose(rng, angle=0.05, shift=0.03):
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx
    return np.hstack([R, rng.uniform(-shift, shift, (3, 1))]).astype(np.float32)


def surface_normals(p):
    """unit normals of `surface` points from its two formulas (the height field z = 0.15 sin(3x) cos(2.5y), else the wall
    x = 0.02 sin(4 y / 1.5)): given normals for the plane estimator, no neighbour search needed"""
    p = np.asarray(p, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    field = np.abs(z - 0.15 * np.sin(3.0 * x) * np.cos(2.5 * y)) < 1e-6
    nf = np.c_[-0.45 * np.cos(3.0 * x) * np.cos(2.5 * y), 0.375 * np.sin(3.0 * x) * np.sin(2.5 * y), np.ones_like(x)]
    nw = np.c_[np.ones_like(x), -(0.08 / 1.5) * np.cos(4.0 * y / 1.5), np.zeros_like(x)]
    n = np.where(field[:, None], nf, nw)
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)


def _dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _same(a, b):
    """equality of bytes"""
    import torch
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


class Batch:
    """pairs of the given sizes: host clouds, normals and start poses, and their padded device arrays (`fill`: what the padding holds)"""

    def __init__(self, sizes, seed, cap=None):
        rng = np.random.default_rng(seed)
        self.sizes = list(sizes)
        self.src = [surface(j, rng).astype(np.float32) for j, _ in sizes]
        self.ref = [surface(k, rng).astype(np.float32) for _, k in sizes]
        self.nrm = [surface_normals(r) for r in self.ref]
        self.T0 = np.stack([_pose(rng) for _ in sizes])
        self.cap = cap

    def pick(self, order):
        b = Batch.__new__(Batch)
        b.sizes, b.cap = [self.sizes[i] for i in order], self.cap
        b.src, b.ref, b.nrm = ([x[i] for i in order] for x in (self.src, self.ref, self.nrm))
        b.T0 = self.T0[list(order)]
        return b

    def with_pair(self, p, other, q):
        b = self.pick(range(len(self.sizes)))
        b.sizes[p], b.src[p], b.ref[p], b.nrm[p] = other.sizes[q], other.src[q], other.ref[q], other.nrm[q]
        b.T0 = b.T0.copy()
        b.T0[p] = other.T0[q]
        return b

    def padded(self, fill="nan"):
        """-> src [P,J,3], ref [P,K,3], normals [P,K,3], T0 [P,3,4], counts_src, counts_ref on the device.  fill: "nan", "inf", or
        "copy": the pair's own rows again (row j holds row j mod n) - perfectly good queries and neighbours, were they read"""
        J = self.cap or max(1, max(j for j, _ in self.sizes))
        K = self.cap or max(1, max(k for _, k in self.sizes))

        def pad(rows, cap):
            out = np.full((len(rows), cap, 3), np.inf if fill == "inf" else np.nan, np.float32)
            for i, r in enumerate(rows):
                out[i, :len(r)] = r
                if fill == "copy" and len(r):
                    out[i] = r[np.arange(cap) % len(r)]
            return _dev(out)

        return (pad(self.src, J), pad(self.ref, K), pad(self.nrm, K), _dev(self.T0), _dev([j for j, _ in self.sizes], np.int32),
                _dev([k for _, k in self.sizes], np.int32))


@pytest.fixture(scope="module")
def batch():
    return Batch(SIZES, 20240, CAP)


def _refine(eng, src, ref, nrm, T0, est, search, max_iter, cs=None, cr=None):
    T, st = eng.icp_refine(src, ref, T0, RADIUS, max_iter=max_iter, estimator=est, normals_ref=nrm if est == "plane" else None, search=search,
                           counts_src=cs, counts_ref=cr)
    return T, st


_DENSE = {}


def dense(eng, b, est, search, max_iter):
    """the oracle: every pair of `b` alone through the dense call, [(T [1,3,4], stats [1,4|5])]; computed once per key and left unchanged"""
    key = (id(b), est, search, max_iter)
    if key not in _DENSE:
        _DENSE[key] = (b, [_refine(eng, _dev(b.src[p][None]), _dev(b.ref[p][None]), _dev(b.nrm[p][None]), _dev(b.T0[p][None]), est, search, max_iter)
                           for p in range(len(b.sizes))])                                # (b is kept alive with its results: the key is its id)
    return _DENSE[key][1]


def _assert_pairs(T, st, want, pairs=None, tag=""):
    for p in (range(len(want)) if pairs is None else pairs):
        assert _same(T[p:p + 1], want[p][0]), f"{tag}: T of pair {p}"
        assert _same(st[p:p + 1], want[p][1]), f"{tag}: stats of pair {p}: {st[p].tolist()} != {want[p][1][0].tolist()}"


# ------------------------------------------------------------------ 1. boundary sizes
@pytest.mark.parametrize("max_iter", [2, 30])
@pytest.mark.parametrize("search", SEARCHES)
@pytest.mark.parametrize("est", ESTIMATORS)
def test_gpu_ragged_refine_boundary_sizes(eng, batch, est, search, max_iter):
    src, ref, nrm, T0, cs, cr = batch.padded("nan")
    T, st = _refine(eng, src, ref, nrm, T0, est, search, max_iter, cs, cr)
    want = dense(eng, batch, est, search, max_iter)
    its = st[:, 3].cpu().numpy().astype(int).tolist()
    print(f"RAGGED {est} {search} max_iter={max_iter}: iterations {its}, converged {st[:, 2].cpu().numpy().astype(int).tolist()}, "
          f"fitness {np.round(st[:, 0].cpu().numpy(), 3).tolist()}")
    assert len(set(its)) >= 2                                       # the pairs freeze at different iterations (the device's own counts)
    _assert_pairs(T, st, want, tag=f"{est} {search} {max_iter}")


# ------------------------------------------------------------------ 2. the search step and the information matrix
@pytest.mark.parametrize("search", SEARCHES)
def test_gpu_ragged_search_step_and_information_matrix(eng, batch, search):
    import torch
    src, ref, _, T0, cs, cr = batch.padded("nan")
    idx, d2, st = eng.icp_correspondences(src, ref, T0, RADIUS, search=search, counts_src=cs, counts_ref=cr)
    info, count = eng.information_matrix(src, ref, T0, RADIUS, search=search, counts_src=cs, counts_ref=cr)
    assert int(count.sum()) > 1000
    for p, (Jp, Kp) in enumerate(batch.sizes):
        s1, r1, t1 = _dev(batch.src[p][None]), _dev(batch.ref[p][None]), _dev(batch.T0[p][None])
        i1, d1, st1 = eng.icp_correspondences(s1, r1, t1, RADIUS, search=search)
        f1, c1 = eng.information_matrix(s1, r1, t1, RADIUS, search=search)
        assert _same(idx[p:p + 1, :Jp], i1) and _same(d2[p:p + 1, :Jp], d1) and _same(st[p:p + 1], st1), f"pair {p}"
        assert _same(info[p:p + 1], f1) and _same(count[p:p + 1], c1), f"pair {p}"
        assert bool((idx[p, Jp:] == -1).all()) and _same(d2[p, Jp:], torch.zeros_like(d2[p, Jp:])), f"pair {p}: the padding entries"


# ------------------------------------------------------------------ 3. padding is invisible
@pytest.mark.parametrize("search", SEARCHES)
@pytest.mark.parametrize("est", ESTIMATORS)
def test_gpu_ragged_padding_is_invisible(eng, batch, est, search):
    """NaN, +inf and finite copies of the pair's own points (good neighbours and queries: what a too-long loop bound would take in
    silently) in the padding rows: the same bytes, which are the dense ones"""
    want = dense(eng, batch, est, search, 30)
    outs = {}
    for fill in ("nan", "inf", "copy"):
        src, ref, nrm, T0, cs, cr = batch.padded(fill)
        T, st = _refine(eng, src, ref, nrm, T0, est, search, 30, cs, cr)
        _assert_pairs(T, st, want, tag=f"{est} {search} padding {fill}")
        outs[fill] = (T, st) + tuple(eng.icp_correspondences(src, ref, T0, RADIUS, search=search, counts_src=cs, counts_ref=cr)) + \
            tuple(eng.information_matrix(src, ref, T, RADIUS, search=search, counts_src=cs, counts_ref=cr))
    for fill in ("inf", "copy"):
        assert all(_same(a, b) for a, b in zip(outs["nan"], outs[fill])), fill


# ------------------------------------------------------------------ 4. counts of zero, and clamping at the C ABI
def _ex3(eng, src, ref, nrm, T0, est, search, max_iter, cs, cr, name="dsir_icp_refine_ex3"):
    """the C entry itself -> (T, stats [P,5]); cs / cr: device int32 tensors or None (NULL)"""
    import torch
    P, J, stride = src.shape
    T = torch.empty((P, 3, 4), dtype=torch.float32, device="cuda")
    st = torch.empty((P, 5), dtype=torch.float64, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()
    args = [eng.h, src.data_ptr(), ref.data_ptr(), P, J, ref.shape[1], stride, float(RADIUS), int(max_iter), 1e-6, 1e-6, T0.data_ptr(), T.data_ptr(),
            int(est == "plane"), ptr(nrm) if est == "plane" else None, int(search == "grid"), st.data_ptr()]
    if name == "dsir_icp_refine_ex3":
        args += [ptr(cs), ptr(cr)]
    torch.cuda.synchronize()
    rc = getattr(eng.lib, name)(*args)
    assert rc == 0, eng.lib.dsir_last_error(eng.h).decode()
    eng.sync()
    return T, st


@pytest.fixture(scope="module")
def zbatch():
    return Batch([(700, 650), (700, 650), (700, 650), (1024, 1337)], 77)


@pytest.mark.parametrize("search", SEARCHES)
@pytest.mark.parametrize("est", ESTIMATORS)
def test_gpu_ragged_zero_counts_and_clamping(eng, zbatch, est, search):
    import torch
    src, ref, nrm, T0, cs, cr = zbatch.padded("nan")
    J, K = src.shape[1], ref.shape[1]
    cs0, cr0 = _dev([0, 700, 0, 1024], np.int32), _dev([650, 0, 0, 1337], np.int32)       # Jp = 0, Kp = 0, both, and a pair as it is
    T, st = _refine(eng, src, ref, nrm, T0, est, search, 30, cs0, cr0)
    assert _same(T[:3], T0[:3])                                     # T_out == T_init, bit for bit
    assert bool(torch.isfinite(st).all()) and bool((st[:3, :2] == 0).all())               # fitness and rmse 0, all stats finite
    _assert_pairs(T, st, dense(eng, zbatch, est, search, 30), pairs=[3], tag="beside the empty pairs")
    idx, d2, cst = eng.icp_correspondences(src, ref, T0, RADIUS, search=search, counts_src=cs0, counts_ref=cr0)
    info, count = eng.information_matrix(src, ref, T0, RADIUS, search=search, counts_src=cs0, counts_ref=cr0)
    assert bool((idx[:3] == -1).all()) and bool((d2[:3] == 0).all()) and bool((cst[:3] == 0).all())
    assert bool((info[:3] == 0).all()) and count[:3].tolist() == [0, 0, 0] and int(count[3]) > 0
    # the C ABI clamps: counts of -3 and capacity + 7 are counts of 0 and the capacity
    lo = _ex3(eng, src, ref, nrm, T0, est, search, 30, _dev([-3, 700, J + 7, 1024], np.int32), _dev([650, -3, 650, K + 7], np.int32))
    hi = _ex3(eng, src, ref, nrm, T0, est, search, 30, _dev([0, 700, J, 1024], np.int32), _dev([650, 0, 650, K], np.int32))
    assert _same(lo[0], hi[0]) and _same(lo[1], hi[1])
    assert _same(lo[0][:2], T0[:2])


# ------------------------------------------------------------------ 5. NULL counts are the old entries
@pytest.mark.parametrize("search", SEARCHES)
@pytest.mark.parametrize("est", ESTIMATORS)
def test_gpu_ragged_null_counts_are_the_old_entries(eng, est, search):
    import torch
    b = Batch([(1357, 1100)] * 3, 5)
    src, ref, nrm, T0, cs, cr = b.padded("nan")                      # a dense batch: nothing is padded
    P, J, K = 3, 1357, 1100
    old = _ex3(eng, src, ref, nrm, T0, est, search, 30, None, None, name="dsir_icp_refine_ex2")
    new = _ex3(eng, src, ref, nrm, T0, est, search, 30, None, None)
    assert _same(old[0], new[0]) and _same(old[1], new[1])
    cs2 = _dev([1357, 900, 1], np.int32)
    cr2 = _dev([1100, 64, 1100], np.int32)
    a = _ex3(eng, src, ref, nrm, T0, est, search, 30, cs2, None)
    c = _ex3(eng, src, ref, nrm, T0, est, search, 30, cs2, _dev([K] * 3, np.int32))
    assert _same(a[0], c[0]) and _same(a[1], c[1])                  # one count NULL: that side is full
    a = _ex3(eng, src, ref, nrm, T0, est, search, 30, None, cr2)
    c = _ex3(eng, src, ref, nrm, T0, est, search, 30, _dev([J] * 3, np.int32), cr2)
    assert _same(a[0], c[0]) and _same(a[1], c[1])
    if est == "plane":
        return                                                       # the two entries below have no estimator

    def step(name, *counts):
        idx, d2 = torch.empty((P, J), dtype=torch.int32, device="cuda"), torch.empty((P, J), dtype=torch.float32, device="cuda")
        st = torch.empty((P, 2), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert getattr(eng.lib, name)(eng.h, src.data_ptr(), ref.data_ptr(), P, J, K, 3, float(RADIUS), T0.data_ptr(), int(search == "grid"),
                                      idx.data_ptr(), d2.data_ptr(), st.data_ptr(), *counts) == 0, eng.lib.dsir_last_error(eng.h).decode()
        eng.sync()
        return idx, d2, st

    def info(name, *counts):
        f, n = torch.empty((P, 6, 6), dtype=torch.float64, device="cuda"), torch.empty((P,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert getattr(eng.lib, name)(eng.h, src.data_ptr(), ref.data_ptr(), P, J, K, 3, float(RADIUS), T0.data_ptr(), int(search == "grid"),
                                      f.data_ptr(), n.data_ptr(), *counts) == 0, eng.lib.dsir_last_error(eng.h).decode()
        eng.sync()
        return f, n

    for fn, old_name, new_name in ((step, "dsir_icp_correspondences", "dsir_icp_correspondences_ex"),
                                   (info, "dsir_information_matrix", "dsir_information_matrix_ex")):
        assert all(_same(x, y) for x, y in zip(fn(old_name), fn(new_name, None, None))), new_name
        assert all(_same(x, y) for x, y in zip(fn(new_name, cs2.data_ptr(), None), fn(new_name, cs2.data_ptr(), _dev([K] * 3, np.int32).data_ptr())))
        assert all(_same(x, y) for x, y in zip(fn(new_name, None, cr2.data_ptr()), fn(new_name, _dev([J] * 3, np.int32).data_ptr(), cr2.data_ptr())))


# ------------------------------------------------------------------ 6. two runs, and batch independence
@pytest.mark.parametrize("search", SEARCHES)
@pytest.mark.parametrize("est", ESTIMATORS)
def test_gpu_ragged_two_runs_and_batch_independence(eng, batch, zbatch, est, search):
    want = dense(eng, batch, est, search, 30)
    args = batch.padded("nan")
    T1, st1 = _refine(eng, *args[:4], est, search, 30, *args[4:])
    T2, st2 = _refine(eng, *args[:4], est, search, 30, *args[4:])
    assert _same(T1, T2) and _same(st1, st2)                        # two runs
    order = list(range(len(SIZES)))[::-1]
    args = batch.pick(order).padded("nan")
    T, st = _refine(eng, *args[:4], est, search, 30, *args[4:])
    assert _same(T, T1[order]) and _same(st, st1[order])            # the pairs in reversed order
    args = batch.with_pair(3, zbatch, 3).padded("nan")              # pair 3 replaced by another
    T, st = _refine(eng, *args[:4], est, search, 30, *args[4:])
    keep = [p for p in range(len(SIZES)) if p != 3]
    assert _same(T[keep], T1[keep]) and _same(st[keep], st1[keep])
    assert not _same(T[3:4], T1[3:4])
    _assert_pairs(T, st, want, pairs=keep, tag="beside a replaced pair")


# ------------------------------------------------------------------ launch_kabsch's kernel choice
def test_gpu_ragged_kabsch_kernel_choice():
    """The point-to-point step solves every pair of a launch with the kernel the capacity chooses (kabsch.hip: registers up to 5120
    and up to 8192 points, streaming above); a dense call chooses by the pair's own size.  One pair on each side of both thresholds
    at a capacity that streams: the bytes of the dense calls, so the kernels give the same bits and the choice may follow the
    capacity.  (Small reference clouds: the brute search of 8000 queries stays cheap.)"""
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), 0, max_points=8320, max_pairs=4)
    try:
        b = Batch([(5120, 700), (5121, 640), (8192, 900), (8193, 800)], 31)
        src, ref, nrm, T0, cs, cr = b.padded("nan")
        assert src.shape[1] == 8193
        T, st = _refine(e, src, ref, nrm, T0, "point", "brute", 30, cs, cr)
        _assert_pairs(T, st, dense(e, b, "point", "brute", 30), tag="kabsch kernels")
        assert float(st[:, 0].min()) > 0.05                          # the updates had correspondences to solve over
    finally:
        e.close()


# ------------------------------------------------------------------ 7. register_scene: batching changes nothing
def _scene(seed=3):
    """6 fragments of six sizes, crops of one surface under known poses, and all 15 edges with noise on their initial poses"""
    rng = np.random.default_rng(seed)
    base = surface(6000, rng)
    inv = lambda A: np.hstack([A[:, :3].T, (-A[:, :3].T @ A[:, 3])[:, None]])
    mul = lambda A, B: np.hstack([A[:, :3] @ B[:, :3], (A[:, :3] @ B[:, 3] + A[:, 3])[:, None]])
    frags, X = [], []
    for n in (1030, 1290, 1555, 1801, 2047, 2300):
        c = np.array([rng.uniform(0.55, 0.95), rng.uniform(0.55, 0.95), 0.0])
        crop = base[np.argsort(((base - c) ** 2).sum(1), kind="stable")[:n]]
        Xi = _pose(rng, angle=rng.uniform(0.2, 0.8), shift=0.5).astype(np.float64)        # fragment -> scene
        Xinv = inv(Xi)
        frags.append((crop @ Xinv[:, :3].T + Xinv[:, 3]).astype(np.float32))
        X.append(Xi)
    edges = []
    for s in range(6):
        for t in range(s + 1, 6):
            T = mul(inv(X[t]), X[s])                                                         # p_t = T p_s
            edges.append((s, t, mul(_pose(rng, 0.02, 0.01).astype(np.float64), T), t != s + 1))
    return frags, edges


@pytest.mark.parametrize("est", ESTIMATORS)
def test_gpu_register_scene_is_the_same_for_every_batch(eng, est):
    from deepsir_amd import harness as H
    frags, edges = _scene()
    assert len({len(f) for f in frags}) == 6 and len(edges) == 15
    res = {b: H.register_scene(frags, eng, edges, voxel_size=0.05, estimator=est, search="grid", batch=b) for b in (1, 4, 15)}
    print(f"SCENE {est}: dropped {[e['dropped'] for e in res[1]['edges']]}, counts {[e['count'] for e in res[1]['edges']]}")
    assert sum(e["dropped"] is None for e in res[1]["edges"]) >= 5
    for b in (4, 15):
        assert res[b]["X"].tobytes() == res[1]["X"].tobytes(), b
        for x, y in zip(res[b]["edges"], res[1]["edges"]):
            assert np.asarray(x["T"]).tobytes() == np.asarray(y["T"]).tobytes() and np.asarray(x["info"]).tobytes() == np.asarray(y["info"]).tobytes()
            assert x["count"] == y["count"] and x["dropped"] == y["dropped"] and (x["s"], x["t"]) == (y["s"], y["t"])
            assert np.float64(x["line"]).tobytes() == np.float64(y["line"]).tobytes()
