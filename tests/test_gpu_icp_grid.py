"""The cell-indexed ICP search (csrc/icp_grid.hip: icp_nn_grid_kernel and the per-pair index build) on the MI355X: one search step
(`Engine.icp_correspondences`, dsir_icp_correspondences) against the host rule of deepsir_amd/icp.py and against the brute-force
kernel, bit for bit in idx, d2 and stats; the whole loop (`Engine.icp_refine(search="grid")`, dsir_icp_refine_ex2) against
`search="brute"`, byte for byte in T and stats, for both estimators; determinism; bad arguments.  Every test calls a name or passes
an argument that does not exist before this search, so every test fails without it."""
import numpy as np
import pytest

from deepsir_amd import icp as I
from test_icp_plane import RADIUS, flat_case, surface, surface_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), 0, max_points=4096, max_pairs=3)
    yield e
    e.close()


def _dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _corr(eng, src, ref, T, r, search):
    idx, d2, st = eng.icp_correspondences(_dev(src), _dev(ref), _dev(T), r, search=search)
    return idx.cpu().numpy(), d2.cpu().numpy(), st.cpu().numpy()


def _check_step(eng, src, ref, T, r, tag=""):
    """src [P,J,3], ref [P,K,3], T [P,3,4]: grid == brute == host in idx, d2 and stats, bit for bit -> the host's idx [P,J]"""
    src, ref, T = np.asarray(src, np.float32), np.asarray(ref, np.float32), np.asarray(T, np.float32)
    host = [I.icp_correspondences_host(src[p], ref[p], T[p], r) for p in range(len(src))]
    h_idx, h_d2, h_st = (np.stack([h[k] for h in host]) for k in range(3))
    b = _corr(eng, src, ref, T, r, "brute")
    g = _corr(eng, src, ref, T, r, "grid")
    print(f"STEP {tag} P={src.shape[0]} J={src.shape[1]} K={ref.shape[1]} r={r}: matched {(h_idx >= 0).sum()} of {h_idx.size}, "
          f"grid != host in {(g[0] != h_idx).sum()} idx / {(g[1].view(np.uint32) != h_d2.view(np.uint32)).sum()} d2, "
          f"brute != host in {(b[0] != h_idx).sum()} idx")
    assert g[0].dtype == np.int32 and g[1].dtype == np.float32 and g[2].shape == (len(src), 2)
    assert np.array_equal(g[0], h_idx) and g[1].tobytes() == h_d2.tobytes() and g[2].tobytes() == h_st.tobytes()
    assert np.array_equal(b[0], h_idx) and b[1].tobytes() == h_d2.tobytes() and b[2].tobytes() == h_st.tobytes()
    return h_idx


def _pose(rng, angle=0.05, shift=0.03):
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx
    return np.hstack([R, rng.uniform(-shift, shift, (3, 1))]).astype(np.float32)


def _eye(P):
    return np.tile(np.eye(3, 4, dtype=np.float32), (P, 1, 1))


# ------------------------------------------------------------------ 1. the search step
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("J,K,r", [(1, 1, 3.0), (63, 65, 0.25), (1000, 1337, 0.05), (4096, 4095, 0.03)])
def test_gpu_grid_step_shapes(eng, J, K, r, P):
    rng = np.random.default_rng(1000 * P + J)
    src = np.stack([surface(J, rng) for _ in range(P)]).astype(np.float32)
    ref = np.stack([surface(K, rng) for _ in range(P)]).astype(np.float32)
    T = np.stack([_pose(rng) for _ in range(P)])
    idx = _check_step(eng, src, ref, T, r, "shapes")
    if J >= 1000:
        assert 0.1 < (idx >= 0).mean() < 0.99                   # matches and misses mix


def test_gpu_grid_step_cell_faces_and_exactly_r(eng):
    r = 0.5
    h = float(np.float32(r)) * I.GRID_MARGIN
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    ref_faces = (g * h).astype(np.float32)                      # on the cell faces, up to the rounding to fp32
    ref_half = (g * 0.25).astype(np.float32)                    # a lattice of r / 2: neighbours at exactly d2 == r2 and ties
    src_a = ref_faces + np.float32([r, 0, 0])
    src_b = ref_half + np.float32([0.375, 0, 0])
    idx = _check_step(eng, np.stack([src_a, ref_faces - np.float32([0, r, 0]), src_b]), np.stack([ref_faces, ref_faces, ref_half]),
                      _eye(3), r, "faces")
    assert (idx >= 0).mean() > 0.8
    idx, d2, _ = _corr(eng, src_b[None], ref_half[None], _eye(1), 0.125, "grid")      # the neighbour at exactly r = 0.125
    assert (idx[0] >= 0).sum() == len(ref_half) - 32 and (d2[0][idx[0] >= 0] == np.float32(0.015625)).all()
    _check_step(eng, src_b[None], ref_half[None], _eye(1), 0.125, "exactly r")
    q = np.array([[0, 0, 0], [10, 0, 0], [0, 20, 0], [0, 0, 30], [40, 40, 40]], np.float32)
    t = q + np.array([[0.5, 0, 0], [-0.5, 0, 0], [0, 0.5, 0], [0, 0, -0.5], [0.5, 0.5, 0]], np.float32)
    idx = _check_step(eng, q[None], t[None], _eye(1), 0.5, "offset 0.5")
    assert np.array_equal(idx[0], [0, 1, 2, 3, -1])


def test_gpu_grid_step_exact_ties_on_an_integer_lattice(eng):
    """queries at cell centres and edge midpoints of an integer lattice: 8, 4 and 2 distinct points at the same d2, exactly; the
    reference rows shuffled, so the lower ORIGINAL index is not the first in cell order"""
    rng = np.random.default_rng(4)
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    ref = np.stack([g[rng.permutation(len(g))] for _ in range(3)])
    src = np.stack([g[:125] * 0 + g[rng.permutation(len(g))[:125]] + off for off in
                    (np.float32([0.5, 0.5, 0.5]), np.float32([0.5, 0.5, 0]), np.float32([0.5, 0, 0]))])
    idx = _check_step(eng, src, ref, _eye(3), 1.0, "ties")
    assert (idx >= 0).mean() > 0.5
    _check_step(eng, src, ref, _eye(3), 3.0, "ties, r = 3 cells")


def test_gpu_grid_step_duplicated_reference_points(eng):
    rng = np.random.default_rng(8)
    base = surface(300, rng).astype(np.float32)
    ref = np.concatenate([base, base[::-1], base])[None]
    src = np.concatenate([base, base + np.float32(0.003)])[None]
    idx = _check_step(eng, src, ref, _eye(1), 0.05, "duplicates")
    assert np.array_equal(idx[0, :300], np.arange(300))         # the first of the three copies
    _check_step(eng, src, ref[:, 300:], _eye(1), 0.05, "duplicates, reversed copy first")


def test_gpu_grid_step_queries_far_outside(eng):
    rng = np.random.default_rng(9)
    src = np.stack([surface(500, rng) for _ in range(3)]).astype(np.float32)
    ref = np.stack([surface(700, rng) for _ in range(3)]).astype(np.float32)
    T = _eye(3)
    T[0, :, 3] = [1e4, -1e4, 3e3]                               # clamped cells on the high and the low side
    T[1, :, 3] = [-1e30, 1e30, 0]
    T[2, :, 3] = [0.3, 0, 0]                                    # partly outside
    idx = _check_step(eng, src, ref, T, 0.05, "far")
    assert (idx[:2] == -1).all() and 0 < (idx[2] >= 0).sum() < 500


def test_gpu_grid_step_radius_larger_than_the_cloud(eng):
    rng = np.random.default_rng(10)
    src = np.stack([surface(600, rng) for _ in range(2)]).astype(np.float32)
    ref = np.stack([surface(900, rng) for _ in range(2)]).astype(np.float32)
    idx = _check_step(eng, src, ref, np.stack([_pose(rng), _pose(rng)]), 5.0, "one cell")     # every run spans the whole cloud
    assert (idx >= 0).all()
    _check_step(eng, src, ref, _eye(2), 1e18, "r^2 just finite")


def test_gpu_grid_step_tiny_radius_takes_the_coarse_edge(eng):
    rng = np.random.default_rng(11)
    r = 1e-5
    cl = [np.float32(rng.uniform(0, 1000, 3)) + rng.uniform(0, 3e-4, (80, 3)).astype(np.float32) for _ in range(6)]
    ref = np.concatenate(cl + [np.float32([[0, 0, 0], [1000, 1000, 10]])]).astype(np.float32)
    o, h = I.grid_lattice(ref, r)
    assert h == 1000.0 / 2 ** 20                                 # extent / 2^20, fifty radii: not the radius term
    src = ref[rng.permutation(len(ref))]
    idx = _check_step(eng, src[None], ref[None], _eye(1), r, "coarse h")
    assert (idx >= 0).all()
    _check_step(eng, (src + np.float32(6e-5))[None], ref[None], _eye(1), 1e-4, "coarse h, offset")
    _check_step(eng, src[None, :50] * np.float32(1e-20), ref[None, :60] * np.float32(1e-20), _eye(1), 1e-30, "r^2 underflows")


def test_gpu_grid_step_non_finite_rows(eng):
    rng = np.random.default_rng(12)
    src = np.stack([surface(400, rng) for _ in range(3)]).astype(np.float32)
    ref = np.stack([surface(500, rng) for _ in range(3)]).astype(np.float32)
    src[0, 5] = np.nan; src[0, 6, 1] = np.inf; src[0, 7, 2] = -np.inf
    ref[0, 10] = np.nan; ref[0, 11, 0] = np.inf; ref[0, 12, 2] = -np.inf; ref[0, 0, 1] = np.nan
    ref[1] = np.nan                                              # a pair with no finite reference point
    ref[1, 3] = [np.inf, 0, 0]
    src[2] = np.inf                                              # and one with no finite query
    idx = _check_step(eng, src, ref, np.stack([_pose(rng), _pose(rng), _eye(1)[0]]), 0.05, "non-finite")
    assert (idx[0, 5:8] == -1).all() and (idx[0] >= 0).sum() > 100 and not np.isin(idx[0], [0, 10, 11, 12]).any()
    assert (idx[1:] == -1).all()


def test_gpu_grid_step_coordinates_offset_by_1e5(eng):
    rng = np.random.default_rng(13)
    src = (np.stack([surface(1500, rng) for _ in range(2)]) + 1e5).astype(np.float32)
    ref = (np.stack([surface(1500, rng) for _ in range(2)]) + 1e5).astype(np.float32)
    T = _eye(2)
    T[1, :, 3] = [0.0625, -0.03125, 0]
    idx = _check_step(eng, src, ref, T, 0.05, "1e5")
    assert 0.1 < (idx >= 0).mean() < 0.99


# ------------------------------------------------------------------ 2. the loop
def _loop_batch():
    """P = 3 at J = K = 1024: a surface pair 3 degrees off (point-to-point: 10 updates on the host, test_icp_plane), a pair that is
    converged at the start (src == ref, T0 = identity: its `skip` flag is set from the second iteration on), a flat target (the
    plane estimator's system is singular)"""
    a, b, f = surface_case(1024, 1024, 7), surface_case(1024, 1024, 9), flat_case(1024, 1024)
    src = np.stack([a["src"], b["ref"], f["src"]])
    ref = np.stack([a["ref"], b["ref"], f["ref"]])
    T0 = np.stack([a["T0"], np.eye(3, 4, dtype=np.float32), f["T0"]])
    normals = np.stack([a["normals"], b["normals"], f["normals"]])
    return src, ref, T0, normals


def _refine(eng, src, ref, T0, normals, estimator, search, **kw):
    extra = dict(estimator="plane", normals_ref=_dev(normals)) if estimator == "plane" else {}
    T, st = eng.icp_refine(_dev(src), _dev(ref), _dev(T0), RADIUS, search=search, **extra, **kw)
    return T.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("estimator", ["point", "plane"])
@pytest.mark.parametrize("max_iter", [2, 30])
def test_gpu_grid_loop_equals_brute_loop(eng, estimator, max_iter):
    src, ref, T0, normals = _loop_batch()
    T_b, st_b = _refine(eng, src, ref, T0, normals, estimator, "brute", max_iter=max_iter)
    T_g, st_g = _refine(eng, src, ref, T0, normals, estimator, "grid", max_iter=max_iter)
    print(f"LOOP {estimator} max_iter={max_iter}: iterations {st_g[:, 3].tolist()} converged {st_g[:, 2].tolist()} fitness {st_g[:, 0].tolist()}")
    assert st_g.shape == st_b.shape == (3, 4 if estimator == "point" else 5)
    assert T_g.tobytes() == T_b.tobytes() and st_g.tobytes() == st_b.tobytes()
    assert np.isfinite(T_g).all() and st_g[1, 2] == 1.0 and st_g[1, 3] == 1.0 and st_g[1, 0] == 1.0     # converged at the start
    if max_iter == 2:
        assert st_g[0, 2] == 0.0 and st_g[0, 3] == 2.0                                                   # stopped on max_iter
    else:
        assert st_g[0, 2] == 1.0 and 2 <= st_g[0, 3] < 30                                                # converged early


def test_gpu_four_c_entries_agree(eng):
    """dsir_icp_refine, dsir_icp_refine_ex, dsir_icp_refine_ex2 (search 0 and 1) and dsir_icp_correspondences (search 0 and 1), called
    through the C ABI on the same input, write the same bytes: P = 2, J = 300 (no multiple of 64 or 256), K = 257 (no multiple of
    the brute kernel's four support slices), rows of 6 columns whose columns 3..5 carry the normals, max_iter 5."""
    import torch
    P, J, K, max_iter = 2, 300, 257, 5
    cases = [surface_case(J, K, seed) for seed in (7, 9)]
    src = _dev(np.stack([np.c_[c["src"], np.zeros((J, 3), np.float32)] for c in cases]))
    ref = _dev(np.stack([np.c_[c["ref"], c["normals"]] for c in cases]))
    T0 = _dev(np.stack([c["T0"] for c in cases]))
    assert tuple(src.shape) == (P, J, 6) and tuple(ref.shape) == (P, K, 6)

    def refine(name, cols, *tail):
        T = torch.zeros((P, 3, 4), dtype=torch.float32, device="cuda")
        st = torch.full((P, cols), -1.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc = getattr(eng.lib, name)(eng.h, src.data_ptr(), ref.data_ptr(), P, J, K, 6, float(RADIUS), max_iter, 1e-6, 1e-6, T0.data_ptr(),
                                    T.data_ptr(), *tail, st.data_ptr())
        eng.sync()
        assert rc == 0, (name, tail, eng.lib.dsir_last_error(eng.h))
        return T, T.cpu().numpy(), st.cpu().numpy()

    T_dev, T_ref, st_ref = refine("dsir_icp_refine", 4)
    print(f"ENTRIES point: stats {st_ref.tolist()}")
    assert (st_ref[:, 0] > 0).all() and np.isfinite(T_ref).all()                                # not a comparison of empty sets
    for name, tail in (("dsir_icp_refine_ex", (0, None)), ("dsir_icp_refine_ex2", (0, None, 0)), ("dsir_icp_refine_ex2", (0, None, 1))):
        _, T, st = refine(name, 5, *tail)
        assert T.tobytes() == T_ref.tobytes() and st[:, :4].tobytes() == st_ref.tobytes(), (name, tail)
    _, T_pl, st_pl = refine("dsir_icp_refine_ex", 5, 1, None)
    print(f"ENTRIES plane: stats {st_pl.tolist()}")
    assert (st_pl[:, 0] > 0).all() and np.isfinite(T_pl).all()
    for search in (0, 1):
        _, T, st = refine("dsir_icp_refine_ex2", 5, 1, None, search)
        assert T.tobytes() == T_pl.tobytes() and st.tobytes() == st_pl.tobytes(), search

    def corr(search):
        idx = torch.full((P, J), -7, dtype=torch.int32, device="cuda")
        d2 = torch.full((P, J), -1.0, dtype=torch.float32, device="cuda")
        st = torch.full((P, 2), -1.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc = eng.lib.dsir_icp_correspondences(eng.h, src.data_ptr(), ref.data_ptr(), P, J, K, 6, float(RADIUS), T_dev.data_ptr(), search,
                                              idx.data_ptr(), d2.data_ptr(), st.data_ptr())
        eng.sync()
        assert rc == 0, (search, eng.lib.dsir_last_error(eng.h))
        return idx.cpu().numpy(), d2.cpu().numpy(), st.cpu().numpy()

    b, g = corr(0), corr(1)
    print(f"ENTRIES correspondences: stats {b[2].tolist()}")
    assert (b[2][:, 0] > 0).all() and (b[0] >= 0).any(axis=1).all()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(b, g))


# ------------------------------------------------------------------ 3. determinism
def test_gpu_grid_two_runs_and_batch_independence(eng):
    src, ref, T0, normals = _loop_batch()
    for estimator in ("point", "plane"):
        T_a, st_a = _refine(eng, src, ref, T0, normals, estimator, "grid", max_iter=6)
        T_b, st_b = _refine(eng, src, ref, T0, normals, estimator, "grid", max_iter=6)
        assert T_a.tobytes() == T_b.tobytes() and st_a.tobytes() == st_b.tobytes()
        for p in range(3):
            T_1, st_1 = _refine(eng, src[p:p + 1], ref[p:p + 1], T0[p:p + 1], normals[p:p + 1], estimator, "grid", max_iter=6)
            assert T_1.tobytes() == T_a[p:p + 1].tobytes() and st_1.tobytes() == st_a[p:p + 1].tobytes()
    a = _corr(eng, src, ref, T0, RADIUS, "grid")
    b = _corr(eng, src, ref, T0, RADIUS, "grid")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for p in range(3):
        one = _corr(eng, src[p:p + 1], ref[p:p + 1], T0[p:p + 1], RADIUS, "grid")
        assert all(x.tobytes() == y[p:p + 1].tobytes() for x, y in zip(one, a))


def test_gpu_auto_equals_brute_on_both_sides_of_the_threshold(eng):
    from deepsir_amd.engine import Engine
    assert Engine.ICP_GRID_MIN_REF & (Engine.ICP_GRID_MIN_REF - 1) == 0            # a power of two
    assert eng._icp_search("auto", Engine.ICP_GRID_MIN_REF) == 1 and eng._icp_search("auto", Engine.ICP_GRID_MIN_REF - 1) == 0
    assert eng._icp_search("brute", 1 << 20) == 0 and eng._icp_search("grid", 1) == 1
    rng = np.random.default_rng(14)
    eng.ICP_GRID_MIN_REF = 1024                                                     # this engine only: both sides within 4096 points
    try:
        for K in (1023, 1024):
            src, ref = surface(900, rng).astype(np.float32)[None], surface(K, rng).astype(np.float32)[None]
            T0 = _pose(rng)[None]
            assert eng._icp_search("auto", K) == int(K >= 1024)
            T_a, st_a = _refine(eng, src, ref, T0, None, "point", "auto", max_iter=5)
            T_b, st_b = _refine(eng, src, ref, T0, None, "point", "brute", max_iter=5)
            assert T_a.tobytes() == T_b.tobytes() and st_a.tobytes() == st_b.tobytes()
            a, b = _corr(eng, src, ref, T0, RADIUS, "auto"), _corr(eng, src, ref, T0, RADIUS, "brute")
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    finally:
        del eng.ICP_GRID_MIN_REF


# ------------------------------------------------------------------ 4. bad arguments
def test_gpu_grid_bad_arguments(eng):
    from deepsir_amd.engine import EngineError
    rng = np.random.default_rng(15)
    src, ref, T0 = _dev(surface(100, rng)[None]), _dev(surface(120, rng)[None]), _dev(_eye(1))
    with pytest.raises(ValueError):
        eng.icp_refine(src, ref, T0, RADIUS, search="nope")
    with pytest.raises(ValueError):
        eng.icp_correspondences(src, ref, T0, RADIUS, search="kd")
    with pytest.raises(EngineError):
        eng.icp_refine(src, ref, T0, 1e20, search="grid")                          # fl(r r) = inf: no lattice for it
    with pytest.raises(EngineError):
        eng.icp_correspondences(src, ref, T0, 1e20, search="grid")
    idx, _, st = eng.icp_correspondences(src, ref, T0, 1e20, search="brute")        # the brute search takes it, as before
    assert (idx.cpu().numpy() >= 0).all() and st.cpu().numpy()[0, 0] == 1.0
    T, st = eng.icp_refine(src, ref, T0, RADIUS, search="grid", max_iter=1)         # the engine still serves after the refusals
    assert np.isfinite(T.cpu().numpy()).all()
