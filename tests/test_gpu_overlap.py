"""Fragment overlap on the device (csrc/overlap.hip, ``Engine.nn_within`` / ``overlap_ratio``): counts and neighbour lists bit for bit
against the float32 restatement (deepsir_amd/overlap.py::nn_within_host), on the smallest shapes that can break the kernel."""
import numpy as np
import pytest
import torch

from deepsir_amd import overlap as O

pytestmark = pytest.mark.gpu

R = 0.03
H = float(np.float32(R)) * (1.0 + 1.0 / 1024.0)      # the lattice's cell edge (csrc/overlap.hip)


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), 0, max_points=8192, max_pairs=2)
    yield e
    e.close()


def surface(n, seed, side=1.5, shift=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2)) * side
    z = 0.2 * np.sin(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1]) + rng.normal(0.0, 0.004, n)
    return (np.concatenate([xy, z[:, None]], 1) + np.asarray(shift)).astype(np.float32)


def pack(frags):
    off = np.concatenate([[0], np.cumsum([len(f) for f in frags])]).astype(np.int64)
    pts = np.concatenate([np.asarray(f, np.float32).reshape(-1, 3) for f in frags]) if off[-1] else np.zeros((0, 3), np.float32)
    return pts, off


def device(eng, frags, jobs, r=R, poses=None, fill=True):
    pts, off = pack(frags)
    jobs = np.asarray(jobs, np.int32).reshape(-1, 2)
    T = None if poses is None else torch.from_numpy(np.ascontiguousarray(poses, np.float32)).cuda()
    counts, nn = eng.nn_within(torch.from_numpy(pts).cuda(), off, jobs, r, poses=T, fill=np.arange(len(jobs)) if fill else None)
    torch.cuda.synchronize()
    return counts.cpu().numpy(), (None if nn is None else [k.cpu().numpy() for k in nn])


def check(eng, frags, jobs, r=R, poses=None):
    """Device == host, bit for bit; -> (counts, nn)."""
    pts, off = pack(frags)
    want_c, want_nn = O.nn_within_host(pts, off, jobs, r, poses)
    got_c, got_nn = device(eng, frags, jobs, r, poses)
    assert got_c.dtype == np.int32 and np.array_equal(got_c, want_c)
    for j, (g, w) in enumerate(zip(got_nn, want_nn)):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (j, np.nonzero(g != w)[0][:5])
    return got_c, got_nn


SIZES = [0, 1, 63, 64, 65, 1000, 2500]


@pytest.fixture(scope="module")
def ragged():
    frags = [surface(n, 10 + i) for i, n in enumerate(SIZES)]
    jobs = [(a, b) for a in range(len(SIZES)) for b in range(len(SIZES))]
    return frags, jobs


def test_ragged_store_all_ordered_pairs(eng, ragged):
    frags, jobs = ragged
    counts, nn = check(eng, frags, jobs)
    assert counts.sum() > 2000 and any((k < 0).any() for k in nn)          # matches and misses both occur
    # count mode equals the tally of fill mode; two runs give the same bytes
    c2, none = device(eng, frags, jobs, fill=False)
    assert none is None and np.array_equal(c2, [(k >= 0).sum() for k in nn])
    c3, nn3 = device(eng, frags, jobs)
    assert c3.tobytes() == counts.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(nn, nn3))
    # a job alone writes the bytes it writes inside the full list
    for j in (jobs.index((6, 5)), jobs.index((5, 6)), jobs.index((4, 6)), jobs.index((6, 0))):
        c1, nn1 = device(eng, frags, [jobs[j]])
        assert c1[0] == counts[j] and nn1[0].tobytes() == nn[j].tobytes()


def test_self_and_copies_shifted_by_the_radius(eng):
    a = surface(1000, 3)
    r32 = np.float32(R)
    shifts = [r32, np.nextafter(r32, np.float32(0)), np.nextafter(r32, np.float32(1))]
    frags = [a] + [a + np.array([s, 0, 0], np.float32) for s in shifts]
    counts, nn = check(eng, frags, [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (2, 0), (3, 0)])
    assert counts[0] == 1000 and np.array_equal(nn[0], np.arange(1000))


def test_cell_faces_corners_and_targets_1_9_cells_away(eng):
    # an anchor at the origin pins the lattice; queries on cell faces and corners (k h rounded to fp32, and one ulp to either side)
    k = np.array([1, 2, 3, 17, 40], np.float64)
    on = (k * H).astype(np.float32)
    vals = np.concatenate([on, np.nextafter(on, np.float32(0)), np.nextafter(on, np.float32(10))])
    g = np.stack(np.meshgrid(vals, vals[:6], vals[:4], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    q = np.concatenate([np.zeros((1, 3), np.float32), g])
    rng = np.random.default_rng(5)
    d = rng.standard_normal((len(g), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    near = (g + d * (R * rng.choice([0.5, 0.98, 0.9999, 1.0001, 1.02], len(g)))[:, None]).astype(np.float32)
    axis = np.eye(3)[rng.integers(0, 3, len(g))]
    far = (g + axis * (1.9 * H)).astype(np.float32)         # 1.9 cells along one axis: inside the 27 cells or just out, never a match
    t = np.concatenate([np.zeros((1, 3), np.float32), np.abs(near)])
    counts, nn = check(eng, [q, t, np.concatenate([np.zeros((1, 3), np.float32), np.abs(far)])], [(0, 1), (1, 0), (0, 2), (2, 0)])
    assert counts[0] > 0 and counts[1] < len(t) and counts[2] < len(q)          # matches and misses both occur
    # against the far targets only the anchors (and grid points that are 1.9 h from ANOTHER grid point's target) may match: check by distance
    pts_far = np.concatenate([np.zeros((1, 3), np.float32), np.abs(far)])
    hit = nn[2] >= 0
    dist = np.linalg.norm(pts_far[nn[2][hit]].astype(np.float64) - q[hit].astype(np.float64), axis=1)
    assert (dist < R * (1 + 1e-6)).all()
    own = np.linalg.norm(pts_far[1:].astype(np.float64) - g.astype(np.float64), axis=1)
    assert (own > 1.8 * H).all() and not (nn[2][1:] == np.arange(1, len(q))).any()


@pytest.mark.parametrize("shift", [(50.0, -50.0, 50.0), (-50.0, 50.0, -50.0), (-3.0, -2.0, -1.0)])
def test_offset_and_negative_coordinates(eng, shift):
    frags = [surface(1500, 21, shift=shift), surface(1400, 22, shift=shift)]
    counts, _ = check(eng, frags, [(0, 1), (1, 0)])
    assert counts.min() > 100


def test_disjoint_boxes_duplicates_and_non_finite_rows(eng):
    a, b = surface(700, 31), surface(900, 32)
    far = surface(300, 33, shift=(40.0, 0.0, 0.0))
    dup = np.concatenate([b, b[:200], b[100:300]])                        # duplicated targets: the lower index wins
    a_bad, b_bad = a.copy(), b.copy()
    a_bad[5], a_bad[640] = [np.nan, 0.1, 0.1], [0.2, np.inf, 0.1]
    b_bad[7], b_bad[850] = [0.3, 0.3, np.nan], [-np.inf, 0.2, 0.1]
    frags = [a, b, far, dup, a_bad, b_bad]
    jobs = [(0, 2), (2, 0), (2, 1), (0, 3), (3, 0), (3, 3), (4, 5), (5, 4), (4, 1), (0, 5), (4, 4)]
    counts, nn = check(eng, frags, jobs)
    assert counts[0] == counts[1] == counts[2] == 0 and (nn[0] == -1).all()
    assert (nn[3][nn[3] >= 0] < len(b)).all()                            # never the copy at 900 + i
    assert np.array_equal(nn[5][:len(b)], np.arange(len(b))) and (nn[5][len(b):] < len(b)).all()
    assert nn[6][5] == -1 and nn[6][640] == -1 and not np.isin(nn[6], [7, 850]).any()


def test_poses(eng):
    from deepsir_amd import augment as A
    a, b = surface(1200, 41), surface(1300, 42)
    Rm = A.rodrigues(np.array([0.3, -0.5, 0.8]), 0.7)
    T = np.concatenate([Rm, [[0.4], [-1.1], [0.25]]], 1).astype(np.float32)
    src = ((a.astype(np.float64) - T[:, 3].astype(np.float64)) @ T[:, :3].astype(np.float64)).astype(np.float32)   # T src ~ a
    eye = np.eye(4, dtype=np.float32)[:3]
    frags, jobs = [src, b, a], [(0, 1), (2, 1), (0, 1)]
    poses = np.stack([T, eye, eye])
    counts, nn = check(eng, frags, jobs, poses=poses)
    assert counts[0] > 300 and counts[2] < counts[0]
    # the host rule on host-moved points
    moved = O.move_host(T, src)
    want_c, want_nn = O.nn_within_host(*pack([moved, b]), [(0, 1)], R)
    assert counts[0] == want_c[0] and np.array_equal(nn[0], want_nn[0])
    # identity poses equal no poses
    c_eye, nn_eye = device(eng, frags, jobs, poses=np.stack([eye] * 3))
    c_none, nn_none = device(eng, frags, jobs)
    assert c_eye.tobytes() == c_none.tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(nn_eye, nn_none))


def test_count_equals_the_non_empty_rows_of_radius_matches(eng):
    P, n = 3, 2000
    src = np.stack([surface(n, 50 + p) for p in range(P)])
    ref = np.stack([surface(n, 60 + p) for p in range(P)])
    eye = torch.eye(4)[:3].repeat(P, 1, 1).contiguous().cuda()
    off, _cols = eng.radius_matches(torch.from_numpy(src).cuda(), torch.from_numpy(ref).cuda(), eye, R)
    rows = np.diff(off.cpu().numpy().astype(np.int64)).reshape(P, n)
    counts, _ = device(eng, list(src) + list(ref), [(p, P + p) for p in range(P)], fill=False)
    assert np.array_equal(counts, (rows > 0).sum(1)) and counts.min() > 500


def test_overlap_ratio(eng):
    from deepsir_amd import augment as A
    P, J, K = 2, 1500, 1700
    ref = np.stack([surface(K, 70 + p) for p in range(P)])
    T = np.stack([np.concatenate([A.rodrigues(np.array([0.1, 0.9, -0.2]), 0.3 + p), [[0.5], [0.2], [-0.3 * p]]], 1) for p in range(P)]).astype(np.float32)
    src = np.stack([((surface(J, 80 + p).astype(np.float64) - T[p, :, 3]) @ T[p, :, :3].astype(np.float64)).astype(np.float32) for p in range(P)])
    got = eng.overlap_ratio(torch.from_numpy(src).cuda(), torch.from_numpy(ref).cuda(), torch.from_numpy(T).cuda(), R)
    want, _ = O.nn_within_host(*pack(list(src) + list(ref)), [(p, P + p) for p in range(P)], R, poses=T)
    assert got.dtype == np.float64 and got.shape == (P,) and np.array_equal(got, want.astype(np.float64) / J)
    assert 0.2 < got.min() and got.max() < 1.0


def test_refusals_return_the_reason_and_launch_nothing(eng):
    from deepsir_amd import _lib
    lib = _lib.load()
    a = surface(100, 90)
    pts = torch.from_numpy(np.concatenate([a, a])).cuda()
    off = np.array([0, 100, 200], np.int64)
    for r in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            eng.nn_within(pts, off, [(0, 1)], r)
    for bad in ([(0, 2)], [(-1, 0)], [(0, 1), (2, 0)]):
        with pytest.raises(ValueError, match="job index out of range"):
            eng.nn_within(pts, off, bad, R)
    wide = torch.tensor([[0.0, 0.0, 0.0], [0.0, 70000.0, 0.0]]).cuda()          # 0.03 m cells: more than 2^21 of them along y
    with pytest.raises(ValueError, match="2\\^21"):
        eng.nn_within(wide, np.array([0, 1, 2], np.int64), [(0, 1)], R)
    # the C entries themselves: an error code, and the buffers they would have written are untouched
    stream = torch.cuda.current_stream().cuda_stream
    jobs_ok, jobs_bad = np.array([[0, 1]], np.int32), np.array([[0, 2]], np.int32)
    b_ok = np.array([0, 0, 0, 2, 2, 2], np.float32)
    b_wide = np.array([0, 0, 0, 2, 70000, 2], np.float32)
    p = lambda x: x.ctypes.data
    assert lib.dsir_t_nn_within_check(p(off), 2, p(jobs_ok), 1, R, p(b_ok)) is None
    assert b"job index" in lib.dsir_t_nn_within_check(p(off), 2, p(jobs_bad), 1, R, p(b_ok))
    assert b"2^21" in lib.dsir_t_nn_within_check(p(off), 2, p(jobs_ok), 1, R, p(b_wide))
    assert b"radius" in lib.dsir_t_nn_within_check(p(off), 2, p(jobs_ok), 1, 0.0, p(b_ok))
    index = torch.full((int(lib.dsir_t_nn_index_scratch(200, 2)),), 0x5a, dtype=torch.uint8, device="cuda")
    counts = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    nn = torch.full((100,), -7, dtype=torch.int32, device="cuda")
    scratch = torch.full((int(lib.dsir_t_nn_within_scratch(1)),), 0x5a, dtype=torch.uint8, device="cuda")
    for r, b in ((0.0, b_ok), (R, b_wide)):
        assert lib.dsir_t_nn_index_build(stream, pts.data_ptr(), 3, p(off), 2, r, p(b), index.data_ptr()) != 0
    for r, b, jb in ((0.0, b_ok, jobs_ok), (R, b_wide, jobs_ok), (R, b_ok, jobs_bad)):
        assert lib.dsir_t_nn_within(stream, index.data_ptr(), p(off), 2, p(jb), 1, None, r, p(b), counts.data_ptr(), nn.data_ptr(),
                                    scratch.data_ptr()) != 0
    torch.cuda.synchronize()
    assert (index == 0x5a).all() and (scratch == 0x5a).all() and counts.item() == -7 and (nn == -7).all()
    assert lib.dsir_t_nn_index_scratch(-1, 2) == 0 and lib.dsir_t_nn_index_scratch(1 << 31, 2) == 0 and lib.dsir_t_nn_index_scratch(10, 0) == 0
