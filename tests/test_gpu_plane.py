"""dsir_segment_plane (csrc/plane.hip) through Engine.segment_plane and the C ABI, against the host restatement
deepsir_amd/plane.py on the cases of tests/plane_cases.py.

Without refits every output is the host rule's bit for bit: draws are integers, the fit is fp64 with correctly rounded sqrt and
division on both sides, the score is fp32 with every operation rounded on its own, the pick is an integer key - no tolerance.
With refits two places differ by construction (Jacobi SVD against LAPACK, the order of the fp64 sums), so:
  exact      labels and plane_counts against count_inliers on the DEVICE's planes; stats columns 0 .. 2 against the host's
  measured   device plane against host plane: ANGLE_TOL / D_TOL = 4 x the host refit's largest deviation under +-1 ulp moves of its
             inlier rows (50 draws per case, sizes 65 .. 5000, measured on the CPU: angle 2.3e-10 rad, |delta d| 8.2e-10 m for the
             scenes at the origin; 7.4e-5 rad and 7.4 m at the 1e5 m offset, where one ulp of a coordinate is 7.8 mm)."""
import ctypes as C

import numpy as np
import pytest
import torch

import plane_cases as K
from deepsir_amd import plane as P

pytestmark = pytest.mark.gpu

ANGLE_TOL, D_TOL = 4 * 2.3e-10, 4 * 8.2e-10
ANGLE_TOL_OFFSET, D_TOL_OFFSET = 4 * 7.4e-5, 4 * 7.4


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), max_points=20480, max_pairs=2)          # no weights: dsir_segment_plane needs none
    yield e
    e.close()


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _run(eng, pts, thr, **kw):
    return tuple(t.cpu().numpy() for t in eng.segment_plane(_cuda(pts), thr, **kw))


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(dev, host, what):
    for name, d, h in zip(P.NAMES, dev, host):
        assert d.dtype == h.dtype and d.shape == h.shape, (what, name, d.dtype, h.dtype, d.shape, h.shape)
        assert np.array_equal(_bits(d), _bits(h)), (what, name, np.nonzero(_bits(d) != _bits(h)))


@pytest.mark.parametrize("n", K.SIZES)
def test_without_refits_every_output_is_the_host_rules(eng, n):
    i = 0
    for kind in sorted(K.KINDS):
        for mp in (1, 3):
            for with_axis in (False, True):
                H = K.HYPS[(i + K.SIZES.index(n)) % len(K.HYPS)]
                i += 1
                dev = _run(eng, K.cloud(kind, n)[None], K.thr(kind), hypotheses=H, max_planes=mp, refine_iters=0,
                           **(K.AXIS if with_axis else {}))
                _same(dev, K.host(kind, n, H, mp, with_axis), (kind, n, H, mp, with_axis))
                assert 0 <= dev[1][0] <= mp and dev[0].min() >= -1 and dev[0].max() < max(int(dev[1][0]), 1)


@pytest.mark.parametrize("H", K.HYPS)
def test_every_hypothesis_count_on_the_scene(eng, H):
    for n in (1025, 5000):
        dev = _run(eng, K.cloud("scene", n)[None], K.THR, hypotheses=H, max_planes=3, refine_iters=0)
        _same(dev, K.host("scene", n, H, 3, False), ("scene", n, H))


def _check_against_own_planes(pts, thr, dev, what):
    """labels and plane_counts are count_inliers' on the device's own planes, peeled in order"""
    labels, num, planes, anchors, counts, _ = dev
    for c in range(len(pts)):
        p = pts[c][:, :3]
        live = np.isfinite(p).all(1)
        want = np.full(len(p), -1, np.int32)
        for j in range(int(num[c])):
            m = np.zeros(len(p), bool)
            m[live] = P.inlier_mask(planes[c, j, :3], anchors[c, j], p[live], thr)
            assert int(m.sum()) == int(counts[c, j]) == int(P.count_inliers(planes[c, j, :3], anchors[c, j], p[live], thr)), (what, c, j)
            want[m] = j
            live &= ~m
        assert np.array_equal(labels[c], want), (what, c)
        assert (planes[c, int(num[c]):] == 0).all() and (counts[c, int(num[c]):] == 0).all()


@pytest.mark.parametrize("n", (65, 257, 1025, 5000))
def test_with_refits(eng, n):
    for kind in ("scene", "two_planes", "nonfinite", "offset"):
        pts, thr = K.cloud(kind, n)[None], K.thr(kind)
        for refits in (1, 3):
            dev = _run(eng, pts, thr, max_planes=1, refine_iters=refits, **K.AXIS)
            host = K.host(kind, n, 1024, 1, True, refits)
            _check_against_own_planes(pts, thr, dev, (kind, n, refits))
            assert np.array_equal(dev[5][..., :3], host[5][..., :3]) and dev[1][0] == host[1][0] == 1, (kind, n, refits, dev[5], host[5])
            a, b = dev[2][0, 0].astype(np.float64), host[2][0, 0].astype(np.float64)
            angle, dd = float(np.linalg.norm(np.cross(a[:3], b[:3]))), abs(a[3] - b[3])
            print(f"{kind} n={n} refits={refits}: angle {angle:.3g} rad, |delta d| {dd:.3g} m, kept {dev[5][0, 0, 3]} / {host[5][0, 0, 3]}")
            tol = (ANGLE_TOL_OFFSET, D_TOL_OFFSET) if kind == "offset" else (ANGLE_TOL, D_TOL)
            assert angle <= tol[0] and dd <= tol[1], (kind, n, refits, angle, dd)
        dev = _run(eng, pts, thr, max_planes=3, refine_iters=2, hypotheses=257)
        _check_against_own_planes(pts, thr, dev, (kind, n, "three planes"))
        assert dev[1][0] >= 1 and (dev[5][0, :int(dev[1][0]), 3] <= 2).all()


def test_strided_rows_with_nan_beyond_the_coordinates(eng):
    pts = np.full((2, 700, 6), np.nan, np.float32)
    pts[0, :, :3], pts[1, :, :3] = K.scene(700), K.two_planes(700)
    dev = _run(eng, pts, K.THR, hypotheses=257, max_planes=2, refine_iters=0)
    _same(dev, P.segment_plane_host(pts, K.THR, hypotheses=257, max_planes=2, refine_iters=0), "stride 6")
    assert (dev[1] == 2).all()


def test_ragged_batch_equals_each_cloud_alone_and_cloud_ids(eng):
    from deepsir_amd.harness import pad_clouds
    clouds = [K.scene(65, 1), K.two_planes(1025, 0.6, 2), K.nonfinite_scene(700, 3), K.collinear(40)]
    pad, counts = pad_clouds([_cuda(c) for c in clouds])
    kw = dict(hypotheses=257, max_planes=3, refine_iters=1, seed=12345)
    out = tuple(t.cpu().numpy() for t in eng.segment_plane(pad, K.THR, counts=counts, **kw))
    host0 = P.segment_plane_host(pad.cpu().numpy(), K.THR, counts=counts.cpu().numpy(), **dict(kw, refine_iters=0))
    _same(tuple(t.cpu().numpy() for t in eng.segment_plane(pad, K.THR, counts=counts, **dict(kw, refine_iters=0))), host0, "ragged")
    for i, c in enumerate(clouds):
        n = len(c)
        # the cloud alone, drawing as position i: by cloud_ids, and by the seed of the rule
        by_id = _run(eng, c[None], K.THR, cloud_ids=[i], **kw)
        by_seed = _run(eng, c[None], K.THR, **dict(kw, seed=kw["seed"] ^ (i << 40)))
        for name, b, a, s in zip(P.NAMES, out, by_id, by_seed):
            mine = b[i, :n] if name == "labels" else b[i]
            assert np.array_equal(_bits(mine), _bits(a[0])) and np.array_equal(_bits(a[0]), _bits(s[0])), (name, i)
        assert (out[0][i, n:] == -1).all()
    assert out[1].tolist()[3] == 0 and out[1][1] == 2
    # ids as a tensor reorder the draws with the clouds
    perm = [2, 0, 3, 1]
    pad2, counts2 = pad_clouds([_cuda(clouds[i]) for i in perm])
    out2 = tuple(t.cpu().numpy() for t in eng.segment_plane(pad2, K.THR, counts=counts2, cloud_ids=torch.tensor(perm, dtype=torch.int32), **kw))
    for b, b2 in zip(out, out2):
        assert np.array_equal(_bits(b[perm]), _bits(b2))


def test_two_runs_write_the_same_bytes(eng):
    p = _cuda(np.stack([K.scene(5000), K.lattice(5000), K.offset_scene(5000)]))
    a = eng.segment_plane(p, K.THR, max_planes=4, refine_iters=2)
    b = eng.segment_plane(p, K.THR, max_planes=4, refine_iters=2)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_cloud_that_finishes_at_once_beside_one_that_takes_three_rounds(eng):
    pts = np.stack([K.collinear(1025), K.scene(1025), K.duplicates(1025)])
    dev = _run(eng, pts, K.THR, hypotheses=64, max_planes=3, refine_iters=0)
    _same(dev, P.segment_plane_host(pts, K.THR, hypotheses=64, max_planes=3, refine_iters=0), "finished beside running")
    assert dev[1].tolist() == [0, 3, 0] and (dev[0][[0, 2]] == -1).all() and (dev[5][[0, 2]] == 0).all()
    # the min_inliers stop: the scene's second plane holds fewer rows than the first
    first, second = int(dev[4][1, 0]), int(dev[4][1, 1])
    assert second < first
    stop = _run(eng, pts, K.THR, hypotheses=64, max_planes=3, refine_iters=0, min_inliers=second + 1)
    assert stop[1].tolist() == [0, 1, 0] and (stop[4][1, 1:] == 0).all() and np.array_equal(stop[0] == 0, dev[0] == 0) and (stop[0] <= 0).all()
    # no live row at all is no error
    none = _run(eng, np.full((1, 5, 3), np.nan, np.float32), K.THR)
    assert none[1][0] == 0 and (none[0] == -1).all()
    empty = tuple(t.cpu().numpy() for t in eng.segment_plane(_cuda(pts), K.THR, counts=[0, 2, 1025], hypotheses=64))
    assert empty[1].tolist() == [0, 0, 0]


def test_refused_calls_launch_nothing(eng):
    from deepsir_amd.engine import EngineError
    p = _cuda(K.scene(65)[None].repeat(3, 0))
    out = [torch.full((3, 65), -7, dtype=torch.int32, device="cuda"), torch.full((3,), -7, dtype=torch.int32, device="cuda"),
           torch.full((3, 2, 4), -7.0, device="cuda"), torch.full((3, 2, 3), -7.0, device="cuda"),
           torch.full((3, 2), -7, dtype=torch.int32, device="cuda"), torch.full((3, 2, 4), -7, dtype=torch.int32, device="cuda")]
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(points=p, stride=3, clouds=3, cap=65, thr=0.08, H=64, mp=2, mi=3, ri=1, axis=(0.0, 0.0, 0.0), cos_min=0.0, labels=out[0],
             num=out[1], planes=out[2], anchors=out[3], counts=out[4], stats=out[5]):
        return eng.lib.dsir_segment_plane(eng.h, ptr(points), stride, None, None, clouds, cap, thr, H, mp, mi, ri, axis[0], axis[1], axis[2],
                                          cos_min, 7, ptr(labels), ptr(num), ptr(planes), ptr(anchors), ptr(counts), ptr(stats))

    for kw, word in ((dict(points=None), b"null"), (dict(labels=None), b"null"), (dict(num=None), b"null"), (dict(planes=None), b"null"),
                     (dict(anchors=None), b"null"), (dict(counts=None), b"null"), (dict(stats=None), b"null"),
                     (dict(clouds=0), b"clouds"), (dict(clouds=65536), b"clouds"), (dict(cap=0), b"cap"), (dict(clouds=65535, cap=32769), b"cap"),
                     (dict(stride=2), b"stride"), (dict(H=0), b"hypotheses"), (dict(H=(1 << 20) + 1), b"hypotheses"),
                     (dict(thr=0.0), b"distance_threshold"), (dict(thr=-1.0), b"distance_threshold"), (dict(thr=float("nan")), b"distance_threshold"),
                     (dict(thr=float("inf")), b"distance_threshold"), (dict(mp=0), b"max_planes"), (dict(mp=9), b"max_planes"),
                     (dict(mi=2), b"min_inliers"), (dict(ri=-1), b"refine_iters"), (dict(ri=9), b"refine_iters"),
                     (dict(axis=(float("nan"), 0.0, 1.0)), b"axis"), (dict(cos_min=float("inf")), b"axis"),
                     (dict(clouds=65535, cap=32768), b"workspace")):
        assert call(**kw) != 0, kw
        assert word in eng.lib.dsir_last_error(eng.h), (kw, eng.lib.dsir_last_error(eng.h))
    eng.sync()
    assert all((o == -7).all() for o in out)
    for args, kw, word in (((p, 0.0), {}, "distance_threshold"), ((p, float("nan")), {}, "distance_threshold"), ((p, 0.08), dict(hypotheses=0), "hypotheses"),
                           ((p, 0.08), dict(hypotheses=(1 << 20) + 1), "hypotheses"), ((p, 0.08), dict(max_planes=0), "max_planes"),
                           ((p, 0.08), dict(max_planes=9), "max_planes"), ((p, 0.08), dict(min_inliers=2), "min_inliers"),
                           ((p, 0.08), dict(refine_iters=9), "refine_iters"), ((p, 0.08), dict(refine_iters=1.5), "refine_iters"),
                           ((p, 0.08), dict(seed=-1), "seed"), ((p, 0.08), dict(axis=(0, 0, 0)), "axis"), ((p, 0.08), dict(max_angle_deg=10.0), "axis"),
                           ((p, 0.08), dict(axis=(0, 0, 1), max_angle_deg=91.0), "max_angle_deg"), ((p, 0.08), dict(counts=[1, 2]), "counts"),
                           ((p, 0.08), dict(counts=[1, 2, 66]), "counts"), ((p, 0.08), dict(cloud_ids=[1, 2]), "cloud_ids"),
                           ((p, 0.08), dict(cloud_ids=[1, 2, -1]), "cloud_ids"), ((p[0], 0.08), {}, "points"), ((p[:, :, :2], 0.08), {}, "points")):
        with pytest.raises(ValueError, match=word):
            eng.segment_plane(*args, **kw)
    with pytest.raises(EngineError):
        eng.segment_plane(p.cpu(), 0.08)
    assert call() == 0                                           # the same buffers are accepted once the call is well formed
    eng.sync()
    assert (out[1] >= 1).all() and (out[0] >= -1).all() and (out[4][:, 0] >= 3).all()


def test_symbol_is_exported():
    from deepsir_amd import _lib
    lib = C.CDLL(_lib.load()._name)
    assert lib.dsir_segment_plane is not None
