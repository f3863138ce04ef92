"""dsir_farthest_point_sample (csrc/fps.hip) through Engine.farthest_point_sample and the C ABI, against the host restatement
deepsir_amd/fps.py on the cases of tests/fps_cases.py: index, counts_out and min_d2 bit for bit - the rule is fp32 with every
operation rounded on its own and a total order on the candidates, so there is no tolerance.  Sizes cover the lane, wave and
workgroup edges, both sides of the register / streaming tier edge (8192) and a streaming case."""
import ctypes as C

import numpy as np
import pytest
import torch

import fps_cases as K
from deepsir_amd.fps import farthest_point_sample_host as fps_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), max_points=20480, max_pairs=2)          # no weights: dsir_farthest_point_sample needs none
    yield e
    e.close()


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _run(eng, pts, k, **kw):
    return tuple(t.cpu().numpy() for t in eng.farthest_point_sample(_cuda(pts), k, **kw))


def _same(dev, host, what):
    for name, d, h in zip(("index", "counts_out", "min_d2"), dev, host):
        assert d.dtype == h.dtype and d.shape == h.shape, (what, name)
        assert np.array_equal(d.view(np.uint32), h.view(np.uint32)), (what, name, np.nonzero(d.view(np.uint32) != h.view(np.uint32)))


@pytest.mark.parametrize("n", K.SIZES)
def test_against_the_host_rule(eng, n):
    for kind in sorted(K.KINDS):
        for k in K.ks(n):
            dev = _run(eng, K.cloud(kind, n)[None], k)
            _same(dev, K.host(kind, n, k), (kind, n, k))
            cnt = int(dev[1][0])
            d = dev[2][0, :cnt].astype(np.float64)
            assert cnt == 0 or (np.isposinf(d[0]) and (np.diff(d[1:]) <= 0).all())
            assert len(set(dev[0][0, :cnt].tolist())) == cnt


@pytest.mark.parametrize("n", K.SIZES)
def test_start_rows(eng, n):
    p = K.nonfinite_cloud(n)
    bad = K.nonfinite_rows(n)
    k = min(n, 300)
    for start in sorted({0, n - 1, int(bad[-1]) if len(bad) else 0, n + 3}):        # row 0 is non-finite where n > 1
        _same(_run(eng, p[None], k, start=start), fps_host(p[None], k, start=start), (n, start))
    q = K.random_cloud(n)
    dev = _run(eng, q[None], k, start=n - 1)
    _same(dev, K.host("random", n, k, n - 1), (n, "last"))
    assert dev[0][0, 0] == n - 1


def test_strided_rows_and_a_batch(eng):
    rng = np.random.Generator(np.random.Philox(key=77))
    pts = rng.uniform(-2, 2, (2, 700, 6)).astype(np.float32)       # columns 3..5 are not coordinates
    pts[:, :, 3:] = np.nan
    dev = _run(eng, pts, 128, start=5)
    _same(dev, fps_host(pts, 128, start=5), "stride 6")


@pytest.mark.parametrize("sizes", [(65, 1025, 700), (20000, 5000, 8193)], ids=["register", "streaming"])
def test_ragged_batch_equals_each_cloud_alone(eng, sizes):
    """three clouds through pad_clouds (NaN padding): each gives the bytes of that cloud alone - in the streaming case the capacity
    sits in the streaming tier while one cloud's count (5000) sits in the register range, so the two tiers must agree"""
    from deepsir_amd.harness import pad_clouds
    clouds = [K.random_cloud(n, 20 + i) for i, n in enumerate(sizes)]
    clouds[2] = K.nonfinite_cloud(sizes[2], 5)
    pad, counts = pad_clouds([_cuda(c) for c in clouds])
    k = 300
    index, cnt, d2 = (t.cpu().numpy() for t in eng.farthest_point_sample(pad, k, counts=counts, start=64))
    _same((index, cnt, d2), fps_host(pad.cpu().numpy(), k, counts=counts.cpu().numpy(), start=64), sizes)
    for i, c in enumerate(clouds):
        kk = min(k, len(c))
        alone = _run(eng, c[None], kk, start=64)
        assert cnt[i] == alone[1][0] and np.array_equal(index[i, :kk], alone[0][0]), (sizes, i)
        assert np.array_equal(d2[i, :kk].view(np.uint32), alone[2][0].view(np.uint32)) and (index[i, kk:] == -1).all() and (d2[i, kk:] == 0).all()
    # counts as a sequence, and a count of 0
    z = tuple(t.cpu().numpy() for t in eng.farthest_point_sample(pad, 4, counts=[0, 3, 1]))
    _same(z, fps_host(pad.cpu().numpy(), 4, counts=[0, 3, 1]), "counts 0, 3, 1")
    assert z[1].tolist() == [0, 3, 0] and (z[0][0] == -1).all() and z[0][1, 3] == -1          # cloud 2's only row is not finite


def test_two_runs_write_the_same_bytes(eng):
    for n in (5000, 20000):
        p = _cuda(np.stack([K.duplicate_cloud(n), K.lattice_cloud(n)]))
        a, b = eng.farthest_point_sample(p, 300), eng.farthest_point_sample(p, 300)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_refused_calls_launch_nothing(eng):
    from deepsir_amd.engine import EngineError
    p = _cuda(K.random_cloud(65)[None].repeat(3, 0))
    out = [torch.full((3, 8), -7, dtype=torch.int32, device="cuda"), torch.full((3,), -7, dtype=torch.int32, device="cuda"),
           torch.full((3, 8), -7.0, device="cuda")]
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(points=p, stride=3, clouds=3, cap=65, k=8, start=0, index=out[0], counts_out=out[1], min_d2=out[2]):
        return eng.lib.dsir_farthest_point_sample(eng.h, ptr(points), stride, None, clouds, cap, k, start, ptr(index), ptr(counts_out), ptr(min_d2))

    for kw, word in ((dict(points=None), b"null"), (dict(index=None), b"null"), (dict(counts_out=None), b"null"), (dict(min_d2=None), b"null"),
                     (dict(clouds=0), b"clouds"), (dict(clouds=65536), b"clouds"), (dict(cap=0), b"cap"), (dict(stride=2), b"stride"),
                     (dict(k=0), b"k in"), (dict(k=66), b"k in"), (dict(start=-1), b"start"), (dict(cap=65537, k=8), b"65536"),
                     (dict(cap=65536, clouds=65535), b"workspace")):           # 64 TiB of packed copy: no arena holds it
        assert call(**kw) != 0, kw
        assert word in eng.lib.dsir_last_error(eng.h), (kw, eng.lib.dsir_last_error(eng.h))
    eng.sync()
    assert all((o == -7).all() for o in out)
    for args, kw in (((p, 0), {}), ((p, 66), {}), ((p, 1.5), {}), ((p, 8), dict(start=-1)), ((p, 8), dict(counts=[1, 2])),
                     ((p, 8), dict(counts=[1, 2, 66])), ((p[0], 8), {}), ((p[:, :, :2], 8), {})):
        with pytest.raises(ValueError) as ei:
            eng.farthest_point_sample(*args, **kw)
        assert str(ei.value)
    big = torch.zeros((1, 65537, 3), device="cuda")
    with pytest.raises(ValueError, match="65536"):
        eng.farthest_point_sample(big, 8)
    with pytest.raises(EngineError):
        eng.farthest_point_sample(p.cpu(), 8)
    assert call() == 0                                           # the same buffers are accepted once the call is well formed
    eng.sync()
    assert (out[0] >= 0).all() and (out[1] == 8).all() and torch.isinf(out[2][:, 0]).all()


def test_symbol_is_exported():
    from deepsir_amd import _lib
    lib = C.CDLL(_lib.load()._name)
    assert lib.dsir_farthest_point_sample is not None
