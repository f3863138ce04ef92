"""dsir_iss_keypoints (csrc/iss.hip) through Engine.iss_keypoints and the C ABI, against the host restatement deepsir_amd/iss.py on the
cases of tests/iss_cases.py.

Stage 1 (saliency): outside the host rule's band (a ratio within 1e-9 of its gamma; capped at 1 % per case by tests/test_iss_host.py)
the zero / non-zero pattern is equal, and where both are non-zero |s_dev - s_host| <= 1e-9 e1_host + one fp32 ulp of s_host: loose for
fp64 sums of up to 512 terms plus a Jacobi sweep, a hundred times tighter than an fp32 path could meet (measured on an MI355X: every
fp32 saliency of every case equals the host's bits, spread 0; each case prints its figure before it asserts).  Stage 2 (mask, index, counts)
equals iss_select_host applied to the DEVICE's saliency bit for bit, band points included."""
import ctypes as C

import numpy as np
import pytest
import torch

import iss_cases as K
from deepsir_amd import iss as I

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), max_points=4096, max_pairs=2)          # no weights: dsir_iss_keypoints needs none
    yield e
    e.close()


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _dev_csr(csr):
    return _cuda(csr[0]), _cuda(csr[1])


def _run(eng, pts, sal, nms, **kw):
    index, counts, s, mask = eng.iss_keypoints(_cuda(pts), csr_salient=_dev_csr(sal), csr_nms=_dev_csr(nms), **kw)
    return {"index": index.cpu().numpy(), "counts": counts.cpu().numpy(), "saliency": s.cpu().numpy(), "mask": mask.cpu().numpy()}


def _compare(dev, host, nms, what, **kw):
    keep = ~host["band"]
    sd, sh = dev["saliency"], host["saliency"]
    assert np.isfinite(sd).all() and (sd >= 0).all(), what
    assert np.array_equal(sd[keep] > 0, sh[keep] > 0), (what, np.nonzero((sd > 0) != (sh > 0)))
    both = (sd > 0) & (sh > 0)
    err = np.abs(sd[both].astype(np.float64) - sh[both].astype(np.float64))
    bound = 1e-9 * host["eig"][both][:, 0] + np.spacing(sh[both]).astype(np.float64)
    print(what, "max |s_dev - s_host| / e1 =", float((err / host["eig"][both][:, 0]).max()) if both.any() else 0.0)
    assert (err <= bound).all(), (what, float((err - bound).max()))
    sel = I.iss_select_host(sd, nms, **kw)
    for k in ("mask", "index", "counts"):
        assert np.array_equal(dev[k], sel[k]), (what, k)


@pytest.mark.parametrize("name", K.CASE_NAMES)
def test_against_the_host_rule(eng, name):
    pts, sal, nms = K.case(name)
    _compare(_run(eng, pts, sal, nms), K.host(name), nms, name)


def test_other_parameters(eng):
    pts, sal, nms = K.case("fixed257")
    for kw in (dict(gamma_21=0.6, gamma_32=0.5, min_neighbors=5), dict(gamma_21=2.0, gamma_32=2.0, min_neighbors=1), dict(min_neighbors=12)):
        host = I.iss_saliency_host(pts, sal, **kw)
        _compare(_run(eng, pts, sal, nms, **kw), host, nms, str(kw), min_neighbors=kw["min_neighbors"])


def test_degenerate_inputs_give_no_keypoint(eng):
    pts, csr, rows = K.degenerate_case()
    d = _run(eng, pts, csr, csr)
    assert not d["saliency"][1:].any() and not d["mask"][1:].any() and d["counts"][1:].tolist() == [0, 0, 0] and (d["index"][1:] == -1).all()
    assert not d["saliency"][0, rows["touched"]].any()
    a, b = rows["dup"]
    assert d["saliency"][0, a] > 0 and d["saliency"][0, a].view(np.uint32) == d["saliency"][0, b].view(np.uint32) and d["mask"][0, b] == 0
    assert d["counts"][0] > 0
    d = _run(eng, *K.case("fixed4"))                    # every row below min_neighbors
    assert not d["saliency"].any() and not d["counts"].any() and (d["index"] == -1).all()


def test_bad_column_indices_are_clamped(eng):
    pts, sal, nms = K.bad_index_case()
    n = pts.shape[1]
    d = _run(eng, pts, sal, nms)
    clamp = lambda csr: (csr[0], np.clip(csr[1], 0, n - 1))
    e = _run(eng, pts, clamp(sal), clamp(nms))
    for k in d:
        assert np.array_equal(d[k].view(np.uint32), e[k].view(np.uint32)), k
    base = _run(eng, *[(x[:1] if i == 0 else (x[0][:n + 1], x[1][:x[0][n]])) for i, x in enumerate(K.fixed_case(257)[:3])])
    assert not np.array_equal(base["saliency"], d["saliency"])          # the bad entries did change rows 10, 20, 30


def test_two_runs_and_a_cloud_alone_write_the_same_bytes(eng):
    pts, sal, nms, _ = K.fixed_case(1024)
    n = pts.shape[1]
    a, b = _run(eng, pts, sal, nms), _run(eng, pts, sal, nms)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    for c in range(3):
        one = lambda csr: (csr[0][c * n:(c + 1) * n + 1] - csr[0][c * n], csr[1][csr[0][c * n]:csr[0][(c + 1) * n]])
        alone = _run(eng, pts[c:c + 1], one(sal), one(nms))
        for k in a:
            assert np.array_equal(alone[k][0].view(np.uint32), a[k][c].view(np.uint32)), (c, k)


def test_radius_form_equals_csr_form(eng):
    full = K.fixed_case(1024)[0][0]                              # the cloud without padding rows: the cell index bounds its extent
    pts = _cuda(np.stack([full, full[::-1]]))
    by_radius = eng.iss_keypoints(pts, salient_radius=K.R_SALIENT, non_max_radius=K.R_NMS)
    sal, nms = eng.radius_neighbors(pts, K.R_SALIENT, 0), eng.radius_neighbors(pts, K.R_NMS, 0)
    by_csr = eng.iss_keypoints(pts, csr_salient=sal, csr_nms=nms)
    mixed = eng.iss_keypoints(pts, salient_radius=K.R_SALIENT, csr_nms=nms)
    for x, y, z in zip(by_radius, by_csr, mixed):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert int(by_csr[1].sum()) > 0
    host_csr = I.radius_csr_host(pts.cpu().numpy(), K.R_SALIENT)
    assert np.array_equal(sal[0].cpu().numpy(), host_csr[0]) and np.array_equal(sal[1].cpu().numpy(), host_csr[1])


def test_refused_calls_launch_nothing(eng):
    from deepsir_amd.engine import EngineError
    pts, sal, nms = K.case("fixed65")
    p, (so, sc), (no, nc) = _cuda(pts), _dev_csr(sal), _dev_csr(nms)
    out = [torch.full((3, 65), -7.0, device="cuda"), torch.full((3, 65), -7, dtype=torch.int32, device="cuda"),
           torch.full((3, 65), -7, dtype=torch.int32, device="cuda"), torch.full((3,), -7, dtype=torch.int32, device="cuda")]
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(points=p, stride=3, s_off=so, clouds=3, n=65, g21=0.975, g32=0.975, mn=5, counts=out[3]):
        return eng.lib.dsir_iss_keypoints(eng.h, ptr(points), stride, ptr(s_off), ptr(sc), ptr(no), ptr(nc), clouds, n, g21, g32, mn,
                                          ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(counts))

    for kw, word in ((dict(points=None), b"null"), (dict(s_off=None), b"null"), (dict(counts=None), b"null"), (dict(clouds=0), b"clouds"),
                     (dict(n=0), b"n >= 1"), (dict(stride=2), b"stride"), (dict(g21=0.0), b"gamma"), (dict(g32=float("nan")), b"gamma"),
                     (dict(g21=float("inf")), b"gamma"), (dict(g32=-1.0), b"gamma"), (dict(mn=0), b"min_neighbors")):
        assert call(**kw) != 0, kw
        assert word in eng.lib.dsir_last_error(eng.h), (kw, eng.lib.dsir_last_error(eng.h))
    eng.sync()
    assert (out[0] == -7.0).all() and all((o == -7).all() for o in out[1:])
    for kw in (dict(), dict(salient_radius=0.3), dict(salient_radius=0.3, csr_salient=(so, sc), non_max_radius=0.2),
               dict(salient_radius=0.3, non_max_radius=0.2, gamma_21=0.0), dict(salient_radius=0.3, non_max_radius=0.2, gamma_32=float("nan")),
               dict(salient_radius=0.3, non_max_radius=0.2, min_neighbors=0), dict(salient_radius=-1.0, non_max_radius=0.2)):
        with pytest.raises(ValueError) as ei:
            eng.iss_keypoints(p, **kw)
        assert str(ei.value)
    with pytest.raises(EngineError) as ei:                       # offsets that leave cols
        eng.iss_keypoints(p, csr_salient=(so, sc[:10].contiguous()), csr_nms=(no, nc))
    assert str(ei.value)
    assert call() == 0                                           # the same buffers are accepted once the call is well formed
    eng.sync()
    assert (out[0] >= 0).all() and (out[3] >= 0).all()


def test_symbol_is_exported():
    from deepsir_amd import _lib
    lib = C.CDLL(_lib.load()._name)
    assert lib.dsir_iss_keypoints is not None
