"""dsir_fpfh (csrc/fpfh.hip) through Engine.fpfh and the C ABI, against the host restatement deepsir_amd/fpfh.py: bytes of the
descriptors and the flags on every point outside the host rule's ambiguity band (tests/fpfh_cases.py; the band's share is capped
at 1 % per case and is 0 on the committed seeds), both list forms, degenerate rows, refused calls, determinism, the pyramid and
radius routes at n = 1024, and harness.register_fpfh on the pair whose pose the host chain recovers in tests/test_fpfh_host.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import fpfh_cases as K
from deepsir_amd import fpfh as F
from deepsir_amd.metrics import THRESHOLDS, rte_rre

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    from deepsir_amd.weights import generate_state_dict
    cfg = NetConfig()
    e = Engine(cfg, max_points=2048, max_pairs=2)
    e.load_state_dict(generate_state_dict(cfg, 0))          # the pyramid and the search refuse a context without weights
    yield e
    e.close()


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def _compare(desc, flags, host, what):
    """bytes of desc and flags outside the band; the band under the cap per cloud; the padding columns +0 everywhere"""
    keep = ~host["band"]
    for c in range(keep.shape[0]):
        assert 1.0 - keep[c].mean() <= K.BAND_CAP, (what, c, 1.0 - keep[c].mean())
    d, h = _bits(desc), _bits(host["desc"])
    assert d.shape == h.shape, (what, d.shape, h.shape)
    bad = np.nonzero((d != h).any(2) & keep)
    assert bad[0].size == 0, (what, "rows", list(zip(*bad))[:8])
    assert np.array_equal(flags.cpu().numpy()[keep], host["flags"][keep]), what
    assert not d[:, :, F.DIM:].any(), what


@pytest.mark.parametrize("out_ld", [33, 64])
@pytest.mark.parametrize("n", K.FIXED_SIZES)
def test_fixed_lists(eng, n, out_ld):
    pts, nrm, nb, _ = K.fixed_case(n)
    desc, flags = eng.fpfh(_cuda(pts), _cuda(nrm), neigh_multi=_cuda(nb), pad_to=out_ld)
    _compare(desc, flags, F.fpfh_host(pts, nrm, neigh=nb, out_ld=out_ld), f"n={n} out_ld={out_ld}")


def test_csr_lists(eng):
    pts, nrm, off, cols = K.csr_case()
    host = F.fpfh_host(pts, nrm, csr=(off, cols))
    desc, flags = eng.fpfh(_cuda(pts), _cuda(nrm), csr=(_cuda(off), _cuda(cols)))
    _compare(desc, flags, host, "csr")
    deg = np.diff(off)
    assert set(K.CSR_DEGREES) == set(deg.tolist()) and flags.cpu().numpy()[0][deg <= 1].all()


def test_degenerate_rows_and_clamped_indices(eng):
    pts, nrm, nb, rows = K.degenerate_case()
    n = pts.shape[1]
    nb = nb.copy()
    nb[0, 20, 5], nb[0, 21, 6], nb[0, 22, 0] = -1, n, 2 ** 31 - 1
    host = F.fpfh_host(pts, nrm, neigh=nb)
    desc, flags = eng.fpfh(_cuda(pts), _cuda(nrm), neigh_multi=_cuda(nb))
    _compare(desc, flags, host, "degenerate")
    f = flags.cpu().numpy()[0]
    dead = [rows["zero_normal"], rows["nan"], rows["self"], rows["inf_normal"]]
    assert f[dead].all() and f.sum() == len(dead) and not _bits(desc)[0][dead].any() and torch.isfinite(desc).all()
    # normals from columns 3..5 against the same normals passed separately
    rows6 = np.concatenate([pts, nrm, np.full((1, n, 1), 7.0, np.float32)], 2)
    d6, f6 = eng.fpfh(_cuda(rows6), None, neigh_multi=_cuda(nb))
    assert np.array_equal(_bits(d6), _bits(desc)) and torch.equal(f6, flags)


def test_refused_calls_launch_nothing(eng):
    pts, nrm, nb, _ = K.fixed_case(17)
    p, v, l = _cuda(pts), _cuda(nrm), _cuda(nb)
    off = torch.arange(0, 3 * 17 * 16 + 1, 16, dtype=torch.int32).cuda()
    desc = torch.full((3, 17, 64), -5.0, device="cuda")
    torch.cuda.synchronize()

    def call(normals, neigh, o, c, stride=3, points=p):
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        return eng.lib.dsir_fpfh(eng.h, ptr(points), stride, ptr(normals), ptr(neigh), 17 * 16, ptr(o), ptr(c), 3, 17, ptr(desc), 64, None)

    assert call(v, l, off, l) != 0 and b"exactly one" in eng.lib.dsir_last_error(eng.h)
    assert call(v, None, None, None) != 0 and b"exactly one" in eng.lib.dsir_last_error(eng.h)
    assert call(v, None, off, None) != 0
    assert call(None, l, None, None) != 0 and b"6 columns" in eng.lib.dsir_last_error(eng.h)
    eng.sync()
    assert (desc == -5.0).all()
    from deepsir_amd.engine import EngineError
    for kw in ({}, {"neigh_multi": l, "csr": (off, l.reshape(-1))}):
        with pytest.raises(EngineError):
            eng.fpfh(p, v, **kw)
    with pytest.raises(EngineError):
        eng.fpfh(p, None, neigh_multi=l)
    with pytest.raises(EngineError):                        # offsets that leave cols
        eng.fpfh(p, v, csr=(off, l.reshape(-1)[:100].contiguous()))
    assert call(v, l, None, None) == 0                      # and the same buffers are accepted once the call is well formed
    eng.sync()
    assert (desc != -5.0).all()


def test_two_runs_and_a_cloud_alone_write_the_same_bytes(eng):
    pts, nrm, nb, _ = K.fixed_case(257)
    p, v, l = _cuda(pts), _cuda(nrm), _cuda(nb)
    d0, f0 = eng.fpfh(p, v, neigh_multi=l)
    d1, f1 = eng.fpfh(p, v, neigh_multi=l)
    assert np.array_equal(_bits(d0), _bits(d1)) and torch.equal(f0, f1)
    for k in range(3):
        dk, fk = eng.fpfh(p[k:k + 1].contiguous(), v[k:k + 1].contiguous(), neigh_multi=l[k:k + 1].contiguous())
        assert np.array_equal(_bits(dk)[0], _bits(d0)[k]) and torch.equal(fk[0], f0[k]), k
    cp, cn, off, cols = K.csr_case()
    two = (np.concatenate([cp, cp[:, ::-1]], 0), np.concatenate([cn, cn[:, ::-1]], 0))
    n = cp.shape[1]
    # the second cloud: the first one's rows reversed, its lists with them
    deg = np.diff(off)
    rcols = np.concatenate([n - 1 - cols[off[i]:off[i + 1]] for i in range(n - 1, -1, -1)]).astype(np.int32)
    off2 = np.concatenate([off, off[-1] + np.cumsum(deg[::-1])]).astype(np.int32)
    dd, _ = eng.fpfh(_cuda(two[0]), _cuda(two[1]), csr=(_cuda(off2), _cuda(np.concatenate([cols, rcols]))))
    da, _ = eng.fpfh(_cuda(cp), _cuda(cn), csr=(_cuda(off), _cuda(cols)))
    assert np.array_equal(_bits(dd)[0], _bits(da)[0])
    host = F.fpfh_host(two[0], two[1], csr=(off2, np.concatenate([cols, rcols])))
    assert np.array_equal(_bits(dd)[~host["band"]], _bits(host["desc"])[~host["band"]])


def test_pyramid_and_radius_routes(eng):
    n = 1024
    pts = K.pair()["points_ref"]
    x = _cuda(pts)
    _, neigh, _, _ = eng.knn_pyramid(x)
    normals, nflags = eng.estimate_normals(x, neigh, (1.5, 1.5, 10.0))
    assert not nflags.any()
    desc, flags = eng.fpfh(x, normals, neigh_multi=neigh)
    nv = normals.cpu().numpy()
    _compare(desc, flags, F.fpfh_host(pts, nv, neigh=neigh[:, :n].cpu().numpy()), "pyramid route")
    assert not flags.any()
    eye = torch.eye(3, 4, device="cuda")[None].contiguous()
    off, cols = eng.radius_matches(x, x, eye, 0.25)
    assert off.numel() == n + 1 and int(off[-1]) == cols.numel() > 16 * n
    desc_r, flags_r = eng.fpfh(x, normals, csr=(off, cols))
    _compare(desc_r, flags_r, F.fpfh_host(pts, nv, csr=(off.cpu().numpy(), cols.cpu().numpy())), "radius route")


def _device_inputs(eng, pr):
    """the 16-NN lists and normals the device makes for the pair: what the host chain is fed, so that only the FPFH rule, the
    arg-min and RANSAC are compared"""
    lists, normals = [], []
    for side in ("src", "ref"):
        x = _cuda(pr["points_" + side])
        _, neigh, _, _ = eng.knn_pyramid(x)
        nv, _ = eng.estimate_normals(x, neigh, tuple(float(t) for t in pr["viewpoint_" + side].reshape(-1)))
        lists.append(neigh[0, :x.shape[1]].cpu().numpy())
        normals.append(nv[0].cpu().numpy())
    return lists, normals


def test_register_fpfh(eng):
    from deepsir_amd.harness import evaluate_align, register_fpfh
    pr, pr2 = K.pair(), F.bumpy_pair(K.PAIR_SEED + 1)       # the second pair has other viewpoints: the per-cloud normals branch
    kw = dict(voxel_size=K.PAIR_VOXEL, hypotheses=K.PAIR_HYPOTHESES, mutual=True, seed=0, want_corr=True)
    alone, stats, corr1 = register_fpfh([pr], eng, num_reg=2, batch=1, **kw)
    both, stats2, corr2 = register_fpfh([pr, pr2], eng, num_reg=2, batch=2, **kw)
    assert alone.shape == (1, 2, 3, 4) and both.shape == (2, 2, 3, 4) and stats.shape == (1, 5) and stats2.shape == (2, 5)
    assert np.array_equal(_bits(alone[0]), _bits(both[0])) and np.array_equal(alone[:, 0], alone[:, 1])
    rte_t, rre_t = THRESHOLDS["3DMatch"]
    for pair, p, T, st, (corr, fs, fr) in ((pr, 0, alone[0, 0], stats[0], corr1[0]), (pr, 0, both[0, 0], stats2[0], corr2[0]),
                                           (pr2, 1, both[1, 0], stats2[1], corr2[1])):
        succ, rte, rre = rte_rre(T, pair["transform_gt"][0], rte_t, rre_t)
        assert succ == 1.0 and st[0] == 1.0 and st[3] > 0, (rte, rre)
        lists, normals = _device_inputs(eng, pair)
        host = F.host_chain(pair, K.PAIR_VOXEL, K.PAIR_HYPOTHESES, seed=0, p=p, lists=lists, normals=normals)
        bs, br = host["src"]["band"][0], host["ref"]["band"][0]
        assert bs.mean() <= K.BAND_CAP and br.mean() <= K.BAND_CAP
        keep = lambda c: c[~bs[c[:, 0]] & ~br[c[:, 1]]]
        assert np.array_equal(keep(corr), keep(host["corr"])) and len(corr) > 100
        assert not fs.any() and not fr.any()
        assert rte_rre(host["T"], pair["transform_gt"][0], rte_t, rre_t)[0] == 1.0
    metrics, summary = evaluate_align(both, [pr, pr2], eng)
    assert len(metrics) == 2 and all(np.isfinite(v).all() for v in metrics[-1].values()) and (metrics[-1]["succ"] == 1).all()
    # the radius route registers the pair as well
    rad, st, _ = register_fpfh([pr], eng, radius=0.25, num_reg=1, batch=1, **kw)
    assert rte_rre(rad[0, 0], pr["transform_gt"][0], rte_t, rre_t)[0] == 1.0
