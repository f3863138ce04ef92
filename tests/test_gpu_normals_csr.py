"""dsir_estimate_normals_csr (csrc/ppf.hip) through ``Engine.estimate_normals(csr=)``: the bytes of the 16-NN entry on the pyramid's own
lists, the analytic cloud over radius and hybrid neighbourhoods against the host rule (deepsir_amd/ppf.py), and short rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_ENGINE = []


def _eng():
    """One engine for the module, with weights loaded (the pyramid of the first test refuses a context without)."""
    if not _ENGINE:
        from deepsir_amd.arch import NetConfig
        from deepsir_amd.engine import Engine
        from deepsir_amd.weights import generate_state_dict
        cfg = NetConfig()
        e = Engine(cfg, max_points=2048, max_pairs=1)
        e.load_state_dict(generate_state_dict(cfg, 1))
        _ENGINE.append(e)
    return _ENGINE[0]


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def normal_filters(pts, normals64, w, viewpoint=(0.0, 0.0, 0.0)):
    """The filters of test_normals_match_the_host_rule, restated: the points a comparison of normals is meaningful on - a separated
    smallest eigenvalue ((l1 - l0) / l2 >= 0.05) and a sign the orientation decides (|cos(n, v - p)| >= 1e-2)."""
    to_v = np.asarray(viewpoint, np.float64)[None] - pts.astype(np.float64)
    cosv = np.abs((normals64 * to_v).sum(1)) / np.linalg.norm(to_v, axis=1)
    return ((w[:, 1] - w[:, 0]) / w[:, 2] >= 0.05) & (cosv >= 1e-2)


def line_angle(a, b):
    """Angle between the lines along a and b, from the cross product (arccos of a dot product near 1 loses half the digits)."""
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs((a * b).sum(1)))


def test_csr_of_the_level_0_lists_gives_the_bytes_of_the_16_nn_entry():
    from deepsir_amd import ppf
    eng = _eng()
    pts = np.stack([ppf.analytic_normals_cloud(1100, 31), ppf.analytic_normals_cloud(1100, 32)])
    pts[1, :16] = np.array([0.25, -1.5, 2.0], np.float32)                    # a degenerate neighbourhood: flags agree too
    d = cu(pts)
    _, neigh, _, _ = eng.knn_pyramid(d)
    want, wflags = eng.estimate_normals(d, neigh, (0.5, -0.25, 9.0))
    want, wflags = want.clone(), wflags.clone()
    n = pts.shape[1]
    cols = neigh[:, :n].reshape(-1).contiguous()                              # 16 per row, in list order, cloud-local
    off = (torch.arange(2 * n + 1, device=cols.device, dtype=torch.int32) * 16).contiguous()
    got, flags = eng.estimate_normals(d, viewpoint=(0.5, -0.25, 9.0), csr=(off, cols))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(flags, wflags)
    assert wflags[1, :16].all() and int(wflags.sum()) == 16


@pytest.mark.parametrize("n,seed,r,max_nn", [(2048, 22, 0.25, 0), (1024, 21, 0.3, 0), (2048, 22, 0.25, 30), (1024, 21, 0.3, 30)])
def test_radius_and_hybrid_normals_match_the_host_rule(n, seed, r, max_nn):
    """The yardstick of test_normals_match_the_host_rule on radius neighbourhoods (rows of 7 - 76 and 3 - 54 entries) and on hybrid ones
    (max_nn = 30): flags equal everywhere; angle <= 1e-5 rad with equal sign on every point with a separated smallest eigenvalue and a
    decided orientation.  The filters leave out 0.63 % (2048, 22) and 0.78 % (1024, 21) of the points, in float64 on the CPU, for
    max_nn = 0 and for max_nn = 30 alike; at most 1 % is asserted."""
    from deepsir_amd import ppf
    eng = _eng()
    pts = ppf.analytic_normals_cloud(n, seed)
    d = cu(pts[None])
    off, cols = eng.radius_neighbors(d, r, max_nn)
    got, flags = eng.estimate_normals(d, csr=(off, cols))
    off, cols = off.cpu().numpy().astype(np.int64), cols.cpu().numpy().astype(np.int64)
    lens = np.diff(off)
    assert lens.min() >= 3 and lens.max() == (30 if max_nn else {2048: 76, 1024: 54}[n])
    want, wflags = ppf.estimate_normals(pts[None], csr=(off, cols))
    p64 = pts.astype(np.float64)
    w = np.zeros((n, 3))
    for i in range(n):
        e = p64[cols[off[i]:off[i + 1]]]
        e = e - e.mean(0)
        w[i] = np.linalg.eigvalsh(e.T @ e)
    keep = normal_filters(pts, want[0].astype(np.float64), w)
    assert 1.0 - keep.mean() <= 0.01, keep.mean()
    np.testing.assert_array_equal(flags.cpu().numpy(), wflags)
    a, b = got[0].cpu().numpy().astype(np.float64), want[0].astype(np.float64)
    ang = line_angle(a, b)
    print(f"normals n={n} r={r} max_nn={max_nn}: max angle on the kept points = {ang[keep].max():.3e} rad, left out {1 - keep.mean():.4f}")
    assert ang[keep].max() <= 1e-5
    assert np.all((a * b).sum(1)[keep] > 0)


def test_rows_under_three_entries_are_flagged_with_zero_normals():
    from deepsir_amd import ppf
    eng = _eng()
    pts = ppf.analytic_normals_cloud(1024, 23)
    pts[0] = [40.0, 0.0, 0.0]                                                 # alone: a row of 1
    pts[1] = [0.0, 40.0, 0.0]; pts[2] = [0.0, 40.05, 0.0]                     # a pair: rows of 2
    pts[3] = [np.nan, 0.0, 0.0]                                               # a non-finite query: an empty row
    d = cu(pts[None])
    off, cols = eng.radius_neighbors(d, 0.3)
    lens = np.diff(off.cpu().numpy())
    assert list(lens[:4]) == [1, 2, 2, 0] and lens[4:].min() >= 3
    got, flags = eng.estimate_normals(d, csr=(off, cols))
    f, g = flags[0].cpu().numpy(), got[0].cpu().numpy()
    assert f[:4].all() and not f[4:].any() and not g[:4].any() and np.isfinite(g).all()
    want, wflags = ppf.estimate_normals(pts[None], csr=(off.cpu().numpy(), cols.cpu().numpy()))
    np.testing.assert_array_equal(f, wflags[0])
    from deepsir_amd.engine import EngineError
    with pytest.raises(EngineError):
        eng.estimate_normals(d)
    with pytest.raises(EngineError):
        eng.estimate_normals(d, eng.knn_pyramid(d)[1], csr=(off, cols))
