"""The FPFH rule on the host (deepsir_amd/fpfh.py restates the header of csrc/fpfh.hip): what the rule computes on a plane, its block
sums, its invariance under rigid motion, its skips, and that the host chain FPFH -> mutual arg-min -> RANSAC (deepsir_amd/ransac.py)
recovers the pose of the pair the GPU test registers.  Also: the ambiguity band of every input tests/test_gpu_fpfh.py compares
bytes on stays under the cap, and the C ABI declares dsir_fpfh."""
import numpy as np
import pytest

import fpfh_cases as K
from deepsir_amd import fpfh as F
from deepsir_amd.metrics import THRESHOLDS, rte_rre


def _qualifies(points, neigh, r):
    """Rows whose blocks sum to 200: the point and at least one neighbour (at L2 > 0) have a valid pair.  One cloud."""
    p = points[0, :, :3].astype(np.float64)
    n = p.shape[0]
    nb = np.clip(neigh[0], 0, n - 1)
    with np.errstate(all="ignore"):
        L2 = ((p[nb] - p[:, None, :]) ** 2).sum(-1)
        return (r["valid"][0] > 0) & ((L2 > 0) & (r["valid"][0][nb] > 0)).any(1)


def test_plane():
    g = np.arange(12, dtype=np.float64) * 0.1
    pts = np.stack([*np.meshgrid(g, g, indexing="ij"), np.zeros((12, 12))], -1).reshape(-1, 3).astype(np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (144, 1))
    nb = F.knn_lists(pts)
    r = F.fpfh_host(pts[None], nrm[None], neigh=nb[None])
    has = r["valid"][0] > 0
    assert has.all() and not r["flags"].any()
    want = np.zeros(33)
    want[[5, 16, 27]] = 100.0
    assert np.array_equal(F.spfh_values(r["counts"][0], r["valid"][0])[has], np.tile(want, (has.sum(), 1)))
    assert np.array_equal(r["desc"][0][has][:, :33], np.tile(2 * want, (has.sum(), 1)).astype(np.float32))
    assert not r["desc"][0][:, 33:].any() and r["desc"].shape == (1, 144, 64)


@pytest.mark.parametrize("which", ["surface", "degenerate", "csr"])
def test_block_sums(which):
    if which == "csr":
        pts, nrm, off, cols = K.csr_case()
        r = F.fpfh_host(pts, nrm, csr=(off, cols))
        p = pts[0].astype(np.float64)
        ok = np.zeros(pts.shape[1], bool)
        for i in range(pts.shape[1]):
            j = cols[off[i]:off[i + 1]]
            ok[i] = r["valid"][0, i] > 0 and bool(((((p[j] - p[i]) ** 2).sum(1) > 0) & (r["valid"][0][j] > 0)).any())
    else:
        pts, nrm, nb = K.degenerate_case()[:3] if which == "degenerate" else (lambda t: (t[0][:1], t[1][:1], t[2][:1]))(K.fixed_case(257))
        r = F.fpfh_host(pts, nrm, neigh=nb)
        ok = _qualifies(pts, nb, r)
    assert ok.sum() > 0.5 * ok.size          # the CSR case has rows of degree 0 and 1 (self alone)
    sums = r["desc64"][0].reshape(-1, 3, 11).sum(2)
    assert np.abs(sums[ok] - 200.0).max() <= 200.0 * 1e-9, np.abs(sums[ok] - 200.0).max()


def _ulp_move(a, rng):
    a = np.asarray(a, np.float32)
    step = rng.integers(-1, 2, a.shape)
    return np.where(step > 0, np.nextafter(a, np.float32(np.inf)), np.where(step < 0, np.nextafter(a, np.float32(-np.inf)), a)).astype(np.float32)


def test_rigid_motion():
    """The descriptor of the moved cloud differs from the original's by at most 4 x the spread that +-1 ulp moves of the fp32 inputs
    (points and normals, before and after the motion) cause in fpfh_host itself; the spread is measured here."""
    n = 256
    pts, nrm = F.jittered_surface(n, 31)
    nb = F.knn_lists(pts)
    rng = np.random.Generator(np.random.Philox(key=5))
    M = F.random_pose(rng)
    mp = (pts.astype(np.float64) @ M[:, :3].T + M[:, 3]).astype(np.float32)
    mn = (nrm.astype(np.float64) @ M[:, :3].T).astype(np.float32)
    base = F.fpfh_host(pts[None], nrm[None], neigh=nb[None])["desc64"][0]
    moved = F.fpfh_host(mp[None], mn[None], neigh=nb[None])["desc64"][0]
    spread = 0.0
    for _ in range(4):
        for (a, b), ref in (((pts, nrm), base), ((mp, mn), moved)):
            got = F.fpfh_host(_ulp_move(a, rng)[None], _ulp_move(b, rng)[None], neigh=nb[None])["desc64"][0]
            spread = max(spread, float(np.abs(got - ref).max()))
    diff = float(np.abs(moved - base).max())
    print(f"RIGID n={n}: spread under +-1 ulp moves {spread:.3e}, moved - original {diff:.3e}")
    assert spread > 0.0 and diff <= 4.0 * spread, (diff, spread)


def test_skips():
    pts, nrm, nb, rows = K.degenerate_case()
    r = F.fpfh_host(pts, nrm, neigh=nb)
    clean_p, clean_n = F.jittered_surface(K.DEGENERATE_N, 777)
    dead = [rows["zero_normal"], rows["nan"], rows["self"], rows["inf_normal"]]
    assert r["flags"][0][dead].all() and not r["desc"][0][dead].any() and r["flags"][0].sum() == len(dead)
    a, b = rows["dup"]                                    # duplicates: the pair between them is skipped, the others count
    bad = np.isin(nb[0], [rows["zero_normal"], rows["nan"], rows["inf_normal"]])
    for i, other in ((a, b), (b, a)):
        assert r["valid"][0, i] == int(((nb[0, i] != i) & (nb[0, i] != other) & ~bad[i]).sum()) > 8 and not r["flags"][0, i]
    # the other rows are unaffected: a row none of whose list entries (nor their lists) touches an edited row equals the clean cloud's
    clean = F.fpfh_host(clean_p[None], clean_n[None], neigh=F.knn_lists(clean_p)[None])
    touched = np.zeros(K.DEGENERATE_N, bool)
    touched[[a, b] + dead] = True
    near = touched | touched[nb[0]].any(1)
    far = ~(near | near[nb[0]].any(1))
    assert far.sum() >= 32
    assert np.array_equal(r["desc"][0][far].view(np.uint32), clean["desc"][0][far].view(np.uint32))
    # a degenerate neighbour contributes nothing, and nothing non-finite leaks into the rows around it
    assert np.isfinite(r["desc"]).all()
    # normals from columns 3..5 are the same rule
    r6 = F.fpfh_host(np.concatenate([pts, nrm], 2), None, neigh=nb, out_ld=33)
    assert np.array_equal(r6["desc"].view(np.uint32), r["desc"][:, :, :33].view(np.uint32))
    with pytest.raises(ValueError):
        F.fpfh_host(pts, nrm)
    with pytest.raises(ValueError):
        F.fpfh_host(pts, None, neigh=nb)


def test_pair_recovers_its_pose_on_the_host_chain():
    pr, out = K.pair(), K.pair_host_chain()
    succ, rte, rre = rte_rre(out["T"], pr["transform_gt"][0], *THRESHOLDS["3DMatch"])
    right = float((pr["perm"][out["corr"][:, 0]] == out["corr"][:, 1]).mean())
    print(f"PAIR seed {K.PAIR_SEED}: {len(out['corr'])} mutual matches, {right:.3f} of them right, rte {rte:.2e} m, rre {rre:.2e} deg")
    assert succ == 1.0 and len(out["corr"]) > 100


def test_band_of_every_gpu_case_is_under_the_cap():
    shares = {}
    for n in K.FIXED_SIZES:
        pts, nrm, nb, counts = K.fixed_case(n)
        band = F.fpfh_host(pts, nrm, neigh=nb)["band"]
        shares[n] = max(float(band[c].mean()) for c in range(3))
    pts, nrm, off, cols = K.csr_case()
    shares["csr"] = float(F.fpfh_host(pts, nrm, csr=(off, cols))["band"].mean())
    shares["degenerate"] = float(F.fpfh_host(*K.degenerate_case()[:2], neigh=K.degenerate_case()[2])["band"].mean())
    out = K.pair_host_chain()
    shares["pair"] = max(float(out[s]["band"].mean()) for s in ("src", "ref"))
    print("BAND shares:", shares)
    assert all(v <= K.BAND_CAP for v in shares.values()), shares


def test_band_marks_the_bin_edges():
    """Anti-parallel normals put f1 on the edge at +-pi between bins 0 and 10: every such pair is in the band."""
    pts = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 0, -1]], np.float32)
    nb = np.array([[0, 1] + [0] * 14, [1, 0] + [1] * 14], np.int32)
    r = F.fpfh_host(pts[None], nrm[None], neigh=nb[None])
    assert r["band"].all() and (r["valid"] == 1).all()


def test_cabi_declares_dsir_fpfh():
    from deepsir_amd import _lib
    assert "dsir_fpfh" in _lib.SYMBOLS and len(_lib.SYMBOLS["dsir_fpfh"][1]) == 13
    assert hasattr(_lib.load(), "dsir_fpfh")
