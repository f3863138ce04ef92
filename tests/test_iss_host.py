"""The ISS rule on the host (deepsir_amd/iss.py restates the header of csrc/iss.hip): the vectorised restatement against a plain
per-point loop, the selection's corner cases, the band condition tests/test_gpu_iss.py relies on for every shared case, and the host
chain (host ISS -> host FPFH -> mutual arg-min -> Kabsch on the inliers) on the bumpy pair."""
import numpy as np
import pytest

import iss_cases as K
from deepsir_amd import fpfh as F
from deepsir_amd import iss as I
from deepsir_amd.metrics import THRESHOLDS, rte_rre


def _loop(points, sal, nms, g21=I.GAMMA_21, g32=I.GAMMA_32, mn=I.MIN_NEIGHBORS):
    """the rule, one point at a time"""
    pts = np.asarray(points, np.float32)
    c, n = pts.shape[:2]
    s = np.zeros((c, n), np.float32)
    with np.errstate(all="ignore"):
        for cl in range(c):
            for i in range(n):
                r = cl * n + i
                j = np.clip(sal[1][sal[0][r]:sal[0][r + 1]], 0, n - 1)
                if len(j) < mn:
                    continue
                q = pts[cl, j, :3].astype(np.float64)
                m = q.sum(0) / len(j)
                C = sum(np.outer(v - m, v - m) for v in q) / len(j)
                if not np.isfinite(C).all() or not C.any():
                    continue
                e3, e2, e1 = np.sort(np.abs(np.linalg.eigh(C)[0]))
                if e1 > 0 and e2 > 0 and e2 / e1 < g21 and e3 / e2 < g32:
                    s[cl, i] = np.float32(e3)
    mask = np.zeros((c, n), np.int32)
    for cl in range(c):
        for i in range(n):
            r = cl * n + i
            j = np.clip(nms[1][nms[0][r]:nms[0][r + 1]], 0, n - 1)
            if s[cl, i] > 0 and len(j) >= mn and not (s[cl, j] > s[cl, i]).any() and not ((s[cl, j] == s[cl, i]) & (j < i)).any():
                mask[cl, i] = 1
    return s, mask


@pytest.mark.parametrize("name", ["fixed1", "fixed6", "fixed65", "fixed257", "degree", "degenerate", "bad_index"])
def test_host_rule_against_a_plain_loop(name):
    pts, sal, nms = K.case(name)
    h = K.host(name)
    s, mask = _loop(pts, sal, nms)
    keep = ~h["band"]
    assert np.array_equal(h["saliency"][keep] > 0, s[keep] > 0)
    both = keep & (s > 0)
    assert np.all(np.abs(h["saliency"][both].astype(np.float64) - s[both]) <= 1e-12 * h["eig"][both][:, 0] + np.spacing(s[both]))
    sel = I.iss_select_host(s, nms)             # the selection is exact on a given saliency array
    assert np.array_equal(sel["mask"], mask)
    assert np.array_equal(sel["counts"], mask.sum(1))
    for cl in range(mask.shape[0]):
        k = sel["counts"][cl]
        assert np.array_equal(sel["index"][cl, :k], np.nonzero(mask[cl])[0]) and (sel["index"][cl, k:] == -1).all()


def test_selection_corner_cases():
    n = 8
    full = (np.arange(0, n * n + 1, n, dtype=np.int32), np.tile(np.arange(n, dtype=np.int32), n))
    s = np.array([[0.0, 2.0, 2.0, 1.0, 0.0, 2.0, 0.5, 0.0]], np.float32)
    r = I.iss_select_host(s, full, min_neighbors=5)
    assert r["mask"].tolist() == [[0, 1, 0, 0, 0, 0, 0, 0]] and r["counts"].tolist() == [1] and r["index"][0].tolist() == [1] + [-1] * 7
    assert I.iss_select_host(s, full, min_neighbors=9)["counts"].tolist() == [0]             # |R_i| < min_neighbors
    assert I.iss_select_host(np.zeros((1, n), np.float32), full)["counts"].tolist() == [0]   # s == 0 is never a keypoint
    # disjoint rows: {0..4} and {5..7} (too short); a point only competes inside its own row
    off = np.array([0, 5, 10, 15, 20, 25, 28, 31, 34], np.int32)
    cols = np.concatenate([np.tile(np.arange(5), 5), np.tile(np.arange(5, 8), 3)]).astype(np.int32)
    r = I.iss_select_host(s, (off, cols), min_neighbors=5)
    assert r["mask"].tolist() == [[0, 1, 0, 0, 0, 0, 0, 0]]
    r = I.iss_select_host(s, (off, cols), min_neighbors=3)
    assert r["mask"].tolist() == [[0, 1, 0, 0, 0, 1, 0, 0]] and r["index"][0, :2].tolist() == [1, 5]


def test_duplicates_and_degenerate_clouds():
    pts, csr, rows = K.degenerate_case()
    h = K.host("degenerate")
    a, b = rows["dup"]
    assert h["saliency"][0, a].view(np.uint32) == h["saliency"][0, b].view(np.uint32) and h["saliency"][0, a] > 0
    assert h["mask"][0, b] == 0                                  # the lower index wins a tie; open3d would keep both
    assert not h["saliency"][0, rows["touched"]].any() and len(rows["touched"]) >= 2
    assert not h["saliency"][1:].any() and not h["mask"][1:].any() and h["counts"][1:].tolist() == [0, 0, 0]
    assert h["counts"][0] > 0
    assert (h["eig"][1, :, 2] == 0).all() and (h["eig"][2, :, 1:] == 0).all() and (h["eig"][3] == 0).all()


def test_refused_arguments():
    pts, sal, nms = K.case("fixed6")
    for kw in ({"gamma_21": 0.0}, {"gamma_32": float("nan")}, {"gamma_21": float("inf")}, {"min_neighbors": 0}):
        with pytest.raises(ValueError):
            I.iss_saliency_host(pts, sal, **kw)
    with pytest.raises(ValueError):
        I.iss_saliency_host(pts, (sal[0][:-1], sal[1]))


@pytest.mark.parametrize("name", K.CASE_NAMES)
def test_band_condition(name):
    """a condition on the inputs: the GPU test compares the zero / non-zero pattern outside the band only"""
    h = K.host(name)
    for cl in range(h["band"].shape[0]):
        assert h["band"][cl].mean() <= K.BAND_CAP, (name, cl, h["band"][cl].mean())


def _pair_keypoints(pr):
    out = {}
    for side in ("src", "ref"):
        pts = pr["points_" + side]
        out[side] = I.iss_keypoints_host(pts, I.radius_csr_host(pts, K.PAIR_SALIENT), I.radius_csr_host(pts, K.PAIR_NMS))
    return out


def test_bumpy_pair_keypoint_share_and_host_chain():
    from deepsir_amd import ppf, ransac
    pr = K.pair()
    kp = _pair_keypoints(pr)
    n = pr["points_ref"].shape[1]
    desc, idx = {}, {}
    for side in ("src", "ref"):
        h = kp[side]
        share = h["counts"][0] / n
        assert 0.01 <= share <= 0.5 and h["band"].mean() <= K.BAND_CAP, (side, share)
        pts = pr["points_" + side][0][:, :3]
        nb = F.knn_lists(pts)
        nv = ppf.estimate_normals(pts[None], nb[None], tuple(pr["viewpoint_" + side].reshape(-1)))[0][0]
        idx[side] = h["index"][0, :h["counts"][0]]
        desc[side] = F.fpfh_host(pts[None], nv[None], neigh=nb[None])["desc"][0][idx[side]]
    corr, count = ransac.feature_correspondences(desc["src"], desc["ref"], mutual=True)
    corr = corr[:count]
    s = pr["points_src"][0][idx["src"][corr[:, 0]]].astype(np.float64)
    r = pr["points_ref"][0][idx["ref"][corr[:, 1]]].astype(np.float64)
    gt = pr["transform_gt"][0].astype(np.float64)
    inl = np.linalg.norm(s @ gt[:, :3].T + gt[:, 3] - r, axis=1) < 2.0 * K.PAIR_VOXEL
    assert inl.sum() >= 3, (count, inl.sum())
    s, r = s[inl], r[inl]
    H = (s - s.mean(0)).T @ (r - r.mean(0))
    U, _, Vt = np.linalg.svd(H)
    R = Vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
    T = np.concatenate([R, (r.mean(0) - R @ s.mean(0))[:, None]], 1)
    assert rte_rre(T, pr["transform_gt"][0], *THRESHOLDS["3DMatch"])[0] == 1.0
