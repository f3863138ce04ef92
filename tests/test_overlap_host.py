"""Fragment overlap on the host (no GPU): the float32 restatement of the radius-bounded nearest-neighbour rule
(deepsir_amd/overlap.py::nn_within_host) against a float64 KD-tree, its tie rule, and the 3DMatch table logic with the search
injected as a callable."""
import os
import pickle

import numpy as np
import pytest

from deepsir_amd import overlap as O

R = 0.03
BAND = 1e-3          # relative band around r^2 inside which fp32 and fp64 may disagree


def surface(n, seed, side=1.7):
    """Random samples of a wavy surface (not lattice points): about one point per r x r at n = 3000, so matches and misses mix."""
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2)) * side
    z = 0.2 * np.sin(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1]) + rng.normal(0.0, 0.004, n)
    return np.concatenate([xy, z[:, None]], 1).astype(np.float32)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_rule_against_a_float64_kdtree(seed):
    from scipy.spatial import cKDTree
    a, b = surface(3000, seed), surface(2800, 100 + seed)
    counts, (nn,) = O.nn_within_host(np.concatenate([a, b]), [0, len(a), len(a) + len(b)], [(0, 1)], R)
    d, k = cKDTree(b.astype(np.float64)).query(a.astype(np.float64), k=2)
    d2, r2 = d * d, R * R
    m64 = d2[:, 0] < r2
    band = np.abs(d2[:, 0] - r2) <= BAND * r2
    share = (m64 & band).sum() / max(1, m64.sum())
    print(f"seed {seed}: fp64 matches {m64.sum()} of {len(a)}, fp32 {counts[0]}, in band {(m64 & band).sum()} ({100 * share:.3f} %)")
    assert 0.2 * len(a) < m64.sum() < 0.95 * len(a)            # both outcomes are exercised
    assert share <= 0.01
    assert np.array_equal((nn >= 0)[~band], m64[~band])
    assert counts[0] == (nn >= 0).sum()
    sure = m64 & ~band & (d2[:, 1] - d2[:, 0] > BAND * r2)
    assert sure.sum() > 0.9 * (m64 & ~band).sum()
    assert np.array_equal(nn[sure], k[sure, 0])


def test_ties_go_to_the_lower_index_and_non_finite_rows_match_nothing():
    b = surface(200, 7)
    b = np.concatenate([b, b[:50], b[:50]])                    # every one of the first 50 three times
    a = b[:60].copy()
    a[:, 0] += np.float32(0.001)
    a[55] = [np.nan, 0.0, 0.0]
    a[56] = [np.inf, 0.0, 0.0]
    bb = b.copy()
    bb[57] = np.nan                                            # a's row 57 loses its own twin, a non-finite b is never a neighbour
    counts, (nn,) = O.nn_within_host(np.concatenate([a, bb]), [0, 60, 60 + len(bb)], [(0, 1)], R)
    assert np.array_equal(nn[:50], np.arange(50))              # not 200 + i, not 250 + i
    assert nn[55] == -1 and nn[56] == -1 and nn[57] != 57
    assert counts[0] == (nn >= 0).sum()
    c0, (e0,) = O.nn_within_host(a, [0, 0, 60], [(0, 1)], R)   # an empty side
    c1, (e1,) = O.nn_within_host(a, [0, 0, 60], [(1, 0)], R)
    assert c0[0] == 0 and len(e0) == 0 and c1[0] == 0 and (e1 == -1).all()


def test_pose_is_applied_in_float32_before_the_search():
    a, b = surface(300, 4), surface(300, 5)
    T = np.array([[0.0, -1.0, 0.0, 0.5], [1.0, 0.0, 0.0, -0.25], [0.0, 0.0, 1.0, 0.125]], np.float32)
    pts = np.concatenate([a, b])
    c, (nn,) = O.nn_within_host(pts, [0, 300, 600], [(0, 1)], 0.1, poses=T[None])
    moved = np.stack([-a[:, 1] + np.float32(0.5), a[:, 0] - np.float32(0.25), a[:, 2] + np.float32(0.125)], 1)
    c2, (nn2,) = O.nn_within_host(np.concatenate([moved, b]), [0, 300, 600], [(0, 1)], 0.1)
    assert np.array_equal(nn, nn2) and c[0] == c2[0]
    eye = np.eye(4, dtype=np.float32)[None, :3]
    assert np.array_equal(O.nn_within_host(pts, [0, 300, 600], [(0, 1)], 0.1, poses=eye)[1][0], O.nn_within_host(pts, [0, 300, 600], [(0, 1)], 0.1)[1][0])


# ------------------------------------------------------------------------------------------------ the 3DMatch tables
def _tree(tmp_path):
    """Two scenes (the list names them in non-sorted order), sequences out of order, fragment numbers that sort differently as text."""
    root = tmp_path / "frags"
    layout = {"sceneB": {"seq-02": [0, 1], "seq-01": [10, 9, 2], "notes": [5]}, "sceneA": {"seq-01": [1, 0, 11]}}
    for scene, seqs in layout.items():
        for seq, nums in seqs.items():
            os.makedirs(root / scene / seq)
            for k in nums:
                (root / scene / seq / f"cloud_bin_{k}.ply").write_text("ply\n")
                (root / scene / seq / f"cloud_bin_{k}.pose.npy").write_text("")
            (root / scene / seq / "readme.txt").write_text("")
    (root / "scene_list_train.txt").write_text("sceneB\nsceneA\n")
    return str(root)


def test_fragment_list_order(tmp_path):
    from deepsir_amd.data import list_3dmatch_fragments
    got = list_3dmatch_fragments(_tree(tmp_path), "train")
    assert list(got) == ["sceneB", "sceneA"]
    assert got["sceneB"] == ["sceneB/seq-01/cloud_bin_2", "sceneB/seq-01/cloud_bin_9", "sceneB/seq-01/cloud_bin_10",
                             "sceneB/seq-02/cloud_bin_0", "sceneB/seq-02/cloud_bin_1"]
    assert got["sceneA"] == ["sceneA/seq-01/cloud_bin_0", "sceneA/seq-01/cloud_bin_1", "sceneA/seq-01/cloud_bin_11"]


def test_tables_with_an_injected_search(tmp_path):
    from deepsir_amd.data import list_3dmatch_fragments
    scene_to_ids = list_3dmatch_fragments(_tree(tmp_path), "train")
    ids = [i for v in scene_to_ids.values() for i in v]
    # points 0.4 apart (far more than r), fragment k = rows [100 k, 100 k + 200) moved by much less than r: neighbours in the list
    # share exactly half of their points, everything else shares nothing; the last fragment repeats the first
    rng = np.random.default_rng(0)
    g = np.stack(np.meshgrid(np.arange(30), np.arange(30), indexing="ij"), -1).reshape(-1, 2) * 0.4
    cloud = np.concatenate([g, rng.random((900, 1))], 1)
    pts = {i: cloud[100 * k:100 * k + 200] + rng.normal(0, 1e-4, (200, 3)) for k, i in enumerate(ids)}
    pts[ids[4]] = pts[ids[0]][::-1].copy()            # sceneB's first and last fragment: ratio 1, indices reversed
    pts[ids[2]] = np.concatenate([pts[ids[2]][:128], pts[ids[2]][:128] + 50.0, pts[ids[2]][:128] + 90.0, pts[ids[2]][:128] + 130.0])
    calls = []

    def load_points(want):
        calls.append(("load", list(want)))
        return {i: pts[i] for i in want}

    def search(frags, jobs, radius, fill):
        calls.append(("fill" if fill else "count", len(jobs)))
        assert radius == 0.03 and all(f.dtype == np.float32 for f in frags)
        return O.host_search(frags, jobs, radius, fill)

    save = str(tmp_path / "out" / "3dmatch_train_val")
    points, overlap, keypts = O.write_3dmatch_tables(save, "train", 0.03, scene_to_ids, load_points, search, 0.30)
    assert sorted(os.listdir(save)) == ["3DMatch_train_0.030_keypts.pkl", "3DMatch_train_0.030_overlap.pkl", "3DMatch_train_0.030_points.pkl"]
    assert calls[0] == ("load", ids) and list(points) == ids and all(points[i].dtype == np.float64 for i in ids)
    assert [c for c in calls[1:]] == [("count", 10), ("fill", 4), ("count", 3), ("fill", 2)]
    b, a = scene_to_ids["sceneB"], scene_to_ids["sceneA"]
    # sceneB: (0,1) 0.5, (0,4) 1.0, (1,2) 0.5, (1,4) 0.5 stay; (2,3): fragment 2 shares 28 of its 512 rows with 3: 0.055 is dropped
    want = [(b[0], b[1], 0.5), (b[0], b[4], 1.0), (b[1], b[2], 0.5), (b[1], b[4], 0.5), (a[0], a[1], 0.5), (a[1], a[2], 0.5)]
    assert list(overlap) == [f"{s}@{r}" for s, r, _ in want] == list(keypts)
    assert [overlap[f"{s}@{r}"] for s, r, _ in want] == [v for _, _, v in want]
    assert all(v > 0.30 for v in overlap.values())
    k01 = keypts[f"{b[0]}@{b[1]}"]
    assert k01.dtype == np.int32 and k01.shape == (100, 2) and np.array_equal(k01, np.stack([np.arange(100, 200), np.arange(100)], 1))
    assert np.array_equal(keypts[f"{b[0]}@{b[4]}"], np.stack([np.arange(200), np.arange(200)[::-1]], 1))
    for fn, obj in zip(O.table_paths(save, "train", 0.03), (points, overlap, keypts)):
        with open(fn, "rb") as f:
            back = pickle.load(f)
        assert list(back) == list(obj)

    # a second call reloads: neither callable may run
    def boom(*_a):
        raise AssertionError("recomputed instead of reloaded")
    p2, o2, k2 = O.write_3dmatch_tables(save, "train", 0.03, scene_to_ids, boom, boom, 0.30)
    assert list(p2) == ids and o2 == overlap and all(np.array_equal(k2[k], keypts[k]) for k in keypts)
    # the points alone are reloaded when only the pair tables are missing
    os.remove(O.table_paths(save, "train", 0.03)[1])
    _, o3, _ = O.write_3dmatch_tables(save, "train", 0.03, scene_to_ids, boom, search, 0.30)
    assert o3 == overlap
