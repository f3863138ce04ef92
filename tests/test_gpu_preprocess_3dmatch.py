"""``deepsir_amd.data.preprocess_3dmatch`` end to end on a fabricated 3DMatch download: PLY fragments and poses in, the three tables
out, equal to the host rule applied to the stored points, readable by ``ThreeDMatchTrain``."""
import os
import pickle

import numpy as np
import pytest

from deepsir_amd import data as D
from deepsir_amd import overlap as O

pytestmark = pytest.mark.gpu

SCENES = {"scene-x": ("seq-01", 4), "scene-a": ("seq-02", 3)}


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), 0, max_points=8192, max_pairs=2)
    yield e
    e.close()


def _write_tree(root):
    """Fragments cut from one synthetic surface, 0.5 m apart along x and 1.6 m wide, each stored in a frame of its own (ASCII PLY)
    with the pose back into the common frame next to it: about 3000 points after the 0.03 m voxel grid."""
    from deepsir_amd import augment as A
    rng = np.random.default_rng(3)
    for s, (scene, (seq, n)) in enumerate(SCENES.items()):
        os.makedirs(os.path.join(root, scene, seq))
        for k in range(n):
            xy = rng.random((6000, 2)) * 1.6 + [0.5 * k + 3.0 * s, -0.4]
            z = 0.2 * np.sin(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1]) + rng.normal(0.0, 0.003, len(xy))
            world = np.concatenate([xy, z[:, None]], 1)
            M = np.eye(4)
            M[:3, :3] = A.rodrigues(rng.random(3) - 0.5, 0.3 + 0.2 * k)
            M[:3, 3] = rng.random(3) * 2 - 1
            local = (world - M[:3, 3]) @ M[:3, :3]
            stem = os.path.join(root, scene, seq, f"cloud_bin_{k}")
            with open(stem + ".ply", "w") as f:
                f.write(f"ply\nformat ascii 1.0\nelement vertex {len(local)}\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
                np.savetxt(f, local, fmt="%.7f")
            np.save(stem + ".pose.npy", M)
    with open(os.path.join(root, "scene_list_train.txt"), "w") as f:
        f.write("\n".join(SCENES) + "\n")


def test_preprocess_3dmatch_writes_tables_the_loaders_read(eng, tmp_path):
    root = str(tmp_path)
    _write_tree(root)
    save = os.path.join(root, "3dmatch_train_val")
    points, overlap, keypts = D.preprocess_3dmatch(root, save, "train", eng, max_jobs_bytes=40000)     # small: the job lists are cut
    names = ["3DMatch_train_0.030_keypts.pkl", "3DMatch_train_0.030_overlap.pkl", "3DMatch_train_0.030_points.pkl"]
    assert sorted(os.listdir(save)) == names
    ids = [f"{scene}/{seq}/cloud_bin_{k}" for scene, (seq, n) in SCENES.items() for k in range(n)]
    assert list(points) == ids
    for i in ids:
        p = points[i]
        assert p.dtype == np.float64 and p.ndim == 2 and p.shape[1] == 3 and 2000 < len(p) < 3600
        scene = list(SCENES).index(i.split("/")[0])
        k = int(i.split("_")[-1])
        lo, hi = p.min(0), p.max(0)                        # back in the common frame: the patch the fragment was cut from
        assert abs(lo[0] - (0.5 * k + 3.0 * scene)) < 0.05 and abs(hi[0] - (0.5 * k + 3.0 * scene + 1.6)) < 0.05 and abs(lo[1] + 0.4) < 0.05
    # ratios and key points: the host rule on the stored points
    want_o, want_k = {}, {}
    for scene, (seq, n) in SCENES.items():
        O.scene_tables([i for i in ids if i.startswith(scene)], points, O.host_search, 0.03, 0.30, want_o, want_k)
    print({k: round(v, 4) for k, v in want_o.items()})
    assert 2 <= len(want_o) < 9                             # some pairs pass the threshold, some do not
    assert list(overlap) == list(want_o) == list(keypts) and all(overlap[k] == want_o[k] for k in want_o)
    for k in want_k:
        assert keypts[k].dtype == np.int32 and np.array_equal(keypts[k], want_k[k])
        assert len(keypts[k]) == round(overlap[k] * len(points[k.split("@")[0]]))
    for fn, obj in zip(O.table_paths(save, "train", 0.03), (points, overlap, keypts)):
        with open(fn, "rb") as f:
            assert list(pickle.load(f)) == list(obj)
    # the training split opens it and yields these pairs
    ds = D.ThreeDMatchTrain(root, eng, split="train")
    assert ds.files == [tuple(k.split("@")) for k in overlap] and len(ds) == len(overlap)
    src, ref, pose, others = ds.raw(0)
    s_id, r_id = ds.files[0]
    assert np.array_equal(src, points[s_id].astype(np.float32)) and np.array_equal(ref, points[r_id].astype(np.float32))
    assert np.array_equal(pose, np.eye(4)) and others["seq"] == "scene-x"
    # a second call reloads: without an engine nothing could be recomputed
    p2, o2, k2 = D.preprocess_3dmatch(root, save, "train", None)
    assert list(p2) == ids and o2 == overlap and all(np.array_equal(k2[k], keypts[k]) for k in keypts)
