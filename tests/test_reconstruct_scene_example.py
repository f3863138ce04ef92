"""examples/reconstruct_scene.py on a folder laid out as the 3DMatch test split is (`<root>/test/<scene>/cloud_bin_<i>.ply`,
`<root>/test/<scene>-evaluation/gt.log` and `gt.info`): the walk without a GPU, one scene end to end on the MI355X."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example():
    spec = importlib.util.spec_from_file_location("reconstruct_scene", os.path.join(ROOT, "examples", "reconstruct_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_ply(path, pts):
    with open(path, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {len(pts)}\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
        for p in pts:
            f.write(f"{p[0]:.9g} {p[1]:.9g} {p[2]:.9g}\n")


def _write_scene(root, scene, frags, gt, with_info=True):
    os.makedirs(os.path.join(root, "test", scene))
    os.makedirs(os.path.join(root, "test", scene + "-evaluation"))
    for i, f in enumerate(frags):
        _write_ply(os.path.join(root, "test", scene, f"cloud_bin_{i}.ply"), f)
    with open(os.path.join(root, "test", scene + "-evaluation", "gt.log"), "w") as f:
        for (i, j), T in gt.items():                                  # record (i, j, n): the pose taking fragment j into i's frame
            f.write(f"{i}\t{j}\t{len(frags)}\n" + "".join(" ".join(f"{v:.17g}" for v in row) + "\n" for row in np.vstack([T, [0, 0, 0, 1]])))
    if with_info:
        with open(os.path.join(root, "test", scene + "-evaluation", "gt.info"), "w") as f:
            for (i, j) in gt:
                f.write(f"{i}\t{j}\t{len(frags)}\n" + "".join(" ".join(f"{v:.17g}" for v in row) + "\n" for row in 100.0 * np.eye(6)))


def test_scene_files_walks_the_test_split_layout(tmp_path):
    ex = _example()
    rng = np.random.default_rng(0)
    frags = [rng.uniform(0, 1, (20, 3)).astype(np.float32) for _ in range(3)]
    gt = {(0, 1): np.eye(3, 4), (0, 2): np.eye(3, 4), (1, 2): np.eye(3, 4)}
    _write_scene(str(tmp_path), "room", frags, gt)
    files, g, gi = ex.scene_files(str(tmp_path), "room")
    assert [os.path.basename(f) for f in files] == ["cloud_bin_0.ply", "cloud_bin_1.ply", "cloud_bin_2.ply"]
    assert sorted(g) == [(1, 0), (2, 0), (2, 1)] and sorted(gi) == sorted(g) and g[(1, 0)].shape == (4, 4) and gi[(2, 1)].shape == (6, 6)
    from deepsir_amd.data import read_ply_xyz
    assert np.array_equal(read_ply_xyz(files[1]), frags[1])
    files, g, _ = ex.scene_files(str(tmp_path), "room", max_fragments=2)
    assert len(files) == 2 and sorted(g) == [(1, 0)]
    with pytest.raises(FileNotFoundError):
        ex.scene_files(str(tmp_path), "room-evaluation")              # the evaluation folder is not a scene
    with pytest.raises(FileNotFoundError):
        ex.scene_files(str(tmp_path), "absent")
    with pytest.raises(FileNotFoundError):
        ex.main(["--root", str(tmp_path / "test")])                   # no test/ below it: said, not skipped


@pytest.mark.gpu
def test_gpu_example_runs_one_scene_end_to_end(tmp_path):
    from test_gpu_register_scene import _scene
    ex = _example()
    frags, X, gt, _, _ = _scene()
    _write_scene(str(tmp_path), "synth", frags, {(t, s): T for (s, t), T in gt.items()})     # gt[(s, t)] takes s into t: record (t, s)
    out, = ex.main(["--root", str(tmp_path), "--scenes", "synth", "--voxel", "0.1", "--hypotheses", "2048"])
    print(out)
    assert out["scene"] == "synth" and out["fragments"] == 6 and all(1000 < n < 1700 for n in out["points"])
    if "skipped" in out:                                              # descriptors of a uniform random cloud may fail the pairwise stage
        assert "disconnected" in out["skipped"]
    else:
        # measured on this scene: 6 of the 15 FPFH edges switched off by the line process, pairwise recall 0.6 raw -> 1.0 optimised
        assert out["edges"] == 15 and out["pairs"] == 15 and out["pairs_info"] == 15
        assert out["recall_optimized"] >= out["recall_raw"] and out["recall_optimized_info"] >= out["recall_raw_info"]
