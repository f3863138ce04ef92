"""Scene-level registration of the 3DMatch test split, scene by scene: a scene's fragments are registered pairwise
(--method fpfh | feat), the pairs are refined and weighted (icp_refine, information_matrix) and the pose graph is optimised with
its line process (harness.register_scene).  Per scene it prints the pairwise recall (RTE / RRE thresholds, and the benchmark's
info_rmse where the scene has a gt.info) of the raw pair poses and of the poses the optimised nodes imply (X_t^-1 X_s), and the
number of pruned edges.

  python examples/reconstruct_scene.py --root <3dmatch root> [--method fpfh] [--voxel 0.05] [--scenes NAME ...] [--weights w.pth]

Layout of --root, the one `deepsir_amd.data.ThreeDMatchTest` walks: `<root>/test/<scene>/cloud_bin_<i>.ply` are the fragments,
`<root>/test/<scene>-evaluation/gt.log` (and `gt.info`, where the benchmark ships it) the ground truth: a record (i, j, n) holds
the pose taking fragment j into fragment i's frame.  Fragments are voxel-averaged at --voxel on the device and keep their ragged
sizes.  A scene whose kept edges do not connect it (the pairwise stage failed on too many pairs) is reported and skipped."""
import argparse
import glob
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deepsir_amd import harness as H                                                    # noqa: E402
from deepsir_amd.arch import NetConfig                                                  # noqa: E402
from deepsir_amd.data import THREEDMATCH_TEST_SCENES, _voxelize, read_ply_xyz, read_trajectory   # noqa: E402
from deepsir_amd.weights import generate_state_dict                                     # noqa: E402


def scene_files(root, scene, max_fragments=None):
    """-> (fragment .ply paths in index order, gt {(src j, ref i): T [4,4]}, gt_info {(j, i): info [6,6]}) of one test scene;
    FileNotFoundError when the scene has no fragments or no gt.log"""
    test = os.path.join(root, "test")
    plys = {}
    for f in glob.glob(os.path.join(test, scene, "cloud_bin_*.ply")):
        m = re.fullmatch(r"cloud_bin_(\d+)\.ply", os.path.basename(f))
        if m:
            plys[int(m.group(1))] = f
    if not plys or sorted(plys) != list(range(len(plys))):
        raise FileNotFoundError(f"{os.path.join(test, scene)}: expected cloud_bin_0.ply .. cloud_bin_<n-1>.ply, found {len(plys)} fragment files")
    n = len(plys) if max_fragments is None else min(len(plys), int(max_fragments))
    ev = os.path.join(test, scene + "-evaluation")
    if not os.path.exists(os.path.join(ev, "gt.log")):
        raise FileNotFoundError(os.path.join(ev, "gt.log"))

    def records(name, dim):
        path = os.path.join(ev, name)
        if not os.path.exists(path):
            return {}
        return {(int(m[1]), int(m[0])): mat for m, mat in read_trajectory(path, dim=dim) if m[0] < n and m[1] < n}

    return [plys[i] for i in range(n)], records("gt.log", 4), records("gt.info", 6)


def run_scene(root, scene, method="fpfh", voxel=0.05, max_fragments=None, weights=None, hypotheses=8192, icp_batch=1, icp_kernel="l2",
              icp_kernel_scale=None):
    """One scene end to end -> the dict that is printed: `harness.summarize_scene`'s, or {"skipped": reason}.  icp_batch: edges per
    ICP and information-matrix call of `harness.register_scene` (same result for every value; the engine is made for that many pairs);
    icp_kernel / icp_kernel_scale: the robust kernel of its edge refinement (open3d's `robust_kernel`; "l2": none)"""
    files, gt, gt_info = scene_files(root, scene, max_fragments)
    raw = [read_ply_xyz(f) for f in files]
    cfg = NetConfig(pipeline="feat") if method == "feat" else NetConfig()
    model = eng = None
    try:
        if method == "fpfh":
            from deepsir_amd.engine import Engine
            eng = Engine(cfg, 0, max_points=max(1024, max(len(p) for p in raw)), max_pairs=max(1, icp_batch))
            eng.load_state_dict(generate_state_dict(cfg, 0))      # the FPFH path reads no weight; the context wants them loaded
            frags = _voxelize(eng, raw, voxel)
            edges = H.scene_edges_fpfh(frags, eng, voxel_size=voxel, radius=5 * voxel, normal_radius=2 * voxel, normal_max_nn=30,
                                       max_nn=100, search="grid", hypotheses=hypotheses)
            use = eng
        else:
            from deepsir_amd.model import Network
            model = Network(cfg).cuda()
            sd = torch.load(weights, map_location="cpu") if weights else generate_state_dict(cfg, 0)
            model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
            use = model._ensure_engine(max(1024, max(len(p) for p in raw)), max(1, icp_batch))
            frags = _voxelize(use, raw, voxel)
            edges = H.scene_edges_feat(frags, model, voxel_size=voxel, hypotheses=hypotheses)
        out = {"scene": scene, "fragments": len(frags), "points": [int(len(f)) for f in frags]}
        try:
            res = H.register_scene(frags, use, edges, voxel_size=voxel, batch=max(1, icp_batch), icp_kernel=icp_kernel, icp_kernel_scale=icp_kernel_scale)
        except ValueError as e:                                   # the kept edges do not connect the scene
            out["skipped"] = str(e)
            return out
        out.update(H.summarize_scene(res, gt, "3DMatch", gt_info))
        return out
    finally:
        if eng is not None:
            eng.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True, help="the 3DMatch root: holds test/<scene>/ and test/<scene>-evaluation/")
    ap.add_argument("--scenes", nargs="*", default=list(THREEDMATCH_TEST_SCENES))
    ap.add_argument("--method", choices=("fpfh", "feat"), default="fpfh")
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--hypotheses", type=int, default=8192)
    ap.add_argument("--max-fragments", type=int, default=None)
    ap.add_argument("--weights", default=None)
    ap.add_argument("--icp-batch", type=int, default=1, help="edges per ICP / information-matrix call of register_scene (any sizes; same result)")
    ap.add_argument("--icp-kernel", choices=("l2", "huber", "cauchy", "gm", "tukey"), default="l2",
                    help="robust loss kernel of the edges' ICP refinement (open3d's robust_kernel)")
    ap.add_argument("--icp-kernel-scale", type=float, default=None, help="its scale k in metres (needed unless --icp-kernel l2), e.g. the voxel size")
    a = ap.parse_args(argv)
    if not os.path.isdir(os.path.join(a.root, "test")):
        raise FileNotFoundError(f"Invalid path: {os.path.join(a.root, 'test')}")
    outs = []
    for scene in a.scenes:
        outs.append(run_scene(a.root, scene, a.method, a.voxel, a.max_fragments, a.weights, a.hypotheses, a.icp_batch, a.icp_kernel, a.icp_kernel_scale))
        print(outs[-1], flush=True)
    return outs


if __name__ == "__main__":
    main()
