"""Evaluate a checkpoint on the reference's test splits read from disk (the reference's `test.py` main for
`--pipeline align`, test.py:386-457): dataset -> device pre-processing -> registration -> RTE / RRE / success.

    python examples/eval_dataset.py --dataset 3DMatch --root /data/3DMatch --num-points 5000 [--ckpt model.pth] [--limit 50]
    python examples/eval_dataset.py --dataset KITTI   --root /data/kitti   --num-points 16384 --voxel-size 0.3
    python examples/eval_dataset.py --dataset Oxford  --root /data/oxford  --num-points 10000

Directory layouts are the reference's (dataloader/threeDMatch_loader.py, kitti_loader.py); see deepsir_amd/data.py.
Without --ckpt a seeded random state-dict is used (plumbing check only).  `--method fpfh` needs no checkpoint at all: the
weight-independent baseline, FPFH descriptors + feature-matching RANSAC on the device (`harness.register_fpfh`; `--fpfh-radius R`
takes the descriptors over radius lists instead of the pyramid's 16-NN lists; `--keypoints iss` matches and solves on ISS keypoints
only, `--salient-radius` / `--non-max-radius` default to 6 and 4 voxel sizes; `--keypoints fps` on `--num-keypoints` farthest-point
samples per cloud, one batched matching and pose call per batch)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepsir_amd import data as D  # noqa: E402
from deepsir_amd.arch import NetConfig  # noqa: E402
from deepsir_amd.harness import evaluate_align, inference_align, register_feat, register_fpfh, summarize  # noqa: E402
from deepsir_amd.model import Network  # noqa: E402
from deepsir_amd.weights import generate_state_dict, to_torch_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", choices=["3DMatch", "KITTI", "Oxford"], required=True)
    ap.add_argument("--root", required=True)
    ap.add_argument("--ckpt", default="")
    ap.add_argument("--num-points", type=int, default=5000)
    ap.add_argument("--voxel-size", type=float, default=None)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--limit", type=int, default=0)
    ap.add_argument("--pose-opt", choices=["none", "icp", "icp_plane", "ndt", "tune", "ransac", "consensus", "fgr"], default="none")
    ap.add_argument("--ndt-resolution", type=float, default=None,
                    help="with --pose-opt ndt: the cell edge of the NDT map (default: 4 x the voxel size)")
    ap.add_argument("--icp-search", choices=["brute", "grid", "auto"], default="auto",
                    help="with --pose-opt icp / icp_plane: the nearest-neighbour search of the refinement (same poses, other time)")
    ap.add_argument("--pipeline", choices=["align", "feat"], default="align")
    ap.add_argument("--ransac", action="store_true", help="with --pipeline feat: descriptors -> mutual nearest neighbours -> RANSAC pose")
    ap.add_argument("--num-sub", type=int, default=1024, help="key points per cloud of the feat pipeline")
    ap.add_argument("--hypotheses", type=int, default=8192)
    ap.add_argument("--pose", choices=["ransac", "consensus", "fgr"], default="ransac",
                    help="pose stage of --method fpfh and --pipeline feat: seeded RANSAC, the spatial-consensus stage (no sampling) or "
                         "fast global registration (tuple pre-filter, graduated Gauss-Newton)")
    ap.add_argument("--method", choices=["network", "fpfh"], default="network", help="fpfh: FPFH + RANSAC instead of the network")
    ap.add_argument("--fpfh-radius", type=float, default=None, help="with --method fpfh: radius lists instead of the 16-NN lists")
    ap.add_argument("--fpfh-search", choices=["brute", "grid"], default="brute",
                    help="with --fpfh-radius: brute-force radius lists, or the cell-indexed search (same lists, linear workspace)")
    ap.add_argument("--fpfh-max-nn", type=int, default=0, help="with --fpfh-search grid: keep the max_nn nearest of a radius list (0 = all)")
    ap.add_argument("--normal-radius", type=float, default=None,
                    help="with --method fpfh: normals from radius neighbourhoods over the cell index instead of the 16-NN lists")
    ap.add_argument("--normal-max-nn", type=int, default=0, help="with --normal-radius: the max_nn nearest of a neighbourhood (0 = all)")
    ap.add_argument("--keypoints", choices=["none", "iss", "fps"], default="none",
                    help="with --method fpfh: match and solve on ISS keypoints, or on farthest-point samples, only (descriptors still come "
                         "from every point)")
    ap.add_argument("--num-keypoints", type=int, default=1024, help="with --keypoints fps: the samples per cloud")
    ap.add_argument("--salient-radius", type=float, default=None, help="with --keypoints iss: the covariance neighbourhood (default 6 x voxel size)")
    ap.add_argument("--non-max-radius", type=float, default=None, help="with --keypoints iss: the non-maximum-suppression radius (default 4 x voxel size)")
    ap.add_argument("--match-k", type=int, default=1,
                    help="--method fpfh / --pipeline feat: the k nearest descriptors of every src point as candidate matches (1 .. 8)")
    ap.add_argument("--match-ratio", type=float, default=0.0,
                    help="--method fpfh / --pipeline feat: Lowe's ratio test on the 1-NN matches (0 < ratio < 1; 0 = off; needs --match-k 1)")
    ap.add_argument("--remove-ground", type=float, default=None, metavar="THR",
                    help="--method fpfh: drop the dominant near-horizontal plane of both clouds first (harness.remove_ground, RANSAC "
                         "inlier distance THR in metres; pairs then run one at a time).  Default: off.  The network paths take no such option")
    ap.add_argument("--ground-angle", type=float, default=15.0, metavar="DEG", help="with --remove-ground: the cone about +z the plane's normal must lie in")
    a = ap.parse_args()
    if a.remove_ground is not None and a.method != "fpfh":
        ap.error("--remove-ground applies to --method fpfh only (the network was trained on clouds with their ground)")
    ground = None if a.remove_ground is None else dict(distance_threshold=a.remove_ground, max_angle_deg=a.ground_angle)
    kitti = a.dataset == "KITTI"
    cfg = NetConfig(feat_len=4 if kitti else 3)
    if a.pipeline == "feat" and not a.ransac:
        ap.error("--pipeline feat evaluates as a registration only with --ransac")
    feat = a.pipeline == "feat"
    if feat:
        cfg = NetConfig(feat_len=cfg.feat_len, pipeline="feat", num_sub=a.num_sub)
    args = argparse.Namespace(pipeline=a.pipeline, num_sub=a.num_sub if feat else -1, num_knn=16, out_feat_dim=64, clip_weight_thresh=0.0,
                              feat_len=cfg.feat_len, d_out=[16, 64, 128, 256], num_points=a.num_points,
                              sub_sampling_ratio=[4, 4, 4, 4], use_ppf=False)
    model = Network(args)
    sd = torch.load(a.ckpt, map_location="cpu") if a.ckpt else to_torch_state_dict(generate_state_dict(cfg, 0))
    model.load_state_dict(sd["state_dict"] if "state_dict" in sd else sd)
    model = model.cuda().eval()
    # the engine also runs the datasets' device steps; the pose stages take J x match_k <= max_points rows
    eng = model._ensure_engine(max(a.num_points * (a.match_k if a.method == "fpfh" else 1), 1024), a.batch)
    oxford = a.dataset == "Oxford"
    voxel = a.voxel_size or (0.3 if kitti or oxford else 0.03)
    ds = (D.KittiOdometryTest(a.root, eng, voxel_size=voxel, feat_len=cfg.feat_len, num_points=a.num_points) if kitti
          else D.OxfordTest(a.root, eng, "test", voxel_size=voxel, feat_len=cfg.feat_len, num_points=a.num_points) if oxford
          else D.ThreeDMatchTest(a.root, eng, voxel_size=voxel, num_points=a.num_points))
    n = min(len(ds), a.limit) if a.limit else len(ds)
    pairs = [D.as_batch(ds[i]) for i in range(n)]
    if a.method == "fpfh":
        pred, stats = register_fpfh(pairs, eng, voxel_size=voxel, radius=a.fpfh_radius, hypotheses=a.hypotheses, dataset_type=a.dataset,
                                    batch=1 if ground else a.batch, ground=ground, pose=a.pose, match_k=a.match_k, match_ratio=a.match_ratio, search=a.fpfh_search,
                                    max_nn=a.fpfh_max_nn, normal_radius=a.normal_radius, normal_max_nn=a.normal_max_nn,
                                    keypoints=None if a.keypoints == "none" else a.keypoints, salient_radius=a.salient_radius,
                                    non_max_radius=a.non_max_radius, num_keypoints=a.num_keypoints)
    elif feat:
        pred, stats = register_feat(pairs, model, voxel_size=voxel, hypotheses=a.hypotheses, dataset_type=a.dataset, batch=a.batch,
                                    pose=a.pose, match_k=a.match_k, match_ratio=a.match_ratio)
    else:
        pred, stats = inference_align(pairs, model, a.iters, a.dataset, batch=a.batch,
                                      pose_opt=None if a.pose_opt == "none" else a.pose_opt, voxel_size=voxel,
                                      icp_search=a.icp_search, ndt_resolution=a.ndt_resolution)
    print({k: round(float(v), 4) for k, v in summarize(stats).items()})
    _, summary = evaluate_align(pred, pairs, eng, a.dataset)
    print({k: round(float(v), 5) for k, v in summary.items()})


if __name__ == "__main__":
    main()
