"""tools/bench_train.py [--pairs P] [--points N] [--iters I] [--steps K] [--use-ppf] [--wt-pose-loss W]: time of one `align` training step of the inlier model
(deepsir_amd.train.train_step_align: 5 training-mode forwards, loss + gradient, 5 backwards, Adam) on one GPU; the
inference half (Engine.register) is timed separately.  Prints one JSON line.

--targets: where the confidence term's 0/1 targets come from INSIDE the timed step.  random (default): pre-made random labels
already on the device - the step with no target work at all; host: find_correct_correspondence on the host against the batch's
match lists (copy of idx down, np.isin per pair and iteration, copy up); matches: the same lists hashed, sorted and searched on
the device (deepsir_amd.train.inlier_targets); radius: no list, the distance test on the device.  The lists themselves come from
Engine.radius_matches with --radius (default 0.09 for --shape 3dmatch, 0.9 for kitti), once, outside the timed steps.

--wt-pose-loss W: the loss with its pose-error term at weight W (default 0: off).

--use-ppf: the networks of args.use_ppf (point rows of xyz + seeded unit normals; the taped point-pair-feature front end, csrc/ppf.hip)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepsir_amd.arch import NetConfig  # noqa: E402
from deepsir_amd.engine import Engine  # noqa: E402
from deepsir_amd.synth import make_pair  # noqa: E402
from deepsir_amd.train import (AggregationTrainer, AlignTrainStep, RandlaTrainer, as_reference_matches, find_correct_correspondence,  # noqa: E402
                               inlier_targets, train_step_align_full)
from deepsir_amd.weights import generate_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=8)
ap.add_argument("--points", type=int, default=5000)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--full", action="store_true", help="whole network in training mode (train_step_align_full), as train.py runs it")
ap.add_argument("--eager", action="store_true", help="launch every operator from the host (no hipGraph replay)")
ap.add_argument("--targets", choices=("random", "host", "matches", "radius"), default="random", help="source of the confidence targets in the timed step")
ap.add_argument("--shape", choices=("3dmatch", "kitti"), default="3dmatch", help="extent of the synthetic clouds")
ap.add_argument("--radius", type=float, default=None, help="match radius (default 0.09 for 3dmatch, 0.9 for kitti)")
ap.add_argument("--use-ppf", action="store_true", help="train the use_ppf networks (rows of xyz + normal)")
ap.add_argument("--wt-pose-loss", type=float, default=0.0, help="weight of the loss's pose-error term (0 = off)")
a = ap.parse_args()
cfg = NetConfig(feat_len=6, use_ppf=True) if a.use_ppf else NetConfig(feat_len=3)
sd = generate_state_dict(cfg, 3, "plain")
dev = torch.device("cuda:0")
eng = Engine(cfg, max_points=a.points, max_pairs=a.pairs)
eng.load_state_dict(sd)
raws = [make_pair(a.points, 100 + b, 3, a.shape) for b in range(a.pairs)]
if a.use_ppf:
    rng = np.random.Generator(np.random.Philox(key=0x99F))
    for r in raws:
        for k in ("points_src", "points_ref"):
            nrm = rng.standard_normal(r[k].shape)
            r[k] = np.concatenate([r[k], nrm / np.linalg.norm(nrm, axis=2, keepdims=True)], 2).astype(np.float32)
src = torch.from_numpy(np.concatenate([r["points_src"] for r in raws])).to(dev)
ref = torch.from_numpy(np.concatenate([r["points_ref"] for r in raws])).to(dev)
gt = torch.from_numpy(np.concatenate([r["transform_gt"] for r in raws]).astype(np.float32)).to(dev)
sx, sn, ss, si = eng.knn_pyramid(src)
batch = {"points_src": src, "points_ref": ref, "src_xyz": sx, "src_neigh": sn, "src_sub": ss, "src_interp": si}
tr = RandlaTrainer(cfg, sd, "inlier_model", 6, 1, dev)
labels = (torch.rand(a.iters, a.pairs, a.points) < 0.5).float().to(dev)
radius = a.radius if a.radius is not None else {"3dmatch": 0.09, "kitti": 0.9}[a.shape]
matches = None
if a.targets in ("host", "matches"):                           # the loader's work: once per batch, not part of the step
    matches = as_reference_matches(*eng.radius_matches(src, ref, gt, radius), a.pairs, a.points)


def targets(idx):
    """The confidence targets of one step for idx [iters][pairs][points], by the --targets route."""
    if a.targets == "random":
        return labels
    if a.targets == "host":
        return torch.from_numpy(find_correct_correspondence(matches, idx, a.points)).to(dev)
    if a.targets == "matches":
        return inlier_targets(tr.ops, idx, a.points, matches=matches)
    return inlier_targets(tr.ops, idx, a.points, match_radius=radius, src=src, ref=ref, transform_gt=gt)


if a.full:
    fe, ag = RandlaTrainer(cfg, sd, "feat_extractor", cfg.feat_len, cfg.num_classes, dev), AggregationTrainer(cfg, sd, dev)
    rx, rn, rs, ri = eng.knn_pyramid(ref)
    batch.update({"ref_xyz": rx, "ref_neigh": rn, "ref_sub": rs, "ref_interp": ri})
stepper = AlignTrainStep(eng, tr, a.pairs, a.points, a.points, a.iters, dropout=True, use_graph=not a.eager, wt_pose_loss=a.wt_pose_loss)
t_inf, t_train, losses = [], [], []
for s in range(a.steps + 2):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    res = eng.register(src, ref, n_iter=a.iters)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    if a.full:
        g_ = torch.Generator(device=dev).manual_seed(s)
        keep = lambda *sh: (torch.rand(*sh, generator=g_, device=dev) >= 0.5).to(torch.uint8)
        masks = {"fe_src": keep(a.pairs, a.points, 64), "fe_ref": keep(a.pairs, a.points, 64), "inlier": keep(a.iters, a.pairs, a.points, 64)}
        out = train_step_align_full(eng, tr, fe, ag, batch, gt, a.iters, targets, lr=1e-3, masks=masks, wt_pose_loss=a.wt_pose_loss)
    else:
        out = stepper.step(batch, res, gt, labels=targets(res["idx"]), lr=1e-3, dropout_seed=s)
    torch.cuda.synchronize(); t2 = time.perf_counter()
    eng.load_state_dict({**sd, **tr.state_dict()})            # the updated inlier model serves the next step's inference
    if s >= 2:                                              # step 0 runs eagerly, step 1 captures
        t_inf.append(t1 - t0); t_train.append(t2 - t1)
    losses.append(out["losses"]["total"])
extra = {} if a.targets == "random" else {"targets": a.targets, "shape": a.shape, "radius": radius}
if matches is not None:
    extra["matches_per_point"] = round(sum(len(m) for m in matches) / (a.pairs * a.points), 2)
if a.use_ppf:
    extra["use_ppf"] = True
if a.wt_pose_loss:
    extra["wt_pose_loss"] = a.wt_pose_loss
print(json.dumps({"mode": "whole network in training mode (eager)" if a.full else "eager" if a.eager else "hipGraph replay", "pairs": a.pairs, "points": a.points, "iters": a.iters, "inference_ms": round(1e3 * float(np.median(t_inf)), 2),
                  "train_step_ms": round(1e3 * float(np.median(t_train)), 2),
                  "train_pairs_per_s": round(a.pairs / float(np.median(t_train)), 2), "losses": [round(l, 5) for l in losses],
                  "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2**30, 2), **extra}))
