"""Train the `align` pipeline from a dataset directory in the reference's layout - the shape of the reference's train.py:303-488
over ``deepsir_amd.data.TrainBatches`` (no open3d, no reference code):

    python examples/train_dataset.py --dataset 3dmatch --root /data/3dmatch --points 2048 --batch 2 --steps 100 --out runs/a
    python examples/train_dataset.py --dataset kitti --root /data/kitti --points 18000 --batch 8 --epochs 2 --out runs/k
    python examples/train_dataset.py --dataset Oxford --root /data/oxford --points 10000 --batch 8 --epochs 2 --out runs/o

Per epoch: device-resident batches (voxel grid, augmentation, ground-truth matches: all HIP) -> ``Network.train_step`` (Adam on the
device).  Every --val-every steps: the val split through the evaluation-mode network, ``loss_align_fun(..., reduction='none')``
accumulated per pair plus ``harness.evaluate_align`` metrics.  Checkpoints are the reference's ``{'state_dict', 'optimizer',
'step'}`` (common/torch_utils.py:64-66): `<out>/ckpt.pth` is written at every validation and at the end, and picked up again by
--resume.  The log is JSON lines in `<out>/log.jsonl`."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepsir_amd import data as D  # noqa: E402
from deepsir_amd.engine import Engine  # noqa: E402
from deepsir_amd.harness import evaluate_align, summarize_metrics  # noqa: E402
from deepsir_amd.model import Network  # noqa: E402
from deepsir_amd.weights import generate_state_dict, to_torch_state_dict  # noqa: E402


def validate(model, batches, n_iter, dataset_type):
    """validate_align (train.py:113-137): per-pair losses of the evaluation-mode network and the registration metrics."""
    model.eval()
    totals, preds, pairs = [], [], []
    with torch.no_grad():
        for data in batches:
            pred, endpoints = model(data, (n_iter, False))
            endpoints["transform_gt"], endpoints["transform_pred"] = data["transform_gt"], pred
            if "matches" in data:
                endpoints["matches"] = data["matches"]
            totals.append(model.loss_align_fun(endpoints, reduction="none")["total"].detach().cpu().numpy())
            preds.append(torch.stack(pred, 1).cpu().numpy())
            B = data["points_src"].shape[0]
            pairs.extend({"points_src": data["points_src"][b:b + 1], "points_ref": data["points_ref"][b:b + 1],
                          "transform_gt": data["transform_gt"][b:b + 1].cpu().numpy()} for b in range(B))
    model.train()
    if not totals:
        return {}
    eng = model._ensure_engine(pairs[0]["points_src"].shape[1], 1)
    metrics, _ = evaluate_align(np.concatenate(preds), pairs, eng, dataset_type)
    out = {"val_loss": float(np.concatenate(totals).mean()), "val_pairs": len(pairs)}
    out.update({"val_" + k: float(v) for k, v in summarize_metrics(metrics[-1]).items()})
    return out


def save_checkpoint(path, model, lr, step):
    tmp = path + ".tmp"
    torch.save({"state_dict": model.state_dict(), "optimizer": model.optimizer_state_dict(lr), "step": step}, tmp)
    os.replace(tmp, path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", choices=["3dmatch", "kitti", "Oxford"], default="3dmatch")
    ap.add_argument("--root", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3, help="num_train_reg_iter")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--wt_pose_loss", type=float, default=0.0, help="weight of the rotation + translation error term (0 = off, the reference's default)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--epochs", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=100, help="stop after this many optimisation steps (counted across resumes)")
    ap.add_argument("--val-every", type=int, default=50)
    ap.add_argument("--num-val", type=int, default=-1)
    ap.add_argument("--voxel-size", type=float, default=None)
    ap.add_argument("--sequences", type=int, nargs="*", default=None, help="kitti: drives of the train split")
    ap.add_argument("--val-sequences", type=int, nargs="*", default=None)
    ap.add_argument("--no-refine", action="store_true", help="kitti: odometry poses without the ICP refinement")
    ap.add_argument("--no-list", action="store_true", help="no match list: the targets from data['match_radius']")
    ap.add_argument("--data-max-points", type=int, default=65536, help="sizes the data engine's workspace for the raw clouds of a batch")
    ap.add_argument("--resume", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    kitti = a.dataset == "kitti"
    args = SimpleNamespace(pipeline="align", feat_len=4 if kitti else 3, num_sub=-1, num_knn=16, out_feat_dim=64, clip_weight_thresh=0.0,
                           d_out=[16, 64, 128, 256], sub_sampling_ratio=[4, 4, 4, 4], use_ppf=False, num_reg_iter=a.iters, loss_type="mae",
                           wt_ptDist_loss=1.0, wt_inlier_loss=1.0, wt_pose_loss=a.wt_pose_loss, loss_discount_factor=0.5, lr=a.lr)
    model = Network(args)
    os.makedirs(a.out, exist_ok=True)
    ckpt, step = os.path.join(a.out, "ckpt.pth"), 0
    saved = torch.load(ckpt, map_location="cpu", weights_only=False) if a.resume and os.path.exists(ckpt) else None
    model.load_state_dict(saved["state_dict"] if saved else to_torch_state_dict(generate_state_dict(model.cfg, 1, "separated")))
    model.to(dev)
    model.train()
    if saved:
        model.prepare_training()
        model.load_optimizer_state_dict(saved["optimizer"])
        step = int(saved["step"])
    # the data path's own engine: its workspace is sized for the RAW clouds of a batch (voxel grid), not for the network's input
    eng = Engine(model.cfg, 0, max_points=max(a.points, a.data_max_points), max_pairs=1)
    if kitti:
        kw = dict(voxel_size=a.voxel_size or 0.3, num_points=a.points, refine_pose=not a.no_refine,
                  with_labels=os.path.isdir(os.path.join(a.root, "dataset", "sequences", "%02d" % (a.sequences or [0])[0], "labels")))
        train = D.KittiOdometryTrain(a.root, eng, "train", sequences=a.sequences, **kw)
        val = D.KittiOdometryTrain(a.root, eng, "val", sequences=a.val_sequences, num_val=a.num_val, **kw)
    elif a.dataset == "Oxford":        # one scan per sample, cropped twice on the device; validation on the ground-truth pairs
        train = D.OxfordTrain(a.root, eng, num_points=a.points, voxel_size=a.voxel_size or 0.3)
        val = D.OxfordTest(a.root, eng, "val", num_val=a.num_val, voxel_size=a.voxel_size or 0.3, num_points=a.points)
    else:
        kw = dict(voxel_size=a.voxel_size or 0.03, num_points=a.points)
        train = D.ThreeDMatchTrain(a.root, eng, "train", **kw)
        val = D.ThreeDMatchTrain(a.root, eng, "val", num_val=a.num_val, **kw)
    radius = train.match_radius if a.no_list else None
    batches = D.TrainBatches(train, a.batch, a.seed, shuffle=True, match_radius=radius)
    val_batches = D.TrainBatches(val, 1, a.seed, shuffle=False, match_radius=radius, drop_last=False)
    if len(batches) == 0:
        raise SystemExit(f"{len(train)} training pairs do not fill one batch of {a.batch}")
    log = open(os.path.join(a.out, "log.jsonl"), "a")

    def emit(rec):
        log.write(json.dumps(rec) + "\n")
        log.flush()
        print(json.dumps(rec), flush=True)
    emit({"event": "start", "step": step, "train_pairs": len(train), "val_pairs": len(val), "resumed": bool(saved)})
    epoch = step // len(batches)
    while step < a.steps and epoch < a.epochs:
        batches.set_epoch(epoch)
        for b, data in enumerate(batches):
            if b < step - epoch * len(batches):          # a resumed epoch continues where the checkpoint left it
                continue
            out = model.train_step(data, (a.iters, True), lr=a.lr, dropout_seed=a.seed * 1000003 + step)
            step += 1
            rec = {"event": "train", "step": step, "epoch": epoch, "loss": float(out["loss"]),
                   "invalid_clouds": int((data["invalid"] != 0).sum().item())}
            if a.wt_pose_loss > 0:      # the term of the last iteration, when it is on
                rec["pose_error"] = float(out["losses"][f"poseError_{a.iters - 1}"])
            emit(rec)
            if step % a.val_every == 0 or step == a.steps:
                rec = {"event": "val", "step": step}
                rec.update(validate(model, val_batches, a.iters, "KITTI" if kitti else ("Oxford" if a.dataset == "Oxford" else "3DMatch")))
                save_checkpoint(ckpt, model, a.lr, step)
                emit(rec)
            if step >= a.steps:
                break
        epoch += 1
    save_checkpoint(ckpt, model, a.lr, step)
    emit({"event": "end", "step": step, "checkpoint": ckpt})


if __name__ == "__main__":
    main()
