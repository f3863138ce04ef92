"""The reference's `align` training loop (train.py:396-446) with the confidence term switched on by a
ground-truth match list that is built HERE, on the device - the reference's loader needs open3d's KD-tree for it
(dataloader/data_base.py:436-449):

    python examples/train_matches.py --pairs 4 --points 2048 --radius 0.09 --steps 10

Per batch: ``Engine.radius_matches`` (every (src, ref) pair closer than --radius under the ground-truth pose) ->
``as_reference_matches`` (the reference's data['matches']: per pair an int array [n', 2]).  The loop below is the reference's,
line for line.  ``--no-list`` hands over the radius alone (endpoints['match_radius']): the same targets, no list at all."""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepsir_amd.model import Network  # noqa: E402
from deepsir_amd.synth import make_batch  # noqa: E402
from deepsir_amd.train import as_reference_matches  # noqa: E402
from deepsir_amd.weights import generate_state_dict, to_torch_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=3, help="num_train_reg_iter")
    ap.add_argument("--radius", type=float, default=0.09, help="voxel_size * positive_pair_radius_multiplier")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--wt_pose_loss", type=float, default=0.0, help="weight of the rotation + translation error term (0 = off, the reference's default)")
    ap.add_argument("--no-list", action="store_true", help="no match list: the targets from endpoints['match_radius']")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    _args = SimpleNamespace(pipeline="align", feat_len=3, num_sub=-1, num_knn=16, out_feat_dim=64, clip_weight_thresh=0.0, d_out=[16, 64, 128, 256],
                            sub_sampling_ratio=[4, 4, 4, 4], use_ppf=False, num_reg_iter=a.iters, loss_type="mae", wt_ptDist_loss=1.0,
                            wt_inlier_loss=1.0, wt_pose_loss=a.wt_pose_loss, loss_discount_factor=0.5, lr=a.lr)
    my_model = Network(_args)
    my_model.load_state_dict(to_torch_state_dict(generate_state_dict(my_model.cfg, 1, "separated")))
    my_model.to(dev)
    raw = make_batch(a.points, [2000 + b for b in range(a.pairs)], 3, "3dmatch", partial_overlap=True)
    train_data = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in raw.items()}
    # ---- the loader's part: data['matches'], once per batch, on the device
    eng = my_model._ensure_engine(a.points, a.pairs)
    offsets, cols = eng.radius_matches(train_data["points_src"], train_data["points_ref"], train_data["transform_gt"], a.radius)
    train_data["matches"] = as_reference_matches(offsets, cols, a.pairs, a.points)
    print(f"{cols.numel()} ground-truth matches within {a.radius} m in {a.pairs} pairs of {a.points} points "
          f"({cols.numel() / (a.pairs * a.points):.2f} per source point)")
    # ---- train.py:323, :379-446, unchanged
    optimizer = torch.optim.Adam(my_model.parameters(), lr=_args.lr)
    my_model.train()
    opt_tuple = (a.iters, True)
    for step in range(1, a.steps + 1):
        optimizer.zero_grad()
        pred_transforms, endpoints = my_model(train_data, opt_tuple)
        endpoints['transform_gt'] = train_data['transform_gt']
        endpoints['transform_pred'] = pred_transforms
        if a.no_list:
            endpoints['match_radius'] = a.radius
        else:
            endpoints['matches'] = train_data['matches']
        losses = my_model.loss_align_fun(endpoints, reduction='mean')
        loss = losses['total']
        loss.backward()
        backprop_flag = False
        for name, param in my_model.named_parameters():
            if param.grad is not None and torch.any(torch.isnan(param.grad)):
                optimizer.zero_grad()
                backprop_flag = True
                break
        if not (backprop_flag or endpoints['invalid_gradient']):
            optimizer.step()
        last = a.iters - 1
        pose = f"  poseError_{last} {losses[f'poseError_{last}'].item():.5f}" if f"poseError_{last}" in losses else ""
        print(f"step {step:3d}  total {loss.item():.5f}  mae_{last} {losses[f'mae_{last}'].item():.5f}  outlier_{last} {losses[f'outlier_{last}'].item():.5f}{pose}",
              flush=True)


if __name__ == "__main__":
    main()
