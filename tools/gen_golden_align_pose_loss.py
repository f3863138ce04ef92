"""Golden vectors for ScanAlignmentLoss WITH its pose-error term (wt_pose_loss > 0, network/loss.py:830-842): values for both
reductions and d total / d logits, produced by the REFERENCE's own ``ScanAlignmentLoss``, ``compute_rigid_transform_2`` and
``se3_torch`` under torch autograd on the CPU (build container only; TEST INFRASTRUCTURE).  Modelled on
oracle/gen_golden_align_loss.py, whose problem maker and ``.cuda()`` handling it shares; nothing of the reference is written
anywhere but the numbers in tests/golden/align_pose_loss_cases.npz.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_align_pose_loss.py <root of the reference checkout>

Conditioning cap - a condition on the stored cases, not a measurement: for every pair and iteration 0.05 <= err_r <= pi - 0.05 rad
and err_t >= 1e-2, so that 1 / sqrt(1 - s^2) <= 20 in the reference's own float32 and its autograd is not the noisy side of a
comparison.  A draw that misses the cap is discarded and the next seed is drawn; the accepted seed is stored with the case.

The problem maker's own solutions land 0.004 - 0.09 rad from the pair's true pose at these sizes and outlier rates (0.3 - 0.6, its
weakly separating logits) - under the cap's floor in every draw.  The ground truth handed to the loss is therefore the true pose
followed by a seeded offset (0.15 - 0.5 rad about a random axis, 0.05 - 0.3 per axis of translation), as a pair early in training
presents itself; the match list, and with it the confidence term's labels, stay those of the true pose."""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden_align_loss import make_case  # noqa: E402

# (P, J, K, n_iter, loss_type, wt_ptDist, wt_inlier, wt_pose, outlier rate)
CASES = [(2, 600, 600, 3, "mae", 1.0, 1.0, 0.5, 0.3),
         (3, 257, 300, 2, "mse", 1.0, 1.0, 2.0, 0.4),
         (1, 100, 130, 1, "mae", 0.0, 0.0, 1.0, 0.5),        # the pose term alone, fewer rows than the workgroup has threads
         (1, 1500, 1700, 5, "mae", 1.0, 1.0, 1.0, 0.6),      # more rows than threads
         (2, 320, 320, 8, "mae", 1.0, 0.0, 0.25, 0.45)]      # the n_iter ceiling
MAX_TRIES = 200


def offset_pose(rng, T):
    """[3,4] float32 -> the pose followed by a seeded rigid offset (module docstring)."""
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    ang = rng.uniform(0.15, 0.5)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    dR = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    dt = rng.uniform(0.05, 0.3, 3) * rng.choice([-1.0, 1.0], 3)
    T = T.astype(np.float64)
    return np.concatenate([dR @ T[:, :3], (dR @ T[:, 3] + dt)[:, None]], 1).astype(np.float32)


def main(ref_root):
    warnings.filterwarnings("ignore")
    sys.path.insert(0, ref_root)
    import arguments  # type: ignore
    import network.model as ref_model  # type: ignore
    from common.math import se3_torch  # type: ignore
    from network.loss import ScanAlignmentLoss, batch_rotation_error, batch_translation_error  # type: ignore

    args = arguments.train_arguments().parse_args([]) if hasattr(arguments, "train_arguments") else arguments.eval_arguments().parse_args([])
    out = {}
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self                       # no GPU here; see oracle/gen_golden_align_loss.py
    try:
        for c, (B, J, K, n_iter, ltype, wt_pt, wt_in, wt_pose, outl) in enumerate(CASES):
            args.loss_type, args.wt_ptDist_loss, args.wt_inlier_loss, args.wt_pose_loss, args.loss_discount_factor = ltype, wt_pt, wt_in, wt_pose, 0.5
            loss_fn = ScanAlignmentLoss(args)
            for attempt in range(MAX_TRIES):
                rng = np.random.Generator(np.random.Philox(key=[2025 + c, attempt]))
                src, ref, gt, matches, idx, logits = make_case(rng, B, J, K, n_iter, outl)
                gt = np.stack([offset_pose(rng, T) for T in gt])
                ps, pr = torch.from_numpy(src), torch.from_numpy(ref)
                lg = [torch.from_numpy(logits[i]).requires_grad_(True) for i in range(n_iter)]
                xyz = ps
                transforms, pred_pairs = [], []
                for i in range(n_iter):
                    ix = torch.from_numpy(idx[i])
                    ref_new = torch.gather(pr, 1, ix[:, :, None].expand(-1, -1, 3))
                    R_t, bad = ref_model.compute_rigid_transform_2(xyz, ref_new, weights=lg[i].sigmoid()[:, :, None])
                    assert not bad
                    xyz = se3_torch.transform(R_t.detach(), xyz)
                    transforms.append(R_t if i == 0 else se3_torch.concatenate(R_t, transforms[-1]))
                    ar = torch.arange(J)[None, :, None].expand(B, J, 1).int()
                    pred_pairs.append(torch.cat([ar, ix.int()[:, :, None]], dim=2))
                tg = torch.from_numpy(gt)
                with torch.no_grad():
                    err_r = torch.stack([batch_rotation_error(tg[:, :3, :3], t[:, :3, :3]) for t in transforms]).numpy()
                    err_t = torch.stack([batch_translation_error(tg[:, :3, 3], t[:, :3, 3]) for t in transforms]).numpy()
                if err_r.min() >= 0.05 and err_r.max() <= np.pi - 0.05 and err_t.min() >= 1e-2:
                    break
            else:
                raise SystemExit(f"case {c}: no seed in {MAX_TRIES} meets the conditioning cap")
            data = {"pt_src": ps, "perm_matrices": lg, "transform_pred": transforms, "transform_gt": tg,
                    "pred_pairs": pred_pairs, "matches": [torch.from_numpy(m) for m in matches]}
            d = loss_fn(data, reduction="mean")
            d["total"].backward()
            with torch.no_grad():
                dn = loss_fn(data, reduction="none")
            labels = np.stack([loss_fn.find_correct_correspondence(data["matches"], pred_pairs[i], hash_seed=J) for i in range(n_iter)])
            out[f"c{c}_src"], out[f"c{c}_ref"], out[f"c{c}_gt"] = src, ref, gt
            out[f"c{c}_idx"], out[f"c{c}_logits"], out[f"c{c}_labels"] = idx.astype(np.int32), logits, labels.astype(np.float32)
            out[f"c{c}_transforms"] = np.stack([t.detach().numpy() for t in transforms], 1)
            out[f"c{c}_grad_logits"] = np.stack([l.grad.numpy() for l in lg])
            names = sorted(d.keys())
            assert names == sorted(dn.keys())
            out[f"c{c}_loss_names"] = np.array(names)
            out[f"c{c}_loss_values"] = np.array([float(d[k]) for k in names], np.float64)
            out[f"c{c}_loss_per_pair"] = np.stack([np.broadcast_to(dn[k].detach().numpy().astype(np.float64), (B,)) for k in names])
            out[f"c{c}_loss_type"] = np.array(ltype)
            out[f"c{c}_weights"] = np.array([wt_pt, wt_in, wt_pose, 0.5], np.float64)      # ptDist, inlier, pose, discount
            out[f"c{c}_err_r"], out[f"c{c}_err_t"] = err_r, err_t                             # [n_iter][B], the cap's evidence
            out[f"c{c}_seed"] = np.array([2025 + c, attempt])
            print(f"case {c}: seed attempt {attempt}, total {float(d['total']):.6f}, |grad| max {np.abs(out[f'c{c}_grad_logits']).max():.3e}, "
                  f"err_r in [{err_r.min():.3f}, {err_r.max():.3f}], err_t min {err_t.min():.3f}, keys {names}")
    finally:
        torch.Tensor.cuda = orig_cuda
    out["n_cases"] = np.asarray(len(CASES))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "align_pose_loss_cases.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
