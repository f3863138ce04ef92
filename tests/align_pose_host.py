"""The differentiable tail of the `align` training step, restated in float64 and differentiated by torch's autograd in double
precision (a helper of tests/test_align_pose_loss.py; TEST INFRASTRUCTURE).  Written from the formulas in
deepsir_amd/csrc/align_loss.hip's header and include/dsir.h:

    w = sigmoid(x),  wn = w / (sum |w| + 1e-16),  c_s = sum wn s,  c_t = sum wn t,  H = sum wn (s - c_s)(t - c_t)^T = U S V^T,
    R = V diag(1, 1, d) U^T with d = sign det(V U^T),  t = -R c_s + c_t,  src <- T.detach() src,  Tc_i = T_i o Tc_{i-1},
    dist_i = mean |Tc_i p - T_gt p| (mae) or its square (mse),  outlier_i = wt_inlier BCEWithLogits(x_i, y_i),
    s_i = (<R_gt, Rc_i>_F - 1) / 2,  err_r = acos(clamp(s_i, -1, 1)),  err_t = |t_gt - tc_i|,
    poseError_i = wt_pose (mean err_r + mean err_t)      ('none': (err_r + err_t) wt_pose per pair),
    total = sum over the keys of discount^(n_iter - 1 - i) x the key's value.

The two corner rules of the pose term are built into the graph, so autograd itself returns what the kernel must: where
1 - s_i^2 <= 0 the rotation error is the CONSTANT acos(clamp(s_i)) (zero gradient), and where err_t == 0 torch.norm's own
subgradient is zero."""
import numpy as np
import torch
import torch.nn.functional as F


def kabsch(src, tgt, w):
    """src, tgt [B,J,3], w [B,J] (float64) -> [B,3,4]."""
    wn = (w / (w.abs().sum(1, keepdim=True) + 1e-16))[:, :, None]
    cs, ct = (src * wn).sum(1), (tgt * wn).sum(1)
    H = (src - cs[:, None]).transpose(1, 2) @ ((tgt - ct[:, None]) * wn)
    U, _, Vh = torch.linalg.svd(H)
    V = Vh.transpose(1, 2)
    d = torch.sign(torch.linalg.det(V @ U.transpose(1, 2))).detach()
    D = torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], 1))
    R = V @ D @ U.transpose(1, 2)
    t = -(R @ cs[:, :, None])[:, :, 0] + ct
    return torch.cat([R, t[:, :, None]], 2)


def apply(T, p):
    return p @ T[:, :, :3].transpose(1, 2) + T[:, None, :, 3]


def compose(A, B):
    """A o B: first B, then A."""
    return torch.cat([A[:, :, :3] @ B[:, :, :3], A[:, :, :3] @ B[:, :, 3:] + A[:, :, 3:]], 2)


def chain(src, ref, idx, logits):
    """The cumulative transforms Tc_i, list of [B,3,4], from the logits on."""
    xyz, out = src, []
    for i in range(len(logits)):
        tgt = torch.gather(ref, 1, idx[i][:, :, None].expand(-1, -1, 3))
        T = kabsch(xyz, tgt, torch.sigmoid(logits[i]))
        xyz = apply(T.detach(), xyz)
        out.append(T if i == 0 else compose(T, out[-1]))
    return out


def pose_errors(Tc, gt):
    """err_r, err_t [B] with the corner rules (module docstring)."""
    s = ((gt[:, :, :3] * Tc[:, :, :3]).sum((1, 2)) - 1.0) / 2.0
    inside = (1.0 - s * s) > 0
    safe = torch.where(inside, s, torch.zeros_like(s))                       # keeps acos' derivative finite on the other branch
    err_r = torch.where(inside, torch.acos(safe), torch.acos(s.detach().clamp(-1.0, 1.0)))
    err_t = torch.linalg.vector_norm(gt[:, :, 3] - Tc[:, :, 3], dim=1)      # zero subgradient at 0
    return err_r, err_t


def loss_terms(src, Tc, gt, logits, labels, loss_type, wt_pt, wt_in, wt_pose, discount, reduction):
    n, d = len(Tc), {}
    want = apply(gt, src)
    mean = (lambda v: v.mean()) if reduction == "mean" else (lambda v: v.reshape(v.shape[0], -1).mean(1))
    for i in range(n):
        if wt_pt > 0:
            df = apply(Tc[i], src) - want
            d[f"{loss_type}_{i}"] = mean(df.abs() if loss_type == "mae" else df * df)
        else:
            d[f"{loss_type}_{i}"] = mean(torch.zeros_like(src))
    if wt_in > 0 and labels is not None:
        for i in range(n):
            d[f"outlier_{i}"] = mean(F.binary_cross_entropy_with_logits(logits[i], labels[i], reduction="none") * wt_in)
    if wt_pose > 0:
        for i in range(n):
            er, et = pose_errors(Tc[i], gt)
            d[f"poseError_{i}"] = (er.mean() + et.mean()) * wt_pose if reduction == "mean" else (er + et) * wt_pose
    d["total"] = sum(v * discount ** (n - 1 - int(k[k.rfind("_") + 1:])) for k, v in list(d.items()))
    return d


def loss_and_grad(src, ref, idx, logits, labels, gt, loss_type="mae", wt_pt=1.0, wt_in=1.0, wt_pose=0.0, discount=0.5):
    """numpy in (idx, logits, labels [n,B,J]; labels may be None) -> (values for 'mean', per-pair values for 'none',
    d total / d logits [n,B,J] float64, transforms [B,n,3,4] float64)."""
    f = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    ps, pr, g = f(src), f(ref), f(gt)
    lg = [f(l).requires_grad_(True) for l in logits]
    ix = [torch.from_numpy(np.asarray(i, np.int64)) for i in idx]
    lb = None if labels is None else [f(l) for l in labels]
    Tc = chain(ps, pr, ix, lg)
    d = loss_terms(ps, Tc, g, lg, lb, loss_type, wt_pt, wt_in, wt_pose, discount, "mean")
    d["total"].backward()
    with torch.no_grad():
        pp = loss_terms(ps, Tc, g, lg, lb, loss_type, wt_pt, wt_in, wt_pose, discount, "none")
    grad = np.stack([np.zeros(l.shape) if l.grad is None else l.grad.numpy() for l in lg])
    return ({k: float(v.detach()) for k, v in d.items()}, {k: v.numpy() for k, v in pp.items()}, grad,
            np.stack([t.detach().numpy() for t in Tc], 1))
