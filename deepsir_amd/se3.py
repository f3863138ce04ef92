"""SE(3) helpers on ``[B,3,4]`` tensors — host-side mirror of the reference's
common/math/se3_torch.py:6-77 (identity / inverse / concatenate / transform),
used by the evaluation harness.  Inside the registration loop the same algebra
runs in the Kabsch kernel (csrc/kabsch.hip)."""
import torch


def identity(batch_size: int) -> torch.Tensor:
    return torch.eye(3, 4)[None].repeat(batch_size, 1, 1)


def inverse(Rt: torch.Tensor) -> torch.Tensor:
    R, t = Rt[..., :3, :3], Rt[..., :3, 3]
    Rt_ = R.transpose(-1, -2)
    return torch.cat([Rt_, Rt_ @ -t[..., None]], dim=-1)


def concatenate(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a o b : apply b first, then a."""
    Ra, ta, Rb, tb = a[..., :3, :3], a[..., :3, 3], b[..., :3, :3], b[..., :3, 3]
    return torch.cat([Ra @ Rb, Ra @ tb[..., None] + ta[..., None]], dim=-1)


def transform(Rt: torch.Tensor, pts: torch.Tensor) -> torch.Tensor:
    """pts [B,N,3] -> pts R^T + t."""
    return pts @ Rt[..., :3, :3].transpose(-1, -2) + Rt[..., :3, 3][..., None, :]


def xyzquat2mat(xyzquat):
    """[x, y, z, qw, qx, qy, qz] -> the [4, 4] float64 pose (numpy) with that translation and the rotation of the quaternion: the
    reference's common/math/se3.py:140-153 as its Oxford loader calls it (dataloader/oxford_loader.py:163-166).  The quaternion is
    normalised first (a near-zero one gives the identity rotation), then the standard unit-quaternion matrix."""
    import numpy as np
    v = np.asarray(xyzquat, np.float64).reshape(7)
    q = v[3:]
    nq = float(q @ q)
    M = np.eye(4)
    M[:3, 3] = v[:3]
    if nq < 1e-8:
        return M
    w, x, y, z = q / np.sqrt(nq)
    M[:3, :3] = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                 [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                 [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]
    return M
