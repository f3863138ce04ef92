"""The training augmentation RULE, written down once on the host (numpy): the restatement csrc/augment.hip is tested against and
the generator of the handful of per-cloud numbers the device path uploads.

The reference augments with numpy's global RNG, an unseeded ``np.random.RandomState()`` and python's ``random.random()``
(dataloader/data_base.py:221-296, :397-407; dataloader/transformation.py:63-107, :239-297): nothing there can be pinned, so
the rule is this project's own, like the resampling rule of csrc/preprocess.hip.

Random numbers.  Every number is ``splitmix64`` of a key:

    cloud key  k = sm(sm(sm(sm(seed) ^ epoch) ^ index) ^ side)        side: 0 = src, 1 = ref, 2 = the pair
    draw       d = sm(k ^ (stream << 40) ^ element)                   uniform u = (d >> 11) 2^-53 in [0, 1), float64

``index`` is the sample's index in its dataset - never its position in a batch, the batch size or a process rank - so a sample is
the same bytes whatever batch it lands in.  Streams:

    STREAM_PARAM   the cloud's own parameters (elements 0-2 axis, 3 angle | 4 z angle, 5-7 Euler angles, 8-10 translation)
                   and, under the PAIR key, 0 jitter gate, 1 scale gate, 2 scale
    STREAM_PERM    sort keys of the resampling permutation, element = input row      (the rule of dsir_resample, keyed by the
    STREAM_TOPUP   top-up rows drawn with replacement, element = output row           cloud instead of its position in the call)
    STREAM_JITTER  element = 8 * output row + 2 * coordinate + {0, 1}

Per point (fp32, every operation rounded, no fused multiply-add; R, t, s and the centroid m rounded to fp32 once):

    d = p - m                                   (only where the transform is about the centroid; m = mean of the WHOLE cloud)
    r_i = ((R_i0 d_0 + R_i1 d_1) + R_i2 d_2) + t_i
    q_i = r_i + jitter_i                        (only where the jitter gate fired)
    out_i = s q_i                               (only where the scale gate fired)

in the reference's order rotate -> resample -> jitter -> scale (the rotation is pointwise, so it is applied after the gather).

Deviations from the reference:
  * scale: the ground-truth translation is scaled with the clouds (``reference_gt=True`` keeps the reference's unscaled one);
  * columns 3:6 are rotated only when the caller says they are normals (``normals=True``);
  * an empty cloud (bit 0, rows zero) or a non-finite centroid (bit 1) is flagged per cloud, not an error.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

MASK = (1 << 64) - 1
STREAM_PARAM, STREAM_PERM, STREAM_TOPUP, STREAM_JITTER, STREAM_ORDER = 0, 1, 2, 3, 4
SIDE_SRC, SIDE_REF, SIDE_PAIR = 0, 1, 2
JITTER_NONE, JITTER_UNIFORM, JITTER_NORMAL = 0, 1, 2
RESAMPLE_RANDOM, RESAMPLE_FIXED, RESAMPLE_PERMUTED_FIXED = 0, 1, 2
INVALID_EMPTY, INVALID_NONFINITE = 1, 2
PARAM_SLOTS = 24            # 8-byte slots of one cloud's parameter block (csrc/augment.hip, struct AugParams)


def splitmix64(x):
    """splitmix64 of a python int or a uint64 array (the function of csrc/preprocess.hip)."""
    if isinstance(x, (int, np.integer)):
        z = (int(x) + 0x9E3779B97F4A7C15) & MASK
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        return z ^ (z >> 31)
    with np.errstate(over="ignore"):
        z = np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def cloud_key(seed: int, epoch: int, index: int, side: int) -> int:
    k = splitmix64(int(seed) & MASK)
    for v in (epoch, index, side):
        k = splitmix64(k ^ (int(v) & MASK))
    return k


def draws(key: int, stream: int, elements) -> np.ndarray:
    """uint64 draws of a key's stream at the given element indices."""
    e = np.asarray(elements, dtype=np.uint64)
    return splitmix64(np.uint64(int(key) ^ (int(stream) << 40)) ^ e)


def uniform(key: int, stream: int, elements) -> np.ndarray:
    """float64 in [0, 1): the top 53 bits of the draw."""
    return (draws(key, stream, elements) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def epoch_order(seed: int, epoch: int, n: int, shuffle: bool = True) -> np.ndarray:
    """The epoch's sample order: the permutation that sorts the draws of (seed, epoch) (ties by index)."""
    if not shuffle:
        return np.arange(n)
    k = splitmix64(splitmix64(int(seed) & MASK) ^ (int(epoch) & MASK))
    return np.argsort(draws(k, STREAM_ORDER, np.arange(n)), kind="stable")


@dataclass
class AugmentConfig:
    """The switches of DataBase.apply_augment (variant 'v1', 3DMatch) / apply_augment_V2 ('v2', KITTI)."""
    variant: str = "v1"
    num_points: int = 0
    fixed: bool = False                 # v1: FixedResampler instead of Resampler
    random_rotation: bool = True
    rotation_range: float = 90.0        # v1, degrees
    random_jitter: bool = True
    jitter_scale: float = 0.005         # v1: uniform[0, 1) * jitter_scale
    jitter_sigma: float = 0.01          # v2: RandomJitter(scale, clip)
    jitter_clip: float = 0.05
    random_scale: bool = True
    min_scale: float = 0.8
    max_scale: float = 1.2
    gate: float = 0.95                  # v1: probability of jitter / of scale
    z_rot_mag: float = 60.0             # v2: RandomRotatorZ(60)
    rot_mag: float = 45.0               # v2: RandomTransformSE3_euler
    trans_mag: float = 2.0
    xy_rot_scale: float = 1.0
    normals: bool = False               # columns 3:6 are normals: rotate them
    reference_gt: bool = False          # keep the reference's unscaled ground-truth translation
    permute: bool = True                # v2: permute before FixedResampler (the Oxford loader's val / test: False)


def rodrigues(axis: np.ndarray, theta: float) -> np.ndarray:
    """expm of the skew matrix of axis / |axis| * theta (data_base.py:391-394) in closed form."""
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt((a * a).sum())
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)


def rot_z(a: float) -> np.ndarray:
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def euler_xyz(ax: float, ay: float, az: float) -> np.ndarray:
    """Rx Ry Rz of RandomTransformSE3_euler (transformation.py:257-272)."""
    cx, cy, sx, sy = np.cos(ax), np.cos(ay), np.sin(ax), np.sin(ay)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    return Rx @ Ry @ rot_z(az)


@dataclass
class CloudParams:
    """One cloud's parameter block (float64 on the host; the device rounds R, t, s to fp32 once)."""
    R: np.ndarray
    t: np.ndarray
    scale: float = 1.0
    scaled: bool = False
    jitter_mode: int = JITTER_NONE
    jitter_scale: float = 0.0
    jitter_clip: float = 0.0
    centered: bool = False
    normals: bool = False
    key: int = 0
    resample_mode: int = RESAMPLE_RANDOM


def pair_params(cfg: AugmentConfig, seed: int, epoch: int, index: int) -> Tuple[CloudParams, CloudParams]:
    """The per-cloud numbers of one sample (src, ref): everything random that is not per point."""
    out = []
    kp = cloud_key(seed, epoch, index, SIDE_PAIR)
    g = uniform(kp, STREAM_PARAM, np.arange(3))
    v1 = cfg.variant == "v1"
    if cfg.variant not in ("v1", "v2"):
        raise ValueError(f"unknown augmentation variant {cfg.variant!r}")
    jitter_on = cfg.random_jitter and (g[0] < cfg.gate if v1 else True)
    scale_on = cfg.random_scale and (g[1] < cfg.gate if v1 else True)
    scale = cfg.min_scale + (cfg.max_scale - cfg.min_scale) * g[2] if scale_on else 1.0
    for side in (SIDE_SRC, SIDE_REF):
        k = cloud_key(seed, epoch, index, side)
        u = uniform(k, STREAM_PARAM, np.arange(11))
        R, t, centered = np.eye(3), np.zeros(3), False
        if cfg.random_rotation and v1:                 # sample_random_trans, about the centroid
            R = rodrigues(u[0:3] - 0.5, cfg.rotation_range * np.pi / 180.0 * (u[3] - 0.5))
            centered = True
        elif cfg.random_rotation:                      # RandomRotatorZ, then (src only) RandomTransformSE3_euler
            R = rot_z(u[4] * cfg.z_rot_mag * np.pi / 180.0)
            if side == SIDE_SRC:
                a = u[5:8] * np.pi * cfg.rot_mag / 180.0 * np.array([cfg.xy_rot_scale, cfg.xy_rot_scale, 1.0])
                R = euler_xyz(a[0], a[1], a[2]) @ R
                t = (2.0 * u[8:11] - 1.0) * cfg.trans_mag
        if v1:
            mode = RESAMPLE_FIXED if cfg.fixed else RESAMPLE_RANDOM
            jm, js, jc = (JITTER_UNIFORM, cfg.jitter_scale, 0.0) if jitter_on else (JITTER_NONE, 0.0, 0.0)
        else:
            mode = RESAMPLE_PERMUTED_FIXED if cfg.permute else RESAMPLE_FIXED
            jm, js, jc = (JITTER_NORMAL, cfg.jitter_sigma, cfg.jitter_clip) if jitter_on else (JITTER_NONE, 0.0, 0.0)
        out.append(CloudParams(R, t, float(scale), bool(scale_on), jm, js, jc, centered, cfg.normals, k, mode))
    return out[0], out[1]


def pack_params(params: List[CloudParams]) -> np.ndarray:
    """[clouds][PARAM_SLOTS] float64 whose integer slots hold int64 / uint64 bit patterns (struct AugParams)."""
    a = np.zeros((len(params), PARAM_SLOTS), np.float64)
    i = a.view(np.uint64)
    for c, p in enumerate(params):
        a[c, 0:9] = np.asarray(p.R, np.float64).reshape(9)
        a[c, 9:12] = p.t
        a[c, 12], a[c, 13], a[c, 14] = p.scale, p.jitter_scale, p.jitter_clip
        i[c, 15], i[c, 16], i[c, 17], i[c, 18] = p.jitter_mode, int(p.centered), int(p.normals), p.key
        i[c, 19], i[c, 20] = p.resample_mode, int(p.scaled)
    return a


def resample_rows(key: int, n: int, k: int, mode: int) -> np.ndarray:
    """Source row of every output row: Resampler (random order, top-up with replacement), FixedResampler (tile) or the
    KITTI loader's permutation followed by FixedResampler."""
    j = np.arange(k)
    if n <= 0:
        return np.zeros(k, np.int64)
    if mode == RESAMPLE_FIXED:
        return j % n
    perm = np.argsort(draws(key, STREAM_PERM, np.arange(n)) >> np.uint64(1), kind="stable")
    if mode == RESAMPLE_PERMUTED_FIXED:
        return perm[j % n]
    rows = np.empty(k, np.int64)
    m = min(n, k)
    rows[:m] = perm[:m]
    if k > n:
        rows[n:] = (draws(key, STREAM_TOPUP, j[n:]) % np.uint64(n)).astype(np.int64)
    return rows


def jitter(key: int, k: int, mode: int, scale: float, clip: float) -> np.ndarray:
    """[k, 3] float32: float64 arithmetic, rounded once."""
    if mode == JITTER_NONE:
        return np.zeros((k, 3), np.float32)
    e = (np.arange(k)[:, None] * 8 + np.arange(3)[None, :] * 2)
    if mode == JITTER_UNIFORM:
        return (uniform(key, STREAM_JITTER, e) * scale).astype(np.float32)
    u1 = ((draws(key, STREAM_JITTER, e) >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0 ** -53      # (0, 1]
    u2 = uniform(key, STREAM_JITTER, e + 1)
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)                                         # Box-Muller
    return np.clip(scale * z, -clip, clip).astype(np.float32)


def centroid(points: np.ndarray) -> np.ndarray:
    """float64 mean xyz of a cloud; zeros for an empty one."""
    if len(points) == 0:
        return np.zeros(3)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(points[:, :3], np.float64).sum(0) / len(points)


def augment_cloud(points: np.ndarray, p: CloudParams, k: int):
    """points [n, C] float32 -> (out [k, C] float32, rows [k], invalid bits, centroid float64 [3])."""
    pts = np.ascontiguousarray(points, np.float32)
    n, C = pts.shape
    m = centroid(pts)
    invalid = (INVALID_EMPTY if n == 0 else 0) | (0 if np.isfinite(m).all() else INVALID_NONFINITE)
    rows = resample_rows(p.key, n, k, p.resample_mode)
    if n == 0:
        return np.zeros((k, C), np.float32), rows, invalid, m
    out = pts[rows].copy()
    R, t, f = p.R.astype(np.float32), np.asarray(p.t).astype(np.float32), np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        d = out[:, :3] - m.astype(np.float32) if p.centered else out[:, :3].copy()
        q = np.stack([((R[i, 0] * d[:, 0] + R[i, 1] * d[:, 1]) + R[i, 2] * d[:, 2]) + t[i] for i in range(3)], 1).astype(f)
        if p.jitter_mode != JITTER_NONE:
            q = q + jitter(p.key, k, p.jitter_mode, p.jitter_scale, p.jitter_clip)
        if p.scaled:
            q = f(p.scale) * q
        out[:, :3] = q
        if p.normals and C >= 6:
            v = out[:, 3:6].copy()
            out[:, 3:6] = np.stack([(R[i, 0] * v[:, 0] + R[i, 1] * v[:, 1]) + R[i, 2] * v[:, 2] for i in range(3)], 1)
    return out, rows, invalid, m


def compose_gt(M: np.ndarray, ps: CloudParams, pr: CloudParams, m_src: np.ndarray, m_ref: np.ndarray,
               reference_gt: bool = False) -> np.ndarray:
    """transform_gt [3, 4] float32 = A_ref M A_src^-1 with A = [R | t - R m] (m = the fp32-rounded centroid where the transform is
    about it, else 0), float64 throughout, rounded to fp32 when it leaves; the translation times the scale unless reference_gt."""
    def affine(p, m):
        A = np.eye(4)
        A[:3, :3] = p.R
        mm = m.astype(np.float32).astype(np.float64) if p.centered else np.zeros(3)
        A[:3, 3] = p.t - p.R @ mm
        return A
    M4 = np.eye(4)
    M4[:M.shape[0], :] = M
    As, Ar = affine(ps, m_src), affine(pr, m_ref)
    Ai = np.eye(4)
    Ai[:3, :3] = As[:3, :3].T
    Ai[:3, 3] = -As[:3, :3].T @ As[:3, 3]
    T = Ar @ M4 @ Ai
    if ps.scaled and not reference_gt:
        T[:3, 3] *= ps.scale
    return T[:3, :].astype(np.float32)


def augment_pair(src: np.ndarray, ref: np.ndarray, M: np.ndarray, cfg: AugmentConfig, seed: int, epoch: int, index: int,
                 k: Optional[int] = None) -> Dict[str, object]:
    """One sample through the whole rule on the host."""
    ps, pr = pair_params(cfg, seed, epoch, index)
    k = int(k or cfg.num_points)
    so, srows, sinv, ms = augment_cloud(src, ps, k)
    ro, rrows, rinv, mr = augment_cloud(ref, pr, k)
    with np.errstate(invalid="ignore"):
        gt = compose_gt(np.asarray(M, np.float64), ps, pr, ms, mr, cfg.reference_gt)
    return {"points_src": so, "points_ref": ro, "transform_gt": gt, "invalid": np.array([sinv, rinv], np.int32),
            "rows_src": srows, "rows_ref": rrows, "params": (ps, pr)}
