"""The half-space crop RULE, written down once on the host (numpy): the restatement csrc/crop.hip is tested against and the
generator of the per-cloud direction the device path uploads.

The reference crops with ``Transforms.RandomCrop.crop`` (dataloader/transformation.py:121-145): a direction from numpy's global
RNG, the projection of the centred cloud onto it, and ``dist > np.percentile(dist, (1 - p_keep) * 100)``.  Neither the RNG nor
the rounding of the percentile's interpolation can be pinned, so the rule is this project's own, like the augmentation rule of
deepsir_amd/augment.py whose keys and draws it uses.

Direction.  Two uniforms of the cloud key ``cloud_key(seed, epoch, index, side)`` on stream ``STREAM_CROP``:

    z = 2 u0 - 1,  phi = 2 pi u1,  r = sqrt(1 - z^2),  u = (r cos phi, r sin phi, z)      float64, rounded to fp32 once

Projection.  m = float64 mean xyz of the WHOLE cloud rounded to fp32 (``augment.centroid``, dsir_t_cloud_centroids); per row, fp32,
every operation rounded on its own, no fused multiply-add:

    d_j = ((px - mx) ux + (py - my) uy) + (pz - mz) uz

Threshold by rank.  With n rows: v = (n - 1) * (((1.0 - p_keep) * 100) / 100) in float64 (numpy's expression for the virtual
index of the percentile, in numpy's order of operations), lo = floor(v), and row j is kept iff d_j > d_(lo), the lo-th smallest
projection (0-based), compared as fp32 values (-0 equals +0).  ``p_keep == 0.5`` keeps the reference's special case d_j > 0;
``p_keep >= 1`` keeps every row.  Kept rows stay in input order, all columns copied.

This is what ``dist > np.percentile(dist, q)`` keeps in exact arithmetic.  numpy interpolates d_(lo) + frac(v) (d_(lo+1) - d_(lo));
when v lies within rounding of an integer from below (frac(v) > 1 - 1e-9) that threshold rounds onto d_(lo+1) and numpy keeps
one row fewer than this rule.  Nowhere else do the two differ.

Refusals, per cloud, never errors (bits of ``augment.INVALID_*``), decided in this order:
  * no rows: count 0, INVALID_EMPTY;
  * a non-finite centroid: count 0, INVALID_NONFINITE;
  * (``p_keep >= 1`` keeps every row of any other cloud, whatever its projections would be;)
  * a row with a non-finite projection is dropped but still counts in n; its sort key is the largest, so it sits at rank lo only
    when at most lo rows are finite, and then the cloud's count is 0 with INVALID_NONFINITE;
  * a cloud none of whose rows is kept (all projections equal, a single row) has count 0 and INVALID_EMPTY: what comes out is an
    empty cloud.
"""
from __future__ import annotations

import math
from typing import Sequence, Tuple

import numpy as np

from .augment import INVALID_EMPTY, INVALID_NONFINITE, MASK, centroid, splitmix64, uniform

STREAM_CROP = 5
KEY_NONFINITE = 0xFFFFFFFF


def _direction(u0: float, u1: float) -> Tuple[float, float, float]:
    """The unit vector of two uniforms, float64 (python's scalar libm: the same number wherever in a call the cloud sits)."""
    z = 2.0 * u0 - 1.0
    phi = 2.0 * math.pi * u1
    r = math.sqrt(1.0 - z * z)
    return r * math.cos(phi), r * math.sin(phi), z


def crop_direction(key: int) -> np.ndarray:
    """Unit direction [3] float32 of a cloud key: uniform on the sphere from two draws of STREAM_CROP."""
    u = uniform(key, STREAM_CROP, np.arange(2))
    return np.array(_direction(float(u[0]), float(u[1])), np.float64).astype(np.float32)


def crop_directions(seed: int, epoch: int, indices: Sequence[int], sides: Sequence[int]) -> np.ndarray:
    """[clouds, 3] float32: the direction of every (index, side) of a call - `crop_direction(cloud_key(seed, epoch, index, side))`
    with the keys and draws of all clouds formed in one pass over uint64 arrays (per call this is the host's whole share)."""
    n = len(indices)
    if n == 0:
        return np.zeros((0, 3), np.float32)
    k = splitmix64(splitmix64(int(seed) & MASK) ^ (int(epoch) & MASK))
    idx = np.array([int(i) & MASK for i in indices], np.uint64)
    sd = np.array([int(x) & MASK for x in np.broadcast_to(np.asarray(sides), (n,))], np.uint64)
    keys = splitmix64(splitmix64(np.uint64(k) ^ idx) ^ sd)
    base = keys ^ np.uint64(STREAM_CROP << 40)
    u = (np.stack([splitmix64(base), splitmix64(base ^ np.uint64(1))], 1) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return np.array([_direction(a, b) for a, b in u.tolist()], np.float64).astype(np.float32)


def rank_index(n: int, p_keep: float) -> int:
    """lo = floor of numpy's virtual index of the (1 - p_keep) * 100 percentile of n values."""
    v = (n - 1) * (((1.0 - float(p_keep)) * 100) / 100)
    return min(max(int(np.floor(v)), 0), max(n - 1, 0))


def projection(points: np.ndarray, direction: np.ndarray, m: np.ndarray) -> np.ndarray:
    """d_j [n] float32 of the rule; m the float64 centroid (rounded to fp32 here)."""
    p = np.ascontiguousarray(points[:, :3], np.float32)
    u, c = np.asarray(direction, np.float32), np.asarray(m, np.float64).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return ((p[:, 0] - c[0]) * u[0] + (p[:, 1] - c[1]) * u[1]) + (p[:, 2] - c[2]) * u[2]


def order_key(d: np.ndarray) -> np.ndarray:
    """The order-preserving 32-bit key of fp32 values (uint32): -0 keyed as +0, a non-finite value as KEY_NONFINITE."""
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore"):
        bits = (d + np.float32(0.0)).view(np.uint32)            # -0 + 0 = +0
    key = np.where(bits >> np.uint32(31), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isfinite(d), key, np.uint32(KEY_NONFINITE)).astype(np.uint32)


def keep_mask(d: np.ndarray, p_keep: float) -> Tuple[np.ndarray, int]:
    """The rule on projections alone: (mask [n] bool, invalid bits).  d fp32, n >= 1, p_keep < 1."""
    key = order_key(d)
    finite = key != np.uint32(KEY_NONFINITE)
    if float(p_keep) == 0.5:
        mask = finite & (key > order_key(np.zeros(1, np.float32))[0])
    else:
        key_lo = np.partition(key, rank_index(len(key), p_keep))[rank_index(len(key), p_keep)]
        if key_lo == np.uint32(KEY_NONFINITE):
            return np.zeros(len(key), bool), INVALID_NONFINITE
        mask = finite & (key > key_lo)
    return mask, (0 if mask.any() else INVALID_EMPTY)


def halfspace_crop_host(points: np.ndarray, p_keep: float, direction: np.ndarray) -> Tuple[np.ndarray, int]:
    """points [n, C] float32 -> (kept rows [n', C] float32 in input order, invalid bits)."""
    pts = np.ascontiguousarray(points, np.float32)
    n = pts.shape[0]
    if n == 0:
        return pts[:0].copy(), INVALID_EMPTY
    m = centroid(pts)
    if not np.isfinite(m).all():
        return pts[:0].copy(), INVALID_NONFINITE
    if float(p_keep) >= 1.0:
        return pts.copy(), 0
    mask, invalid = keep_mask(projection(pts, direction, m), p_keep)
    return pts[mask].copy(), invalid
