"""Plane segmentation: the rule of csrc/plane.hip (dsir_segment_plane, Engine.segment_plane) restated in numpy.  What open3d's
``segment_plane`` and PCL's ``SACSegmentation`` do; open3d cannot be imported here, so parity is unpinned and the rule is the engine's
own.  Host code for tests and for reading; the engine never calls it.

The rule, per cloud and round ``j`` (a row is *live* iff it is below the count, finite in xyz and not yet taken by a plane):

* draw ``k`` of hypothesis ``h``: ``d = splitmix64(splitmix64(seed ^ (id << 40)) ^ (j << 32) ^ (h << 8) ^ k)``,
  ``r_k = ((d >> 32) * n_live) >> 32``, the ``r_k``-th live row in ascending row order; ``n_live < 3`` or a repeated row rejects;
* fit in float64 from the fp32 rows ``a, b, c``: ``m = (b - a) x (c - a)``, ``len2 = (mx mx + my my) + mz mz`` (rejected unless
  positive and finite), ``n = m / sqrt(len2)``; candidate = (``n``, anchor ``a``) rounded to fp32 once; with an axis rejected unless
  ``|n . axis| >= cos_min`` in float64 before the rounding;
* score in fp32, every operation rounded on its own: ``e = ((nx (x - ax)) + (ny (y - ay))) + (nz (z - az))``, inlier iff
  ``|e| < thr``; the integer count over the live rows; the largest count wins, ties to the lower ``h``; the cloud is finished when no
  hypothesis is valid or the winner counts fewer than ``min_inliers``;
* ``refine_iters`` refits of the kept plane: float64 centroid and covariance of its inliers, the singular vector of the smallest
  singular value, centroid as anchor, rounded to fp32 once, recounted; kept iff finite, inside the axis cone and counting at least
  as many (the device sums in a fixed order and uses a Jacobi SVD: not bit for bit, see tests/test_gpu_plane.py);
* finish: labels, ``planes = (n, d)`` with ``d = -((nx ax + ny ay) + nz az)`` in float64 from the fp32 values, oriented by exact
  negation (``n . axis >= 0``, or ``d >= 0`` without an axis; on an exact zero the first non-zero component of ``n`` positive).

Departures from open3d: a draw with a repeated row is rejected, every hypothesis is scored (no early exit), the tie-break is by
``h``, several planes per call, the angle constraint."""
import numpy as np

from .augment import MASK, splitmix64

MAX_CLOUDS, MAX_HYPOTHESES, MAX_PLANES, MIN_INLIERS, MAX_REFITS = 65535, 1 << 20, 8, 3, 8       # csrc/plane.h


def cloud_key(seed: int, cloud_id: int) -> int:
    return splitmix64((int(seed) ^ (int(cloud_id) << 40)) & MASK)


def draw_rows(seed: int, cloud_id: int, j: int, hyps, n_live: int) -> np.ndarray:
    """[len(hyps), 3] int64 positions in the live list of the hypotheses ``hyps`` of round ``j``.  Depends on (seed, cloud_id, j, h,
    k, n_live) alone."""
    h = np.asarray(hyps, dtype=np.uint64).reshape(-1)
    key = np.uint64(cloud_key(seed, cloud_id) ^ (int(j) << 32))
    out = np.zeros((len(h), 3), np.int64)
    for k in range(3):
        d = splitmix64(key ^ (h << np.uint64(8)) ^ np.uint64(k))
        out[:, k] = ((d >> np.uint64(32)) * np.uint64(max(int(n_live), 0))) >> np.uint64(32)
    return out


def plane_distance(normal, anchor, points) -> np.ndarray:
    """e [..., n] fp32 of points [n, 3] under the planes (normal [..., 3], anchor [..., 3]) in the device's rounding sequence."""
    nrm = np.asarray(normal, np.float32)[..., None, :]
    a = np.asarray(anchor, np.float32)[..., None, :]
    p = np.asarray(points, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        t = nrm * (p - a)
        return (t[..., 0] + t[..., 1]) + t[..., 2]


def inlier_mask(normal, anchor, points, thr) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return np.abs(plane_distance(normal, anchor, points)) < np.float32(thr)


def count_inliers(normal, anchor, points, thr) -> np.ndarray:
    """Inlier counts [...] of the planes over points [n, 3]: exact integers."""
    nrm, a = np.asarray(normal, np.float32), np.asarray(anchor, np.float32)
    if nrm.ndim == 1:
        return np.int64(inlier_mask(nrm, a, points, thr).sum())
    out = np.zeros(len(nrm), np.int64)
    for s in range(0, len(nrm), 256):
        out[s:s + 256] = inlier_mask(nrm[s:s + 256], a[s:s + 256], points, thr).sum(-1)
    return out


def unit_axis(axis):
    """the axis as the engine takes it: 3 fp32 of the float64 unit vector; None -> zeros (no constraint)"""
    if axis is None:
        return np.zeros(3, np.float32)
    a = np.asarray(axis, np.float64).reshape(-1)
    if a.shape != (3,) or not np.isfinite(a).all() or not np.linalg.norm(a) > 0:
        raise ValueError("axis: three finite numbers, not all zero, expected")
    return (a / np.linalg.norm(a)).astype(np.float32)


def cos_min_of(max_angle_deg) -> float:
    return float(np.cos(np.radians(np.float64(max_angle_deg))))


def axis_args(axis, max_angle_deg):
    """(axis [3] fp32, cos_min) as the C entry takes them.  An axis without an angle orients the planes and rejects nothing
    (cos_min = 0); an angle needs an axis and lies in [0, 90]."""
    if max_angle_deg is None:
        return unit_axis(axis), 0.0
    if axis is None:
        raise ValueError("max_angle_deg needs an axis")
    if not 0.0 <= float(max_angle_deg) <= 90.0:
        raise ValueError(f"max_angle_deg in [0, 90] expected, got {max_angle_deg}")
    return unit_axis(axis), cos_min_of(max_angle_deg)


def _axis_ok(n64, axis32, cos_min):
    if not axis32.any():
        return np.ones(n64.shape[:-1], bool)
    ax = axis32.astype(np.float64)
    dot = (n64[..., 0] * ax[0] + n64[..., 1] * ax[1]) + n64[..., 2] * ax[2]
    return np.abs(dot) >= cos_min


def fit_hypotheses(live_pts, rows, axis32, cos_min):
    """live_pts [n_live, 3] fp32, rows [H, 3] -> (cand [H, 6] fp32 = (n, anchor), zeros where rejected; valid [H])."""
    H, n = len(rows), len(live_pts)
    cand = np.zeros((H, 6), np.float32)
    valid = np.zeros(H, bool)
    if n < 3:
        return cand, valid
    ok = (rows[:, 0] != rows[:, 1]) & (rows[:, 0] != rows[:, 2]) & (rows[:, 1] != rows[:, 2])
    a, b, c = (live_pts[rows[:, k]].astype(np.float64) for k in range(3))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        u, v = b - a, c - a
        m = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], -1)
        len2 = (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]
        ok &= (len2 > 0) & np.isfinite(len2)
        nrm = m / np.sqrt(len2)[:, None]
    ok &= np.where(ok, _axis_ok(np.where(ok[:, None], nrm, 0.0), axis32, cos_min), False)
    cand[ok, :3] = nrm[ok].astype(np.float32)
    cand[ok, 3:] = live_pts[rows[ok, 0]]
    return cand, ok


def pick(valid, counts) -> int:
    """arg-max of (count, lower h) over the valid hypotheses, or -1"""
    valid = np.asarray(valid, bool)
    if not valid.any():
        return -1
    c = np.where(valid, np.asarray(counts, np.int64), -1)
    return int(np.argmax(c))                                    # the first maximum: the lower h


def refit(live_pts, cand, thr, axis32, cos_min):
    """one refit of cand [6] over its inliers among live_pts -> (trial [6] fp32, valid)"""
    m = inlier_mask(cand[:3], cand[3:], live_pts, thr)
    q = live_pts[m].astype(np.float64)
    if len(q) < 3:
        return np.zeros(6, np.float32), False
    cen = q.sum(0) / len(q)
    d = q - cen
    cov = d.T @ d
    n64 = np.linalg.svd(cov)[2][2]
    trial = np.concatenate([n64, cen]).astype(np.float32)
    ok = bool(np.isfinite(trial).all() and trial[:3].any() and _axis_ok(n64, axis32, cos_min))
    return trial, ok


def orient(cand, axis32):
    """(plane [4] fp32, anchor [3] fp32) of the kept candidate: d in float64 from the fp32 values, orientation by exact negation"""
    n = cand[:3].astype(np.float64)
    a = cand[3:].astype(np.float64)
    d = -((n[0] * a[0] + n[1] * a[1]) + n[2] * a[2])
    s = (n[0] * float(axis32[0]) + n[1] * float(axis32[1])) + n[2] * float(axis32[2]) if axis32.any() else d
    first = next((x for x in cand[:3] if x != 0), np.float32(0))
    nrm = cand[:3].copy()
    if s < 0 or (s == 0 and first < 0):
        nrm, d = -nrm, -d
    if d == 0:
        d = 0.0
    nrm = np.where(nrm == 0, np.float32(0), nrm)                 # a zero d and a zero component of n are written as +0
    return np.concatenate([nrm, [np.float32(d)]]).astype(np.float32), cand[3:].copy()


def segment_cloud(points, distance_threshold, count=None, hypotheses=1024, max_planes=1, min_inliers=3, axis=None, max_angle_deg=None,
                  refine_iters=1, seed=0, cloud_id=0):
    """One cloud [cap, >= 3] fp32 through the whole rule -> dict(labels, num_planes, planes, anchors, plane_counts, stats)."""
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] < 3 or points.dtype != np.float32:
        raise ValueError("segment_cloud: points [cap, C >= 3] float32 expected")
    thr = np.float32(distance_threshold)
    if not (np.isfinite(thr) and thr > 0) or not 1 <= hypotheses <= MAX_HYPOTHESES or not 1 <= max_planes <= MAX_PLANES or \
            min_inliers < MIN_INLIERS or not 0 <= refine_iters <= MAX_REFITS:
        raise ValueError("segment_cloud: an argument outside the limits of csrc/plane.h")
    axis32, cos_min = axis_args(axis, max_angle_deg)
    cap = len(points)
    n = cap if count is None else min(max(int(count), 0), cap)
    labels = np.full(cap, -1, np.int32)
    planes, anchors = np.zeros((max_planes, 4), np.float32), np.zeros((max_planes, 3), np.float32)
    plane_counts, stats = np.zeros(max_planes, np.int32), np.zeros((max_planes, 4), np.int32)
    num = 0
    p = points[:n, :3]                                           # rows at and past n are never read
    finite = np.isfinite(p).all(1)
    for j in range(max_planes):
        live = np.nonzero(finite & (labels[:n] < 0))[0]
        lp = p[live]
        cand, valid = fit_hypotheses(lp, draw_rows(seed, cloud_id, j, np.arange(hypotheses), len(live)), axis32, cos_min)
        counts = np.zeros(hypotheses, np.int64)
        if valid.any():
            counts[valid] = count_inliers(cand[valid, :3], cand[valid, 3:], lp, thr)
        h = pick(valid, counts)
        if h < 0 or counts[h] < min_inliers:
            break
        cur, cur_cnt, kept = cand[h], int(counts[h]), 0
        for _ in range(refine_iters):
            trial, ok = refit(lp, cur, thr, axis32, cos_min)
            if ok:
                c = int(count_inliers(trial[:3], trial[3:], lp, thr))
                if c >= cur_cnt:
                    cur, cur_cnt, kept = trial, c, kept + 1
        labels[live[inlier_mask(cur[:3], cur[3:], lp, thr)]] = j
        planes[j], anchors[j] = orient(cur, axis32)
        plane_counts[j] = cur_cnt
        stats[j] = (h, int(valid.sum()), int(counts[h]), kept)
        num = j + 1
    return dict(labels=labels, num_planes=np.int32(num), planes=planes, anchors=anchors, plane_counts=plane_counts, stats=stats)


NAMES = ("labels", "num_planes", "planes", "anchors", "plane_counts", "stats")


def segment_plane_host(points, distance_threshold, counts=None, cloud_ids=None, **kw):
    """The batch: points [clouds, cap, >= 3] fp32 -> the six arrays of ``Engine.segment_plane`` in its order.  Cloud ``c`` draws
    with ``cloud_ids[c]`` (None: ``c``)."""
    points = np.asarray(points)
    if points.ndim != 3:
        raise ValueError("segment_plane_host: points [clouds, cap, C >= 3] float32 expected")
    res = [segment_cloud(points[c], distance_threshold, None if counts is None else counts[c],
                         cloud_id=c if cloud_ids is None else int(cloud_ids[c]), **kw) for c in range(len(points))]
    return tuple(np.stack([r[k] for r in res]) for k in NAMES)
