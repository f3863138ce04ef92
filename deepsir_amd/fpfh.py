"""Host restatement of the FPFH rule of ``csrc/fpfh.hip`` (include/dsir.h, dsir_fpfh) in numpy.

The classical descriptor of the feature-matching baseline (open3d ``compute_fpfh_feature``, PCL ``FPFHEstimation``; Rusu et al.,
ICRA 2009).  open3d cannot be imported here, so parity is unpinned and the engine owns the rule; the header of csrc/fpfh.hip states
it, this module states it a second time, the way ``ransac.py`` and ``ppf.py`` do for their rules: the tests compare the device
against it, the product path never calls it.

All arithmetic is float64 on the fp32 inputs, every operation rounded once (numpy neither contracts nor reorders element-wise
expressions), so ``arctan2`` is the one operation whose last bit may differ from the device's.  It can move a count only where
``11 (f1 + pi) / (2 pi)`` sits on an integer: ``band`` marks the points that have such a pair, or a neighbour with one.

    dot(a, b)   = (a0 b0 + a1 b1) + a2 b2
    cross(a, b) = (a1 b2 - a2 b1,  a2 b0 - a0 b2,  a0 b1 - a1 b0)
    pair (i, j), j in the list of i, indices clamped into the cloud:
      d = p_j - p_i;  L2 = dot(d, d);  L = sqrt(L2)
      skipped: j == i, not (L2 > 0), a non-finite coordinate, a zero or non-finite normal
      a1 = dot(n_i, d) / L;  a2 = dot(n_j, d) / L
      |a1| < |a2|:  s = n_j, t = n_i, d = -d, f3 = -a2      else:  s = n_i, t = n_j, f3 = a1
      v = cross(d, s);  |v| = sqrt(dot(v, v));  skipped when |v| == 0;  v = v / |v|  (three divisions)
      w = cross(s, v);  f2 = dot(v, t);  f1 = atan2(dot(w, t), dot(s, t))
      b1 = clamp(floor((11 (f1 + pi)) / (2 pi)), 0, 10);  b2 = 11 + clamp(floor((11 (f2 + 1)) / 2), 0, 10);  b3 = 22 + the same of f3
    SPFH(i): integer counts of b1, b2, b3 over the pairs of i that were not skipped, and their number valid(i);
             as a value, bin = (100 count) / valid(i), all zero when valid(i) == 0
    FPFH(i): acc = 0; for j in list order with L2 > 0:  acc[b] = acc[b] + SPFH_value(j)[b] / L2
             per block of 11 bins: sum = ((acc[0] + acc[1]) + ...) ascending; sum > 0: acc[b] = acc[b] * (100 / sum)
             row[b] = fp32(acc[b] + SPFH_value(i)[b]);  zeros up to out_ld;  flags[i] = 1 and the row all zeros when valid(i) == 0
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

BINS = 11
DIM = 3 * BINS                    # 33 values per row
SPFH_LD = DIM + 1                 # the device's table row: 33 counts and valid(i)
PI = float(np.pi)
TWO_PI = 2.0 * PI
BAND_EPS = 1e-9


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _bin(x):
    return np.clip(np.floor(x), 0, BINS - 1).astype(np.int64)


def knn_lists(points: np.ndarray, k: int = 16) -> np.ndarray:
    """Brute-force k nearest neighbours of one cloud [n, >= 3] (self first, ties to the lower index) as int32 [n, k]; a cloud of fewer
    than k points pads its lists with self."""
    p = np.asarray(points, np.float32)[:, :3].astype(np.float64)
    n = p.shape[0]
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    d2[np.arange(n), np.arange(n)] = -1.0
    order = np.argsort(d2, axis=1, kind="stable")[:, :k].astype(np.int32)
    if n < k:
        order = np.concatenate([order, np.repeat(np.arange(n, dtype=np.int32)[:, None], k - n, 1)], 1)
    return order


def _edges(neigh, csr, c: int, n: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(start [c n], deg [c n], cols [E]) of either list form; cols are cloud-local."""
    if (neigh is None) == (csr is None):
        raise ValueError("fpfh: exactly one of neigh and csr")
    if neigh is not None:
        nb = np.asarray(neigh)
        if nb.shape != (c, n, 16):
            raise ValueError(f"fpfh: neigh must be [{c}, {n}, 16]")
        return np.arange(c * n, dtype=np.int64) * 16, np.full(c * n, 16, np.int64), nb.reshape(-1).astype(np.int64)
    off, cols = np.asarray(csr[0], np.int64), np.asarray(csr[1], np.int64)
    if off.shape != (c * n + 1,):
        raise ValueError(f"fpfh: csr offsets must be [{c * n + 1}]")
    return off[:-1], np.maximum(off[1:] - off[:-1], 0), cols


def fpfh_host(points: np.ndarray, normals: Optional[np.ndarray] = None, neigh: Optional[np.ndarray] = None, csr=None,
              out_ld: int = 64) -> Dict[str, np.ndarray]:
    """points [c, n, >= 3] fp32 (normals in columns 3..5 when ``normals`` is None), normals [c, n, 3] fp32, and exactly one of
    neigh [c, n, 16] and csr = (offsets [c n + 1], cols) with cloud-local columns.  Returns dict(desc [c, n, out_ld] fp32, flags [c, n]
    i32, band [c, n] bool, counts [c, n, 33] i32, valid [c, n] i32, desc64 [c, n, 33]: the row before its rounding to fp32)."""
    pts = np.asarray(points, np.float32)
    c, n = pts.shape[:2]
    if normals is None:
        if pts.shape[2] < 6:
            raise ValueError("fpfh: rows without normals need at least 6 columns")
        nrm = pts[:, :, 3:6]
    else:
        nrm = np.asarray(normals, np.float32)
    if out_ld < DIM:
        raise ValueError("fpfh: out_ld >= 33")
    P = pts[:, :, :3].astype(np.float64).reshape(c * n, 3)
    N = nrm.astype(np.float64).reshape(c * n, 3)
    start, deg, cols = _edges(neigh, csr, c, n)
    E = int(deg.sum())
    rows = np.repeat(np.arange(c * n, dtype=np.int64), deg)                       # global row of every list entry ...
    pos = np.arange(E, dtype=np.int64) - np.repeat(np.cumsum(deg) - deg, deg) + np.repeat(start, deg)
    gj = (rows // n) * n + np.clip(cols[pos], 0, n - 1)                           # ... and the global row of its neighbour
    with np.errstate(all="ignore"):
        d = P[gj] - P[rows]
        L2 = _dot(d, d)
        L = np.sqrt(L2)
        ni, nj = N[rows], N[gj]
        ok_n = np.isfinite(N).all(1) & (N != 0.0).any(1)
        ok = (gj != rows) & (L2 > 0.0) & np.isfinite(P[rows]).all(1) & np.isfinite(P[gj]).all(1) & ok_n[rows] & ok_n[gj]
        a1 = _dot(ni, d) / L
        a2 = _dot(nj, d) / L
        swap = np.abs(a1) < np.abs(a2)
        s = np.where(swap[:, None], nj, ni)
        t = np.where(swap[:, None], ni, nj)
        d = np.where(swap[:, None], -d, d)
        f3 = np.where(swap, -a2, a1)
        v = _cross(d, s)
        vn = np.sqrt(_dot(v, v))
        ok &= vn > 0.0
        v = v / vn[:, None]
        w = _cross(s, v)
        f2 = _dot(v, t)
        f1 = np.arctan2(_dot(w, t), _dot(s, t))
        x1 = (11.0 * (f1 + PI)) / TWO_PI
        b1 = _bin(np.where(ok, x1, 0.0))
        b2 = BINS + _bin(np.where(ok, (11.0 * (f2 + 1.0)) / 2.0, 0.0))
        b3 = 2 * BINS + _bin(np.where(ok, (11.0 * (f3 + 1.0)) / 2.0, 0.0))
        edge_band = ok & (np.abs(x1 - np.round(x1)) < BAND_EPS)
    counts = np.zeros((c * n, DIM), np.int64)
    for b in (b1, b2, b3):
        np.add.at(counts, (rows[ok], b[ok]), 1)
    valid = np.bincount(rows[ok], minlength=c * n).astype(np.int64)
    own_band = np.bincount(rows[edge_band], minlength=c * n) > 0
    with np.errstate(all="ignore"):
        value = np.where(valid[:, None] > 0, (100.0 * counts) / np.maximum(valid, 1)[:, None], 0.0)
    # the weighted sum, in list order: trip k adds the k-th entry of every list that has one
    acc = np.zeros((c * n, DIM))
    band = own_band.copy()
    base = np.cumsum(deg) - deg
    with np.errstate(all="ignore"):
        for k in range(int(deg.max()) if deg.size else 0):
            r = np.nonzero(deg > k)[0]
            e = base[r] + k
            band[r] |= own_band[gj[e]]
            use = L2[e] > 0.0
            r, e = r[use], e[use]
            acc[r] = acc[r] + value[gj[e]] / L2[e][:, None]
        for blk in range(3):
            a = acc[:, blk * BINS:(blk + 1) * BINS]
            sm = np.zeros(c * n)
            for b in range(BINS):
                sm = sm + a[:, b]
            pos_sum = sm > 0.0
            a[pos_sum] = a[pos_sum] * (100.0 / sm[pos_sum])[:, None]
        desc64 = acc + value
    flags = (valid == 0).astype(np.int32)
    desc64[valid == 0] = 0.0
    desc = np.zeros((c * n, out_ld), np.float32)
    desc[:, :DIM] = desc64.astype(np.float32)
    return {"desc": desc.reshape(c, n, out_ld), "flags": flags.reshape(c, n), "band": band.reshape(c, n),
            "counts": counts.astype(np.int32).reshape(c, n, DIM), "valid": valid.astype(np.int32).reshape(c, n),
            "desc64": desc64.reshape(c, n, DIM)}


def spfh_values(counts: np.ndarray, valid: np.ndarray) -> np.ndarray:
    """The SPFH of ``fpfh_host``'s counts as values: (100 count) / valid, zero where valid == 0."""
    valid = np.asarray(valid, np.int64)[..., None]
    return np.where(valid > 0, (100.0 * np.asarray(counts, np.int64)) / np.maximum(valid, 1), 0.0)


# ---------------------------------------------------------------------------------------------------------------- test problems
def _height(x, y):
    """A sum of a few sines with incommensurate wave numbers: no two patches of the surface are congruent."""
    return (0.11 * np.sin(2.3 * x + 0.4) + 0.09 * np.sin(3.1 * y + 1.1) + 0.07 * np.sin(1.7 * x + 2.9 * y + 0.3) +
            0.05 * np.sin(4.3 * x - 3.7 * y + 2.0) + 0.04 * np.sin(5.9 * y - 1.3 * x + 0.7))


def _height_normal(x, y):
    gx = (0.11 * 2.3 * np.cos(2.3 * x + 0.4) + 0.07 * 1.7 * np.cos(1.7 * x + 2.9 * y + 0.3) + 0.05 * 4.3 * np.cos(4.3 * x - 3.7 * y + 2.0) -
          0.04 * 1.3 * np.cos(5.9 * y - 1.3 * x + 0.7))
    gy = (0.09 * 3.1 * np.cos(3.1 * y + 1.1) + 0.07 * 2.9 * np.cos(1.7 * x + 2.9 * y + 0.3) - 0.05 * 3.7 * np.cos(4.3 * x - 3.7 * y + 2.0) +
          0.04 * 5.9 * np.cos(5.9 * y - 1.3 * x + 0.7))
    nv = np.stack([-gx, -gy, np.ones_like(gx)], -1)
    return nv / np.linalg.norm(nv, axis=-1, keepdims=True)


def jittered_surface(n: int, seed: int, extent: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray]:
    """n points on the bumpy height field over [0, extent]^2 (default: the extent that keeps the density of 1024 points on [0, 3]^2):
    a jittered lattice (cells of a ceil(sqrt(n)) grid, a random n of them, +-0.4 of a cell), rows shuffled, and the analytic upward
    normals with a small seeded tilt.  -> (points [n, 3], normals [n, 3]) fp32."""
    rng = np.random.Generator(np.random.Philox(key=int(seed)))
    side = int(np.ceil(np.sqrt(n)))
    extent = 3.0 * np.sqrt(n / 1024.0) if extent is None else float(extent)
    cells = rng.permutation(side * side)[:n]
    h = extent / side
    x = ((cells % side) + 0.5 + rng.uniform(-0.4, 0.4, n)) * h
    y = ((cells // side) + 0.5 + rng.uniform(-0.4, 0.4, n)) * h
    pts = np.stack([x, y, _height(x, y)], 1)
    nv = _height_normal(x, y) + rng.normal(scale=0.01, size=(n, 3))
    nv = nv / np.linalg.norm(nv, axis=1, keepdims=True)
    return pts.astype(np.float32), nv.astype(np.float32)


def random_pose(rng, max_angle: float = 1.0, max_shift: float = 2.0) -> np.ndarray:
    """A random rigid motion [3, 4] float64: rotation of 0.3 .. max_angle rad about a random axis, translation up to max_shift."""
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(0.3, max_angle)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    return np.concatenate([R, rng.uniform(-max_shift, max_shift, (3, 1))], 1)


def bumpy_pair(seed: int, n: int = 1024) -> Dict[str, np.ndarray]:
    """The registration pair of the FPFH tests, in the harness's pair layout: ``points_ref`` [1, n, 3] = n points on the bumpy height
    field over [0, 3]^2, ``points_src`` the same points moved by a random pose and row-permuted, ``transform_gt`` [1, 3, 4] the pose
    that takes src back onto ref, ``viewpoint_ref`` [1, 3] above the surface and ``viewpoint_src`` the same point moved with src;
    ``perm`` [n]: src row r is ref row perm[r]."""
    rng = np.random.Generator(np.random.Philox(key=int(seed) + 7919))
    ref, _ = jittered_surface(n, seed, 3.0)
    M = random_pose(rng)
    perm = rng.permutation(n)
    src = (ref[perm].astype(np.float64) @ M[:, :3].T + M[:, 3]).astype(np.float32)
    v_ref = np.array([1.5, 1.5, 10.0])
    v_src = M[:, :3] @ v_ref + M[:, 3]
    gt = np.concatenate([M[:, :3].T, -(M[:, :3].T @ M[:, 3])[:, None]], 1)
    return {"points_src": src[None], "points_ref": ref[None], "transform_gt": gt[None].astype(np.float32),
            "viewpoint_src": v_src[None].astype(np.float32), "viewpoint_ref": v_ref[None].astype(np.float32), "perm": perm}


def host_chain(pair: Dict[str, np.ndarray], voxel_size: float, hypotheses: int, seed: int = 0, p: int = 0, lists=None, normals=None):
    """The host restatement of ``harness.register_fpfh`` for one pair: 16-NN lists (``lists`` = (src, ref) replaces the brute-force
    ones), ``ppf.estimate_normals`` (or ``normals`` = (src, ref)), ``fpfh_host``, the float64 arg-min with the mutual check, the
    RANSAC rule of ``ransac.py``.  -> dict(T [3, 4], corr [count, 2], src / ref: the two ``fpfh_host`` results)."""
    from . import ppf, ransac
    out = {}
    for k, side in enumerate(("src", "ref")):
        pts = pair["points_" + side][0][:, :3]
        nb = knn_lists(pts) if lists is None else np.asarray(lists[k])
        nv = ppf.estimate_normals(pts[None], nb[None], tuple(pair["viewpoint_" + side].reshape(-1)))[0][0] if normals is None else normals[k]
        out[side] = fpfh_host(pts[None], nv[None], neigh=nb[None])
    corr, count = ransac.feature_correspondences(out["src"]["desc"][0], out["ref"]["desc"][0], mutual=True)
    r = ransac.ransac_pair(pair["points_src"][0], pair["points_ref"][0], corr, count, max_dist=2.0 * voxel_size, hypotheses_n=hypotheses,
                           seed=seed, p=p)
    out.update(T=r["T"], corr=corr[:count])
    return out
