"""The ICP search: the host restatement of the nearest-neighbour rule of csrc/icp.hip, and of the per-pair lattice of csrc/icp_grid.hip.

The rule, the same for the brute-force kernel (`search="brute"`) and the cell index (`search="grid"`) -

    d = ref - cur,  d2 = (dx dx + dy dy) + dz dz     float32, every operation rounded on its own
    the neighbour is the reference point with the smallest d2; ties go to the lower original index
    accepted  <=>  d2 <= r2,  r2 = r r in float32     `<=`, not the strict `<` of deepsir_amd/overlap.py
    a query with a non-finite coordinate matches nothing; a non-finite reference point is never a neighbour
    idx = the index or -1, d2 = the distance or 0

`icp_search_host` is that rule in numpy float32, brute force; the GPU tests compare both kernels with it bit for bit.
`icp_move_host` is the move by a pose as icp_apply_kernel rounds it, `icp_stats_host` the fitness and inlier RMSE in the kernels'
summation order.  The lattice (`grid_cell_edge`, `grid_lattice`, `grid_cells`, `grid_key`) restates csrc/icp_grid.h and
csrc/cell_index.h in float64, as the device computes it: tests/test_icp_search_host.py checks on it that every accepted neighbour
lies in the 27 cells around its query.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

_CHUNK = 1 << 22          # distance tests per block of the brute force

GRID_MARGIN = 1.0 + 2.0 ** -10      # kIcpGridMargin
GRID_MIN_EDGE = 2.0 ** -60          # kIcpGridMinEdge
GRID_MAX_CELLS = 2.0 ** 20          # kIcpGridMaxCells
MAXC = (1 << 21) - 1                # largest coordinate a key holds
KEY_NONE = (1 << 64) - 1


def icp_move_host(T: np.ndarray, pts: np.ndarray) -> np.ndarray:
    """icp_apply_kernel (se3_row of csrc/device_utils.h) in numpy: fl(fma(z, T2, fma(y, T1, fl(x T0))) + T3) per row.  The fused
    steps are taken in float64, where the product of two float32 values is exact, and rounded to float32 once each."""
    T = np.asarray(T, np.float32).reshape(3, 4)
    p = np.asarray(pts, np.float32)
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    out = np.empty((len(p), 3), np.float32)
    with np.errstate(all="ignore"):
        for r in range(3):
            t = T[r].astype(np.float64)
            a = (x * t[0]).astype(np.float32)
            a = (y * t[1] + a.astype(np.float64)).astype(np.float32)
            a = (z * t[2] + a.astype(np.float64)).astype(np.float32)
            out[:, r] = a + T[r, 3]
    return out


def icp_search_host(cur: np.ndarray, ref: np.ndarray, radius: float) -> Tuple[np.ndarray, np.ndarray]:
    """The rule for one pair: cur [J, >=3] (already moved), ref [K, >=3] float32 -> (idx int32 [J], d2 float32 [J])."""
    a = np.asarray(cur, np.float32)[:, :3]
    b = np.asarray(ref, np.float32)[:, :3]
    n, m = a.shape[0], b.shape[0]
    idx = np.full(n, -1, np.int32)
    dist = np.zeros(n, np.float32)
    if n == 0 or m == 0:
        return idx, dist
    r = np.float32(radius)
    with np.errstate(all="ignore"):
        r2 = np.float32(r * r)
        bad_b = ~np.isfinite(b).all(1)
        ok_a = np.isfinite(a).all(1)
        step = max(1, _CHUNK // m)
        for s in range(0, n, step):
            q = a[s:s + step]
            dx = b[None, :, 0] - q[:, None, 0]
            dy = b[None, :, 1] - q[:, None, 1]
            dz = b[None, :, 2] - q[:, None, 2]
            d2 = ((dx * dx + dy * dy) + dz * dz).astype(np.float32)
            d2[:, bad_b] = np.inf
            d2[~np.isfinite(d2)] = np.inf              # a non-finite query row, an overflow: never smaller than anything
            k = np.argmin(d2, 1)                       # the first minimum: the lower index on a tie
            best = d2[np.arange(len(q)), k]
            hit = (best <= r2) & np.isfinite(best) & ok_a[s:s + step]
            idx[s:s + step] = np.where(hit, k, -1).astype(np.int32)
            dist[s:s + step] = np.where(hit, best, np.float32(0))
    return idx, dist


def icp_stats_host(idx: np.ndarray, d2: np.ndarray) -> np.ndarray:
    """{fitness, inlier RMSE} of one pair's search in the summation order of icp_stats_kernel: thread t of 256 adds rows
    t, t + 256, ..., the wave butterfly (xor 32, 16, .. 1), then the four waves in order -> float64 [2]."""
    idx = np.asarray(idx)
    J = len(idx)
    inl = idx >= 0
    pad = (-J) % 256
    cnt = np.concatenate([inl.astype(np.float64), np.zeros(pad)]).reshape(-1, 256)
    sse = np.concatenate([np.where(inl, np.asarray(d2, np.float32).astype(np.float64), 0.0), np.zeros(pad)]).reshape(-1, 256)

    def total(v):
        t = np.zeros(256)
        for row in v:                                   # in row order, as the thread's loop adds
            t = t + row
        t = t.reshape(4, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            t = t + t[:, lane ^ o]
        return ((t[0, 0] + t[1, 0]) + t[2, 0]) + t[3, 0]

    c, s = total(cnt), total(sse)
    return np.array([c / float(J), np.sqrt(s / c) if c > 0 else 0.0], np.float64)


def icp_correspondences_host(src: np.ndarray, ref: np.ndarray, T: np.ndarray, radius: float):
    """`Engine.icp_correspondences` on the host for one pair -> (idx [J], d2 [J], stats [2])."""
    idx, d2 = icp_search_host(icp_move_host(T, np.asarray(src, np.float32)[:, :3]), ref, radius)
    return idx, d2, icp_stats_host(idx, d2)


# ---------------------------------------------------------------------- the lattice of csrc/icp_grid.h
def grid_cell_edge(radius: float, extent: float) -> float:
    """h = max(r (1 + 2^-10), 2^-60, longest axis extent / 2^20) in float64, r the float32 radius"""
    h = float(np.float32(radius)) * GRID_MARGIN
    if not h >= GRID_MIN_EDGE:
        h = GRID_MIN_EDGE
    return max(h, float(extent) / GRID_MAX_CELLS)


def grid_lattice(ref: np.ndarray, radius: float) -> Tuple[np.ndarray, float]:
    """(origin float64 [3], h) of one pair: the minimum of the finite reference points, the edge from their longest axis"""
    b = np.asarray(ref, np.float32)[:, :3]
    b = b[np.isfinite(b).all(1)].astype(np.float64)
    if not len(b):
        return np.zeros(3), grid_cell_edge(radius, 0.0)
    lo = b.min(0)
    return lo, grid_cell_edge(radius, float((b.max(0) - lo).max()))


def grid_cells(pts: np.ndarray, origin: np.ndarray, h: float) -> np.ndarray:
    """cell_of per coordinate: floor((a - o) / h) in float64, clamped to [-2, MAXC + 2] -> int64 [n, 3] (finite rows only)"""
    with np.errstate(all="ignore"):
        u = np.floor((np.asarray(pts, np.float32)[:, :3].astype(np.float64) - origin) / h)
    return np.clip(u, -2.0, float(MAXC + 2)).astype(np.int64)


def grid_key(cells: np.ndarray) -> np.ndarray:
    """cell_key of reference cells (clamped to [0, MAXC] as the key kernel does): x | y << 21 | z << 42 -> uint64 [n]"""
    c = np.clip(np.asarray(cells, np.int64), 0, MAXC).astype(np.uint64)
    return c[:, 0] | (c[:, 1] << np.uint64(21)) | (c[:, 2] << np.uint64(42))
