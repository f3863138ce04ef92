"""Fragment overlap: the host restatement of the radius-bounded nearest-neighbour rule, and the 3DMatch train-table logic.

The reference makes `3DMatch_{split}_{voxel}_points.pkl`, `_overlap.pkl` and `_keypts.pkl` offline with
dataloader/3DMatch_preprocess.py (open3d for the PLY reader and the voxel grid, cv2.BFMatcher for the nearest neighbours).  Neither
library is installable here: parity is unpinned and the engine owns the rule (csrc/overlap.hip, `Engine.nn_within`) -

    d2 = (dx dx + dy dy) + dz dz,  d = b - a     float32, every operation rounded on its own
    the neighbour of a is the b with the smallest d2; ties go to the lower original index of b
    match  <=>  d2 < r r                          strict; r r one float32 product
    a query with a non-finite coordinate matches nothing; a non-finite b is never a neighbour; an empty a or b gives count 0
    with a pose T [3, 4] per job the query is moved first: c_r = ((T[r,0] x + T[r,1] y) + T[r,2] z) + T[r,3], in float32

`nn_within_host` is that rule in numpy float32, brute force; the GPU tests compare the kernels with it bit for bit.  The table logic
(`write_3dmatch_tables`) takes the point loader and the search as callables, so that it runs without a device;
`deepsir_amd.data.preprocess_3dmatch` plugs the engine in.
"""
from __future__ import annotations

import os
import pickle
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

_CHUNK = 1 << 22          # distance tests per block of the brute force


def move_host(T: np.ndarray, pts: np.ndarray) -> np.ndarray:
    """match_move of csrc/match_targets.hip in numpy float32: ((T0 x + T1 y) + T2 z) + T3 per row, no fused multiply-add."""
    T = np.asarray(T, np.float32).reshape(3, 4)
    p = np.asarray(pts, np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1).astype(np.float32)


def nn_pair_host(a: np.ndarray, b: np.ndarray, radius: float) -> np.ndarray:
    """The rule for one pair: a [n, >=3], b [m, >=3] float32 -> int32 [n]: the original index in b of a's neighbour, or -1."""
    a = np.asarray(a, np.float32)[:, :3]
    b = np.asarray(b, np.float32)[:, :3]
    n, m = a.shape[0], b.shape[0]
    out = np.full(n, -1, np.int32)
    if n == 0 or m == 0:
        return out
    r = np.float32(radius)
    r2 = np.float32(r * r)
    bad_b = ~np.isfinite(b).all(1)
    ok_a = np.isfinite(a).all(1)
    step = max(1, _CHUNK // m)
    with np.errstate(all="ignore"):
        for s in range(0, n, step):
            q = a[s:s + step]
            dx = b[None, :, 0] - q[:, None, 0]
            dy = b[None, :, 1] - q[:, None, 1]
            dz = b[None, :, 2] - q[:, None, 2]
            d2 = ((dx * dx + dy * dy) + dz * dz).astype(np.float32)
            d2[:, bad_b] = np.inf
            d2[~np.isfinite(d2)] = np.inf              # a non-finite query row: every distance is NaN or inf
            k = np.argmin(d2, 1)                       # the first minimum: the lower index on a tie
            hit = (d2[np.arange(len(q)), k] < r2) & ok_a[s:s + step]
            out[s:s + step] = np.where(hit, k, -1).astype(np.int32)
    return out


def nn_within_host(points: np.ndarray, offsets: Sequence[int], jobs: Sequence[Sequence[int]], radius: float,
                   poses: Optional[np.ndarray] = None) -> Tuple[np.ndarray, List[np.ndarray]]:
    """`Engine.nn_within` on the host: points [total, >=3] float32 holding ragged fragments (offsets [F + 1]), jobs [n, 2] of
    (query fragment, target fragment), poses None or [n, 3, 4] -> (counts int32 [n], per job the int32 [n_query] neighbour list)."""
    pts = np.asarray(points, np.float32)
    off = np.asarray(offsets, np.int64)
    jobs = np.asarray(jobs, np.int64).reshape(-1, 2)
    counts = np.zeros(len(jobs), np.int32)
    nn = []
    for j, (q, t) in enumerate(jobs):
        a = pts[off[q]:off[q + 1], :3]
        if poses is not None:
            a = move_host(np.asarray(poses)[j], a)
        k = nn_pair_host(a, pts[off[t]:off[t + 1], :3], radius)
        counts[j] = int((k >= 0).sum())
        nn.append(k)
    return counts, nn


def radius_pair_host(a: np.ndarray, b: np.ndarray, radius: float, max_nn: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The neighbour-list rule for one pair (csrc/radius_nn.hip): a [n, >=3], b [m, >=3] float32 -> (counts int32 [n], cols int32
    [sum], d2 float32 [sum]): per row of a every b with d2 < r r, or with ``max_nn`` > 0 the max_nn smallest under (d2, index), each
    row in ascending index."""
    a = np.asarray(a, np.float32)[:, :3]
    b = np.asarray(b, np.float32)[:, :3]
    n, m = a.shape[0], b.shape[0]
    counts = np.zeros(n, np.int32)
    cols: List[np.ndarray] = []
    dist: List[np.ndarray] = []
    if n and m:
        r = np.float32(radius)
        r2 = np.float32(r * r)
        bad_b = ~np.isfinite(b).all(1)
        ok_a = np.isfinite(a).all(1)
        step = max(1, _CHUNK // m)
        with np.errstate(all="ignore"):
            for s in range(0, n, step):
                q = a[s:s + step]
                dx = b[None, :, 0] - q[:, None, 0]
                dy = b[None, :, 1] - q[:, None, 1]
                dz = b[None, :, 2] - q[:, None, 2]
                d2 = ((dx * dx + dy * dy) + dz * dz).astype(np.float32)
                hit = (d2 < r2) & ~bad_b[None, :] & ok_a[s:s + step, None]
                for i in range(len(q)):
                    k = np.nonzero(hit[i])[0]                       # ascending index
                    if max_nn > 0 and len(k) > max_nn:
                        k = np.sort(k[np.lexsort((k, d2[i, k]))[:max_nn]])     # (d2, index) ascending, the first max_nn, back in index order
                    counts[s + i] = len(k)
                    cols.append(k.astype(np.int32))
                    dist.append(d2[i, k])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return counts, cat(cols, np.int32), cat(dist, np.float32)


def radius_neighbors_host(points: np.ndarray, offsets: Sequence[int], jobs: Sequence[Sequence[int]], radius: float,
                          poses: Optional[np.ndarray] = None, max_nn: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``NNIndex.neighbors`` on the host, selection included: points [total, >=3] float32 holding ragged fragments (offsets [F + 1]),
    jobs [n, 2] of (query fragment, target fragment), poses None or [n, 3, 4] (applied in float32 before the search) ->
    (offsets int32 [rows + 1], cols int32 [total], d2 float32 [total]) over the jobs' query rows in job order."""
    pts = np.asarray(points, np.float32)
    off = np.asarray(offsets, np.int64)
    jobs = np.asarray(jobs, np.int64).reshape(-1, 2)
    counts, cols, dist = [np.zeros(0, np.int32)], [np.zeros(0, np.int32)], [np.zeros(0, np.float32)]
    for j, (q, t) in enumerate(jobs):
        a = pts[off[q]:off[q + 1], :3]
        if poses is not None:
            a = move_host(np.asarray(poses)[j], a)
        c, k, d = radius_pair_host(a, pts[off[t]:off[t + 1], :3], radius, int(max_nn))
        counts.append(c); cols.append(k); dist.append(d)
    row_off = np.concatenate([[0], np.cumsum(np.concatenate(counts), dtype=np.int64)]).astype(np.int32)
    return row_off, np.concatenate(cols), np.concatenate(dist)


def keypoint_pairs(nn: np.ndarray) -> np.ndarray:
    """A job's neighbour list as the reference's key-point pairs (3DMatch_preprocess.py:82-89): int32 [m, 2] of (query, target) in
    ascending query index."""
    nn = np.asarray(nn)
    q = np.nonzero(nn >= 0)[0]
    return np.stack([q, nn[q]], 1).astype(np.int32).reshape(-1, 2)


def fragment_sort_key(frag_id: str) -> int:
    """3DMatch_preprocess.py:44: the integer after the last '_'."""
    return int(frag_id.split("_")[-1])


def table_paths(savepath: str, split: str, downsample: float) -> Tuple[str, str, str]:
    stem = os.path.join(savepath, f"3DMatch_{split}_{downsample:.3f}")
    return stem + "_points.pkl", stem + "_overlap.pkl", stem + "_keypts.pkl"


# search(fragments: list of float32 [n_i, 3], jobs: int [n, 2], radius, fill: bool) -> (counts [n], list of nn [n_query] or None)
Search = Callable[[List[np.ndarray], np.ndarray, float, bool], Tuple[np.ndarray, Optional[List[np.ndarray]]]]


def host_search(fragments: List[np.ndarray], jobs: np.ndarray, radius: float, fill: bool):
    """The `Search` of `nn_within_host` (slow: for tests and tiny trees)."""
    off = np.concatenate([[0], np.cumsum([len(f) for f in fragments])])
    pts = np.concatenate([np.asarray(f, np.float32).reshape(-1, 3) for f in fragments]) if fragments else np.zeros((0, 3), np.float32)
    counts, nn = nn_within_host(pts, off, jobs, radius)
    return counts, (nn if fill else None)


def scene_tables(ids: Sequence[str], points: Dict[str, np.ndarray], search: Search, downsample: float, overlap_thres: float,
                 overlap: Dict[str, float], keypts: Dict[str, np.ndarray]) -> None:
    """cal_overlap for one scene (3DMatch_preprocess.py:107-131): every pair i < j in id order through `search` in count mode, then
    fill mode for the pairs whose count / len(src) exceeds the threshold; those alone enter `overlap` and `keypts`, in (i, j) order."""
    frags = [np.ascontiguousarray(points[i], dtype=np.float32) for i in ids]
    jobs = np.array([(i, j) for i in range(len(ids)) for j in range(i + 1, len(ids))], np.int32).reshape(-1, 2)
    if not len(jobs):
        return
    counts, _ = search(frags, jobs, downsample, False)
    ratios = [(int(c) / len(frags[q]) if len(frags[q]) else 0.0) for c, (q, _t) in zip(counts, jobs)]
    keep = [k for k, r in enumerate(ratios) if r > overlap_thres]
    if not keep:
        return
    _, nn = search(frags, jobs[keep], downsample, True)
    for k, lst in zip(keep, nn):
        key = f"{ids[jobs[k][0]]}@{ids[jobs[k][1]]}"
        keypts[key] = keypoint_pairs(lst)
        overlap[key] = ratios[k]


def write_3dmatch_tables(savepath: str, split: str, downsample: float, scene_to_ids: Dict[str, List[str]],
                         load_points: Callable[[List[str]], Dict[str, np.ndarray]], search: Search, overlap_thres: float = 0.30):
    """The three tables of 3DMatch_preprocess.py under `savepath`; an existing points file, and an existing overlap + keypts pair,
    are reloaded instead of recomputed (:65-69, :95-104).  -> (points, overlap, keypts)."""
    os.makedirs(savepath, exist_ok=True)
    pts_fn, ovl_fn, key_fn = table_paths(savepath, split, downsample)
    if os.path.exists(pts_fn):
        with open(pts_fn, "rb") as f:
            points = pickle.load(f)
    else:
        points = load_points([i for ids in scene_to_ids.values() for i in ids])
        with open(pts_fn, "wb") as f:
            pickle.dump(points, f)
    if os.path.exists(ovl_fn) and os.path.exists(key_fn):
        with open(ovl_fn, "rb") as f:
            overlap = pickle.load(f)
        with open(key_fn, "rb") as f:
            keypts = pickle.load(f)
        return points, overlap, keypts
    overlap: Dict[str, float] = {}
    keypts: Dict[str, np.ndarray] = {}
    for ids in scene_to_ids.values():
        scene_tables(ids, points, search, float(downsample), float(overlap_thres), overlap, keypts)
    with open(ovl_fn, "wb") as f:
        pickle.dump(overlap, f)
    with open(key_fn, "wb") as f:
        pickle.dump(keypts, f)
    return points, overlap, keypts
