"""Farthest-point sampling: the rule of csrc/fps.hip (dsir_farthest_point_sample, Engine.farthest_point_sample) restated in numpy
float32, line by line.  What the reference does in dataloader/data_base.py:328 (farthest_point_sampler) and network/tools.py:30
(farthest_point_sample), and open3d in farthest_point_down_sample; open3d cannot be imported here, so parity is unpinned and the rule
is the engine's own.  Host code for tests and for reading; the engine never calls it."""
import numpy as np


def farthest_point_sample_host(points, k: int, counts=None, start: int = 0):
    """points [clouds, cap, >= 3] float32, counts [clouds] or None (rows at and past a count are never read), k >= 1, start >= 0 ->
    (index [clouds, k] int32 in selection order, -1 beyond counts_out; counts_out [clouds] int32; min_d2 [clouds, k] float32: the
    dist of each chosen row when it was chosen, +inf for the first, 0 beyond counts_out)."""
    points = np.asarray(points)
    if points.ndim != 3 or points.shape[2] < 3 or points.dtype != np.float32:
        raise ValueError("farthest_point_sample_host: points [clouds, cap, C >= 3] float32 expected")
    clouds, cap = points.shape[:2]
    if k < 1 or k > cap or start < 0:
        raise ValueError("farthest_point_sample_host: k in [1, cap] and start >= 0 expected")
    index = np.full((clouds, k), -1, np.int32)
    min_d2 = np.zeros((clouds, k), np.float32)
    counts_out = np.zeros(clouds, np.int32)
    for c in range(clouds):
        n = cap if counts is None else min(max(int(counts[c]), 0), cap)
        p = points[c, :n, :3]                                       # rows at and past n are never read
        cand = np.isfinite(p).all(1)                                # a row with a non-finite coordinate is never a candidate
        dist = np.full(n, np.inf, np.float32)
        for t in range(k):
            if not cand.any():
                break                                               # no candidate remains: the cloud ends with count_out = t
            if t == 0:
                s = start if start < n and cand[start] else int(np.argmax(cand))      # else the lowest finite row
                chosen = np.float32(np.inf)
            else:
                live = np.nonzero(cand)[0]
                with np.errstate(over="ignore"):
                    d = p[live] - p[index[c, t - 1]]                # fp32, every operation rounded on its own
                    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                dist[live] = np.minimum(dist[live], d2)
                s = int(live[np.argmax(dist[live])])                # the largest dist; argmax returns the first, i.e. the lower index
                chosen = dist[s]
            index[c, t], min_d2[c, t] = s, chosen
            cand[s] = False                                         # a selected row is never selected again
            counts_out[c] = t + 1
    return index, counts_out, min_d2
