#!/usr/bin/env python
"""Fragment overlap: the grid search (csrc/overlap.hip, ``Engine.nn_index`` + ``search`` in count mode) timed against the only
other way this engine can produce the same number - ``Engine.radius_matches`` under the identity pose, brute force: a row is
overlapped iff its list is not empty.

Two cases: `scene`, one synthetic scene of 40 fragments x 16384 points cut from one surface (windows of a jittered 0.03 m grid,
so that most pairs do not touch and the rest overlap in part), all 780 pairs i < j; `pair`, one pair of 16384 x 16384.  Device
events around whole calls, warm-up first, the two sides alternating, the median of --repeats; the counts of the two sides are
compared before anything is timed.  Prints one JSON line per case: both times, the ratio, and the index build's share of the grid
side.  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

R = 0.03


def fragment(rng, cx, cy, side=128):
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2) * R
    xy = g + [cx, cy] + rng.random(2) * R + rng.uniform(-0.4 * R, 0.4 * R, g.shape)
    z = 0.3 * np.sin(1.3 * xy[:, 0]) * np.cos(0.9 * xy[:, 1]) + rng.normal(0.0, 0.002, len(xy))
    return np.concatenate([xy, z[:, None]], 1).astype(np.float32)[rng.permutation(len(xy))]


def scene(n_frag, seed):
    """Windows of 3.84 m on a 14 x 9 m sheet: a pair's windows are disjoint more often than not."""
    rng = np.random.default_rng(seed)
    return [fragment(rng, rng.random() * 10.0, rng.random() * 5.0) for _ in range(n_frag)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def run_case(eng, name, frags, jobs, repeats, warmup):
    n = len(frags[0])
    pts = torch.from_numpy(np.concatenate(frags)).cuda()
    off = np.arange(len(frags) + 1, dtype=np.int64) * n
    host = np.concatenate(frags)
    bounds = np.concatenate([host.min(0), host.max(0)])
    per_call = max(1, (2 ** 31 - 1) // (n * n))                      # radius_matches takes pairs J K <= 2^31 - 1 per call
    store = pts.reshape(len(frags), n, 3)
    batches = []
    for s in range(0, len(jobs), per_call):
        jb = torch.from_numpy(jobs[s:s + per_call].astype(np.int64)).cuda()
        batches.append((store[jb[:, 0]].contiguous(), store[jb[:, 1]].contiguous(), torch.eye(4, device="cuda")[:3].repeat(len(jb), 1, 1).contiguous()))

    def grid_build():
        return eng.nn_index(pts, off, R, bounds)

    def grid_all():
        return grid_build().search(jobs)[0]

    def brute():
        out = []
        for src, ref, eye in batches:
            o, _ = eng.radius_matches(src, ref, eye, R)
            rows = (o[1:] - o[:-1]).reshape(src.shape[0], n)
            out.append((rows > 0).sum(1))
        return torch.cat(out)

    want, got = brute().cpu().numpy(), grid_all().cpu().numpy()
    if not np.array_equal(want, got):
        raise SystemExit(f"{name}: the two sides disagree on {int((want != got).sum())} of {len(jobs)} jobs")
    for _ in range(warmup):
        grid_all(); brute(); grid_build()
    torch.cuda.synchronize()
    t_grid, t_brute, t_build = [], [], []
    for _ in range(repeats):
        t_grid.append(timed(grid_all)[0])
        t_brute.append(timed(brute)[0])
        t_build.append(timed(grid_build)[0])
    g, b, d = float(np.median(t_grid)), float(np.median(t_brute)), float(np.median(t_build))
    res = {"case": name, "fragments": len(frags), "points": n, "jobs": len(jobs), "touching_jobs": int((got > 0).sum()),
           "mean_ratio_of_touching": float((got[got > 0] / n).mean()) if (got > 0).any() else 0.0,
           "grid_ms": round(g, 3), "grid_ms_min_max": [round(min(t_grid), 3), round(max(t_grid), 3)],
           "brute_ms": round(b, 3), "brute_ms_min_max": [round(min(t_brute), 3), round(max(t_brute), 3)],
           "brute_over_grid": round(b / g, 2), "index_build_ms": round(d, 3), "index_build_share": round(d / g, 3)}
    print(json.dumps(res), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fragments", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_overlap: needs a GPU (a CPU run measures nothing)")
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    eng = Engine(NetConfig(), 0)
    frags = scene(a.fragments, a.seed)
    jobs = np.array([(i, j) for i in range(len(frags)) for j in range(i + 1, len(frags))], np.int32)
    run_case(eng, "scene", frags, jobs, a.repeats, a.warmup)
    rng = np.random.default_rng(a.seed + 1)
    run_case(eng, "pair", [fragment(rng, 0.0, 0.0), fragment(rng, 1.5, 0.7)], np.array([(0, 1)], np.int32), a.repeats * 3, a.warmup)
    eng.close()


if __name__ == "__main__":
    main()
