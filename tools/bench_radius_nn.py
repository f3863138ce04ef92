#!/usr/bin/env python
"""Radius neighbour lists: the cell-indexed search (csrc/radius_nn.hip, ``Engine.radius_neighbors``) timed against the brute-force
lists (``Engine.radius_matches`` under the identity pose), and FPFH end to end over either, per side.

Clouds: n points of the bumpy height field at the density of 1024 points on [0, 3]^2 (``fpfh.jittered_surface``), voxel = 3 / 32, the
radius 5 x voxel (about 78 neighbours a row); n = 5000, 16384 and 65536.  Per n: the index build, the count pass and the fill pass
of the grid for max_nn 0, 100 and 30 (30 binds at ~70 entries a row: the hybrid selection; device events around the C entries),
the whole ``radius_neighbors`` call, the whole ``radius_matches`` call where it takes the shape (J K <= 2^31 - 1 per call: 65536 x 65536 is refused, reported as null), and
``fpfh`` on the lists including the search.  Warm-up first, the sides alternating, the median of --repeats; the two CSRs are compared
before anything is timed.  Prints one JSON line per n.  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VOXEL = 3.0 / 32.0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def med(xs):
    return round(float(np.median(xs)), 3)


def passes(index, jobs, max_nn):
    """The count and the fill pass of one search, each between its own events -> (count ms, fill ms, total entries)."""
    from deepsir_amd.train import _ptr
    ops = index.ops
    rows = int(index.rows(jobs)[-1])
    counts, offsets = ops.empty(rows, dtype=torch.int32), ops.empty(rows + 1, dtype=torch.int32)
    scratch = torch.empty(int(ops.lib.dsir_t_nn_radius_scratch(len(jobs), rows)), dtype=torch.uint8, device=ops.device)
    head = (_ptr(index.index), index.offsets.ctypes.data, index.fragments, jobs.ctypes.data, len(jobs), None, index.radius,
            index.bounds.ctypes.data, int(max_nn))
    ops.begin()
    t_count, _ = timed(lambda: ops._launch("dsir_t_nn_radius_count", *head, _ptr(counts), _ptr(offsets), _ptr(scratch)))
    total = int(offsets[-1].item())
    cols = ops.empty(total, dtype=torch.int32)
    t_fill, _ = timed(lambda: ops._launch("dsir_t_nn_radius_fill", *head, _ptr(offsets), _ptr(scratch), _ptr(cols), None, total))
    return t_count, t_fill, total


def run_case(eng, n, repeats, warmup, seed):
    from deepsir_amd import fpfh as F
    radius = 5.0 * VOXEL
    rows = np.concatenate(F.jittered_surface(n, seed), 1)                       # xyz + normal
    x = torch.from_numpy(rows[None]).cuda()
    eye = torch.eye(4, device="cuda")[:3][None].contiguous()
    jobs = np.array([[0, 0]], np.int32)
    off = np.array([0, n], np.int64)
    brute_ok = n * n <= 2 ** 31 - 1
    sides = {"grid": lambda: eng.radius_neighbors(x, radius), "grid_nn100": lambda: eng.radius_neighbors(x, radius, 100),
             "grid_nn30": lambda: eng.radius_neighbors(x, radius, 30)}
    if brute_ok:
        sides["brute"] = lambda: eng.radius_matches(x, x, eye, radius)
        want, got = sides["brute"](), sides["grid"]()
        if not (torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])):
            raise SystemExit(f"n = {n}: the grid's CSR differs from the brute-force one")
    fp = {k: (lambda f=f: eng.fpfh(x, csr=f())) for k, f in sides.items()}
    build = lambda: eng.nn_index(x[0], off, radius)
    for _ in range(warmup):
        for f in list(sides.values()) + list(fp.values()):
            f()
        passes(build(), jobs, 0)
    torch.cuda.synchronize()
    t = {k: [] for k in list(sides) + ["fpfh_" + k for k in fp] + ["build", "count", "fill", "count_nn100", "fill_nn100", "count_nn30", "fill_nn30"]}
    entries = {}
    for _ in range(repeats):
        for k, f in sides.items():
            t[k].append(timed(f)[0])
        for k, f in fp.items():
            t["fpfh_" + k].append(timed(f)[0])
        ms, index = timed(build)
        t["build"].append(ms)
        for tag, m in (("", 0), ("_nn100", 100), ("_nn30", 30)):
            c, f, entries[m] = passes(index, jobs, m)
            t["count" + tag].append(c)
            t["fill" + tag].append(f)
    res = {"points": n, "radius": round(radius, 5), "mean_row": round(entries[0] / n, 2), "mean_row_nn100": round(entries[100] / n, 2),
           "mean_row_nn30": round(entries[30] / n, 2)}
    res.update({k + "_ms": med(v) for k, v in t.items()})
    for k in ("brute", "fpfh_brute"):
        res.setdefault(k + "_ms", None)
    if brute_ok:
        res["brute_over_grid"] = round(res["brute_ms"] / res["grid_ms"], 2)
        res["fpfh_brute_over_grid"] = round(res["fpfh_brute_ms"] / res["fpfh_grid_ms"], 2)
    print(json.dumps(res), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, nargs="+", default=[5000, 16384, 65536])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_radius_nn: needs a GPU (a CPU run measures nothing)")
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    eng = Engine(NetConfig(), 0, max_points=max(a.points), max_pairs=1)
    for n in a.points:
        run_case(eng, n, a.repeats, a.warmup, a.seed)
    eng.close()


if __name__ == "__main__":
    main()
