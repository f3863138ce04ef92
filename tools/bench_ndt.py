"""Time per call of the NDT registration (csrc/ndt.hip) beside the grid point-to-plane ICP on the same inputs: surface clouds (the
clouds of tests/test_icp_plane.py), started 3 degrees and up to 0.05 per axis off the truth.

    python tools/bench_ndt.py                       # the three shapes: 8 x 5000, 1 x 65536, 1 x 100000
    python tools/bench_ndt.py --pairs 1 --points 65536 --resolution 0.2

One JSON line per shape: map build (dsir_ndt_map, which also copies the map out), the call with max_iter = 0 (map build and the
statistics pass), the full call, milliseconds per iteration ((full - max_iter 0) / the largest iteration count of its pairs), and
icp_refine(estimator="plane", search="grid") on the same inputs - medians over --reps calls after --warmup.  The surface is scaled
so that a cell of edge --resolution holds about --per-cell points.  Every timed step runs in a child process of its own under
--limit seconds; a step that does not end in time is reported as such and the tool goes on to the next shape."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(8, 5000), (1, 65536), (1, 100000)]


def surface(n, rng, scale):
    m = n * 3 // 4
    xy = rng.uniform(0, 1.5, (m, 2))
    a = np.c_[xy, 0.15 * np.sin(3.0 * xy[:, 0]) * np.cos(2.5 * xy[:, 1])]
    uv = rng.uniform(0, 1.0, (n - m, 2))
    b = np.c_[0.02 * np.sin(4.0 * uv[:, 0]), 1.5 * uv[:, 0], 0.8 * uv[:, 1] - 0.15]
    return (np.r_[a, b][rng.permutation(n)] * scale).astype(np.float32)


def rodrigues(ax, a):
    ax = np.asarray(ax, np.float64) / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def make(pairs, n, scale, seed=0):
    src, ref, T0 = [], [], []
    for p in range(pairs):
        rng = np.random.default_rng(seed + p)
        base = surface(n, rng, scale).astype(np.float64)
        R, t = rodrigues(rng.standard_normal(3), rng.uniform(0.3, 1.0)), rng.uniform(-0.5, 0.5, 3) * scale
        src.append(((base[rng.permutation(n)] - t) @ R).astype(np.float32))
        ref.append(base.astype(np.float32))
        dR = rodrigues(rng.standard_normal(3), np.deg2rad(3.0))
        T0.append(np.hstack([dR @ R, (dR @ t + rng.uniform(-0.05, 0.05, 3) * scale)[:, None]]).astype(np.float32))
    return np.stack(src), np.stack(ref), np.stack(T0)


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def step(a):
    """one timed step in this process: prints one JSON object"""
    import torch
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    scale = a.resolution * np.sqrt(a.points / a.per_cell / 3.0)        # about 3 unit squares of surface
    src, ref, T0 = (torch.from_numpy(x).cuda() for x in make(a.pairs, a.points, scale))
    eng = Engine(NetConfig(), 0, max_points=max(a.points, 1024), max_pairs=a.pairs)
    if a.step == "map":
        ms, _ = timed(lambda: eng.ndt_map(ref, a.resolution), a.reps, a.warmup)
        out = dict(ms=ms)
    elif a.step in ("ndt0", "ndt"):
        it = 0 if a.step == "ndt0" else a.max_iter
        ms, (T, st) = timed(lambda: eng.ndt_refine(src, ref, T0, a.resolution, neighbors=a.neighbors, max_iter=it), a.reps, a.warmup)
        out = dict(ms=ms, iterations=st[:, 3].cpu().tolist(), converged=st[:, 2].cpu().tolist(), matched=st[:, 1].cpu().tolist())
    else:
        nrm = torch.zeros_like(ref)
        nrm[..., 2] = 1.0                                               # the timing does not depend on the normals' values
        ms, (T, st) = timed(lambda: eng.icp_refine(src, ref, T0, a.resolution / 2, max_iter=a.max_iter, estimator="plane", normals_ref=nrm,
                                                   search="grid"), a.reps, a.warmup)
        out = dict(ms=ms, iterations=st[:, 3].cpu().tolist())
    print("STEP " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=0)
    ap.add_argument("--points", type=int, default=0)
    ap.add_argument("--resolution", type=float, default=0.2)
    ap.add_argument("--per-cell", type=float, default=25.0)
    ap.add_argument("--neighbors", type=int, default=7)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds every timed step may take")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a)
    shapes = [(a.pairs, a.points)] if a.pairs and a.points else SHAPES
    for pairs, points in shapes:
        row = dict(pairs=pairs, points=points, resolution=a.resolution, neighbors=a.neighbors)
        for name in ("map", "ndt0", "ndt", "icp_plane_grid"):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--pairs", str(pairs), "--points", str(points), "--resolution",
                   str(a.resolution), "--per-cell", str(a.per_cell), "--neighbors", str(a.neighbors), "--max-iter", str(a.max_iter), "--reps",
                   str(a.reps), "--warmup", str(a.warmup)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                row[name] = "time limit"
                break                                                   # nothing more on the GPU after a step that did not end
            line = [l for l in r.stdout.splitlines() if l.startswith("STEP ")]
            if r.returncode != 0 or not line:
                row[name] = f"failed (exit {r.returncode}): {r.stderr[-300:]}"
                break
            row[name] = json.loads(line[-1][5:])
        if isinstance(row.get("ndt"), dict) and isinstance(row.get("ndt0"), dict):
            row["ms_per_iteration"] = (row["ndt"]["ms"] - row["ndt0"]["ms"]) / max(1.0, max(row["ndt"]["iterations"]))
        print(json.dumps(row), flush=True)
        if any(isinstance(v, str) for k, v in row.items() if k in ("map", "ndt0", "ndt", "icp_plane_grid")):
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
