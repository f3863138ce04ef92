"""Time per call of the ICP refinement (csrc/icp.hip) for both estimators on surface clouds (the clouds of tests/test_icp_plane.py: a
height field and a wall), started 3 degrees and up to 0.05 per axis off the truth, radius 0.1, 30 iterations allowed.

    python tools/bench_icp.py --pairs 8 --points 5000 --estimator point plane
    python tools/bench_icp.py --pairs 1 --points 20000 --estimator point plane

    python tools/bench_icp.py --pairs 1 --points 65536 --estimator point --search brute grid
    python tools/bench_icp.py --pairs 1 --points 100000 --scale 8.5 --init-angle 0.3 --radius 0.2 --max-iter 200 --estimator point --search brute grid

``--search`` times the brute-force search and the cell index of csrc/icp_grid.hip side by side (same poses, byte for byte: the tool
checks it); the second line above is the shape of the KITTI ground-truth refinement (two scans thinned at 0.05 m: about 400 points
per square metre, hence the surface scaled by 8.5 at 10^5 points; started close, as from odometry).

One JSON line per estimator and search: median / min / max milliseconds per call over --reps calls (after --warmup), the iterations each pair
took.  ``--estimator point`` alone runs on a build that predates the plane estimator, for A/B runs against it.  The per-kernel
split is the profiler's: ``rocprofv3 --kernel-trace --stats -- python tools/bench_icp.py ...``."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _rodrigues(ax, a):
    ax = np.asarray(ax, np.float64) / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def surface_pair(n, seed, noise, scale=1.0, init_angle=3.0):
    rng = np.random.default_rng(seed)
    m = n * 3 // 4
    xy = rng.uniform(0, 1.5, (m, 2))
    uv = rng.uniform(0, 1.0, (n - m, 2))
    base = np.r_[np.c_[xy, 0.15 * np.sin(3.0 * xy[:, 0]) * np.cos(2.5 * xy[:, 1])],
                 np.c_[0.02 * np.sin(4.0 * uv[:, 0]), 1.5 * uv[:, 0], 0.8 * uv[:, 1] - 0.15]][rng.permutation(n)] * scale
    R, t = _rodrigues(rng.standard_normal(3), rng.uniform(0.3, 1.0)), rng.uniform(-0.5, 0.5, 3)
    src = ((base[rng.permutation(n)] - t) @ R).astype(np.float32)
    ref = (base + rng.normal(0, noise, base.shape)).astype(np.float32)
    dR = _rodrigues(rng.standard_normal(3), np.deg2rad(init_angle))
    T0 = np.hstack([dR @ R, (dR @ t + rng.uniform(-0.05, 0.05, 3))[:, None]]).astype(np.float32)
    return src, ref, T0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--noise", type=float, default=0.002)
    ap.add_argument("--radius", type=float, default=0.1)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--estimator", nargs="+", choices=["point", "plane"], default=["point", "plane"])
    ap.add_argument("--search", nargs="+", choices=["brute", "grid", "auto"], default=None,
                    help="searches to time; without the flag the call is made as before it existed (the brute force)")
    ap.add_argument("--scale", type=float, default=1.0, help="stretch the surface (1.0: about 1.5 x 1.5)")
    ap.add_argument("--init-angle", type=float, default=3.0, help="degrees the start is off the truth")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    cases = [surface_pair(a.points, 100 + k, a.noise, a.scale, a.init_angle) for k in range(a.pairs)]
    src, ref, T0 = (torch.from_numpy(np.stack([c[i] for c in cases])).cuda() for i in range(3))
    eng = Engine(NetConfig(), 0, max_points=max(a.points, 1024), max_pairs=a.pairs)
    for est in a.estimator:
        kw = {}
        if est == "plane":
            kw = dict(estimator="plane", normals_ref=eng.icp_normals(ref))
        first = None
        for search in a.search or [None]:
            if search is not None:
                kw["search"] = search
            ms = []
            for i in range(a.warmup + a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                T, st = eng.icp_refine(src, ref, T0, a.radius, max_iter=a.max_iter, **kw)
                torch.cuda.synchronize()
                if i >= a.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            out = (T.cpu().numpy().tobytes(), st.cpu().numpy().tobytes())
            first = first or out
            st = st.cpu().numpy()
            row = {"tag": a.tag, "estimator": est, "pairs": a.pairs, "points": a.points, "ms_median": round(float(np.median(ms)), 3),
                   "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "iterations": st[:, 3].astype(int).tolist(),
                   "converged": st[:, 2].astype(int).tolist(), "fitness_mean": round(float(st[:, 0].mean()), 4)}
            if search is not None:
                row.update(search=search, radius=a.radius, same_bytes_as_first=out == first)
            print(json.dumps(row), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
