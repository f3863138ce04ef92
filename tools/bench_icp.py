"""Time per call of the ICP refinement (csrc/icp.hip) for both estimators on surface clouds (the clouds of tests/test_icp_plane.py: a
height field and a wall), started 3 degrees and up to 0.05 per axis off the truth, radius 0.1, 30 iterations allowed.

    python tools/bench_icp.py --pairs 8 --points 5000 --estimator point plane
    python tools/bench_icp.py --pairs 1 --points 20000 --estimator point plane

    python tools/bench_icp.py --pairs 1 --points 65536 --estimator point --search brute grid
    python tools/bench_icp.py --pairs 1 --points 100000 --scale 8.5 --init-angle 0.3 --radius 0.2 --max-iter 200 --estimator point --search brute grid

``--search`` times the brute-force search and the cell index of csrc/icp_grid.hip side by side (same poses, byte for byte: the tool
checks it); the second line above is the shape of the KITTI ground-truth refinement (two scans thinned at 0.05 m: about 400 points
per square metre, hence the surface scaled by 8.5 at 10^5 points; started close, as from odometry).

``--ragged`` times the refinement of clouds of unequal sizes: 32 seeded pairs with J and K drawn uniformly from 2000..6000 (the same
surfaces, cut to size), both estimators (unless --estimator narrows them), search brute and grid, --max-iter iterations allowed.

    python tools/bench_icp.py --ragged
    python tools/bench_icp.py --ragged --ragged-modes per-pair          # runs on a build that predates the counts, for A/B runs

Mode "per-pair" is one dense call per pair, 32 calls; mode "batched" is one call with counts_src / counts_ref per batch of 8 and of 32
pairs (batches as harness.register_scene makes them, padded with harness.pad_clouds), and checks that its poses and statistics are
the per-pair ones byte for byte.  One JSON line per estimator, search and mode: the time for all 32 pairs.

``--kernel`` / ``--kernel-scale`` time the loop under a robust loss kernel of the estimator (csrc/icp_robust.h); the iteration counts
change with the kernel, so every line also carries the time per iteration (the call's time over the largest iteration count of its pairs).

    python tools/bench_icp.py --pairs 8 --points 5000 --kernel l2 huber cauchy gm tukey --kernel-scale 0.03

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


def _timed(fn, warmup, reps):
    """-> (the last result, [ms per call of fn] over reps calls after warmup), every call between two device synchronisations"""
    ms, out = [], None
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def ragged(a):
    """--ragged: the module docstring says what is timed"""
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    P, LO, HI = 32, 2000, 6000
    rng = np.random.default_rng(2024)
    sizes = [(int(j), int(k)) for j, k in rng.integers(LO, HI + 1, (P, 2))]
    cases = [surface_pair(max(j, k), 500 + p, a.noise, a.scale, a.init_angle) for p, (j, k) in enumerate(sizes)]
    src = [torch.from_numpy(c[0][:j]).cuda() for c, (j, k) in zip(cases, sizes)]
    ref = [torch.from_numpy(c[1][:k]).cuda() for c, (j, k) in zip(cases, sizes)]
    T0 = torch.from_numpy(np.stack([c[2] for c in cases])).cuda()
    eng = Engine(NetConfig(), 0, max_points=HI, max_pairs=P)
    nrm = [eng.icp_normals(r[None])[0] for r in ref] if "plane" in a.estimator else None
    row = lambda est, search, mode, ms, st, **kw: print(json.dumps(dict(
        tag=a.tag, ragged=True, estimator=est, search=search, mode=mode, pairs=P, sizes=[LO, HI], max_iter=a.max_iter,
        ms_median=round(float(np.median(ms)), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), reps=len(ms),
        iterations_mean=round(float(st[:, 3].mean()), 2), fitness_mean=round(float(st[:, 0].mean()), 4), **kw)), flush=True)
    for est in a.estimator:
        for search in a.search or ["brute", "grid"]:
            kw = dict(max_iter=a.max_iter, estimator=est, search=search)

            def per_pair():
                outs = [eng.icp_refine(src[p][None], ref[p][None], T0[p:p + 1], a.radius, normals_ref=nrm[p][None] if est == "plane" else None, **kw)
                        for p in range(P)]
                return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])

            base = None
            if "per-pair" in a.ragged_modes:
                base, ms = _timed(per_pair, a.warmup, a.reps)
                row(est, search, "per-pair", ms, base[1].cpu().numpy(), calls=P)
            if "batched" not in a.ragged_modes:
                continue
            from deepsir_amd import harness as H
            base = base or per_pair()
            for batch in (8, 32):
                plan = H.scene_batches(sizes, batch)
                packs = []
                for kb in plan:                                         # padded once, outside the timed calls: what a caller keeps
                    s_, cs = H.pad_clouds([src[k] for k in kb])
                    r_, cr = H.pad_clouds([ref[k] for k in kb])
                    packs.append((kb, s_, r_, H.pad_clouds([nrm[k] for k in kb])[0] if est == "plane" else None, T0[kb].contiguous(), cs, cr))

                def batched():
                    T, st = torch.empty_like(base[0]), torch.empty_like(base[1])
                    for kb, s_, r_, n_, t_, cs, cr in packs:
                        T[kb], st[kb] = eng.icp_refine(s_, r_, t_, a.radius, normals_ref=n_, counts_src=cs, counts_ref=cr, **kw)
                    return T, st

                out, ms = _timed(batched, a.warmup, a.reps)
                same = out[0].cpu().numpy().tobytes() == base[0].cpu().numpy().tobytes() and out[1].cpu().numpy().tobytes() == base[1].cpu().numpy().tobytes()
                row(est, search, f"batched-{batch}", ms, out[1].cpu().numpy(), calls=len(plan), same_bytes_as_per_pair=same)
    eng.close()


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
    ap.add_argument("--ragged", action="store_true", help="32 pairs of unequal sizes (2000..6000): one call per pair against one call with counts")
    ap.add_argument("--ragged-modes", nargs="+", choices=["per-pair", "batched"], default=["per-pair", "batched"])
    ap.add_argument("--kernel", nargs="+", choices=["l2", "huber", "cauchy", "gm", "tukey"], default=None,
                    help="robust kernels to time; without the flag the call is made as before it existed (least squares)")
    ap.add_argument("--kernel-scale", type=float, default=0.03, help="the kernels' scale k (gm takes k * k: its k is a squared length)")
    a = ap.parse_args()
    if a.ragged:
        return ragged(a)
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
        for search, kernel in [(s_, k_) for s_ in a.search or [None] for k_ in a.kernel or [None]]:
            if search is not None:
                kw["search"] = search
            if kernel is not None:
                kw.update(kernel=kernel, kernel_scale=a.kernel_scale ** 2 if kernel == "gm" else a.kernel_scale)
            ms = []
            for i in range(a.warmup + a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                T, st = eng.icp_refine(src, ref, T0, a.radius, max_iter=a.max_iter, **kw)
                torch.cuda.synchronize()
                if i >= a.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            out = (T.cpu().numpy().tobytes(), st.cpu().numpy().tobytes())
            first = first if kernel not in (None, "l2") or first else out      # same_bytes_as_first compares the least-squares runs
            st = st.cpu().numpy()
            row = {"tag": a.tag, "estimator": est, "pairs": a.pairs, "points": a.points, "ms_median": round(float(np.median(ms)), 3),
                   "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "iterations": st[:, 3].astype(int).tolist(),
                   "converged": st[:, 2].astype(int).tolist(), "fitness_mean": round(float(st[:, 0].mean()), 4)}
            if search is not None:
                row.update(search=search, radius=a.radius)
                if kernel in (None, "l2"):
                    row.update(same_bytes_as_first=out == first)
            if kernel is not None:
                row.update(kernel=kernel, kernel_scale=kw["kernel_scale"], ms_per_iteration=round(float(np.median(ms)) / max(1, int(st[:, 3].max())), 4))
            print(json.dumps(row), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
