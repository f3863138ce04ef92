"""Times of the scene-registration entries (profiles/README.md, "Pose graph"); nothing is asserted.

  python tools/bench_pose_graph.py [--reps 5] [--host]

information_matrix at 8 x 5000 and 1 x 65536 points next to icp_correspondences alone at the same shapes (the added cost is the
quantity of interest); pose_graph_optimize at the 3DMatch scene shape (N = 60, E ~ 400), at N = 128, and 8 graphs per call, with
a fixed number of solves (max_iter) so that the time per solve can be read off.  --host: also time pose_graph.optimize_host on
the CPU, the baseline.  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deepsir_amd import pose_graph as PG                      # noqa: E402
from deepsir_amd.arch import NetConfig                        # noqa: E402
from deepsir_amd.engine import Engine                         # noqa: E402
from deepsir_amd.synth import make_pose_graph as make_graph   # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    eng = Engine(NetConfig(), 0, max_points=65536, max_pairs=8)
    rng = np.random.default_rng(0)
    for P, n in ((8, 5000), (1, 65536)):
        ref = torch.from_numpy(rng.uniform(0, 3, (P, n, 3)).astype(np.float32)).cuda()
        src = (ref + 0.01).contiguous()
        T = torch.eye(3, 4).repeat(P, 1, 1).cuda().contiguous()
        for search in ("brute", "grid"):
            t_c = timed(lambda: eng.icp_correspondences(src, ref, T, 0.1, search=search), a.reps)
            t_i = timed(lambda: eng.information_matrix(src, ref, T, 0.1, search=search), a.reps)
            print(json.dumps({"op": "information_matrix", "pairs": P, "points": n, "search": search, "icp_correspondences_ms": round(t_c, 3),
                              "information_matrix_ms": round(t_i, 3), "added_ms": round(t_i - t_c, 3)}), flush=True)
    for name, N, loops, G in (("scene60", 60, 341, 1), ("n128", 128, 400, 1), ("scene60x8", 60, 341, 8)):
        gs = [make_graph(N, 100 + k, loops=loops, noise=(0.002, 0.005), start=(0.02, 0.02))[0] for k in range(G)]
        row = {"op": "pose_graph_optimize", "case": name, "graphs": G, "N": N, "E": int(len(gs[0].st)), "unknowns": 6 * (N - 1)}
        for it in (2, 10):
            row[f"device_ms_max_iter_{it}"] = round(timed(lambda: eng.pose_graph_optimize(gs, max_iter=it), a.reps), 3)
        row["device_ms_per_solve"] = round((row["device_ms_max_iter_10"] - row["device_ms_max_iter_2"]) / 8, 3)
        if a.host:
            t0 = time.perf_counter()
            for g in gs:
                PG.optimize_host(g, 10)
            row["host_ms_max_iter_10"] = round((time.perf_counter() - t0) * 1e3, 1)
        print(json.dumps(row), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
