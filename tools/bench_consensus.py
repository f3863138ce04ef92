"""Time dsir_consensus_correspondence (csrc/consensus.hip) against dsir_ransac_correspondence on the same correspondences.

    python tools/bench_consensus.py [--pairs 1 4 8] [--m 1000 5000] [--outliers 0.9] [--hypotheses 8192] [--reps 5]

For every (pairs, M): `ransac.make_problem` inputs, one warm-up call, then the mean time of a synchronised call through
Engine.consensus_correspondence and through Engine.ransac_correspondence, and each result's worst pose error against T_gt over the
pairs.  Prints one JSON line per shape.  Under `rocprofv3 --kernel-trace --stats -- python tools/bench_consensus.py ...` the kernel
shares come from the profiler's table."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepsir_amd import ransac as R  # noqa: E402
from deepsir_amd.arch import NetConfig  # noqa: E402
from deepsir_amd.engine import Engine  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def worst_error(T, probs):
    err = [R.pose_error(T[p].cpu().numpy(), probs[p]["T_gt"]) for p in range(len(probs))]
    return [float(f"{max(e[0] for e in err):.2e}"), float(f"{max(e[1] for e in err):.2e}")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--m", type=int, nargs="+", default=[1000, 5000])
    ap.add_argument("--outliers", type=float, default=0.9)
    ap.add_argument("--hypotheses", type=int, default=8192)
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--members", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    eng = Engine(NetConfig(), max_points=max(max(a.m), 1024), max_pairs=max(a.pairs))
    for m in a.m:
        for pairs in a.pairs:
            probs = [R.make_problem(m, a.outliers, 0.005, 100 + p) for p in range(pairs)]
            src = torch.from_numpy(np.stack([p["src"] for p in probs])).cuda()
            ref = torch.from_numpy(np.stack([p["ref"] for p in probs])).cuda()
            corr = torch.from_numpy(np.stack([p["corr"] for p in probs]).astype(np.int32)).cuda()
            tc, (Tc, sc, _) = timed(lambda: eng.consensus_correspondence(src, ref, corr, 0.05, seeds=a.seeds, members=a.members), a.reps)
            tr, (Tr, sr, _) = timed(lambda: eng.ransac_correspondence(src, ref, corr, 0.05, hypotheses=a.hypotheses), a.reps)
            print(json.dumps({"pairs": pairs, "M": m, "outliers": a.outliers, "consensus_ms_per_call": round(tc * 1e3, 3),
                              "consensus_worst_rad_m": worst_error(Tc, probs), "consensus_inliers": [int(x) for x in sc[:, 4].cpu()],
                              "ransac_hypotheses": a.hypotheses, "ransac_ms_per_call": round(tr * 1e3, 3),
                              "ransac_worst_rad_m": worst_error(Tr, probs), "ransac_inliers": [int(x) for x in sr[:, 4].cpu()]}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
