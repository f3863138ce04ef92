"""Time dsir_fgr_correspondence (csrc/fgr.hip) against dsir_ransac_correspondence and dsir_consensus_correspondence on the same
correspondences, each estimator at its defaults.

    python tools/bench_fgr.py [--pairs 1 8 64] [--m 2000 5000 20000] [--outliers 0.5 0.9] [--reps 5] [--no-tuple-test]

For every (outlier share, M, pairs): `ransac.make_problem` inputs, one warm-up call, then the mean time of a synchronised call through
Engine.fgr_correspondence, Engine.ransac_correspondence and Engine.consensus_correspondence, and each result's worst pose error
against T_gt over the pairs.  An estimator that refuses the shape (consensus: its bit matrix) is reported as null with the refusal's
text.  Prints one JSON line per shape.  The optimise kernel keeps one workgroup per pair busy: a call uses P of the 256 CUs in that
phase.  Under `rocprofv3 --kernel-trace --stats -- python tools/bench_fgr.py ...` the split between the tuple selection
(fgr_select_kernel), fgr_optimize_kernel and the tail (pose_score / pick / weights / finish, kabsch) comes from the profiler's table."""
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
from deepsir_amd.engine import Engine, EngineError  # noqa: E402


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


def report(name, fn, reps, probs, rec):
    try:
        t, (T, s, _) = timed(fn, reps)
    except EngineError as e:
        rec[f"{name}_ms_per_call"], rec[f"{name}_refused"] = None, str(e)[:160]
        return
    rec[f"{name}_ms_per_call"] = round(t * 1e3, 3)
    rec[f"{name}_worst_rad_m"] = worst_error(T, probs)
    rec[f"{name}_min_inliers"] = int(s[:, 4].min())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--m", type=int, nargs="+", default=[2000, 5000, 20000])
    ap.add_argument("--outliers", type=float, nargs="+", default=[0.5, 0.9])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-tuple-test", action="store_true", help="also time FGR with tuple_test = 0 (every live row listed)")
    a = ap.parse_args()
    eng = Engine(NetConfig(), max_points=max(max(a.m), 1024), max_pairs=max(a.pairs))
    for share in a.outliers:
        for m in a.m:
            for pairs in a.pairs:
                probs = [R.make_problem(m, share, 0.005, 100 + p) for p in range(pairs)]
                src = torch.from_numpy(np.stack([p["src"] for p in probs])).cuda()
                ref = torch.from_numpy(np.stack([p["ref"] for p in probs])).cuda()
                corr = torch.from_numpy(np.stack([p["corr"] for p in probs]).astype(np.int32)).cuda()
                rec = {"pairs": pairs, "M": m, "outliers": share}
                report("fgr", lambda: eng.fgr_correspondence(src, ref, corr, 0.05), a.reps, probs, rec)
                if a.no_tuple_test:
                    report("fgr_all_rows", lambda: eng.fgr_correspondence(src, ref, corr, 0.05, tuple_test=False), a.reps, probs, rec)
                report("ransac", lambda: eng.ransac_correspondence(src, ref, corr, 0.05), a.reps, probs, rec)
                report("consensus", lambda: eng.consensus_correspondence(src, ref, corr, 0.05), a.reps, probs, rec)
                print(json.dumps(rec), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
