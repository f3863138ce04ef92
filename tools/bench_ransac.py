"""Time dsir_ransac_correspondence (csrc/ransac.hip) and, optionally, the host restatement on the same problem.

    python tools/bench_ransac.py [--pairs 8] [--m 5000] [--hypotheses 8192] [--reps 5] [--host]

Prints one JSON line: the mean device time per call (a synchronised call through Engine.ransac_correspondence, after a warm-up),
the result's fitness per pair and, with --host, the restatement's wall time for ONE pair times the pair count.  Under
`rocprofv3 --kernel-trace --stats -- python tools/bench_ransac.py ...` the kernel shares come from the profiler's table."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--m", type=int, default=5000)
    ap.add_argument("--hypotheses", type=int, default=8192)
    ap.add_argument("--outliers", type=float, default=0.7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    probs = [R.make_problem(a.m, a.outliers, 0.005, 100 + p) for p in range(a.pairs)]
    eng = Engine(NetConfig(), max_points=max(a.m, 1024), max_pairs=a.pairs)
    src = torch.from_numpy(np.stack([p["src"] for p in probs])).cuda()
    ref = torch.from_numpy(np.stack([p["ref"] for p in probs])).cuda()
    corr = torch.from_numpy(np.stack([p["corr"] for p in probs]).astype(np.int32)).cuda()
    eng.ransac_correspondence(src, ref, corr, 0.05, hypotheses=a.hypotheses)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        T, stats, _ = eng.ransac_correspondence(src, ref, corr, 0.05, hypotheses=a.hypotheses)
    torch.cuda.synchronize()
    dev = (time.perf_counter() - t0) / a.reps
    out = {"pairs": a.pairs, "M": a.m, "hypotheses": a.hypotheses, "device_ms_per_call": round(dev * 1e3, 3),
           "fitness": [round(float(x), 4) for x in stats[:, 0].cpu()], "valid_hypotheses": [int(x) for x in stats[:, 3].cpu()]}
    if a.host:
        t0 = time.perf_counter()
        res = R.ransac_pair(probs[0]["src"], probs[0]["ref"], probs[0]["corr"], hypotheses_n=a.hypotheses)
        one = time.perf_counter() - t0
        out["host_restatement_ms_one_pair"] = round(one * 1e3, 1)
        out["host_restatement_ms_all_pairs"] = round(one * 1e3 * a.pairs, 1)
        out["host_equals_device_inliers_pair0"] = bool(res["stats"][4] == float(stats[0, 4]))
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
