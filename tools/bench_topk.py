"""Time dsir_nn_match_topk (csrc/nn_topk.hip) beside dsir_nn_match, and dsir_feature_correspondences_ex beside
dsir_feature_correspondences, on the same descriptors.

    python tools/bench_topk.py [--pairs 1 8] [--points 5000 2048] [--k 1 2 4 8] [--rounds 9] [--calls 20]

For every (pairs, points): unit-norm random descriptors, every variant warmed up, then `rounds` rounds in which the variants take
turns (arg-min, top-k at every k, the two correspondence entries), each turn `calls` back-to-back calls ending in a device
synchronise.  Reported per variant: the median over the rounds of the time per call, and the spread (min .. max) over the rounds;
for top-k also the ratio to the arg-min entry's median of the same run - the yardstick, there is no ratio fixed in advance.
Prints one JSON line per shape."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepsir_amd.arch import NetConfig  # noqa: E402
from deepsir_amd.engine import Engine  # noqa: E402


def turn(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--points", type=int, nargs="+", default=[5000, 2048])
    ap.add_argument("--k", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_topk: no GPU (there is no CPU path to time)")
    # J x k rows for the correspondence entry: the context is sized for the k = 2 list
    eng = Engine(NetConfig(), max_points=max(2 * max(a.points), 1024), max_pairs=max(a.pairs))
    rng = np.random.default_rng(0)
    for n in a.points:
        for pairs in a.pairs:
            d = rng.normal(size=(2, pairs, n, 64))
            d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
            ds, dr = torch.from_numpy(d[0]).cuda(), torch.from_numpy(d[1]).cuda()
            variants = {"nn_match": lambda: eng.nn_match(ds, dr)}
            for k in a.k:
                variants[f"topk_k{k}"] = lambda k=k: eng.nn_match_topk(ds, dr, k)
            variants["corr_mutual"] = lambda: eng.feature_correspondences(ds, dr, mutual=True)
            variants["corr_ex_mutual_ratio0.8"] = lambda: eng.feature_correspondences(ds, dr, mutual=True, ratio=0.8)
            variants["corr_ex_mutual_k2"] = lambda: eng.feature_correspondences(ds, dr, mutual=True, k=2)
            for fn in variants.values():                                   # warm-up: code objects, allocator
                turn(fn, 3)
            times = {name: [] for name in variants}
            for _ in range(a.rounds):                                      # alternating turns
                for name, fn in variants.items():
                    times[name].append(turn(fn, a.calls))
            med = {name: statistics.median(t) for name, t in times.items()}
            out = {"pairs": pairs, "J": n, "K": n, "rounds": a.rounds, "calls_per_turn": a.calls}
            for name, t in times.items():
                out[name + "_ms"] = {"median": round(med[name], 4), "min": round(min(t), 4), "max": round(max(t), 4)}
            for k in a.k:
                out[f"topk_k{k}_over_nn_match"] = round(med[f"topk_k{k}"] / med["nn_match"], 3)
                out[f"topk_k{k}_splits"] = eng.nn_match_topk_splits(pairs, n, n, k)
            out["corr_ex_ratio_over_corr"] = round(med["corr_ex_mutual_ratio0.8"] / med["corr_mutual"], 3)
            out["corr_ex_k2_over_corr"] = round(med["corr_ex_mutual_k2"] / med["corr_mutual"], 3)
            print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
