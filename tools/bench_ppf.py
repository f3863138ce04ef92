"""Times of the use_ppf kernels (csrc/ppf.hip) on the device, for profiles/README.md ("PPF front end").

    python tools/bench_ppf.py [--clouds 256] [--n 5000] [--pairs 8] [--iters 20]

Prints one JSON line: HIP-event time per call of ``dsir_ppf_pre`` (both kernels) and ``dsir_estimate_normals`` on
``clouds`` x ``n`` points, and ``dsir_register`` per pair (5 iterations, ``pairs`` pairs of ``n`` points per call) with and
without DSIR_FLAG_PPF.  Per-kernel times - ``ppf_stats_kernel``, ``ppf_apply_kernel``, ``estimate_normals_kernel``, and for scale
the non-PPF ``mlp_pre`` launch (the first ``pw_stream_kernel`` of a RandLA pass) - come from a trace of their own:
``rocprofv3 --kernel-trace --stats -- python tools/bench_ppf.py``.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deepsir_amd.arch import NetConfig  # noqa: E402
from deepsir_amd.engine import Engine  # noqa: E402
from deepsir_amd.weights import generate_state_dict  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = __import__("time").perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (__import__("time").perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.Generator(np.random.Philox(key=5))
    res = {"clouds": a.clouds, "n": a.n, "pairs": a.pairs}
    for ppf in (True, False):
        cfg = NetConfig(feat_len=6 if ppf else 3, use_ppf=ppf)
        eng = Engine(cfg, max_points=a.n, max_pairs=max(a.pairs, (a.clouds + 1) // 2))
        eng.load_state_dict(generate_state_dict(cfg, 0))
        xyz = rng.uniform(0.0, 3.0, (a.clouds, a.n, 3)).astype(np.float32)
        pts = torch.from_numpy(xyz).cuda()
        if ppf:
            _, neigh, _, _ = eng.knn_pyramid(pts)
            res["estimate_normals_ms"] = timed(lambda: eng.estimate_normals(pts, neigh), a.iters)
            rows = torch.cat([pts, eng.estimate_normals(pts, neigh)[0]], 2).contiguous()
            res["ppf_pre_ms"] = timed(lambda: eng.ppf_pre("feat_extractor", rows, neigh), a.iters)
        else:
            rows = pts
        src, ref = rows[:a.pairs].contiguous(), rows[a.pairs:2 * a.pairs].contiguous()
        res["register_ms_per_pair_ppf" if ppf else "register_ms_per_pair"] = timed(lambda: eng.register(src, ref, 5), max(a.iters // 4, 3)) / a.pairs
        eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
