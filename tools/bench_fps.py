"""Farthest-point sampling (csrc/fps.hip).  Per shape (clouds, n, k) = (1, 5000, 1024), (8, 5000, 1024), (128, 5000, 512),
(1, 16384, 1024), (1, 65536, 4096) on jittered surface points:
  kernel_us     dsir_farthest_point_sample, device events, stream-ordered (its one launch)
  torch_us      the same rule as a loop of torch ops on the device - the form of the reference's network/tools.py:30
                (farthest_point_sample): per step a gather, a distance, a minimum and an arg-max; device events around the whole loop.
                Its selection is compared with the kernel's (equal where no near-tie falls differently: torch's arg-max names no
                tie order and its sum of three squares no association)
and, at 16384 points, harness.register_fpfh on one pair with keypoints=None (the path and bytes of the parent commit: the yardstick),
keypoints="iss" and keypoints="fps" (1024 samples a side), wall clock per pair, with the success flag of each.  One JSON line per
measurement; `--out FILE` also writes them to a file.  Kernel shares and hardware counters are not collected here.

    python tools/bench_fps.py [--out runs/fps_bench.json]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepsir_amd import fpfh as F
from deepsir_amd.arch import NetConfig
from deepsir_amd.engine import Engine
from deepsir_amd.harness import register_fpfh
from deepsir_amd.weights import generate_state_dict

R_SAL, R_NMS, VOXEL = 0.3, 0.2, 0.05                              # tools/bench_iss.py's pair and radii


def device_us(fn, reps=20, rounds=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(round(e0.elapsed_time(e1) / reps * 1e3, 1))
    return out


def surface_pair(n, seed):
    """bumpy_pair's layout at jittered_surface's own density (the extent grows with n), as tools/bench_iss.py builds it"""
    rng = np.random.Generator(np.random.Philox(key=seed + 7919))
    ref, _ = F.jittered_surface(n, seed)
    M = F.random_pose(rng)
    perm = rng.permutation(n)
    src = (ref[perm].astype(np.float64) @ M[:, :3].T + M[:, 3]).astype(np.float32)
    mid = float(ref[:, 0].max()) / 2
    v_ref = np.array([mid, mid, 10.0])
    gt = np.concatenate([M[:, :3].T, -(M[:, :3].T @ M[:, 3])[:, None]], 1)
    return {"points_src": src[None], "points_ref": ref[None], "transform_gt": gt[None].astype(np.float32),
            "viewpoint_src": (M[:, :3] @ v_ref + M[:, 3])[None].astype(np.float32), "viewpoint_ref": v_ref[None].astype(np.float32)}

SHAPES = ((1, 5000, 1024), (8, 5000, 1024), (128, 5000, 512), (1, 16384, 1024), (1, 65536, 4096))


def torch_fps(xyz, k, start=0):
    """network/tools.py:30 with the first row fixed and selected rows excluded: [B, N, 3] -> [B, k] long"""
    B, N, _ = xyz.shape
    centroids = torch.zeros(B, k, dtype=torch.long, device=xyz.device)
    distance = torch.full((B, N), float("inf"), device=xyz.device)
    farthest = torch.full((B,), start, dtype=torch.long, device=xyz.device)
    batch = torch.arange(B, device=xyz.device)
    for i in range(k):
        centroids[:, i] = farthest
        centroid = xyz[batch, farthest, :].view(B, 1, 3)
        d = xyz - centroid
        dist = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        distance = torch.minimum(distance, dist)
        distance[batch, farthest] = -1.0
        farthest = torch.max(distance, -1)[1]
    return centroids


def main():
    res = []
    cfg = NetConfig()
    for clouds, n, k in SHAPES:
        eng = Engine(cfg, 0, max_points=n, max_pairs=1)              # the entry takes any number of clouds: no workspace but the streaming copy
        pts = torch.from_numpy(np.stack([F.jittered_surface(n, 31 + n + c)[0] for c in range(clouds)])).cuda()
        out = eng.farthest_point_sample(pts, k)
        eng.use_torch_stream(True)                                 # stream-ordered: the events bracket the launch, no host sync inside
        bufs = [torch.empty((clouds, k), dtype=torch.int32, device="cuda"), torch.empty((clouds,), dtype=torch.int32, device="cuda"),
                torch.empty((clouds, k), device="cuda")]

        def raw():
            rc = eng.lib.dsir_farthest_point_sample(eng.h, pts.data_ptr(), 3, None, clouds, n, k, 0, *[t.data_ptr() for t in bufs])
            assert rc == 0, eng.lib.dsir_last_error(eng.h)

        kernel = device_us(raw)
        assert all(torch.equal(a, b) for a, b in zip(bufs, out))
        eng.use_torch_stream(False)
        loop = device_us(lambda: torch_fps(pts, k), reps=1, rounds=3)
        same = float((torch_fps(pts, k) == out[0].long()).float().mean())
        r = {"what": "farthest_point_sample", "clouds": clouds, "points": n, "k": k, "kernel_us": kernel, "torch_loop_us": loop,
             "us_per_step": round(float(np.median(kernel)) / k, 3), "torch_selection_equal": round(same, 4)}
        print(json.dumps(r), flush=True)
        res.append(r)
        eng.close()
    n = 16384
    eng = Engine(cfg, 0, max_points=n, max_pairs=1)
    eng.load_state_dict(generate_state_dict(cfg, 0))
    pr = surface_pair(n, 5)
    kw = dict(voxel_size=VOXEL, hypotheses=1024, seed=0)
    for name, extra in (("register_fpfh keypoints=None (the parent commit's path)", {}),
                        ("register_fpfh keypoints='iss'", dict(keypoints="iss", salient_radius=R_SAL, non_max_radius=R_NMS)),
                        ("register_fpfh keypoints='fps'", dict(keypoints="fps", num_keypoints=1024))):
        register_fpfh([pr], eng, **kw, **extra)
        times, last = [], None
        for _ in range(3):
            last = register_fpfh([pr], eng, want_keypoints=True, **kw, **extra)
            times.append(round(float(last[1][0, 3]) * 1e6, 1))
        r = {"what": name, "points": n, "pair_us": times, "succ": float(last[1][0, 0]), "rte": round(float(last[1][0, 1]), 4),
             "rre": round(float(last[1][0, 2]), 3), "matched_on": [int(len(last[2][0][0])), int(len(last[2][0][1]))],
             "fell_back": bool(last[2][0][2])}
        print(json.dumps(r), flush=True)
        res.append(r)
    eng.close()
    if "--out" in sys.argv:
        fn = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(fn)), exist_ok=True)
        json.dump(res, open(fn, "w"), indent=1)


if __name__ == "__main__":
    main()
