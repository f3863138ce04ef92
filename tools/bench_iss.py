"""ISS keypoints (csrc/iss.hip).  Per shape (one cloud of 5000 / 16384 / 65536 surface points, salient radius 0.3, non-max radius 0.2
on a point spacing of ~0.094: rows of ~32 and ~14 entries; `--wide` takes 6 and 4 spacings instead: ~113 and ~50):
  kernels_us          dsir_iss_keypoints on ready CSR lists, device events, stream-ordered (its three launches)
  saliency_us         the same call with a non-max CSR of empty rows: the saliency kernel plus two launches that have nothing to scan
  select_compact_us   the difference of the two (no per-kernel trace is taken here)
  call_radius_us      Engine.iss_keypoints from the two radii, wall clock: two cell-index builds and radius searches, then the above
and, at 16384 points, harness.register_fpfh on one pair with keypoints=None (the path and bytes of the parent commit: the yardstick)
and with keypoints="iss", wall clock per pair, with the success flag of both.  One JSON line per measurement; `--out FILE` also writes
them to a file.

    python tools/bench_iss.py [--wide] [--out runs/iss_bench.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepsir_amd import fpfh as F
from deepsir_amd.arch import NetConfig
from deepsir_amd.engine import Engine
from deepsir_amd.harness import register_fpfh
from deepsir_amd.weights import generate_state_dict

SPACING = 3.0 / 32.0
R_SAL, R_NMS = (6 * SPACING, 4 * SPACING) if "--wide" in sys.argv else (0.3, 0.2)
VOXEL = 0.05


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


def wall_us(fn, rounds=5):
    fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(round((time.perf_counter() - t0) * 1e6, 1))
    return out


def surface_pair(n, seed):
    """bumpy_pair's layout at jittered_surface's own density (the extent grows with n)"""
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


res = []
cfg = NetConfig()
for n in (5000, 16384, 65536):
    eng = Engine(cfg, 0, max_points=n, max_pairs=1)
    eng.load_state_dict(generate_state_dict(cfg, 0))
    dev = torch.from_numpy(F.jittered_surface(n, 31 + n)[0][None]).cuda()
    sal, nms = eng.radius_neighbors(dev, R_SAL, 0), eng.radius_neighbors(dev, R_NMS, 0)
    empty = (torch.zeros(n + 1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))
    out = eng.iss_keypoints(dev, csr_salient=sal, csr_nms=nms)
    call = wall_us(lambda: eng.iss_keypoints(dev, salient_radius=R_SAL, non_max_radius=R_NMS))
    eng.use_torch_stream(True)                                     # stream-ordered: the events bracket the launches, no host sync inside
    bufs = [torch.empty((1, n), device="cuda")] + [torch.empty((1, n), dtype=torch.int32, device="cuda") for _ in range(3)]

    def raw(a, b):                                                 # the C entry itself: Engine._csr's checks read back from the device
        rc = eng.lib.dsir_iss_keypoints(eng.h, dev.data_ptr(), 3, a[0].data_ptr(), a[1].data_ptr(), b[0].data_ptr(), b[1].data_ptr(), 1, n,
                                        0.975, 0.975, 5, *[t.data_ptr() for t in bufs])
        assert rc == 0, eng.lib.dsir_last_error(eng.h)

    whole = device_us(lambda: raw(sal, nms))
    assert torch.equal(bufs[2], out[0]) and torch.equal(bufs[0], out[2])
    first = device_us(lambda: raw(sal, empty))
    eng.use_torch_stream(False)
    r = {"what": "iss_keypoints", "points": n, "salient_radius": round(R_SAL, 4), "non_max_radius": round(R_NMS, 4),
         "salient_row_mean": round(sal[1].numel() / n, 1), "nms_row_mean": round(nms[1].numel() / n, 1), "keypoints": int(out[1][0]),
         "kernels_us": whole, "saliency_us": first, "select_compact_us": round(float(np.median(whole) - np.median(first)), 1),
         "call_radius_us": call}
    print(json.dumps(r), flush=True)
    res.append(r)
    if n == 16384:
        pr = surface_pair(n, 5)
        kw = dict(voxel_size=VOXEL, hypotheses=1024, seed=0)
        for name, extra in (("register_fpfh keypoints=None (the parent commit's path)", {}),
                            ("register_fpfh keypoints='iss'", dict(keypoints="iss", salient_radius=R_SAL, non_max_radius=R_NMS))):
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
