"""FPFH descriptors (csrc/fpfh.hip): one `Engine.fpfh` call (dsir_fpfh: the SPFH pass and the gather pass) over the pyramid's 16-NN
lists timed by device events, against the numpy restatement `fpfh_host` on the same clouds, normals and lists plus the upload of its
result.  One JSON line per shape; `--out FILE` also writes them to a file.

    python tools/bench_fpfh.py [--out runs/fpfh_bench.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepsir_amd.arch import NetConfig
from deepsir_amd.engine import Engine
from deepsir_amd.fpfh import fpfh_host
from deepsir_amd.weights import generate_state_dict

res = []
for clouds, n in ((8, 5000), (2, 65536)):
    cfg = NetConfig()
    eng = Engine(cfg, 0, max_points=n, max_pairs=(clouds + 1) // 2)
    eng.load_state_dict(generate_state_dict(cfg, 0))                   # the pyramid refuses a context without weights
    rng = np.random.default_rng(clouds)
    xy = rng.uniform(0.0, 3.0 * np.sqrt(n / 1024.0), (clouds, n, 2))
    z = 0.11 * np.sin(2.3 * xy[..., 0]) + 0.09 * np.sin(3.1 * xy[..., 1]) + 0.07 * np.sin(1.7 * xy[..., 0] + 2.9 * xy[..., 1])
    host = np.concatenate([xy, z[..., None]], 2).astype(np.float32)
    dev = torch.from_numpy(host).cuda()
    _, neigh, _, _ = eng.knn_pyramid(dev)
    normals, _ = eng.estimate_normals(dev, neigh, (0.0, 0.0, 100.0))
    for _ in range(5):
        out = eng.fpfh(dev, normals, neigh_multi=neigh)
    torch.cuda.synchronize()
    times = []
    eng.use_torch_stream(True)                                         # stream-ordered: the events bracket the launches, no host sync inside
    for rep in range(5):
        reps = 50
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            out = eng.fpfh(dev, normals, neigh_multi=neigh)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / reps * 1e3)
    eng.use_torch_stream(False)
    nb, nv = neigh[:, :n].cpu().numpy(), normals.cpu().numpy()
    htimes = []
    for rep in range(3):
        t0 = time.perf_counter()
        h = fpfh_host(host, nv, neigh=nb)
        up = torch.from_numpy(h["desc"]).cuda()
        torch.cuda.synchronize()
        htimes.append((time.perf_counter() - t0) * 1e6)
    keep = ~h["band"]
    same = bool(np.array_equal(out[0].cpu().numpy().view(np.uint32)[keep], h["desc"].view(np.uint32)[keep]))
    r = {"clouds": clouds, "points": n, "device_us_per_call": [round(t, 1) for t in times],
         "host_numpy_plus_upload_us": [round(t, 1) for t in htimes], "same_bytes_outside_band": same,
         "band_share": round(float(1.0 - keep.mean()), 6), "flagged_rows": int(out[1].sum().item())}
    print(json.dumps(r), flush=True)
    res.append(r)
    eng.close()
if "--out" in sys.argv:
    fn = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(fn)), exist_ok=True)
    json.dump(res, open(fn, "w"), indent=1)
