"""Half-space crop (csrc/crop.hip): one `Engine.halfspace_crop` call (dsir_t_cloud_centroids + dsir_t_halfspace_crop, the upload of the
directions included) timed by device events, against the numpy restatement of RandomCrop.crop on the same clouds on the host plus the
upload the host route would need.  One JSON line per shape; `--out FILE` also writes them to a file.

    python tools/bench_crop.py [--out runs/crop_bench.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepsir_amd.arch import NetConfig
from deepsir_amd.engine import Engine
from deepsir_amd import crop as K

eng = Engine(NetConfig(), 0, max_points=2048, max_pairs=1)
res = []
for clouds, rows, stride in ((16, 40000, 3), (64, 20000, 3)):
    rng = np.random.default_rng(clouds)
    host = (rng.standard_normal((clouds, rows, stride)) * 20).astype(np.float32)
    dev = torch.from_numpy(host).cuda()
    counts = torch.full((clouds,), rows, dtype=torch.int32, device="cuda")
    idx = list(range(clouds))
    dirs = K.crop_directions(0, 0, idx, [0] * clouds)
    for _ in range(5):
        out = eng.halfspace_crop(dev, counts, 0.6, 0, 0, idx, 0)
    torch.cuda.synchronize()
    times, given = [], []
    for rep in range(5):
        # `times`: the call as TrainBatches makes it (the host draws the directions per call); `given`: the directions handed in,
        # which leaves the device work and the launches - the two alternate
        for acc, kw in ((times, {}), (given, {"directions": dirs})):
            n = 200
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                out = eng.halfspace_crop(dev, counts, 0.6, 0, 0, idx, 0, **kw)
            e1.record()
            torch.cuda.synchronize()
            acc.append(e0.elapsed_time(e1) / n * 1e3)
    # host route: numpy RandomCrop.crop restatement (mean, dot, percentile, mask) per cloud, then the upload of the kept rows
    htimes = []
    for rep in range(5):
        t0 = time.perf_counter()
        kept = []
        for c in range(clouds):
            p = host[c]
            d = (p[:, :3] - p[:, :3].mean(0)) @ dirs[c]
            kept.append(p[d > np.percentile(d, 40.0)])
        buf = np.zeros((clouds, rows, stride), np.float32)
        for c, k in enumerate(kept):
            buf[c, :len(k)] = k
        up = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        htimes.append((time.perf_counter() - t0) * 1e6)
    kept_rows = int(out[1].sum().item())
    bytes_min = clouds * rows * (stride * 4 + 4 + 5 * 4) + kept_rows * stride * 4 * 2
    r = {"clouds": clouds, "rows": rows, "stride": stride, "device_us_per_call": [round(t, 1) for t in times],
         "device_us_per_call_directions_given": [round(t, 1) for t in given],
         "host_numpy_plus_upload_us": [round(t, 1) for t in htimes], "kept_rows": kept_rows, "bytes_model": bytes_min,
         "GBps_at_median_directions_given": round(bytes_min / (sorted(given)[2] * 1e-6) / 1e9, 1)}
    print(json.dumps(r), flush=True)
    res.append(r)
if "--out" in sys.argv:
    fn = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(fn)), exist_ok=True)
    json.dump(res, open(fn, "w"), indent=1)
eng.close()
