"""Plane segmentation (csrc/plane.hip).  Per shape (clouds, n) = (1, 120000), (1, 16384), (8, 5000), (128, 5000) with 1024
hypotheses, one plane and one refit on scenes with a ground sheet (55 % of the rows), and (1, 120000) once more with max_planes = 4:
  call_us       dsir_segment_plane, device events, stream-ordered (all its launches)
  scoring_us    the scoring launches alone, BY DIFFERENCE: call_us minus the same call with one hypothesis (every launch the same but
                for a scoring kernel with one candidate); not a kernel trace
  torch_us      the same rule as a loop of torch ops on the device (draws made on the host beforehand, the fit in float64, the
                residual in chunks of 128 hypotheses x n, arg-max, one refit through torch.linalg.svd, the labels), device events
                around the whole loop; the two are run alternately, round by round.  Its plane is compared with the kernel's.
One JSON line per measurement; `--out FILE` also writes them to a file.

    python tools/bench_segment_plane.py [--out runs/plane_bench.json]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepsir_amd import plane as P
from deepsir_amd.arch import NetConfig
from deepsir_amd.engine import Engine

THR, H = 0.08, 1024
SHAPES = ((1, 120000, 1), (1, 16384, 1), (8, 5000, 1), (128, 5000, 1), (1, 120000, 4))


def scene(n, seed):
    """a z = 0 sheet (sigma 0.02 m) with 55 % of the rows, a wall, a second level and scattered points, 40 m across"""
    rng = np.random.Generator(np.random.Philox(key=5000 + seed))
    ns = int(0.55 * n)
    nw = (n - ns) // 3
    sheet = np.stack([rng.uniform(-20, 20, ns), rng.uniform(-20, 20, ns), rng.normal(0, 0.02, ns)], -1)
    wall = np.stack([8 + rng.normal(0, 0.02, nw), rng.uniform(-20, 20, nw), rng.uniform(0.2, 6, nw)], -1)
    deck = np.stack([rng.uniform(-20, 0, nw), rng.uniform(-20, 0, nw), 3 + rng.normal(0, 0.02, nw)], -1)
    rest = n - ns - 2 * nw
    scatter = np.stack([rng.uniform(-20, 20, rest), rng.uniform(-20, 20, rest), rng.uniform(0.3, 8, rest)], -1)
    return np.concatenate([sheet, wall, deck, scatter])[rng.permutation(n)].astype(np.float32)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / reps * 1e3, 1)


def torch_round(pts, rows, thr):
    """one round of the rule on every live row of pts [B, n, 3] with the drawn positions rows [B, H, 3] -> (plane [B, 6], labels)"""
    B, n, _ = pts.shape
    g = torch.gather(pts.double(), 1, rows.reshape(B, -1, 1).expand(-1, -1, 3)).reshape(B, -1, 3, 3)
    a, u, v = g[:, :, 0], g[:, :, 1] - g[:, :, 0], g[:, :, 2] - g[:, :, 0]
    m = torch.cross(u, v, dim=-1)
    len2 = (m * m).sum(-1)
    ok = (len2 > 0) & (rows[..., 0] != rows[..., 1]) & (rows[..., 0] != rows[..., 2]) & (rows[..., 1] != rows[..., 2])
    nrm = (m / len2.sqrt().unsqueeze(-1)).float()
    a = a.float()
    counts = torch.zeros(rows.shape[:2], dtype=torch.int64, device=pts.device)
    for h0 in range(0, rows.shape[1], 128):
        nn, aa = nrm[:, h0:h0 + 128, None], a[:, h0:h0 + 128, None]
        t = nn * (pts[:, None] - aa)
        counts[:, h0:h0 + 128] = (((t[..., 0] + t[..., 1]) + t[..., 2]).abs() < thr).sum(-1)
    best = torch.where(ok, counts, torch.full_like(counts, -1)).argmax(1)
    bi = torch.arange(B, device=pts.device)
    cur = torch.cat([nrm[bi, best], a[bi, best]], -1)

    def inl(c):
        t = c[:, None, :3] * (pts - c[:, None, 3:])
        return ((t[..., 0] + t[..., 1]) + t[..., 2]).abs() < thr

    w = inl(cur).double().unsqueeze(-1)
    cen = (pts.double() * w).sum(1) / w.sum(1)
    d = (pts.double() - cen[:, None]) * w
    n64 = torch.linalg.svd(d.transpose(1, 2) @ d)[2][:, 2]
    trial = torch.cat([n64, cen], -1).float()
    keep = (inl(trial).sum(1) >= inl(cur).sum(1)).unsqueeze(-1)
    cur = torch.where(keep, trial, cur)
    return cur, inl(cur)


def main():
    res = []
    cfg = NetConfig()
    for clouds, n, planes in SHAPES:
        eng = Engine(cfg, 0, max_points=n, max_pairs=1)             # the scratch is 20 B per row and 32 B per hypothesis: any batch here fits
        host = np.stack([scene(n, 31 + c) for c in range(clouds)])
        pts = torch.from_numpy(host).cuda()
        kw = dict(hypotheses=H, max_planes=planes, refine_iters=1, seed=0)
        out = eng.segment_plane(pts, THR, **kw)
        eng.use_torch_stream(True)                                 # stream-ordered: the events bracket the launches, no host sync inside
        bufs = [torch.empty_like(t) for t in out]

        def raw(hyp=H):
            rc = eng.lib.dsir_segment_plane(eng.h, pts.data_ptr(), 3, None, None, clouds, n, THR, hyp, planes, 3, 1, 0.0, 0.0, 0.0, 0.0, 0,
                                            *[t.data_ptr() for t in bufs])
            assert rc == 0, eng.lib.dsir_last_error(eng.h)

        rows = torch.from_numpy(np.stack([P.draw_rows(0, c, 0, np.arange(H), n) for c in range(clouds)])).cuda()
        loop = lambda: torch_round(pts, rows, THR)
        for _ in range(3):
            raw(), raw(1)
        loop()
        torch.cuda.synchronize()
        call, one, torch_us = [], [], []
        for _ in range(5):                                         # alternating: drift hits every variant alike
            call.append(timed(raw, 20))
            one.append(timed(lambda: raw(1), 20))
            if planes == 1:
                torch_us.append(timed(loop, 1))
        raw()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(bufs, out))
        eng.use_torch_stream(False)
        r = {"what": "segment_plane", "clouds": clouds, "points": n, "hypotheses": H, "max_planes": planes, "call_us": call,
             "one_hypothesis_call_us": one, "scoring_us_by_difference": round(float(np.median(call) - np.median(one)), 1),
             "num_planes": out[1].tolist()[:4], "plane_counts": out[4][0].tolist()}
        if planes == 1:
            cur, lab = loop()
            dev = out[2][:, 0, :3].double()
            r["torch_loop_us"] = torch_us
            r["ratio_torch_over_call"] = round(float(np.median(torch_us) / np.median(call)), 1)
            r["torch_normal_max_angle"] = float(torch.linalg.cross(cur[:, :3].double(), dev).norm(dim=1).max())
            r["torch_labels_equal"] = round(float((lab == (out[0] == 0)).float().mean()), 6)
        print(json.dumps(r), flush=True)
        res.append(r)
        eng.close()
    if "--out" in sys.argv:
        fn = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(fn)), exist_ok=True)
        json.dump(res, open(fn, "w"), indent=1)


if __name__ == "__main__":
    main()
