"""Every output of the pose kernels (csrc/kabsch.hip, icp.hip, align_loss.hip) on seeded inputs, dumped to an .npz: two runs that
differ only in the library (DSIR_LIB) or in an environment switch (DSIR_KABSCH_STREAM, read once per process) are compared array by
array, bit by bit (tests/test_gpu_parity.py::test_kabsch_kernels_agree_at_their_size_boundaries).

    pose_dump.py OUT.npz [kabsch]          kabsch: the Engine.kabsch cases alone

Engine.kabsch at the size boundaries of the three one-workgroup kernels (1024-thread trips, 5 x 1024 and 8 x 1024 register-resident
points) and, with the threshold of the chunked solve at 4096, at 1 .. 4 chunks with a ragged last one; Engine.icp_refine with a pair
that converges at once (the frozen-pair step of every kernel, src moved in place); Engine.align_loss_backward on the golden cases."""
import os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepsir_amd.arch import NetConfig
from deepsir_amd.engine import Engine

KABSCH_SIZES = (1, 2, 63, 1024, 1025, 5120, 5121, 8192, 8193)
CHUNKED_SIZES = (4096, 4097, 8193, 12289)      # threshold 4096: 1, 2, 3, 4 chunks of 4096 points


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rot(ang):
    cx, cy, cz = np.cos(ang); sx, sy, sz = np.sin(ang)
    return np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx], [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
                     [-sy, cy * sx, cy * cx]])


def kabsch_case(m, P=3):
    """P = 3 pairs of m matched points: pair 1 with a third of its weights zero, pair 2 with one NaN coordinate"""
    rng = np.random.Generator(np.random.Philox(key=1000 + m))
    src = rng.uniform(-2, 2, (P, m, 3)).astype(np.float32)
    tgt = np.empty_like(src)
    for p in range(P):
        tgt[p] = (src[p].astype(np.float64) @ rot(rng.uniform(-0.5, 0.5, 3)).T + rng.uniform(-1, 1, 3)).astype(np.float32)
    tgt += rng.normal(0, 0.01, tgt.shape).astype(np.float32)
    w = rng.uniform(0, 1, (P, m)).astype(np.float32)
    w[1, : m // 3] = 0.0
    src[2, m // 2, 1] = np.nan
    return src, tgt, w


def icp_case(n, P=2):
    """pair 0 moves by a small rigid motion; pair 1 is its own target: it converges at the first check"""
    rng = np.random.Generator(np.random.Philox(key=2000 + n))
    src = rng.uniform(-2, 2, (P, n, 3)).astype(np.float32)
    ref = src.copy()
    ref[0] = (src[0].astype(np.float64) @ rot(np.array([0.02, -0.015, 0.01])).T + np.array([0.02, -0.01, 0.015])).astype(np.float32)
    ref[0] = ref[0][rng.permutation(n)]
    T0 = np.tile(np.eye(4, dtype=np.float32)[:3], (P, 1, 1))
    return src, ref, T0


def kabsch_outputs(eng):
    """T and invalid of every Engine.kabsch case: kabsch_m* by the one-workgroup kernels, chunked_m* by the chunked solve"""
    res = {}
    for m in KABSCH_SIZES:
        T, bad = eng.kabsch(*map(cu, kabsch_case(m)))
        res[f"kabsch_m{m}_T"], res[f"kabsch_m{m}_invalid"] = T.cpu().numpy(), bad.cpu().numpy()
    eng.set_kabsch_chunked_min(4096)
    try:
        for m in CHUNKED_SIZES:
            T, bad = eng.kabsch(*map(cu, kabsch_case(m)))
            res[f"chunked_m{m}_T"], res[f"chunked_m{m}_invalid"] = T.cpu().numpy(), bad.cpu().numpy()
    finally:
        eng.set_kabsch_chunked_min(0)
    return res


def main(out, only_kabsch):
    eng = Engine(NetConfig(), 0, max_points=16384, max_pairs=4)
    res = kabsch_outputs(eng)
    if not only_kabsch:
        for n in (1500, 6000, 9000):
            T, st = eng.icp_refine(*map(cu, icp_case(n)), 0.3, max_iter=5)
            res[f"icp_n{n}_T"], res[f"icp_n{n}_stats"] = T.cpu().numpy(), st.cpu().numpy()
        g = np.load(os.path.join(ROOT, "tests", "golden", "align_loss_cases.npz"))
        for c in range(int(g["n_cases"])):
            d = {k[len(f"c{c}_"):]: g[k] for k in g.files if k.startswith(f"c{c}_")}
            o = eng.align_loss_backward(cu(d["src"]), cu(d["ref"]), cu(d["idx"].astype(np.int32)), cu(d["logits"]), cu(d["labels"]), cu(d["gt"]),
                                        loss_type=str(d["loss_type"]))
            names = sorted(o["losses"])
            res[f"align{c}_losses"] = np.array([o["losses"][k] for k in names], np.float64)
            res[f"align{c}_grad_logits"], res[f"align{c}_transforms"] = o["grad_logits"].cpu().numpy(), o["transforms"].cpu().numpy()
    eng.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], len(sys.argv) > 2 and sys.argv[2] == "kabsch")
