"""Register the whole-path case of tests/test_gpu_feat_chain.py and dump the results to an .npz: the test compares child processes
that differ only in DSIR_NO_FEAT_CHAIN / DSIR_FEAT_CHAIN_MIN_BLOCKS (mlp_feat in one launch, csrc/feat_chain.hip, or as three point-wise
launches; the switches are read once per process).

    feat_chain_dump.py OUT"""
import os, sys
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepsir_amd.arch import NetConfig
from deepsir_amd.engine import Engine
from deepsir_amd.synth import make_batch
from deepsir_amd.weights import generate_state_dict, to_torch_state_dict

PAIRS, POINTS, ITERS = 2, 257, 2
KEYS = ("transforms", "idx", "desc_src", "desc_ref")
# the default pyramid (a quarter of the points per level) takes no cloud under 1024 points: 257 points keep 16 at the deepest level
# with half of the points per level
RATIOS = (2, 2, 2, 2)


def run_case():
    cfg = NetConfig(feat_len=3, sub_sampling_ratio=RATIOS)
    eng = Engine(cfg, 0, max_points=1024, max_pairs=PAIRS)
    eng.load_state_dict(to_torch_state_dict(generate_state_dict(cfg, 3)))
    b = make_batch(POINTS, [700, 701], 3)
    src, ref = torch.from_numpy(b["points_src"]).cuda(), torch.from_numpy(b["points_ref"]).cuda()
    o = eng.register(src, ref, ITERS, want_aux=True, want_desc=True)
    res = {k: o[k].cpu().numpy() for k in KEYS}
    # which schedule ran: the kernel nodes of the same registration, captured
    eng.enable_graph(True)
    eng.register(src, ref, ITERS)
    res["census_kernels"] = np.int64(eng.graph_stats()["kernels"])
    eng.enable_graph(False)
    eng.close()
    return res


if __name__ == "__main__":
    np.savez(sys.argv[1], **run_case())
