"""Register the cases of tests/test_gpu_att_enc2.py in ONE process and dump every result to an .npz: the test compares two processes
that differ only in DSIR_NO_ATT_ENC2 / DSIR_ATT_ENC2_MIN_BLOCKS (lfa.mlp2 of level 0 from the first pooling launch, or as a launch of
its own; the switches are read once per process).

    att_enc2_dump.py OUT"""
import os, sys
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepsir_amd.arch import NetConfig
from deepsir_amd.engine import Engine
from deepsir_amd.synth import make_batch
from deepsir_amd.weights import generate_state_dict, to_torch_state_dict

POINTS, PAIRS, ITERS, FEAT_LEN = (1024, 1027, 1100), (1, 3), (1, 3), (3, 4)
KEYS = ("transforms", "idx", "logits", "desc_src", "desc_ref")

if __name__ == "__main__":
    res = {}
    for fl in FEAT_LEN:
        cfg = NetConfig(feat_len=fl)
        eng = Engine(cfg, 0, max_points=max(POINTS), max_pairs=max(PAIRS))
        eng.load_state_dict(to_torch_state_dict(generate_state_dict(cfg, 3)))
        for n in POINTS:
            b = make_batch(n, list(range(700, 700 + max(PAIRS))), fl)
            for P in PAIRS:
                src, ref = torch.from_numpy(b["points_src"][:P]).cuda(), torch.from_numpy(b["points_ref"][:P]).cuda()
                for it in ITERS:
                    o = eng.register(src, ref, it, want_aux=True, want_desc=True)
                    for k in KEYS:
                        res[f"{fl}_{n}_{P}_{it}_{k}"] = o[k].cpu().numpy()
        if fl == 3:
            # which schedule ran: the kernel nodes of one captured registration (1 pair, 1027 points, 3 iterations)
            b = make_batch(1027, [700], fl)
            eng.enable_graph(True)
            eng.register(torch.from_numpy(b["points_src"]).cuda(), torch.from_numpy(b["points_ref"]).cuda(), 3)
            res["census_kernels"] = np.int64(eng.graph_stats()["kernels"])
            eng.enable_graph(False)
        eng.close()
    np.savez(sys.argv[1], **res)
