"""Register P synthetic pairs of J src and K ref points and dump, to an .npz, everything the descriptor search decides and everything
that depends on it: used by tests/test_gpu_search_sites.py to compare processes that differ only in the search mode (the environment
switches are read once per process), and to compare two builds of the library.

    search_sites_dump.py OUT PAIRS J K ITERS [GRAPH]      GRAPH: 1 = register through a captured hipGraph and record its node census

Also fed back: each iteration's descriptors through the stand-alone entry points (dsir_nn_match, dsir_nn_match_screened)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
import numpy as np
import torch
import deepsir_amd  # noqa: F401
from deepsir_amd.arch import NetConfig
from deepsir_amd.engine import Engine
from deepsir_amd.synth import make_batch
from deepsir_amd.weights import generate_state_dict, to_torch_state_dict


def run(out, P, J, K, iters, graph=False):
    cfg = NetConfig(feat_len=3)
    eng = Engine(cfg, 0, max_points=max(J, K, 1024), max_pairs=P)
    eng.load_state_dict(to_torch_state_dict(generate_state_dict(cfg, 3)))
    b = make_batch(max(J, K), list(range(700, 700 + P)), 3)
    src = torch.from_numpy(np.ascontiguousarray(b["points_src"][:, :J])).cuda()
    ref = torch.from_numpy(np.ascontiguousarray(b["points_ref"][:, :K])).cuda()
    census = dict(nodes=-1, kernels=-1, memsets=-1, memcpys=-1)
    if graph:
        eng.enable_graph(True)
    o = eng.register(src, ref, iters, want_desc=True)
    if graph:
        census = eng.graph_stats()
        o = eng.register(src, ref, iters, want_desc=True, out=o)      # a replay of the captured registration
    st = eng.screen_stats()
    kept, total = eng.prune_stats()
    o = {k: v.cpu().numpy() for k, v in o.items() if torch.is_tensor(v)}      # "_keep" holds the call's staging buffers
    eng.enable_graph(False)
    ref_d = torch.from_numpy(o["desc_ref"]).cuda()
    idx_nn = np.stack([eng.nn_match(torch.from_numpy(o["desc_src"][i]).cuda(), ref_d).cpu().numpy() for i in range(iters)])
    idx_sc = np.stack([eng.nn_match_screened(torch.from_numpy(o["desc_src"][i]).cuda(), ref_d)[0].cpu().numpy() for i in range(iters)])
    eng.close()
    np.savez(out, idx_nn_match=idx_nn, idx_nn_match_screened=idx_sc, tiles_unpruned=np.int64(total), tiles_visited=np.int64(kept),
             census=np.array([census[k] for k in ("nodes", "kernels", "memsets", "memcpys")], np.int64),
             **{k: np.int64(v) for k, v in st.items()}, **o)


if __name__ == "__main__":
    a = sys.argv
    run(a[1], int(a[2]), int(a[3]), int(a[4]), int(a[5]), len(a) > 6 and a[6] == "1")
