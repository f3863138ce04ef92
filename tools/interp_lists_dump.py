"""The clouds on which interp_idx read off the 16-NN lists (csrc/knn.hip, interp_lists_kernel) is pinned against the searches it replaces,
and one process's answers for them:

    interp_lists_dump.py OUT.npz      Engine.knn_pyramid of every case of cases() (xyz, neigh, sub, interp per case) and the transforms
                                      of one registration of 2 pairs x 1100 points x 2 iterations

tests/test_gpu_interp_lists.py runs it as a child process with DSIR_NO_INTERP_LISTS set (the switch is read once per process) and
compares with its own process; tests/test_interp_lists_host.py states the rule in numpy on the same clouds."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
import numpy as np


def random_clouds(n, seeds, **kw):
    from deepsir_amd.synth import make_pair
    out = []
    for s in seeds:
        pr = make_pair(n, s, 3, **kw)
        out += [pr["points_src"][0, :, :3], pr["points_ref"][0, :, :3]]
    return np.ascontiguousarray(np.stack(out), np.float32)


def sorted_clouds(clouds=2, n=1100):
    """Sorted along x: every level's prefix is one slab, most queries have no neighbour in it."""
    c = random_clouds(n, range(40, 40 + (clouds + 1) // 2))[:clouds]
    return np.ascontiguousarray(np.stack([p[np.argsort(p[:, 0], kind="stable")] for p in c]))


def duplicate_cloud(n=1100, seed=7):
    """An 8 x 8 x 8 lattice of quarter units, every lattice point twice (ties at d2 = 0) and equal positive d2 all over (exact in fp32),
    plus n - 1024 lattice points a third time, in a random order: the copies of a point fall on both sides of every prefix boundary."""
    rng = np.random.Generator(np.random.Philox(key=seed))
    g = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.25
    p = np.concatenate([g, g, g[rng.choice(512, n - 1024, replace=False)]])
    return np.ascontiguousarray(p[rng.permutation(n)][None], np.float32)


def nonfinite_cloud(n=1100):
    """A few rows with a NaN or an infinity, inside and outside every level's prefix (index 3 is a point of every level and of every
    support set)."""
    p = random_clouds(n, [55])[:1].copy()
    p[0, 3, 0] = np.nan
    p[0, 40, 1] = np.inf
    p[0, 100, 2] = -np.inf
    p[0, 300] = np.nan
    p[0, 1099, 0] = np.inf
    return p


def cases():
    """name -> (points [clouds, n, 3] fp32, compared with oracle.knn too)"""
    return {
        "r1027": (random_clouds(1027, [11, 12])[:3], True),      # 1027 / 256 / 64 / 16: grid at level 0, both brute-force kinds, the floor
        "r4224": (random_clouds(4224, range(20, 28)), True),      # 16 x 4224 >= 65536: the launch size of the parent's grid_nn1_kernel
        "r5000": (random_clouds(5000, [31]), True),
        "sorted1100": (sorted_clouds(), True),
        "dups1100": (duplicate_cloud(), True),
        "nonfinite1100": (nonfinite_cloud(), False),              # expected: whatever the searches give
    }


def run(out):
    import torch
    import deepsir_amd  # noqa: F401
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    from deepsir_amd.synth import make_batch
    from deepsir_amd.weights import generate_state_dict, to_torch_state_dict

    cfg = NetConfig(feat_len=3)
    eng = Engine(cfg, 0, max_points=5000, max_pairs=8)
    eng.load_state_dict(to_torch_state_dict(generate_state_dict(cfg, 3)))
    res = {}
    for name, (pts, _) in cases().items():
        got = eng.knn_pyramid(torch.from_numpy(pts).cuda())
        for k, v in zip(("xyz", "neigh", "sub", "interp"), got):
            res[f"{name}.{k}"] = v.cpu().numpy()
    b = make_batch(1100, [700, 701], 3)
    o = eng.register(torch.from_numpy(b["points_src"]).cuda(), torch.from_numpy(b["points_ref"]).cuda(), 2)
    res["transforms"] = o["transforms"].cpu().numpy()
    eng.close()
    np.savez(out, **res)


if __name__ == "__main__":
    run(sys.argv[1])
