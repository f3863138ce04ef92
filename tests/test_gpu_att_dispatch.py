"""Attentive pooling outside the tuned widths.

Sched::att serves d = 16, 64 and 128 in att_pool.hip and d = 256 in pw_tile.hip; every other width takes the general EPI_ATT kernel
of pw_gemm.hip, which no default-architecture test reaches.  One forward parity case at d_out = [32, 64, 128, 256] puts that kernel
under level 0 of both networks; the other levels keep their usual kernels.  Tolerances: those of the default-architecture forward
parity case, test_gpu_parity.test_stages_vs_oracle_and_golden (features and logits 2e-4, inlier logits 5e-4, values of O(1)).
"""
import numpy as np
import pytest
import torch

from test_gpu_parity import cu, engine_for

pytestmark = pytest.mark.gpu


def test_forward_parity_with_a_level_on_the_general_att_kernel():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.synth import make_pair
    from deepsir_amd.weights import generate_state_dict
    from oracle.knn import add_pyramids
    from oracle.network import OracleNet, to_torch

    torch.set_num_threads(1)
    n = 1024                                   # 1024 -> 256 -> 64 -> 16: the deepest searched level keeps 16 points
    cfg = NetConfig(feat_len=3, d_out=(32, 64, 128, 256), sub_sampling_ratio=(4, 4, 4, 4))
    sd = generate_state_dict(cfg, 7)
    data = add_pyramids(make_pair(n, 31, 3), cfg.num_knn, cfg.sub_sampling_ratio)
    d = to_torch(data)
    net = OracleNet(cfg, sd)
    eng = engine_for(cfg, sd, "att_dispatch_d32", max_points=1024, max_pairs=1)
    pyr = [cu(data["points_src_xyz"]), cu(data["points_src_neigh_idx"], torch.int32), cu(data["points_src_sub_idx"], torch.int32),
           cu(data["points_src_interp_idx"], torch.int32)]
    ref = [d["points_src_xyz"], d["points_src_neigh_idx"], d["points_src_sub_idx"], d["points_src_interp_idx"]]

    feat, logits = eng.randla_forward("feat_extractor", cu(data["points_src"]), *pyr)
    f_ref, _, lg_ref = net.randla("feat_extractor", d["points_src"], *ref)
    np.testing.assert_allclose(feat[0].cpu().numpy().T, f_ref[0].numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(logits[0].cpu().numpy().T, lg_ref[0].numpy(), rtol=2e-4, atol=2e-4)

    # the inlier model's rows: [src xyz ; matched ref xyz], here under a fixed permutation of the ref points
    perm = np.random.default_rng(5).permutation(n)
    cat = np.concatenate([data["points_src_xyz"][0, :n], data["points_ref_xyz"][0, :n][perm]], 1)[None].astype(np.float32)
    _, lg_in = eng.randla_forward("inlier_model", cu(cat), *pyr)
    _, _, lg_in_ref = net.randla("inlier_model", torch.from_numpy(cat), *ref)
    np.testing.assert_allclose(lg_in[0, :, 0].cpu().numpy(), lg_in_ref[0, 0].numpy(), rtol=5e-4, atol=5e-4)
