"""The CPU oracle run in float64 (``OracleNet(..., dtype=torch.float64)``) is the same function as the fp32 oracle the imported
reference's vectors pin: against tests/golden/train_cases.npz it meets the tolerances the fp32 oracle meets
(tests/test_train.py).  The GPU tests at the reference's training scale (tests/test_gpu_train_scale.py) measure the HIP
training path against this fp64 oracle."""
import numpy as np
import pytest
import torch

from oracle.network import OracleNet, to_torch
from oracle import train as otrain
from test_train import CFG, GOLD, _align_case, _case, _check_align_grads, _check_feat_grads, _check_grads, _feat_case

F64 = torch.float64


@pytest.mark.parametrize("c", range(int(GOLD["n_cases"])))
def test_fp64_oracle_training_pass_matches_reference_autograd(c):
    meta, d, sd, keep = _case(c)
    net = OracleNet(CFG, sd, F64)
    params = otrain.trainable(net)
    assert len(params) > 100 and all(v.dtype == F64 for v in params.values())
    t = to_torch(d, F64)
    logits = otrain.randla_train(net, "inlier_model", t["cat"], t["points_src_xyz"], t["points_src_neigh_idx"], t["points_src_sub_idx"],
                                 t["points_src_interp_idx"], torch.from_numpy(keep))
    assert logits.dtype == F64
    assert np.abs(logits.detach().numpy() - GOLD[f"c{c}_logits"]).max() < 2e-5
    (logits * t["G"]).sum().backward()
    _check_grads(c, {k: v.grad.numpy() for k, v in params.items()}, meta["seed"], 2e-4)
    for k in GOLD.files:
        if k.startswith(f"c{c}_buf_"):
            assert np.allclose(net.p[k[len(f"c{c}_buf_"):]].numpy(), GOLD[k], rtol=1e-5, atol=1e-6), k


def test_fp64_oracle_feat_pipeline_matches_reference_autograd():
    meta, cfg, sd, t = _feat_case()
    net = OracleNet(cfg, sd, F64)
    params = {k: v.requires_grad_(True) for k, v in net.p.items()
              if k.startswith(("mlp_feat", "mlp_att", "mlp_proj")) and v.is_floating_point() and not k.endswith(("running_mean", "running_var"))}
    assert len(params) == 30
    t = {k: v.to(F64) for k, v in t.items()}
    d_src = otrain.aggregate_train(net, t["xyz_src"], t["feat_src"], t["score_src"])
    d_ref = otrain.aggregate_train(net, t["xyz_ref"], t["feat_ref"], t["score_ref"])
    assert d_src.dtype == F64
    assert np.abs(d_src.detach().numpy() - GOLD["feat_desc_src"]).max() < 1e-5
    assert np.abs(d_ref.detach().numpy() - GOLD["feat_desc_ref"]).max() < 1e-5
    loss, acc = otrain.det_des_loss(d_src, d_ref, t["xyz_src"], t["xyz_ref"], t["score_ref"], torch.from_numpy(GOLD["feat_transform_gt"]).to(F64),
                                    meta["thres_radius"], meta["det_loss_weight"])
    assert loss.dtype == F64
    assert abs(float(loss) - GOLD["feat_loss_acc"][0]) < 1e-5 and abs(float(acc) - GOLD["feat_loss_acc"][1]) < 1e-3
    loss.backward()
    _check_feat_grads({k: v.grad.numpy() for k, v in params.items()}, 1e-3)
    for k in GOLD.files:
        if k.startswith("feat_buf_"):
            assert np.allclose(net.p[k[len("feat_buf_"):]].numpy(), GOLD[k], rtol=1e-5, atol=1e-6), k


def test_fp64_oracle_whole_network_training_forward_matches_reference():
    from oracle import align_loss as oal
    meta, cfg, sd, d, masks = _align_case()
    net = OracleNet(cfg, sd, F64)
    params = otrain.trainable(net)
    t = to_torch(d, F64)
    tm = {"fe_src": torch.from_numpy(masks["fe_src"]), "fe_ref": torch.from_numpy(masks["fe_ref"]),
          "inlier": [torch.from_numpy(m) for m in masks["inlier"]]}
    T, idx, lg = otrain.register_train(net, t, meta["n_iter"], tm)
    assert T[0].dtype == F64 and lg[0].dtype == F64
    assert np.array_equal(torch.stack(idx).numpy(), GOLD["align_idx"].astype(np.int64))
    assert np.abs(torch.stack(lg).detach().numpy() - GOLD["align_logits"]).max() < 5e-5
    assert np.abs(torch.stack(T, 1).detach().numpy() - GOLD["align_transforms"]).max() < 1e-5
    loss = oal.scan_alignment_loss(t["points_src"][:, :, :3], T, t["transform_gt"], lg, None)["total"]
    assert abs(float(loss.detach()) - float(GOLD["align_loss"])) < 1e-5
    loss.backward()
    _check_align_grads({k: v.grad.numpy() for k, v in params.items()}, 1e-3, 1e-8)
    for k in [k for k in GOLD.files if k.startswith("align_buf_")]:
        assert np.allclose(net.p[k[len("align_buf_"):]].numpy(), GOLD[k], rtol=1e-4, atol=1e-6), k
