"""Training `align` with the loss's pose-error term on (wt_pose_loss = 0.5): the reference's loop on the drop-in ``Network``, the
one-call step, and the hipGraph-replayed step.  2 pairs x 1024 points, 2 iterations, seeded weights (the shape of
tests/test_train_loop.py's second test)."""
import numpy as np
import pytest
import torch

from test_train_loop import _args

pytestmark = pytest.mark.gpu

N, P, N_ITER, WT, SEED, LR = 1024, 2, 2, 0.5, 5, 1e-3


def _dev():
    return torch.device("cuda", 0)


def _net(wt):
    from deepsir_amd.model import Network
    from deepsir_amd.weights import generate_state_dict, to_torch_state_dict
    net = Network(_args("align", num_reg_iter=N_ITER, wt_pose_loss=wt))
    net.load_state_dict(to_torch_state_dict(generate_state_dict(net.cfg, 8, "separated")))
    net.to(_dev())
    net.train()
    return net


def _data():
    from deepsir_amd.synth import make_pair
    raws = [make_pair(N, 800 + b, 3) for b in range(P)]
    d = {k: torch.from_numpy(np.concatenate([r[k] for r in raws])).to(_dev()) for k in ("points_src", "points_ref")}
    d["transform_gt"] = torch.from_numpy(np.concatenate([r["transform_gt"] for r in raws]).astype(np.float32)).to(_dev())
    return d


def _loop(net, data):
    """The body of the reference's loop (train.py:396-446) up to the optimiser step: (loss dict, gradients by name)."""
    net.dropout_masks = net._seeded_masks(SEED, P, N, N, _dev(), N_ITER)       # the draw ``train_step(dropout_seed=SEED)`` makes
    for p in net.parameters():
        p.grad = None
    pred_transforms, endpoints = net(data, (N_ITER, True))
    endpoints['transform_gt'] = data['transform_gt']
    endpoints['transform_pred'] = pred_transforms
    losses = net.loss_align_fun(endpoints, reduction='mean')
    losses['total'].backward()
    assert not endpoints['invalid_gradient']
    return losses, {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def test_reference_loop_and_the_one_call_step():
    data = _data()
    net = _net(WT)
    optimizer = torch.optim.Adam(net.parameters(), lr=LR)
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    losses, grads = _loop(net, data)
    keys = {f"{t}_{i}" for t in ("mae", "poseError") for i in range(N_ITER)}      # no match list, no radius: no confidence term
    assert set(losses) == keys | {"total"}
    want = sum(0.5 ** (N_ITER - 1 - int(k[k.rfind("_") + 1:])) * float(losses[k]) for k in keys)
    assert abs(losses["total"].item() - want) <= 1e-6 * max(1.0, abs(want)), (losses["total"].item(), want)
    assert all(float(losses[f"poseError_{i}"]) > 0 for i in range(N_ITER))
    inlier = [k for k, p in net.named_parameters() if k.startswith("inlier_model.") and p.requires_grad]
    assert set(grads) == set(inlier) and len(grads) > 150
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    # the term reaches the parameters: the same loop with weight 0 leaves other gradients
    off_losses, off = _loop(_net(0.0), data)
    assert set(off_losses) == {f"mae_{i}" for i in range(N_ITER)} | {"total"}
    assert all(float(off_losses[f"mae_{i}"]) == float(losses[f"mae_{i}"]) for i in range(N_ITER))
    differ = [k for k in grads if not torch.equal(grads[k], off[k])]
    assert len(differ) > len(grads) // 2, len(differ)
    # validation's reduction: per-pair values whose mean is the batch value
    net.eval()
    with torch.no_grad():
        pred_transforms, ep = net(data, (N_ITER, True))
        ep['transform_gt'], ep['transform_pred'] = data['transform_gt'], pred_transforms
        val, mean = net.loss_align_fun(ep, reduction='none'), net.loss_align_fun(ep, reduction='mean')
    assert set(val) == set(mean) == keys | {"total"}
    for k in val:
        assert val[k].shape == (P,) and abs(val[k].mean().item() - mean[k].item()) < 1e-5, k
    net.train()
    optimizer.step()

    # ---- the one-call step on a second network with the same weights: the same kernels in the same order
    one = _net(WT)
    out = one.train_step(data, (N_ITER, True), lr=LR, dropout_seed=SEED)           # reads args.wt_pose_loss
    assert not out["skipped"]
    assert np.float32(out["losses"]["total"]) == np.float32(losses["total"].item()), (out["losses"]["total"], losses["total"].item())
    assert all(np.float32(out["losses"][k]) == np.float32(losses[k].item()) for k in keys)
    got = one._tstate.main.grad_dict()
    for k, g in grads.items():
        assert np.array_equal(got[k] if k in got else got[k[len("inlier_model."):]], g.cpu().numpy()), k
    # torch's Adam (the loop) against the device's (the step): the bounds of test_train.py::test_device_adam_steps_match_reference
    # for one step - an entry whose gradient is rounding noise may move by lr in either direction, the bulk is tight
    worst, meds = 0.0, []
    after_loop, after_one = dict(net.named_parameters()), dict(one.named_parameters())
    for k in grads:
        err = (after_loop[k].detach() - after_one[k].detach()).abs()
        worst = max(worst, float(err.max()))
        meds.append(float(err.median()))
        assert float(err.max()) <= 2 * 1 * LR * 1.05 and float(err.median()) <= 2e-4, k
        assert not torch.equal(after_one[k].detach(), before[k])
    print(f"[pose-train] loop vs one-call step after one Adam step: max {worst:.2e}, worst median {max(meds):.2e}")
    # the explicit argument overrides args; the weight is part of the call
    out0 = _net(WT).train_step(data, (N_ITER, True), lr=LR, dropout_seed=SEED, wt_pose_loss=0.0)
    assert not any(k.startswith("poseError_") for k in out0["losses"])
    torch.cuda.synchronize()


def test_graph_replayed_step_carries_the_weight():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    from deepsir_amd.train import AlignTrainStep, RandlaTrainer, train_step_align
    from deepsir_amd.weights import generate_state_dict
    cfg = NetConfig(feat_len=3)
    sd = generate_state_dict(cfg, 6, "plain")
    eng = Engine(cfg, max_points=N, max_pairs=P)
    eng.load_state_dict(sd)
    data = _data()
    src, ref, gt = data["points_src"], data["points_ref"], data["transform_gt"]
    sx, sn, ss, si = eng.knn_pyramid(src)
    res = eng.register(src, ref, n_iter=N_ITER)
    batch = {"points_src": src, "points_ref": ref, "src_xyz": sx, "src_neigh": sn, "src_sub": ss, "src_interp": si}
    mk = lambda: RandlaTrainer(cfg, sd, "inlier_model", 6, 1, _dev())
    a, b = mk(), mk()
    stepper = AlignTrainStep(eng, b, P, N, N, N_ITER, dropout=True, wt_pose_loss=WT)
    for s in range(4):          # eager, capture + replay, replay, replay
        oa = train_step_align(eng, a, batch, res, gt, lr=LR, dropout_seed=40 + s, wt_pose_loss=WT)
        ob = stepper.step(batch, res, gt, lr=LR, dropout_seed=40 + s)
        assert oa["losses"] == ob["losses"], (s, oa["losses"], ob["losses"])
        assert f"poseError_{N_ITER - 1}" in ob["losses"]
        assert torch.equal(oa["grad_logits"], ob["grad_logits"]) and torch.equal(a.flat_g, b.flat_g), s
        assert torch.equal(a.flat_p, b.flat_p), s
    assert stepper.gf is not None and stepper.gb is not None
    # the same object asked for another weight raises: it never steps with a scalar it was not built for
    p_before = b.flat_p.clone()
    for other in (0.0, 1.0):
        with pytest.raises(ValueError, match="wt_pose_loss"):
            stepper.step(batch, res, gt, lr=LR, dropout_seed=50, loss_kwargs={"wt_pose_loss": other})
    assert torch.equal(b.flat_p, p_before)
    assert stepper.step(batch, res, gt, lr=LR, dropout_seed=50, loss_kwargs={"wt_pose_loss": WT})["losses"]["total"] > 0
    torch.cuda.synchronize()
    eng.close()
