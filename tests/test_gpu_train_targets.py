"""The confidence term's targets are made on the device, and training is unchanged by it.

``Network.train_step`` (both ``frozen_mode``s) and ``ScanAlignmentLoss`` used to call ``train.find_correct_correspondence`` - idx to the
host, ``np.isin`` per pair and iteration, labels back up.  They now take the targets from ``train.inlier_targets`` (HIP,
csrc/match_targets.hip).  The targets are exact 0 / 1 values, so every loss, gradient and weight must be BYTE-identical to the same
steps driven with the host function's labels, which go in through the entry points that always took device labels:
``train_step_align_full(labels_fn=)`` and ``AlignTrainStep.step(labels=)``.

Sizes and fixtures are those of tests/test_gpu_train_interleave.py (one pair of 1024 points, 2 iterations)."""
import numpy as np
import pytest
import torch

from test_gpu_train_interleave import N_ITER, _case, _dev, _forward, _grads, _net, _params, _zero

pytestmark = pytest.mark.gpu

RADIUS = 0.2


def _host_labels(c, idx, J):
    from deepsir_amd.train import find_correct_correspondence
    return torch.from_numpy(find_correct_correspondence(c["matches"], idx, J)).to(_dev())


_STEPPERS = {}


def _host_step(net, c, seed, frozen_mode):
    """One ``Network.train_step`` of the align pipeline as the parent commit composed it, labels from the host function."""
    from deepsir_amd import train as T
    data = c["data"]
    src, ref = data["points_src"].float(), data["points_ref"].float()
    B, J, _ = src.shape
    K = ref.shape[1]
    dev = src.device
    eng = net._ensure_engine(max(J, K), B)
    st = net._training_state(dev)
    tr = st.main
    batch = net._pyramids(eng, data, src, ref)
    gt = data["transform_gt"].float().to(dev)
    if frozen_mode == "train":
        fe, ag = st.frozen
        out = T.train_step_align_full(eng, tr, fe, ag, batch, gt, N_ITER, lambda idx: _host_labels(c, idx, J), 1e-3,
                                      net._seeded_masks(seed, B, J, K, dev, N_ITER), None)
    else:
        res = eng.register(src, ref, N_ITER)
        if id(net) not in _STEPPERS:
            _STEPPERS[id(net)] = (net, T.AlignTrainStep(eng, tr, B, J, K, N_ITER))
        out = _STEPPERS[id(net)][1].step(batch, res, gt, _host_labels(c, res["idx"], J), 1e-3, seed, None)
    net._dirty = net._pool_dirty = net._server_dirty = True
    assert not out["skipped"]
    return out["losses"]


def _assert_same_training(a, b, what):
    ga, gb = a._tstate.main.grad_dict(), b._tstate.main.grad_dict()
    assert set(ga) == set(gb) and any(float(abs(v).max()) > 0 for v in ga.values())
    bad = [k for k in ga if not np.array_equal(ga[k], gb[k])]
    assert not bad, f"{what}: {len(bad)} of {len(ga)} gradients differ (first {bad[0]})"
    sa, sb = a.state_dict(), b.state_dict()
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, f"{what}: {len(bad)} of {len(sa)} state_dict tensors differ (first {bad[0]})"


@pytest.mark.parametrize("frozen_mode", ["train", "eval"])
def test_train_step_with_matches_equals_the_host_labelled_step(frozen_mode):
    a, b = _net("align"), _net("align")
    c = _case("align", "A")
    before = {k: p.detach().clone() for k, p in _params(a).items()}
    for seed in (3, 4):
        out = a.train_step({**c["data"], "matches": c["matches"]}, (N_ITER, False), dropout_seed=seed, frozen_mode=frozen_mode)
        want = _host_step(b, c, seed, frozen_mode)
        assert not out["skipped"]
        assert out["losses"] == want, f"{frozen_mode}, seed {seed}: {out['losses']} != {want}"
        assert any(k.startswith("outlier_") for k in want)                 # the confidence term is in
    _assert_same_training(a, b, frozen_mode)
    assert all(not torch.equal(p.detach(), before[k]) for k, p in _params(a).items())
    torch.cuda.synchronize()


def _radius_lists(net, c):
    from deepsir_amd.train import as_reference_matches
    d = c["data"]
    J = d["points_src"].shape[1]
    eng = net._ensure_engine(J, 1)
    lists = as_reference_matches(*eng.radius_matches(d["points_src"].float(), d["points_ref"].float(), d["transform_gt"].float(), RADIUS), 1, J)
    assert len(lists[0]) >= J                                              # rigid copies: every source point has its partner
    return lists


@pytest.mark.parametrize("frozen_mode", ["train", "eval"])
def test_train_step_with_match_radius_equals_the_step_with_radius_matches(frozen_mode):
    a, b = _net("align"), _net("align")
    c = _case("align", "A")
    lists = _radius_lists(b, c)
    for seed in (3, 4):
        data = {**c["data"], "match_radius": RADIUS} if seed == 3 else dict(c["data"])     # the data key, then the argument
        out_a = a.train_step(data, (N_ITER, False), dropout_seed=seed, frozen_mode=frozen_mode, match_radius=None if seed == 3 else RADIUS)
        out_b = b.train_step({**c["data"], "matches": lists}, (N_ITER, False), dropout_seed=seed, frozen_mode=frozen_mode)
        assert out_a["losses"] == out_b["losses"] and any(k.startswith("outlier_") for k in out_a["losses"])
    _assert_same_training(a, b, frozen_mode)
    none = _net("align").train_step(dict(c["data"]), (N_ITER, False), dropout_seed=3, frozen_mode=frozen_mode)
    assert not any(k.startswith("outlier_") for k in none["losses"])        # neither a list nor a radius: no confidence term
    torch.cuda.synchronize()


@pytest.mark.parametrize("frozen_mode", ["train", "eval"])
def test_train_step_does_not_call_the_host_function(frozen_mode, monkeypatch):
    import deepsir_amd.train as T

    def boom(*args, **kw):
        raise AssertionError("find_correct_correspondence was called: the targets must be made on the device")
    monkeypatch.setattr(T, "find_correct_correspondence", boom)
    net = _net("align")
    c = _case("align", "A")
    out = net.train_step({**c["data"], "matches": c["matches"]}, (N_ITER, False), dropout_seed=1, frozen_mode=frozen_mode)
    assert np.isfinite(out["loss"]) and any(k.startswith("outlier_") for k in out["losses"])
    ep = _forward(net, c)                                                    # the verbatim loop's loss too
    ep["transform_gt"], ep["matches"] = c["data"]["transform_gt"], c["matches"]
    res = net.loss_align_fun(ep, reduction="mean")
    assert np.isfinite(res["total"].item()) and "outlier_0" in res
    torch.cuda.synchronize()


def _loop_grads(net, c, how):
    """The reference loop's forward + loss + backward; how: 'matches' | 'radius' | 'radius_lists' | 'host' (labels from the host
    function handed straight to the loss operator's autograd node)."""
    from deepsir_amd.autograd import _AlignLoss
    _zero(net)
    ep = _forward(net, c)
    ep["transform_gt"] = c["data"]["transform_gt"]
    if how == "host":
        tr = ep["_train"]
        J = ep["pt_src"].shape[1]
        f = net.loss_align_fun
        kw = dict(loss_type=f.loss_type, wt_ptDist_loss=f.wt_ptDist_loss, wt_inlier_loss=f.wt_inlier_loss, loss_discount_factor=f.discount_factor)
        loss = _AlignLoss.apply(tr["logits"], tr["engine"], ep["pt_src"].float().contiguous(), ep["pt_ref"].float().contiguous(),
                                tr["idx"].to(torch.int32).contiguous(), _host_labels(c, tr["idx"], J), ep["transform_gt"].float().contiguous(), kw)
    else:
        if how == "matches":
            ep["matches"] = c["matches"]
        elif how == "radius":
            ep["match_radius"] = RADIUS
        else:
            ep["matches"] = _radius_lists(net, c)
        res = net.loss_align_fun(ep, reduction="mean")
        assert "outlier_0" in res
        loss = res["total"]
    loss.backward()
    return loss.item(), _grads(net)


def test_reference_loop_loss_takes_device_targets_and_changes_nothing():
    net = _net("align")
    c = _case("align", "A")
    la, ga = _loop_grads(net, c, "matches")
    lb, gb = _loop_grads(net, c, "host")
    assert la == lb and all(torch.equal(ga[k], gb[k]) for k in ga), "matches on the device vs labels from the host function"
    lr_, gr = _loop_grads(net, c, "radius")
    ll, gl = _loop_grads(net, c, "radius_lists")
    assert lr_ == ll and all(torch.equal(gr[k], gl[k]) for k in gr), "match_radius vs matches = radius_matches(...)"
    assert any(float(v.abs().max()) > 0 for v in ga.values())
    # the loss object's own radius (constructor argument / args.match_radius)
    from deepsir_amd.autograd import ScanAlignmentLoss
    from test_train_loop import _args
    net.loss_align_fun = ScanAlignmentLoss(net, _args("align", num_reg_iter=N_ITER), match_radius=RADIUS)
    _zero(net)
    ep = _forward(net, c)
    ep["transform_gt"] = c["data"]["transform_gt"]
    assert net.loss_align_fun(ep, reduction="mean")["total"].item() == lr_
    torch.cuda.synchronize()
