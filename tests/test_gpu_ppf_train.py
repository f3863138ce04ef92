"""Training under ``use_ppf`` on the device: the taped point-pair-feature front end (dsir_t_ppf_fwd / dsir_t_ppf_bwd, csrc/ppf.hip),
the trainers with a 12-channel level 0, and the reference's training loop on the drop-in ``Network``.  References: the imported
reference's autograd (tests/golden/ppf_train_*.npz, tools/gen_golden_ppf_train.py) and the host restatement
(deepsir_amd/ppf.py::ppf_pre_backward; its own distance to the reference is measured in tests/test_ppf_train_host.py)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from deepsir_amd import ppf
from deepsir_amd.arch import NetConfig
from deepsir_amd.weights import generate_state_dict, to_torch_state_dict
from oracle.gen_golden_train import case_inputs, sample_index
from test_ppf_train_host import NAMES, front_case

pytestmark = pytest.mark.gpu

GOLD_NET = np.load(os.path.join(ROOT, "tests", "golden", "ppf_train_net_n1024.npz"))
CFG = NetConfig(feat_len=6, use_ppf=True)
ZERO_BY_CONSTRUCTION = ("fc_label.0.bias", "fc_label.3.bias")   # a bias in front of BatchNorm: the batch mean removes it
RTOL, ATOL = 2e-3, 1e-6                                          # the project's rule for gradient comparisons (tests/test_train.py)


def _dev():
    return torch.device("cuda:0")


def _cu(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(_dev())


def _close(got, ref, name=""):
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"{name}: max error {err:.3e}, scale {scale:.3e}")
    assert err <= RTOL * scale + ATOL, f"{name}: {err:.3e} vs scale {scale:.3e}"


class _Front:
    """The front end's operators on one set of inputs, gradients in fresh zeroed buffers."""

    def __init__(self, rows, neigh, w):
        from deepsir_amd.train import _Ops
        self.o = _Ops(_dev())
        self.rows, self.neigh = _cu(rows), _cu(neigh, torch.int32)
        self.w = [_cu(np.asarray(t, np.float32).reshape(t.shape[0], -1) if t.ndim > 1 else t) for t in w]
        self.out, self.saved = self.o.ppf_fwd(self.rows, self.neigh, *self.w)

    def zeros(self):
        return [torch.zeros(12, 10, device=_dev())] + [torch.zeros(12, device=_dev()) for _ in range(3)]

    def backward(self, dout, into=None):
        """-> ([dW, db, dgamma, dbeta] device tensors, per-cloud sums [clouds][24] float64 (copied))"""
        g = into if into is not None else self.zeros()
        per_cloud = self.o.ppf_bwd(self.rows, self.neigh, *self.w, self.saved, dout, *g).clone()
        torch.cuda.synchronize()
        return g, per_cloud


def _random_front(clouds, n, stride, seed, degenerate_cloud=None):
    """Seeded rows (points in a unit cube, unit normals, extra columns of noise), random neighbour lists with the point itself first,
    seeded weights.  degenerate_cloud: that cloud's neighbours all coincide with the point and its normals are zero."""
    rng = np.random.Generator(np.random.Philox(key=seed))
    rows = rng.random((clouds, n, stride)).astype(np.float32)
    nrm = rng.standard_normal((clouds, n, 3))
    rows[:, :, 3:6] = nrm / np.linalg.norm(nrm, axis=2, keepdims=True)
    neigh = rng.integers(0, n, (clouds, n, 16)).astype(np.int32)
    neigh[:, :, 0] = np.arange(n)
    if degenerate_cloud is not None:
        neigh[degenerate_cloud] = np.arange(n)[:, None]
        rows[degenerate_cloud, :, 3:6] = 0.0
    w = [rng.standard_normal((12, 10)).astype(np.float32) * 0.5, rng.standard_normal(12).astype(np.float32) * 0.1,
         (1.0 + 0.2 * rng.standard_normal(12)).astype(np.float32), rng.standard_normal(12).astype(np.float32) * 0.1]
    G = rng.standard_normal((clouds, n, 12)).astype(np.float32)
    return rows, neigh, w, G


def test_taped_forward_is_the_inference_front_end_byte_for_byte():
    from deepsir_amd.engine import Engine
    rows, neigh, w, _, _ = front_case()
    meta = json.loads(str(np.load(os.path.join(ROOT, "tests", "golden", "ppf_train_front_n1024.npz"))["meta"]))
    eng = Engine(CFG, max_points=1024, max_pairs=2)
    eng.load_state_dict(generate_state_dict(CFG, meta["wseed"]))
    want = eng.ppf_pre("feat_extractor", _cu(rows), _cu(neigh, torch.int32))
    f = _Front(rows, neigh, w)
    torch.cuda.synchronize()
    assert torch.equal(f.out.view(torch.int32), want.view(torch.int32))
    assert bool(torch.isfinite(f.saved).all())
    eng.close()


def test_front_end_gradients_match_reference_autograd_and_the_restatement():
    """Fixture (a): n = 1024, two clouds, duplicate points and zero normals.  Tolerance: the project's rule, 2e-3 of the tensor's
    maximum + 1e-6.  The restatement itself sits 1.9e-6 .. 4.9e-6 of the maximum from the reference (tests/test_ppf_train_host.py), so
    the rule holds for the fixture as it stands and the 10x-the-host-distance fallback (5e-5) is not needed."""
    rows, neigh, w, G, ref = front_case()
    f = _Front(rows, neigh, w)
    g, _ = f.backward(_cu(G))
    host = ppf.ppf_pre_backward(rows, neigh, *w, G)
    for name, got, want, h in zip(NAMES, g, ref, host):
        _close(got.cpu().numpy(), want, "reference " + name)
        _close(got.cpu().numpy(), h, "restatement " + name)


@pytest.mark.parametrize("clouds,n,stride,degenerate", [(1, 70, 6, None), (3, 1100, 7, None), (2, 200, 6, 1)])
def test_front_end_edge_shapes_match_the_restatement(clouds, n, stride, degenerate):
    """n = 70: two workgroups, the second with 6 live points; four neighbour indices below 0 or at / beyond n (the kept clamp of
    ppf_row, in the forward and in both backward passes).  3 x 1100 x 7 columns: ragged, multi-cloud, strided rows; cloud 1 alone
    gives the bytes of its d gamma / d beta contribution inside the batch.  A cloud whose neighbours all coincide, normals zero:
    every angle is atan2(0, 0), the variance is that of the point coordinates alone - finite gradients."""
    rows, neigh, w, G = _random_front(clouds, n, stride, 1000 + n, degenerate)
    if n == 70:                                     # indices outside the cloud, in both workgroups: clamped to [0, n) by ppf_row and by the restatement
        neigh[0, 3, 5], neigh[0, 40, 9], neigh[0, 66, 2], neigh[0, 69, 15] = -7, n, n + 1000, -1
    f = _Front(rows, neigh, w)
    want_out = ppf.ppf_pre(rows, neigh, *w)
    assert np.abs(f.out.cpu().numpy() - want_out).max() <= 1e-4 * np.abs(want_out).max() + 1e-5
    g, per_cloud = f.backward(_cu(G))
    host = ppf.ppf_pre_backward(rows, neigh, *w, G, per_cloud=True)
    for name, got, h in zip(NAMES, g, host):
        assert np.isfinite(got.cpu().numpy()).all(), name
        _close(got.cpu().numpy(), h, name)
    _close(per_cloud.cpu().numpy()[:, :12], host[4], "per-cloud d beta")
    _close(per_cloud.cpu().numpy()[:, 12:], host[5], "per-cloud d gamma")
    if clouds == 3:
        alone = _Front(rows[1:2], neigh[1:2], w)
        _, pc1 = alone.backward(_cu(G[1:2]))
        assert torch.equal(pc1[0].view(torch.int64), per_cloud[1].view(torch.int64))
        assert torch.equal(alone.out.view(torch.int32), f.out[1:2].view(torch.int32))


def test_front_end_gradients_accumulate_and_repeat():
    rows, neigh, w, G = _random_front(2, 333, 6, 77)
    f = _Front(rows, neigh, w)
    dout = _cu(G)
    once, _ = f.backward(dout)
    again, _ = f.backward(dout)
    twice, _ = f.backward(dout, into=[t.clone() for t in once])
    for name, a, b, c in zip(NAMES, once, again, twice):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name              # two fresh runs: identical bytes
        assert torch.allclose(c, 2 * a, rtol=1e-6, atol=0.0), name                      # two backwards into the same buffers


def _check_net_grads(grads, seed):
    """tests/test_train.py::_check_grads on fixture (b): whole tensors, or samples + norm for the large ones."""
    checked = 0
    for name, g in grads.items():
        g = np.asarray(g, np.float64).reshape(-1)
        key = "g_" + name
        if name.endswith(ZERO_BY_CONSTRUCTION):
            wscale = np.abs(GOLD_NET[f"g_{name[:-4]}weight"] if f"g_{name[:-4]}weight" in GOLD_NET else GOLD_NET[f"g_{name[:-4]}weight_samples"]).max()
            assert np.abs(g).max() <= 1e-4 * wscale and np.abs(GOLD_NET[key]).max() <= 1e-4 * wscale, name
            continue
        if key in GOLD_NET:
            ref = GOLD_NET[key].astype(np.float64)
        else:
            ref = GOLD_NET[key + "_samples"].astype(np.float64)
            s, nrm = GOLD_NET[key + "_sum_norm"]
            assert abs(np.sqrt((g ** 2).sum()) - nrm) <= RTOL * nrm + ATOL * np.sqrt(g.size), name
            g = g[sample_index(name[len("inlier_model."):], g.size, seed)]
        scale = np.abs(ref).max()
        assert np.abs(g - ref).max() <= RTOL * scale + ATOL, f"{name}: {np.abs(g - ref).max():.3e} vs scale {scale:.3e}"
        checked += 1
    assert checked > 100


def test_whole_network_training_pass_matches_reference_autograd():
    """Fixture (b): the reference's RandLA with use_ppf (feat_in 6, one class) in training mode, two clouds of 1024 points."""
    from deepsir_amd.train import RandlaTrainer
    meta = json.loads(str(GOLD_NET["meta"]))
    n = meta["n"]
    d = case_inputs(CFG, n, meta["seed"])
    sd = generate_state_dict(CFG, meta["wseed"], meta["variant"])
    keep = np.unpackbits(GOLD_NET["keep"])[: 2 * 64 * n].reshape(2, 64, n)
    tr = RandlaTrainer(CFG, sd, "inlier_model", 6, 1, _dev())
    inp = (_cu(d["cat"]), _cu(d["points_src_xyz"]), _cu(d["points_src_neigh_idx"], torch.int32), _cu(d["points_src_sub_idx"], torch.int32),
           _cu(d["points_src_interp_idx"], torch.int32))
    logits, tape = tr.forward(*inp, dropout_mask=_cu(keep.transpose(0, 2, 1), torch.uint8))
    err = np.abs(logits.cpu().numpy() - GOLD_NET["logits"].transpose(0, 2, 1)).max()
    print(f"logits: max error {err:.3e}")
    assert err < 5e-4
    tr.backward(tape, _cu(d["G"].transpose(0, 2, 1)))
    torch.cuda.synchronize()
    assert tr.params["inlier_model.dilated_res_blocks.0.mlp1.conv.weight"].shape[1] == 12
    _check_net_grads({k: v.cpu().numpy() for k, v in tr.grads.items()}, meta["seed"])


def _ppf_pairs(n, seeds):
    """``make_pair`` clouds with three more columns: seeded unit normals."""
    from deepsir_amd.synth import make_pair
    raws = [make_pair(n, s, 3) for s in seeds]
    rng = np.random.Generator(np.random.Philox(key=0x99F + int(seeds[0])))
    out = {}
    for side in ("points_src", "points_ref"):
        xyz = np.concatenate([r[side] for r in raws]).astype(np.float32)
        nrm = rng.standard_normal(xyz.shape)
        out[side] = np.ascontiguousarray(np.concatenate([xyz, nrm / np.linalg.norm(nrm, axis=2, keepdims=True)], 2), dtype=np.float32)
    out["transform_gt"] = np.concatenate([r["transform_gt"] for r in raws]).astype(np.float32)
    return out


def test_align_step_trains_the_front_end_and_replays_from_graphs():
    """train_step_align with a use_ppf trainer (2 pairs x 1024 points x 3 iterations): the loss falls, mlp_pre's weight receives a
    gradient; AlignTrainStep's graph-replayed steps equal the eager steps bit for bit under the same dropout seeds."""
    from deepsir_amd.engine import Engine
    from deepsir_amd.train import AlignTrainStep, RandlaTrainer, train_step_align
    n, P, n_iter = 1024, 2, 3
    sd = generate_state_dict(CFG, 3, "plain")
    eng = Engine(CFG, max_points=n, max_pairs=P)
    eng.load_state_dict(sd)
    raw = _ppf_pairs(n, [100, 101])
    src, ref, gt = _cu(raw["points_src"]), _cu(raw["points_ref"]), _cu(raw["transform_gt"])
    sx, sn, ss, si = eng.knn_pyramid(src)
    res = eng.register(src, ref, n_iter=n_iter)
    batch = {"points_src": src, "points_ref": ref, "src_xyz": sx, "src_neigh": sn, "src_sub": ss, "src_interp": si}
    a, b = (RandlaTrainer(CFG, sd, "inlier_model", 6, 1, _dev()) for _ in range(2))
    stepper = AlignTrainStep(eng, b, P, n, n, n_iter, dropout=True)
    losses = []
    for s in range(5):
        oa = train_step_align(eng, a, batch, res, gt, lr=2e-3, dropout_seed=40 + s)
        assert not oa["skipped"]
        if s == 0:
            assert float(a.grads["inlier_model.mlp_pre.conv.weight"].abs().max()) > 0.0
        ob = stepper.step(batch, res, gt, lr=2e-3, dropout_seed=40 + s)
        torch.cuda.synchronize()
        assert torch.equal(oa["logits"].view(torch.int32), ob["logits"].view(torch.int32)), s
        assert torch.equal(a.flat_g.view(torch.int32), b.flat_g.view(torch.int32)), s
        assert torch.equal(a.flat_p.view(torch.int32), b.flat_p.view(torch.int32)), s
        losses.append(oa["losses"]["total"])
    assert stepper.gf is not None and stepper.gb is not None
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


def _args(pipeline, **kw):
    base = dict(pipeline=pipeline, feat_len=6, num_sub=-1, num_knn=16, out_feat_dim=64, clip_weight_thresh=0.0, d_out=[16, 64, 128, 256],
                sub_sampling_ratio=[4, 4, 4, 4], use_ppf=True, num_reg_iter=3, loss_type="mae", wt_ptDist_loss=1.0, wt_inlier_loss=1.0,
                wt_pose_loss=0.0, loss_discount_factor=0.5, thres_radius=0.1, det_loss_weight=1.0)
    base.update(kw)
    return SimpleNamespace(**base)


@pytest.mark.parametrize("pipeline", ["label", "align"])
def test_reference_training_loop_under_use_ppf(pipeline):
    """The loop of tests/test_train_loop.py (torch's Adam, a few steps) on a use_ppf ``Network``: the loss falls, only the pipeline's
    trainable tensors receive gradients - mlp_pre's four among them -, and the next evaluation-mode forward serves the new weights."""
    from deepsir_amd.model import Network
    n, P = 1024, 2
    dev = _dev()
    my_model = Network(_args(pipeline))
    my_model.load_state_dict(to_torch_state_dict(generate_state_dict(my_model.cfg, 8, "plain")))
    my_model.to(dev)
    optimizer = torch.optim.Adam([p for p in my_model.parameters() if p.requires_grad], lr=2e-3)
    raw = _ppf_pairs(n, [800, 801])
    train_data = {k: _cu(v) for k, v in raw.items()}
    opt_tuple = (3, True) if pipeline == "align" else None
    g = torch.Generator().manual_seed(2)
    labels = [torch.randint(0, 20, (P, n), generator=g) for _ in range(2)]
    key = "perm_matrices" if pipeline == "align" else "logits_src"
    my_model.eval()
    with torch.no_grad():
        before = my_model(train_data, opt_tuple)[1][key]
        before = (before[-1] if pipeline == "align" else before).clone()
    my_model.train()
    # one fixed set of Dropout keep flags for every step (the Network's test aid): the objective the steps lower is one function
    from deepsir_amd.train import dropout_keep_masks
    my_model.dropout_masks = {"fe_src": dropout_keep_masks(1, (P, n, 64), dev), "fe_ref": dropout_keep_masks(2, (P, n, 64), dev),
                              "inlier": dropout_keep_masks(3, (3, P, n, 64), dev)}
    trained = "inlier_model" if pipeline == "align" else "feat_extractor"
    losses = []
    for step in range(5):
        optimizer.zero_grad()
        pred, endpoints = my_model(train_data, opt_tuple)
        endpoints['transform_gt'] = train_data['transform_gt']
        if pipeline == "align":
            endpoints['transform_pred'] = pred
            loss = my_model.loss_align_fun(endpoints, reduction='mean')['total']
        else:
            endpoints['labels_src'], endpoints['labels_ref'] = labels
            loss, _ = my_model.loss_label_fun(endpoints)
        loss.backward()
        optimizer.step()
        losses.append(loss.item())
        with_grad = {k for k, p in my_model.named_parameters() if p.grad is not None}
        assert {k.split(".", 1)[0] for k in with_grad} == {trained}, with_grad
        assert all(f"{trained}.mlp_pre.{k}" in with_grad for k in NAMES)
    assert float(dict(my_model.named_parameters())[f"{trained}.mlp_pre.conv.weight"].grad.abs().max()) > 0.0
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    my_model.eval()
    with torch.no_grad():
        after = my_model(train_data, opt_tuple)[1][key]
        after = after[-1] if pipeline == "align" else after
    assert bool(torch.isfinite(after).all()) and not torch.equal(after, before)


def test_training_forward_with_estimated_normals_or_the_reference_assertion():
    from deepsir_amd.model import Network
    raw = _ppf_pairs(1024, [810, 811])
    bare = {"points_src": _cu(raw["points_src"][:, :, :3]), "points_ref": _cu(raw["points_ref"][:, :, :3])}
    labels = [torch.randint(0, 20, (2, 1024), generator=torch.Generator().manual_seed(3)) for _ in range(2)]
    for estimate in (True, False):
        net = Network(_args("label", feat_len=3, ppf_estimate_normals=estimate))
        net.load_state_dict(to_torch_state_dict(generate_state_dict(net.cfg, 8, "plain")))
        net.to(_dev()).train()
        if not estimate:
            with pytest.raises(AssertionError, match="feature dimension error"):
                net(bare, None)
            continue
        _, endpoints = net(bare, None)
        endpoints['labels_src'], endpoints['labels_ref'] = labels
        loss, _ = net.loss_label_fun(endpoints)
        loss.backward()
        g = dict(net.named_parameters())["feat_extractor.mlp_pre.conv.weight"].grad
        assert np.isfinite(loss.item()) and g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0
