"""The HIP training path at the reference's default training shape (KITTI-shaped clouds of 18000 points, feat_len 4,
arguments.py:23-87) against the CPU oracle run in float64, and the training operators at the sizes where their plans change.

Error model.  The device runs in fp32 (unit roundoff u = 2^-24 ~ 6e-8) through ~40 layers; its inputs are handed to the fp64
oracle unchanged, so what remains is accumulated rounding.  Per tensor the relative L2 error of a gradient is required below 1e-3;
entry-wise the error is bounded relative to the tensor's largest entry (1e-2; a gradient entry that sums many cancelling
terms keeps the absolute error of its larger neighbours).  Gradients that are themselves sums of cancelling terms (the
attention scores' weights: a softmax gradient sums to zero over the 16 neighbours) sit highest.  The gradient is piecewise
in the forward values: LeakyReLU's sign is left as it falls, the max-pool is teacher-forced - the oracle gathers at the
device's arg-max (``oracle.train.randla_train(pool_args=...)``) - and the device's arg-max is separately checked to be a
true maximum within the device's own forward error at that level.  A bias in front of a BatchNorm / GroupNorm has a zero
gradient by construction; there both sides are required to be noise.

Worst errors measured on an MI355X (relative L2 / entry-wise relative to the tensor's max):
    label, P = 1:  2.0e-04 (dilated_res_blocks.2.lfa.mlp2.norm.weight) / 4.1e-04
    label, P = 2 (18000 / 17011 points):  8.7e-04 (dilated_res_blocks.0.lfa.att_pooling_1.fc.weight) / 1.6e-03
    align, n_iter = 2:  8.8e-04 / 1.0e-03
    feat, num_sub = 2048:  9.3e-05 (mlp_att.0.weight) / 1.8e-04
(printed by each test as a ``SCALE`` line)."""
import numpy as np
import pytest
import torch

from deepsir_amd.arch import NetConfig, semantic_class_weights
from oracle.network import OracleNet
from oracle import train as otrain

pytestmark = pytest.mark.gpu

F64 = torch.float64
U32 = 2.0 ** -24
N_PTS = 18000
REL_L2, REL_MAX = 1e-3, 1e-2


def _dev():
    return torch.device("cuda", 0)


def _threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))


def _compare_grads(got: dict, want: dict, what: str):
    """got: name -> device tensor, want: name -> fp64 oracle tensor.  -> (worst relative L2, its tensor, worst entry-wise / max)."""
    gmax = max(float(w.abs().max()) for w in want.values())
    worst_l2 = worst_mx = 0.0
    worst_k = None
    n = 0
    for k, w in want.items():
        g = got[k].detach().double().cpu().reshape(-1)
        w = w.detach().reshape(-1)
        wmax = float(w.abs().max())
        if wmax <= 1e-9 * gmax:                    # zero by construction (a bias in front of a normalisation): noise on both sides
            assert float(g.abs().max()) <= 1e-4 * gmax, (what, k, float(g.abs().max()), gmax)
            continue
        l2 = float((g - w).norm() / w.norm())
        mx = float((g - w).abs().max()) / wmax
        assert l2 <= REL_L2, (what, k, "relative L2", l2)
        assert mx <= REL_MAX, (what, k, "entry-wise", mx)
        if l2 > worst_l2:
            worst_l2, worst_k = l2, k
        worst_mx = max(worst_mx, mx)
        n += 1
    assert n >= 20, (what, n)
    return worst_l2, worst_k, worst_mx


def _pyramid(eng, pts):
    x, nb, sb, it = eng.knn_pyramid(pts)
    return [t.contiguous() for t in (x, nb, sb, it)]


def _oracle_pyr(pyr):
    x, nb, sb, it = pyr
    return [x.cpu().to(F64), nb.cpu().long(), sb.cpu().long(), it.cpu().long()]


def _check_argmax_is_max(tape, prefix, taps, L, what):
    """The device's max-pool winner per (output row, channel) is a maximum of the fp64 values up to the device's own forward
    error at that level (a near-tie may go either way; a wrong row would sit far below the maximum)."""
    net = tape.misc["net"]
    for l in range(L):
        enc64 = taps[f"enc{l}"]                                                   # [B, C, n]
        B, C_, n = enc64.shape
        enc_dev = tape.misc[f"{prefix}.dilated_res_blocks.{l}"][0].reshape(B, n, C_).permute(0, 2, 1).double().cpu()
        err = float((enc_dev - enc64).abs().max())
        pool = taps[f"pool{l}"]                                                   # [B, m, k]
        m, k = pool.shape[1], pool.shape[2]
        vals = torch.gather(enc64, 2, pool.reshape(B, 1, m * k).expand(B, C_, m * k)).reshape(B, C_, m, k)
        mx = vals.max(dim=3)[0]
        arg = net["args"][l].long().cpu().permute(0, 2, 1)                        # [B, C, m]
        assert bool((pool.reshape(B, 1, m, k) == arg.reshape(B, C_, m, 1)).any(3).all()), (what, l, "arg-max outside the pool")
        at = torch.gather(enc64, 2, arg)
        gap = float((mx - at).max())
        assert gap <= 2 * err + 4 * U32 * float(mx.abs().max()), (what, l, gap, err)


# ------------------------------------------------------------------------------------------------------------------- label
@pytest.mark.parametrize("n_ref,P", [(N_PTS, 1), (17011, 2)])
def test_label_pipeline_at_training_scale_matches_fp64_oracle(n_ref, P):
    """`label` (feature extractor + semantic head): two training-mode forwards (src, ref), weighted cross entropy, backward -
    every feat_extractor gradient, every BatchNorm running statistic and the loss against fp64 autograd of the oracle on the
    same pyramids and Dropout masks."""
    from deepsir_amd.engine import Engine
    from deepsir_amd.synth import make_pair
    from deepsir_amd.train import RandlaTrainer, dropout_keep_masks
    from deepsir_amd.weights import generate_state_dict
    _threads()
    cfg = NetConfig(feat_len=4)
    sd = generate_state_dict(cfg, 31, "plain")
    sizes = {"src": N_PTS, "ref": n_ref}
    pts = {}
    for s, n in sizes.items():
        raws = [make_pair(n, 1700 + 10 * b + (s == "ref"), 4, shape="kitti") for b in range(P)]
        pts[s] = torch.from_numpy(np.concatenate([r[f"points_{s}"] for r in raws])).to(_dev())
    eng = Engine(cfg, max_points=N_PTS, max_pairs=P)
    eng.load_state_dict(sd)
    g = torch.Generator().manual_seed(17)
    labels = {s: torch.randint(0, 20, (P, n), generator=g) for s, n in sizes.items()}
    tr = RandlaTrainer(cfg, sd, "feat_extractor", cfg.feat_len, cfg.num_classes, _dev())
    cw = torch.tensor(semantic_class_weights(), dtype=torch.float32, device=_dev())
    o = tr.ops
    tr.zero_grad()
    dev_out = {}
    for si, (s, n) in enumerate(sizes.items()):
        pyr = _pyramid(eng, pts[s])
        mask = dropout_keep_masks(50 + si, (P, n, 64), _dev())
        lg, tape = tr.forward(pts[s], *pyr, mask)
        d, out = o.weighted_ce(lg.reshape(P * n, cfg.num_classes), labels[s].int().to(_dev()).reshape(-1).contiguous(), cw)
        tr.backward(tape, d)
        dev_out[s] = (pyr, mask, lg, tape, out)
    torch.cuda.synchronize()
    # ---- fp64 oracle on the same pyramids and masks, max-pool teacher-forced at the device's arg-max
    net = OracleNet(cfg, sd, F64)
    params = otrain.trainable(net, "feat_extractor")
    total, dev_total = 0.0, 0.0
    for s in sizes:
        pyr, mask, lg, tape, out = dev_out[s]
        taps = {}
        lgt = otrain.randla_train(net, "feat_extractor", pts[s].cpu().to(F64), *_oracle_pyr(pyr), mask.cpu().permute(0, 2, 1).bool(),
                                  pool_args=[a.cpu() for a in tape.misc["net"]["args"]], taps=taps)
        _check_argmax_is_max(tape, "feat_extractor", taps, len(cfg.d_out), f"label/{s}")
        lerr = float((lg.double().cpu() - lgt.detach().permute(0, 2, 1)).abs().max() / lgt.detach().abs().max())
        assert lerr < 1e-4, (s, lerr)
        total = total + otrain.semantic_loss(lgt, labels[s], semantic_class_weights())
        dev_total += float(out[0])
    total.backward()
    total = float(total.detach())
    assert abs(dev_total - total) <= 1e-5 * abs(total), (dev_total, total)
    l2, wk, mx = _compare_grads(tr.grads, {k: p.grad for k, p in params.items()}, "label")
    for k, v in tr.buffers.items():
        w = net.p[k]
        assert float((v.double().cpu() - w).abs().max()) <= 1e-5 * float(w.abs().max()) + 1e-7, k
    print(f"SCALE label P={P} n_ref={n_ref}: worst relative L2 {l2:.2e} ({wk}), entry-wise {mx:.2e}")


# ------------------------------------------------------------------------------------------------------------------- align
def test_align_inlier_step_at_training_scale_matches_fp64_oracle():
    """`align` (the inlier model, n_iter = 2, with the correspondence-confidence labels): the device's arg-min correspondences
    and poses of the inference half are fed to the oracle (as test_train_step_align_gradients_match_the_oracle does); the loss,
    the logits and every inlier-model gradient against fp64 autograd."""
    from deepsir_amd.engine import Engine
    from deepsir_amd.synth import make_pair
    from deepsir_amd.train import RandlaTrainer, dropout_keep_masks
    from deepsir_amd.weights import generate_state_dict
    from oracle import align_loss as oal
    _threads()
    n, P, n_iter = N_PTS, 1, 2
    cfg = NetConfig(feat_len=4)
    sd = generate_state_dict(cfg, 32, "separated")
    raw = make_pair(n, 1800, 4, shape="kitti")
    src, ref, gt = (torch.from_numpy(raw[k]).to(_dev()) for k in ("points_src", "points_ref", "transform_gt"))
    eng = Engine(cfg, max_points=n, max_pairs=P)
    eng.load_state_dict(sd)
    pyr = _pyramid(eng, src)
    res = eng.register(src, ref, n_iter=n_iter)
    idx, T = res["idx"], res["transforms"]
    rng = np.random.Generator(np.random.Philox(key=18))
    labels = torch.from_numpy((rng.random((n_iter, P, n)) < 0.6).astype(np.float32))
    masks = dropout_keep_masks(19, (n_iter, P, n, 64), _dev())
    tr = RandlaTrainer(cfg, sd, "inlier_model", 6, 1, _dev())
    o = tr.ops
    xyz_s, xyz_r = src[:, :, :3].contiguous(), ref[:, :, :3].contiguous()
    tr.zero_grad()
    shared, tapes, lgs = {}, [], []
    for it in range(n_iter):
        cat = o.inlier_input(xyz_s, xyz_r, idx[it], None if it == 0 else T[:, it - 1])
        lg, tape = tr.forward(cat, *pyr, masks[it], shared=shared)
        tapes.append(tape)
        lgs.append(lg.reshape(P, n))
    lg_all = torch.stack(lgs).contiguous()
    out = eng.align_loss_backward(xyz_s, xyz_r, idx, lg_all, labels.to(_dev()), gt)
    for it in range(n_iter):
        tr.backward(tapes[it], out["grad_logits"][it], shared=shared)
    tr.backward_shared(shared)
    torch.cuda.synchronize()
    # ---- fp64 oracle
    net = OracleNet(cfg, sd, F64)
    params = otrain.trainable(net)
    ps, pr = src[:, :, :3].cpu().to(F64), ref[:, :, :3].cpu().to(F64)
    opyr = _oracle_pyr(pyr)
    Tc = T.cpu().to(F64)
    logits = []
    for it in range(n_iter):
        cur = ps if it == 0 else OracleNet.se3_apply(Tc[:, it - 1], ps)
        cat = torch.cat([cur, torch.gather(pr, 1, idx[it].cpu().long()[:, :, None].expand(-1, -1, 3))], 2)
        taps = {}
        lgt = otrain.randla_train(net, "inlier_model", cat, *opyr, masks[it].cpu().permute(0, 2, 1).bool(),
                                  pool_args=[a.cpu() for a in tapes[it].misc["net"]["args"]], taps=taps).squeeze(1)
        _check_argmax_is_max(tapes[it], "inlier_model", taps, len(cfg.d_out), f"align/{it}")
        logits.append(lgt)
    lerr = float((lg_all.double().cpu() - torch.stack(logits).detach()).abs().max() / torch.stack(logits).detach().abs().max())
    assert lerr < 1e-4, lerr
    poses = oal.replay(ps, pr, [i.cpu().long() for i in idx], logits)
    d = oal.scan_alignment_loss(ps, poses, gt.cpu().to(F64), logits, [l.to(F64) for l in labels])
    d["total"].backward()
    assert abs(out["losses"]["total"] - float(d["total"])) <= 1e-5 * max(1.0, abs(float(d["total"]))), (out["losses"]["total"], float(d["total"]))
    l2, wk, mx = _compare_grads(tr.grads, {k: p.grad for k, p in params.items()}, "align")
    print(f"SCALE align n_iter={n_iter}: worst relative L2 {l2:.2e} ({wk}), entry-wise {mx:.2e}")


# ------------------------------------------------------------------------------------------------------------------- feat
def test_feat_pipeline_at_training_scale_matches_fp64_oracle():
    """`feat` (num_sub = 2048): the frozen extractor in training mode scores 18000 points, the top-k keeps the reference's
    selection rule (descending score, equal scores in ascending index); DetDesLoss and every aggregation gradient against fp64
    autograd of the oracle on the selected key points."""
    from deepsir_amd.engine import Engine
    from deepsir_amd.synth import make_pair
    from deepsir_amd.train import AggregationTrainer, RandlaTrainer, dropout_keep_masks, feat_pipeline_inputs_train, train_step_feat
    from deepsir_amd.weights import generate_state_dict
    _threads()
    n, P, M = N_PTS, 1, 2048
    cfg = NetConfig(feat_len=4, pipeline="feat", num_sub=M)
    sd = generate_state_dict(cfg, 33, "separated")
    raw = make_pair(n, 1900, 4, shape="kitti")
    batch = {f"points_{s}": torch.from_numpy(raw[f"points_{s}"]).to(_dev()) for s in ("src", "ref")}
    gt = torch.from_numpy(raw["transform_gt"]).to(_dev())
    gt[:, :, 3] += 2e-3                                                  # off the exact-coincidence knife edge
    eng = Engine(cfg, max_points=n, max_pairs=P)
    eng.load_state_dict(sd)
    for s in ("src", "ref"):
        batch[f"{s}_xyz"], batch[f"{s}_neigh"], batch[f"{s}_sub"], batch[f"{s}_interp"] = _pyramid(eng, batch[f"points_{s}"])
    masks = {f"fe_{s}": dropout_keep_masks(60 + i, (P, n, 64), _dev()) for i, s in enumerate(("src", "ref"))}
    fe = RandlaTrainer(cfg, sd, "feat_extractor", cfg.feat_len, cfg.num_classes, _dev())
    inp = feat_pipeline_inputs_train(eng, fe, batch, M, masks)
    # the selection: the device's scores of all points, ranked by the reference's rule, give the same key points in the same order
    for s in ("src", "ref"):
        lg, tape = fe.forward(batch[f"points_{s}"].contiguous(), batch[f"{s}_xyz"], batch[f"{s}_neigh"], batch[f"{s}_sub"], batch[f"{s}_interp"],
                              masks[f"fe_{s}"], update_running_stats=False)
        score, _ = eng.score(tape.misc["feat"].contiguous(), lg.contiguous(), batch[f"{s}_xyz"], batch[f"{s}_neigh"])
        sc = score.cpu()
        want = torch.sort(sc + 0.0, dim=-1, descending=True, stable=True)[1][:, :M]
        assert torch.equal(inp[f"index_{s}"].cpu().long(), want), s
        assert torch.equal(inp[f"score_{s}"].cpu(), torch.gather(sc, 1, want))
    tr = AggregationTrainer(cfg, sd, _dev())
    res = train_step_feat(tr, inp, gt, 0.6, 1.0, apply=False)
    torch.cuda.synchronize()
    # ---- fp64 oracle on the device's key points
    net = OracleNet(cfg, sd, F64)
    params = {k: v.requires_grad_(True) for k, v in net.p.items()
              if k.startswith(("mlp_feat", "mlp_att", "mlp_proj")) and v.is_floating_point() and not k.endswith(("running_mean", "running_var"))}
    cm = lambda t: t.cpu().to(F64).permute(0, 2, 1).contiguous()
    d_src = otrain.aggregate_train(net, cm(inp["xyz_src"]), cm(inp["feat_src"]), inp["score_src"].cpu().to(F64))
    d_ref = otrain.aggregate_train(net, cm(inp["xyz_ref"]), cm(inp["feat_ref"]), inp["score_ref"].cpu().to(F64))
    for dd, dv in ((d_src, res["desc_src"]), (d_ref, res["desc_ref"])):
        assert float((dv.double().cpu() - dd.detach().permute(0, 2, 1)).abs().max()) < 1e-5
    loss, acc = otrain.det_des_loss(d_src, d_ref, cm(inp["xyz_src"]), cm(inp["xyz_ref"]), inp["score_ref"].cpu().to(F64), gt.cpu().to(F64), 0.6, 1.0)
    assert abs(res["loss"] - float(loss.detach())) <= 1e-5 * max(1.0, abs(float(loss.detach()))), (res["loss"], float(loss.detach()))
    loss.backward()
    l2, wk, mx = _compare_grads(tr.grads, {k: p.grad for k, p in params.items()}, "feat")
    for k, v in tr.buffers.items():
        w = net.p[k]
        assert float((v.double().cpu() - w).abs().max()) <= 1e-5 * float(w.abs().max()) + 1e-7, k
    print(f"SCALE feat num_sub={M}: worst relative L2 {l2:.2e} ({wk}), entry-wise {mx:.2e}")


# ------------------------------------------------------------------------------------------------------------------- operators
def _rnd(g, *s):
    return torch.randn(*s, generator=g, dtype=F64)


@pytest.mark.parametrize("clouds,M,C_,groups", [(1, 32768, 32, 4), (1, 32769, 32, 1), (1, 32769, 64, 64), (1, 288000, 16, 4),
                                                 (1, 288000, 8, 8), (3, 40000, 32, 4), (3, 40000, 64, 1), (3, 40000, 16, 16)])
def test_groupnorm_at_scale_against_fp64(clouds, M, C_, groups):
    """GroupNorm / BatchNorm (groups = C, one cloud) forward and backward with LeakyReLU where the row chunks stop being 128
    rows (32768 rows per cloud = 256 chunks, the cap) and at the level-0 neighbour layers of an 18000-point cloud (288 000
    rows); the last cloud's first group is nearly constant around 1 (var ~ 1e-6 << eps: rstd ~ 300 amplifies the rounding of
    the fp32 mean).  Entry-wise bounds from the fp32 error model: x^ = (y - mean) rstd carries dx = rstd u |mean| + 4 u |x^|;
    every output entry, every dY entry and every dgamma / dbeta entry stays within 4x what that propagates to.  LeakyReLU's
    branch is taken from the device output (a sign decided by rounding is no kernel error) and the entries where it differs
    from fp64 must be true near-zeros."""
    from deepsir_amd.train import _Ops
    o = _Ops(_dev())
    g = torch.Generator().manual_seed(M + C_ + groups)
    gw = C_ // groups
    y = _rnd(g, clouds, C_, M) * 2.0 + 0.5
    y[-1, :gw] = 1.0 + 1e-3 * _rnd(g, gw, M)
    y = y.float().double()                                                # fp32-representable: both sides see the same values
    ga = (torch.rand(C_, generator=g, dtype=F64) + 0.5).float().double()
    be = _rnd(g, C_).float().double()
    dout = _rnd(g, clouds, C_, M).float().double()
    pm = lambda t: t.permute(0, 2, 1).reshape(clouds * M, C_).float().contiguous().to(_dev())
    un = lambda t: t.double().cpu().reshape(clouds, M, C_).permute(0, 2, 1)
    gd, bd = ga.float().to(_dev()), be.float().to(_dev())
    out, stats = o.gn_fwd(pm(y), clouds, groups, gd, bd, True)
    dga, dbe = torch.zeros(C_, device=_dev()), torch.zeros(C_, device=_dev())
    dy = o.gn_bwd(pm(dout), pm(y), stats, clouds, groups, gd, bd, True, dga, dbe)
    torch.cuda.synchronize()
    out, dy, dga, dbe = un(out), un(dy), dga.double().cpu(), dbe.double().cpu()
    # fp64 reference (per cloud and group), the LeakyReLU branch as the device took it
    yg = y.reshape(clouds, groups, gw * M)
    mean = yg.mean(2, keepdim=True)
    rstd = 1.0 / torch.sqrt(yg.var(2, unbiased=False, keepdim=True) + 1e-5)
    grp = lambda t: t.reshape(clouds, groups, 1).repeat_interleave(gw, 1).reshape(clouds, C_, 1)
    mean_c, rstd_c = grp(mean), grp(rstd)
    xh = (y - mean_c) * rstd_c
    v = xh * ga[:, None] + be[:, None]
    flip = (v > 0) != (out > 0)
    assert bool((v[flip].abs() <= 1e-4 * float(v.abs().max())).all()), "a LeakyReLU branch differs away from zero"
    slope = torch.where(out > 0, 1.0, 0.2).to(F64)
    ref = v * slope
    dx = rstd_c * U32 * mean_c.abs() + 4 * U32 * xh.abs()
    bound = 4 * (ga.abs()[:, None] * dx + 4 * U32 * v.abs())
    assert bool(((out - ref).abs() <= bound).all()), float(((out - ref).abs() / bound).max())
    gg = dout * slope                                                     # d loss / d v
    gam = ga[:, None] * gg
    gmean = lambda t: grp(t.reshape(clouds, groups, gw * M).mean(2))
    m1, m2 = gmean(gam), gmean(gam * xh)
    ref_dy = rstd_c * (gam - m1 - xh * m2)
    bound_dy = 4 * rstd_c * (16 * U32 * (gam.abs() + gmean(gam.abs()) + xh.abs() * gmean((gam * xh).abs()))
                             + dx * m2.abs() + xh.abs() * gmean(gam.abs() * dx))
    assert bool(((dy - ref_dy).abs() <= bound_dy).all()), float(((dy - ref_dy).abs() / bound_dy).max())
    ref_dga, ref_dbe = (gg * xh).sum((0, 2)), gg.sum((0, 2))
    b_dga = 4 * ((gg.abs() * dx).sum((0, 2)) + 32 * U32 * (gg * xh).abs().sum((0, 2)))
    b_dbe = 4 * 32 * U32 * gg.abs().sum((0, 2))
    assert bool(((dga - ref_dga).abs() <= b_dga).all()), float(((dga - ref_dga).abs() / b_dga).max())
    assert bool(((dbe - ref_dbe).abs() <= b_dbe).all()), float(((dbe - ref_dbe).abs() / b_dbe).max())


@pytest.mark.parametrize("cin,cout", [(10, 8), (16, 16), (16, 32), (8, 32), (64, 128)])
def test_conv1x1_at_scale_against_fp64(cin, cout):
    """1x1 convolution at 288 000 rows (the level-0 neighbour layers of feat_len 4 at 18000 points, and 64 -> 128): forward, dX
    and dW / db (the row split of dsir_t_gemm_dw), each entry within 32 u of its fp64 absolute-value product (|X||W|^T,
    |dY||W|, |dY|^T|X|): a summation error bound, not a fit."""
    from deepsir_amd.train import _Ops
    o = _Ops(_dev())
    rows = 288000
    g = torch.Generator().manual_seed(cin * 1000 + cout)
    x, w, b, dy = (_rnd(g, *s).float() for s in ((rows, cin), (cout, cin), (cout,), (rows, cout)))
    xd, wd, bd, dyd = (t.to(_dev()) for t in (x, w, b, dy))
    y = o.conv(xd, wd, bd)
    dx = o.conv_dx(dyd, wd)
    dw, db = torch.zeros(cout, cin, device=_dev()), torch.zeros(cout, device=_dev())
    o.conv_dw(dyd, xd, dw, db)
    torch.cuda.synchronize()
    X, W, B, DY = (t.double() for t in (x, w, b, dy))
    checks = (("y", y, X @ W.t() + B, X.abs() @ W.abs().t() + B.abs(), cin + 1), ("dX", dx, DY @ W, DY.abs() @ W.abs(), cout),
              ("dW", dw, DY.t() @ X, DY.abs().t() @ X.abs(), 32), ("db", db, DY.sum(0), DY.abs().sum(0), 32))
    for name, got, want, absprod, c in checks:
        err = (got.double().cpu() - want).abs()
        assert bool((err <= c * U32 * absprod + 1e-30).all()), (name, float((err / absprod).max()) / U32)


def test_scatter_add_plan_at_scale_with_a_hub_row():
    """dsir_t_scatter_plan + dsir_t_scatter_add over 18000 x 16 gather entries of two clouds, one destination row receiving
    5000 sources (duplicate points do this to a neighbour index): every row is exactly the sequential fp32 sum of its sources
    in ascending source order, and within (sources) u of the fp64 sum of absolute values."""
    from deepsir_amd.train import _Ops
    o = _Ops(_dev())
    clouds, n, k, C_ = 2, N_PTS, 16, 24
    m = n * k
    g = torch.Generator().manual_seed(77)
    idx = torch.randint(0, n, (clouds, m), generator=g)
    hub = torch.randperm(m, generator=g)[:5000]
    idx[0, hub] = 4321
    idx[1, hub[:300]] = 0
    dy = torch.randn(clouds * m, C_ + 3, generator=g)
    got = o.scatter_add(dy.to(_dev()), 3, C_, idx.int().to(_dev()), n).cpu()
    o.new_step()
    assert torch.equal(o.scatter_add(dy.to(_dev()), 3, C_, idx.int().to(_dev()), n).cpu(), got)
    src = dy[:, 3:].reshape(clouds, m, C_)
    for c in range(clouds):
        # the sequential fp32 sum per destination in ascending source order, vectorised over destinations round by round
        order = torch.sort(idx[c] * m + torch.arange(m), stable=True)[1]
        dst = idx[c][order]
        start = torch.searchsorted(dst, torch.arange(n))
        cnt = torch.bincount(dst, minlength=n)
        assert int(cnt.max()) >= 5000 if c == 0 else int(cnt.max()) >= 300
        seq = torch.zeros(n, C_)
        for r in range(int(cnt.max())):
            rows = torch.nonzero(cnt > r).squeeze(1)
            seq[rows] += src[c][order[start[rows] + r]]
        assert torch.equal(got[c], seq), c
        s64 = torch.zeros(n, C_, dtype=F64).index_add_(0, idx[c], src[c].double())
        a64 = torch.zeros(n, C_, dtype=F64).index_add_(0, idx[c], src[c].double().abs())
        assert bool(((got[c].double() - s64).abs() <= cnt.double()[:, None] * U32 * a64).all())     # a sequential sum's bound


def test_maxpool_backward_with_exact_ties_follows_the_first_winner():
    """Max-pool over duplicated rows (equal values in different rows) and rows listed twice by one output: the forward's
    arg-max is the FIRST maximal entry in pool order (strictly greater replaces), the backward routes each output's gradient to
    that row only, once; the per-row sums equal fp64 sums of that routing, and the total gradient is conserved."""
    from deepsir_amd.train import _Ops
    o = _Ops(_dev())
    clouds, n, m, k, C_ = 2, 4000, 1000, 16, 32
    g = torch.Generator().manual_seed(91)
    x = torch.randn(clouds, n, C_, generator=g)
    x[:, n // 2:] = x[:, : n - n // 2]                                  # rows i and i + n/2 equal
    x[:, :, 5] = x[:, :, 5].round()                                      # channel 5: many equal values inside one pool
    pool = torch.randint(0, n, (clouds, m, k), generator=g)
    pool[:, :, 1] = (pool[:, :, 0] + n // 2) % n                          # a row and its duplicate side by side
    pool[:, ::7, 3] = pool[:, ::7, 2]                                    # a row listed twice by one output
    out, arg = o.maxpool_fwd(x.to(_dev()), pool.int().to(_dev()))
    dp = torch.randn(clouds, m, C_, generator=g)
    dx = o.maxpool_bwd(dp.to(_dev()), arg, pool.int().to(_dev()), n).cpu()
    vals = torch.gather(x, 1, pool.reshape(clouds, m * k, 1).expand(-1, -1, C_)).reshape(clouds, m, k, C_)
    mx = vals.max(dim=2)[0]
    first = (vals == mx[:, :, None, :]).int().argmax(dim=2)              # first maximal entry in pool order
    want_arg = torch.gather(pool[:, :, :, None].expand(-1, -1, -1, C_), 2, first[:, :, None, :]).squeeze(2)
    assert torch.equal(out.cpu(), mx)
    assert torch.equal(arg.cpu().long(), want_arg)
    assert int((vals == mx[:, :, None, :]).sum(2).gt(1).sum()) > 1000    # the ties are really there
    want = torch.zeros(clouds, n, C_, dtype=F64)
    want.scatter_add_(1, want_arg, dp.double())
    assert float((dx.double() - want).abs().max()) <= 8 * U32 * float(want.abs().max())
    assert torch.allclose(dx.double().sum(1), dp.double().sum(1), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("scale", [1.0, 50.0, 80.0])
def test_attentive_pooling_with_large_scores_against_fp64(scale):
    """Attentive pooling (softmax over the 16 neighbours, weighted sum) forward and backward with score magnitudes up to 80
    (exp overflows fp32 past 88: the softmax must subtract the maximum)."""
    from deepsir_amd.train import _Ops
    o = _Ops(_dev())
    pts, C_ = 20000, 48
    g = torch.Generator().manual_seed(int(scale))
    cat = torch.randn(pts, 16, C_, generator=g).float().double().requires_grad_()
    sc = (torch.randn(pts, 16, C_, generator=g) * scale).float()
    if scale > 1:
        sc = sc.clamp(-scale, scale)
        sc[::3] = scale * torch.sign(sc[::3])                             # ties at the top value
    sc = sc.double().requires_grad_()
    a = torch.softmax(sc, dim=1)
    ref = (cat * a).sum(1)
    dout = torch.randn(pts, C_, generator=g).float().double()
    ref.backward(dout)
    sd = sc.detach().float().reshape(pts * 16, C_).contiguous().to(_dev())
    cd = cat.detach().float().reshape(pts * 16, C_).contiguous().to(_dev())
    out = o.attpool_fwd(cd, sd, pts)
    dcat, ds = o.attpool_bwd(dout.float().to(_dev()), cd, sd, pts)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(ds).all())
    absref = (cat.detach().abs() * a.detach()).sum(1)
    assert bool(((out.double().cpu() - ref.detach()).abs() <= 64 * U32 * absref + 1e-30).all())
    assert float((sd.double().cpu().reshape(pts, 16, C_) - a.detach()).abs().max()) <= 64 * U32
    assert float((dcat.double().cpu().reshape(pts, 16, C_) - cat.grad).abs().max()) <= 64 * U32 * float(dout.abs().max())
    gs = ds.double().cpu().reshape(pts, 16, C_)
    bound = 64 * U32 * (a.detach() * (cat.detach().abs() + absref[:, None, :]) * dout.abs()[:, None, :])
    assert bool(((gs - sc.grad).abs() <= bound + 1e-30).all()), float(((gs - sc.grad).abs() / (bound + 1e-30)).max())
