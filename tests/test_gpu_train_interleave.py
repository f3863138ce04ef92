"""Training forwards and backwards of the drop-in ``Network`` in orders other than the reference loop's one forward, one backward.

torch's autograd gives every tape its own gradient and adds them into ``param.grad``: with gA and gB the gradients of two
isolated forward-backward passes A and B, every order below must leave ``param.grad == gA + gB`` - bit for bit, since the
training operators sum in one fixed order (no float atomics) and torch adds the two fp32 tensors exactly as it accumulates them:

1. F_A, B_A, F_B, B_B (gradient accumulation over two batches);
2. F_A, F_B, B_A, B_B;
3. F_A, F_B, (loss_A + loss_B).backward();
4. F_A, an evaluation-mode forward under ``torch.no_grad()``, B_A (gradient gA alone);
5. F_A at 1024 points, F_C at 2048 points (the training engine grows), then the loss and backward of A, then of C.

Small clouds, one pair, fixed Dropout masks (``Network.dropout_masks``), one ``Network`` per pipeline (no optimiser step: the
weights, hence the gradients, stay put; the BatchNorm running statistics move but training mode reads batch statistics)."""
import numpy as np
import pytest
import torch

from test_train_loop import _args

pytestmark = pytest.mark.gpu

N_ITER = 2
SIZES = {"A": 1024, "B": 1357, "C": 2048}


def _dev():
    return torch.device("cuda", 0)


def _net(pipeline):
    from deepsir_amd.model import Network
    from deepsir_amd.weights import generate_state_dict, to_torch_state_dict
    net = Network(_args(pipeline, num_sub=256 if pipeline == "feat" else -1, num_reg_iter=N_ITER))
    sd = generate_state_dict(net.cfg, 8, "plain" if pipeline == "label" else "separated")
    net.load_state_dict(to_torch_state_dict(sd))
    net.to(_dev())
    net.train()
    return net


def _case(pipeline, name):
    from deepsir_amd.synth import make_pair
    from deepsir_amd.train import dropout_keep_masks
    n = SIZES[name]
    seed = 900 + n
    raw = make_pair(n, seed, 3)
    d = {k: torch.from_numpy(raw[k]).to(_dev()) for k in ("points_src", "points_ref", "transform_gt")}
    if pipeline == "feat":
        d["transform_gt"][:, :, 3] += 2e-3                     # off the exact-coincidence knife edge
    g = torch.Generator().manual_seed(seed)
    labels = [torch.randint(0, 20, (1, n), generator=g) for _ in range(2)]
    rng = np.random.Generator(np.random.Philox(key=seed))
    matches = [np.stack([np.arange(n), np.where(rng.random(n) < 0.7, np.arange(n), rng.integers(0, n, n))], 1)]
    masks = {"fe_src": dropout_keep_masks(3 * seed + 1, (1, n, 64), _dev()), "fe_ref": dropout_keep_masks(3 * seed + 2, (1, n, 64), _dev()),
             "inlier": dropout_keep_masks(3 * seed, (N_ITER, 1, n, 64), _dev())}
    return {"data": d, "labels": labels, "matches": matches, "masks": masks}


def _forward(net, c):
    net.dropout_masks = c["masks"]
    _, ep = net(c["data"], (N_ITER, False) if net.pipeline == "align" else None)
    return ep


def _loss(net, ep, c):
    ep["transform_gt"] = c["data"]["transform_gt"]
    if net.pipeline == "align":
        ep["matches"] = c["matches"]
        return net.loss_align_fun(ep, reduction="mean")["total"]
    if net.pipeline == "label":
        ep["labels_src"], ep["labels_ref"] = c["labels"]
        return net.loss_label_fun(ep)[0]
    return net.loss_feat_fun(ep)[0]


def _params(net):
    return {k: p for k, p in net.named_parameters() if p.requires_grad}


def _zero(net):
    for p in net.parameters():
        p.grad = None


def _grads(net):
    out = {}
    for k, p in _params(net).items():
        assert p.grad is not None, k
        out[k] = p.grad.detach().clone()
    return out


def _isolated(net, c):
    _zero(net)
    _loss(net, _forward(net, c), c).backward()
    return _grads(net)


def _assert_equal(net, want, order):
    got = _grads(net)
    assert set(got) == set(want)
    bad = [k for k in want if not torch.equal(got[k], want[k])]
    worst = max((float((got[k] - want[k]).abs().max() / (want[k].abs().max() + 1e-30)) for k in bad), default=0.0)
    assert not bad, f"order {order}: {len(bad)} of {len(want)} tensors differ from gA + gB (worst relative {worst:.3e}; first {bad[0]})"


_CTX = {}


def _ctx(pipeline):
    """One network per pipeline with the isolated gradients gA, gB, gC (deterministic: the same inputs and masks give the
    same bits - checked once)."""
    if pipeline not in _CTX:
        net = _net(pipeline)
        cases = {k: _case(pipeline, k) for k in "ABC"}
        g = {k: _isolated(net, c) for k, c in cases.items()}
        again = _isolated(net, cases["A"])
        assert all(torch.equal(v, again[k]) for k, v in g["A"].items()), "an isolated pass is not reproducible"
        assert any(float(v.abs().max()) > 0 for v in g["A"].values())
        _CTX[pipeline] = (net, cases, g)
    return _CTX[pipeline]


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("pipeline", ["align", "label", "feat"])
def test_interleaved_training_passes_accumulate_like_autograd(pipeline, order):
    net, cs, g = _ctx(pipeline)
    A, B = cs["A"], cs["B"]
    want = {k: g["A"][k] + g["B"][k] for k in g["A"]}
    if order == 1:                                   # F_A, B_A, F_B, B_B
        _zero(net)
        _loss(net, _forward(net, A), A).backward()
        _loss(net, _forward(net, B), B).backward()
    elif order == 2:                                 # F_A, F_B, B_A, B_B
        _zero(net)
        ep_a, ep_b = _forward(net, A), _forward(net, B)
        _loss(net, ep_a, A).backward()
        _loss(net, ep_b, B).backward()
    elif order == 3:                                 # F_A, F_B, (loss_A + loss_B).backward()
        _zero(net)
        ep_a, ep_b = _forward(net, A), _forward(net, B)
        (_loss(net, ep_a, A) + _loss(net, ep_b, B)).backward()
    elif order == 4:                                 # F_A, an evaluation-mode forward without gradients, B_A
        _zero(net)
        ep_a = _forward(net, A)
        net.eval()
        with torch.no_grad():
            net(B["data"], (N_ITER, False) if pipeline == "align" else None)
        net.train()
        _loss(net, ep_a, A).backward()
        want = g["A"]
    else:                                            # a fresh network (training engine at 1024 points): C's forward grows it
        net = _net(pipeline)
        C = cs["C"]
        ep_a = _forward(net, A)
        ep_c = _forward(net, C)
        assert net._tstate.engine.max_points >= SIZES["C"]
        _loss(net, ep_a, A).backward()
        _loss(net, ep_c, C).backward()
        want = {k: g["A"][k] + g["C"][k] for k in g["A"]}
    _assert_equal(net, want, order)
    torch.cuda.synchronize()


@pytest.mark.parametrize("pipeline", ["align", "label"])
def test_second_backward_through_a_used_tape_is_refused(pipeline):
    net, cs, _ = _ctx(pipeline)
    A = cs["A"]
    ep = _forward(net, A)
    _loss(net, ep, A).backward()
    lo = _loss(net, ep, A)                           # a new loss node on the same forward's outputs
    with pytest.raises(RuntimeError, match="tape has been used"):
        lo.backward()
    torch.cuda.synchronize()
