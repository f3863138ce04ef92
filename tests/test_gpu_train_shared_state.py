"""``Network.train_step`` and the training-mode forward run on ONE training state whose buffers are the module's own tensors, so a
parameter changed in place between two ``train_step`` calls - no ``load_state_dict`` in between - is what the second one trains from.

net A: ``train_step`` (the state exists, one step of Adam moments), an in-place change of the trainable parameters - a plain
``p.mul_(1.01)``, or the reference loop's training forward + loss + ``backward()`` + ``torch.optim.Adam.step()`` -, then
``train_step(dropout_seed=s)``.  net B: a fresh ``Network`` loaded with A's ``state_dict()`` taken right after the change, then the same
``train_step(dropout_seed=s)``.  That step's loss and the gradient it leaves in the main trainer's flat buffer depend on the weights and
the masks alone, not on the Adam moments (A has a step of them, B none: the updated parameters differ and are not compared), so they
must be EQUAL: the training operators sum in one fixed order, and two runs of the same steps are byte-identical (losses, final
``state_dict()`` and Adam moments of four steps, every pipeline and ``frozen_mode``, measured when this test was written).

Sizes and fixtures are those of tests/test_gpu_train_interleave.py."""
import pytest
import torch

from test_gpu_train_interleave import N_ITER, _case, _dev, _forward, _loss, _net, _params

pytestmark = pytest.mark.gpu

SEED = 5


def _step(net, c, seed):
    data = dict(c["data"])
    if net.pipeline == "align":
        data["matches"] = c["matches"]
    if net.pipeline == "label":
        data["labels_src"], data["labels_ref"] = c["labels"]
    out = net.train_step(data, (N_ITER, False) if net.pipeline == "align" else None, dropout_seed=seed)
    assert not out["skipped"]
    return out["loss"]


@pytest.mark.parametrize("change", ["mul", "adam"])
@pytest.mark.parametrize("pipeline", ["align", "label", "feat"])
def test_train_step_trains_from_parameters_changed_in_place(pipeline, change):
    a = _net(pipeline)
    c = _case(pipeline, "A")
    _step(a, c, 0)
    before = {k: p.detach().clone() for k, p in _params(a).items()}
    if change == "mul":
        with torch.no_grad():
            for p in _params(a).values():
                p.mul_(1.01)
    else:
        opt = torch.optim.Adam(_params(a).values(), lr=1e-3)
        opt.zero_grad()
        _loss(a, _forward(a, c), c).backward()
        opt.step()
    assert all(not torch.equal(p.detach(), before[k]) for k, p in _params(a).items())
    b = _net(pipeline)
    b.load_state_dict(a.state_dict())
    loss_a, loss_b = _step(a, c, SEED), _step(b, c, SEED)
    assert loss_a == loss_b, f"{pipeline}/{change}: loss {loss_a!r} after the in-place change, {loss_b!r} from the same weights loaded afresh"
    tr_a, tr_b = a._tstate.main, b._tstate.main
    assert (tr_a.step_count, tr_b.step_count) == (2, 1)             # A kept its optimiser state through the change
    ga, gb = tr_a.grad_dict(), tr_b.grad_dict()
    assert set(ga) == set(gb) and any(float(abs(v).max()) > 0 for v in ga.values())
    bad = [k for k in ga if not (ga[k] == gb[k]).all()]
    assert not bad, f"{pipeline}/{change}: {len(bad)} of {len(ga)} gradients differ (first {bad[0]})"
    torch.cuda.synchronize()
