"""csrc/score.hip (torch.max(logits) + score_fun) and csrc/select.hip (top-k key points, scatter plan) at their decision boundaries,
against the plain references of tests/score_cases.py.  tests/test_score_host.py holds the float32 oracle and the selection
references to the same plain references on the CPU.

Score.  Labels are equal everywhere.  Off ``fragile`` (no point of a boundary case, at most 1 % of a random one) a point whose
reference score is zero - a closed gate, a zero label weight, pr <= 0.2 - scores exactly +-0, and the others agree within
``score_cases.SCORE_RTOL`` = 1.2e-6 relative, no absolute term: four times the 2.8e-7 (recorded as 3e-7) that the host test measures
for the float32 oracle against the float64 reference on these very cases, the factor because the kernel sums the 16 neighbour rows
before its single division; the cap of the stage tests (rtol 1e-4, atol 1e-6) is not reached.  (The kernel's own worst on an MI355X,
printed by the test and never fed back into the tolerance: 2.4e-7.)  Every call is repeated and must
return the same bits, and the per-cloud maxima of one call must not reach the next - neither through dsir_score, which presets
them per call, nor through dsir_forward_pair, which presets them in its opening launch.

Selection.  Index lists are integers: equal or not.  ``score_out`` is bit-equal to ``score[idx]``."""
import numpy as np
import pytest
import torch

import score_cases as S

pytestmark = pytest.mark.gpu

_ALL = S.all_cases()
_DEV = "cuda:0"


def _engine(**kw):
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    from deepsir_amd.weights import generate_state_dict
    e = Engine(NetConfig(**kw), 0, max_points=4608, max_pairs=5)
    e.load_state_dict(generate_state_dict(e.cfg, 0))              # dsir_score reads no weight, but every stage entry wants them loaded
    return e


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def ops():
    from deepsir_amd.train import _Ops
    return _Ops(torch.device(_DEV))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _score(eng, case):
    score, label = eng.score(*(torch.from_numpy(a).to(_DEV) for a in (case.feat, case.logits, case.xyz, case.neigh)))
    return score.cpu().numpy(), label.cpu().numpy()


@pytest.mark.parametrize("cid,case", _ALL, ids=[i for i, _ in _ALL])
def test_score_equals_plain(eng, cid, case):
    want, want_label, fragile = S.reference(cid)
    score, label = _score(eng, case)
    assert np.array_equal(label, want_label)
    assert np.isfinite(score).all()
    keep = ~fragile
    zero, rest = keep & (want == 0), keep & (want != 0)
    rel = np.abs(score.astype(np.float64) - want)[rest] / np.abs(want[rest])
    worst = float(rel.max()) if rest.any() else 0.0
    print(f"SCORE-GPU {cid}: worst relative deviation {worst:.3e} over {int(rest.sum())} points, {int(zero.sum())} zeros, "
          f"{int((score[zero] != 0).sum())} of them not zero, fragile {int(fragile.sum())}")
    assert (score[zero] == 0).all()
    assert (np.abs(score.astype(np.float64) - want)[rest] <= S.SCORE_ATOL + S.SCORE_RTOL * np.abs(want[rest])).all()
    score2, label2 = _score(eng, case)
    assert score2.tobytes() == score.tobytes() and label2.tobytes() == label.tobytes()


def test_a_call_does_not_see_the_maxima_of_the_one_before(eng):
    _, big, small = S.CASES["clouds_apart"]()
    _score(eng, big)
    after = _score(eng, small)
    fresh_engine = _engine()
    try:
        fresh = _score(fresh_engine, small)
    finally:
        fresh_engine.close()
    assert after[0].tobytes() == fresh[0].tobytes() and after[1].tobytes() == fresh[1].tobytes()
    assert (fresh[0] > 0).mean() > 0.3


def test_forward_pair_presets_its_maxima():
    """forward_pair(X) then forward_pair(Y) on one engine against forward_pair(Y) on a fresh one: score, index and label of Y are
    the same bits.  Three X of different extent go first; the teeth: on some cloud an X's largest logit exceeds Y's, so that a
    maximum left behind would change Y's pr."""
    n, num_sub = 1100, 300
    rng = np.random.default_rng(21)
    clouds = lambda scale: [torch.from_numpy((rng.uniform(-1.5, 1.5, (2, n, 3)) * scale).astype(np.float32)).to(_DEV) for _ in range(2)]
    xs, y = [clouds(s) for s in (0.3, 1.0, 5.0)], clouds(1.0)
    engines = [_engine(pipeline="feat", num_sub=num_sub) for _ in range(2)]
    try:
        top = [engines[0].forward_pair(x[0], x[1], num_sub) for x in xs]
        top = np.stack([np.stack([t[s]["logits"].cpu().numpy().max((1, 2)) for s in ("src", "ref")]) for t in top]).max(0)
        a, b = (e.forward_pair(y[0], y[1], num_sub) for e in engines)
        top_y = np.stack([b[s]["logits"].cpu().numpy().max((1, 2)) for s in ("src", "ref")])
        print(f"PRESET largest logit per cloud: before {top.ravel()} Y {top_y.ravel()}")
        assert (top > top_y).any()
        for s in ("src", "ref"):
            assert tuple(a[s]["index"].shape) == (2, num_sub)
            for k in ("score", "index", "label"):
                assert a[s][k].cpu().numpy().tobytes() == b[s][k].cpu().numpy().tobytes(), (s, k)
    finally:
        for e in engines:
            e.close()


# ----------------------------------------------------------------------------------------------------------------------- top-k
def _ks(n):
    return sorted({k for k in (1, n // 2, n - 1, n) if k >= 1})


def _check_topk(ops, s, label):
    t = torch.from_numpy(s).to(_DEV)
    n = s.shape[1]
    for k in _ks(n):
        idx, out = ops.topk(t, k)
        idx, out = idx.cpu().numpy(), out.cpu().numpy()
        assert idx.shape == (s.shape[0], k) and idx.dtype == np.int32
        assert np.array_equal(idx, S.plain_topk(s, k)), (label, k)
        assert np.array_equal(_bits(out), _bits(np.take_along_axis(s, idx.astype(np.int64), 1))), (label, k)


_TOPK_SHAPES = [(c, n) for n in (1, 2, 255, 256, 257, 1000, 4099, 20000) for c in (1, 2, 3, 64) if c < 64 or n <= 1000]


@pytest.mark.parametrize("clouds,n", _TOPK_SHAPES)
def test_topk_rule(ops, clouds, n):
    for pattern in S.TOPK_PATTERNS:
        _check_topk(ops, S.topk_scores(pattern, clouds, n), pattern)


def test_topk_of_tied_device_scores(eng, ops):
    """The score kernel's own output on every_label: the zero-weight classes are exact zeros of either sign, tied."""
    (case,) = S.CASES["every_label"]()
    score, _ = _score(eng, case)
    assert (score == 0).sum() >= 9
    _check_topk(ops, score, "every_label")
    _check_topk(ops, np.concatenate([score, -score, score[:, ::-1]]), "every_label x3")


@pytest.mark.parametrize("clouds,n", [(1, 1), (3, 257), (2, 4099)])
def test_topk_nan_rule(ops, clouds, n):
    """torch.sort's: a NaN of either sign before every number, NaNs among themselves in ascending index."""
    _check_topk(ops, S.nan_scores(clouds, n), "nan")


# ----------------------------------------------------------------------------------------------------------------- scatter plan
@pytest.mark.parametrize("n", [1, 2, 64, 65, 300])
@pytest.mark.parametrize("clouds", [1, 3])
@pytest.mark.parametrize("m", [1, 17, 4800])
def test_scatter_plan(ops, m, clouds, n):
    for pattern in S.PLAN_PATTERNS:
        idx = S.plan_index(pattern, clouds, m, n)
        ops.new_step()
        order, offsets = ops.plan(torch.from_numpy(idx).to(_DEV), n)
        want_order, want_offsets = S.plain_plan(idx, n)
        assert np.array_equal(offsets.cpu().numpy(), want_offsets), pattern
        assert np.array_equal(order.cpu().numpy(), want_order), pattern
    ops.new_step()
