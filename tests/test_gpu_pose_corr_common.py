"""What dsir_ransac_correspondence, dsir_consensus_correspondence and dsir_fgr_correspondence promise ALIKE, before and after their
own middles (csrc/pose_corr.hip, the shared head of csrc/entries_pose.hip, Engine's shared prologue): which calls are refused, and
that a refusal leaves the engine usable; the clamp flag, the counts, the parked rows, the row stride, the pair with no live row,
and that a pair's result does not depend on the batch it is in.  The estimators' own rules are pinned by test_gpu_ransac.py,
test_gpu_consensus.py and test_gpu_fgr.py; everything here is an equality of bytes, so there is no tolerance.

Shapes: 3 pairs of J = K = M = 64, strides 3 and 6, an engine of max_points = 1024."""
import numpy as np
import pytest
import torch

from deepsir_amd import ransac as R

pytestmark = pytest.mark.gpu
THR, P, M, MAX_POINTS, SEED = 0.05, 3, 64, 1024, 0x5EED
# Engine method -> its own keywords here, and whether it draws from a seed (pair p of a call with seed s is pair 0 of a call with
# seed s ^ (p << 40): the convention of test_gpu_ransac.py and test_gpu_fgr.py)
METHODS = {"ransac_correspondence": (dict(hypotheses=300), True), "consensus_correspondence": ({}, False),
           "fgr_correspondence": ({}, True)}
COUNTS = [64, 0, 200]                                             # all rows; none; more than M
T_INIT = np.tile(np.array([[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3]], np.float32), (P, 1, 1)) + np.arange(P, dtype=np.float32)[:, None, None]


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), max_points=MAX_POINTS, max_pairs=P)
    yield e
    e.close()


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _problems():
    """Pair 0 holds a row with both indices out of range, pair 2 a NaN and an infinite coordinate."""
    probs = [R.make_problem(M, 0.3, 0.005, 900 + p) for p in range(P)]
    probs[0]["corr"] = probs[0]["corr"].copy()
    probs[0]["corr"][3] = (-2, M + 9)
    probs[2]["src"][5, 1] = np.nan
    probs[2]["ref"][40, 2] = np.inf
    return probs


def _run(eng, method, pairs=range(P), counts=COUNTS, stride=3, T_init=None, seed=SEED):
    """One device call on the pairs ``pairs`` of the problem set, diagnostics on -> dict of numpy arrays."""
    kw, seeded = METHODS[method]
    probs = _problems()
    pad = lambda a: np.concatenate([a, np.full((a.shape[0], stride - 3), 7.0, np.float32)], 1)
    src = np.stack([pad(probs[p]["src"]) for p in pairs])
    ref = np.stack([pad(probs[p]["ref"]) for p in pairs])
    corr = np.stack([probs[p]["corr"] for p in pairs]).astype(np.int32)
    T, stats, invalid, d = getattr(eng, method)(_cuda(src), _cuda(ref), _cuda(corr), THR,
                                                counts=_cuda(np.asarray([counts[p] for p in pairs], np.int32)),
                                                T_init=None if T_init is None else _cuda(T_init[list(pairs)]), diag=True,
                                                **kw, **(dict(seed=seed) if seeded else {}))
    out = {k: v.cpu().numpy() for k, v in d.items()}
    out.update(T=T.cpu().numpy(), stats=stats.cpu().numpy(), invalid=invalid.cpu().numpy())
    return out


@pytest.fixture(scope="module")
def batch(eng):
    """The batch of three through every estimator, with and without T_init: computed once, read by every test."""
    return {(m, init): _run(eng, m, T_init=T_INIT if init else None) for m in METHODS for init in (False, True)}


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _assert_same(a, b, rows_a=slice(None), rows_b=slice(None)):
    assert a.keys() == b.keys()
    for k in a:
        assert _same_bits(a[k][rows_a], b[k][rows_b]), k


@pytest.mark.parametrize("method", METHODS)
def test_refusals_name_the_entry_and_leave_the_engine_usable(eng, batch, method):
    from deepsir_amd.engine import EngineError
    fn = getattr(eng, method)
    probs = _problems()
    x = _cuda(np.stack([p["src"] for p in probs]))
    y = _cuda(np.stack([p["ref"] for p in probs]))
    c = _cuda(np.stack([p["corr"] for p in probs]).astype(np.int32))
    i32 = dict(dtype=torch.int32, device="cuda")
    bad = [((x, y, c, md), {}) for md in (0.0, -1.0, float("nan"), float("inf"))]
    bad += [((x, y, c, THR), dict(refine_iters=r)) for r in (-1, 9)]
    bad += [((x, y, torch.zeros(P, MAX_POINTS + 1, 2, **i32), THR), {}),                       # M = max_points + 1
            ((x, y, torch.zeros(P, M, 3, **i32), THR), {}),                                    # corr [P,M,3]
            ((x, y, c, THR), dict(counts=torch.zeros(P - 1, **i32))),                          # counts [P-1]
            ((x, y, c, THR), dict(T_init=torch.zeros(P, 4, 4, device="cuda")))]                # T_init [P,4,4]
    for args, kw in bad:
        with pytest.raises(EngineError, match=method):
            fn(*args, **kw)
        _assert_same(_run(eng, method), batch[method, False])                                  # the same engine, the same bytes as before


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("init", [False, True])
def test_counts_and_the_pair_without_rows(eng, batch, method, init):
    out = batch[method, init]
    assert out["invalid"].tolist() == [2, 0, 0]                                                # the clamp in pair 0; NaNs raise nothing
    assert np.isfinite(out["T"]).all() and np.isfinite(out["stats"]).all()
    assert _same_bits(out["T"][1], T_INIT[1] if init else R.IDENTITY) and out["stats"][1].tolist() == [0, 0, -1, 0, 0]
    assert out["stats"][0][4] > 0 and out["stats"][2][4] > 0                                   # the other two found a pose
    clamped = _run(eng, method, counts=[64, 0, M], T_init=T_INIT if init else None)            # counts above M act as M
    _assert_same(out, clamped)


def test_invalid_is_the_same_for_all_three(batch):
    first = batch["ransac_correspondence", False]["invalid"]
    for key, out in batch.items():
        assert _same_bits(out["invalid"], first), key


@pytest.mark.parametrize("method", METHODS)
def test_stride_6_is_stride_3(eng, batch, method):
    _assert_same(_run(eng, method, stride=6), batch[method, False])


@pytest.mark.parametrize("method", METHODS)
def test_a_batch_is_its_single_pairs(eng, batch, method):
    for p in range(P):
        one = _run(eng, method, pairs=[p], T_init=T_INIT, seed=SEED ^ (p << 40))
        _assert_same(batch[method, True], one, rows_a=slice(p, p + 1))
