"""The two-row-tile instantiations of the exact descriptor search - nn_match_kernel<2>, nn_topk_kernel<2, 2> and <4, 2>
(csrc/exact_search_body.h is their common tile walk) - at the smallest shapes that reach them: the launchers take two row tiles per
wave from pairs x ceil(J / 128) >= 256 (csrc/search_plan.h; tools/search_plan_check.cpp pins rt = 2 at exactly these shapes).  The
oracle is the one-row-tile kernel, which a single pair of the same batch takes: equality is exact, byte for byte.

Arg-min: 128 pairs x J = 129 x K = 70 - the second 128-row block holds one live row, the one column tile is ragged.
Top-k:   64 pairs x J = 385 x K = 70 - k = 2 / 4 run <2, 2> / <4, 2>, k = 8 runs <8, 1> on the same data."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C_INF, C_LOW, C_HIGH, ROW_DUP = 33, 20, 50, 5      # pair 0 of the arg-min batch: a +inf ref column, two identical ref columns


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), max_points=1024, max_pairs=128)
    yield e
    e.close()


def _unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def _same(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def _argmin_batch():
    """Descriptors of the arg-min batch and the float64 reference: (a, b, ref index, rows the reference decides)."""
    P, J, K = 128, 129, 70
    rng = np.random.default_rng(129070)
    a, b = _unit(rng.normal(size=(P, J, 64))), _unit(rng.normal(size=(P, K, 64)))
    b[0, C_LOW] = a[0, ROW_DUP]
    b[0, C_HIGH] = a[0, ROW_DUP]
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    D = (a64 ** 2).sum(2)[:, :, None] - 2.0 * a64 @ b64.transpose(0, 2, 1) + (b64 ** 2).sum(2)[:, None, :]
    D[0, :, C_INF] = np.inf                                   # the rule: a +inf distance never wins
    part = np.partition(D, 1, axis=2)
    clear = part[:, :, 1] - part[:, :, 0] > 1e-5              # the rule of test_nn_match_properties_full_size
    clear[0, J - 1] = False                                   # the all-NaN row has no float64 answer
    a[0, J - 1] = np.nan
    b[0, C_INF] = np.inf
    return a, b, D.argmin(2), clear


def test_argmin_two_row_tiles(eng):
    a, b, ref, clear = _argmin_batch()
    P, J, K = a.shape[0], a.shape[1], b.shape[1]
    assert P * ((J + 127) // 128) == 256                      # the threshold itself
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    idx = eng.nn_match(ta, tb).cpu().numpy()
    assert idx.shape == (P, J) and idx.dtype == np.int32
    # a pair alone takes one row tile per wave: the same bytes
    for p in (0, 1, 63, 127):
        alone = eng.nn_match(ta[p:p + 1].contiguous(), tb[p:p + 1].contiguous()).cpu().numpy()
        assert _same(alone[0], idx[p]), f"pair {p}"
    # edge rows of pair 0
    assert idx[0, J - 1] == 0                                 # all-NaN row: nothing ever wins, index 0
    assert (idx[0] != C_INF).all()
    assert idx[0, ROW_DUP] == C_LOW                           # exact tie: the lower column
    assert (idx >= 0).all() and (idx < K).all()
    # float64 arg-min wherever it decides; the reference alone leaves out at most 1 % of the rows
    left_out = 1.0 - float(clear.mean())
    print(f"RT2 argmin: float64 reference leaves out {int((~clear).sum())} of {clear.size} rows ({100 * left_out:.3f} %)")
    assert left_out <= 0.01
    assert np.array_equal(idx[clear], ref[clear])


def _topk_batch(K):
    rng = np.random.default_rng(385000 + K)
    return _unit(rng.normal(size=(64, 385, 64))), _unit(rng.normal(size=(64, K, 64)))


def test_topk_two_row_tiles(eng):
    a, b = _topk_batch(70)
    P, J = a.shape[0], a.shape[1]
    assert P * ((J + 127) // 128) == 256
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    idx8, dist8 = (t.cpu().numpy() for t in eng.nn_match_topk(ta, tb, 8))
    nn = eng.nn_match(ta, tb).cpu().numpy()
    assert _same(idx8[..., 0], nn)
    for k in (2, 4):
        idx, dist = (t.cpu().numpy() for t in eng.nn_match_topk(ta, tb, k))
        assert idx.shape == (P, J, k)
        # the two-row-tile kernel's lists are the prefix of the one-row-tile kernel's
        assert _same(idx, idx8[..., :k]) and _same(dist, dist8[..., :k]), f"k={k}"
        assert _same(idx[..., 0], nn)
        for p in (0, 63):                                     # a pair alone: one row tile per wave
            ia, da = (t.cpu().numpy() for t in eng.nn_match_topk(ta[p:p + 1].contiguous(), tb[p:p + 1].contiguous(), k))
            assert _same(ia[0], idx[p]) and _same(da[0], dist[p]), f"k={k} pair {p}"


def test_topk_two_row_tiles_k_beyond_K_pads(eng):
    """test_k_beyond_K_pads's rule at K = 3: ranks below K hold a column, the others index -1 and distance +inf."""
    a, b = _topk_batch(3)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    idx8, dist8 = (t.cpu().numpy() for t in eng.nn_match_topk(ta, tb, 8))
    for k in (4, 8):
        idx, dist = (t.cpu().numpy() for t in eng.nn_match_topk(ta, tb, k))
        assert (idx[..., :3] >= 0).all() and (idx[..., :3] < 3).all() and (idx[..., 3:] == -1).all()
        assert np.isfinite(dist[..., :3]).all() and np.isposinf(dist[..., 3:]).all()
        assert (np.sort(idx[..., :3], axis=-1) == np.arange(3)).all()        # every column once
        assert _same(idx, idx8[..., :k]) and _same(dist, dist8[..., :k])
    idx2, dist2 = (t.cpu().numpy() for t in eng.nn_match_topk(ta, tb, 2))
    assert _same(idx2, idx8[..., :2]) and _same(dist2, dist8[..., :2])
