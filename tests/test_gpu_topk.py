"""dsir_nn_match_topk and dsir_feature_correspondences_ex (csrc/nn_topk.hip) against the rule its header states: rank 0 is
dsir_nn_match's result bit for bit, keys ascend, a smaller k is a prefix, pairs are independent, runs repeat, and outside the
host's band (deepsir_amd/match.py) the indices are the float64 order's.  The correspondence entry is compared, bit for bit, with
the host compaction applied to the device's own lists.

Shapes: (1, 1) (every rank beyond 0 padded), (65, 300) (two row blocks of 64, a ragged last column tile), (512, 512), and 16 rows
against a column range long enough for the launcher to split it (K placed 37 columns past a tile boundary).  Unit-norm random
descriptors; up to half of the src rows have a noisy copy among the ref columns so that mutual and ratio tests keep some rows and drop others."""
import numpy as np
import pytest
import torch

from deepsir_amd import match as Mt

pytestmark = pytest.mark.gpu
MAX_POINTS = 5120
KS = (1, 2, 3, 8)


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), max_points=MAX_POINTS, max_pairs=4)
    yield e
    e.close()


def _unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def _descs(J, K, seed, P=2):
    rng = np.random.default_rng(seed)
    a = _unit(rng.normal(size=(P, J, 64)))
    b = _unit(rng.normal(size=(P, K, 64)))
    n = min(J, K // 3) // 2
    for p in range(P):                                      # noisy copies of src rows at random columns
        cols, rows = rng.permutation(K)[:n], rng.permutation(J)[:n]
        b[p, cols] = _unit(a[p, rows] + 0.02 * rng.normal(size=(n, 64)))
    return a, b


_CASES = {}


def _split_K(eng):
    K = 2048
    while eng.nn_match_topk_splits(2, 16, K, 8) < 2 and K < MAX_POINTS - 64:
        K += 512
    return K + 37


def _case(eng, name):
    """Descriptors, the device's k = 8 lists and the host's, computed once per shape."""
    if name not in _CASES:
        J, K = {"1x1": (1, 1), "65x300": (65, 300), "512x512": (512, 512), "16xsplit": (16, None)}[name]
        if K is None:
            K = _split_K(eng)
        a, b = _descs(J, K, seed=J * 7 + K)
        ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        idx8, dist8 = eng.nn_match_topk(ta, tb, 8)
        D = np.stack([((a[p].astype(np.float64) ** 2).sum(1)[:, None] - 2.0 * a[p].astype(np.float64) @ b[p].astype(np.float64).T)
                      + (b[p].astype(np.float64) ** 2).sum(1)[None, :] for p in range(2)])
        _CASES[name] = dict(J=J, K=K, a=a, b=b, ta=ta, tb=tb, idx8=idx8.cpu().numpy(), dist8=dist8.cpu().numpy(), D=D,
                            nn=eng.nn_match(ta, tb).cpu().numpy(), nns=eng.nn_match_screened(ta, tb)[0].cpu().numpy())
    return _CASES[name]


def _order_bits(d):
    u = np.ascontiguousarray(d, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xffffffff), u | np.uint64(0x80000000))


def _same(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


SHAPES = ("1x1", "65x300", "512x512", "16xsplit")


def test_the_long_shape_is_split(eng):
    c = _case(eng, "16xsplit")
    assert c["K"] % 64 == 37
    assert eng.nn_match_topk_splits(2, 16, c["K"], 8) >= 2 and eng.nn_match_topk_splits(2, 16, c["K"], 1) >= 2


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", SHAPES)
def test_topk_rule(eng, name, k):
    c = _case(eng, name)
    J, K = c["J"], c["K"]
    idx_t, dist_t = eng.nn_match_topk(c["ta"], c["tb"], k)
    idx, dist = idx_t.cpu().numpy(), dist_t.cpu().numpy()
    assert idx.shape == (2, J, k) and idx.dtype == np.int32 and dist.dtype == np.float32
    # rank 0 is the arg-min entries' result
    assert _same(idx[..., 0], c["nn"]) and _same(idx[..., 0], c["nns"])
    # ranks beyond K are padded, the others hold a column
    m = min(k, K)
    assert (idx[..., :m] >= 0).all() and (idx[..., :m] < K).all() and (idx[..., m:] == -1).all() and np.isposinf(dist[..., m:]).all()
    # keys ascend strictly along k
    key = (_order_bits(dist[..., :m]) << np.uint64(32)) | idx[..., :m].astype(np.uint64)
    assert (key[..., 1:] > key[..., :-1]).all()
    # the result for k is the prefix of the result for 8
    assert _same(idx, c["idx8"][..., :k]) and _same(dist, c["dist8"][..., :k])
    # two runs give the same bytes; without distances the indices are the same
    idx2, dist2 = eng.nn_match_topk(c["ta"], c["tb"], k)
    assert _same(idx2.cpu().numpy(), idx) and _same(dist2.cpu().numpy(), dist)
    idx3, none = eng.nn_match_topk(c["ta"], c["tb"], k, with_dist=False)
    assert none is None and _same(idx3.cpu().numpy(), idx)
    worst, in_band = 0.0, 0
    for p in range(2):
        # pair p of the batch equals the same pair alone
        ia, da = eng.nn_match_topk(c["ta"][p:p + 1].contiguous(), c["tb"][p:p + 1].contiguous(), k)
        assert _same(ia.cpu().numpy()[0], idx[p]) and _same(da.cpu().numpy()[0], dist[p])
        # against the host: equal indices on every row outside the band
        hidx, hdist, band = Mt.topk_host(c["a"][p], c["b"][p], k)
        in_band += int(band.sum())
        assert np.array_equal(idx[p][~band], hidx[~band])
        # the distance belongs to the column the device reports
        want = np.take_along_axis(c["D"][p], idx[p][:, :m].astype(np.int64), 1)
        worst = max(worst, float(np.abs(dist[p][:, :m].astype(np.float64) - want).max()))
    print(f"TOPK {name} k={k}: band rows {in_band} of {2 * J}, worst |dist - float64| {worst:.2e}")
    assert in_band <= 0.01 * 2 * J
    assert worst <= 2e-6


def test_exact_ties_go_to_the_lower_column(eng):
    c = _case(eng, "65x300")
    b = c["b"].copy()
    for p, row in ((0, 7), (1, 64)):
        b[p, [10, 40, 299]] = c["a"][p, row]
    idx, dist = eng.nn_match_topk(c["ta"], torch.from_numpy(b).cuda(), 8)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    for p, row in ((0, 7), (1, 64)):
        assert idx[p, row, :3].tolist() == [10, 40, 299]
        assert _same(dist[p, row, 0:1], dist[p, row, 1:2]) and _same(dist[p, row, 0:1], dist[p, row, 2:3])
        assert abs(float(dist[p, row, 0])) < 2e-6 and dist[p, row, 3] > 1e-3
    assert _same(idx[..., 0], eng.nn_match(c["ta"], torch.from_numpy(b).cuda()).cpu().numpy())


def test_k_beyond_K_pads(eng):
    c = _case(eng, "1x1")
    assert c["idx8"].shape == (2, 1, 8)
    assert (c["idx8"][..., 0] == 0).all() and (c["idx8"][..., 1:] == -1).all()
    assert np.isfinite(c["dist8"][..., 0]).all() and np.isposinf(c["dist8"][..., 1:]).all()


# ---------------------------------------------------------------------------------------------------------- correspondences
@pytest.mark.parametrize("mutual", [True, False])
@pytest.mark.parametrize("name", ["65x300", "512x512", "16xsplit"])
def test_ex_with_k1_and_no_ratio_is_the_old_entry(eng, name, mutual):
    c = _case(eng, name)
    corr, counts = eng.feature_correspondences(c["ta"], c["tb"], mutual=mutual)
    # through the new C entry itself (the Python method keeps calling the old one for these arguments)
    corr2 = torch.empty_like(corr)
    counts2 = torch.empty_like(counts)
    eng._pre()
    eng._call(eng.lib.dsir_feature_correspondences_ex(eng.h, c["ta"].data_ptr(), c["tb"].data_ptr(), 2, c["J"], c["K"], int(mutual), 1, 0.0,
                                                      corr2.data_ptr(), counts2.data_ptr(), None))
    eng.sync()
    assert _same(corr2.cpu().numpy(), corr.cpu().numpy()) and _same(counts2.cpu().numpy(), counts.cpu().numpy())
    # and through the top-k path (with distances): the same list
    corr3, counts3, dist3 = eng.feature_correspondences(c["ta"], c["tb"], mutual=mutual, with_dist=True)
    assert _same(corr3.cpu().numpy(), corr.cpu().numpy()) and _same(counts3.cpu().numpy(), counts.cpu().numpy())
    assert int(counts.min()) > 0
    if mutual and name != "16xsplit":
        assert int(counts.max()) < c["J"]                                             # the mutual test keeps some, drops some


@pytest.mark.parametrize("mutual,k,ratio", [(True, 2, 0.0), (False, 3, 0.0), (True, 8, 0.0), (False, 8, 0.0), (True, 1, 0.8),
                                            (False, 1, 0.8), (True, 1, 0.97), (False, 1, 0.3)])
@pytest.mark.parametrize("name", ["1x1", "65x300", "512x512", "16xsplit"])
def test_ex_is_the_host_compaction_of_the_device_lists(eng, name, mutual, k, ratio):
    c = _case(eng, name)
    J, K = c["J"], c["K"]
    corr, counts, dist = eng.feature_correspondences(c["ta"], c["tb"], mutual=mutual, k=k, ratio=ratio, with_dist=True)
    corr, counts, dist = corr.cpu().numpy(), counts.cpu().numpy(), dist.cpu().numpy()
    assert corr.shape == (2, J * k, 2) and dist.shape == (2, J * k)
    iba, _ = eng.nn_match_topk(c["tb"], c["ta"], k, with_dist=False)
    iba = iba.cpu().numpy()
    kept = []
    for p in range(2):
        wcorr, wcount, wdist = Mt.correspondences_from_topk(c["idx8"][p], c["dist8"][p], iba[p], mutual, k, ratio)
        assert counts[p] == wcount
        assert _same(corr[p], wcorr) and _same(dist[p], wdist)
        kept.append(wcount)
    print(f"EX {name} mutual={mutual} k={k} ratio={ratio}: kept {kept} of {J * k}")
    if ratio > 0 and name in ("65x300", "512x512"):
        assert 0 < min(kept) and max(kept) < J                         # the ratio test is exercised both ways
    # without distances: the same list
    corr2, counts2 = eng.feature_correspondences(c["ta"], c["tb"], mutual=mutual, k=k, ratio=ratio)
    assert _same(corr2.cpu().numpy(), corr) and _same(counts2.cpu().numpy(), counts)


def test_refusals_leave_the_engine_usable(eng):
    from deepsir_amd.engine import EngineError
    c = _case(eng, "65x300")
    want = eng.feature_correspondences(c["ta"], c["tb"], k=2)[0].cpu().numpy()
    big = torch.zeros((1, 1024, 64), device="cuda")
    for kw, src, ref, word in ((dict(k=0), c["ta"], c["tb"], "k=0"), (dict(k=9), c["ta"], c["tb"], "k=9"),
                               (dict(ratio=1.0), c["ta"], c["tb"], "ratio"), (dict(k=2, ratio=0.5), c["ta"], c["tb"], "1-NN"),
                               (dict(ratio=float("nan")), c["ta"], c["tb"], "ratio"), (dict(k=8), big, big, "max_points")):
        with pytest.raises(EngineError, match=word):
            eng.feature_correspondences(src, ref, **kw)
        assert _same(eng.feature_correspondences(c["ta"], c["tb"], k=2)[0].cpu().numpy(), want)
    for k in (0, 9):
        with pytest.raises(EngineError, match=f"k={k}"):
            eng.nn_match_topk(c["ta"], c["tb"], k)
    too_long = torch.zeros((1, MAX_POINTS + 1, 64), device="cuda")
    with pytest.raises(EngineError, match="max_points"):
        eng.nn_match_topk(c["ta"][:1].contiguous(), too_long, 2)
    assert _same(eng.nn_match_topk(c["ta"], c["tb"], 8)[0].cpu().numpy(), c["idx8"])
