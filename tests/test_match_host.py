"""deepsir_amd/match.py, the host restatement of the top-k descriptor search (csrc/nn_topk.hip), and the three C-ABI entries it
restates (no GPU here: exports and bindings only)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from deepsir_amd import match as Mt
from deepsir_amd import ransac as R

NEW = ("dsir_nn_match_topk", "dsir_nn_match_topk_splits", "dsir_feature_correspondences_ex")


def _plain_topk(a, b, k):
    """The rule spelt out with Python's sort: ascending (distance, index)."""
    idx = np.full((len(a), k), -1, np.int32)
    dist = np.full((len(a), k), np.inf)
    for j, x in enumerate(a):
        d = [(float((x.astype(np.float64) ** 2).sum() - 2.0 * x.astype(np.float64) @ y.astype(np.float64)
                    + (y.astype(np.float64) ** 2).sum()), c) for c, y in enumerate(b)]
        for r, (dv, c) in enumerate(sorted(d)[:k]):
            idx[j, r], dist[j, r] = c, dv
    return idx, dist


@pytest.mark.parametrize("J,K,k", [(5, 7, 1), (9, 13, 3), (4, 20, 8), (3, 2, 2)])
def test_topk_host_against_a_plain_sort(J, K, k):
    rng = np.random.default_rng(J * 100 + K)
    a = rng.normal(size=(J, 8)).astype(np.float32)
    b = rng.normal(size=(K, 8)).astype(np.float32)
    idx, dist, band = Mt.topk_host(a, b, k)
    widx, wdist = _plain_topk(a, b, k)
    assert idx.dtype == np.int32 and idx.shape == (J, k) and band.shape == (J,)
    assert np.array_equal(idx, widx)
    assert np.allclose(dist, wdist, rtol=0, atol=1e-12)
    assert not band.any()                                   # random normal rows: gaps far above 1e-5


def test_topk_host_ties_go_to_the_lower_index_and_set_the_band():
    a = np.eye(4, dtype=np.float32)[:2]
    b = np.stack([np.eye(4, dtype=np.float32)[i] for i in (1, 0, 1, 0, 2, 0)])   # row 0 ties at columns 1, 3, 5; row 1 at 0, 2
    idx, dist, band = Mt.topk_host(a, b, 3)
    assert idx[0].tolist() == [1, 3, 5] and (dist[0] == 0.0).all()
    assert idx[1].tolist() == [0, 2, 1] and dist[1].tolist() == [0.0, 0.0, 2.0]
    assert band.all()


def test_topk_host_band_looks_one_rank_past_k():
    a = np.array([[1.0, 0.0]], np.float32)
    b = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 1.0 + 1e-7]], np.float32)
    assert not Mt.topk_host(a, b[:2], 1)[2][0]
    assert Mt.topk_host(a, b, 2)[2][0]                       # ranks 1 and 2 within 1e-5: which one is rank 1 is the device's call
    assert not Mt.topk_host(a, b, 1)[2][0]                   # k = 1 reads ranks 0 and 1 only


def test_topk_host_pads_beyond_K():
    a = np.ones((2, 4), np.float32)
    b = np.zeros((1, 4), np.float32)
    idx, dist, band = Mt.topk_host(a, b, 8)
    assert (idx[:, 0] == 0).all() and (idx[:, 1:] == -1).all()
    assert (dist[:, 0] == 4.0).all() and np.isposinf(dist[:, 1:]).all()
    assert not band.any()


def test_ratio_keep_corners():
    f = np.float32
    assert Mt.ratio_keep([0.1], None, 0.8).all()                                    # no rank 1 at all
    assert Mt.ratio_keep([0.1], [np.inf], 0.8).all()                                # rank 1 missing (K == 1)
    assert not Mt.ratio_keep([0.0], [0.0], 0.8).any()                               # duplicated ref descriptors: strict comparison
    assert Mt.ratio_keep([-1e-7], [1e-3], 0.8).all()                                # a negative d0 (fp32 cancellation) clamps to 0
    assert not Mt.ratio_keep([-1e-7], [-1e-8], 0.8).any()                           # both clamp to 0
    assert Mt.ratio_keep([5.0], [1.0], 0.0).all() and Mt.ratio_keep([5.0], [1.0], -1.0).all()   # ratio <= 0: no test
    # the fp32 rule exactly: r2 = fp32(0.8 * 0.8), one multiply, strict
    r2 = f(f(0.8) * f(0.8))
    d1 = f(1.5)
    edge = f(r2 * d1)
    assert not Mt.ratio_keep([edge], [d1], 0.8)[0]
    assert Mt.ratio_keep([np.nextafter(edge, f(0))], [d1], 0.8)[0]
    assert Mt.ratio_r2(0.8) == r2
    for bad in (1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            Mt.ratio_keep([0.1], [0.2], bad)


@pytest.mark.parametrize("mutual", [True, False])
def test_correspondences_from_topk_k1_is_the_mutual_nearest_neighbour_list(mutual):
    rng = np.random.default_rng(3)
    a = rng.normal(size=(40, 16)).astype(np.float32)
    b = np.concatenate([a[rng.permutation(40)[:25]] + 0.01 * rng.normal(size=(25, 16)), rng.normal(size=(12, 16))]).astype(np.float32)
    iab, dab, _ = Mt.topk_host(a, b, 1)
    iba, _, _ = Mt.topk_host(b, a, 1)
    corr, count, dist = Mt.correspondences_from_topk(iab, dab, iba, mutual, 1)
    wcorr, wcount = R.feature_correspondences(a, b, mutual=mutual)
    assert count == wcount and np.array_equal(corr, wcorr)
    assert np.array_equal(dist[:count], dab[corr[:count, 0], 0].astype(np.float32)) and np.isposinf(dist[count:]).all()


def test_mutual_k_rule_on_a_hand_made_case():
    # 4 src rows, 4 ref columns, k = 2.  Lists (src -> ref) and (ref -> src) written by hand:
    iab = np.array([[0, 1], [0, 2], [3, 2], [1, -1]], np.int32)       # row 3 has one entry only
    dab = np.array([[.1, .2], [.3, .4], [.5, .6], [.7, np.inf]], np.float32)
    iba = np.array([[0, 1], [2, 0], [1, 3], [3, 2]], np.int32)        # column c's two nearest src rows
    # (0,0): 0 in [0,1] yes   (0,1): 0 in [2,0] yes   (1,0): 1 in [0,1] yes   (1,2): 1 in [1,3] yes
    # (2,3): 2 in [3,2] yes   (2,2): 2 in [1,3] NO    (3,1): 3 in [2,0] NO    (3,-1): no entry
    corr, count, dist = Mt.correspondences_from_topk(iab, dab, iba, True, 2)
    assert count == 5 and corr.shape == (8, 2)
    assert corr[:5].tolist() == [[0, 0], [0, 1], [1, 0], [1, 2], [2, 3]] and (corr[5:] == -1).all()
    assert dist[:5].tolist() == [np.float32(x) for x in (.1, .2, .3, .4, .5)] and np.isposinf(dist[5:]).all()
    # without mutual: every entry, in (j, rank) order
    corr, count, _ = Mt.correspondences_from_topk(iab, dab, None, False, 2)
    assert count == 7 and corr[:7].tolist() == [[0, 0], [0, 1], [1, 0], [1, 2], [2, 3], [2, 2], [3, 1]]
    # k = 1 of the same lists is the classic mutual test on rank 0
    corr, count, _ = Mt.correspondences_from_topk(iab, dab, iba, True, 1)
    assert corr[:count].tolist() == [[0, 0]]                          # iba[0][0] == 0; rows 1, 2, 3 do not point back at rank 0
    # ratio test on ranks 0 / 1, k = 1: 0.1 < 0.64 * 0.2, 0.3 !< 0.64 * 0.4, 0.5 !< 0.64 * 0.6, row 3 has no rank 1 -> kept
    corr, count, _ = Mt.correspondences_from_topk(iab, dab, None, False, 1, ratio=0.8)
    assert corr[:count].tolist() == [[0, 0], [3, 1]]
    with pytest.raises(ValueError):
        Mt.correspondences_from_topk(iab, dab, None, False, 2, ratio=0.8)
    with pytest.raises(ValueError):
        Mt.correspondences_from_topk(iab, dab, None, False, 9)


def test_library_exports_and_binds_the_new_entries():
    from deepsir_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "dsir.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SYMBOLS, f"{name} not bound"
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} not declared"
    assert re.search(r"#define\s+DSIR_TOPK_MAX\s+8\b", hdr) and Mt.TOPK_MAX == 8
    assert len(_lib.SYMBOLS["dsir_nn_match_topk"][1]) == 9
    assert len(_lib.SYMBOLS["dsir_feature_correspondences_ex"][1]) == 12
