"""oracle/network.py's score (float32, torch) and the selection references against the plain float64 references of
tests/score_cases.py, on every case the device test (tests/test_gpu_score_edges.py) runs.  Runs without a GPU.  The case builders'
own assertions (both sides of a threshold occur, a mutated reference differs, ...) run with their first use.

The deviation of the float32 oracle from the float64 reference measured here is what the device test's tolerance is derived from:
relative over the points whose reference score is not zero, absolute over those where it is (a closed gate, a zero weight,
pr <= 0.2), fragile points left out.  Measured over all cases: relative 2.8e-7 (nonpositive_max; 2.0e-7 on the random clouds of 4097 points), absolute 0 - the oracle's
zeros are exact.  ``score_cases.MEASURED_REL`` records the relative figure rounded up; the test fails if a case exceeds it, so the tolerance
the device test derives from it cannot go stale."""
import numpy as np
import pytest
import torch

import score_cases as S
from deepsir_amd.arch import LABEL_WEIGHTS, NetConfig
from oracle.network import OracleNet

MEASURED_REL = S.MEASURED_REL
MEASURED_ABS = 0.0

_ALL = S.all_cases()


def deviation(got, want, keep):
    """(largest |got - want| / |want| where want != 0, largest |got - want| where want == 0) over the kept points."""
    got, want = np.asarray(got, np.float64)[keep], np.asarray(want, np.float64)[keep]
    assert np.isfinite(got).all() and np.isfinite(want).all()
    err, big = np.abs(got - want), want != 0
    rel = float((err[big] / np.abs(want[big])).max()) if big.any() else 0.0
    return rel, float(err[~big].max()) if (~big).any() else 0.0


def oracle_score(case):
    n = case.feat.shape[1]
    net = OracleNet(NetConfig(), {})
    logits = torch.from_numpy(case.logits).permute(0, 2, 1).contiguous()
    prob, label = torch.max(logits, dim=1, keepdim=True)
    score = net.score(torch.from_numpy(case.feat).permute(0, 2, 1).contiguous(), torch.from_numpy(case.xyz[:, :n]).permute(0, 2, 1).contiguous(),
                      prob, label, torch.from_numpy(case.neigh[:, :n]).long())
    return score.numpy(), label[:, 0].numpy()


def test_the_table_is_the_projects():
    assert tuple(S.LABEL_WEIGHTS) == tuple(LABEL_WEIGHTS) and S.NUM_CLASSES == NetConfig().num_classes == len(LABEL_WEIGHTS)


@pytest.mark.parametrize("name", list(S.CASES))
def test_case_builders_hold_their_own_assertions(name):
    for case in S.CASES[name]():
        c, n, ch = case.feat.shape
        assert ch == 64 and case.logits.shape == (c, n, S.NUM_CLASSES) and n <= 4097 and c <= 9
        assert case.xyz.shape[0] == c and case.xyz.shape[1] >= n and case.neigh.shape == (c, case.xyz.shape[1], 16)
        assert case.feat.dtype == case.logits.dtype == case.xyz.dtype == np.float32 and case.neigh.dtype == np.int32
        assert case.neigh.min() >= 0 and case.neigh[:, :n].max() < n


@pytest.mark.parametrize("cid,case", _ALL, ids=[i for i, _ in _ALL])
def test_fragile_share(cid, case):
    fragile = S.reference(cid)[2]
    assert fragile.mean() <= 0.01
    if case.boundary:
        assert not fragile.any()


@pytest.mark.parametrize("cid,case", _ALL, ids=[i for i, _ in _ALL])
def test_oracle_score_equals_plain(cid, case):
    want, want_label, fragile = S.reference(cid)
    got, label = oracle_score(case)
    keep = ~fragile
    assert np.array_equal(label[keep], want_label[keep])
    assert (got[keep & (want == 0)] == 0).all()                   # closed gate, zero weight, pr <= 0.2: exactly +-0
    rel, ab = deviation(got, want, keep)
    print(f"SCORE-HOST {cid}: float32 oracle vs float64 plain: rel {rel:.3e} abs {ab:.3e} (fragile {int(fragile.sum())} of {fragile.size})")
    assert rel <= MEASURED_REL and ab <= MEASURED_ABS


# ------------------------------------------------------------------------------------------------------------------- selection
def _torch_topk(s, k):
    return torch.sort(torch.from_numpy(s) + 0.0, dim=-1, descending=True, stable=True)[1][:, :k].numpy().astype(np.int32)


@pytest.mark.parametrize("n", [1, 2, 257, 1000])
@pytest.mark.parametrize("pattern", S.TOPK_PATTERNS)
def test_topk_references_agree(pattern, n):
    s = S.topk_scores(pattern, 3, n)
    for k in sorted({1, max(1, n // 2), max(1, n - 1), n}):
        want = S.plain_topk(s, k)
        assert np.array_equal(want, _torch_topk(s, k)) and np.array_equal(want, S.key_topk(s, k))
        for b in range(3):
            assert np.array_equal(want[b], np.argsort(-(s[b] + np.float32(0.0)), kind="stable")[:k])


def test_topk_key_needs_its_plus_zero():
    s = S.topk_scores("signed_zeros", 2, 257)
    assert (np.signbit(s) & (s == 0)).any() and (~np.signbit(s) & (s == 0)).any()
    assert np.array_equal(S.key_topk(s, 257), S.plain_topk(s, 257))
    assert not np.array_equal(S.key_topk(s, 257, plus_zero=False), S.plain_topk(s, 257))


def test_topk_nan_rule():
    """torch.sort's: NaN of either sign before every number, NaNs among themselves in ascending index."""
    s = S.nan_scores(3, 257)
    bits = s.view(np.uint32)
    assert all((bits == b).any() for b in (0x7fc00000, 0xffc00000, 0xff800001))
    want = S.plain_topk(s, 257)
    assert np.array_equal(want, _torch_topk(s, 257)) and np.array_equal(want, S.key_topk(s, 257))
    assert not np.array_equal(S.key_topk(s, 257, canonical_nan=False), want)
    for b in range(3):
        m = int(np.isnan(s[b]).sum())
        assert np.array_equal(want[b, :m], np.flatnonzero(np.isnan(s[b])))


@pytest.mark.parametrize("pattern", S.PLAN_PATTERNS)
@pytest.mark.parametrize("clouds,m,n", [(1, 1, 1), (3, 17, 2), (1, 17, 65), (3, 4800, 64), (3, 4800, 300), (1, 4800, 1)])
def test_plan_references_agree(pattern, clouds, m, n):
    idx = S.plan_index(pattern, clouds, m, n)
    order, offsets = S.plain_plan(idx, n)
    o2, f2 = S.bucket_plan(idx, n)
    assert np.array_equal(order, o2) and np.array_equal(offsets, f2)
    assert offsets[0] == 0 and offsets[-1] == clouds * m and sorted(order.tolist()) == list(range(clouds * m))
    if pattern == "one_row" and n > 2:
        assert (np.diff(offsets) == 0).sum() == clouds * (n - 1)
    if pattern == "empty_rows" and n >= 64:
        assert (np.diff(offsets) == 0).sum() >= clouds * (n // 2)
    if pattern == "out_of_range":
        assert (idx >= n).any() and ((idx < 0).any() or clouds * m == 1)
