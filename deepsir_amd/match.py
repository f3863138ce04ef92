"""Host restatement of the top-k descriptor search and the correspondence rules built on it (csrc/nn_topk.hip states them; numpy only).

The device's answer for a src row is its k smallest keys ``order_bits(d) << 32 | column`` in ascending order, d the fp32 distance of
``dsir_nn_match``: ascending (distance, column), ties to the lower column.  ``topk_host`` evaluates the same order in float64 and
marks the rows whose order float64 cannot pin; ``ratio_keep`` and ``correspondences_from_topk`` restate the ratio test and the
compaction exactly (they take the device's own lists, so no tolerance is involved).
"""
from __future__ import annotations

import numpy as np

TOPK_MAX = 8          # DSIR_TOPK_MAX
BAND = 1e-5           # float64 distances closer than this: the fp32 decision (error ~6e-7 on unit descriptors) is not the host's to pin


def topk_host(desc_src, desc_ref, k: int):
    """desc_src [J, C], desc_ref [K, C] -> (idx [J, k] int32, dist [J, k] float64, band [J] bool).

    float64 distances ``(|a|^2 - 2 a.b) + |b|^2``, a stable sort by (distance, index); ranks beyond K are index -1, distance +inf.
    ``band[j]`` is set where two of row j's first k + 1 distances are closer than 1e-5: the device decides in fp32, so such a row's
    order is its own."""
    a = np.asarray(desc_src, np.float64)
    b = np.asarray(desc_ref, np.float64)
    J, K = a.shape[0], b.shape[0]
    D = ((a * a).sum(1)[:, None] - 2.0 * a @ b.T) + (b * b).sum(1)[None, :]
    order = np.argsort(D, axis=1, kind="stable")          # stable: equal distances keep ascending index
    m = min(k, K)
    idx = np.full((J, k), -1, np.int32)
    dist = np.full((J, k), np.inf, np.float64)
    idx[:, :m] = order[:, :m]
    dist[:, :m] = np.take_along_axis(D, order[:, :m], 1)
    head = np.take_along_axis(D, order[:, :min(k + 1, K)], 1)
    band = (np.diff(head, axis=1) < BAND).any(1) if head.shape[1] > 1 else np.zeros(J, bool)
    return idx, dist, band


def ratio_r2(ratio: float) -> np.float32:
    """fp32(ratio * ratio), rounded once - what the device multiplies by."""
    r = np.float32(ratio)
    return np.float32(r * r)


def ratio_keep(d0, d1, ratio: float):
    """Lowe's ratio test in the device's arithmetic: keep iff ``max(d0, 0) < r2 * max(d1, 0)`` in fp32 (one multiply, a strict
    comparison).  ``d1`` None, or +inf where rank 1 is missing (K == 1), keeps the match; ``d0 == d1 == 0`` rejects it.  ``ratio <= 0``
    means no test; ``ratio >= 1`` or a non-finite ratio is refused."""
    if not np.isfinite(ratio) or ratio >= 1.0:
        raise ValueError("ratio must be finite and below 1")
    d0 = np.asarray(d0, np.float32)
    if ratio <= 0.0 or d1 is None:
        return np.ones(d0.shape, bool)
    d1 = np.asarray(d1, np.float32)
    missing = np.isposinf(d1)
    with np.errstate(invalid="ignore"):
        rhs = (ratio_r2(ratio) * np.maximum(d1, np.float32(0.0))).astype(np.float32)
        return missing | (np.maximum(d0, np.float32(0.0)) < rhs)


def correspondences_from_topk(idx_ab, dist_ab, idx_ba, mutual: bool, k: int, ratio: float = 0.0):
    """The compaction rule on given lists of ONE pair: idx_ab / dist_ab [J, >= k] (src -> ref, ascending ranks; >= 2 ranks for the
    ratio test), idx_ba [K, >= k] (ref -> src; read under ``mutual`` only, may be None otherwise).

    Candidate (j, c) for every rank < k of row j with an entry (index >= 0); with ``ratio`` > 0 (k must be 1) row j keeps its rank-0
    match iff rank 1 is missing or ``ratio_keep`` holds; under ``mutual`` a candidate is kept iff j is among the first k entries of
    column c's list.  Output in ascending j, then rank: (corr [J k, 2] int32 with -1 beyond count, count, dist [J k] float32 with
    +inf beyond count)."""
    if not 1 <= k <= TOPK_MAX:
        raise ValueError("k outside [1, 8]")
    if not np.isfinite(ratio) or ratio >= 1.0:
        raise ValueError("ratio must be finite and below 1")
    if ratio > 0.0 and k > 1:
        raise ValueError("the ratio test is defined on the 1-NN set")
    idx_ab = np.asarray(idx_ab).reshape(len(idx_ab), -1)
    dist_ab = np.asarray(dist_ab, np.float32).reshape(idx_ab.shape)
    J = idx_ab.shape[0]
    keep = idx_ab[:, :k] >= 0
    if ratio > 0.0:
        has1 = idx_ab[:, 1] >= 0
        ok = ratio_keep(dist_ab[:, 0], dist_ab[:, 1], ratio)
        keep[:, 0] &= ~has1 | ok
    if mutual:
        idx_ba = np.asarray(idx_ba).reshape(len(idx_ba), -1)[:, :k]
        c = np.clip(idx_ab[:, :k], 0, len(idx_ba) - 1)
        back = (idx_ba[c] == np.arange(J)[:, None, None]).any(2)          # [J, k]: j among column c's first k entries
        keep &= back
    jj, rr = np.nonzero(keep)                                              # row-major: ascending j, then rank
    corr = np.full((J * k, 2), -1, np.int32)
    dist = np.full(J * k, np.inf, np.float32)
    corr[:len(jj), 0] = jj
    corr[:len(jj), 1] = idx_ab[jj, rr]
    dist[:len(jj)] = dist_ab[jj, rr]
    return corr, int(len(jj)), dist
