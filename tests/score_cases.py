"""Inputs and plain references the saliency-score and key-point selection tests share (tests/test_score_host.py on the CPU,
tests/test_gpu_score_edges.py on the device).  No GPU and no engine import here.

``plain_score`` restates torch.max(logits) + score_fun (reference network/model.py:638-639, :701-757) in numpy float64, one step
per line: first-maximum argmax; the three per-cloud maxima, each + 1e-16; divide, then average the 16 neighbours; softplus with
threshold 20; the density gate ``mean 16-NN distance < 2.0``; the channel ratio; the label weight times ``[pr > 0.2]``; the maximum
over the 64 channels.  Its keyword arguments are the mutations the case builders use to prove their teeth (``gate_le``, ``thr_ge``,
``softplus_threshold``; a changed weight goes in through ``label_weights``).

``fragile`` marks the points whose decisions float32 cannot be held to: the float64 mean distance within 1e-5 (relative) of 2.0, or
the float64 pr within 1e-6 of 0.2 - unless the compared quantity is exact in float32 whatever the evaluation order:
  * gate: all 16 distances are float32 values that are multiples of 2^-12 and at most 256 (every partial sum in any order, and
    the division by 16, is exact);
  * threshold: pr is ONE correctly rounded float32 division of two float32 inputs (max + 1e-16 == max in float32), there is no
    order to vary, and that quotient falls on the same side of float32(0.2) as the float64 quotient of 0.2.
The boundary cases are built from such inputs: they sit ON the thresholds and leave nothing out.

``CASES`` maps a name to a builder that returns a list of ``Case``: one device call each.  A builder asserts its own teeth on the
reference's output.  The largest cloud has 4097 points.

Layouts are the engine's: feat [c,n,64], logits [c,n,ncls], xyz [c,S,3], neigh [c,S,16] int32 with S >= n (the pyramid buffers
carry the coarser levels behind the n rows of level 0; the score reads the first n)."""
import functools
from typing import NamedTuple

import numpy as np

LABEL_WEIGHTS = (3, 1, 1, 3, 2, 0, 0, 0, 6, 5, 6, 4, 7, 7, 6, 8, 4, 9, 9)       # reference network/model.py:146-149
NUM_CLASSES = 19
EPS = 1e-16                                                                      # model.py:18
K = 16
F32 = np.float32


# The float32 oracle (oracle/network.py, divide then average, torch on the CPU) against plain_score, largest relative deviation over
# the non-zero reference scores of all cases below: 2.8e-7, rounded up (tests/test_score_host.py measures it and fails beyond it).
# Where the reference is zero the oracle is exactly zero.  The device may use four times that: csrc/score.hip sums the 16 neighbour
# rows before its one division, ~1e-7 of the mean on top.  Capped at the tolerance the stage tests hold the score to.
MEASURED_REL = 3e-7
STAGE_RTOL, STAGE_ATOL = 1e-4, 1e-6
SCORE_RTOL = min(4 * MEASURED_REL, STAGE_RTOL)
SCORE_ATOL = min(4 * 0.0, STAGE_ATOL)


class Case(NamedTuple):
    feat: np.ndarray
    logits: np.ndarray
    xyz: np.ndarray
    neigh: np.ndarray
    label: str
    boundary: bool           # built from float32-exact inputs on a threshold: fragile must be empty


# ---------------------------------------------------------------------------------------------------------------- plain reference
def plain_argmax(logits: np.ndarray):
    """[n, ncls] -> (best [n], label [n]): the first maximum wins (torch.max on the CPU)."""
    n, ncls = logits.shape
    best = logits[:, 0].copy()
    label = np.zeros(n, np.int64)
    for c in range(1, ncls):
        take = logits[:, c] > best
        best[take] = logits[take, c]
        label[take] = c
    return best, label


def _softplus(x, threshold=True):
    with np.errstate(over="ignore"):
        soft = np.log1p(np.exp(x))
    return np.where(x > 20.0, x, soft) if threshold else np.where(np.isinf(soft), x, soft)


def plain_score(feat, logits, xyz, neigh, label_weights=LABEL_WEIGHTS, gate_le=False, thr_ge=False, softplus_threshold=True):
    """-> (score [c,n] float64, label [c,n] int64, fragile [c,n] bool)."""
    feat, logits, xyz = (np.asarray(a, np.float64) for a in (feat, logits, xyz))
    c, n, _ = feat.shape
    w = np.asarray(label_weights, np.float64)
    score, label, fragile = np.zeros((c, n)), np.zeros((c, n), np.int64), np.zeros((c, n), bool)
    for b in range(c):
        F, X, nb = feat[b], xyz[b], np.asarray(neigh[b, :n], np.int64)
        assert nb.min() >= 0 and nb.max() < n
        best, lab = plain_argmax(logits[b])
        fden = F.max() + EPS                                       # per-cloud maxima
        wden = w[lab].max() + EPS
        pden = best.max() + EPS
        fn = F / fden                                              # divide ...
        mean = np.zeros_like(fn)
        for k in range(K):                                         # ... then average
            mean += fn[nb[:, k]]
        mean /= K
        sal = _softplus(fn - mean, softplus_threshold)
        dist = np.zeros((n, K))
        for k in range(K):
            d = X[nb[:, k]] - X[:n]
            dist[:, k] = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        md = dist.sum(1) / K
        gate = ((md <= 2.0) if gate_le else (md < 2.0)).astype(np.float64)
        chan = fn / (fn.max(1, keepdims=True) + EPS)
        pr = best / pden
        on = ((pr >= 0.2) if thr_ge else (pr > 0.2)).astype(np.float64)
        ls = (w[lab] / wden) * on
        score[b] = (sal * gate[:, None] * chan * ls[:, None]).max(1)
        label[b] = lab
        # what float32 cannot be held to
        d32 = dist.astype(F32).astype(np.float64)
        gate_exact = ((d32 == dist) & (np.round(dist * 4096.0) == dist * 4096.0) & (dist <= 256.0)).all(1)
        near_gate = (np.abs(md - 2.0) <= 2e-5) & ~gate_exact
        b32, p32 = best.astype(F32), F32(best.max())
        with np.errstate(divide="ignore", invalid="ignore"):
            q32 = b32 / (p32 + F32(EPS))
        thr_exact = (p32 + F32(EPS) == p32) & ((q32 > F32(0.2)) == (pr > 0.2)) & ((q32 >= F32(0.2)) == (pr >= 0.2))
        near_thr = (np.abs(pr - 0.2) <= 1e-6) & ~thr_exact
        fragile[b] = near_gate | near_thr
    return score, label, fragile


def gate_in_float32(xyz, neigh, n):
    """The gate with every operation in float32, neighbours added in ascending order -> bool [c,n]."""
    X = np.asarray(xyz, F32)
    out = np.zeros((X.shape[0], n), bool)
    for b in range(X.shape[0]):
        s = np.zeros(n, F32)
        for k in range(K):
            d = X[b][neigh[b, :n, k]] - X[b][:n]
            s = s + np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        assert s.dtype == F32
        out[b] = s / F32(16.0) < F32(2.0)
    return out


def threshold_in_float32(logits):
    """``pr > 0.2`` with every operation in float32 -> bool [c,n]."""
    L = np.asarray(logits, F32)
    out = np.zeros(L.shape[:2], bool)
    for b in range(L.shape[0]):
        best, _ = plain_argmax(L[b])
        with np.errstate(divide="ignore", invalid="ignore"):
            pr = best / (best.max() + F32(EPS))
        assert pr.dtype == F32
        out[b] = pr > F32(0.2)
    return out


# ------------------------------------------------------------------------------------------------- top-k and scatter-plan references
def plain_topk(score: np.ndarray, k: int) -> np.ndarray:
    """[clouds, n] -> [clouds, k]: descending score, equal scores (+0 == -0) in ascending index, NaN of either sign before every
    number and NaNs among themselves in ascending index (torch.sort(descending=True, stable=True)).  Without NaN this is
    ``np.argsort(-(s + 0.0), kind="stable")[:k]``."""
    s = np.asarray(score, np.float32)
    out = np.zeros((s.shape[0], k), np.int32)
    for b in range(s.shape[0]):
        nan = np.isnan(s[b])
        if not nan.any():
            out[b] = np.argsort(-(s[b] + F32(0.0)), kind="stable")[:k]
            continue
        vals = [float(v) for v in s[b]]
        order = sorted(range(len(vals)), key=lambda i: (0, 0.0, i) if nan[i] else (1, -(vals[i] + 0.0), i))
        out[b] = order[:k]
    return out


def key_topk(score: np.ndarray, k: int, plus_zero: bool = True, canonical_nan: bool = True) -> np.ndarray:
    """The device's way to the same rule (csrc/select.hip): an unsigned key whose ascending order is the descending score order,
    then a stable sort.  ``plus_zero=False`` and ``canonical_nan=False`` are the mutations: without ``+ 0.0`` a -0 sorts behind
    every +0, without the NaN rule a NaN with its sign bit set sorts last."""
    s = np.asarray(score, np.float32)
    with np.errstate(invalid="ignore"):
        v = (s + F32(0.0)) if plus_zero else s
    b = np.ascontiguousarray(v).view(np.uint32).astype(np.uint64)
    b = np.where(b & 0x80000000, ~b & 0xffffffff, b | 0x80000000)
    key = ~b & 0xffffffff
    if canonical_nan:
        key = np.where(np.isnan(s), 0, key)
    return np.argsort(key, axis=1, kind="stable")[:, :k].astype(np.int32)


def plain_plan(idx: np.ndarray, n: int):
    """idx [clouds, m] into [clouds, n] -> (order [clouds * m], offsets [clouds * n + 1]): the sources e grouped by destination row
    ``cloud * n + clip(idx, 0, n - 1)``, ascending e inside a group; offsets[d] = the first position whose destination is >= d."""
    idx = np.asarray(idx, np.int64)
    clouds, m = idx.shape
    key = (np.arange(clouds)[:, None] * n + np.clip(idx, 0, n - 1)).reshape(-1)
    order = np.argsort(key, kind="stable")
    offsets = np.searchsorted(key[order], np.arange(clouds * n + 1), side="left")
    return order.astype(np.int32), offsets.astype(np.int32)


def bucket_plan(idx: np.ndarray, n: int):
    """The same plan by appending every source to its destination's list, one by one."""
    idx = np.asarray(idx, np.int64)
    clouds, m = idx.shape
    rows = [[] for _ in range(clouds * n)]
    for e in range(clouds * m):
        i = int(idx[e // m, e % m])
        rows[(e // m) * n + min(max(i, 0), n - 1)].append(e)
    order, offsets = [], [0]
    for r in rows:
        order += r
        offsets.append(len(order))
    return np.asarray(order, np.int32), np.asarray(offsets, np.int32)


TOPK_PATTERNS = ("all_equal", "two_values", "signed_zeros", "all_negative", "infinities", "denormals", "ascending", "descending",
                 "per_cloud")


def topk_scores(pattern: str, clouds: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(clouds * 100003 + n * 17 + TOPK_PATTERNS.index(pattern))
    if pattern == "all_equal":
        s = np.full((clouds, n), 0.375)
    elif pattern == "two_values":
        s = rng.choice([1.5, -2.25], (clouds, n))
    elif pattern == "signed_zeros":
        s = rng.choice([0.0, -0.0, 0.0, -0.0, 0.5, -0.5], (clouds, n))
    elif pattern == "all_negative":
        s = -rng.integers(1, 40, (clouds, n)) / 8.0
    elif pattern == "infinities":
        s = rng.choice([np.inf, -np.inf, 0.0, 3.0e38, -3.0e38, 1.0], (clouds, n))
    elif pattern == "denormals":
        s = rng.integers(-3, 4, (clouds, n)) * 1.4e-45 * rng.choice([1, 1000], (clouds, n))
    elif pattern == "ascending":
        s = np.sort(rng.normal(size=(clouds, n)).round(1), axis=1)
    elif pattern == "descending":
        s = -np.sort(rng.normal(size=(clouds, n)).round(1), axis=1)
    else:
        rows = [topk_scores(TOPK_PATTERNS[b % (len(TOPK_PATTERNS) - 1)], 1, n)[0] for b in range(clouds)]
        return np.stack(rows)
    return s.astype(F32)


def nan_scores(clouds: int, n: int) -> np.ndarray:
    """Numbers, infinities and NaNs of both signs (0x7fc00000, 0xffc00000 and a payload-carrying 0xff800001)."""
    rng = np.random.default_rng(7 * clouds + n)
    bits = rng.choice(np.array([0x7fc00000, 0xffc00000, 0xff800001, 0x7f800000, 0xff800000, 0x3f800000, 0xbf800000, 0x0, 0x80000000],
                               np.uint32), (clouds, n))
    return np.ascontiguousarray(bits).view(F32)


PLAN_PATTERNS = ("random", "one_row", "empty_rows", "out_of_range")


def plan_index(pattern: str, clouds: int, m: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(clouds * 1000003 + m * 1009 + n + PLAN_PATTERNS.index(pattern))
    if pattern == "random":
        idx = rng.integers(0, n, (clouds, m))
    elif pattern == "one_row":
        idx = np.full((clouds, m), n // 2)
    elif pattern == "empty_rows":
        idx = rng.integers(0, n, (clouds, m)) // 3 * 3 % n                   # two rows of three never named
    else:
        idx = rng.integers(0, n, (clouds, m))
        idx[rng.random((clouds, m)) < 0.3] = -5
        idx[rng.random((clouds, m)) < 0.3] = n + 3
        idx[0, 0], idx[-1, -1] = -5, n + 3
    return idx.astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------------ builders
def _open_geometry(rng, c, n, S=None):
    """Points in a unit box, random neighbour rows: every mean distance is below sqrt(3), the gate is open everywhere.  Rows beyond
    n hold far-away points and their own index: a kernel that read them would close the gate."""
    S = n if S is None else S
    xyz = np.full((c, S, 3), 1.0e6, F32)
    xyz[:, :n] = rng.uniform(0.0, 1.0, (c, n, 3))
    neigh = np.zeros((c, S, K), np.int32)
    neigh[:, :n] = rng.integers(0, n, (c, n, K))
    return xyz, neigh


def _winner(rng, c, n, labels, top):
    """Logits whose maximum is ``top`` [c,n] at class ``labels`` [c,n]; every other class lies 1 to 3 below."""
    lg = (top[..., None] - rng.uniform(1.0, 3.0, (c, n, NUM_CLASSES))).astype(F32)
    np.put_along_axis(lg, labels[..., None], top[..., None].astype(F32), 2)
    return lg


_NONZERO = [i for i, w in enumerate(LABEL_WEIGHTS) if w > 0]


def _check(case, **mut):
    return plain_score(case.feat, case.logits, case.xyz, case.neigh, **mut)


def gate_boundary():
    """Points at the origin whose 16 neighbours lie at distances 0, 2 and 2.5 exactly: groups of 8 with a mean of exactly 2.0 (all
    at 2), 2.0 again (4 x 2.5 + 1 x 0 + 11 x 2), 1.875 (15 x 2 + the point itself) and 2.03125 (1 x 2.5 + 15 x 2)."""
    rng = np.random.default_rng(11)
    aux = np.array([(2, 0, 0), (-2, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 2), (0, 0, -2), (1.5, 2, 0), (-2, 1.5, 0)], F32)
    n = 32 + len(aux) + 3                                         # 43: no multiple of 16
    xyz = np.zeros((1, n, 3), F32)
    xyz[0, 32:40] = aux
    two, far = np.arange(32, 38), np.array([38, 39])
    neigh = np.zeros((1, n, K), np.int32)
    for i in range(n):
        if i < 8:
            row = rng.choice(two, 16)
        elif i < 16:
            row = np.concatenate([rng.choice(far, 4), [i], rng.choice(two, 11)])
        elif i < 24:
            row = np.concatenate([rng.choice(two, 15), [i]])
        elif i < 32:
            row = np.concatenate([rng.choice(far, 1), rng.choice(two, 15)])
        else:
            row = np.full(16, i)                                  # the auxiliary points: themselves, distance 0
        neigh[0, i] = rng.permutation(row)
    feat = rng.uniform(0.1, 1.0, (1, n, 64)).astype(F32)
    logits = _winner(rng, 1, n, rng.choice(_NONZERO, (1, n)), np.full((1, n), 3.0))
    case = Case(feat, logits, xyz, neigh, "n43", True)
    score, _, fragile = _check(case)
    d = np.linalg.norm(xyz[0][neigh[0]].astype(np.float64) - xyz[0][:, None].astype(np.float64), axis=2).mean(1)
    assert (d[:16] == 2.0).all() and (d[16:24] == 1.875).all() and (d[24:32] == 2.03125).all() and (d[32:] == 0.0).all()
    gate = d < 2.0
    assert (score[0][gate] > 0).all() and (score[0][~gate] == 0).all() and gate.sum() == 19
    assert np.array_equal(gate_in_float32(xyz, neigh, n)[0], gate) and not fragile.any()
    mutant = _check(case, gate_le=True)[0]
    assert (mutant[0, :16] > 0).all() and np.array_equal(mutant[0, 16:], score[0, 16:])
    return [case]


def prob_threshold():
    """Cloud 0: maximum logit 5.0; winning logits of exactly 1.0 (pr == 0.2: weight off), the next float32 above 1.0 (on), 0.5 (off)
    and 4.0 (on).  Cloud 1: negative logits only, so that every pr is at least 1."""
    rng = np.random.default_rng(12)
    n = 41
    top = np.zeros((2, n))
    kinds = np.array([1.0, float(np.nextafter(F32(1.0), F32(2.0))), 0.5, 4.0])
    top[0] = kinds[np.arange(n) % 4]
    top[0, 0] = 5.0
    top[1] = -rng.integers(1, 9, n) / 2.0
    logits = _winner(rng, 2, n, rng.choice(_NONZERO, (2, n)), top)
    xyz, neigh = _open_geometry(rng, 2, n)
    feat = rng.uniform(0.1, 1.0, (2, n, 64)).astype(F32)
    case = Case(feat, logits, xyz, neigh, "n41", True)
    score, _, fragile = _check(case)
    on = np.array([t in (5.0, kinds[1], 4.0) for t in top[0]])
    assert (score[0][on] > 0).all() and (score[0][~on] == 0).all() and on.sum() >= 10 and (~on).sum() >= 10
    assert (score[1] > 0).all()
    assert np.array_equal(threshold_in_float32(logits)[0], on) and threshold_in_float32(logits)[1].all() and not fragile.any()
    mutant = _check(case, thr_ge=True)[0]
    at = top[0] == 1.0
    assert at.sum() >= 5 and (mutant[0][at] > 0).all() and np.array_equal(mutant[0][~at], score[0][~at])
    return [case]


def every_label():
    """Every class wins at three points - the zero-weight classes 5, 6, 7 too -, and at one more point the logits of classes 3
    and 12 are bit-equal maxima: the first, 3, wins."""
    rng = np.random.default_rng(13)
    n = 3 * NUM_CLASSES + 1
    labels = (np.arange(n) % NUM_CLASSES)[None]
    labels[0, -1] = 3
    logits = _winner(rng, 1, n, labels, rng.uniform(2.0, 3.0, (1, n)))
    logits[0, -1, 12] = logits[0, -1, 3]
    xyz, neigh = _open_geometry(rng, 1, n)
    feat = rng.uniform(0.1, 1.0, (1, n, 64)).astype(F32)
    case = Case(feat, logits, xyz, neigh, "n58", False)
    score, lab, fragile = _check(case)
    assert np.array_equal(lab, labels) and not fragile.any()
    zero = np.isin(labels[0], (5, 6, 7))
    assert (score[0][zero] == 0).all() and (score[0][~zero] > 0).all()
    for c in range(NUM_CLASSES):
        w = list(LABEL_WEIGHTS)
        w[c] += 1
        assert not np.array_equal(_check(case, label_weights=w)[0], score), c
    return [case]


def softplus_branch():
    """Feature maximum 1.  Points 0..15 hold features of -30 to -50 (and a label of weight 0); of the others a third average 12 of them (fn - mean > 20),
    a third 4 of them (about 10) and a third none."""
    rng = np.random.default_rng(14)
    n = 64
    feat = rng.uniform(0.0, 1.0, (1, n, 64)).astype(F32)
    feat[0, :16] = -rng.uniform(30.0, 50.0, (16, 64))
    feat[0, 20, 7] = 1.0
    xyz, neigh = _open_geometry(rng, 1, n)
    neigh[0] = rng.integers(16, n, (n, K))
    for i in range(16, n):
        low = (12, 4, 0)[i % 3]
        neigh[0, i, :low] = rng.integers(0, 16, low)
    labels = rng.choice(_NONZERO, (1, n))
    labels[0, :16] = 6                                             # weight 0: their own e^-40 scores are not what the case is about
    logits = _winner(rng, 1, n, labels, np.full((1, n), 3.0))
    case = Case(feat, logits, xyz, neigh, "n64", False)
    score, _, fragile = _check(case)
    fn = feat[0].astype(np.float64)
    x = fn - fn[neigh[0]].mean(1)
    assert feat.max() == 1.0 and ((x > 20).any(1)).sum() >= 10 and ((x[16:] < 20).all(1)).sum() >= 10 and not fragile.any()
    assert (score[0, 18::3] > 20.0 / 9.0).all()                    # the branch's value times a label weight of 1/9 at least
    assert np.allclose(_check(case, softplus_threshold=False)[0], score, rtol=1e-12, atol=0)
    return [case]


def nonpositive_max():
    """Eight clouds.  0-3: the feature maximum is 0.0 / -0.0 with every other feature negative / strictly negative / every
    feature -0.0.  4-7: the same four for the maximum logit.  In clouds 0-3 the features are the integers -1 to -4, every
    neighbour row names one point 16 times, and that point differs from the row's own in every channel: after the division by
    1e-16 values near 1e16 are subtracted, and a float32 evaluation is only as good as the gap between them is wide.  A true
    difference of 0 would make softplus's ln 2 a matter of the last bit of 1e16."""
    rng = np.random.default_rng(15)
    c, n = 8, 40
    xyz, neigh = _open_geometry(rng, c, n)
    step = 4 * rng.integers(0, n // 4, (4, n, 1)) + rng.integers(1, 4, (4, n, 1))
    neigh[:4, :n] = np.repeat((np.arange(n)[None, :, None] + step) % n, K, axis=2)
    feat = rng.uniform(0.1, 1.0, (c, n, 64)).astype(F32)
    feat[:4] = -(1 + (np.arange(n)[:, None] + np.arange(64)[None, :]) % 4)
    feat[0, 3] = 0.0
    feat[1, 3] = -0.0
    feat[3] = -0.0
    top = np.full((c, n), 3.0)
    top[4:] = -rng.integers(1, 9, (4, n)) / 2.0
    logits = _winner(rng, c, n, rng.choice(_NONZERO, (c, n)), top)
    logits[4, 5, LABEL_WEIGHTS.index(8)] = 0.0
    logits[5, 5, LABEL_WEIGHTS.index(8)] = -0.0
    logits[7] = -0.0
    case = Case(feat, logits, xyz, neigh, "c8n40", False)
    score, lab, fragile = _check(case)
    bits = lambda a: np.ascontiguousarray(a, F32).view(np.uint32)
    assert feat[0].max() == 0 and bits(feat[0]).min() == 0 and bits(feat[1].max()) == 0x80000000 and (feat[1] < 0).sum() == (n - 1) * 64
    assert feat[2].max() == -1 and (bits(feat[3]) == 0x80000000).all()
    best = logits.max(2)
    assert best[4].max() == 0 and bits(best[5].max()) == 0x80000000 and (best[5] < 0).sum() == n - 1 and best[6].max() < 0
    assert (bits(logits[7]) == 0x80000000).all() and (lab[7] == 0).all()
    assert np.isfinite(score).all() and not fragile.any()
    assert (score[0] >= 0).all() and (score[0] > 1e15).any() and (score[1] > 1e15).any() and (score[2] > 0).all()
    assert (score[3] == 0).all() and (score[4] == 0).all() and (score[5] == 0).all() and (score[6] > 0).all() and (score[7] == 0).all()
    return [case]


def _apart(rng, c, n, scales, label_sets, name):
    S = n + 341
    xyz, neigh = _open_geometry(rng, c, n, S)
    feat = np.stack([rng.uniform(-1.0, 1.0, (n, 64)) * s for s in scales]).astype(F32)
    labels = np.stack([rng.choice(ls, n) for ls in label_sets])
    top = np.stack([rng.uniform(0.3, 1.0, n) * s for s in scales])
    logits = np.stack([_winner(rng, 1, n, labels[b:b + 1], top[b:b + 1])[0] if scales[b] >= 1 else
                       (_winner(rng, 1, n, labels[b:b + 1], top[b:b + 1] / scales[b])[0] * F32(scales[b])) for b in range(c)])
    return Case(feat, logits.astype(F32), xyz, neigh, name, False)


def clouds_apart():
    """3 and 9 clouds whose feature, logit and label-weight maxima differ by orders of magnitude from one cloud to the next (one
    cloud has a single label), in buffers of S = n + 341 rows; and a third batch of 3 clouds whose maxima are all far below the
    first two's, for the call that follows them on the same engine."""
    rng = np.random.default_rng(16)
    n = 300
    sets = [[1, 2], list(range(NUM_CLASSES)), [4], [0, 3, 9], [17, 18, 5], [1, 4], [15], [2, 11], [0, 1, 2, 3]]
    scl = [1e-3, 1e3, 1.0, 1e-4, 1e2, 1e-2, 1e4, 1e-1, 10.0]
    out = [_apart(rng, 3, n, scl[:3], sets[:3], "c3"), _apart(rng, 9, n, scl, sets, "c9"),
           _apart(rng, 3, n, [1e-5, 1e-6, 1e-5], [[1], [1, 2], [2, 4]], "small")]
    for case in out[:2]:
        score, lab, fragile = _check(case)
        c = len(score)
        wmax = [max(LABEL_WEIGHTS[i] for i in np.unique(lab[b])) for b in range(c)]
        fmax, pmax = case.feat.reshape(c, -1).max(1), case.logits.max(2).max(1)
        for b in range(c - 1):
            assert max(fmax[b] / fmax[b + 1], fmax[b + 1] / fmax[b]) > 50 and max(pmax[b] / pmax[b + 1], pmax[b + 1] / pmax[b]) > 50
            assert wmax[b] != wmax[b + 1]
        assert len(np.unique(lab[2])) == 1 and case.xyz.shape[1] == n + 341 and case.neigh.shape[1] == n + 341
        assert fragile.mean() <= 0.01 and all((score[b] > 0).mean() > 0.3 for b in range(c))
        # two neighbouring clouds sharing their maxima: the one with the smaller maxima scores differently
        for b in range(1, c):
            mixed = Case(np.concatenate([case.feat[b - 1], case.feat[b]])[None], np.concatenate([case.logits[b - 1], case.logits[b]])[None],
                         np.concatenate([case.xyz[b - 1, :n], case.xyz[b, :n]])[None],
                         np.concatenate([case.neigh[b - 1, :n], case.neigh[b, :n] + n])[None], "", False)
            got = _check(mixed)[0][0]
            assert not (np.allclose(got[:n], score[b - 1], rtol=1e-3, atol=0) and np.allclose(got[n:], score[b], rtol=1e-3, atol=0)), b
    assert out[2].feat.max() < 1e-4 * out[1].feat.max() and out[2].logits.max() < 1e-4 * out[1].logits.max()
    return out


def _knn(points: np.ndarray, k: int) -> np.ndarray:
    """Brute-force k nearest (the point itself first); fewer than k points: the row repeats."""
    n = len(points)
    p = points.astype(np.float64)
    out = np.zeros((n, k), np.int32)
    for a in range(0, n, 512):
        d = ((p[a:a + 512, None, :] - p[None, :, :]) ** 2).sum(2)
        d[np.arange(len(d)), np.arange(a, a + len(d))] = -1.0
        order = np.argsort(d, axis=1, kind="stable")[:, :k]
        out[a:a + 512] = order[:, np.arange(k) % order.shape[1]]
    return out


RAGGED_N = (1, 15, 16, 17, 255, 257, 1000, 4097)


def ragged():
    """2 clouds of n in {1, 15, 16, 17, 255, 257, 1000, 4097} points shaped like a lidar sweep (dense near the sensor, sparse far
    out, 3 m high; the radius shrinks with n below 1000 so that the small clouds keep open gates): the 16-NN mean distance falls
    on both sides of 2.0.  Every neighbour row starts with the point itself, and a third of the rows name one neighbour three times."""
    out = []
    for n in RAGGED_N:
        rng = np.random.default_rng(1700 + n)
        r, phi = 1.0 + 60.0 * min(1.0, n / 1000.0) * rng.random((2, n)) ** 2, rng.uniform(0, 2 * np.pi, (2, n))
        xyz = np.stack([r * np.cos(phi), r * np.sin(phi), rng.uniform(-2.0, 1.0, (2, n))], 2).astype(F32)
        neigh = np.stack([_knn(xyz[b], K) for b in range(2)])
        rep = np.arange(n) % 3 == 0
        neigh[:, rep, 14] = neigh[:, rep, 1]
        neigh[:, rep, 15] = neigh[:, rep, 1]
        assert (neigh[:, :, 0] == np.arange(n)).all()
        feat = rng.normal(size=(2, n, 64)).astype(F32)
        logits = (2.0 * rng.normal(size=(2, n, NUM_CLASSES))).astype(F32)
        case = Case(feat, logits, xyz, neigh, f"n{n}", False)
        score, lab, fragile = _check(case)
        assert fragile.mean() <= 0.01
        if n >= 1000:
            d = np.linalg.norm(xyz[:, :, None, :].astype(np.float64) - np.stack([xyz[b][neigh[b]] for b in range(2)]), axis=3).mean(2)
            assert 0.05 <= (d < 2.0).mean() <= 0.95, (n, float((d < 2.0).mean()))
            assert len(np.unique(lab)) == NUM_CLASSES and (score > 0).mean() > 0.03
        out.append(case)
    return out


CASES = {f.__name__: functools.lru_cache(maxsize=None)(f) for f in
         (gate_boundary, prob_threshold, every_label, softplus_branch, nonpositive_max, clouds_apart, ragged)}


def all_cases():
    """(id, Case) of every device call."""
    return [(f"{name}-{case.label}", case) for name, build in CASES.items() for case in build()]


@functools.lru_cache(maxsize=None)
def reference(case_id: str):
    """plain_score of a case, computed once and shared."""
    case = dict(all_cases())[case_id]
    out = plain_score(case.feat, case.logits, case.xyz, case.neigh)
    for a in out:
        a.setflags(write=False)
    return out
