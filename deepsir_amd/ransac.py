"""Host restatement of the RANSAC pose rule of ``csrc/ransac.hip`` (include/dsir.h, dsir_ransac_correspondence) in numpy.

The reference's stage is two open3d calls (network/DGR.py:7-36, used by DGR.safeguard_registration, :249-306); open3d cannot
be imported here, so parity is unpinned and the engine owns the rule.  This module states the same rule a second time, the way
``augment.py`` does for the augmentation: the tests compare the device against it, the product path never calls it.

The rule, per pair ``p`` (see the header of csrc/ransac.hip for the full text):

* live rows ``count``; indices clamped into range (a clamp of a live row is reported); matched points gathered once; a row with a
  non-finite coordinate is *parked* at ``s = 0, q = FLT_MAX``: never an inlier, never sampled, exact zeros in a refit;
* hypothesis ``h``, draw ``k``: ``d = splitmix64(splitmix64(seed ^ (p << 40)) ^ (h << 8) ^ k)``, ``row = ((d >> 32) * count) >> 32``;
  a repeated row, a parked row or ``count < n`` rejects the sample;
* fit: unweighted Kabsch in float64 on the fp32 coordinates (sums in sample order), reflection fix, ``T`` rounded to fp32 once;
* checks: edge lengths (both directions, ``edge_sim``), then every sample member within ``thr``;
* residual in fp32: ``c_r = fma(z, T_r2, fma(y, T_r1, x * T_r0)) + T_r3`` (``se3_row`` of csrc/device_utils.h: the two fused
  multiply-adds are reproduced exactly below), ``d = c - q``, ``d2 = (dx*dx + dy*dy) + dz*dz``; inlier iff ``d2 < fp32(thr * thr)``;
* score: integer inlier count; winner: largest count, ties to the lower ``h``;
* ``refine_iters`` refits on all inliers, recount; result: the last largest count of ``T_0 .. T_r`` (a refit that keeps the count
  wins over the n-point pose it started from; one that loses inliers is dropped).

Two places where the restatement is *not* bit-exact with the device, by construction: the 3x3 SVD (LAPACK here, one-sided Jacobi
there) and the refit's sums (float64 here; fp32 products summed in float64 there).  Both sit below 1e-6 in the pose; everything
integer (draws, counts given a ``T``, the pick) is exact.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from .augment import MASK, splitmix64

FLT_MAX = np.float32(np.finfo(np.float32).max)
CHUNK = 256                      # DSIR_RANSAC_CHUNK of include/dsir.h: correspondences a scoring workgroup stages per step
MAX_HYPOTHESES = 1 << 20         # DSIR_RANSAC_MAX_HYPOTHESES
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32).reshape(3, 4)


# ---------------------------------------------------------------------------------------------------------------- draws
def pair_key(seed: int, p: int) -> int:
    return splitmix64((int(seed) ^ (int(p) << 40)) & MASK)


def sample_rows(seed: int, p: int, hyps, n: int, count: int) -> np.ndarray:
    """[len(hyps), 4] int32 rows of the hypotheses ``hyps`` of pair ``p`` (-1 beyond ``n``).  Depends on (seed, p, h, k, count) alone."""
    h = np.asarray(hyps, dtype=np.uint64).reshape(-1)
    out = np.full((h.shape[0], 4), -1, np.int32)
    key = np.uint64(pair_key(seed, p))
    for k in range(n):
        d = splitmix64(key ^ (h << np.uint64(8)) ^ np.uint64(k))
        out[:, k] = (((d >> np.uint64(32)) * np.uint64(max(int(count), 0))) >> np.uint64(32)).astype(np.int32)
    return out


# ---------------------------------------------------------------------------------------------------------------- fp32 residual
def fma32(a, b, c) -> np.ndarray:
    """fp32 fused multiply-add, exactly: the product of two fp32 numbers is exact in float64; the float64 sum is rounded to ODD
    (TwoSum gives the rounding error), after which the rounding to fp32 cannot be a double rounding (53 >= 2 * 24 + 2)."""
    a64, b64, c64 = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        p = a64 * b64
        s = p + c64
        bb = s - p
        e = (p - (s - bb)) + (c64 - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0.0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def transform_points(T, s) -> np.ndarray:
    """se3_row for every row: T [..., 3, 4] fp32, s [..., 3] fp32 (broadcast) -> [..., 3] fp32."""
    T = np.asarray(T, np.float32)
    s = np.asarray(s, np.float32)
    x, y, z = s[..., 0:1], s[..., 1:2], s[..., 2:3]
    with np.errstate(over="ignore", invalid="ignore"):
        acc = (x * T[..., 0]).astype(np.float32)
        acc = fma32(y, T[..., 1], acc)
        acc = fma32(z, T[..., 2], acc)
        return (acc + T[..., 3]).astype(np.float32)


def residual2(T, s, q) -> np.ndarray:
    """d2 [...] fp32 of the correspondences (s, q) under T, in the device's rounding sequence."""
    with np.errstate(over="ignore", invalid="ignore"):
        d = (transform_points(T, s) - np.asarray(q, np.float32)).astype(np.float32)
        dd = (d * d).astype(np.float32)
        return ((dd[..., 0] + dd[..., 1]).astype(np.float32) + dd[..., 2]).astype(np.float32)


def thr2_of(max_dist: float) -> np.float32:
    return np.float32(np.float32(max_dist) * np.float32(max_dist))


def count_inliers(T, cs, cq, count: int, thr2) -> np.ndarray:
    """Inlier counts of the transforms T [H, 3, 4] (or [3, 4]) over the first ``count`` gathered rows: exact integers."""
    T = np.asarray(T, np.float32)
    single = T.ndim == 2
    T = T.reshape(-1, 1, 3, 4)
    out = np.zeros(T.shape[0], np.int64)
    step = max(1, (1 << 21) // max(count, 1))
    for h0 in range(0, T.shape[0], step):
        d2 = residual2(T[h0:h0 + step], cs[None, :count], cq[None, :count])
        out[h0:h0 + step] = (d2 < thr2).sum(axis=1)
    return out[0] if single else out


# ---------------------------------------------------------------------------------------------------------------- gather
def gather(points_src, points_ref, corr, count: Optional[int] = None):
    """-> (cs [M,3], cq [M,3] fp32 with dead / non-finite rows parked, count, invalid bits)."""
    src = np.asarray(points_src, np.float32)
    ref = np.asarray(points_ref, np.float32)
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    M = corr.shape[0]
    count = M if count is None else max(0, min(int(count), M))
    a = np.clip(corr[:, 0], 0, src.shape[0] - 1)
    b = np.clip(corr[:, 1], 0, ref.shape[0] - 1)
    invalid = 2 if (np.any(a[:count] != corr[:count, 0]) or np.any(b[:count] != corr[:count, 1])) else 0
    cs = src[a, :3].copy()
    cq = ref[b, :3].copy()
    dead = ~(np.isfinite(cs).all(1) & np.isfinite(cq).all(1))
    dead[count:] = True
    cs[dead] = 0.0
    cq[dead] = FLT_MAX
    return cs, cq, count, invalid


def is_parked(cs, cq) -> np.ndarray:
    return (cq == FLT_MAX).all(-1) & (cs == 0).all(-1)


# ---------------------------------------------------------------------------------------------------------------- fit
def kabsch64(s, q, w=None):
    """float64 Kabsch of s -> q ([..., n, 3]), optional weights [..., n]: (T [..., 3, 4] float64, singular values [..., 3])."""
    s = np.asarray(s, np.float64)
    q = np.asarray(q, np.float64)
    n = s.shape[-2]
    if w is None:
        ms = np.zeros(s.shape[:-2] + (3,))
        mq = np.zeros_like(ms)
        for k in range(n):                      # sample order
            ms = ms + s[..., k, :]
            mq = mq + q[..., k, :]
        ms, mq = ms / float(n), mq / float(n)
        H = np.zeros(s.shape[:-2] + (3, 3))
        for k in range(n):
            H = H + (s[..., k, :] - ms)[..., :, None] * (q[..., k, :] - mq)[..., None, :]
    else:
        w = np.asarray(w, np.float64)
        wn = w / (w.sum(-1, keepdims=True) + 1e-16)
        ms = (s * wn[..., None]).sum(-2)
        mq = (q * wn[..., None]).sum(-2)
        H = np.einsum("...ka,...kb->...ab", s - ms[..., None, :], (q - mq[..., None, :]) * wn[..., None])
    with np.errstate(invalid="ignore"):
        U, S, Vh = np.linalg.svd(np.where(np.isfinite(H), H, 0.0))
    V = np.swapaxes(Vh, -1, -2)
    d = np.where(np.linalg.det(V @ np.swapaxes(U, -1, -2)) > 0, 1.0, -1.0)
    D = np.zeros_like(H)
    D[..., 0, 0] = 1.0
    D[..., 1, 1] = 1.0
    D[..., 2, 2] = d
    R = V @ D @ np.swapaxes(U, -1, -2)
    t = mq - ((R[..., 0] * ms[..., 0:1] + R[..., 1] * ms[..., 1:2]) + R[..., 2] * ms[..., 2:3])
    T = np.concatenate([R, t[..., None]], -1)
    T = np.where(np.isfinite(H).all((-1, -2))[..., None, None], T, np.nan)
    return T, S


def hypotheses(cs, cq, count: int, rows, n: int, thr2, edge_sim: float) -> Dict[str, np.ndarray]:
    """Fit and check the samples ``rows`` [H, 4].  Returns T [H,3,4] fp32 (zeros where the sample was rejected before the fit),
    valid [H] bool, sigma [H,3] (singular values of the sample covariance), margin [H] (the smallest relative distance of a
    check's two sides: a verdict with a margin below ~1e-4 may legitimately differ on the device), fitted [H] bool."""
    rows = np.asarray(rows)[:, :n]
    Hn = rows.shape[0]
    pre = np.full(Hn, count >= n)
    for a in range(n):
        for b in range(a + 1, n):
            pre &= rows[:, a] != rows[:, b]
    safe = np.clip(rows, 0, max(cs.shape[0] - 1, 0))
    s, q = cs[safe], cq[safe]                                           # [H, n, 3]
    pre &= ~is_parked(s, q).any(1)
    T = np.zeros((Hn, 3, 4), np.float32)
    sigma = np.zeros((Hn, 3))
    valid = pre.copy()
    margin = np.full(Hn, np.inf)
    if pre.any():
        T64, S = kabsch64(s[pre], q[pre])
        with np.errstate(over="ignore", invalid="ignore"):
            Tf = T64.astype(np.float32)
        T[pre], sigma[pre] = Tf, S
        ok = np.isfinite(Tf).all((1, 2))
        mg = np.full(ok.shape, np.inf)
        if edge_sim > 0:
            for a in range(n):
                for b in range(a + 1, n):
                    ls = np.sqrt(((s[pre, a].astype(np.float64) - s[pre, b]) ** 2).sum(-1))
                    lq = np.sqrt(((q[pre, a].astype(np.float64) - q[pre, b]) ** 2).sum(-1))
                    e = float(np.float32(edge_sim))
                    ok &= (ls >= e * lq) & (lq >= e * ls)
                    scale = np.maximum(np.maximum(ls, lq), 1e-300)
                    mg = np.minimum(mg, np.minimum(np.abs(ls - e * lq), np.abs(lq - e * ls)) / scale)
        d2 = residual2(Tf[:, None], s[pre], q[pre])                    # [H', n]
        ok &= (d2 < thr2).all(1)
        with np.errstate(invalid="ignore"):
            mg = np.minimum(mg, np.nanmin(np.abs(d2.astype(np.float64) - float(thr2)) / float(thr2), axis=1))
        valid[pre] = ok
        margin[pre] = mg
    return {"T": T, "valid": valid, "sigma": sigma, "margin": margin, "fitted": pre}


# ---------------------------------------------------------------------------------------------------------------- pick, refit
def pick(valid, counts) -> int:
    """arg-max of (count, lower h) over the valid hypotheses, or -1."""
    valid = np.asarray(valid, bool)
    if not valid.any():
        return -1
    c = np.where(valid, np.asarray(counts, np.int64), -1)
    return int(np.argmax(c))                                            # numpy's argmax returns the first maximum


def refit_sequence(T0, cs, cq, count: int, thr2, refine_iters: int):
    """[T_0 .. T_r] fp32 and their counts: T_{r+1} = Kabsch(all inliers of T_r) in float64."""
    Ts, cnts = [np.asarray(T0, np.float32)], []
    cnts.append(int(count_inliers(Ts[0], cs, cq, count, thr2)))
    for _ in range(refine_iters):
        w = (residual2(Ts[-1], cs[:count], cq[:count]) < thr2).astype(np.float64)
        if w.sum() > 0:
            T64, _ = kabsch64(cs[:count], cq[:count], w)
            Tn = T64.astype(np.float32)
        else:
            Tn = IDENTITY.copy()
        Ts.append(Tn)
        cnts.append(int(count_inliers(Tn, cs, cq, count, thr2)))
    return Ts, cnts


def finish(Ts, cnts, cs, cq, count: int, thr2, h: int, n_valid: int):
    """(T_out, stats [5]) from the refit sequence: last largest count; RMSE over the fp32 residuals in float64."""
    c = np.asarray(cnts)
    best = int(len(c) - 1 - np.argmax(c[::-1]))
    T = Ts[best]
    d2 = residual2(T, cs[:count], cq[:count])
    inl = d2 < thr2
    k = int(inl.sum())
    rmse = float(np.sqrt(d2[inl].astype(np.float64).sum() / k)) if k else 0.0
    return T, np.array([k / count if count else 0.0, rmse, float(h), float(n_valid), float(k)])


def ransac_pair(points_src, points_ref, corr, count=None, max_dist=0.05, ransac_n=3, edge_sim=0.9, hypotheses_n=1024,
                refine_iters=2, seed=0, p=0, T_init=None) -> Dict[str, np.ndarray]:
    """One pair through the whole rule.  ``p`` is the pair's index in the batch (it enters the draws)."""
    if ransac_n not in (3, 4):
        raise ValueError("ransac_n must be 3 or 4")
    if not 1 <= hypotheses_n <= MAX_HYPOTHESES:
        raise ValueError("hypotheses out of range")
    cs, cq, count, invalid = gather(points_src, points_ref, corr, count)
    thr2 = thr2_of(max_dist)
    rows = sample_rows(seed, p, np.arange(hypotheses_n), ransac_n, count)
    hyp = hypotheses(cs, cq, count, rows, ransac_n, thr2, edge_sim)
    counts = np.zeros(hypotheses_n, np.int64)
    if hyp["valid"].any():
        counts[hyp["valid"]] = count_inliers(hyp["T"][hyp["valid"]], cs, cq, count, thr2)
    h = pick(hyp["valid"], counts)
    out = {"hyp_sample": rows, "hyp_T": hyp["T"], "hyp_valid": hyp["valid"], "hyp_count": counts, "sigma": hyp["sigma"],
           "margin": hyp["margin"], "invalid": invalid, "h": h, "cs": cs, "cq": cq, "count": count}
    if h < 0:
        T0 = IDENTITY.copy() if T_init is None else np.asarray(T_init, np.float32).reshape(3, 4)
        out.update(T=T0, T_winner=T0, stats=np.array([0.0, 0.0, -1.0, 0.0, 0.0]))
        return out
    Ts, cnts = refit_sequence(hyp["T"][h], cs, cq, count, thr2, refine_iters)
    T, stats = finish(Ts, cnts, cs, cq, count, thr2, h, int(hyp["valid"].sum()))
    out.update(T=T, T_winner=hyp["T"][h], stats=stats, refit_counts=np.array(cnts))
    return out


def ransac(points_src, points_ref, corr, counts=None, T_init=None, **kw):
    """The batch: pair ``p`` of [P, ...] inputs with its own draws.  Returns a list of ``ransac_pair`` results."""
    P = len(points_src)
    return [ransac_pair(points_src[p], points_ref[p], corr[p], None if counts is None else int(counts[p]), p=p,
                        T_init=None if T_init is None else T_init[p], **kw) for p in range(P)]


# ---------------------------------------------------------------------------------------------------------------- correspondences
def feature_correspondences(desc_src, desc_ref, mutual: bool = True):
    """Mutual-nearest-neighbour list of one pair in float64 (exact arg-min, ties to the lower index): (corr [J,2] int32 with -1
    padding, count).  The device decides in fp32: compare on descriptors whose nearest / second-nearest gap is far above 1e-6."""
    a = np.asarray(desc_src, np.float64)
    b = np.asarray(desc_ref, np.float64)
    D = ((a * a).sum(1)[:, None] - 2.0 * a @ b.T) + (b * b).sum(1)[None, :]
    ab = D.argmin(1)
    keep = np.ones(a.shape[0], bool)
    if mutual:
        keep = D.argmin(0)[ab] == np.arange(a.shape[0])
    corr = np.full((a.shape[0], 2), -1, np.int32)
    j = np.nonzero(keep)[0]
    corr[:len(j), 0] = j
    corr[:len(j), 1] = ab[j]
    return corr, int(len(j))


# ---------------------------------------------------------------------------------------------------------------- test problems
def make_problem(M: int, outlier_frac: float, noise: float, seed: int, extent: float = 3.0):
    """A synthetic correspondence problem: M src points in a cube of ``extent`` metres (3 m: the indoor scale that a 0.05 m
    threshold = 2 x a 0.025 m voxel belongs to; a pose is judged at the origin, so the extent is the lever arm of its rotation error), a random rigid motion (rotation up to
    ~1 rad, translation up to 2 m), Gaussian noise on the inliers' ref side, and a fraction of rows whose ref point is replaced by
    an unrelated point of the cube.  corr is the identity list.  Returns dict(src, ref, corr, T_gt [3,4] float64, inlier [M] bool)."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-extent / 2, extent / 2, (M, 3)).astype(np.float32)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(0.3, 1.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    t = rng.uniform(-2, 2, 3)
    ref = src.astype(np.float64) @ R.T + t + rng.normal(scale=noise, size=(M, 3))
    out = rng.permutation(M)[:int(round(outlier_frac * M))]
    ref[out] = rng.uniform(-extent / 2, extent / 2, (len(out), 3)) @ R.T + t
    inl = np.ones(M, bool)
    inl[out] = False
    corr = np.stack([np.arange(M), np.arange(M)], 1).astype(np.int32)
    return {"src": src, "ref": ref.astype(np.float32), "corr": corr, "T_gt": np.concatenate([R, t[:, None]], 1), "inlier": inl}


def pose_error(T, T_gt):
    """(rotation angle in rad, translation distance) between two [3,4] poses."""
    T, T_gt = np.asarray(T, np.float64), np.asarray(T_gt, np.float64)
    c = (np.trace(T[:, :3].T @ T_gt[:, :3]) - 1.0) / 2.0
    return float(np.arccos(np.clip(c, -1.0, 1.0))), float(np.linalg.norm(T[:, 3] - T_gt[:, 3]))
