"""Host restatement of the fast-global-registration pose rule of ``csrc/fgr.hip`` (include/dsir.h, dsir_fgr_correspondence) in numpy.

FGR (Zhou, Park, Koltun, ECCV 2016) is open3d's ``registration_fgr_based_on_feature_matching``; open3d cannot be imported here, so
parity is unpinned and the engine owns the rule.  This module states the same rule a second time, the way ``ransac.py`` and
``consensus.py`` do for their stages: the tests compare the device against it, the product path never calls it.

The rule, per pair ``p`` (the header of csrc/fgr.hip has the full text):

* gather as ``ransac.gather``: clamp (reported), park non-finite and dead rows;
* tuple test: trial ``t`` of ``min(100 count, max_trials)`` draws three rows with RANSAC's keys (``ransac.sample_rows`` with the trial
  in the place of the hypothesis); accepted iff on every edge ``d2s ts2 < d2q`` and ``d2q ts2 < d2s`` in fp32, ``d2 = (dx dx + dy dy)
  + dz dz``, ``ts2 = fp32(tuple_scale^2)``; the list is the rows of the first ``max_tuples`` accepted trials in trial order, duplicates
  kept.  Without the test: every live row that is not parked, ascending.  Fewer than 3 rows: no pose;
* normalise in float64: means of the listed points, ``scale`` = the largest distance of a listed point from its side's mean;
* ``iterations`` Gauss-Newton steps in float64 from ``T = I``, ``mu = 1``: weights ``l = (mu / (mu + r.r))^2``, the 6 x 6 system of the
  three residual components, ``solve`` (the LDL^T of csrc/icp_plane.h with its singularity rule; a refusal ends the loop),
  ``T <- M(x) T`` with ``M = Rz Ry Rx``; every fourth iteration ``mu /= division_factor`` while ``mu > (max_dist / scale)^2``;
* un-normalise, round to fp32 once; that pose is the single candidate of the RANSAC tail (count, refits, finish).

Everything integer (draws, verdicts, the list) is exact against the device; the float64 sums are added in another order there, so
the trajectory agrees to rounding (tests/test_gpu_fgr.py states the tolerance and where it comes from).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from . import ransac as rs

MAX_TUPLES = 65536           # DSIR_FGR_MAX_TUPLES of include/dsir.h
MAX_TRIALS = 1 << 22         # DSIR_FGR_MAX_TRIALS
MAX_ITERS = 1024             # DSIR_FGR_MAX_ITERS
TRIALS_PER_ROW = 100         # kFgrTrialsPerRow of csrc/fgr.h
PIVOT_MIN = 1e-10            # kIcpPlanePivotMin of csrc/icp_plane.h


def trials_of(count: int, max_trials: int) -> int:
    return min(TRIALS_PER_ROW * max(int(count), 0), int(max_trials))


def ts2_of(tuple_scale: float) -> np.float32:
    return np.float32(np.float32(tuple_scale) * np.float32(tuple_scale))


# ---------------------------------------------------------------------------------------------------------------- the row list
def _d2(a, b) -> np.ndarray:
    with np.errstate(over="ignore", invalid="ignore"):
        d = (a - b).astype(np.float32)
        dd = (d * d).astype(np.float32)
        return ((dd[..., 0] + dd[..., 1]).astype(np.float32) + dd[..., 2]).astype(np.float32)


def tuple_trials(cs, cq, count: int, seed: int, p: int, tuple_scale: float, trials):
    """The trials ``trials`` of pair ``p``: (rows [len, 3] int32, accepted [len] bool)."""
    ts2 = ts2_of(tuple_scale)
    rows = rs.sample_rows(seed, p, trials, 3, count)[:, :3]
    s, q = cs[rows], cq[rows]
    ok = np.ones(rows.shape[0], bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            for b in range(a + 1, 3):
                d2s, d2q = _d2(s[:, a], s[:, b]), _d2(q[:, a], q[:, b])
                ok &= ((d2s * ts2).astype(np.float32) < d2q) & ((d2q * ts2).astype(np.float32) < d2s)
    return rows, ok


def tuple_rows(cs, cq, count: int, seed: int, p: int, tuple_scale: float, max_tuples: int, max_trials: int):
    """-> (rows [n] int32 of the list, trials).  Vectorised; tests/test_fgr_host.py checks it against a plain loop."""
    n = trials_of(count, max_trials)
    out = []
    kept = 0
    step = 1 << 16
    for t0 in range(0, n, step):
        rows, ok = tuple_trials(cs, cq, count, seed, p, tuple_scale, np.arange(t0, min(n, t0 + step)))
        acc = rows[ok][:max(max_tuples - kept, 0)]
        out.append(acc)
        kept += acc.shape[0]
        if kept >= max_tuples:
            break
    rows = np.concatenate(out).reshape(-1) if out else np.zeros(0, np.int32)
    return rows.astype(np.int32), n


def all_rows(cs, cq, count: int) -> np.ndarray:
    return np.nonzero(~rs.is_parked(cs[:count], cq[:count]))[0].astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- the solve
def tri(r: int, c: int) -> int:
    return r * 6 - r * (r - 1) // 2 + (c - r)


def solve(A, b, rows: float):
    """icp_plane_solve of csrc/icp_plane.h: A x = -b through the LDL^T of the matrix scaled to unit diagonal.  -> (x [6], ok)."""
    x = np.zeros(6)
    if not rows >= 6.0:
        return x, False
    s = np.zeros(6)
    for i in range(6):
        d = A[i, i]
        if not d > 0.0 or not np.isfinite(d):
            return x, False
        s[i] = 1.0 / np.sqrt(d)
    L = np.zeros((6, 6))
    D = np.zeros(6)
    for j in range(6):
        d = 1.0
        for k in range(j):
            d -= L[j, k] * L[j, k] * D[k]
        if not d >= PIVOT_MIN:
            return x, False
        D[j] = d
        for i in range(j + 1, 6):
            v = A[j, i] * s[i] * s[j]
            for k in range(j):
                v -= L[i, k] * L[j, k] * D[k]
            L[i, j] = v / d
    y = np.zeros(6)
    for i in range(6):
        v = -b[i] * s[i]
        for k in range(i):
            v -= L[i, k] * y[k]
        y[i] = v
    y /= D
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v -= L[k, i] * y[k]
        y[i] = v
    y *= s
    if not np.isfinite(y).all():
        return x, False
    return y, True


def vec6_to_T(x) -> np.ndarray:
    """icp_plane_transform: R = Rz(x2) Ry(x1) Rx(x0), t = (x3, x4, x5) -> [3, 4] float64."""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    return np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa, x[3]],
                     [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa, x[4]],
                     [-sb, cb * sa, cb * ca, x[5]]])


# ---------------------------------------------------------------------------------------------------------------- normalise, optimise
def normalise(s, q):
    """float64 points of the listed rows [n, 3] -> (ms, mq, scale)."""
    n = s.shape[0]
    ms, mq = s.sum(0) / float(n), q.sum(0) / float(n)
    ds, dq = s - ms, q - mq
    far2 = max(((ds[:, 0] * ds[:, 0] + ds[:, 1] * ds[:, 1]) + ds[:, 2] * ds[:, 2]).max(),
               ((dq[:, 0] * dq[:, 0] + dq[:, 1] * dq[:, 1]) + dq[:, 2] * dq[:, 2]).max())
    return ms, mq, float(np.sqrt(far2))


def unnormalise(T, ms, mq, scale) -> np.ndarray:
    """The normalised-frame pose [3, 4] float64 in the frame of the inputs, float64."""
    R = T[:, :3]
    Rm = (R[:, 0] * ms[0] + R[:, 1] * ms[1]) + R[:, 2] * ms[2]
    return np.concatenate([R, ((scale * T[:, 3] + mq) - Rm)[:, None]], 1)


def system(T, sn, qn, mu: float):
    """(A [6, 6] symmetric, b [6], energy) of one iteration over the normalised rows."""
    u = ((sn[:, 0:1] * T[:, 0] + sn[:, 1:2] * T[:, 1]) + sn[:, 2:3] * T[:, 2]) + T[:, 3]
    r = qn - u
    rr = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    w = mu / (mu + rr)
    l = w * w
    A = np.zeros((6, 6))
    b = np.zeros(6)
    for c in range(3):
        c1, c2 = (c + 1) % 3, (c + 2) % 3
        J = np.zeros((sn.shape[0], 6))
        J[:, c1] = -u[:, c2]
        J[:, c2] = u[:, c1]
        J[:, 3 + c] = -1.0
        lJ = l[:, None] * J
        A += lJ.T @ J
        b += (lJ * r[:, c:c + 1]).sum(0)
    e = 1.0 - np.sqrt(l)
    return A, b, float((l * rr + mu * (e * e)).sum())


def optimise(sn, qn, floor: float, iterations: int, division_factor: float) -> Dict[str, np.ndarray]:
    T = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    mu = 1.0
    df = float(np.float32(division_factor))
    iter_T = np.zeros((iterations, 3, 4))
    iter_mu = np.zeros(iterations)
    iter_energy = np.zeros(iterations)
    iters_run = 0
    for it in range(iterations):
        A, b, energy = system(T, sn, qn, mu)
        iter_mu[it], iter_energy[it] = mu, energy
        x, ok = solve(A, b, float(sn.shape[0]))
        if not ok:
            iters_run = -(it + 1)
            break
        Mx = vec6_to_T(x)
        Tn = np.zeros((3, 4))
        for a in range(3):
            Tn[a] = (Mx[a, 0] * T[0] + Mx[a, 1] * T[1]) + Mx[a, 2] * T[2]
            Tn[a, 3] += Mx[a, 3]
        T = Tn
        iter_T[it] = T
        iters_run = it + 1
        if df > 1.0 and it % 4 == 0 and mu > floor:
            mu = mu / df
    return {"T": T, "iter_T": iter_T, "iter_mu": iter_mu, "iter_energy": iter_energy, "iters_run": iters_run}


def pose_from_rows(cs, cq, rows, max_dist: float, iterations: int, division_factor: float) -> Dict[str, np.ndarray]:
    """Steps 3 - 5 on a given row list.  ``T`` is the fp32 candidate pose [3, 4] or None (no pose); ``T64`` the same before rounding."""
    out = {"norm": np.zeros(8), "iter_T": np.zeros((iterations, 3, 4)), "iter_mu": np.zeros(iterations),
           "iter_energy": np.zeros(iterations), "iters_run": 0, "T": None, "T64": None}
    rows = np.asarray(rows, np.int64)
    if rows.shape[0] < 3:
        return out
    s, q = cs[rows].astype(np.float64), cq[rows].astype(np.float64)
    ms, mq, scale = normalise(s, q)
    out["norm"] = np.concatenate([ms, mq, [scale, 0.0]])
    if not (scale > 0.0 and np.isfinite(scale)):
        return out
    md = float(np.float32(max_dist))
    opt = optimise((s - ms) / scale, (q - mq) / scale, (md / scale) * (md / scale), iterations, division_factor)
    out.update({k: opt[k] for k in ("iter_T", "iter_mu", "iter_energy", "iters_run")})
    T64 = unnormalise(opt["T"], ms, mq, scale)
    with np.errstate(over="ignore", invalid="ignore"):
        T = T64.astype(np.float32)
    if np.isfinite(T).all():
        out["T"], out["T64"] = T, T64
    return out


# ---------------------------------------------------------------------------------------------------------------- the whole rule
def fgr_pair(points_src, points_ref, corr, count: Optional[int] = None, max_dist: float = 0.05, tuple_test: bool = True,
             tuple_scale: float = 0.95, max_tuples: int = 1000, max_trials: int = 1 << 20, iterations: int = 64,
             division_factor: float = 1.4, refine_iters: int = 2, seed: int = 0, p: int = 0, T_init=None, rows=None) -> Dict[str, np.ndarray]:
    """One pair through the whole rule.  ``p`` is the pair's index in the batch (it enters the draws).  ``rows``: a row list to use
    in the place of step 2's (the device's own, in the trajectory tests)."""
    if not 0.0 < float(np.float32(tuple_scale)) <= 1.0:
        raise ValueError("tuple_scale outside (0, 1]")
    if not 1 <= max_tuples <= MAX_TUPLES or not 1 <= max_trials <= MAX_TRIALS or not 1 <= iterations <= MAX_ITERS:
        raise ValueError("max_tuples, max_trials or iterations out of range")
    cs, cq, count, invalid = rs.gather(points_src, points_ref, corr, count)
    thr2 = rs.thr2_of(max_dist)
    trials = 0
    if rows is None:
        if tuple_test:
            rows, trials = tuple_rows(cs, cq, count, seed, p, tuple_scale, max_tuples, max_trials)
        else:
            rows = all_rows(cs, cq, count)
    elif tuple_test:
        trials = trials_of(count, max_trials)
    rows = np.asarray(rows, np.int32)
    out = pose_from_rows(cs, cq, rows, max_dist, iterations, division_factor)
    out.update(rows=rows, n_rows=int(rows.shape[0]), trials=trials, invalid=invalid, cs=cs, cq=cq, count=count)
    if out["T"] is None:
        T0 = rs.IDENTITY.copy() if T_init is None else np.asarray(T_init, np.float32).reshape(3, 4)
        out.update(T_candidate=None, T=T0, stats=np.array([0.0, 0.0, -1.0, 0.0, 0.0]))
        return out
    cand = out["T"]
    Ts, cnts = rs.refit_sequence(cand, cs, cq, count, thr2, refine_iters)
    T, stats = rs.finish(Ts, cnts, cs, cq, count, thr2, 0, 1)
    out.update(T_candidate=cand, T=T, stats=stats, refit_counts=np.array(cnts))
    return out


def fgr(points_src, points_ref, corr, counts=None, T_init=None, **kw):
    """The batch: pair ``p`` of [P, ...] inputs with its own draws.  Returns a list of ``fgr_pair`` results."""
    P = len(points_src)
    return [fgr_pair(points_src[p], points_ref[p], corr[p], None if counts is None else int(counts[p]), p=p,
                     T_init=None if T_init is None else T_init[p], **kw) for p in range(P)]
