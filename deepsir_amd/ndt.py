"""NDT registration on the host: the rule of csrc/ndt.hip (its header states it once) restated in numpy float64.

PCL is not installable here, so **parity is unpinned** and the rule is the engine's own; this file is what the HIP path
(``Engine.ndt_refine``, ``Engine.ndt_map``; include/dsir.h ``dsir_ndt_refine``, ``dsir_ndt_map``) is held to.  The order of
operations is the device's wherever the order decides a bit of a per-point or per-cell value (the lattice, the keys, the stable
sort, the cell means and covariances in run order, q, e, g, the 21 + 6 products).  What differs: the eigen-decomposition of a
cell's covariance (``numpy.linalg.eigh`` here, the Jacobi ``svd3`` there), ``exp`` / ``log`` / ``sin`` / ``cos`` in the last bit,
the order in which the source points' contributions are added up (numpy's here; chunks of 1024, wave butterflies there), and
the fp32 transform arithmetic (computed in fp64 and rounded once here, a chain of fused multiply-adds there).

    ndt_constants      PCL's d1, d2, d3 from the outlier ratio and the resolution
    ndt_lattice_host   origin and cell edge of a reference cloud
    ndt_map_host       sorted keys, original indices, run lengths and the ten-double records at run heads
    ndt_step_host      the 31 sums of one iteration over moved points, and the solved update
    ndt_refine_host    the loop: (T, stats) as the engine returns them, and a trace of the step norms
"""
from __future__ import annotations

import numpy as np

MAXC = (1 << 21) - 1
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
MIN_POINTS = 6                      # PCL's min_points_per_voxel
EIG_MULT = 0.01                     # PCL's min_covar_eigvalue_mult
PIVOT_MIN = 1e-10                   # csrc/icp_plane.h kIcpPlanePivotMin
OFFSETS = np.array([[0, 0, 0], [-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]], np.int64)   # the visit order
IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))])


def ndt_constants(outlier_ratio: float = 0.55, resolution: float = 1.0):
    """-> (d1, d2, d3) in float64; the resolution enters as its fp32 value, the outlier ratio as given (the engine passes its fp32 value)"""
    o, r = float(outlier_ratio), float(np.float32(resolution))
    c1, c2 = 10.0 * (1.0 - o), o / (r * r * r)
    d3 = -np.log(c2)
    d1 = -np.log(c1 + c2) - d3
    d2 = -2.0 * np.log((-np.log(c1 * np.exp(-0.5) + c2) - d3) / d1)
    return float(d1), float(d2), float(d3)


def ndt_lattice_host(ref, resolution: float):
    """ref [K,>=3] fp32 -> (origin [3] float64, h): the per-axis minimum of the finite rows and h = max(res, longest extent / 2^20);
    without a finite row the origin is 0 and h = res"""
    p = np.ascontiguousarray(np.asarray(ref)[:, :3], np.float32).reshape(-1, 3)
    fin = np.isfinite(p).all(1)
    res = float(np.float32(resolution))
    if not fin.any():
        return np.zeros(3), res
    lo, hi = p[fin].min(0).astype(np.float64), p[fin].max(0).astype(np.float64)
    return lo, max(res, float((hi - lo).max()) / 1048576.0)


def cell_of(a, o, h):
    """cell coordinates of fp32 values a [n,3] (as float64) under the lattice: floor((a - o) / h), clamped to -2 .. MAXC + 2"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.clip(np.floor((a - o) / h), -2.0, float(MAXC + 2)).astype(np.int64)


def cell_key(c):
    c = np.asarray(c, np.int64)
    return (c[..., 0] | (c[..., 1] << 21) | (c[..., 2] << 42)).astype(np.uint64)


def ndt_map_host(ref, resolution: float):
    """ref [K,>=3] fp32 -> dict: origin [3], h, keys [K] uint64 ascending (KEY_NONE last), index [K] int32 (the original row of
    every sorted position; the sort is stable), runs [K] int32 (a run's length at its first position, else 0), records [K,10]
    float64 (mu 3, B 6 as 00 01 02 11 12 22, n at the first position of a valid cell, else 0), and for tests sums [K,9] (the
    three sums of x and the six of (x - mu)(x - mu)^T before their divisions) and lam [K,3] (the regularised eigenvalues,
    descending) at the same positions."""
    p32 = np.ascontiguousarray(np.asarray(ref)[:, :3], np.float32).reshape(-1, 3)
    K = len(p32)
    origin, h = ndt_lattice_host(p32, resolution)
    p = p32.astype(np.float64)
    fin = np.isfinite(p32).all(1)
    keys = np.full(K, KEY_NONE, np.uint64)
    if fin.any():
        keys[fin] = cell_key(np.clip(cell_of(p[fin], origin, h), 0, MAXC))
    order = np.argsort(keys, kind="stable")
    skeys = keys[order]
    runs, records, sums, lam_out = np.zeros(K, np.int32), np.zeros((K, 10)), np.zeros((K, 9)), np.zeros((K, 3))
    heads = np.flatnonzero((skeys != KEY_NONE) & np.r_[True, skeys[1:] != skeys[:-1]]) if K else np.zeros(0, np.int64)
    ends = np.r_[heads[1:], int((skeys != KEY_NONE).sum())] if len(heads) else heads
    for i, e in zip(heads, ends):
        n = int(e - i)
        runs[i] = n
        if n < MIN_POINTS:
            continue
        x = p[order[i:e]]
        sx = np.zeros(3)
        for row in x:                                   # run order
            sx = sx + row
        mu = sx / n
        d = x - mu
        prods = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1)
        sc = np.zeros(6)
        for row in prods:
            sc = sc + row
        sums[i] = np.r_[sx, sc]
        c = sc / (n - 1)
        B, lam = inverse_covariance(c)
        if B is None:
            continue
        records[i] = np.r_[mu, B, n]
        lam_out[i] = lam
    return dict(origin=origin, h=h, keys=skeys, index=order.astype(np.int32), runs=runs, records=records, sums=sums, lam=lam_out)


def inverse_covariance(c):
    """c: the six upper entries (00 01 02 11 12 22) of a cell's covariance -> (B: the six upper entries of V diag(1 / lambda') V^T,
    lambda' [3] descending), or (None, None) where lambda_1 is not a positive finite number"""
    C = np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])
    if not np.isfinite(C).all():
        return None, None
    lam, V = np.linalg.eigh(C)
    lam, V = lam[::-1], V[:, ::-1]
    if not (lam[0] > 0.0 and np.isfinite(lam[0])):
        return None, None
    lam = np.maximum(lam, EIG_MULT * lam[0])
    il = 1.0 / lam
    B = [((V[a, 0] * il[0]) * V[b, 0] + (V[a, 1] * il[1]) * V[b, 1]) + (V[a, 2] * il[2]) * V[b, 2] for a in range(3) for b in range(a, 3)]
    return np.array(B), lam


def _tri(A21):
    A = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = A21[k]
            k += 1
    return A


def solve6(A, b, rows):
    """csrc/icp_plane.h icp_plane_solve: x of A x = -b, or None where the rule calls the system singular (fewer than 6 rows, a
    diagonal entry that is not a positive finite number, a pivot of the unit-diagonal matrix below PIVOT_MIN, x not finite)"""
    if not rows >= 6:
        return None
    d = np.diag(A).astype(np.float64)
    if not (np.isfinite(d).all() and (d > 0).all()):
        return None
    s = 1.0 / np.sqrt(d)
    L, D = np.eye(6), np.zeros(6)
    for j in range(6):
        D[j] = 1.0 - sum(L[j, k] * L[j, k] * D[k] for k in range(j))
        if not D[j] >= PIVOT_MIN:
            return None
        for i in range(j + 1, 6):
            L[i, j] = (A[j, i] * s[i] * s[j] - sum(L[i, k] * L[j, k] * D[k] for k in range(j))) / D[j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = -b[i] * s[i] - sum(L[i, k] * y[k] for k in range(i))
    y /= D
    for i in range(5, -1, -1):
        y[i] -= sum(L[k, i] * y[k] for k in range(i + 1, 6))
    x = y * s
    return x if np.isfinite(x).all() else None


def vec6_to_T(x):
    """csrc/icp_plane.h icp_plane_transform: R = Rz(x2) Ry(x1) Rx(x0), t = (x3, x4, x5)"""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    return np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa, x[3]],
                     [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa, x[4]],
                     [-sb, cb * sa, cb * ca, x[5]]])


def ndt_step_host(cur, m, d2: float, neighbors: int = 7):
    """One iteration's sums over the moved points cur [J,3] fp32 against the map m (ndt_map_host) -> dict: A [6,6], b [6], score,
    matched, rows, bad (source points that are not finite), x (the solved update [6], or None: the identity update)."""
    cur32 = np.ascontiguousarray(np.asarray(cur)[:, :3], np.float32).reshape(-1, 3)
    fin = np.isfinite(cur32).all(1)
    bad = int((~fin).sum())
    s = cur32[fin].astype(np.float64)
    keys, records, K = m["keys"], m["records"], len(m["keys"])
    A21, b6, score, rows = np.zeros(21), np.zeros(6), 0.0, 0
    matched = np.zeros(len(s), bool)
    if len(s) and K:
        c = cell_of(s, m["origin"], m["h"])
        zero, one = np.zeros(len(s)), np.ones(len(s))
        Jc_all = [np.stack(v, 1) for v in ([zero, -s[:, 2], s[:, 1]], [s[:, 2], zero, -s[:, 0]], [-s[:, 1], s[:, 0], zero],
                                           [one, zero, zero], [zero, one, zero], [zero, zero, one])]
        for off in OFFSETS[:neighbors]:
            cc = c + off
            ok = ((cc >= 0) & (cc <= MAXC)).all(1)
            key = cell_key(np.where(ok[:, None], cc, 0))
            pos = np.searchsorted(keys, key, side="left")
            hit = ok & (pos < K)
            hit[hit] = keys[pos[hit]] == key[hit]
            hit[hit] = records[pos[hit], 9] >= MIN_POINTS
            if not hit.any():
                continue
            rec, sv = records[pos[hit]], s[hit]
            d = sv - rec[:, :3]
            B = {(0, 0): rec[:, 3], (0, 1): rec[:, 4], (0, 2): rec[:, 5], (1, 1): rec[:, 6], (1, 2): rec[:, 7], (2, 2): rec[:, 8]}
            Bm = lambda r, c_: B[(min(r, c_), max(r, c_))]
            q = (((((Bm(0, 0) * d[:, 0]) * d[:, 0] + (Bm(1, 1) * d[:, 1]) * d[:, 1]) + (Bm(2, 2) * d[:, 2]) * d[:, 2])
                  + 2.0 * ((Bm(0, 1) * d[:, 0]) * d[:, 1])) + 2.0 * ((Bm(0, 2) * d[:, 0]) * d[:, 2])) + 2.0 * ((Bm(1, 2) * d[:, 1]) * d[:, 2])
            with np.errstate(over="ignore", invalid="ignore"):
                e = np.exp(-(d2 * q) / 2.0)
            use = (q >= 0.0) & (e > 0.0) & np.isfinite(e)
            if not use.any():
                continue
            idx = np.flatnonzero(hit)[use]
            matched[idx] = True
            d, e, sv = d[use], e[use], sv[use]
            Bu = lambda r, c_: Bm(r, c_)[use]
            w = d2 * e
            g = [(Bu(r, 0) * d[:, 0] + Bu(r, 1) * d[:, 1]) + Bu(r, 2) * d[:, 2] for r in range(3)]
            Jc = [j[hit][use] for j in Jc_all]
            BJ = [[(Bu(r, 0) * Jc[k][:, 0] + Bu(r, 1) * Jc[k][:, 1]) + Bu(r, 2) * Jc[k][:, 2] for r in range(3)] for k in range(6)]
            k = 0
            for a in range(6):
                for b_ in range(a, 6):
                    A21[k] += float(np.sum(w * ((Jc[a][:, 0] * BJ[b_][0] + Jc[a][:, 1] * BJ[b_][1]) + Jc[a][:, 2] * BJ[b_][2])))
                    k += 1
            b6[0] += float(np.sum(w * (sv[:, 1] * g[2] - sv[:, 2] * g[1])))
            b6[1] += float(np.sum(w * (sv[:, 2] * g[0] - sv[:, 0] * g[2])))
            b6[2] += float(np.sum(w * (sv[:, 0] * g[1] - sv[:, 1] * g[0])))
            for r in range(3):
                b6[3 + r] += float(np.sum(w * g[r]))
            score += float(np.sum(e))
            rows += int(use.sum())
    A = _tri(A21)
    x = solve6(A, b6, rows) if bad == 0 else None
    return dict(A=A, b=b6, score=score, matched=int(matched.sum()), rows=rows, bad=bad, x=x)


def apply32(T, pts32):
    """the fp32 points moved by the fp32 transform T [3,4]: computed in float64, rounded once"""
    T = np.asarray(T, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return (pts32.astype(np.float64) @ T[:, :3].T + T[:, 3]).astype(np.float32)


def compose32(U, T):
    """U o T for fp32 transforms [3,4]: computed in float64, rounded once"""
    U, T = np.asarray(U, np.float32).astype(np.float64), np.asarray(T, np.float32).astype(np.float64)
    return np.hstack([U[:, :3] @ T[:, :3], (U[:, :3] @ T[:, 3] + U[:, 3])[:, None]]).astype(np.float32)


def ndt_refine_host(src, ref, T_init, resolution: float, neighbors: int = 7, max_iter: int = 30, step_tol: float = 1e-4,
                    outlier_ratio: float = 0.55, perturb_ulps=None, m=None):
    """src [J,>=3], ref [K,>=3] fp32 (J, K may be 0), T_init [3,4] -> (T [3,4] float32, stats [5] float32: mean likelihood, matched
    fraction, converged, iterations, identity updates, trace: per iteration (|rotation part of x|, |translation part of x|), or
    None for an identity update).  ``perturb_ulps``: a seed; every coordinate of the moved points is shifted by -1, 0 or +1 fp32
    ulp at random after T_init is applied and after each update (the yardstick of the GPU tests' tolerances).  ``m``: the
    reference's map if the caller has it (ndt_map_host(ref, resolution))."""
    if neighbors not in (1, 7):
        raise ValueError("neighbors must be 1 or 7")
    src32 = np.ascontiguousarray(np.asarray(src, np.float32).reshape(-1, np.asarray(src).shape[-1])[:, :3])
    ref32 = np.ascontiguousarray(np.asarray(ref, np.float32).reshape(-1, np.asarray(ref).shape[-1])[:, :3])
    J = len(src32)
    res = float(np.float32(resolution))
    tol = float(np.float32(step_tol))
    d2 = ndt_constants(float(np.float32(outlier_ratio)), res)[1]
    if m is None:
        m = ndt_map_host(ref32, res)
    rng = None if perturb_ulps is None else np.random.default_rng(perturb_ulps)

    def jitter(c):
        if rng is None or not len(c):
            return c
        step = rng.integers(-1, 2, c.shape)
        return np.where(step > 0, np.nextafter(c, np.float32(np.inf)), np.where(step < 0, np.nextafter(c, np.float32(-np.inf)), c)).astype(np.float32)

    T = np.asarray(T_init, np.float32)[:3, :4].copy()
    cur = jitter(apply32(T, src32))
    done, iters, nident, trace = False, 0, 0, []
    for _ in range(max_iter):
        if done:
            break
        x = ndt_step_host(cur, m, d2, neighbors)["x"]
        U = None
        if x is not None:
            with np.errstate(over="ignore"):
                U = vec6_to_T(x).astype(np.float32)
            if not np.isfinite(U).all():
                U = None
        iters += 1
        if U is None:
            nident += 1
            done = True
            trace.append(None)
            continue
        T = compose32(U, T)
        cur = jitter(apply32(U, cur))
        nr, nt = float(np.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])), float(np.sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]))
        trace.append((nr, nt))
        done = nr < tol and nt < tol * res
    last = ndt_step_host(cur, m, d2, neighbors)
    stats = np.array([last["score"] / J if J else 0.0, last["matched"] / J if J else 0.0, float(done), iters, nident], np.float32)
    return T, stats, trace


def matched_fraction_host(src, ref, T, resolution: float, neighbors: int = 7, outlier_ratio: float = 0.55, m=None):
    """the second statistic for a given final pose: the fraction of src moved by T (fp32) with at least one contributing visit.
    The moved points are those of ONE application of T to src, not of the loop's chain of updates."""
    src32 = np.ascontiguousarray(np.asarray(src, np.float32)[:, :3])
    if m is None:
        m = ndt_map_host(ref, resolution)
    d2 = ndt_constants(float(np.float32(outlier_ratio)), float(np.float32(resolution)))[1]
    st = ndt_step_host(apply32(T, src32), m, d2, neighbors)
    return st["matched"] / len(src32) if len(src32) else 0.0
