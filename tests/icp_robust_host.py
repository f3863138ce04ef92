"""Host restatement of the robust loss kernels of the ICP estimators (TEST INFRASTRUCTURE ONLY; a helper, not a test).

open3d's ``robust_kernel`` of ``TransformationEstimationPointToPoint/Plane``: open3d is not installable here, so **parity is
unpinned** and the rule is the engine's own (csrc/icp_robust.h, the head of csrc/icp.hip, include/dsir.h ``dsir_icp_refine_ex4``);
this file is what the HIP path is held to.

The weight of a correspondence from its squared residual q = r^2 and the scale k > 0, float64, every operation one numpy float64
operation in the order of csrc/icp_robust.h (k^2 = k * k first), so the bits are the header's:
    l2 1    huber q <= k^2 ? 1 : k / sqrt(q)    cauchy 1 / (1 + q / k^2)    gm k / ((k + q) * (k + q))    tukey q <= k^2 ? (1 - q / k^2)^2 : 0
k is the fp32 value of the scale, as the C ABI takes it.

Point-to-point (``icp_point``): ``oracle.icp.icp``'s loop; q = the fp32 squared distance of the correspondence, the weight rounded
once to fp32; the update is a float64 weighted Kabsch on those weights (w / sum w, weighted centroids, H = sum w (s - cs)(t - ct)^T,
R = V diag(1, 1, det) U^T).  All weights zero: the identity update, counted, T and the moved points keep their bits.
Point-to-plane (``icp_plane``): ``icp_plane_host.icp_plane``'s loop with weighted sums; q = r^2 of the float64 plane residual,
A = sum (w J) J^T, b = sum (w J) r; a correspondence whose weight is not > 0 is not a row; then ``icp_plane_host.solve`` as it is.
Under every kernel the search, fitness, inlier RMSE (unweighted point distances), convergence test and max_iter are unchanged.
"""
from __future__ import annotations

import numpy as np

from icp_plane_host import IDENTITY, solve, vec6_to_T
from oracle.icp import _nearest

KERNELS = {"l2": 0, "huber": 1, "cauchy": 2, "gm": 3, "tukey": 4}


def weight(kernel: str, q, k: float):
    """float64 weights of squared residuals q under ``kernel`` with scale k: the operation order of csrc/icp_robust.h"""
    q = np.asarray(q, np.float64)
    k = np.float64(k)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kernel == "l2":
            return np.ones_like(q)
        if kernel == "huber":
            kk = k * k
            return np.where(q <= kk, np.float64(1.0), k / np.sqrt(q))
        if kernel == "cauchy":
            kk = k * k
            u = q / kk
            d = np.float64(1.0) + u
            return np.float64(1.0) / d
        if kernel == "gm":
            s = k + q
            ss = s * s
            return k / ss
        if kernel == "tukey":
            kk = k * k
            u = q / kk
            t = np.float64(1.0) - u
            return np.where(q <= kk, t * t, np.float64(0.0))
    raise ValueError(kernel)


def _scale(kernel, k):
    return 0.0 if kernel == "l2" else float(np.float32(k))


def weighted_kabsch(src, tgt, w):
    """float64 weighted Kabsch -> [3,4], or None when every weight is zero (the identity update)"""
    w = np.asarray(w, np.float64)
    S = w.sum()
    if len(w) == 0 or S == 0.0:
        return None
    wn = w / S
    cs, ct = (src * wn[:, None]).sum(0), (tgt * wn[:, None]).sum(0)
    H = (src - cs).T @ ((tgt - ct) * wn[:, None])
    U, _, Vt = np.linalg.svd(H)
    V = Vt.T
    d = 1.0 if np.linalg.det(V @ U.T) > 0 else -1.0
    R = V @ np.diag([1.0, 1.0, d]) @ U.T
    return np.hstack([R, (ct - R @ cs)[:, None]])


def weighted_normal_sums(s, t, n, kernel, k):
    """(A [6,6], b [6], rows) over the correspondences that contribute: finite t and n, n != 0, weight > 0"""
    s, t, n = (np.asarray(a, np.float64).reshape(-1, 3) for a in (s, t, n))
    use = np.isfinite(t).all(1) & np.isfinite(n).all(1) & (n != 0).any(1)
    s, t, n = s[use], t[use], n[use]
    d = s - t
    r = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    w = weight(kernel, r * r, k)
    keep = w > 0
    s, n, r, w = s[keep], n[keep], r[keep], w[keep]
    J = np.concatenate([np.cross(s, n), n], 1)
    wJ = J * w[:, None]
    return wJ.T @ J, wJ.T @ r, int(keep.sum())


def _loop(src, tgt, T_init, max_corr_dist, max_iter, rel_fitness, rel_rmse, perturb_ulps, trace, update):
    """the loop both estimators share (oracle.icp.icp's): ``update(cur64, tgt64, idx, ok, d2)`` -> [3,4] or None (identity, counted)"""
    src32, tgt32 = np.ascontiguousarray(src[:, :3], np.float32), np.ascontiguousarray(tgt[:, :3], np.float32)
    search32 = np.where(np.isfinite(tgt32).all(1, keepdims=True), tgt32, np.float32(3e18))
    r2 = np.float32(max_corr_dist) * np.float32(max_corr_dist)
    T = np.asarray(T_init, np.float64).copy()
    cur = (src32 @ T[:, :3].astype(np.float32).T + T[:, 3].astype(np.float32)).astype(np.float32)
    rng = None if perturb_ulps is None else np.random.default_rng(perturb_ulps)

    def evaluate(c):
        with np.errstate(invalid="ignore", over="ignore"):
            idx, d2 = _nearest(c, search32)
            ok = d2 <= r2
        n = int(ok.sum())
        return idx, ok, d2, n / len(c), (float(np.sqrt(d2[ok].astype(np.float64).sum() / n)) if n else 0.0)

    idx, ok, d2, fitness, rmse = evaluate(cur)
    if trace is not None:
        trace.append((fitness, rmse))
    converged, iters, identity = False, 0, 0
    for _ in range(max_iter):
        upd = update(cur.astype(np.float64), tgt32.astype(np.float64), idx, ok, d2)
        if upd is None:
            identity += 1
        else:
            T = np.hstack([upd[:, :3] @ T[:, :3], (upd[:, :3] @ T[:, 3] + upd[:, 3])[:, None]])
            cur = (cur.astype(np.float64) @ upd[:, :3].T + upd[:, 3]).astype(np.float32)
            if rng is not None:
                step = rng.integers(-1, 2, cur.shape)
                cur = np.where(step > 0, np.nextafter(cur, np.float32(np.inf)),
                               np.where(step < 0, np.nextafter(cur, np.float32(-np.inf)), cur)).astype(np.float32)
        idx, ok, d2, f2, e2 = evaluate(cur)
        if trace is not None:
            trace.append((f2, e2))
        iters += 1
        done = abs(fitness - f2) < rel_fitness and abs(rmse - e2) < rel_rmse
        fitness, rmse = f2, e2
        if done:
            converged = True
            break
    return T, fitness, rmse, converged, iters, identity


def icp_point(src, tgt, T_init, max_corr_dist, kernel="l2", kernel_scale=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
              perturb_ulps=None, trace=None, weights=None):
    """src [J,>=3], tgt [K,>=3] fp32, T_init [3,4] -> (T [3,4] float64, fitness, inlier_rmse, converged, iterations, identity updates
    taken because every weight was zero).  ``weights``: a list that receives every update's fp32 weights of the matched rows."""
    k = _scale(kernel, kernel_scale)

    def update(cur, tgt64, idx, ok, d2):
        w32 = weight(kernel, d2[ok].astype(np.float64), k).astype(np.float32)
        if weights is not None:
            weights.append(w32)
        return weighted_kabsch(cur[ok], tgt64[idx[ok]], w32)

    return _loop(src, tgt, T_init, max_corr_dist, max_iter, rel_fitness, rel_rmse, perturb_ulps, trace, update)


def icp_plane(src, tgt, normals, T_init, max_corr_dist, kernel="l2", kernel_scale=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
              perturb_ulps=None, trace=None):
    """as ``icp_plane_host.icp_plane`` -> (T, fitness, inlier_rmse, converged, iterations, identity updates: fewer than 6 rows of
    weight > 0, a singular system, or a moved source point that is not finite)"""
    k = _scale(kernel, kernel_scale)
    nrm = np.asarray(normals, np.float32)[:, :3].astype(np.float64)

    def update(cur, tgt64, idx, ok, d2):
        if not np.isfinite(cur).all():
            return None
        A, b, rows = weighted_normal_sums(cur[ok], tgt64[idx[ok]], nrm[idx[ok]], kernel, k)
        x = solve(A, b, rows)
        return None if x is None else vec6_to_T(x)

    return _loop(src, tgt, T_init, max_corr_dist, max_iter, rel_fitness, rel_rmse, perturb_ulps, trace, update)


def outlier_case(case, share, offset, seed=0):
    """A ``test_icp_plane.surface_case`` with a fixed share of its source points replaced by copies displaced by ONE common offset
    (given in the reference frame, so the displaced points lie ``offset`` off their partners under T_gt; it stays inside the radius).
    The least-squares minimum is shifted by about share x offset; the true pose is still the minimum of a redescending kernel."""
    c = dict(case)
    J = len(c["src"])
    sel = np.random.default_rng(1000 + seed).permutation(J)[:int(round(share * J))]
    R = c["T_gt"][:, :3]
    src = c["src"].astype(np.float64).copy()
    src[sel] = src[sel] + np.asarray(offset, np.float64) @ R          # R^T offset, as a row vector
    c["src"] = src.astype(np.float32)
    c["outliers"] = sel
    return c
