"""Host restatement of the point-to-plane ICP rule of csrc/icp.hip (TEST INFRASTRUCTURE ONLY).

open3d's ``registration_icp`` with ``TransformationEstimationPointToPlane``: open3d is not installable here, so **parity is
unpinned** and the rule is the engine's own (header of csrc/icp.hip, include/dsir.h ``dsir_icp_refine_ex``); this file is what
the HIP path is held to.  The loop is ``oracle.icp.icp``'s - first search, fitness, inlier RMSE from point distances, the
convergence test, ``max_iter`` - and only the update differs.  float64 throughout except the correspondence distance, which is
``oracle.icp._nearest``'s fp32 expression so both sides pick the same neighbours.

The update, over the correspondences (s = moved source point, t = target point, n = target normal):
    r = (s - t) . n,   J = [s x n ; n],   A = sum J J^T,   b = sum J r,   A x = -b,
    R = Rz(x2) Ry(x1) Rx(x0),  t = (x3, x4, x5)                      (open3d's TransformVector6dToMatrix4d)
Corner cases:
    singular system   fewer than 6 contributing correspondences, or a singular system: the update is the identity and is
                      counted.  Singular = LDL^T without pivoting of A scaled to unit diagonal meets a pivot below
                      ``PIVOT_MIN``; a diagonal entry that is zero (or not a positive finite number) is singular.
    zero normal       (``estimate_normals``' degenerate output) the correspondence contributes nothing.
    non-finite        a non-finite normal or target coordinate takes that correspondence out of the update; a non-finite moved
                      source point makes every update of the pair the identity (counted), so T stays a finite rigid transform.
"""
from __future__ import annotations

import numpy as np

from oracle.icp import _nearest

# A pivot of the unit-diagonal matrix is 1 - (squared multiple correlation of a parameter with the ones before it): in [0, 1]
# whatever the cloud's units, and never below the smallest eigenvalue, so a scaled condition number under 1e10 is never refused
# (surfaces measure 1e2..1e3); the fp64 sums carry about rows x 2^-53 (1e-11 at 1e5 rows), a pivot under 1e-10 is within ten
# times that noise.  The same constant as csrc/icp_plane.h kIcpPlanePivotMin.
PIVOT_MIN = 1e-10

IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))])


def normal_sums(s, t, n):
    """(A [6,6], b [6], rows) over the correspondences that contribute: finite t and n, n != 0."""
    s, t, n = (np.asarray(a, np.float64).reshape(-1, 3) for a in (s, t, n))
    use = np.isfinite(t).all(1) & np.isfinite(n).all(1) & (n != 0).any(1)
    s, t, n = s[use], t[use], n[use]
    d = s - t
    r = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    J = np.concatenate([np.cross(s, n), n], 1)
    return J.T @ J, J.T @ r, int(use.sum())


def solve(A, b, rows):
    """x of A x = -b, or None where the rule calls the system singular."""
    if rows < 6:
        return None
    d = np.diag(A).astype(np.float64)
    if not (np.isfinite(d).all() and (d > 0).all()):
        return None
    s = 1.0 / np.sqrt(d)
    M = A * s[:, None] * s[None, :]
    L, D = np.eye(6), np.zeros(6)
    for j in range(6):
        D[j] = 1.0 - sum(L[j, k] * L[j, k] * D[k] for k in range(j))
        if not D[j] >= PIVOT_MIN:
            return None
        for i in range(j + 1, 6):
            L[i, j] = (M[j, i] - sum(L[i, k] * L[j, k] * D[k] for k in range(j))) / D[j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = -b[i] * s[i] - sum(L[i, k] * y[k] for k in range(i))
    y /= D
    for i in range(5, -1, -1):
        y[i] -= sum(L[k, i] * y[k] for k in range(i + 1, 6))
    x = y * s
    return x if np.isfinite(x).all() else None


def vec6_to_T(x):
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    return np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa, x[3]],
                     [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa, x[4]],
                     [-sb, cb * sa, cb * ca, x[5]]])


def plane_update(cur, tgt, normals, idx, ok):
    """One update from the moved points ``cur`` [J,3] and their correspondences -> ([3,4] float64, singular: bool)."""
    if not np.isfinite(cur).all():
        return IDENTITY.copy(), True
    A, b, rows = normal_sums(cur[ok], tgt[idx[ok]], normals[idx[ok]])
    x = solve(A, b, rows)
    if x is None:
        return IDENTITY.copy(), True
    return vec6_to_T(x), False


def icp_plane(src, tgt, normals, T_init, max_corr_dist, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, perturb_ulps=None,
              trace=None):
    """src [J,>=3], tgt [K,>=3] fp32, normals [K,3], T_init [3,4] ->
    (T [3,4] float64, fitness, inlier_rmse, converged, iterations, identity updates taken for a singular system).
    ``perturb_ulps`` / ``trace``: the hooks of ``oracle.icp.icp`` (every coordinate of the moved points shifted by -1, 0 or +1
    fp32 ulp at random after each update; (fitness, rmse) of the first search and of every iteration)."""
    src32, tgt32 = np.ascontiguousarray(src[:, :3], np.float32), np.ascontiguousarray(tgt[:, :3], np.float32)
    nrm = np.asarray(normals, np.float32)[:, :3].astype(np.float64)
    # a target point with a non-finite coordinate is never a correspondence (the engine's `d < best` is false for NaN and inf):
    # for the search alone it is moved out of every radius, so that numpy's argmin does not stop at its NaN
    search32 = np.where(np.isfinite(tgt32).all(1, keepdims=True), tgt32, np.float32(3e18))
    r2 = np.float32(max_corr_dist) * np.float32(max_corr_dist)
    T = np.asarray(T_init, np.float64).copy()
    cur = (src32 @ T[:, :3].astype(np.float32).T + T[:, 3].astype(np.float32)).astype(np.float32)
    rng = None if perturb_ulps is None else np.random.default_rng(perturb_ulps)

    def evaluate(c):
        with np.errstate(invalid="ignore", over="ignore"):
            idx, d2 = _nearest(c, search32)
            ok = d2 <= r2                                    # a NaN / inf distance is never a correspondence
        n = int(ok.sum())
        return idx, ok, n / len(c), (float(np.sqrt(d2[ok].astype(np.float64).sum() / n)) if n else 0.0)

    idx, ok, fitness, rmse = evaluate(cur)
    if trace is not None:
        trace.append((fitness, rmse))
    converged, iters, singular = False, 0, 0
    for _ in range(max_iter):
        upd, sing = plane_update(cur.astype(np.float64), tgt32.astype(np.float64), nrm, idx, ok)
        singular += int(sing)
        if not sing:
            T = np.hstack([upd[:, :3] @ T[:, :3], (upd[:, :3] @ T[:, 3] + upd[:, 3])[:, None]])
            cur = (cur.astype(np.float64) @ upd[:, :3].T + upd[:, 3]).astype(np.float32)
            if rng is not None:
                step = rng.integers(-1, 2, cur.shape)
                cur = np.where(step > 0, np.nextafter(cur, np.float32(np.inf)),
                               np.where(step < 0, np.nextafter(cur, np.float32(-np.inf)), cur)).astype(np.float32)
        idx, ok, f2, e2 = evaluate(cur)
        if trace is not None:
            trace.append((f2, e2))
        iters += 1
        done = abs(fitness - f2) < rel_fitness and abs(rmse - e2) < rel_rmse
        fitness, rmse = f2, e2
        if done:
            converged = True
            break
    return T, fitness, rmse, converged, iters, singular
