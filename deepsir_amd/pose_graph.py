"""Scene-level registration on the host: the numpy float64 restatement of ``dsir_information_matrix`` (csrc/info_matrix.hip) and
of ``dsir_pose_graph_optimize`` (csrc/pose_graph.hip), the default line-process weight, and the checks and CSR packing that
``Engine.pose_graph_optimize`` runs before a launch.  open3d is absent: the rules are the engine's own, stated in those two headers.

Conventions: node pose ``X_i`` [3,4] maps fragment i's frame to the scene frame; an edge ``(s, t, T, info, uncertain)`` says
``p_t = T p_s``, so a consistent graph has ``X_s = X_t T``; ``info`` is 6 x 6 in the order [rotation; translation]."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Sequence

import numpy as np

MAX_NODES = 128                       # DSIR_POSE_GRAPH_MAX_NODES
MAX_ITER = 100                        # DSIR_POSE_GRAPH_MAX_ITER
ST_MAX_ITER, ST_LAMBDA, ST_PIVOT, ST_NON_FINITE, ST_EDGE_INDEX = 1, 2, 4, 8, 16    # DSIR_PG_*
LAMBDA0, LAMBDA_MAX, STOP_REL = 1e-3, 1e12, 1e-6
PRUNE_LINE = 0.25                     # an uncertain edge whose final l is below this is a rejected loop closure


@dataclass
class PoseGraph:
    """One graph: X0 [N,3,4], edges as parallel arrays (st [E,2] graph-local (s, t), T [E,3,4], info [E,6,6], uncertain [E])."""
    X0: np.ndarray
    st: np.ndarray
    T: np.ndarray
    info: np.ndarray
    uncertain: np.ndarray
    mu: float = 1.0
    reference_node: int = 0

    @staticmethod
    def of(g) -> "PoseGraph":
        if isinstance(g, PoseGraph):
            return g
        return PoseGraph(g["X0"], g["st"], g["T"], g["info"], g["uncertain"], g.get("mu", 1.0), g.get("reference_node", 0))

    def arrays(self):
        X0 = np.ascontiguousarray(self.X0, np.float64).reshape(-1, 3, 4)
        st = np.ascontiguousarray(self.st, np.int32).reshape(-1, 2)
        E = len(st)
        return (X0, st, np.ascontiguousarray(self.T, np.float64).reshape(E, 3, 4), np.ascontiguousarray(self.info, np.float64).reshape(E, 6, 6),
                np.ascontiguousarray(self.uncertain).astype(np.uint8).reshape(E))


# ---------------------------------------------------------------------------------------------------------------------- information
def information_matrix_host(ref: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """ref [K,>=3] fp32, idx [J] (the search's output, -1: none) -> info [6,6] float64 by the ten sums of csrc/info_matrix.hip."""
    idx = np.asarray(idx)
    q = np.asarray(ref)[idx[idx >= 0], :3].astype(np.float32).astype(np.float64)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    n, sx, sy, sz = float(len(q)), x.sum(), y.sum(), z.sum()
    sxx, syy, szz, sxy, sxz, syz = (x * x).sum(), (y * y).sum(), (z * z).sum(), (x * y).sum(), (x * z).sum(), (y * z).sum()
    A = np.zeros((6, 6))
    A[0, 0], A[1, 1], A[2, 2] = syy + szz, sxx + szz, sxx + syy
    A[0, 1], A[0, 2], A[1, 2] = -sxy, -sxz, -syz
    A[0, 4], A[0, 5], A[1, 3], A[1, 5], A[2, 3], A[2, 4] = -sz, sy, sz, -sx, -sy, sx
    A[3, 3] = A[4, 4] = A[5, 5] = n
    A = np.triu(A) + np.triu(A, 1).T
    return A + 0.0                    # no negative zero


def line_process_weight(edge_info, uncertain, max_corr_dist: float, preference: float = 1.0) -> float:
    """The default mu: preference x max_corr_dist^2 x mean over the uncertain edges of info[3,3] (the correspondences of the edge).
    An uncertain edge whose residual costs as much as all its correspondences lying max_corr_dist off gets l = 1/4 at
    preference = 1.  Without an uncertain edge mu is not read: 1."""
    info = np.asarray(edge_info, np.float64).reshape(-1, 6, 6)
    u = np.asarray(uncertain).astype(bool).reshape(-1)
    if not u.any():
        return 1.0
    return float(preference) * float(max_corr_dist) ** 2 * float(info[u, 3, 3].mean())


# ---------------------------------------------------------------------------------------------------------------------- the rule
def _log3(R):
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = np.sqrt(w @ w), 0.5 * (np.trace(R) - 1.0)
    return w * (np.arctan2(s, c) / s) if s >= 1e-12 else w


def _exp3(w):
    t2 = float(w @ w)
    t = np.sqrt(t2)
    a, b = (np.sin(t) / t, (1.0 - np.cos(t)) / t2) if t >= 1e-8 else (1.0, 0.5)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + a * K + b * (K @ K)


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def _edge(Xs, Xt, T):
    """-> (e [6], Js [6,6])"""
    RA = T[:, :3].T @ Xt[:, :3].T
    tA = -T[:, :3].T @ (Xt[:, :3].T @ Xt[:, 3] + T[:, 3])
    e = np.concatenate([_log3(RA @ Xs[:, :3]), RA @ Xs[:, 3] + tA])
    Js = np.zeros((6, 6))
    Js[:3, :3] = RA
    Js[3:, :3] = -RA @ _skew(Xs[:, 3])
    Js[3:, 3:] = RA
    return e, Js


def _terms(chi, l, unc, mu):
    return l * chi + np.where(unc, mu * (np.sqrt(l) - 1.0) ** 2, 0.0)


def _line(chi, unc, mu):
    return np.where(unc, (mu / (mu + chi)) ** 2, 1.0)


def optimize_host(graph, max_iter: int = MAX_ITER, trace: list = None):
    """dsir_pose_graph_optimize for one graph in numpy float64 -> (X [N,3,4], line [E], stats [4]): same objective, same damping
    rule, same stops (header of csrc/pose_graph.hip).  ``trace``: a list that receives F after every accepted step."""
    g = PoseGraph.of(graph)
    X0, st, T, info, unc8 = g.arrays()
    unc = unc8.astype(bool)
    N, E, ref, mu = len(X0), len(st), int(g.reference_node), float(g.mu)
    n = 6 * (N - 1)
    status = 0
    if not (np.isfinite(X0).all() and np.isfinite(T).all() and np.isfinite(info).all() and (E == 0 or (np.isfinite(mu) and mu > 0))):
        status |= ST_NON_FINITE
    if E and ((st < 0).any() or (st >= N).any() or (st[:, 0] == st[:, 1]).any()):
        status |= ST_EDGE_INDEX
    if status or n == 0 or E == 0:
        return X0.copy(), np.ones(E), np.array([0.0, 0.0, 0.0, float(status)])

    def evaluate(X):
        out = [_edge(X[s], X[t], T[k]) for k, (s, t) in enumerate(st)]
        e = np.stack([o[0] for o in out])
        return e, [o[1] for o in out], np.einsum("ka,kab,kb->k", e, info, e)

    def col(i):
        return -1 if i == ref else 6 * (i if i < ref else i - 1)

    def total(terms):
        F = 0.0
        for v in terms:                       # edge order, as the device adds them
            F += v
        return F

    X = X0.copy()
    e, Js, chi = evaluate(X)
    l = _line(chi, unc, mu)
    F = F0 = total(_terms(chi, l, unc, mu))
    if not np.isfinite(F):
        return X0.copy(), np.ones(E), np.array([F0, F0, 0.0, float(ST_NON_FINITE)])
    lam, nu, it, assemble = LAMBDA0, 2.0, 0, True
    while True:
        if it >= max_iter:
            status |= ST_MAX_ITER
            break
        if assemble:
            H, b = np.zeros((n, n)), np.zeros(n)
            for k, (s, t) in enumerate(st):
                JL = Js[k].T @ (l[k] * info[k])
                W, gk = JL @ Js[k], JL @ e[k]
                cs, ct = col(s), col(t)
                if cs >= 0:
                    H[cs:cs + 6, cs:cs + 6] += W
                    b[cs:cs + 6] += gk
                if ct >= 0:
                    H[ct:ct + 6, ct:ct + 6] += W
                    b[ct:ct + 6] -= gk
                if cs >= 0 and ct >= 0:
                    H[cs:cs + 6, ct:ct + 6] -= W
                    H[ct:ct + 6, cs:cs + 6] -= W
            D = np.diag(H).copy()
        A = np.tril(H) + np.tril(H, -1).T + np.diag(lam * D)        # the device reads the lower triangle
        fail = 0
        with np.errstate(all="ignore"):
            try:
                Lc = np.linalg.cholesky(A)
            except np.linalg.LinAlgError:
                fail = ST_PIVOT if np.isfinite(A).all() else ST_NON_FINITE
            if not fail and not np.isfinite(Lc).all():
                fail = ST_NON_FINITE
        if fail:
            return X0.copy(), np.ones(E), np.array([F0, F0, float(it), float(status | fail)])
        d = np.linalg.solve(Lc.T, np.linalg.solve(Lc, -b))
        it += 1
        free = [i for i in range(N) if i != ref]
        if not np.isfinite(d).all():
            return X0.copy(), np.ones(E), np.array([F0, F0, float(it), float(status | ST_NON_FINITE)])
        if np.sqrt(d @ d) <= STOP_REL * np.sqrt(sum(float(X[i, :, 3] @ X[i, :, 3]) + 1.0 for i in free)):
            break
        Xt = X.copy()
        for i in free:
            di = d[col(i):col(i) + 6]
            R = _exp3(di[:3])
            Xt[i, :, :3] = R @ X[i, :, :3]
            Xt[i, :, 3] = R @ X[i, :, 3] + di[3:]
        e_t, Js_t, chi_t = evaluate(Xt)
        Fn = total(_terms(chi_t, l, unc, mu))
        pred = float(d @ (lam * D * d - b))
        if Fn < F and pred > 0.0:
            rho = (F - Fn) / pred
            X, e, Js, chi = Xt, e_t, Js_t, chi_t
            l = _line(chi, unc, mu)
            Fa = total(_terms(chi, l, unc, mu))
            lam *= max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3)
            nu = 2.0
            stop = F - Fa <= STOP_REL * F
            F = Fa
            if trace is not None:
                trace.append(F)
            assemble = True
            if stop:
                break
        else:
            lam *= nu
            nu *= 2.0
            assemble = False
            if not lam <= LAMBDA_MAX:
                status |= ST_LAMBDA
                break
    return X, l, np.array([F0, F, float(it), float(status)])


# ---------------------------------------------------------------------------------------------------------------------- packing
def check_graph(g: PoseGraph, which: int = 0):
    """The host refusals (ValueError): no node, more than MAX_NODES nodes, a reference node outside the graph, several nodes without
    an edge, edges that do not connect the graph (edges with an index outside the graph are left to the device's status bit)."""
    X0, st, _, _, _ = g.arrays()
    N, E = len(X0), len(st)
    if N < 1:
        raise ValueError(f"pose graph {which}: no node")
    if N > MAX_NODES:
        raise ValueError(f"pose graph {which}: {N} nodes, more than DSIR_POSE_GRAPH_MAX_NODES = {MAX_NODES}")
    if not 0 <= int(g.reference_node) < N:
        raise ValueError(f"pose graph {which}: reference_node {g.reference_node} is not one of its {N} nodes")
    if N > 1 and E == 0:
        raise ValueError(f"pose graph {which}: {N} nodes and no edge (disconnected)")
    root = list(range(N))

    def find(i):
        while root[i] != i:
            root[i] = root[root[i]]
            i = root[i]
        return i

    for s, t in st:
        if 0 <= s < N and 0 <= t < N:
            root[find(int(s))] = find(int(t))
    if len({find(i) for i in range(N)}) != 1:
        raise ValueError(f"pose graph {which}: its edges do not connect it (disconnected)")


def pack_graphs(graphs: Sequence) -> dict:
    """Check every graph and concatenate them CSR-style: the host arrays ``dsir_pose_graph_optimize`` takes."""
    gs: List[PoseGraph] = [PoseGraph.of(g) for g in graphs]
    if not gs:
        raise ValueError("pose_graph_optimize: no graph")
    for k, g in enumerate(gs):
        check_graph(g, k)
    arr = [g.arrays() for g in gs]
    cat = lambda k, shape, dt: (np.concatenate([a[k] for a in arr], 0) if sum(len(a[k]) for a in arr) else np.zeros(shape, dt))
    return {
        "node_off": np.cumsum([0] + [len(a[0]) for a in arr]).astype(np.int32),
        "edge_off": np.cumsum([0] + [len(a[1]) for a in arr]).astype(np.int32),
        "X0": cat(0, (0, 3, 4), np.float64), "st": cat(1, (0, 2), np.int32), "T": cat(2, (0, 3, 4), np.float64),
        "info": cat(3, (0, 6, 6), np.float64), "uncertain": cat(4, (0,), np.uint8),
        "mu": np.array([float(g.mu) for g in gs], np.float64),
        "reference_node": np.array([int(g.reference_node) for g in gs], np.int32),
    }
