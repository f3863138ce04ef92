"""Synthetic registration pairs.

``ref``: N points uniform in an extent box; random SO(3) rotation R (QR of a
Gaussian matrix, det fixed to +1) and translation t ~ U(-0.5, 0.5)^3;
``src = (ref - t) @ R`` (so ``R @ src_i + t = ref_i``), then row-permuted so
that the prefix sub-sampling of the KNN pyramid (reference
dataloader/data_base.py:166-168) is a random sub-sample, as the reference's
``Resampler`` guarantees for 3DMatch (dataloader/transformation.py:72-80).
Extra feature channels (reflectance for KITTI-shaped input) are U(0,1).
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

EXTENTS = {
    "3dmatch": ((0.0, 3.0), (0.0, 3.0), (0.0, 3.0)),
    "kitti": ((-50.0, 50.0), (-50.0, 50.0), (-3.0, 3.0)),
}


def random_rotation(rng: np.random.Generator) -> np.ndarray:
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))[None, :]
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def _uniform_cloud(rng, n, extent):
    lo = np.array([e[0] for e in extent])
    hi = np.array([e[1] for e in extent])
    return rng.uniform(0.0, 1.0, (n, 3)) * (hi - lo) + lo


def make_pair(n: int, seed: int, feat_len: int = 3, shape: str = "3dmatch",
              partial_overlap: bool = False) -> Dict[str, np.ndarray]:
    """One pair as the reference's collate would hand it over, batch dim = 1
    (reference dataloader/data_base.py:196-209): ``points_src/ref [1,N,feat_len]``
    fp32 and ``transform_gt [1,3,4]``."""
    rng = np.random.Generator(np.random.Philox(key=int(seed) + 0xC10D))
    extent = EXTENTS[shape]
    R = random_rotation(rng)
    t = rng.uniform(-0.5, 0.5, 3)
    if not partial_overlap:
        ref = _uniform_cloud(rng, n, extent)
        src = (ref - t) @ R
    else:
        # C5: two half-space crops keeping ~75 % each (=> ~50 % mutual overlap),
        # as RandomCrop (reference dataloader/transformation.py:134-145), plus
        # N(0,0.01) jitter clipped at 0.05 (:99-107), then resampled to n.
        base = _uniform_cloud(rng, 2 * n, extent)
        c = base.mean(0)

        def crop(p, keep=0.75):
            d = rng.standard_normal(3)
            d /= np.linalg.norm(d)
            proj = (p - c) @ d
            return p[proj > np.quantile(proj, 1.0 - keep)]

        def jitter(p):
            return p + np.clip(rng.standard_normal(p.shape) * 0.01, -0.05, 0.05)

        def resample(p):
            idx = rng.choice(len(p), n, replace=len(p) < n)
            return p[idx]

        ref = resample(jitter(crop(base)))
        src = resample(jitter((crop(base) - t) @ R))
    src = src[rng.permutation(n)]
    ref = ref[rng.permutation(n)]
    extra_s = rng.uniform(0.0, 1.0, (n, max(feat_len - 3, 0)))
    extra_r = rng.uniform(0.0, 1.0, (n, max(feat_len - 3, 0)))
    T = np.concatenate([R, t[:, None]], axis=1)
    return {
        "points_src": np.concatenate([src, extra_s], 1)[None].astype(np.float32),
        "points_ref": np.concatenate([ref, extra_r], 1)[None].astype(np.float32),
        "transform_gt": T[None].astype(np.float32),
    }


def make_batch(n: int, seeds, feat_len: int = 3, shape: str = "3dmatch",
               partial_overlap: bool = False) -> Dict[str, np.ndarray]:
    """Stack several pairs along the batch dimension."""
    pairs = [make_pair(n, s, feat_len, shape, partial_overlap) for s in seeds]
    return {k: np.concatenate([p[k] for p in pairs], 0) for k in pairs[0]}


# ---------------------------------------------------------------------------------------------------------------------- pose graphs
POSE_GRAPH_RADIUS = 0.05          # max_corr_dist the synthetic information matrices and mu of make_pose_graph stand for


def _pg():
    from . import pose_graph
    return pose_graph


def _rot(axis, angle):
    ax = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def se3_random(rng, angle, shift):
    return np.hstack([_rot(rng.standard_normal(3), angle * rng.uniform(0.5, 1.0)), rng.uniform(-shift, shift, (3, 1))])


def se3_mul(A, B):
    return np.hstack([A[:, :3] @ B[:, :3], (A[:, :3] @ B[:, 3] + A[:, 3])[:, None]])


def se3_inv(A):
    return np.hstack([A[:, :3].T, (-A[:, :3].T @ A[:, 3])[:, None]])


def make_pose_graph(N, seed, loops=4, noise=(0.0, 0.0), start=(0.1, 0.1), false_edges=0, ref=0, points=200):
    """A ring of N random poses: certain edges (i, i+1), `loops` uncertain true loop closures, `false_edges` uncertain edges with an
    unrelated transform (listed last).  noise = (radians, metres) on every true edge's T; start = the same on X0 around the truth.
    Information matrices: information_matrix_host of `points` random points of a 3 m room.  -> (PoseGraph, X_true, is_false [E])"""
    rng = np.random.default_rng(seed)
    Xt = np.stack([se3_random(rng, 2.0, 2.0) for _ in range(N)])
    st = [(i, i + 1) for i in range(N - 1)]
    for _ in range(loops if N > 2 else 0):
        s, t = sorted(rng.choice(N, 2, replace=False))
        st.append((int(s), int(t)))
    nt = len(st)
    for _ in range(false_edges):
        s, t = sorted(rng.choice(N, 2, replace=False))
        st.append((int(s), int(t)))
    T, info = [], []
    for k, (s, t) in enumerate(st):
        Tk = se3_mul(se3_inv(Xt[t]), Xt[s])                                      # X_s = X_t T
        Tk = se3_mul(se3_random(rng, noise[0], noise[1]), Tk) if k < nt else se3_random(rng, 3.0, 1.5)
        T.append(Tk)
        q = rng.uniform(0, 3, (points, 3)).astype(np.float32)
        info.append(_pg().information_matrix_host(q, np.arange(points)))
    unc = np.array([0] * (N - 1) + [1] * (len(st) - (N - 1)), np.uint8)
    X0 = np.stack([Xt[i] if i == ref else se3_mul(se3_random(rng, *start), Xt[i]) for i in range(N)])
    g = _pg().PoseGraph(X0, np.array(st, np.int32).reshape(-1, 2), np.array(T).reshape(-1, 3, 4), np.array(info).reshape(-1, 6, 6), unc,
                     mu=_pg().line_process_weight(info, unc, POSE_GRAPH_RADIUS), reference_node=ref)
    return g, Xt, np.arange(len(st)) >= nt
