"""Host restatement (numpy) of the two rules csrc/ppf.hip owns: the point-pair-feature input layer of ``use_ppf`` (reference
network/RandLANet.py:110-137, :324-332; network/matchnet.py:11-30) in the kernel's written arithmetic, and the normal
estimation (open3d's ``estimate_normals`` is unpinned: the rule is the engine's own).  What the tests compare the kernels with,
as ``deepsir_amd/ransac.py`` and ``augment.py`` are for theirs.  Nothing here runs on the hot path.

Front end, all fp32, every operation rounded once (numpy's float32 arithmetic does that), j = neigh[i, k]:
    d = p_j - p_i;  cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0);  dot(a, b) = ((+0 + a0 b0) + a1 b1) + a2 b2
    (the sum starts from +0 as torch.sum's does: products of a zero vector with negative numbers are -0, and atan2(0, -0) is pi)
    norm(a) = sqrt((a0 a0 + a1 a1) + a2 a2);  angle(a, b) = atan2(norm(cross(a, b)), dot(a, b))     (atan2(0, 0) = 0)
    x = [p_i, d, angle(n_i, d), angle(n_j, d), angle(n_i, n_j), norm(d)]
    y[c] = fma chain over the input channels in ascending order, starting from the bias
    GroupNorm(4 groups of 3 channels, statistics over the cloud's n x 16 rows, fp64 sums, scale / shift rounded to fp32, applied
    as one fma), LeakyReLU(0.2), mean over k as a butterfly (partners 1, 2, 4, 8) times 1/16.
The fma is restated as round32(float64(w) * float64(x) + float64(acc)): the product is exact in fp64, the sum is rounded twice -
to fp64, then to fp32 - where the kernel rounds once; the two differ by one fp32 ulp in about one sum in 2^29.  atan2 is the host
library's, the device's atan2f is its own (both within a few ulp): the comparison is a tolerance, not bits.

Training: ``ppf_pre_backward`` restates the backward of the front end's four parameter tensors (dsir_t_ppf_bwd) - fp32 element-wise
as the kernel writes it, every sum in fp64; what the GPU tests compare against where no golden exists.

Normals, one point at a time: the 16 level-0 neighbours in list order (self included); mean and covariance as fp64 sums of the
fp32 coordinates in that order; the eigenvector of the smallest eigenvalue (``numpy.linalg.eigh`` here, the Jacobi SVD of svd3.h
on the device); normalised in fp64; flipped so that n . (v - p) >= 0 for the viewpoint v (at exactly 0: the component of largest
magnitude positive, ties to the lower axis); rounded to fp32 once.  Largest eigenvalue 0 or anything non-finite: normal (0,0,0),
flag 1.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

F = np.float32


def _norm3(a: np.ndarray) -> np.ndarray:
    return np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])


def angle(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """matchnet.py:11-30 in the kernel's written order; a, b float32 [..., 3]."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    c = np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                  a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                  a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
    dot = ((F(0.0) + a[..., 0] * b[..., 0]) + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]    # from +0: never -0 (atan2(0, -0) = pi)
    return np.arctan2(_norm3(c), dot).astype(F)


def feat_grouping(xyz: np.ndarray, normals: np.ndarray, neigh: np.ndarray) -> np.ndarray:
    """RandLANet.py:110-137: xyz, normals [B, N, 3], neigh [B, N, 16] -> the ten channels [B, N, 16, 10] (float32)."""
    xyz, normals = np.asarray(xyz, F), np.asarray(normals, F)
    B = xyz.shape[0]
    bi = np.arange(B)[:, None, None]
    pj, nj = xyz[bi, neigh], normals[bi, neigh]                    # [B, N, 16, 3]
    pi = np.broadcast_to(xyz[:, :, None, :], pj.shape)
    ni = np.broadcast_to(normals[:, :, None, :], pj.shape)
    d = pj - pi
    return np.concatenate([pi, d, angle(ni, d)[..., None], angle(nj, d)[..., None], angle(ni, nj)[..., None], _norm3(d)[..., None]],
                          -1).astype(F)


def _fma(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def _pre_rows(rows, neigh, W, b, gamma, beta):
    """What the forward and the backward rebuild of every (point, neighbour) row: x [B, N, 16, 10], the raw conv outputs y
    [B, N, 16, 12], the fp32 scale / shift [B, 12] the layer applies and the groups' fp64 mean / rstd [B, 4]."""
    rows = np.asarray(rows, F)
    neigh = np.clip(np.asarray(neigh), 0, rows.shape[1] - 1)           # the kernel's clamp: a bad neighbour index never leaves the cloud
    x = feat_grouping(rows[..., :3], rows[..., 3:6], neigh)            # [B, N, 16, 10]
    W = np.asarray(W, F).reshape(12, 10)
    y = np.broadcast_to(np.asarray(b, F), x.shape[:-1] + (12,)).copy()
    for q in range(10):
        y = _fma(np.broadcast_to(W[:, q], y.shape), np.broadcast_to(x[..., q:q + 1], y.shape), y)
    B, N = y.shape[:2]
    g = y.reshape(B, N * 16, 4, 3)
    s1 = g.astype(np.float64).sum((1, 3))                              # [B, 4]
    s2 = (g * g).astype(np.float64).sum((1, 3))                        # the square is an fp32 product
    inv = 1.0 / (3.0 * N * 16.0)
    mean = s1 * inv
    var = np.maximum(s2 * inv - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + 1e-5)
    sc = np.asarray(gamma, np.float64)[None, :] * np.repeat(rstd, 3, 1)                # [B, 12]
    sh = np.asarray(beta, np.float64)[None, :] - np.repeat(mean, 3, 1) * sc
    return x, y, sc.astype(F), sh.astype(F), mean, rstd


def ppf_pre(rows: np.ndarray, neigh: np.ndarray, W: np.ndarray, b: np.ndarray, gamma: np.ndarray, beta: np.ndarray) -> np.ndarray:
    """The whole front end (RandLANet.py:324-332): rows [B, N, >= 6] = xyz + normal, neigh [B, N, 16] (level 0), mlp_pre's
    conv weight [12, 10(,1,1)], bias, GroupNorm weight, bias -> [B, N, 12], the input of level 0 (point-major)."""
    _, y, sc, sh, _, _ = _pre_rows(rows, neigh, W, b, gamma, beta)
    z = _fma(y, np.broadcast_to(sc[:, None, None, :], y.shape), np.broadcast_to(sh[:, None, None, :], y.shape))
    z = np.where(z < 0, F(0.2) * z, z).astype(F)
    k = np.arange(16)
    for o in (1, 2, 4, 8):
        z = z + z[:, :, k ^ o, :]
    return (z[:, :, 0, :] * F(0.0625)).astype(F)


def ppf_pre_backward(rows: np.ndarray, neigh: np.ndarray, W: np.ndarray, b: np.ndarray, gamma: np.ndarray, beta: np.ndarray,
                     dout: np.ndarray, per_cloud: bool = False):
    """The backward of ``ppf_pre`` w.r.t. its four parameter tensors (the rows are data), the rule of csrc/ppf.hip's training
    paragraph: dout [B, N, 12] = d loss / d output -> (dW [12, 10], db, dgamma, dbeta [12]) as float64.  Element-wise steps in fp32
    as the kernel writes them, every sum in fp64 (the kernel: fp64 per lane and across workgroups; fp32 inside pass B's MFMA tile).
        z  = fma(y, scale, shift) from the forward's fp32 scale / shift;  g = dout / 16 * (z < 0 ? 0.2 : 1);  yh = (y - mean) rstd
        pass A, per cloud:  dbeta_c = sum g,  dgamma_c = sum g yh;  per group  S1 = sum_c gamma_c dbeta_c,  S2 = sum_c gamma_c dgamma_c
        pass B:             dy = rstd (g gamma_c - S1 / m - yh S2 / m),  m = 3 N 16;  dW[c][q] = sum dy x[q],  db[c] = sum dy
    per_cloud: also return every cloud's own (dbeta, dgamma) [B, 12] each - what the parameter gradients add up in cloud order."""
    x, y, sc, sh, mean, rstd = _pre_rows(rows, neigh, W, b, gamma, beta)
    B, N = y.shape[:2]
    gamma32 = np.asarray(gamma, F)
    z = _fma(y, np.broadcast_to(sc[:, None, None, :], y.shape), np.broadcast_to(sh[:, None, None, :], y.shape))
    gd = (np.asarray(dout, F) * F(0.0625))[:, :, None, :]
    g = np.where(z < 0, F(0.2) * gd, gd).astype(F)                                    # [B, N, 16, 12]
    mean32 = np.repeat(mean.astype(F), 3, 1)[:, None, None, :]
    rstd32 = np.repeat(rstd.astype(F), 3, 1)[:, None, None, :]
    yh = ((y - mean32) * rstd32).astype(F)
    dbeta_c = g.astype(np.float64).sum((1, 2))                                        # [B, 12]
    dgamma_c = (g.astype(np.float64) * yh.astype(np.float64)).sum((1, 2))
    m = 3.0 * N * 16.0
    S1 = (gamma32.astype(np.float64)[None] * dbeta_c).reshape(B, 4, 3).sum(2) / m     # [B, 4]
    S2 = (gamma32.astype(np.float64)[None] * dgamma_c).reshape(B, 4, 3).sum(2) / m
    gm1 = np.repeat(S1.astype(F), 3, 1)[:, None, None, :]
    gm2 = np.repeat(S2.astype(F), 3, 1)[:, None, None, :]
    dy = (rstd32 * (((g * gamma32) - gm1) - yh * gm2)).astype(F)
    dW = np.einsum("bnkc,bnkq->cq", dy.astype(np.float64), x.astype(np.float64))
    db = dy.astype(np.float64).sum((0, 1, 2))
    out = (dW, db, dgamma_c.sum(0), dbeta_c.sum(0))
    return out + (dbeta_c, dgamma_c) if per_cloud else out


def _normals_of(pts, q, cnt, v):
    """pts [N, 3] float64, q [N, K, 3] float64 = the lists' points (entries at or past cnt [N] are ignored), v [3] -> (normals, flags)."""
    N, K = q.shape[:2]
    live = np.arange(K)[None, :] < cnt[:, None]
    m = np.zeros((N, 3))
    for k in range(K):
        m = np.where(live[:, k, None], m + q[:, k], m)
    with np.errstate(all="ignore"):
        m = m / cnt[:, None].astype(np.float64)
    C = np.zeros((N, 3, 3))
    for k in range(K):
        e = q[:, k] - m
        C = np.where(live[:, k, None, None], C + e[:, :, None] * e[:, None, :], C)
    ok = np.isfinite(C).all((1, 2)) & (cnt >= 3)
    w, V = np.linalg.eigh(np.where(ok[:, None, None], C, 0.0))         # ascending eigenvalues
    nv = V[:, :, 0]
    nv = nv / np.sqrt((nv * nv).sum(1, keepdims=True))
    t = (nv * (v[None] - pts)).sum(1)
    mx = np.argmax(np.abs(nv), 1)                                      # first maximum = the lower axis
    flip = np.where(t == 0.0, nv[np.arange(N), mx] < 0.0, t < 0.0)
    nv = np.where(flip[:, None], -nv, nv)
    good = ok & (w[:, 2] > 0.0) & np.isfinite(t)
    return np.where(good[:, None], nv, 0.0).astype(F), np.where(good, 0, 1).astype(np.int32)


def estimate_normals(points: np.ndarray, neigh: Optional[np.ndarray] = None, viewpoint=(0.0, 0.0, 0.0), csr=None) -> Tuple[np.ndarray, np.ndarray]:
    """points [B, N, >= 3] float32 and exactly one of neigh [B, N, 16] (level 0) and csr = (offsets [B N + 1], cols, cloud-local: the
    entries of a row in row order; fewer than 3: flag 1, normal 0) -> (normals [B, N, 3] float32, flags [B, N] int32)."""
    if (neigh is None) == (csr is None):
        raise ValueError("estimate_normals: exactly one of neigh and csr expected")
    pts = np.asarray(points, F)[..., :3].astype(np.float64)
    v = np.asarray(viewpoint, F).astype(np.float64)
    B, N = pts.shape[:2]
    out = np.zeros((B, N, 3), F)
    flags = np.ones((B, N), np.int32)
    for bi in range(B):
        if neigh is not None:
            lists, cnt = np.asarray(neigh[bi]), np.full(N, 16, np.int64)
        else:
            off = np.asarray(csr[0], np.int64)[bi * N:(bi + 1) * N + 1]
            cnt = np.diff(off)
            lists = np.zeros((N, max(int(cnt.max()) if N else 0, 1)), np.int64)
            pos = np.arange(lists.shape[1])[None, :]
            live = pos < cnt[:, None]
            lists[live] = np.clip(np.asarray(csr[1], np.int64)[(off[:-1, None] + pos)[live]], 0, N - 1)
        out[bi], flags[bi] = _normals_of(pts[bi], pts[bi][lists], cnt, v)
    return out, flags


def analytic_normals_cloud(n: int, seed: int) -> np.ndarray:
    """The cloud the normal rule is tested on: half the points on the unit sphere centred (0, 0, 3), half on the plane z = 5 with
    x, y in [-1, 1]; Gaussian jitter of sigma 0.002 clipped at 0.01; rows permuted; float32 [n, 3]."""
    rng = np.random.Generator(np.random.Philox(key=int(seed)))
    h = n // 2
    u = rng.standard_normal((h, 3))
    sphere = u / np.linalg.norm(u, axis=1, keepdims=True) + np.array([0.0, 0.0, 3.0])
    plane = np.concatenate([rng.uniform(-1.0, 1.0, (n - h, 2)), np.full((n - h, 1), 5.0)], 1)
    pts = np.concatenate([sphere, plane], 0)
    pts = pts + np.clip(rng.standard_normal(pts.shape) * 0.002, -0.01, 0.01)
    return np.ascontiguousarray(pts[rng.permutation(n)], dtype=F)
