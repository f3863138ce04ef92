"""Host restatement of the ISS keypoint rule of ``csrc/iss.hip`` (include/dsir.h, dsir_iss_keypoints) in numpy.

ISS (intrinsic shape signatures, Zhong 2009; open3d ``compute_iss_keypoints``) keeps the points whose neighbourhood covariance has
three well separated eigenvalues and whose smallest eigenvalue is a local maximum.  open3d cannot be imported here, so parity is
unpinned and the engine owns the rule; the header of csrc/iss.hip states it, this module states it a second time, the way
``fpfh.py`` and ``ppf.py`` do for their rules: the tests compare the device against it, the product path never calls it.

    inputs: points [c, n, >= 3] fp32, a salient CSR and a non-max CSR (offsets [c n + 1], cols: cloud-local, ascending per row, self
            included; a column is clamped into [0, n - 1]), gamma_21, gamma_32, min_neighbors
    stage 1, point i with salient row q_0 .. q_(cnt - 1):
      cnt < min_neighbors                                   s_i = 0
      m = (sum_k q_k) / cnt;  C = (sum_k (q_k - m)(q_k - m)^T) / cnt          float64
      an entry of C not finite, or C all zeros              s_i = 0
      e1 >= e2 >= e3 = |eigenvalues| of C (``numpy.linalg.eigvalsh``; the device takes the singular values of svd3)
      e1 > 0, e2 > 0, e2 / e1 < gamma_21, e3 / e2 < gamma_32 (strict)         s_i = float32(e3), else 0
    stage 2, point i with non-max row R_i:  keypoint iff s_i > 0, |R_i| >= min_neighbors, no j in R_i with s_j > s_i, and no j in R_i
      with s_j == s_i and j < i (exact duplicates yield one keypoint, the lower index; open3d keeps both)
    outputs: saliency [c, n] f32, mask [c, n] i32, index [c, n] i32 (keypoints ascending, then -1), counts [c] i32

The device fixes its summation order (16 lanes per row, an xor butterfly); numpy sums in its own order, so stage 1 agrees to rounding
(the GPU test's bound: 1e-9 e1 + one fp32 ulp) and the two inequalities can differ where a ratio sits within ``BAND_EPS`` of its
gamma: ``band`` marks those points.  Stage 2 only compares floats: it is exact on whatever saliency array it is given.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

BAND_EPS = 1e-9
GAMMA_21 = 0.975
GAMMA_32 = 0.975
MIN_NEIGHBORS = 5


def _csr(csr, c: int, n: int) -> Tuple[np.ndarray, np.ndarray]:
    off, cols = np.asarray(csr[0], np.int64), np.asarray(csr[1], np.int64)
    if off.shape != (c * n + 1,):
        raise ValueError(f"iss: csr offsets must be [{c * n + 1}]")
    return off, cols


def _check(gamma_21, gamma_32, min_neighbors):
    for g in (gamma_21, gamma_32):
        if not (np.isfinite(g) and g > 0):
            raise ValueError("iss: gamma_21 and gamma_32 must be finite and positive")
    if int(min_neighbors) < 1:
        raise ValueError("iss: min_neighbors >= 1 expected")


def _edges(off: np.ndarray, cols: np.ndarray, c: int, n: int):
    """(deg [c n], rows [E]: the global row of every list entry, gj [E]: the global row of its clamped neighbour, jl [E]: cloud-local)."""
    deg = np.maximum(off[1:] - off[:-1], 0)
    rows = np.repeat(np.arange(c * n, dtype=np.int64), deg)
    pos = np.arange(int(deg.sum()), dtype=np.int64) - np.repeat(np.cumsum(deg) - deg, deg) + np.repeat(off[:-1], deg)
    jl = np.clip(cols[pos], 0, n - 1) if pos.size else np.zeros(0, np.int64)
    return deg, rows, (rows // n) * n + jl, jl


def iss_saliency_host(points: np.ndarray, csr, gamma_21: float = GAMMA_21, gamma_32: float = GAMMA_32,
                      min_neighbors: int = MIN_NEIGHBORS) -> Dict[str, np.ndarray]:
    """Stage 1.  points [c, n, >= 3] fp32, csr = the salient lists.  -> dict(saliency [c, n] f32, eig [c, n, 3] f64: e1 >= e2 >= e3
    (zeros where the row is short or C degenerate), band [c, n] bool).  Sums run over a row's entries in row order."""
    _check(gamma_21, gamma_32, min_neighbors)
    pts = np.asarray(points, np.float32)
    c, n = pts.shape[:2]
    off, cols = _csr(csr, c, n)
    P = pts[:, :, :3].astype(np.float64).reshape(c * n, 3)
    deg, rows, gj, _ = _edges(off, cols, c, n)
    R = c * n
    cnt = np.maximum(deg, 1).astype(np.float64)
    with np.errstate(all="ignore"):
        m = np.stack([np.bincount(rows, weights=P[gj, a], minlength=R) for a in range(3)], 1) / cnt[:, None]
        e = P[gj] - m[rows]
        Cm = np.zeros((R, 3, 3))
        for a in range(3):
            for b in range(a, 3):
                Cm[:, a, b] = Cm[:, b, a] = np.bincount(rows, weights=e[:, a] * e[:, b], minlength=R) / cnt
        ok = (deg >= min_neighbors) & np.isfinite(Cm).all((1, 2)) & (Cm != 0.0).any((1, 2))
        eig = np.zeros((R, 3))
        if ok.any():
            eig[ok] = np.sort(np.abs(np.linalg.eigvalsh(Cm[ok])), axis=1)[:, ::-1]
        pos = ok & (eig[:, 0] > 0) & (eig[:, 1] > 0)
        r21 = np.where(pos, eig[:, 1] / np.where(pos, eig[:, 0], 1.0), np.inf)
        r32 = np.where(pos, eig[:, 2] / np.where(pos, eig[:, 1], 1.0), np.inf)
        band = pos & ((np.abs(r21 - gamma_21) <= BAND_EPS) | (np.abs(r32 - gamma_32) <= BAND_EPS))
        sal = np.where(pos & (r21 < gamma_21) & (r32 < gamma_32), eig[:, 2], 0.0).astype(np.float32)
    return {"saliency": sal.reshape(c, n), "eig": eig.reshape(c, n, 3), "band": band.reshape(c, n)}


def iss_select_host(saliency: np.ndarray, csr, min_neighbors: int = MIN_NEIGHBORS) -> Dict[str, np.ndarray]:
    """Stage 2 on a saliency array [c, n] f32 (the host's or the device's), csr = the non-max lists.  -> dict(mask [c, n] i32, index
    [c, n] i32, counts [c] i32)."""
    s = np.ascontiguousarray(saliency, np.float32)
    c, n = s.shape
    off, cols = _csr(csr, c, n)
    deg, rows, gj, jl = _edges(off, cols, c, n)
    flat = s.reshape(-1)
    with np.errstate(invalid="ignore"):
        beaten = (flat[gj] > flat[rows]) | ((flat[gj] == flat[rows]) & (jl < rows % n))
        keep = (flat > 0) & (deg >= min_neighbors) & (np.bincount(rows[beaten], minlength=c * n) == 0)
    mask = keep.astype(np.int32).reshape(c, n)
    index = np.full((c, n), -1, np.int32)
    counts = mask.sum(1).astype(np.int32)
    for cl in range(c):
        index[cl, :counts[cl]] = np.nonzero(mask[cl])[0]
    return {"mask": mask, "index": index, "counts": counts}


def iss_keypoints_host(points: np.ndarray, csr_salient, csr_nms, gamma_21: float = GAMMA_21, gamma_32: float = GAMMA_32,
                       min_neighbors: int = MIN_NEIGHBORS) -> Dict[str, np.ndarray]:
    """Both stages: dict(index, counts, saliency, mask, eig, band)."""
    out = iss_saliency_host(points, csr_salient, gamma_21, gamma_32, min_neighbors)
    out.update(iss_select_host(out["saliency"], csr_nms, min_neighbors))
    return out


def radius_csr_host(points: np.ndarray, radius: float) -> Tuple[np.ndarray, np.ndarray]:
    """The self-neighbourhood CSR of a dense batch [c, n, >= 3] under ``overlap.radius_pair_host``'s rule (what
    ``Engine.radius_neighbors(points, radius, 0)`` returns): (offsets [c n + 1] i32, cols i32)."""
    from .overlap import radius_pair_host
    pts = np.asarray(points, np.float32)
    counts, cols = [], []
    for cl in range(pts.shape[0]):
        k, col, _ = radius_pair_host(pts[cl], pts[cl], radius)
        counts.append(k)
        cols.append(col)
    off = np.concatenate([[0], np.cumsum(np.concatenate(counts), dtype=np.int64)]).astype(np.int32)
    return off, np.concatenate(cols).astype(np.int32)
