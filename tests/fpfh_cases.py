"""Inputs the FPFH tests share (tests/test_fpfh_host.py on the CPU, tests/test_gpu_fpfh.py on the device): seeded jittered
surfaces, never exact lattices with anti-parallel normals, so that the host rule's ambiguity band stays under BAND_CAP; the CPU
test asserts that for every case the GPU test compares bytes on."""
import functools

import numpy as np

from deepsir_amd import fpfh as F

BAND_CAP = 0.01                      # share of a case's points that may sit in the band (and are left out of the byte comparison)
FIXED_SIZES = (1, 2, 15, 16, 17, 63, 64, 65, 257, 1024)
CSR_DEGREES = (0, 1, 15, 16, 17, 63, 64, 65, 300)
PAIR_SEED = 1                        # bumpy_pair: fixed after the host chain recovered the pose (test_fpfh_host.py)
PAIR_VOXEL = 0.05
PAIR_HYPOTHESES = 1024
PAD = np.float32(1e30)
DEGENERATE_N = 400


@functools.lru_cache(maxsize=None)
def fixed_case(n: int):
    """Three clouds of n rows in one call: counts n, max(1, n - 1) and max(1, (n + 1) // 2); rows past a cloud's count hold 1e30 and a
    list that is all self; a cloud of fewer than 16 live points pads its lists with self.  -> (points [3,n,3], normals [3,n,3],
    neigh [3,n,16] i32, counts)."""
    counts = (n, max(1, n - 1), max(1, (n + 1) // 2))
    pts = np.full((3, n, 3), PAD, np.float32)
    nrm = np.zeros((3, n, 3), np.float32)
    nrm[:, :, 2] = 1.0
    nb = np.repeat(np.arange(n, dtype=np.int32)[None, :, None], 3, 0).repeat(16, 2)
    for c, m in enumerate(counts):
        p, v = F.jittered_surface(m, 1000 * n + c)
        pts[c, :m], nrm[c, :m] = p, v
        nb[c, :m] = F.knn_lists(p)
    return pts, nrm, np.ascontiguousarray(nb), counts


@functools.lru_cache(maxsize=None)
def csr_case():
    """One cloud of 512 points whose rows have the degrees of CSR_DEGREES in turn (the d nearest neighbours, self first)."""
    n = 512
    p, v = F.jittered_surface(n, 4242)
    order = F.knn_lists(p, 300)
    deg = np.array([CSR_DEGREES[i % len(CSR_DEGREES)] for i in range(n)], np.int64)
    off = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    cols = np.concatenate([order[i, :deg[i]] for i in range(n)]).astype(np.int32)
    return p[None], v[None], off, cols


@functools.lru_cache(maxsize=None)
def degenerate_case():
    """DEGENERATE_N points of a jittered surface with: rows 3 and 4 duplicates of each other (and each in the other's list), row 7 a zero
    normal, row 9 a NaN coordinate, row 11 a list that is all self, row 13 an infinite normal.  -> (points, normals, neigh, dict of
    the touched rows)."""
    n = DEGENERATE_N
    p, v = F.jittered_surface(n, 777)
    nb = F.knn_lists(p)
    p, v = p.copy(), v.copy()
    p[4] = p[3]
    nb[3, 1], nb[4, 1] = 4, 3
    v[7] = 0.0
    p[9, 1] = np.nan
    nb[11] = 11
    v[13, 0] = np.inf
    return p[None], v[None], np.ascontiguousarray(nb[None]), {"dup": (3, 4), "zero_normal": 7, "nan": 9, "self": 11, "inf_normal": 13}


@functools.lru_cache(maxsize=None)
def pair():
    return F.bumpy_pair(PAIR_SEED)


@functools.lru_cache(maxsize=None)
def pair_host_chain(p: int = 0):
    """The host chain on the fixed pair as pair ``p`` of a batch (p enters RANSAC's draws)."""
    return F.host_chain(pair(), PAIR_VOXEL, PAIR_HYPOTHESES, seed=0, p=p)
