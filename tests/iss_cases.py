"""Inputs the ISS tests share (tests/test_iss_host.py on the CPU, tests/test_gpu_iss.py and tests/test_gpu_fpfh_keypoints.py on the
device): seeded jittered surfaces (deepsir_amd.fpfh.jittered_surface), never exact lattices, with host-built CSR lists, so that the
kernel tests do not depend on the device's radius search.  The CPU test asserts, for every case, the band condition the GPU test's
zero / non-zero comparison relies on."""
import functools

import numpy as np

from deepsir_amd import fpfh as F
from deepsir_amd import iss as I

BAND_CAP = 0.01                      # share of a case's points that may sit within BAND_EPS of a gamma (fpfh_cases.BAND_CAP)
SIZES = (1, 2, 4, 5, 6, 63, 64, 65, 257, 1024, 4096)
DEGREES = (0, 1, 4, 5, 6, 15, 16, 17, 63, 64, 65, 300)
PAD = np.float32(1e30)
R_SALIENT, R_NMS = 0.3, 0.2          # on jittered_surface's density (cell ~0.094): ~32 and ~14 entries per interior row
DEGENERATE_N = 400
# the bumpy pair of fpfh_cases (seed 1), registered on keypoints: fixed after the host chain of test_iss_host.py recovered the pose
PAIR_SEED = 1
PAIR_VOXEL = 0.05
PAIR_SALIENT, PAIR_NMS = 6 * PAIR_VOXEL, 4 * PAIR_VOXEL


def _sorted_lists(order: np.ndarray, deg) -> tuple:
    """CSR of the deg[i] nearest neighbours of every point (self first in ``order``), each row ascending."""
    n = order.shape[0]
    deg = np.broadcast_to(np.asarray(deg, np.int64), (n,))
    off = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    cols = np.concatenate([np.sort(order[i, :deg[i]]) for i in range(n)] + [np.zeros(0, np.int32)]).astype(np.int32)
    return off, cols


def _stack_csr(parts):
    """Per-cloud CSRs (offsets from 0) -> one batch CSR."""
    off, cols, base = [np.zeros(1, np.int64)], [], 0
    for o, c in parts:
        off.append(np.asarray(o[1:], np.int64) + base)
        cols.append(c)
        base += int(o[-1])
    return np.concatenate(off).astype(np.int32), np.concatenate(cols).astype(np.int32)


@functools.lru_cache(maxsize=None)
def fixed_case(n: int):
    """Three clouds of n rows in one call with live counts n, max(1, n - 1), max(1, (n + 1) // 2); rows past a cloud's count hold 1e30
    (coincident: their covariance is all zeros).  -> (points [3, n, 3], salient CSR, non-max CSR, counts); the CSRs are the host
    radius lists of R_SALIENT / R_NMS."""
    counts = (n, max(1, n - 1), max(1, (n + 1) // 2))
    pts = np.full((3, n, 3), PAD, np.float32)
    for c, m in enumerate(counts):
        pts[c, :m] = F.jittered_surface(m, 2000 * n + c)[0]
    return pts, I.radius_csr_host(pts, R_SALIENT), I.radius_csr_host(pts, R_NMS), counts


@functools.lru_cache(maxsize=None)
def degree_case():
    """One cloud of 512 points: salient row i has DEGREES[i % 12] entries (the nearest, self included, ascending), non-max row i
    DEGREES[(i + 5) % 12]: both straddle min_neighbors = 5 and the kernel's 16-lane group.  -> (points [1, 512, 3], salient, nms)."""
    n = 512
    p = F.jittered_surface(n, 4343)[0]
    order = F.knn_lists(p, 300)
    k = len(DEGREES)
    return (p[None], _sorted_lists(order, [DEGREES[i % k] for i in range(n)]),
            _sorted_lists(order, [DEGREES[(i + 5) % k] for i in range(n)]))


@functools.lru_cache(maxsize=None)
def degenerate_case():
    """Four clouds of DEGENERATE_N points, lists = the 24 nearest (self included), one CSR for both stages:
      0  a jittered surface with rows 3 and 4 exact duplicates (identical lists), and the two points farthest from them given a NaN
         and an infinite coordinate, each listed by its neighbours' rows (``touched``: the rows whose list holds one of the two)
      1  a perfect plane z = 0.25 (e3 == 0: the z row and column of C are exactly zero)
      2  collinear points along x (y, z constant: e2 == e3 == 0)
      3  all points coincident (C all zeros)
    -> (points [4, n, 3], csr, dict(dup=(3, 4), touched=rows))."""
    n = DEGENERATE_N
    surf = F.jittered_surface(n, 778)[0].copy()
    surf[4] = surf[3]
    plane = surf.copy(); plane[:, 2] = np.float32(0.25)
    line = surf.copy(); line[:, 1] = np.float32(0.5); line[:, 2] = np.float32(-0.125)
    line[:, 0] = np.linspace(0.0, 3.0, n, dtype=np.float32) + F.jittered_surface(n, 779)[0][:, 2] * np.float32(0.01)
    dot = np.tile(np.array([[0.3, -1.7, 2.5]], np.float32), (n, 1))
    parts, clouds = [], []
    for c, p in enumerate((surf, plane, line, dot)):
        order = F.knn_lists(p, 24)
        if c == 0:
            order[4] = order[3]                     # exact duplicates: identical rows, as a radius list gives them
            assert {3, 4} <= set(order[3].tolist())
        parts.append(_sorted_lists(order, 24))
        clouds.append(p)
    pts = np.stack(clouds)
    off, cols = _stack_csr(parts)
    far = np.argsort(((surf.astype(np.float64) - surf[3]) ** 2).sum(1))[-2:]
    pts[0, far[0], 1], pts[0, far[1], 0] = np.nan, np.inf    # after the lists were made: the neighbours' rows still hold the two
    touched = np.nonzero([np.isin(cols[off[i]:off[i + 1]], far).any() for i in range(n)])[0]
    return pts, (off, cols), {"dup": (3, 4), "touched": touched, "bad": tuple(int(f) for f in far)}


@functools.lru_cache(maxsize=None)
def offset_case():
    """1024 surface points moved by (1e5, -1e5, 1e5) before the rounding to fp32 (ulp 2^-7: the two-pass fp64 covariance must not lose
    the neighbourhood's shape to the offset), host radius lists.  -> (points [1, n, 3], salient, nms)."""
    p = F.jittered_surface(1024, 991)[0].astype(np.float64) + np.array([1e5, -1e5, 1e5])
    pts = p.astype(np.float32)[None]
    return pts, I.radius_csr_host(pts, R_SALIENT), I.radius_csr_host(pts, R_NMS)


@functools.lru_cache(maxsize=None)
def bad_index_case():
    """fixed_case(257)'s first cloud with out-of-range columns: row 10 starts with -1, row 20 ends with n, row 30 ends with 2^31 - 1
    (rows stay ascending).  The rule clamps them to 0 and n - 1.  -> (points [1, n, 3], salient, nms)."""
    pts, sal, nms, _ = fixed_case(257)
    n = pts.shape[1]
    out = []
    for off, cols in (sal, nms):
        off, cols = off[:n + 1].copy(), cols[:off[n]].copy()
        cols[off[10]], cols[off[21] - 1], cols[off[31] - 1] = -1, n, 2 ** 31 - 1
        out.append((off, cols))
    return np.ascontiguousarray(pts[:1]), out[0], out[1]


def all_cases():
    """(name, points, salient CSR, non-max CSR) of every case the device is compared on."""
    for n in SIZES:
        pts, sal, nms, _ = fixed_case(n)
        yield f"fixed{n}", pts, sal, nms
    pts, sal, nms = degree_case()
    yield "degree", pts, sal, nms
    pts, csr, _ = degenerate_case()
    yield "degenerate", pts, csr, csr
    pts, sal, nms = offset_case()
    yield "offset", pts, sal, nms
    pts, sal, nms = bad_index_case()
    yield "bad_index", pts, sal, nms


CASE_NAMES = tuple(f"fixed{n}" for n in SIZES) + ("degree", "degenerate", "offset", "bad_index")


def case(name: str):
    for nm, pts, sal, nms in all_cases():
        if nm == name:
            return pts, sal, nms
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def host(name: str):
    """The host rule on a case, computed once."""
    pts, sal, nms = case(name)
    return I.iss_keypoints_host(pts, sal, nms)


@functools.lru_cache(maxsize=None)
def pair():
    return F.bumpy_pair(PAIR_SEED)


@functools.lru_cache(maxsize=None)
def near_plane_pair():
    """A pair that must fall back: the bumpy pair's layout with the ref side flattened onto the exact plane z = 0.25 (no keypoint on
    ref, whatever rounding leaves on the moved src side) and src = the same points under the pair's pose."""
    pr = {k: v.copy() for k, v in F.bumpy_pair(PAIR_SEED + 2).items()}
    ref = pr["points_ref"][0].copy()
    ref[:, 2] = np.float32(0.25)
    gt = pr["transform_gt"][0].astype(np.float64)
    pr["points_ref"] = ref[None]
    pr["points_src"] = ((ref[pr["perm"]].astype(np.float64) - gt[:, 3]) @ gt[:, :3]).astype(np.float32)[None]
    return pr
