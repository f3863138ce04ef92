"""Inputs shared by tests/test_fps_host.py and tests/test_gpu_fps.py (farthest-point sampling, csrc/fps.hip; the rule's host
restatement is deepsir_amd/fps.py).  Everything is generated from a seed."""
import functools

import numpy as np

SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 5000, 8192, 8193, 20000)      # lane, wave and workgroup edges, both sides of the tier edge


def random_cloud(n: int, seed: int = 0) -> np.ndarray:
    rng = np.random.Generator(np.random.Philox(key=1000 + seed))
    return rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)


def lattice(m: int = 4) -> np.ndarray:
    """m x m x m points at integer coordinates, row = (x m + y) m + z: every distance is an exact small integer, ties everywhere"""
    g = np.arange(m, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def lattice_cloud(n: int) -> np.ndarray:
    """the first n rows of the smallest lattice that holds n points, scaled by 2^-4 (still exact in fp32)"""
    m = 1
    while m ** 3 < n:
        m += 1
    return lattice(m)[:n] * np.float32(0.0625)


def duplicate_cloud(n: int, seed: int = 0) -> np.ndarray:
    """every row of the first half appears again in the second half (n odd: one row without a twin)"""
    p = random_cloud(n, seed)
    h = n // 2
    p[h:2 * h] = p[:h]
    return p


def offset_cloud(n: int, seed: int = 0) -> np.ndarray:
    """coordinates near 1e5: the differences are exact, the squares round"""
    return (random_cloud(n, seed).astype(np.float64) + 1.0e5).astype(np.float32)


def nonfinite_rows(n: int, seed: int = 0) -> np.ndarray:
    """about a fifth of the rows (row 0 among them where n > 1), NaN or +-inf in one coordinate"""
    rng = np.random.Generator(np.random.Philox(key=2000 + seed))
    rows = np.nonzero(rng.random(n) < 0.2)[0]
    return np.unique(np.concatenate([[0], rows])) if n > 1 else rows


def nonfinite_cloud(n: int, seed: int = 0) -> np.ndarray:
    p = random_cloud(n, seed)
    bad = (np.nan, np.inf, -np.inf)
    for j, r in enumerate(nonfinite_rows(n, seed)):
        p[r, j % 3] = bad[j % 3]
    return p


KINDS = {"random": random_cloud, "lattice": lattice_cloud, "duplicates": duplicate_cloud, "offset": offset_cloud,
         "nonfinite": nonfinite_cloud}


def cloud(kind: str, n: int) -> np.ndarray:
    return KINDS[kind](n)


def ks(n: int, with_all: bool = True):
    """the k of the GPU tests at a size: 1, 2, min(n, 300), and n itself up to 1025 rows"""
    out = {1, min(2, n), min(n, 300)}
    if with_all and n <= 1025:
        out.add(n)
    return sorted(out)


@functools.lru_cache(maxsize=None)
def host(kind: str, n: int, k: int, start: int = 0):
    """the host rule's result for a shared case, computed once"""
    from deepsir_amd.fps import farthest_point_sample_host
    return farthest_point_sample_host(cloud(kind, n)[None], k, start=start)
