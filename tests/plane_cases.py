"""Inputs shared by tests/test_plane_host.py, tests/test_gpu_plane.py and tests/test_gpu_remove_ground.py (plane segmentation,
csrc/plane.hip; the rule's host restatement is deepsir_amd/plane.py).  Everything is generated from fixed Philox keys."""
import functools

import numpy as np

SIZES = (3, 4, 63, 64, 65, 255, 256, 257, 1025, 5000)      # lane, wave and workgroup edges; 5000 spans two refit slices and 20 chunks
HYPS = (1, 64, 257, 1024)                                  # one lane, one fitting workgroup, past a scoring workgroup's 512, the default
THR = 0.08                                                 # metres: 4 sigma of the sheet's noise
GRID = np.float32(2.0 ** -7)                               # every coordinate is a multiple: a shift by 1e5 stays exact in fp32


def _rng(key):
    return np.random.Generator(np.random.Philox(key=key))


def _quant(p):
    return (np.round(np.asarray(p, np.float64) / float(GRID)) * float(GRID)).astype(np.float32)


def scene(n: int, seed: int = 0) -> np.ndarray:
    """a noisy z = 0 sheet (sigma 0.02 m over 20 m x 20 m) holding 55 % of the rows, two boxes standing on it and scattered points,
    in shuffled row order"""
    rng = _rng(3000 + seed)
    ns = int(round(0.55 * n))
    nb = (n - ns) // 3
    sheet = np.stack([rng.uniform(-10, 10, ns), rng.uniform(-10, 10, ns), rng.normal(0, 0.02, ns)], -1)
    boxes = []
    for centre, size in (((-4.0, 3.0), (2.0, 3.0, 1.5)), ((5.0, -2.0), (1.0, 1.0, 2.5))):
        q = rng.uniform(0, 1, (nb, 3)) * size
        face = rng.integers(0, 5, nb)                            # four walls and the roof
        q[face == 0, 0] = 0; q[face == 1, 0] = size[0]; q[face == 2, 1] = 0; q[face == 3, 1] = size[1]; q[face == 4, 2] = size[2]
        q[:, :2] += centre
        boxes.append(q)
    rest = n - ns - 2 * nb
    scatter = np.stack([rng.uniform(-10, 10, rest), rng.uniform(-10, 10, rest), rng.uniform(0.3, 4, rest)], -1)
    p = np.concatenate([sheet] + boxes + [scatter])
    return _quant(p[rng.permutation(n)])


def scene_truth(n: int, seed: int = 0) -> int:
    """rows of scene(n) within THR of the true plane z = 0, in float64"""
    return int((np.abs(scene(n, seed)[:, 2].astype(np.float64)) < THR).sum())


def _two_planes(n: int, floor_share: float, seed: int):
    """a floor z = 0 and a wall x = 5, sigma 0.01 m, floor_share of the rows on the floor; shuffled -> (points, is_floor)"""
    rng = _rng(3100 + seed)
    nf = int(round(floor_share * n))
    floor = np.stack([rng.uniform(-5, 5, nf), rng.uniform(-5, 5, nf), rng.normal(0, 0.01, nf)], -1)
    wall = np.stack([5 + rng.normal(0, 0.01, n - nf), rng.uniform(-5, 5, n - nf), rng.uniform(0.2, 6, n - nf)], -1)
    perm = rng.permutation(n)
    return _quant(np.concatenate([floor, wall])[perm]), (np.arange(n) < nf)[perm]


def two_planes(n: int, floor_share: float = 0.6, seed: int = 0) -> np.ndarray:
    return _two_planes(n, floor_share, seed)[0]


def two_planes_is_floor(n: int, floor_share: float = 0.6, seed: int = 0) -> np.ndarray:
    return _two_planes(n, floor_share, seed)[1]


def lattice(n: int = 64) -> np.ndarray:
    """the first n rows of the smallest m x m x m integer lattice holding n points, row = (x m + y) m + z: exact ties everywhere"""
    m = 1
    while m ** 3 < n:
        m += 1
    g = np.arange(m, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:n].copy()


def collinear(n: int) -> np.ndarray:
    """t (1, 2, 3) + (4, 5, 6) for integer t: every cross product is exactly zero, every triple rejected"""
    t = np.arange(n, dtype=np.float32)[:, None]
    return t * np.array([1, 2, 3], np.float32) + np.array([4, 5, 6], np.float32)


def duplicates(n: int) -> np.ndarray:
    """two distinct points repeated: every triple of distinct rows still spans no plane"""
    p = np.empty((n, 3), np.float32)
    p[0::2] = (1.5, -2.0, 0.25)
    p[1::2] = (-3.0, 4.0, 7.5)
    return p


OFFSET = np.float32(1.0e5)


def offset_scene(n: int, seed: int = 0) -> np.ndarray:
    """scene shifted by 1e5 m along every coordinate; fp32 addition, exact wherever the row survives scene + 1e5 - 1e5"""
    return scene(n, seed) + OFFSET


def nonfinite_rows(n: int, seed: int = 0) -> np.ndarray:
    """about a tenth of the rows, row 0 among them"""
    rows = np.nonzero(_rng(3200 + seed).random(n) < 0.1)[0]
    return np.unique(np.concatenate([[0], rows]))


def nonfinite_scene(n: int, seed: int = 0) -> np.ndarray:
    p = scene(n, seed)
    bad = (np.nan, np.inf, -np.inf)
    for j, r in enumerate(nonfinite_rows(n, seed)):
        p[r, j % 3] = bad[j % 3]
    return p


KINDS = {"scene": scene, "two_planes": two_planes, "lattice": lattice, "collinear": collinear, "duplicates": duplicates,
         "offset": offset_scene, "nonfinite": nonfinite_scene}
THRS = {"lattice": 0.5}                                    # lattice planes: neighbours sit at exact multiples of the spacing


def cloud(kind: str, n: int) -> np.ndarray:
    return KINDS[kind](n)


def thr(kind: str) -> float:
    return THRS.get(kind, THR)


AXIS = dict(axis=(0.0, 0.0, 1.0), max_angle_deg=15.0)


@functools.lru_cache(maxsize=None)
def host(kind: str, n: int, hypotheses: int, max_planes: int, with_axis: bool, refine_iters: int = 0, seed: int = 0):
    """the host rule's result for a shared case, computed once: the six arrays of Engine.segment_plane for a batch of one"""
    from deepsir_amd.plane import segment_plane_host
    kw = dict(AXIS) if with_axis else {}
    return segment_plane_host(cloud(kind, n)[None], thr(kind), hypotheses=hypotheses, max_planes=max_planes, refine_iters=refine_iters,
                              seed=seed, **kw)
