"""Inputs and a plain reference the pre-processing tests share (tests/test_preprocess_host.py on the CPU,
tests/test_gpu_preprocess_edges.py on the device).  No GPU and no engine import here.

``plain_voxel_downsample`` / ``plain_resample`` restate the rule of oracle/preprocess.py's docstring without any of the oracle's
machinery: a Python dict keyed by the (ix, iy, iz) tuple of Python ints instead of a packed 64-bit key and a stable sort, Python
float (IEEE double) sums added one by one instead of ``np.add.at``, an own splitmix64.  The host test holds the oracle against
them; the device test holds csrc/preprocess.hip against the oracle.  Every comparison is integer work or a float64 sum in a fixed
order, so all of it is bit for bit.

``CASES`` maps a name to a builder that returns a list of ``Batch`` (clouds, voxel, crop, cap, ...): one device call each.  A
builder asserts, on the CPU, the property that gives its case its teeth (the share of rows whose voxel changes under float32 index
arithmetic, a point that a fused crop classifies differently, "exactly one voxel", ...).  No cloud has more than 4096 points, no
batch more than about 20 000."""
import functools
import math
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

INDEX_LIMIT = 1 << 18                # a voxel index has 18 bits per axis
MAX_CLOUDS = 1000                    # per dsir_voxel_downsample call (include/dsir.h)
_M64 = (1 << 64) - 1

CROP = (3.0, 25.0, -2.5, 1.75)       # r_min, r_max, z_min, z_max: all exact in float32, and so are their squares


class Batch(NamedTuple):
    clouds: List[np.ndarray]         # ragged [n_i, C] float32
    voxel: float
    crop: Optional[Tuple[float, float, float, float]]
    cap: int
    label: str
    refused: Optional[Tuple[int, int, int]] = None     # (cloud, cloud-local row, axis) of the first point that cannot be keyed


# ---------------------------------------------------------------------------------------------------------------- plain reference
def plain_crop_keep(points: np.ndarray, crop) -> np.ndarray:
    p = np.asarray(points, np.float32)
    if crop is None:
        return np.ones(len(p), bool)
    r_min, r_max, z_min, z_max = (np.float32(c) for c in crop)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    r2 = (x * x + y * y) + z * z                                   # float32 arrays: every product and sum rounds to float32
    assert r2.dtype == np.float32
    return (r2 <= r_max * r_max) & (r2 > r_min * r_min) & (z >= z_min) & (z <= z_max)


def plain_voxel_index(points: np.ndarray, voxel: float, crop=None):
    """-> (surviving rows, their (ix, iy, iz) tuples of Python ints).  ValueError on a surviving row that has a coordinate that is
    not finite or an index outside [0, 2^18)."""
    pts = np.asarray(points, np.float32)
    keep = plain_crop_keep(pts, crop)
    rows = [i for i in range(len(pts)) if keep[i]]
    xyz = pts[:, :3].astype(np.float64).tolist()
    for r in rows:
        for a in range(3):
            if not math.isfinite(xyz[r][a]):
                raise ValueError(f"row {r} axis {a}: coordinate {xyz[r][a]} is not finite")
    if not rows:
        return rows, []
    v = float(np.float32(voxel))
    lo = [min(xyz[r][a] for r in rows) for a in range(3)]
    cells = []
    for r in rows:
        t = tuple(int(math.floor((xyz[r][a] - (lo[a] - 0.5 * v)) / v)) for a in range(3))
        for a in range(3):
            if not 0 <= t[a] < INDEX_LIMIT:
                raise ValueError(f"row {r} axis {a}: voxel index {t[a]} outside [0, 2^18)")
        cells.append(t)
    return rows, cells


def plain_voxel_downsample(points: np.ndarray, voxel: float, crop=None) -> np.ndarray:
    pts = np.asarray(points, np.float32)
    C = pts.shape[1]
    rows, cells = plain_voxel_index(pts, voxel, crop)
    members = {}
    for r, t in zip(rows, cells):                                  # ascending input order inside a voxel
        members.setdefault(t, []).append(r)
    vals = pts.astype(np.float64).tolist()
    out = np.zeros((len(members), C), np.float32)
    for s, t in enumerate(sorted(members)):
        acc = [0.0] * C
        for r in members[t]:
            for c in range(C):
                acc[c] += vals[r][c]
        for c in range(C):
            out[s, c] = np.float32(acc[c] / float(len(members[t])))
    return out


def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _M64
    x ^= x >> 31
    return x


def plain_resample(points: np.ndarray, k: int, cloud: int, seed: int, mode: str = "random") -> np.ndarray:
    pts = np.asarray(points, np.float32)
    n = len(pts)
    out = np.zeros((k, pts.shape[1]), np.float32)
    if n == 0:
        return out
    seed &= _M64
    if mode == "fixed":
        picks = [j % n for j in range(k)]
    else:
        order = sorted(range(n), key=lambda i: (_splitmix64(seed ^ (cloud << 40) ^ i) >> 1, i))
        picks = order[:min(k, n)]
        for j in range(n, k):
            picks.append(_splitmix64((seed ^ _M64) ^ (cloud << 40) ^ j) % n)
    for j, r in enumerate(picks):
        out[j] = pts[r]
    return out


# ------------------------------------------------------------------------------------------------------------------------ builders
def _cloud(rng, n, stride, lo=-40.0, hi=25.0):
    p = np.empty((n, stride), np.float32)
    p[:, :3] = rng.uniform(lo, hi, (n, 3))
    p[:, 3:] = rng.uniform(-1.0, 1.0, (n, stride - 3))
    return p


def _cap(clouds):
    return max(1, max(len(c) for c in clouds))


def signs_and_strides():
    """Coordinates of both signs; one batch per stride in {3, 4, 6, 16} (16 is the kernel's accumulator limit); cloud sizes 1, 2 (the
    same point twice), 257, 1025 (past one 1024-thread pass of the bounds kernel) and 4096."""
    out = []
    for stride in (3, 4, 6, 16):
        rng = np.random.default_rng(100 + stride)
        clouds = [_cloud(rng, n, stride) for n in (1, 2, 257, 1025, 4096)]
        clouds[1][1] = clouds[1][0]
        out.append(Batch(clouds, 2.5, None, _cap(clouds), f"stride{stride}"))
    return out


def empty_members():
    """A zero-point cloud first, in the middle, last, and two in a row: offsets repeat where the key kernel binary-searches them."""
    rng = np.random.default_rng(200)
    full = lambda n: _cloud(rng, n, 4, -3.0, 3.0)
    none = lambda: np.zeros((0, 4), np.float32)
    out = []
    for label, sizes in (("first", (0, 300, 700)), ("middle", (300, 0, 700)), ("last", (300, 700, 0)), ("two", (300, 0, 0, 700, 0))):
        clouds = [full(n) if n else none() for n in sizes]
        out.append(Batch(clouds, 0.4, None, _cap(clouds), label))
    return out


def one_voxel():
    """Every point of a cloud in one voxel: one thread walks the whole run of 4096.  Stride 6."""
    rng = np.random.default_rng(300)
    a = _cloud(rng, 4096, 6)
    a[:, :3] = (np.array([5.2, -3.1, 0.7]) + rng.uniform(0.0, 1e-3, (4096, 3))).astype(np.float32)
    assert len(np.unique(a[:, :3], axis=0)) == 4096
    b = np.repeat(_cloud(rng, 1, 6), 4096, 0)
    for c in (a, b):
        assert len(set(plain_voxel_index(c, 1.0)[1])) == 1
    return [Batch([a, b], 1.0, None, 4096, "distinct+identical")]


FACE_VOXELS = (0.25, 0.1, 0.06)
FACE_ORIGINS = (-7.3, 0.0, 1234.5)
FACE_FLIP_SHARE = 0.25


def float32_voxel_index(points: np.ndarray, voxel: float) -> np.ndarray:
    """The index rule with every operation in float32: what a kernel that skipped the float64 conversion would compute."""
    p = np.asarray(points, np.float32)[:, :3]
    v = np.float32(voxel)
    q = np.floor((p - (p.min(0) - np.float32(0.5) * v)) / v)
    assert q.dtype == np.float32
    return q.astype(np.int64)


def voxel_faces():
    """Points on the faces of the voxel lattice: p = float32(m + (k + 0.5) * v) with integer k uniform in [0, 200)^3, plus the
    point (m, m, m), which is the min bound, so that the quotient of every other point is an integer up to the rounding of p to
    float32 and of v to float32.  One batch per voxel size, one cloud per origin m.

    Shares of rows whose voxel changes when the index is evaluated in float32 (measured with this builder):
        v = 0.1 : m = -7.3: 0.62, m = 0: 0.86, m = 1234.5: 0.93        v = 0.06: m = -7.3: 0.03, m = 0: 0.50, m = 1234.5: 0.57
    Asserted: at least FACE_FLIP_SHARE of the rows of each non-dyadic size's batch, and at least one row of every cloud of it.
    For v = 0.25 and the two origins that float32 holds exactly the quotient of every lattice point is an exact integer (asserted;
    float32 and float64 agree there, the case pins the closed side of the face); at m = -7.3 the rounding of p moves it off it."""
    out = []
    for v in FACE_VOXELS:
        clouds, flips = [], []
        for m in FACE_ORIGINS:
            rng = np.random.default_rng(int(1000 * v) * 7 + int(abs(m)))
            k = rng.integers(0, 200, (4095, 3))
            p = np.concatenate([np.full((1, 3), m), np.float64(m) + (k + 0.5) * v]).astype(np.float32)
            rows, cells = plain_voxel_index(p, v)
            flip = (np.asarray(cells, np.int64) != float32_voxel_index(p, v)).any(1)
            if v == 0.25:
                vf = float(np.float32(v))
                quo = (p[1:].astype(np.float64) - (p.min(0).astype(np.float64) - 0.5 * vf)) / vf
                if float(np.float32(m)) == m:
                    assert np.array_equal(quo, np.round(quo)) and np.array_equal(quo, k + 1.0), (v, m)
            else:
                assert flip.any(), (v, m)
            clouds.append(p)
            flips.append(flip)
        if v != 0.25:
            share = float(np.concatenate(flips).mean())
            assert share >= FACE_FLIP_SHARE, (v, share)
        out.append(Batch(clouds, v, None, 4096, f"v{v}"))
    return out


def _r2_unfused(p):
    x, y, z = (p[:, i].astype(np.float32) for i in range(3))
    return (x * x + y * y) + z * z


def _r2_fused(p):
    """fma(z, z, fma(y, y, x * x)) emulated: the products of float32 values are exact in float64."""
    x, y, z = (p[:, i].astype(np.float64) for i in range(3))
    t = (x * x).astype(np.float32).astype(np.float64)
    t = (y * y + t).astype(np.float32).astype(np.float64)
    return (z * z + t).astype(np.float32)


def _near_sphere(rng, radius, n, z_lo, z_hi):
    """n float32 points whose unfused float32 r2 lies within 4 ulp of radius^2, on both sides, with z strictly inside (z_lo, z_hi)."""
    target = np.float32(radius) * np.float32(radius)
    ulp = np.spacing(target)
    got = []
    while sum(len(g) for g in got) < n:
        d = rng.normal(size=(4 * n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        d = d[(d[:, 2] * radius > z_lo + 0.01) & (d[:, 2] * radius < z_hi - 0.01)]
        p = (d * radius * (1.0 + rng.integers(-3, 4, (len(d), 1)) * 2.0 ** -25)).astype(np.float32)
        got.append(p[np.abs(_r2_unfused(p) - target) <= 4 * ulp])
    return np.concatenate(got)[:n]


def crop_faces():
    """Points within 4 float32 ulp of r_max^2 (cloud 0) and of r_min^2 (cloud 1), and (cloud 2) points with z exactly z_min, z_max
    and their float32 neighbours, points with r2 == r_max^2 exactly (kept) and r2 == r_min^2 exactly (dropped).  Asserted: both
    sides of every threshold are populated, and a fused evaluation of r2 classifies at least one point of each sphere cloud
    differently from the unfused float32 rule that crop_ok and the oracle pin."""
    r_min, r_max, z_min, z_max = CROP
    rng = np.random.default_rng(500)
    clouds = []
    for radius in (r_max, r_min):
        p = _near_sphere(rng, radius, 4096, z_min, z_max)
        t = np.float32(radius) * np.float32(radius)
        u, f = _r2_unfused(p), _r2_fused(p)
        if radius == r_max:
            assert (u <= t).sum() > 100 and (u > t).sum() > 100 and (u == t).any()
            assert ((u <= t) != (f <= t)).any()
        else:
            assert (u > t).sum() > 100 and (u <= t).sum() > 100 and (u == t).any()
            assert ((u > t) != (f > t)).any()
        clouds.append(p)
    f32 = np.float32
    zs = []
    for z in (z_min, z_max):
        zs += [np.nextafter(f32(z), f32(-np.inf)), f32(z), np.nextafter(f32(z), f32(np.inf))]
    edge = [(10.0, 0.5 * i, float(z)) for i, z in enumerate(zs)]
    edge += [(15.0, 20.0, 0.0), (7.0, -24.0, 0.0), (-25.0, 0.0, 0.0), (-20.0, 15.0, 0.0), (0.0, -25.0, 0.0)]    # r2 == 625: kept
    edge += [(3.0, 0.0, 0.0), (0.0, -3.0, 0.0), (1.0, 2.0, -2.0), (-2.0, 2.0, 1.0)]                            # r2 == 9: dropped
    edge = np.asarray(edge, np.float32)
    keep = plain_crop_keep(edge, CROP)
    assert keep.tolist() == [False, True, True, True, True, False] + [True] * 5 + [False] * 4
    u = _r2_unfused(edge)
    assert (u[6:11] == f32(625.0)).all() and (u[11:] == f32(9.0)).all()
    clouds.append(edge)
    clouds = [np.concatenate([c, rng.uniform(-1, 1, (len(c), 1)).astype(np.float32)], 1) for c in clouds]
    return [Batch(clouds, 0.3, CROP, 4096, "faces")]


def crop_removes_all():
    """The crop leaves one cloud of three, then every cloud, without survivors: the min bound stays +inf and no voxel claims the
    cloud's first ordinal."""
    rng = np.random.default_rng(600)
    inside = lambda n: _cloud(rng, n, 3, -1.5, 1.5)               # r2 <= 6.75 < r_min^2: all cropped
    ring = _cloud(rng, 900, 3, -20.0, 20.0)
    ring[:, 2] = rng.uniform(-2.0, 1.5, 900)
    ring2 = ring[::-1] * np.float32(0.5)
    out = [Batch([ring, inside(500), ring2.copy()], 0.8, CROP, 900, "one"),
           Batch([inside(500), inside(1), inside(1025)], 0.8, CROP, 1025, "every")]
    assert [int(plain_crop_keep(c, CROP).sum()) > 0 for c in out[0].clouds] == [True, False, True]
    assert not any(plain_crop_keep(c, CROP).any() for c in out[1].clouds)
    return out


def cap_overflow():
    """cap = half the voxel count of the largest cloud: rows beyond cap are dropped, counts reports the full number."""
    rng = np.random.default_rng(700)
    clouds = [_cloud(rng, n, 4, -4.0, 4.0) for n in (3000, 40, 1500)]
    n_vox = [len(set(plain_voxel_index(c, 0.5)[1])) for c in clouds]
    cap = n_vox[0] // 2
    assert n_vox[0] == max(n_vox) and n_vox[1] < cap < n_vox[2] < n_vox[0], (n_vox, cap)
    return [Batch(clouds, 0.5, None, cap, "half")]


def index_range():
    """Index 2^18 - 1 on each axis is accepted; index 2^18, +inf and NaN (without a crop) are refused, never dropped or aliased; the
    NaN cloud with a crop is accepted (NaN fails the crop's comparisons)."""
    v = 0.5
    rng = np.random.default_rng(800)
    base = _cloud(rng, 64, 3, -2.0, 2.0)

    def far(axis, steps):
        c = np.concatenate([base, base[:2]])
        c[64] = 0.0
        c[65] = 0.0
        c[64, axis] = base[:, axis].min()
        c[65, axis] = np.float32(np.float64(c[64, axis]) + steps * v)
        return c

    ok = [far(a, 262143.2) for a in range(3)]
    for a, c in enumerate(ok):
        assert max(t[a] for t in plain_voxel_index(c, v)[1]) == INDEX_LIMIT - 1
    out = [Batch(ok, v, None, 66, "last index")]
    for a in range(3):
        clouds = [base.copy(), far(a, 262144.2), base.copy()]
        out.append(Batch(clouds, v, None, 66, f"axis{a} index 2^18", refused=(1, 65, a)))
    inf = base.copy()
    inf[7, 1] = np.inf
    nan = base.copy()
    nan[9, 2] = np.nan
    out.append(Batch([base.copy(), np.zeros((0, 3), np.float32), inf], v, None, 64, "+inf", refused=(2, 7, 1)))
    out.append(Batch([nan, base.copy()], v, None, 64, "nan", refused=(0, 9, 2)))
    wide = (0.0, 25.0, -2.5, 2.5)
    assert plain_crop_keep(nan, wide).sum() == 63
    out.append(Batch([nan, base.copy()], v, wide, 64, "nan cropped"))
    return out


def many_clouds(clouds: int = MAX_CLOUDS):
    """1000 clouds of 3 to 5 points, each about its own offset: cloud indices of 512 and more set the top bit of the packed key."""
    rng = np.random.default_rng(900)
    out = []
    for c in range(clouds):
        p = _cloud(rng, 3 + c % 3, 3, -0.3, 0.3)
        p[:, :3] += np.float32(c * 0.37 - 150.0)
        out.append(p)
    return [Batch(out, 0.2, None, 5, f"{clouds} clouds")]


CASES = {f.__name__: functools.lru_cache(maxsize=None)(f) for f in
         (signs_and_strides, empty_members, one_voxel, voxel_faces, crop_faces, crop_removes_all, cap_overflow, index_range,
          many_clouds)}


def batches(accepted: bool = True):
    """(case name, Batch) of every batch the rule accepts (or refuses)."""
    return [(name, b) for name, build in CASES.items() for b in build() if (b.refused is None) == accepted]


# resample: the counts a cloud can have relative to k and the buffer's capacity
RESAMPLE_KS = (1, 7, 300)
RESAMPLE_SEEDS = (0, 1234, 2 ** 63, 2 ** 64 - 1)
RESAMPLE_CLOUDS = (0, 1, 999)


def resample_counts(k: int, cap: int):
    """0, 1, k - 1, k, k + 1, cap and cap + 5 (more voxels than the buffer holds: the kernel clamps to cap)."""
    return [max(0, n) for n in (0, 1, k - 1, k, k + 1, cap, cap + 5)]
