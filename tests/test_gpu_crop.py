"""`Engine.halfspace_crop` (csrc/crop.hip) against the host rule `crop.halfspace_crop_host`, bit for bit on rows, counts and invalid
bits: ragged sizes across the wave, the workgroup and the 2048-row slice, projections built to hit every digit of the select."""
import numpy as np
import pytest
import torch

from deepsir_amd import augment as A
from deepsir_amd import crop as K

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 40000, 2049]       # 16 clouds; 40000 rows = 20 slices
P_KEEPS = [0.5, 0.6, 0.7, 0.999, 1.0, 1e-4]
SEED, EPOCH = 11, 3


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), 0, max_points=2048, max_pairs=1)
    yield e
    e.close()


def _lattice_cloud(rng, n, stride):
    """Coordinates on a 1/64 lattice inside +-64: every float64 partial sum is exact, so the centroid is the same number in any
    order of summation and the device's projections are the host's bit for bit."""
    pts = np.zeros((n, stride), np.float32)
    pts[:, :3] = rng.integers(-4096, 4097, (n, 3)).astype(np.float32) / 64.0
    if stride > 3:
        pts[:, 3:] = rng.random((n, stride - 3)).astype(np.float32)
    return pts


def _padded(clouds, stride):
    """[clouds][cap][stride] with rows past the count that must never be read as data."""
    cap = max(1, max(len(c) for c in clouds))
    buf = np.full((len(clouds), cap, stride), 1e30, np.float32)
    for i, c in enumerate(clouds):
        buf[i, :len(c)] = c
    return buf, np.array([len(c) for c in clouds], np.int32)


def _device(eng, clouds, stride, p_keep, indices, sides, directions=None, out_cap=None):
    buf, counts = _padded(clouds, stride)
    out, n, inv = eng.halfspace_crop(torch.from_numpy(buf).cuda(), torch.from_numpy(counts).cuda(), p_keep, SEED, EPOCH, indices, sides,
                                     out_cap=out_cap, directions=directions)
    torch.cuda.synchronize()
    return out.cpu().numpy(), n.cpu().numpy(), inv.cpu().numpy()


def _check(clouds, p_keep, dirs, out, n, inv, out_cap=None):
    for c, pts in enumerate(clouds):
        want, bits = K.halfspace_crop_host(pts, p_keep[c], dirs[c])
        assert int(n[c]) == len(want), (c, len(pts), p_keep[c], int(n[c]), len(want))
        assert int(inv[c]) == bits, (c, len(pts), p_keep[c])
        m = len(want) if out_cap is None else min(len(want), out_cap)
        assert out[c, :m].tobytes() == want[:m].tobytes(), (c, len(pts), p_keep[c])


@pytest.fixture(scope="module")
def ragged():
    """The ragged clouds of every stride, their p_keep and drawn directions: made once, shared, never written to."""
    rng = np.random.default_rng(5)
    indices = [100 + i for i in range(len(SIZES))]
    sides = [i % 2 for i in range(len(SIZES))]
    p_keep = [P_KEEPS[i % len(P_KEEPS)] for i in range(len(SIZES))]
    p_keep[SIZES.index(40000)] = 0.6
    p_keep[SIZES.index(4097)] = 1e-4
    dirs = K.crop_directions(SEED, EPOCH, indices, sides)
    return {s: [_lattice_cloud(rng, n, s) for n in SIZES] for s in (3, 4, 7)}, p_keep, indices, sides, dirs


@pytest.mark.parametrize("stride", [3, 4, 7])
def test_ragged_call_equals_the_host_rule(eng, ragged, stride):
    clouds, p_keep, indices, sides, dirs = ragged
    out, n, inv = _device(eng, clouds[stride], stride, p_keep, indices, sides)
    _check(clouds[stride], p_keep, dirs, out, n, inv)
    big = SIZES.index(40000)
    assert abs(int(n[big]) - 24000) <= 4                              # n - 1 - lo rows, less the ties with d_(lo)
    assert int(n[SIZES.index(4097)]) <= 1                             # p_keep 1e-4: lo = 4095, at most the largest row is above it


def _axis(xs, stride=3):
    pts = np.zeros((len(xs), stride), np.float32)
    pts[:, 0] = xs
    pts[:, 3:] = np.arange(len(xs), dtype=np.float32)[:, None]
    return pts


def _crafted():
    """(cloud, p_keep, direction) built so that the projection d = x - 0 is the stored x (symmetric clouds with exact sums) and the
    rank falls where the select can go wrong."""
    rng = np.random.default_rng(9)
    ex, cases = np.array([1.0, 0.0, 0.0], np.float32), []
    cases.append((_axis(np.full(300, 2.5, np.float32)), 0.7, ex))                                   # all equal: nothing kept
    two = np.concatenate([np.full(400, -1.5, np.float32), np.full(600, 1.0, np.float32)])           # mean 0; two distinct values
    cases.append((_axis(rng.permutation(two)), 0.7, ex))                                            # lo = 299: on the lower, keeps 600
    cases.append((_axis(rng.permutation(two)), 0.3, ex))                                            # lo = 699: on the upper, keeps 0
    low = (np.float32(1.0) + rng.integers(0, 256, 2048).astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)
    assert len(np.unique(low.view(np.uint32) >> 8)) == 1                                            # only the lowest key byte differs
    cases.append((_axis(rng.permutation(np.concatenate([low, -low]))), 0.3, ex))                    # 4096 rows: two slices, with ties
    cases.append((_axis(rng.permutation(np.concatenate([low, -low]))), 0.8, ex))
    high = (np.float32(1.25) * np.float32(2.0) ** (2 * rng.integers(-12, 13, 700))).astype(np.float32)
    assert len(np.unique(high.view(np.uint32) & 0xFFFFFF)) == 1                                      # only the highest key byte differs
    cases.append((_axis(rng.permutation(np.concatenate([high, -high]))), 0.6, ex))
    zeros = np.concatenate([np.full(100, -1.0), np.full(200, -0.0), np.full(200, 0.0), np.full(100, 1.0)]).astype(np.float32)
    cases.append((_axis(rng.permutation(zeros)), 0.6, ex))                                          # d_(lo) is a zero: no zero of either sign kept
    cases.append((_axis(rng.permutation(zeros)), 0.5, ex))
    cases.append((_axis(rng.permutation(zeros)), 0.9, ex))                                          # d_(lo) = -1: the zeros of both signs are kept
    sub = (rng.integers(1, 500, 333).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    assert (np.abs(sub) < np.finfo(np.float32).tiny).all() and (sub != 0).all()
    cases.append((_axis(rng.permutation(np.concatenate([sub, -sub]))), 0.7, ex))                    # subnormal projections
    cases.append((_axis(rng.permutation(np.concatenate([sub, -sub]))), 0.25, ex))
    nan_row = _axis(rng.standard_normal(500).astype(np.float32))
    nan_row[77, 1] = np.nan
    cases.append((nan_row, 0.6, ex))                                                                # a NaN row: the centroid is NaN
    inf_row = _axis(rng.standard_normal(500).astype(np.float32))
    inf_row[5, 2] = -np.inf
    cases.append((inf_row, 0.6, ex))
    both = _axis(rng.standard_normal(64).astype(np.float32))
    both[0, 0], both[1, 0] = np.inf, -np.inf
    cases.append((both, 1.0, ex))                                                                   # refused even where every row would be kept
    # a finite centroid under which one row's projection overflows to +Inf, and one where it is Inf - Inf = NaN: dropped, counted in n
    huge = _lattice_cloud(rng, 900, 3)
    # (the directions are the caller's numbers: 2^100 along x makes (2^30 - m) u overflow while the lattice rows stay finite and distinct)
    huge[123] = [2.0 ** 30, 2.0 ** 30, 0.0]
    cases.append((huge, 0.6, np.array([2.0 ** 100, 0.0, 0.0], np.float32)))
    cases.append((huge, 0.6, np.array([2.0 ** 100, -2.0 ** 100, 0.0], np.float32)))
    few = np.zeros((10, 3), np.float32)                                                             # 7 of 10 projections not finite: d_(lo = 3) is
    few[:7] = [2.0 ** 30, 2.0 ** 30, 0.0]                                                           # one of them -> refused
    few[7:, 0] = [1.0, 2.0, 3.0]
    cases.append((few, 0.6, np.array([2.0 ** 100, -2.0 ** 100, 0.0], np.float32)))
    return cases


def test_projections_built_to_hit_the_select(eng):
    cases = _crafted()
    clouds, p_keep, dirs = [c[0] for c in cases], [c[1] for c in cases], np.stack([c[2] for c in cases])
    out, n, inv = _device(eng, clouds, 3, p_keep, list(range(len(cases))), 0, directions=dirs)
    _check(clouds, p_keep, dirs, out, n, inv)
    assert n.tolist()[:3] == [0, 600, 0] and inv.tolist()[:3] == [A.INVALID_EMPTY, 0, A.INVALID_EMPTY]
    assert n.tolist()[6:9] == [100, 100, 500]
    assert inv.tolist()[11:14] == [A.INVALID_NONFINITE] * 3 and n.tolist()[11:14] == [0, 0, 0]
    assert int(inv[14]) == 0 and int(inv[15]) == 0 and int(inv[16]) == A.INVALID_NONFINITE and int(n[16]) == 0
    # the dropped non-finite row is absent from the output although its key is the largest
    assert n[14] > 300 and n[15] > 300
    assert not (out[15, :n[15], 0] == np.float32(2.0 ** 30)).any() and not (out[14, :n[14], 0] == np.float32(2.0 ** 30)).any()


def test_overflow_reports_the_count_and_writes_the_first_rows(eng, ragged):
    clouds, p_keep, indices, sides, dirs = ragged
    out, n, inv = _device(eng, clouds[4], 4, p_keep, indices, sides, out_cap=100)
    assert out.shape[1] == 100 and int(n.max()) > 100
    _check(clouds[4], p_keep, dirs, out, n, inv, out_cap=100)


def test_same_bytes_twice_and_alone(eng, ragged):
    clouds, p_keep, indices, sides, dirs = ragged
    a = _device(eng, clouds[7], 7, p_keep, indices, sides)
    b = _device(eng, clouds[7], 7, p_keep, indices, sides)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for c in (SIZES.index(40000), SIZES.index(1025), SIZES.index(65)):
        out, n, inv = _device(eng, [clouds[7][c]], 7, [p_keep[c]], [indices[c]], [sides[c]])
        assert int(n[0]) == int(a[1][c]) and int(inv[0]) == int(a[2][c])
        assert out[0, :n[0]].tobytes() == a[0][c, :n[0]].tobytes()


def test_refused_arguments(eng):
    from deepsir_amd.engine import EngineError
    pts, counts = torch.zeros((1, 8, 3), device="cuda"), torch.full((1,), 8, dtype=torch.int32, device="cuda")
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(EngineError):
            eng.halfspace_crop(pts, counts, bad, 0, 0, [0], 0)
    with pytest.raises(EngineError):
        eng.halfspace_crop(pts[:, :, :2], counts, 0.6, 0, 0, [0], 0)
