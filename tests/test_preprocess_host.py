"""oracle/preprocess.py against the plain reference of tests/preprocess_cases.py, bit for bit, on every edge case the device test
(tests/test_gpu_preprocess_edges.py) runs: the oracle is what csrc/preprocess.hip is held to, so it is held to the written rule
here.  Runs without a GPU.  The case builders' own assertions (the float32 face-flip share, "a fused crop differs", ...) run with
their first use."""
import numpy as np
import pytest

import preprocess_cases as P
from oracle.preprocess import crop_mask, resample, voxel_downsample

_ACCEPTED = P.batches(True)
_REFUSED = P.batches(False)


@pytest.mark.parametrize("name", list(P.CASES))
def test_case_builders_hold_their_own_assertions(name):
    for b in P.CASES[name]():
        assert all(c.dtype == np.float32 and c.ndim == 2 and len(c) <= 4096 for c in b.clouds)
        assert sum(len(c) for c in b.clouds) <= 20000 and len({c.shape[1] for c in b.clouds}) == 1


@pytest.mark.parametrize("name,batch", _ACCEPTED, ids=[f"{n}-{b.label}" for n, b in _ACCEPTED])
def test_oracle_voxel_downsample_equals_plain(name, batch):
    for i, c in enumerate(batch.clouds):
        assert np.array_equal(crop_mask(c, batch.crop), P.plain_crop_keep(c, batch.crop)), i
        got, want = voxel_downsample(c, batch.voxel, batch.crop), P.plain_voxel_downsample(c, batch.voxel, batch.crop)
        assert got.dtype == np.float32 and got.shape == want.shape, (i, got.shape, want.shape)
        assert np.array_equal(got, want), i


@pytest.mark.parametrize("name,batch", _REFUSED, ids=[f"{n}-{b.label}" for n, b in _REFUSED])
def test_unkeyable_points_are_refused_by_both(name, batch):
    cloud, row, axis = batch.refused
    for i, c in enumerate(batch.clouds):
        if i != cloud:
            assert np.array_equal(voxel_downsample(c, batch.voxel, batch.crop), P.plain_voxel_downsample(c, batch.voxel, batch.crop))
            continue
        with pytest.raises(ValueError, match=f"row {row} axis {axis}"):
            P.plain_voxel_downsample(c, batch.voxel, batch.crop)
        with pytest.raises(ValueError, match=f"row {row} axis {axis}"):
            voxel_downsample(c, batch.voxel, batch.crop)


@pytest.mark.parametrize("mode", ["random", "fixed"])
@pytest.mark.parametrize("k", P.RESAMPLE_KS)
def test_oracle_resample_equals_plain(k, mode):
    rng = np.random.default_rng(k)
    for n in sorted({0, 1, max(0, k - 1), k, k + 1}):
        pts = rng.uniform(-5, 5, (n, 4)).astype(np.float32)
        for cloud in P.RESAMPLE_CLOUDS:
            for seed in P.RESAMPLE_SEEDS:
                got, want = resample(pts, k, cloud, seed, mode), P.plain_resample(pts, k, cloud, seed, mode)
                assert got.shape == (k, 4) and np.array_equal(got, want), (n, cloud, seed)


def test_resample_keys_depend_on_cloud_and_seed():
    """The cases above would pass a resampler that ignored ``cloud`` or ``seed`` if the plain one ignored them too: they matter."""
    pts = np.arange(40, dtype=np.float32).reshape(20, 2)
    base = P.plain_resample(pts, 30, 0, 0)
    for cloud, seed in ((1, 0), (999, 0), (0, 1234), (0, 2 ** 63), (0, 2 ** 64 - 1)):
        other = P.plain_resample(pts, 30, cloud, seed)
        assert not np.array_equal(other[:20], base[:20]) and not np.array_equal(other[20:], base[20:]), (cloud, seed)
    assert np.array_equal(P.plain_resample(pts, 30, 3, -1), P.plain_resample(pts, 30, 3, 2 ** 64 - 1))
