"""csrc/preprocess.hip and csrc/resample.hip (crop, voxel average, resample) against oracle/preprocess.py, bit for bit, at the edges that
tests/preprocess_cases.py builds: strides 3 to 16, clouds of 0 / 1 / 2 / 1025 points, one voxel holding a whole cloud, points on
voxel faces and on the crop's thresholds, a crop that leaves nothing, cap below the voxel count, the last representable voxel index
and the first unrepresentable one, non-finite coordinates, 1000 clouds in one call.  tests/test_preprocess_host.py holds the oracle
to the plain reference on the same inputs.  Integer work and float64 sums in a fixed order: no tolerance anywhere."""
import numpy as np
import pytest
import torch

import preprocess_cases as P
from oracle.preprocess import preprocess, resample, voxel_downsample

pytestmark = pytest.mark.gpu

_ACCEPTED = P.batches(True)
_REFUSED = P.batches(False)


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(feat_len=3), 0, max_points=8192, max_pairs=4)
    yield e
    e.close()


def _dev(clouds):
    return [torch.from_numpy(c).to("cuda:0") for c in clouds]


def _check_voxels(eng, batch):
    """counts and the first min(count, cap) rows equal the oracle's, and a second call returns the same bits."""
    vox, counts = eng.voxel_downsample(_dev(batch.clouds), batch.voxel, batch.crop, cap=batch.cap)
    vox, counts = vox.cpu().numpy(), counts.cpu().numpy()
    assert vox.shape == (len(batch.clouds), batch.cap, batch.clouds[0].shape[1])
    refs = [voxel_downsample(c, batch.voxel, batch.crop) for c in batch.clouds]
    for i, ref in enumerate(refs):
        assert counts[i] == len(ref), (batch.label, i, int(counts[i]), len(ref))
        m = min(len(ref), batch.cap)
        assert np.array_equal(vox[i, :m], ref[:m]), (batch.label, i)
    vox2, counts2 = eng.voxel_downsample(_dev(batch.clouds), batch.voxel, batch.crop, cap=batch.cap)
    assert np.array_equal(counts2.cpu().numpy(), counts)
    for i, ref in enumerate(refs):
        m = min(len(ref), batch.cap)
        assert vox2[i, :m].cpu().numpy().tobytes() == vox[i, :m].tobytes(), (batch.label, i)
    return vox, counts, refs


@pytest.mark.parametrize("name,batch", _ACCEPTED, ids=[f"{n}-{b.label}" for n, b in _ACCEPTED])
def test_voxel_downsample_equals_oracle(eng, name, batch):
    _check_voxels(eng, batch)


def test_cap_below_the_voxel_count(eng):
    (batch,) = P.CASES["cap_overflow"]()
    vox, counts, refs = _check_voxels(eng, batch)
    assert counts[0] > batch.cap and counts[2] > batch.cap and counts[1] < batch.cap          # the full count, not min(count, cap)
    dv, dc = torch.from_numpy(vox).to("cuda:0"), torch.from_numpy(counts).to("cuda:0")
    for mode in ("random", "fixed"):
        for k in (batch.cap - 1, batch.cap + 300):
            out = eng.resample(dv, dc, k, seed=77, mode=mode).cpu().numpy()
            for i, ref in enumerate(refs):
                assert np.array_equal(out[i], resample(ref[:batch.cap], k, i, 77, mode)), (mode, k, i)


def _stride4(eng):
    batch = P.CASES["signs_and_strides"]()[1]
    assert batch.label == "stride4"
    _check_voxels(eng, batch)


@pytest.mark.parametrize("name,batch", _REFUSED, ids=[f"{n}-{b.label}" for n, b in _REFUSED])
def test_unkeyable_points_are_refused(eng, name, batch):
    from deepsir_amd.engine import EngineError
    cloud, row, _ = batch.refused
    with pytest.raises(EngineError, match=rf"cloud {cloud} row {row} .*voxel index outside \[0, 2\^18\).*not finite"):
        eng.voxel_downsample(_dev(batch.clouds), batch.voxel, batch.crop, cap=batch.cap)
    _stride4(eng)


def test_1001_clouds_are_refused(eng):
    from deepsir_amd.engine import EngineError
    (batch,) = P.many_clouds(P.MAX_CLOUDS + 1)
    assert len(batch.clouds) == 1001
    with pytest.raises(EngineError, match="1001 clouds"):
        eng.voxel_downsample(_dev(batch.clouds), batch.voxel, batch.crop, cap=batch.cap)
    _stride4(eng)


def _check_resample(eng, clouds, cap, k, stride, seeds):
    """A hand-built [clouds, cap, stride] buffer of distinct rows; cloud c of pass p has count menu[(p * clouds + c) % 7], so that with
    three clouds three passes use every count and with 1000 every count meets cloud indices on both sides of 512."""
    rng = np.random.default_rng(clouds * 31 + k)
    menu = P.resample_counts(k, cap)
    for p in range(-(-len(menu) // clouds)):
        table = rng.uniform(-9, 9, (clouds, cap, stride)).astype(np.float32)
        counts = np.array([menu[(p * clouds + c) % len(menu)] for c in range(clouds)], np.int32)
        dv, dc = torch.from_numpy(table).to("cuda:0"), torch.from_numpy(counts).to("cuda:0")
        for mode in ("random", "fixed"):
            for seed in seeds:
                out = eng.resample(dv, dc, k, seed=seed, mode=mode).cpu().numpy()
                assert out.shape == (clouds, k, stride)
                for c in range(clouds):
                    n = min(int(counts[c]), cap)
                    assert np.array_equal(out[c], resample(table[c, :n], k, c, seed & (2 ** 64 - 1), mode)), (mode, seed, c, n)
                    if n == 0:
                        assert not out[c].any()


_SEEDS = P.RESAMPLE_SEEDS + (-1,)


@pytest.mark.parametrize("stride", [3, 6])
@pytest.mark.parametrize("k", P.RESAMPLE_KS)
def test_resample_three_clouds(eng, k, stride):
    _check_resample(eng, 3, k + 3, k, stride, _SEEDS)


@pytest.mark.parametrize("stride", [3, 6])
@pytest.mark.parametrize("k", P.RESAMPLE_KS)
def test_resample_thousand_clouds(eng, k, stride):
    _check_resample(eng, 1000, 8, k, stride, _SEEDS)


@pytest.mark.parametrize("counts", [(0, 1, 8), (5, 8, 9)])
@pytest.mark.parametrize("stride", [3, 6])
def test_both_resample_entries_share_one_body(eng, stride, counts):
    """dsir_resample and dsir_t_resample_keyed run the same two kernels (csrc/resample.hip) with different draws: the engine's entry
    in both modes against the oracle, the loader's entry in its three modes against augment.resample_rows, at 3 clouds of cap 8 with
    an empty cloud, a single row, a full cloud and a count above cap, k below, at and above the counts."""
    from deepsir_amd import augment as A
    cap, seed, epoch, indices = 8, 11, 4, [5, 900, 10 ** 9]
    table = np.random.default_rng(stride * 10 + counts[0]).uniform(-9, 9, (3, cap, stride)).astype(np.float32)
    dv, dc = torch.from_numpy(table).to("cuda:0"), torch.tensor(counts, dtype=torch.int32, device="cuda:0")
    live = [min(n, cap) for n in counts]
    cfgs = {A.RESAMPLE_RANDOM: A.AugmentConfig(variant="v1", fixed=False), A.RESAMPLE_FIXED: A.AugmentConfig(variant="v1", fixed=True),
            A.RESAMPLE_PERMUTED_FIXED: A.AugmentConfig(variant="v2", permute=True)}
    assert sorted(cfgs) == [0, 1, 2]
    for k in (1, 5, 8, 11):
        for mode in ("random", "fixed"):
            out = eng.resample(dv, dc, k, seed=seed, mode=mode).cpu().numpy()
            for c in range(3):
                assert np.array_equal(out[c], resample(table[c, :live[c]], k, c, seed, mode)), (k, mode, c)
        for rmode, cfg in cfgs.items():
            src, ref, _, _, rows_s, rows_r = eng.augment(dv, dc, dv, dc, None, cfg, seed, epoch, indices, k, return_rows=True)
            for side, (pts, rows) in enumerate(((src, rows_s), (ref, rows_r))):
                pts, rows = pts.cpu().numpy(), rows.cpu().numpy()
                for c in range(3):
                    prm = A.pair_params(cfg, seed, epoch, indices[c])[side]
                    assert prm.resample_mode == rmode
                    want = A.resample_rows(prm.key, live[c], k, rmode)
                    assert np.array_equal(rows[c], want), (k, rmode, side, c)
                    if live[c] == 0:
                        assert not pts[c].any()
                    else:
                        assert np.array_equal(pts[c][:, 3:], table[c][want][:, 3:]), (k, rmode, side, c)    # untouched columns


@pytest.mark.parametrize("name", ["empty_members", "crop_removes_all"])
def test_preprocess_end_to_end(eng, name):
    for batch in P.CASES[name]():
        for mode in ("random", "fixed"):
            out, counts = eng.preprocess(_dev(batch.clouds), batch.voxel, 96, seed=5, crop=batch.crop, mode=mode)
            ref, n_ref = preprocess(batch.clouds, batch.voxel, 96, 5, batch.crop, mode)
            assert counts.cpu().numpy().tolist() == n_ref, (batch.label, mode)
            assert np.array_equal(out.cpu().numpy(), ref), (batch.label, mode)
