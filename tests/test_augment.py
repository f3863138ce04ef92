"""The augmentation rule on the host (deepsir_amd/augment.py: the restatement csrc/augment.hip is compared against in
tests/test_gpu_train_data.py) and the train / val pair selection of deepsir_amd/data.py.  No GPU."""
import os
import pickle

import numpy as np
import pytest

from deepsir_amd import augment as A
from deepsir_amd import data as D


def test_counter_key_known_answers():
    # splitmix64 reference vectors (Vigna's generator seeded with 0: the first outputs are sm(0), sm-chain of the state increments)
    assert A.splitmix64(0) == 0xE220A8397B1DCDAF
    assert A.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert int(A.splitmix64(np.array([0], np.uint64))[0]) == 0xE220A8397B1DCDAF
    # the key chain and a draw, spelled out
    k = A.splitmix64(A.splitmix64(A.splitmix64(A.splitmix64(7) ^ 3) ^ 11) ^ 1)
    assert A.cloud_key(7, 3, 11, 1) == k
    d = A.draws(k, A.STREAM_JITTER, [5, 6])
    assert int(d[0]) == A.splitmix64(k ^ (3 << 40) ^ 5) and int(d[1]) == A.splitmix64(k ^ (3 << 40) ^ 6)
    u = A.uniform(k, A.STREAM_JITTER, [5])
    assert u[0] == (int(d[0]) >> 11) * 2.0 ** -53 and 0.0 <= u[0] < 1.0
    # every field of the key matters; the batch position is not a field at all
    keys = {A.cloud_key(*a) for a in [(7, 3, 11, 1), (8, 3, 11, 1), (7, 4, 11, 1), (7, 3, 12, 1), (7, 3, 11, 0), (3, 7, 11, 1)]}
    assert len(keys) == 6


V1 = A.AugmentConfig(variant="v1", num_points=512)
V2 = A.AugmentConfig(variant="v2", num_points=512, random_scale=False, xy_rot_scale=0.1)


def _angle(R):
    return np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))


def test_rotations_are_proper_and_in_range():
    for i in range(300):
        for cfg in (V1, V2, A.AugmentConfig(variant="v2", xy_rot_scale=1.0, rot_mag=170.0)):
            for p in A.pair_params(cfg, 5, 1, i):
                assert np.abs(p.R @ p.R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(p.R) - 1.0) < 1e-12
        ps, pr = A.pair_params(V1, 5, 1, i)
        assert _angle(ps.R) <= 45.0 + 1e-9 and _angle(pr.R) <= 45.0 + 1e-9 and ps.centered and pr.centered
        # v2: the ref cloud turns about z by [0, 60) degrees; the src adds Rx Ry Rz with the x / y angles discounted
        ps, pr = A.pair_params(V2, 5, 1, i)
        a = np.degrees(np.arctan2(pr.R[1, 0], pr.R[0, 0]))
        assert 0.0 <= a < 60.0 and np.abs(pr.R[2] - [0, 0, 1]).max() == 0.0 and not pr.centered and np.all(pr.t == 0)
        u = A.uniform(ps.key, A.STREAM_PARAM, np.arange(11))
        ang = u[5:8] * np.pi * 45.0 / 180.0 * np.array([0.1, 0.1, 1.0])
        assert (ang >= 0).all() and ang[0] < np.pi / 40 and ang[1] < np.pi / 40 and ang[2] < np.pi / 4
        np.testing.assert_allclose(ps.R, A.euler_xyz(*ang) @ A.rot_z(u[4] * np.pi / 3), atol=1e-15)
        assert np.abs(ps.t).max() <= 2.0
        # xy_rot_scale = 0: a pure z rotation
        p0, _ = A.pair_params(A.AugmentConfig(variant="v2", xy_rot_scale=0.0), 5, 1, i)
        assert np.abs(p0.R[2] - [0, 0, 1]).max() < 1e-15 and np.abs(p0.R[:, 2] - [0, 0, 1]).max() < 1e-15


def test_rodrigues_equals_the_matrix_exponential():
    rng = np.random.default_rng(0)
    for _ in range(20):
        ax, th = rng.random(3) - 0.5, (rng.random() - 0.5) * np.pi / 2
        K = np.cross(np.eye(3), ax / np.linalg.norm(ax) * th)        # data_base.py:394
        E, term = np.eye(3), np.eye(3)
        for n in range(1, 30):                                      # expm by its series: |K| < 1
            term = term @ K / n
            E = E + term
        np.testing.assert_allclose(A.rodrigues(ax, th), E, atol=1e-14)


def test_jitter_distributions():
    k = A.cloud_key(1, 2, 3, 0)
    u = A.jitter(k, 40000, A.JITTER_UNIFORM, 0.005, 0.0)
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 0.005 and abs(u.mean() - 0.0025) < 5e-5
    g = A.jitter(k, 34000, A.JITTER_NORMAL, 0.01, 0.05)             # > 1e5 draws
    assert np.abs(g).max() <= np.float32(0.05) and abs(g.mean()) < 1e-4 and abs(g.std() - 0.01) < 1e-4
    # the clip is reached with sigma large enough, and never passed
    c = A.jitter(k, 1000, A.JITTER_NORMAL, 0.05, 0.05)
    assert np.abs(c).max() == np.float32(0.05) and (np.abs(c) == np.float32(0.05)).mean() > 0.2
    assert not A.jitter(k, 7, A.JITTER_NONE, 1.0, 1.0).any()


def test_gates_and_scale():
    jit = sc = 0
    for i in range(10000):
        ps, pr = A.pair_params(V1, 9, 0, i)
        jit += ps.jitter_mode == A.JITTER_UNIFORM
        sc += ps.scaled
        assert ps.jitter_mode == pr.jitter_mode and ps.scaled == pr.scaled and ps.scale == pr.scale     # one draw per pair
        assert (0.8 <= ps.scale <= 1.2) if ps.scaled else ps.scale == 1.0
    for n in (jit, sc):                        # binomial(1e4, 0.95): sigma = 21.8; 5 sigma
        assert abs(n - 9500) < 110
    # v2 has no gate: jitter always, in its own mode
    ps, _ = A.pair_params(V2, 9, 0, 1)
    assert ps.jitter_mode == A.JITTER_NORMAL and not ps.scaled and ps.resample_mode == A.RESAMPLE_PERMUTED_FIXED


def test_resample_rows():
    k = A.cloud_key(4, 0, 2, 1)
    r = A.resample_rows(k, 100, 40, A.RESAMPLE_RANDOM)
    assert len(set(r)) == 40 and r.max() < 100                      # n > k: no repeats
    r = A.resample_rows(k, 30, 100, A.RESAMPLE_RANDOM)
    assert sorted(r[:30]) == list(range(30)) and r.max() < 30       # n < k: every point, then a top-up
    assert np.array_equal(A.resample_rows(k, 30, 70, A.RESAMPLE_FIXED), np.arange(70) % 30)
    r = A.resample_rows(k, 30, 70, A.RESAMPLE_PERMUTED_FIXED)
    assert sorted(r[:30]) == list(range(30)) and np.array_equal(r[30:60], r[:30]) and np.array_equal(r[60:], r[:10])
    assert np.array_equal(r[:20], A.resample_rows(k, 30, 20, A.RESAMPLE_PERMUTED_FIXED))               # permutation, then prefix


def _rigid(rng):
    M = np.eye(4)
    M[:3, :3] = A.rodrigues(rng.random(3) - 0.5, 0.7)
    M[:3, 3] = rng.random(3) * 2 - 1
    return M


@pytest.mark.parametrize("variant", ["v1", "v2"])
@pytest.mark.parametrize("scaled", [False, True])
def test_ground_truth_maps_src_onto_ref(variant, scaled):
    """ref = M src in the same order; no jitter; the same rows on both sides (fixed resampling): transform_gt src_aug = ref_aug."""
    rng = np.random.default_rng(3)
    src = (rng.random((700, 3)) * [8, 6, 3] + [20, -10, 1]).astype(np.float32)
    M = _rigid(rng)
    ref = (src.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    cfg = A.AugmentConfig(variant=variant, num_points=700, fixed=True, random_jitter=False, random_scale=scaled, gate=1.0)
    extent = float(np.abs(ref).max())
    for idx in range(5):
        out = A.augment_pair(src, ref, M, cfg, 2, 0, idx)
        ps, pr = out["params"]
        if variant == "v2":                                         # the loader's permutation differs per side: undo it
            s_, r_ = out["points_src"][np.argsort(out["rows_src"])], out["points_ref"][np.argsort(out["rows_ref"])]
        else:
            s_, r_ = out["points_src"], out["points_ref"]
        T = out["transform_gt"].astype(np.float64)
        assert out["transform_gt"].dtype == np.float32 and out["transform_gt"].shape == (3, 4)
        assert ps.scaled == scaled
        err = np.abs(s_.astype(np.float64) @ T[:, :3].T + T[:, 3] - r_).max()
        assert err < 1e-5 * extent, err
        if scaled:                                                  # the reference leaves the translation unscaled
            cfg_r = A.AugmentConfig(**{**cfg.__dict__, "reference_gt": True})
            Tr = A.augment_pair(src, ref, M, cfg_r, 2, 0, idx)["transform_gt"].astype(np.float64)
            np.testing.assert_allclose(Tr[:, :3], T[:, :3], atol=1e-7)
            np.testing.assert_allclose(Tr[:, 3] * ps.scale, T[:, 3], rtol=1e-6, atol=1e-6)
            assert abs(ps.scale - 1.0) > 1e-3
            if np.abs(T[:, 3]).max() > 0.1:                         # (about the centroids of a rigid copy the translation is ~0)
                assert np.abs(s_.astype(np.float64) @ Tr[:, :3].T + Tr[:, 3] - r_).max() > 1e-3
            else:
                assert variant == "v1"


def test_samples_depend_on_seed_epoch_index_only():
    rng = np.random.default_rng(4)
    clouds = [rng.standard_normal((300 + 17 * i, 3)).astype(np.float32) for i in range(6)]
    cfg = A.AugmentConfig(variant="v1", num_points=256)

    def sample(seed, epoch, idx):
        o = A.augment_pair(clouds[idx], clouds[(idx + 1) % 6], np.eye(4), cfg, seed, epoch, idx)
        return o["points_src"].tobytes() + o["points_ref"].tobytes() + o["transform_gt"].tobytes()
    a = sample(1, 0, 2)
    assert a == sample(1, 0, 2)
    assert a != sample(1, 1, 2) and a != sample(2, 0, 2)
    # "batches" are only a grouping of indices: whichever batch index 2 lands in, and at whatever position, it is `a`
    for batch in ([0, 1, 2, 3], [2, 5], [4, 2]):
        assert [sample(1, 0, i) for i in batch][batch.index(2)] == a
    # the epoch's order: a permutation, the same for the same (seed, epoch), another for another epoch
    o0, o1 = A.epoch_order(1, 0, 50), A.epoch_order(1, 1, 50)
    assert sorted(o0) == list(range(50)) and np.array_equal(o0, A.epoch_order(1, 0, 50)) and not np.array_equal(o0, o1)
    assert np.array_equal(A.epoch_order(1, 0, 50, shuffle=False), np.arange(50))


def test_invalid_clouds_and_untouched_columns():
    rng = np.random.default_rng(5)
    ps, _ = A.pair_params(V1, 0, 0, 0)
    out, rows, inv, _ = A.augment_cloud(np.zeros((0, 4), np.float32), ps, 16)
    assert inv == A.INVALID_EMPTY and out.shape == (16, 4) and not out.any()
    bad = rng.standard_normal((20, 3)).astype(np.float32)
    bad[7, 1] = np.nan
    assert A.augment_cloud(bad, ps, 16)[2] == A.INVALID_NONFINITE
    # [x, y, z, reflectance, label, 0]: columns 3:6 ride through unless they are declared normals
    six = np.concatenate([rng.standard_normal((50, 3)), rng.random((50, 1)), rng.integers(0, 19, (50, 2))], 1).astype(np.float32)
    out, rows, inv, _ = A.augment_cloud(six, ps, 64)
    assert inv == 0 and np.array_equal(out[:, 3:], six[rows][:, 3:])
    pn = A.pair_params(A.AugmentConfig(variant="v1", normals=True), 0, 0, 0)[0]
    outn = A.augment_cloud(six, pn, 64)[0]
    np.testing.assert_allclose(outn[:, 3:6], six[rows][:, 3:6] @ pn.R.T.astype(np.float32), atol=1e-4)
    assert np.array_equal(outn[:, :3], out[:, :3])


# ------------------------------------------------------------------------------------------------ pair selection
def test_threedmatch_overlap_selection(tmp_path):
    rng = np.random.default_rng(6)
    ids = [f"scene{s}/cloud_bin_{i}" for s in range(2) for i in range(4)]
    pts = {k: rng.random((50, 3)).astype(np.float32) for k in ids}
    ovl = {f"{a}@{b}": float(v) for a, b, v in [(ids[0], ids[1], 0.5), (ids[0], ids[2], 0.3), (ids[1], ids[3], 0.31), (ids[4], ids[5], 0.1),
                                               (ids[6], ids[4], 0.9), (ids[7], ids[5], 0.30000001)]}
    for split in ("train", "val"):
        d = tmp_path / "3dmatch_train_val"
        os.makedirs(d, exist_ok=True)
        pickle.dump(pts, open(d / f"3DMatch_{split}_0.030_points.pkl", "wb"))
        pickle.dump(ovl, open(d / f"3DMatch_{split}_0.030_overlap.pkl", "wb"))
    # threeDMatch_loader.py:110-115, line by line
    want = []
    for idpair in ovl.keys():
        src_idx, ref_idx = idpair.split("@")
        if ovl[idpair] > 0.3:
            want.append((src_idx, ref_idx))
    ds = D.ThreeDMatchTrain(str(tmp_path), None, "train")
    assert ds.files == want and len(want) == 4
    src, ref, M, others = ds.raw(2)
    assert np.array_equal(src, pts[ids[6]]) and np.array_equal(ref, pts[ids[4]]) and np.array_equal(M, np.eye(4))
    assert others == {"seq": "scene1", "id_ref": 0, "id_src": 2}
    assert ds.augment_cfg.random_jitter and ds.augment_cfg.random_scale and ds.augment_cfg.random_rotation
    val = D.ThreeDMatchTrain(str(tmp_path), None, "val", num_val=3)
    assert val.files == want[:3]
    c = val.augment_cfg                                             # :62-65: val keeps the rotation only
    assert c.random_rotation and not c.random_jitter and not c.random_scale
    assert ds.match_radius == pytest.approx(0.09)
    with pytest.raises(FileNotFoundError):
        D.ThreeDMatchTrain(str(tmp_path / "nowhere"), None, "train")


def _fake_kitti(root, drive, ids, step=1.0):
    seq = os.path.join(root, "dataset", "sequences", "%02d" % drive, "velodyne")
    os.makedirs(seq, exist_ok=True)
    os.makedirs(os.path.join(root, "dataset", "poses"), exist_ok=True)
    for t in ids:
        np.zeros((1, 4), np.float32).tofile(os.path.join(seq, "%06d.bin" % t))
    poses = []
    for t in range(max(ids) + 1):
        T = np.eye(4)
        T[2, 3] = step * t
        poses.append(T[:3].reshape(-1))
    np.savetxt(os.path.join(root, "dataset", "poses", "%02d.txt" % drive), np.array(poses))


def test_kitti_train_and_val_selection(tmp_path):
    root = str(tmp_path)
    ids = {0: [0, 1, 2, 3, 5, 6, 8, 9, 10], 1: [0, 1, 2, 3, 4], 6: list(range(40))}
    for drive, names in ids.items():
        _fake_kitti(root, drive, names)
    # kitti_loader.py:80-96, line by line
    MIN_TIME_DIFF, MAX_TIME_DIFF = 2, 3
    want = []
    for drive_id in (0, 1):
        inames = ids[drive_id]
        if (drive_id == 1) and (MAX_TIME_DIFF - 1) > MIN_TIME_DIFF:
            max_time_diff = MAX_TIME_DIFF - 1
        else:
            max_time_diff = MAX_TIME_DIFF
        for start_time in inames:
            for time_diff in range(MIN_TIME_DIFF, max_time_diff):
                pair_time = time_diff + start_time
                if pair_time in inames:
                    want.append((drive_id, start_time, pair_time))
    ds = D.KittiOdometryTrain(root, None, "train", sequences=[0, 1])
    assert ds.files == want and (0, 3, 5) in want and (0, 5, 7) not in want and (1, 2, 4) in want
    c = ds.augment_cfg
    assert c.variant == "v2" and c.random_rotation and c.random_jitter and not c.random_scale and c.xy_rot_scale == 0.1
    # val: the >= 10 m selection of the test split on the val sequences, no rotation, no jitter
    val = D.KittiOdometryTrain(root, None, "val", sequences=[6], num_val=2)
    test = D.KittiOdometryTest(root, None, sequences=[6])
    assert val.files == test.files[:2] and len(test.files) > 2 and val.files[0] == (6, 0, 10)
    assert not val.augment_cfg.random_rotation and not val.augment_cfg.random_jitter
    assert ds.match_radius == pytest.approx(0.9) and ds.label_col == 4 and ds.crop == (3.0, 60.0, -3.0, 10.0)
