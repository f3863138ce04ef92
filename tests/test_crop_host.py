"""The half-space crop rule on the host (deepsir_amd/crop.py) and the host side of the Oxford loaders (deepsir_amd/data.py)."""
import logging
import os
import pickle

import numpy as np
import pytest

from deepsir_amd import augment as A
from deepsir_amd import crop as K
from deepsir_amd import data as D
from deepsir_amd.se3 import xyzquat2mat

P_KEEPS = (0.123, 0.3, 0.51, 0.6, 0.7, 0.75, 0.9, 0.999)


def test_rank_rule_against_np_percentile():
    """dist > np.percentile(dist, q) and the rank rule keep the same rows unless numpy's virtual index v lies within 1e-9 of an
    integer FROM BELOW; there numpy's interpolated threshold may round onto the next order statistic and the two differ by at most
    one row.  At or just above an integer (frac(v) < 1e-9: every n - 1 that is a multiple of 4 at p_keep = 0.75, a tenth of this
    grid) the interpolation adds at most 1e-9 of the gap to d_(lo) and stays below d_(lo+1), so equality is asserted there too.
    Inside the band a difference is one row that numpy drops and the rule keeps, nothing else.  The band itself holds 46 of this
    grid's 3200 cases by the arithmetic of v alone (39 at p_keep = 0.9, 7 at 0.3: 1.44 %), whatever the rule under test does, so the
    1 % cap on what the test may excuse is put on the cases that actually differ (0.35 % where the rule was first checked)."""
    rng = np.random.default_rng(2024)
    cases = excused = 0
    for n in range(1, 401):
        for p in P_KEEPS:
            d = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3)).astype(np.float32)
            if cases % 5 == 0 and n > 1:                                   # one case in five: duplicated projections
                d = d[rng.integers(0, max(1, n // 3), n)]
            cases += 1
            mask, _ = K.keep_mask(d, p)
            d64 = d.astype(np.float64)
            ref = d64 > np.percentile(d64, (1.0 - p) * 100)
            v = (n - 1) * (((1.0 - p) * 100) / 100)
            frac = v - np.floor(v)
            if frac <= 1.0 - 1e-9:
                assert np.array_equal(mask, ref), (n, p)
            elif not np.array_equal(mask, ref):
                excused += 1
                assert int((mask != ref).sum()) == 1 and int((mask & ~ref).sum()) == 1, (n, p)
    assert cases == 400 * len(P_KEEPS)
    print(f"cases {cases}, differing inside the band {excused}")
    assert excused < 0.01 * cases, (excused, cases)


def test_direction_is_a_unit_vector_of_the_key():
    seen = set()
    for index in range(50):
        for side in (A.SIDE_SRC, A.SIDE_REF):
            for epoch in (0, 1):
                u = K.crop_direction(A.cloud_key(7, epoch, index, side))
                assert u.dtype == np.float32 and u.shape == (3,)
                assert abs(float(np.sqrt((u.astype(np.float64) ** 2).sum())) - 1.0) <= 1e-7
                assert np.array_equal(u, K.crop_direction(A.cloud_key(7, epoch, index, side)))
                seen.add(u.tobytes())
    assert len(seen) == 50 * 2 * 2                                          # differs across index, side and epoch
    many = K.crop_directions(7, 0, list(range(50)), [A.SIDE_SRC] * 50)
    assert np.array_equal(many[3], K.crop_direction(A.cloud_key(7, 0, 3, A.SIDE_SRC)))
    # uniform on the sphere: the mean of 4000 directions is near the origin (|mean| ~ 1 / sqrt(n))
    big = K.crop_directions(1, 0, list(range(4000)), [0] * 4000).astype(np.float64)
    assert np.abs(big.mean(0)).max() < 0.05 and abs(float((big[:, 2] ** 2).mean()) - 1.0 / 3.0) < 0.02


def _line(n, xs=None, C=3, seed=0):
    """A cloud on the x axis with the given x (direction e_x: the projection is x - mean x)."""
    rng = np.random.default_rng(seed)
    pts = np.zeros((n, C), np.float32)
    pts[:, 0] = rng.standard_normal(n) if xs is None else xs
    if C > 3:
        pts[:, 3:] = rng.random((n, C - 3))
    return pts


EX = np.array([1.0, 0.0, 0.0], np.float32)


def test_edges():
    pts = _line(101, C=4)
    d = pts[:, 0] - np.float32(A.centroid(pts)[0])
    out, inv = K.halfspace_crop_host(pts, 0.5, EX)                          # the reference's special case: d > 0
    assert inv == 0 and np.array_equal(out, pts[d > 0])
    out, inv = K.halfspace_crop_host(pts, 1.0, EX)
    assert inv == 0 and np.array_equal(out, pts)
    out, inv = K.halfspace_crop_host(pts, 0.6, EX)                          # v = 100 * 0.4 = 40: keeps the rows above the 40th smallest
    assert inv == 0 and len(out) == 60 and np.array_equal(out, pts[d > np.sort(d)[40]])
    assert np.array_equal(out[:, 3], pts[d > np.sort(d)[40], 3])            # whole rows, input order
    # all projections equal: nothing is strictly above the threshold
    out, inv = K.halfspace_crop_host(_line(9, xs=np.full(9, 2.5)), 0.7, EX)
    assert out.shape == (0, 3) and inv == A.INVALID_EMPTY
    # -0 equals +0
    mask, inv = K.keep_mask(np.array([-0.0, 0.0, -0.0, 0.0], np.float32), 0.7)
    assert not mask.any() and inv == A.INVALID_EMPTY
    # n = 0 and n = 1
    out, inv = K.halfspace_crop_host(np.zeros((0, 5), np.float32), 0.6, EX)
    assert out.shape == (0, 5) and inv == A.INVALID_EMPTY
    out, inv = K.halfspace_crop_host(_line(1), 0.6, EX)
    assert out.shape == (0, 3) and inv == A.INVALID_EMPTY
    out, inv = K.halfspace_crop_host(_line(1), 1.0, EX)
    assert out.shape == (1, 3) and inv == 0
    # an Inf row makes the centroid of the whole cloud non-finite, whatever the direction
    pts = _line(11)
    pts[4, 1] = np.inf
    out, inv = K.halfspace_crop_host(pts, 0.6, EX)
    assert out.shape == (0, 3) and inv == A.INVALID_NONFINITE
    # a NaN projection under a finite centroid, on projections directly
    d = np.arange(11, dtype=np.float32)
    d[2] = np.nan
    mask, inv = K.keep_mask(d, 0.6)                                         # lo = 4: sorted finite 0 1 3 4 [5] ... -> d > 5, NaN dropped
    assert inv == 0 and np.array_equal(np.nonzero(mask)[0], np.arange(6, 11))
    mask, inv = K.keep_mask(d, 0.5)
    assert inv == 0 and np.array_equal(np.nonzero(mask)[0], np.array([1, 3, 4, 5, 6, 7, 8, 9, 10]))
    d[:] = np.nan
    d[0] = 1.0                                                              # rank lo = 4 sits on a NaN: refused
    mask, inv = K.keep_mask(d, 0.6)
    assert not mask.any() and inv == A.INVALID_NONFINITE
    # a NaN centroid
    pts = _line(11)
    pts[3, 0] = np.nan
    out, inv = K.halfspace_crop_host(pts, 0.6, EX)
    assert out.shape == (0, 3) and inv == A.INVALID_NONFINITE


def test_order_key_orders_like_fp32():
    v = np.array([-np.inf, -3.0e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.0e38], np.float32)
    k = K.order_key(v)
    assert k[0] == K.KEY_NONFINITE and k[4] == k[5]
    fin = k[1:]
    assert (np.diff(fin[[0, 1, 2, 3, 5, 6, 7]].astype(np.int64)) > 0).all()
    assert (K.order_key(np.array([np.nan, np.inf], np.float32)) == K.KEY_NONFINITE).all()


# ---- the Oxford loaders on the host (no engine: the constructors only parse)
def test_train_list_parsing_with_a_malformed_line(tmp_path, caplog):
    d = tmp_path / "train_np_nofilter"
    d.mkdir()
    (d / "train_relative.txt").write_text("a/0.npy | 1 2 3 | 1 2 3 4\nbroken line without bars\nb/7.npy |  | 9\n")
    with caplog.at_level(logging.INFO, logger=D.__name__):
        ds = D.OxfordTrain(str(tmp_path), None, num_points=512)
    assert len(ds) == 2 and any("Invalid line 1" in r.getMessage() for r in caplog.records)
    assert ds.files[0] == {"file": "a/0.npy", "pos_list": [1, 2, 3], "nonneg_list": [1, 2, 3, 4]}
    assert ds.files[1] == {"file": "b/7.npy", "pos_list": [], "nonneg_list": [9]}
    assert ds.self_pair_crop == 0.6 and ds.crop == (0.0, 50.0, -3.0, 20.0) and ds.match_radius == pytest.approx(0.9)
    cfg = ds.augment_cfg
    assert cfg.variant == "v2" and cfg.random_rotation and cfg.random_jitter and cfg.random_scale and (cfg.min_scale, cfg.max_scale) == (0.8, 1.2)
    (d / "a").mkdir()
    scan = np.arange(70, dtype=np.float64).reshape(10, 7)
    np.save(str(d / "a" / "0.npy"), scan)
    raw = ds.raw(0)
    assert raw.dtype == np.float32 and np.array_equal(raw, scan[:, :3].astype(np.float32))
    with pytest.raises(FileNotFoundError):
        D.OxfordTrain(str(tmp_path / "nowhere"), None, num_points=512)


def _quat_matrix(q):
    """Rotation of a unit quaternion [w x y z] applied as q v q* to the basis vectors, float64, written out here."""
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)

    def mul(a, b):
        return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                         a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])
    qq, qc = np.array([w, x, y, z]), np.array([w, -x, -y, -z])
    return np.stack([mul(mul(qq, np.array([0.0, *e])), qc)[1:] for e in np.eye(3)], 1)


def test_groundtruths_to_poses_and_num_val(tmp_path):
    d = tmp_path / "test_models_20k_np_nofilter"
    d.mkdir()
    rng = np.random.default_rng(3)
    recs = []
    for i in range(5):
        q = rng.standard_normal(4)
        recs.append({"anc_idx": 2 * i, "pos_idx": 2 * i + 1, "neg_idx": 0, "t": rng.standard_normal(3), "q": q / np.linalg.norm(q)})
    with open(d / "groundtruths.pkl", "wb") as f:
        pickle.dump(recs, f)
    ds = D.OxfordTest(str(tmp_path), None, "test")
    assert len(ds) == 5 and ds.augment_cfg.permute is False and not ds.augment_cfg.random_rotation
    for i, r in enumerate(recs):
        M = ds.pose(i)
        assert M.dtype == np.float64 and M.shape == (4, 4)
        assert np.abs(M[:3, :3] - _quat_matrix(r["q"])).max() < 1e-14 and np.array_equal(M[:3, 3], r["t"]) and np.array_equal(M[3], [0, 0, 0, 1])
        assert np.abs(M[:3, :3] @ M[:3, :3].T - np.eye(3)).max() < 1e-14 and np.linalg.det(M[:3, :3]) > 0
    assert np.array_equal(xyzquat2mat([1, 2, 3, 1, 0, 0, 0]), np.array([[1, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1.0]]))
    assert np.allclose(xyzquat2mat([0, 0, 0, 0, 2, 0, 0])[:3, :3], np.diag([1.0, -1.0, -1.0]))       # not unit: normalised first
    assert len(D.OxfordTest(str(tmp_path), None, "val", num_val=2)) == 2
    assert len(D.OxfordTest(str(tmp_path), None, "test", num_val=2)) == 5                           # only the val split is truncated
    assert len(D.OxfordTest(str(tmp_path), None, "val")) == 5
    with pytest.raises(ValueError):
        D.OxfordTest(str(tmp_path), None, "train")


def test_permute_switch_of_the_v2_resampler():
    on = A.AugmentConfig(variant="v2", num_points=64)
    off = A.AugmentConfig(variant="v2", num_points=64, permute=False)
    assert on.permute is True
    assert [p.resample_mode for p in A.pair_params(on, 1, 0, 5)] == [A.RESAMPLE_PERMUTED_FIXED] * 2
    assert [p.resample_mode for p in A.pair_params(off, 1, 0, 5)] == [A.RESAMPLE_FIXED] * 2 and A.RESAMPLE_FIXED == 1
    # v1 does not look at it
    assert [p.resample_mode for p in A.pair_params(A.AugmentConfig(variant="v1", permute=False), 1, 0, 5)] == [A.RESAMPLE_RANDOM] * 2
    # and nothing else of a cloud's parameters moves
    a, b = A.pair_params(on, 1, 0, 5)[0], A.pair_params(off, 1, 0, 5)[0]
    assert np.array_equal(a.R, b.R) and np.array_equal(a.t, b.t) and a.key == b.key and a.scale == b.scale
