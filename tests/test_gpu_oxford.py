"""The Oxford loaders on the device: a fabricated tree in the reference's layout (dataloader/oxford_loader.py) through
`TrainBatches` (one scan cropped twice by `Engine.halfspace_crop`) into `Network.train_step`, and the val / test pairs through
`harness.inference_align` / `evaluate_align`."""
import os
import pickle

import numpy as np
import pytest
import torch

from deepsir_amd import augment as A
from deepsir_amd import crop as K
from deepsir_amd import data as D

pytestmark = pytest.mark.gpu

SEED, N, VOXEL = 3, 2048, 1.0       # N above a crop's voxel count: every voxel of a crop is in the sample (tiled)
SCAN_SIZES = [3000, 3400, 3800, 4200, 4600, 5000]
POSE_T, POSE_ANGLE = np.array([1.5, -0.8, 0.2]), 0.3


def _scan(rng, n):
    """[n, 7] = [x y z nx ny nz curvature] inside the loader's range crop (r <= 50, -3 <= z <= 20)."""
    xyz = np.stack([rng.uniform(-25, 25, n), rng.uniform(-25, 25, n), rng.uniform(-2, 6, n)], 1)
    nrm = rng.standard_normal((n, 3))
    return np.concatenate([xyz, nrm / np.linalg.norm(nrm, axis=1, keepdims=True), rng.random((n, 1))], 1)


def _quat(angle, axis):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """6 train scans of 3000 to 5000 points and 3 test pairs built from a known pose: anc = R pos + t."""
    root = tmp_path_factory.mktemp("oxford")
    rng = np.random.default_rng(17)
    tr = root / "train_np_nofilter"
    (tr / "seq0").mkdir(parents=True)
    lines = []
    for i, n in enumerate(SCAN_SIZES):
        np.save(str(tr / "seq0" / f"{i}.npy"), _scan(rng, n))
        lines.append(f"seq0/{i}.npy | {(i + 1) % 6} | {(i + 1) % 6} {(i + 2) % 6}\n")
    lines.insert(2, "not a record\n")
    (tr / "train_relative.txt").write_text("".join(lines))
    te = root / "test_models_20k_np_nofilter"
    te.mkdir()
    q = _quat(POSE_ANGLE, [0.1, -0.2, 1.0])
    from deepsir_amd.se3 import xyzquat2mat
    M = xyzquat2mat(np.concatenate([POSE_T, q]))
    recs = []
    for k in range(3):
        anc = _scan(rng, 4000)
        pos = anc.copy()
        pos[:, :3] = (anc[:, :3] - M[:3, 3]) @ M[:3, :3]                     # anc = R pos + t
        np.save(str(te / f"{2 * k}.npy"), anc)
        np.save(str(te / f"{2 * k + 1}.npy"), pos)
        recs.append({"anc_idx": 2 * k, "pos_idx": 2 * k + 1, "neg_idx": [], "t": POSE_T.copy(), "q": q.copy()})
    with open(te / "groundtruths.pkl", "wb") as f:
        pickle.dump(recs, f)
    return str(root), M


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), 0, max_points=16384, max_pairs=2)
    yield e
    e.close()


def _network():
    from types import SimpleNamespace
    from deepsir_amd.model import Network
    from deepsir_amd.weights import generate_state_dict, to_torch_state_dict
    args = SimpleNamespace(pipeline="align", feat_len=3, num_sub=-1, num_knn=16, out_feat_dim=64, clip_weight_thresh=0.0,
                           d_out=[16, 64, 128, 256], sub_sampling_ratio=[4, 4, 4, 4], use_ppf=False, num_reg_iter=2, loss_type="mae",
                           wt_ptDist_loss=1.0, wt_inlier_loss=1.0, wt_pose_loss=0.0, loss_discount_factor=0.5, num_points=N)
    net = Network(args)
    net.load_state_dict(to_torch_state_dict(generate_state_dict(net.cfg, 1, "separated")))
    return net.cuda()


def _sample(batch, b):
    return b"".join(batch[k][b].cpu().numpy().tobytes() for k in ("points_src", "points_ref", "transform_gt")) + batch["matches"][b].tobytes()


def test_self_pairs_through_train_batches(tree, eng):
    root, _ = tree
    ds = D.OxfordTrain(root, eng, num_points=N, voxel_size=VOXEL)
    assert len(ds) == 6 and ds.self_pair_crop == 0.6 and ds.raw(2).shape == (SCAN_SIZES[2], 3)
    it = D.TrainBatches(ds, 2, seed=SEED, shuffle=False)
    first = it.batch([0, 1])
    assert tuple(first["points_src"].shape) == (2, N, 3) and tuple(first["transform_gt"].shape) == (2, 3, 4)
    assert not first["invalid"].any() and [o["id_src"] for o in first["others"]] == ["seq0/0.npy", "seq0/1.npy"]
    # the cache holds the raw scan on the device, once per index - not voxels
    assert sorted(it.cache) == [0, 1] and tuple(it.cache[1][0].shape) == (SCAN_SIZES[1], 3) and it.cache[1][0].is_cuda
    src, ref, T = (first[k].double().cpu().numpy() for k in ("points_src", "points_ref", "transform_gt"))
    for p in range(2):
        # the two half-spaces differ (the draws of the two sides), so the crops overlap in part only
        us, ur = (K.crop_direction(A.cloud_key(SEED, 0, p, s)).astype(np.float64) for s in (A.SIDE_SRC, A.SIDE_REF))
        assert float(us @ ur) < 0.9
        m = first["matches"][p]
        moved = src[p] @ T[p, :, :3].T + T[p, :, 3]
        assert len(m) > 1000 and np.linalg.norm(moved[m[:, 0]] - ref[p][m[:, 1]], axis=1).max() < ds.match_radius + 1e-5
        # transform_gt maps the src crop ONTO the ref crop: a src voxel of the overlap meets its own voxel in ref (both jittered by at
        # most 0.05 per axis and scaled by at most 1.2: 0.21 apart at most)
        nearest = np.sqrt(((moved[:, None, :] - ref[p][None, :, :]) ** 2).sum(-1)).min(1)
        shared = nearest < 0.25
        back = np.sqrt(((ref[p][:, None, :] - moved[None, :, :]) ** 2).sum(-1)).min(1) < 0.25
        # what the rule says of this scan on the host: the share of a crop's rows that the other crop keeps too (0.75 and 0.91 here).
        # The voxel grid (most 1 m voxels hold one point) and chance neighbours (1.3 % at this density) move it by a few percent.
        rows = np.concatenate([ds.raw(p), np.arange(SCAN_SIZES[p], dtype=np.float32)[:, None]], 1)
        ids = [set(K.halfspace_crop_host(rows, 0.6, u.astype(np.float32))[0][:, 3].tolist()) for u in (us, ur)]
        want = len(ids[0] & ids[1]) / len(ids[0])
        assert 0.3 < want < 0.95 and len(ids[0]) == len(ids[1])
        for got in (shared, back):                                             # the overlap: not empty, smaller than either crop
            assert abs(got.mean() - want) < 0.06 and 0.1 * N < got.sum() < 0.97 * N
        assert set(np.nonzero(shared)[0]) <= set(m[:, 0].tolist())             # every shared point is among the matches
    # a sample is the same bytes whatever batch it lands in, and differs between epochs
    other = it.batch([1, 3])
    assert _sample(first, 1) == _sample(other, 0) and _sample(first, 0) != _sample(other, 1)
    it.set_epoch(1)
    later = it.batch([0, 1])
    assert _sample(first, 0) != _sample(later, 0) and _sample(first, 1) != _sample(later, 1)
    assert sorted(it.cache) == [0, 1, 3]
    # the iterator itself: 3 batches an epoch
    assert len(it) == 3 and len(list(D.TrainBatches(ds, 4, seed=SEED))) == 1
    net = _network().train()
    out = net.train_step(first, (2, True), lr=1e-3, dropout_seed=0)
    assert np.isfinite(float(out["loss"]))


def test_val_and_test_pairs_through_the_harness(tree, eng):
    from deepsir_amd.harness import evaluate_align, inference_align
    root, M = tree
    ds = D.OxfordTest(root, eng, "test", voxel_size=VOXEL, num_points=N)
    assert len(ds) == 3 and len(D.OxfordTest(root, eng, "val", num_val=2)) == 2
    pairs = [D.as_batch(ds[i]) for i in range(3)]
    for p in pairs:
        assert p["points_src"].is_cuda and tuple(p["points_src"].shape) == (1, N, 3)
        assert np.array_equal(p["transform_gt"][0], M[:3].astype(np.float32))              # the fabricated pose
    assert [p["others"][0]["id_src"] for p in pairs] == [1, 3, 5] and [p["others"][0]["id_ref"] for p in pairs] == [0, 2, 4]
    # src moved by the ground truth lands on ref: the same scan seen from two frames, voxel means of the same points up to the grid
    free = D.OxfordTest(root, eng, "test", voxel_size=VOXEL)[1]                 # every voxel of both clouds
    s, r = free["points_src"].double().cpu().numpy(), free["points_ref"].double().cpu().numpy()
    moved = s @ M[:3, :3].T + M[:3, 3]
    assert np.median(np.sqrt(((moved[:256, None] - r[None]) ** 2).sum(-1)).min(1)) < VOXEL
    net = _network().eval()
    pred, stats = inference_align(pairs, net, 2, "Oxford", batch=1)
    assert pred.shape == (3, 3, 3, 4) and np.isfinite(pred).all() and stats.shape == (3, 5)
    metrics, summary = evaluate_align(pred, pairs, net._ensure_engine(N, 1), "Oxford")
    assert len(metrics) == 3 and set(metrics[-1]) == set(eng.METRIC_NAMES) and all(np.isfinite(v).all() for v in metrics[-1].values())
    assert {"r_rmse", "t_rmse", "err_r_deg_mean", "err_t_mean", "succ", "chamfer_dist"} <= set(summary)
    # without num_points: the cloud with fewer voxels is tiled to the size of the other, in voxel order (no permutation)
    assert free["points_src"].shape == free["points_ref"].shape and free["points_src"].shape[0] > N
    # as validation batches of the training loop: no augmentation, no permutation -> the voxels in their own order
    val = D.TrainBatches(D.OxfordTest(root, eng, "val", num_val=2, voxel_size=VOXEL, num_points=N), 1, seed=SEED, shuffle=False, drop_last=False)
    vb = next(iter(val))
    assert vb["points_src"].cpu().numpy().tobytes() == pairs[0]["points_src"].cpu().numpy().tobytes()
    assert np.array_equal(vb["transform_gt"][0].cpu().numpy(), M[:3].astype(np.float32)) and len(vb["matches"][0]) > 100


def test_pair_datasets_still_cache_voxels(tmp_path, eng):
    """A dataset without `self_pair_crop` takes the path it took before: the cache entry is the pair of voxelised clouds."""
    rng = np.random.default_rng(2)
    d = tmp_path / "3dmatch_train_val"
    d.mkdir()
    base = rng.random((6000, 3)) * [3.0, 2.0, 1.5]
    pts = {"s/seq-01/cloud_bin_0": base[:4000], "s/seq-01/cloud_bin_1": base[2000:]}
    with open(d / "3DMatch_train_0.030_points.pkl", "wb") as f:
        pickle.dump(pts, f)
    with open(d / "3DMatch_train_0.030_overlap.pkl", "wb") as f:
        pickle.dump({"s/seq-01/cloud_bin_0@s/seq-01/cloud_bin_1": 0.5}, f)
    ds = D.ThreeDMatchTrain(str(tmp_path), eng, "train", num_points=512, voxel_size=0.1)
    assert not hasattr(ds, "self_pair_crop")
    it = D.TrainBatches(ds, 1, seed=1)
    batch = it.batch([0])
    entry = it.cache[0]
    assert len(entry) == 4 and entry[0].is_cuda and entry[1].is_cuda and entry[0].dim() == 2 and entry[0].shape[1] == 3
    assert 0 < entry[0].shape[0] < 4000 and 0 < entry[1].shape[0] < 4000            # voxels, fewer than the raw points
    assert np.array_equal(entry[2], np.identity(4)) and tuple(batch["points_src"].shape) == (1, 512, 3)
