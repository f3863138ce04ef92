"""Training batches on the device: csrc/augment.hip against the host rule (deepsir_amd/augment.py), then fabricated datasets in the
reference's layout through ``TrainBatches`` into ``Network.train_step`` and examples/train_dataset.py."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from deepsir_amd import augment as A
from deepsir_amd import data as D

pytestmark = pytest.mark.gpu

COUNTS = [1, 63, 64, 65, 1200, 1500]       # both ends, the wave boundary, more than one block; cap = 1500
CAP = 1500


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), 0, max_points=8192, max_pairs=2)
    yield e
    e.close()


def _voxels(stride, seed, counts=COUNTS, cap=CAP):
    """[clouds][cap][stride] as dsir_voxel_downsample leaves it: rows past the count are garbage that must never be read as data."""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal((len(counts), cap, stride)) * 3.0 + np.array([20.0, -7.0, 1.5] + [0.0] * (stride - 3))).astype(np.float32)
    if stride > 3:
        v[:, :, 3:] = rng.integers(0, 20, (len(counts), cap, stride - 3)).astype(np.float32) * 0.25
    for c, n in enumerate(counts):
        v[c, n:] = 1e30
    return v


def _poses(P, seed):
    rng = np.random.default_rng(seed)
    M = np.tile(np.eye(4), (P, 1, 1))
    for p in range(P):
        M[p, :3, :3] = A.rodrigues(rng.random(3) - 0.5, 0.4)
        M[p, :3, 3] = rng.random(3) * 4 - 2
    return M


def _run(eng, vs, cs, vr, cr, M, cfg, seed, epoch, indices, k):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    out = eng.augment(t(vs, torch.float32), t(cs, torch.int32), t(vr, torch.float32), t(cr, torch.int32), M, cfg, seed, epoch, indices, k,
                      return_rows=True)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _ulp_bound(cloud):
    """8 fp32 ulp of the cloud's largest |coordinate|: device and host differ in the float64 reduction order of the centroid and of
    the 3x3 compositions (1e-16 relative), which can move each of the at most four fp32 roundings on a coordinate's path by one ulp."""
    return 8.0 * float(np.spacing(np.float32(np.abs(cloud[:, :3]).max())))


CASES = [(variant, stride, k, gate, normals)
         for variant in ("v1", "v2") for stride in (3, 4, 6) for k in (64, 2048) for gate in (1.0, 0.0)
         for normals in ((False, True) if stride == 6 and gate == 1.0 else (False,))]


@pytest.mark.parametrize("variant,stride,k,gate,normals", CASES)
def test_device_augmentation_equals_the_host_rule(eng, variant, stride, k, gate, normals):
    P = len(COUNTS)
    vs, vr = _voxels(stride, 1), _voxels(stride, 2)
    cs, cr = np.array(COUNTS, np.int32), np.array(COUNTS[::-1], np.int32)
    for c, n in enumerate(cr):
        vr[c, n:] = 1e30
    M = _poses(P, 3)
    # v1: the 0.95 gates forced on / off; v2 has no gate: its jitter (and a scale, which the rule allows) switched on / off
    on = gate == 1.0
    cfg = A.AugmentConfig(variant=variant, num_points=k, gate=gate, normals=normals, random_jitter=on or variant == "v1",
                          random_scale=on or variant == "v1", xy_rot_scale=0.1)
    indices = [5, 900, 2, 77, 31, 10 ** 9]
    src, ref, gt, invalid, rows_s, rows_r = _run(eng, vs, cs, vr, cr, M, cfg, 11, 4, indices, k)
    assert src.shape == (P, k, stride) and ref.shape == (P, k, stride) and gt.shape == (P, 3, 4) and invalid.shape == (2, P)
    assert not invalid.any()
    for p in range(P):
        want = A.augment_pair(vs[p, :cs[p]], vr[p, :cr[p]], M[p], cfg, 11, 4, indices[p], k)
        pp = want["params"]
        assert (pp[0].jitter_mode != A.JITTER_NONE) == on and pp[0].scaled == on
        for got, rows, key, cloud in ((src[p], rows_s[p], "src", vs[p, :cs[p]]), (ref[p], rows_r[p], "ref", vr[p, :cr[p]])):
            assert np.array_equal(rows, want["rows_" + key])                                   # which row every output row came from
            w = want["points_" + key]
            lo = 6 if normals else 3
            assert np.array_equal(got[:, lo:].view(np.uint32), cloud[rows][:, lo:].view(np.uint32))    # untouched columns: bit-exact
            bound = _ulp_bound(cloud)
            assert np.abs(got[:, :3].astype(np.float64) - w[:, :3]).max() <= bound, (p, key)
            if normals:
                assert np.abs(got[:, 3:6].astype(np.float64) - w[:, 3:6]).max() <= 8.0 * float(np.spacing(np.float32(np.abs(cloud[:, 3:6]).max())))
        extent = max(float(np.abs(vs[p, :cs[p], :3]).max()), float(np.abs(vr[p, :cr[p], :3]).max()))
        assert np.abs(gt[p, :, :3] - want["transform_gt"][:, :3]).max() <= 1e-6
        assert np.abs(gt[p, :, 3] - want["transform_gt"][:, 3]).max() <= 1e-6 * extent
    if not on:
        # gates off == the switches off, bit for bit: nothing was jittered or scaled
        off = A.AugmentConfig(variant=variant, num_points=k, normals=normals, random_jitter=False, random_scale=False, xy_rot_scale=0.1)
        src0, ref0, gt0, *_ = _run(eng, vs, cs, vr, cr, M, off, 11, 4, indices, k)
        assert src0.tobytes() == src.tobytes() and ref0.tobytes() == ref.tobytes() and gt0.tobytes() == gt.tobytes()


def test_reference_gt_keeps_the_unscaled_translation(eng):
    vs, vr = _voxels(3, 1), _voxels(3, 2)
    cs = np.array(COUNTS, np.int32)
    M = _poses(len(COUNTS), 3)
    idx = list(range(len(COUNTS)))
    cfg = A.AugmentConfig(variant="v2", num_points=64, random_scale=True)
    ref_cfg = A.AugmentConfig(variant="v2", num_points=64, random_scale=True, reference_gt=True)
    a = _run(eng, vs, cs, vr, cs, M, cfg, 1, 0, idx, 64)
    b = _run(eng, vs, cs, vr, cs, M, ref_cfg, 1, 0, idx, 64)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    for p in idx:
        s = A.pair_params(cfg, 1, 0, p)[0].scale
        assert np.array_equal(a[2][p, :, :3], b[2][p, :, :3])
        np.testing.assert_allclose(b[2][p, :, 3] * s, a[2][p, :, 3], rtol=1e-6, atol=1e-6)


def test_same_bytes_across_runs_and_batches(eng):
    vs, vr = _voxels(4, 5), _voxels(4, 6)
    cs = np.array(COUNTS, np.int32)
    M = _poses(len(COUNTS), 7)
    cfg = A.AugmentConfig(variant="v1", num_points=256)
    idx = [3, 1, 4, 15, 9, 2]
    a = _run(eng, vs, cs, vr, cs, M, cfg, 8, 2, idx, 256)
    b = _run(eng, vs, cs, vr, cs, M, cfg, 8, 2, idx, 256)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # a call of 4 pairs (other positions, other neighbours) and calls of 1 pair: the sample's bytes are the same
    sel = [4, 2, 5, 0]
    four = _run(eng, vs[sel], cs[sel], vr[sel], cs[sel], M[sel], cfg, 8, 2, [idx[i] for i in sel], 256)
    for j, i in enumerate(sel):
        one = _run(eng, vs[i:i + 1], cs[i:i + 1], vr[i:i + 1], cs[i:i + 1], M[i:i + 1], cfg, 8, 2, [idx[i]], 256)
        for full, part4, part1 in zip(a[:3], four[:3], one[:3]):
            assert full[i].tobytes() == part4[j].tobytes() == part1[0].tobytes()
    # another epoch, another sample
    c = _run(eng, vs, cs, vr, cs, M, cfg, 8, 3, idx, 256)
    assert all(a[0][p].tobytes() != c[0][p].tobytes() for p in range(len(idx)))


@pytest.mark.parametrize("variant", ["v1", "v2"])
def test_empty_and_non_finite_clouds_are_flagged_and_isolated(eng, variant):
    counts, cap = [40, 70, 33, 64], 70
    vs, vr = _voxels(3, 8, counts, cap), _voxels(3, 9, counts, cap)
    M = _poses(4, 10)
    cfg = A.AugmentConfig(variant=variant, num_points=96)
    idx = [0, 1, 2, 3]
    cs = np.array(counts, np.int32)
    good = _run(eng, vs, cs, vr, cs, M, cfg, 1, 0, idx, 96)
    cs_bad, vs_bad, vr_bad = cs.copy(), vs.copy(), vr.copy()
    cs_bad[1] = 0                                  # src cloud of pair 1 is empty
    vr_bad[2, 5, 1] = np.nan                       # ref cloud of pair 2 holds a NaN point
    bad = _run(eng, vs_bad, cs_bad, vr_bad, cs, M, cfg, 1, 0, idx, 96)
    assert bad[3].tolist() == [[0, A.INVALID_EMPTY, 0, 0], [0, 0, A.INVALID_NONFINITE, 0]]
    assert not bad[0][1].any()                     # the empty cloud: rows written as zeros
    for p in range(4):
        if p != 1:
            assert bad[0][p].tobytes() == good[0][p].tobytes()
        if p != 2:
            assert bad[1][p].tobytes() == good[1][p].tobytes()
        if p not in (1, 2) or (variant == "v2" and p == 1):      # v2 does not use the centroid: only v1's pose needs it
            assert bad[2][p].tobytes() == good[2][p].tobytes()
    want = A.augment_pair(vs_bad[1, :0], vr_bad[1, :cs[1]], M[1], cfg, 1, 0, 1, 96)
    assert want["invalid"].tolist() == [A.INVALID_EMPTY, 0]


# ================================================================================================== end to end
def _write_3dmatch(root, n_clouds=3, n_points=4000):
    rng = np.random.default_rng(20)
    base = (rng.random((n_points * 2, 3)) * [2.4, 1.8, 1.2]).astype(np.float32)
    ids = [f"scene_a/cloud_bin_{i}" for i in range(n_clouds)]
    pts = {k: base[rng.permutation(len(base))[:n_points]] for k in ids}       # overlapping fragments in a common frame
    ovl = {f"{ids[0]}@{ids[1]}": 0.6, f"{ids[1]}@{ids[2]}": 0.5, f"{ids[0]}@{ids[2]}": 0.4, f"{ids[2]}@{ids[0]}": 0.2}
    d = os.path.join(root, "3dmatch_train_val")
    os.makedirs(d, exist_ok=True)
    for split in ("train", "val"):
        pickle.dump(pts, open(os.path.join(d, f"3DMatch_{split}_0.030_points.pkl"), "wb"))
        pickle.dump(ovl, open(os.path.join(d, f"3DMatch_{split}_0.030_overlap.pkl"), "wb"))
    return pts


def _check_dict(batch, B, N, F, labels):
    assert set(batch) == {"points_src", "points_ref", "transform_gt", "others", "matches", "invalid"} | ({"labels_src", "labels_ref"} if labels else set())
    for k in ("points_src", "points_ref"):
        assert batch[k].is_cuda and batch[k].dtype == torch.float32 and tuple(batch[k].shape) == (B, N, F) and batch[k].is_contiguous()
    assert batch["transform_gt"].is_cuda and batch["transform_gt"].dtype == torch.float32 and tuple(batch["transform_gt"].shape) == (B, 3, 4)
    assert len(batch["others"]) == B and all(set(o) == {"seq", "id_src", "id_ref"} for o in batch["others"])
    assert len(batch["matches"]) == B and all(m.dtype == np.int64 and m.ndim == 2 and m.shape[1] == 2 for m in batch["matches"])
    if labels:
        for k in ("labels_src", "labels_ref"):
            assert batch[k].dtype == torch.int64 and tuple(batch[k].shape) == (B, N)


def _same_batch(a, b):
    return all(a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() for k in ("points_src", "points_ref", "transform_gt")) and \
        all(np.array_equal(x, y) for x, y in zip(a["matches"], b["matches"]))


def _network(feat_len):
    from types import SimpleNamespace
    from deepsir_amd.model import Network
    from deepsir_amd.weights import generate_state_dict, to_torch_state_dict
    args = SimpleNamespace(pipeline="align", feat_len=feat_len, num_sub=-1, num_knn=16, out_feat_dim=64, clip_weight_thresh=0.0,
                           d_out=[16, 64, 128, 256], sub_sampling_ratio=[4, 4, 4, 4], use_ppf=False, num_reg_iter=2, loss_type="mae",
                           wt_ptDist_loss=1.0, wt_inlier_loss=1.0, wt_pose_loss=0.0, loss_discount_factor=0.5)
    net = Network(args)
    net.load_state_dict(to_torch_state_dict(generate_state_dict(net.cfg, 1, "separated")))
    return net.cuda().train(), args


def test_threedmatch_batches_train_the_network(tmp_path, eng):
    from deepsir_amd.train import as_reference_matches
    _write_3dmatch(str(tmp_path))
    net, _ = _network(3)
    ds = D.ThreeDMatchTrain(str(tmp_path), eng, "train", num_points=1024)
    assert len(ds) == 3
    it = D.TrainBatches(ds, 2, seed=5)
    assert len(it) == 1
    first = next(iter(it))
    _check_dict(first, 2, 1024, 3, labels=False)
    assert not first["invalid"].any()
    # matches == the reference's get_matches on the yielded clouds: radius search around T_gt src among ref
    off, cols = eng.radius_matches(first["points_src"], first["points_ref"], first["transform_gt"], ds.match_radius)
    again = as_reference_matches(off, cols, 2, 1024)
    assert all(np.array_equal(x, y) for x, y in zip(first["matches"], again)) and sum(len(m) for m in again) > 200
    src, ref, T = (first[k].double().cpu().numpy() for k in ("points_src", "points_ref", "transform_gt"))
    for p in range(2):
        m = first["matches"][p]
        d = np.linalg.norm(src[p][m[:, 0]] @ T[p, :, :3].T + T[p, :, 3] - ref[p][m[:, 1]], axis=1)
        assert d.max() < ds.match_radius + 1e-5
    # the same seed reproduces epoch 0's first batch byte for byte (fresh iterator, cold cache); epoch 1 differs
    again0 = next(iter(D.TrainBatches(ds, 2, seed=5)))
    assert _same_batch(first, again0) and [o["id_src"] for o in first["others"]] == [o["id_src"] for o in again0["others"]]
    it.set_epoch(1)
    second = next(iter(it))
    assert not _same_batch(first, second) and 2 <= len(it.cache) <= 3
    # the radius alone instead of a list
    lean = next(iter(D.TrainBatches(ds, 2, seed=5, match_radius=ds.match_radius)))
    assert "matches" not in lean and lean["match_radius"] == ds.match_radius
    # two optimisation steps
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    losses = [float(net.train_step(b, (2, True), lr=1e-3, dropout_seed=s)["loss"]) for s, b in enumerate((first, second))]
    assert np.isfinite(losses).all()
    moved = [k for k, p in net.named_parameters() if not torch.equal(p.detach(), before[k])]
    assert moved and all(k.startswith("inlier_model.") for k in moved)


def test_kitti_batches_with_labels(tmp_path):
    from test_data import make_kitti
    rng = np.random.default_rng(21)
    scene = np.stack([rng.uniform(-30, 30, 20000), rng.uniform(-2, 1.6, 20000), rng.uniform(-10, 70, 20000)], 1)
    root = str(tmp_path / "kitti")
    make_kitti(root, 3, 5, 1.0, rng=rng, scene=scene)
    lab = os.path.join(root, "dataset", "sequences", "03", "labels")
    os.makedirs(lab)
    keys = np.array(sorted(D.SEMANTIC_KITTI_LEARNING_MAP), dtype=np.uint32)
    for t in range(5):
        keys[rng.integers(0, len(keys), len(scene))].tofile(os.path.join(lab, "%06d.label" % t))
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    net, _ = _network(4)
    eng = Engine(NetConfig(feat_len=4), 0, max_points=65536, max_pairs=1)      # the data path's own engine: raw scans are large
    ds = D.KittiOdometryTrain(root, eng, "train", sequences=[3], voxel_size=0.8, num_points=1024, refine_pose=False)
    assert ds.files == [(3, 0, 2), (3, 1, 3), (3, 2, 4)]
    batch = next(iter(D.TrainBatches(ds, 2, seed=1)))
    _check_dict(batch, 2, 1024, 4, labels=True)
    for k in ("labels_src", "labels_ref"):
        assert int(batch[k].min()) >= 0 and int(batch[k].max()) <= 19
    # src moved by transform_gt lands on ref (a static scene, exact odometry; jitter 0.01 m): checked with every voxel kept
    # (num_points above the voxel count tiles the permuted cloud), since two random 1024-subsets are not neighbours of each other
    dense = D.KittiOdometryTrain(root, eng, "train", sequences=[3], voxel_size=0.8, num_points=16384, refine_pose=False)
    full = next(iter(D.TrainBatches(dense, 1, seed=1, match_radius=1.0)))
    T = full["transform_gt"]
    moved = full["points_src"][0, :, :3] @ T[0, :, :3].T + T[0, :, 3]
    d = torch.cdist(moved[:512], full["points_ref"][0, :, :3]).min(1)[0]
    assert float(d.median()) < 0.3
    ident = torch.cdist(full["points_src"][0, :512, :3], full["points_ref"][0, :, :3]).min(1)[0]
    assert float(ident.median()) > 2.0 * float(d.median())          # and not without it: the augmentation moved the clouds apart
    assert sum(len(m) for m in batch["matches"]) > 500
    out = net.train_step(batch, (2, True), lr=1e-3, dropout_seed=0)
    assert np.isfinite(float(out["loss"]))
    eng.close()


def test_driver_trains_checkpoints_and_resumes(tmp_path):
    _write_3dmatch(str(tmp_path / "data"))
    out = str(tmp_path / "run")
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_dataset.py"), "--dataset", "3dmatch", "--root", str(tmp_path / "data"),
           "--out", out, "--points", "1024", "--batch", "2", "--iters", "2", "--val-every", "2", "--num-val", "1"]
    r = subprocess.run(cmd + ["--steps", "3"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    ck = torch.load(os.path.join(out, "ckpt.pth"), map_location="cpu", weights_only=False)
    assert set(ck) == {"state_dict", "optimizer", "step"} and ck["step"] == 3 and ck["optimizer"]["state"]
    net, _ = _network(3)
    net.load_state_dict(ck["state_dict"], strict=True)
    import json
    log = [json.loads(ln) for ln in open(os.path.join(out, "log.jsonl"))]
    assert [e["step"] for e in log if e["event"] == "train"] == [1, 2, 3]
    vals = [e for e in log if e["event"] == "val"]
    assert [e["step"] for e in vals] == [2, 3] and all(np.isfinite(e["val_loss"]) and e["val_pairs"] == 1 for e in vals)
    r = subprocess.run(cmd + ["--steps", "4", "--resume"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    log = [json.loads(ln) for ln in open(os.path.join(out, "log.jsonl"))]
    assert [e["step"] for e in log if e["event"] == "train"] == [1, 2, 3, 4] and log[-1] == {"event": "end", "step": 4, "checkpoint": log[-1]["checkpoint"]}
    starts = [e for e in log if e["event"] == "start"]
    assert [s["resumed"] for s in starts] == [False, True] and starts[1]["step"] == 3
    ck2 = torch.load(os.path.join(out, "ckpt.pth"), map_location="cpu", weights_only=False)
    assert ck2["step"] == 4 and any(not torch.equal(ck2["state_dict"][k], ck["state_dict"][k]) for k in ck["state_dict"])
