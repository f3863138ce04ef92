"""pose="fgr" through the harness: register_fpfh and register_feat on two small synthetic pairs (the shapes of the sibling routes'
tests in test_gpu_consensus.py and test_gpu_ransac.py) return inference_align's layout and a pose within the dataset thresholds, and
the default pose="ransac" route writes the same bytes with and without the new keyword arguments.

The network of the register_feat test carries the generated (untrained) weights of the sibling test.  Its descriptors are functions of
absolute coordinates, so how many of its mutual matches are correct depends on the pair's motion alone: measured on the two clouds of
this test, before any estimator runs (correct within 0.05 m / matches): identical clouds 512 / 512; 2 degrees and 0.1 m 264 / 366 and
87 / 259; 0.35 m 16 / 195 and 2 / 157; 0.5 m or 20 degrees and beyond - the sibling test's own pairs - 0 to 4 correct, where RANSAC,
consensus and FGR all return the same wrong poses.  The pairs here therefore move by 2 degrees and 0.1 m: the largest motion of that
sweep at which both pairs still hand the pose stage a third of correct matches.  The identity would pass the dataset thresholds on
such a pair, so the pose is also asked to halve both components of the motion (0.05 m, 1 degree), which the identity cannot.
Descriptors of absolute position also shape the WRONG matches: they pair points that lie at nearly the same place in the two clouds,
which is what the identity predicts, so their residual under the true pose is about the motion itself (0.1 m).  The inlier threshold
therefore has to stay below the motion or that second consensus set merges with the true one: voxel_size = 0.025 (max_dist 0.05 m).
With the sibling test's voxel_size = 0.05 (max_dist = the motion) all three estimators keep those rows and end 1.4 to 3 degrees off
on the second pair, where the Kabsch fit of the truly correct matches alone is 0.1 degrees off."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FGR_KW = dict(fgr_iterations=64, tuple_scale=0.95, max_tuples=1000, tuple_test=True)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _check(pred, stats, pairs):
    from deepsir_amd.metrics import THRESHOLDS, rte_rre
    assert pred.shape == (2, 2, 3, 4) and stats.shape == (2, 5) and np.isfinite(pred).all() and np.isfinite(stats).all()
    assert np.array_equal(pred[:, 0], pred[:, 1])
    for T, pr in zip(pred[:, 0], pairs):
        assert np.abs(T[:, :3] @ T[:, :3].T - np.eye(3)).max() < 1e-5 and np.linalg.det(T[:, :3]) > 0.999
        ok, rte, rre = rte_rre(T, pr["transform_gt"][0], *THRESHOLDS["3DMatch"])
        print(f"FGR pose: success {ok}, rte {rte:.4f} m, rre {rre:.4f}")
        assert ok == 1.0


def test_register_fpfh_fgr():
    from deepsir_amd import fpfh as F
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    from deepsir_amd.harness import evaluate_align, register_fpfh
    from deepsir_amd.weights import generate_state_dict
    cfg = NetConfig()
    e = Engine(cfg, max_points=2048, max_pairs=2)
    try:
        e.load_state_dict(generate_state_dict(cfg, 0))
        pairs = [F.bumpy_pair(1), F.bumpy_pair(2)]
        kw = dict(voxel_size=0.05, batch=2, num_reg=2)
        plain, _ = register_fpfh(pairs, e, hypotheses=1024, **kw)
        named, _ = register_fpfh(pairs, e, hypotheses=1024, pose="ransac", **FGR_KW, **kw)
        assert _same_bits(plain, named)                                             # the default route is untouched
        pred, stats = register_fpfh(pairs, e, pose="fgr", **kw)
        _check(pred, stats, pairs)
        again, _ = register_fpfh(pairs, e, pose="fgr", **FGR_KW, **kw)
        assert _same_bits(pred, again)
        loose, _ = register_fpfh(pairs, e, pose="fgr", tuple_test=False, fgr_iterations=32, **kw)
        assert loose.shape == pred.shape and np.isfinite(loose).all()
        metrics, _ = evaluate_align(pred, pairs, e)
        assert len(metrics) == 2 and all(np.isfinite(v).all() for v in metrics[-1].values())
    finally:
        e.close()


def _small_motion_pair(ref, seed, deg=2.0, dist=0.1):
    """ref [1, N, 3] and a copy of it moved by `deg` degrees about a random axis and `dist` metres: ref = R src + t."""
    rng = np.random.default_rng(seed)
    d, ax = rng.normal(size=3), rng.normal(size=3)
    d, ax, a = d / np.linalg.norm(d), ax / np.linalg.norm(ax), np.radians(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rm, t = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K, dist * d
    src = ((ref[0].astype(np.float64) - t) @ Rm)[None].astype(np.float32)
    return {"points_src": src, "points_ref": ref, "transform_gt": np.concatenate([Rm, t[:, None]], 1)[None].astype(np.float32)}


def test_register_feat_fgr():
    from test_gpu_ransac import _network
    from deepsir_amd.harness import register_feat
    from deepsir_amd.synth import make_pair
    net = _network("feat", 512)
    pairs = [_small_motion_pair(make_pair(2048, s, 3)["points_ref"], s) for s in (51, 52)]
    kw = dict(voxel_size=0.025, mutual=True, num_reg=2, batch=2)                     # max_dist = 0.05 m: half the motion (docstring)
    plain, _ = register_feat(pairs, net, hypotheses=1024, **kw)
    named, _ = register_feat(pairs, net, hypotheses=1024, pose="ransac", **FGR_KW, **kw)
    assert _same_bits(plain, named)
    pred, stats = register_feat(pairs, net, pose="fgr", **kw)
    _check(pred, stats, pairs)
    assert (stats[:, 1] < 0.05).all() and (stats[:, 2] < 1.0).all()                 # half the motion: not the identity's errors
    again, _ = register_feat(pairs, net, pose="fgr", **FGR_KW, **kw)
    assert _same_bits(pred, again)
    with pytest.raises(ValueError):
        register_feat(pairs, net, pose="nope", **kw)
