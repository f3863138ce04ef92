"""harness.register_fpfh(keypoints="fps"): matching and pose on farthest-point samples (csrc/fps.hip), one batched matching call and
one batched pose call per batch, on the bumpy pair of tests/test_gpu_fpfh_keypoints.py and with that file's criterion (the 3DMatch
thresholds through rte_rre, success == 1); the default path's bytes, the result's shape, batch independence, the fall-back and
scene_edges_fpfh's forwarding."""
import numpy as np
import pytest
import torch

import iss_cases as K
from deepsir_amd import fpfh as F
from deepsir_amd.metrics import THRESHOLDS, rte_rre

pytestmark = pytest.mark.gpu

KW = dict(voxel_size=K.PAIR_VOXEL, hypotheses=1024, mutual=True, seed=0, want_corr=True)
NK = 256                   # of 1024 points a side


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    from deepsir_amd.weights import generate_state_dict
    cfg = NetConfig()
    e = Engine(cfg, max_points=2048, max_pairs=3)
    e.load_state_dict(generate_state_dict(cfg, 0))          # the pyramid and the search refuse a context without weights
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_default_is_todays_call(eng):
    from deepsir_amd.harness import register_fpfh
    pr = K.pair()
    a, sa, ca = register_fpfh([pr], eng, **KW)
    b, sb, cb = register_fpfh([pr], eng, keypoints=None, num_keypoints=NK, **KW)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(sa[:, :3], sb[:, :3])
    assert all(np.array_equal(x, y) for x, y in zip(ca[0], cb[0]))
    for bad in (dict(keypoints="harris"), dict(keypoints="fps", num_keypoints=0), dict(keypoints="fps", num_keypoints=2.5)):
        with pytest.raises(ValueError):
            register_fpfh([pr], eng, **bad, **KW)


def test_registers_on_fps_keypoints(eng):
    from deepsir_amd.harness import register_fpfh
    pr = K.pair()
    pred, stats, corr, kp = register_fpfh([pr], eng, keypoints="fps", num_keypoints=NK, want_keypoints=True, **KW)
    rte_t, rre_t = THRESHOLDS["3DMatch"]
    succ, rte, rre = rte_rre(pred[0, 0], pr["transform_gt"][0], rte_t, rre_t)
    print("fps keypoints: rte", rte, "rre", rre)
    assert succ == 1.0 and stats[0, 0] == 1.0, (rte, rre)
    idx_s, idx_r, fell_back = kp[0]
    assert fell_back is False
    for idx, side in ((idx_s, "src"), (idx_r, "ref")):
        assert idx.dtype == np.int32 and idx.shape == (NK,) and len(set(idx.tolist())) == NK        # exactly num_keypoints distinct rows
        own, counts, _ = eng.farthest_point_sample(torch.from_numpy(pr["points_" + side]).cuda(), NK)
        assert int(counts[0]) == NK and np.array_equal(own[0].cpu().numpy(), idx)
    c = corr[0][0]
    assert c.dtype == np.int32 and len(c) >= 3 and np.isin(c[:, 0], idx_s).all() and np.isin(c[:, 1], idx_r).all()
    assert c[:, 0].max() >= NK                              # original indices, not positions in the sample


@pytest.mark.parametrize("pose", ["consensus", "ransac"])
def test_batch_of_three_equals_single_pairs(eng, pose):
    """consensus has no random draws: a pair's bytes do not depend on the batch.  ransac keys a pair's draws by (seed, position in the
    call) - csrc/ransac.hip: pair p under seed s is pair 0 under seed s ^ (p << 40) - so the single calls take that seed."""
    from deepsir_amd.harness import register_fpfh
    prs = [K.pair(), F.bumpy_pair(K.PAIR_SEED + 2), F.bumpy_pair(K.PAIR_SEED + 3)]
    kw = dict(KW, keypoints="fps", num_keypoints=NK, want_keypoints=True, pose=pose)
    both, _, cb, kb = register_fpfh(prs, eng, batch=3, **kw)
    for i, pr in enumerate(prs):
        one, _, c1, k1 = register_fpfh([pr], eng, batch=1, **dict(kw, seed=0 ^ (i << 40)))
        assert np.array_equal(_bits(one[0]), _bits(both[i])), (pose, i)
        assert np.array_equal(c1[0][0], cb[i][0]) and np.array_equal(k1[0][0], kb[i][0]) and np.array_equal(k1[0][1], kb[i][1])
        assert k1[0][2] is False and kb[i][2] is False


def test_fallback_equals_all_points(eng):
    from deepsir_amd.harness import register_fpfh
    pr = K.pair()
    n = pr["points_ref"].shape[1]
    base, _, cb = register_fpfh([pr], eng, **KW)
    # fewer points than num_keypoints, and fewer sampled rows than min_keypoints
    for kw in (dict(num_keypoints=n + 1), dict(num_keypoints=16, min_keypoints=32), dict(num_keypoints=NK, min_keypoints=NK + 1)):
        pred, _, corr, kp = register_fpfh([pr], eng, keypoints="fps", want_keypoints=True, **kw, **KW)
        assert kp[0][2] is True and np.array_equal(kp[0][0], np.arange(n)) and np.array_equal(kp[0][1], np.arange(n)), kw
        assert np.array_equal(_bits(pred), _bits(base)) and np.array_equal(corr[0][0], cb[0][0]), kw


def test_scene_edges_forward_the_keywords(eng):
    from deepsir_amd.harness import register_fpfh, scene_edges_fpfh
    pr = K.pair()
    frags = [pr["points_src"][0], pr["points_ref"][0]]
    kw = dict(keypoints="fps", num_keypoints=NK, voxel_size=K.PAIR_VOXEL, hypotheses=1024, seed=0)
    edge = scene_edges_fpfh(frags, eng, **kw)
    bare = [{"points_src": frags[0][None], "points_ref": frags[1][None]}]           # a scene's pairs carry no viewpoints
    direct = register_fpfh(bare, eng, **kw)[0]
    plain = register_fpfh(bare, eng, voxel_size=K.PAIR_VOXEL, hypotheses=1024, seed=0)[0]
    assert np.array_equal(_bits(np.asarray(edge[0][2], np.float32)), _bits(direct[0, 0]))
    assert not np.array_equal(_bits(direct), _bits(plain))
    with pytest.raises(ValueError):
        scene_edges_fpfh(frags, eng, keypoints="fps", num_keypoints=0)
