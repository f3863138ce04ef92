"""harness.register_fpfh(keypoints="iss"): matching and pose on ISS keypoints only (csrc/iss.hip), on the bumpy pair whose pose the
host chain of tests/test_iss_host.py recovers; the default path's bytes, the fall-back, ragged batches and scene_edges_fpfh's
forwarding."""
import numpy as np
import pytest
import torch

import iss_cases as K
from deepsir_amd import fpfh as F
from deepsir_amd.metrics import THRESHOLDS, rte_rre

pytestmark = pytest.mark.gpu

KW = dict(voxel_size=K.PAIR_VOXEL, hypotheses=1024, mutual=True, seed=0, want_corr=True)


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    from deepsir_amd.weights import generate_state_dict
    cfg = NetConfig()
    e = Engine(cfg, max_points=2048, max_pairs=2)
    e.load_state_dict(generate_state_dict(cfg, 0))          # the pyramid and the search refuse a context without weights
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_default_is_todays_call(eng):
    from deepsir_amd.harness import register_fpfh
    pr = K.pair()
    a, sa, ca = register_fpfh([pr], eng, **KW)
    b, sb, cb, kb = register_fpfh([pr], eng, keypoints=None, want_keypoints=True, **KW)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(sa[:, :3], sb[:, :3])
    assert all(np.array_equal(x, y) for x, y in zip(ca[0], cb[0]))
    n = pr["points_src"].shape[1]
    assert np.array_equal(kb[0][0], np.arange(n)) and np.array_equal(kb[0][1], np.arange(n)) and kb[0][2] is False
    with pytest.raises(ValueError):
        register_fpfh([pr], eng, keypoints="harris", **KW)


def test_registers_on_keypoints(eng):
    from deepsir_amd.harness import register_fpfh
    pr = K.pair()
    pred, stats, corr, kp = register_fpfh([pr], eng, keypoints="iss", want_keypoints=True, **KW)
    rte_t, rre_t = THRESHOLDS["3DMatch"]
    succ, rte, rre = rte_rre(pred[0, 0], pr["transform_gt"][0], rte_t, rre_t)
    assert succ == 1.0 and stats[0, 0] == 1.0, (rte, rre)
    idx_s, idx_r, fell_back = kp[0]
    n = pr["points_src"].shape[1]
    assert fell_back is False and 32 <= len(idx_s) < n // 2 and 32 <= len(idx_r) < n // 2
    assert (np.diff(idx_s) > 0).all() and (np.diff(idx_r) > 0).all()
    c = corr[0][0]
    assert c.dtype == np.int32 and len(c) >= 3 and np.isin(c[:, 0], idx_s).all() and np.isin(c[:, 1], idx_r).all()
    assert c[:, 0].max() >= len(idx_s)                      # original indices, not positions in the keypoint list
    # the keypoints are the engine's own for the default radii (6 and 4 voxel sizes)
    x = torch.from_numpy(pr["points_src"]).cuda()
    index, counts, _, _ = eng.iss_keypoints(x, salient_radius=K.PAIR_SALIENT, non_max_radius=K.PAIR_NMS)
    assert np.array_equal(index[0, :int(counts[0])].cpu().numpy(), idx_s)


def test_too_few_keypoints_fall_back_to_all_points(eng):
    from deepsir_amd.harness import register_fpfh
    pr = K.near_plane_pair()
    base, _, cb = register_fpfh([pr], eng, **KW)
    pred, _, corr, kp = register_fpfh([pr], eng, keypoints="iss", want_keypoints=True, **KW)
    n = pr["points_ref"].shape[1]
    assert kp[0][2] is True and np.array_equal(kp[0][0], np.arange(n)) and np.array_equal(kp[0][1], np.arange(n))
    assert np.array_equal(_bits(pred), _bits(base)) and np.array_equal(corr[0][0], cb[0][0])
    # min_keypoints above the count forces the same on a pair that has keypoints
    pr = K.pair()
    base, _, _ = register_fpfh([pr], eng, **KW)
    pred, _, _, kp = register_fpfh([pr], eng, keypoints="iss", min_keypoints=1024, want_keypoints=True, **KW)
    assert kp[0][2] is True and np.array_equal(_bits(pred), _bits(base))


def test_ragged_batch_equals_single_pairs(eng):
    from deepsir_amd.harness import register_fpfh, scene_edges_fpfh
    prs = [K.pair(), F.bumpy_pair(K.PAIR_SEED + 2), K.near_plane_pair()]       # 32, 33 and (after the fall-back) 1024 rows per side
    kw = dict(keypoints="iss", want_keypoints=True, **KW)
    both, _, cb, kb = register_fpfh(prs, eng, batch=2, **kw)
    sizes = set()
    for i, pr in enumerate(prs):
        one, _, c1, k1 = register_fpfh([pr], eng, batch=1, **kw)
        assert np.array_equal(_bits(one[0]), _bits(both[i])), i
        assert np.array_equal(c1[0][0], cb[i][0]) and np.array_equal(k1[0][0], kb[i][0]) and k1[0][2] == kb[i][2]
        sizes.add((len(k1[0][0]), len(k1[0][1])))
    assert len(sizes) == 3                                  # three different keypoint counts went through
    # scene_edges_fpfh forwards the keywords
    frags = [prs[0]["points_src"][0], prs[0]["points_ref"][0]]
    edge = scene_edges_fpfh(frags, eng, keypoints="iss", voxel_size=K.PAIR_VOXEL, hypotheses=1024, seed=0)
    bare = [{"points_src": frags[0][None], "points_ref": frags[1][None]}]           # a scene's pairs carry no viewpoints
    direct = register_fpfh(bare, eng, keypoints="iss", voxel_size=K.PAIR_VOXEL, hypotheses=1024, seed=0)[0]
    plain = register_fpfh(bare, eng, voxel_size=K.PAIR_VOXEL, hypotheses=1024, seed=0)[0]
    assert np.array_equal(_bits(np.asarray(edge[0][2], np.float32)), _bits(direct[0, 0]))
    assert not np.array_equal(_bits(direct), _bits(plain))
    with pytest.raises(ValueError):
        scene_edges_fpfh(frags, eng, keypoints="harris")
