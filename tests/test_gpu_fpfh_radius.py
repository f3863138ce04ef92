"""FPFH over the cell-indexed radius lists (``Engine.radius_neighbors``, csrc/radius_nn.hip): the descriptors and poses of the brute-force
route byte for byte, and the open3d recipe (radius normals, hybrid lists) on a pair below the pyramid's floor."""
import numpy as np
import pytest
import torch

from deepsir_amd import fpfh as F
from deepsir_amd.metrics import THRESHOLDS, rte_rre

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    from deepsir_amd.weights import generate_state_dict
    cfg = NetConfig()
    e = Engine(cfg, max_points=2048, max_pairs=2)
    e.load_state_dict(generate_state_dict(cfg, 0))
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_same_descriptors_as_the_brute_force_lists(eng):
    pts = np.stack([np.concatenate(F.jittered_surface(1024, 41), 1), np.concatenate(F.jittered_surface(1024, 42), 1)])
    x = torch.from_numpy(pts).cuda()                                          # rows of xyz + normal
    eye = torch.eye(4)[:3].repeat(2, 1, 1).contiguous().cuda()
    brute = eng.radius_matches(x, x, eye, 0.25)
    grid = eng.radius_neighbors(x, 0.25)
    assert torch.equal(grid[0], brute[0]) and torch.equal(grid[1], brute[1]) and grid[1].numel() > 16 * 2048
    want, wflags = eng.fpfh(x, csr=brute)
    want, wflags = want.clone(), wflags.clone()
    got, flags = eng.fpfh(x, csr=grid)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(flags, wflags) and not bool(flags.any())
    capped = eng.radius_neighbors(x, 0.25, max_nn=8)                          # the hybrid list feeds the same entry
    assert int(torch.diff(capped[0]).max()) == 8
    d8, f8 = eng.fpfh(x, csr=capped)
    assert bool(torch.isfinite(d8).all()) and not torch.equal(d8, want)


def test_same_poses_as_the_brute_force_search(eng):
    from deepsir_amd.harness import register_fpfh
    pairs = [F.bumpy_pair(1), F.bumpy_pair(2)]                                # 2 pairs x 1024 points
    kw = dict(voxel_size=0.05, radius=0.25, hypotheses=1024, batch=2, num_reg=1, seed=0)
    brute, _ = register_fpfh(pairs, eng, **kw)
    named, _ = register_fpfh(pairs, eng, search="brute", **kw)
    grid, _ = register_fpfh(pairs, eng, search="grid", **kw)
    assert np.array_equal(_bits(brute), _bits(named)) and np.array_equal(_bits(brute), _bits(grid))
    for T, pr in zip(grid[:, 0], pairs):
        assert rte_rre(T, pr["transform_gt"][0], *THRESHOLDS["3DMatch"])[0] == 1.0
    for bad in (dict(search="tree"), dict(max_nn=10), dict(search="grid", max_nn=-1), dict(normal_max_nn=5)):
        with pytest.raises(ValueError):
            register_fpfh(pairs, eng, **{**kw, **bad})


def test_open3d_recipe_on_a_pair_below_the_pyramid_floor(eng):
    """600 points a side: the pyramid refuses the cloud, so the call was impossible before.  normal_radius = 2 voxel with max_nn 30,
    radius = 5 voxel with max_nn 100, voxel = 0.12 (the spacing of 600 points on [0, 3]^2).  The host rules (radius_neighbors_host ->
    ppf.estimate_normals(csr=) -> fpfh_host(csr=) -> mutual arg-min -> ransac_pair) recover this pair on the CPU: 600 mutual
    correspondences, RTE 1.5e-8, RRE 0.03 degrees."""
    from deepsir_amd.engine import EngineError
    from deepsir_amd.harness import register_fpfh
    pr = F.bumpy_pair(3, 600)
    vox = 0.12
    with pytest.raises(EngineError):
        register_fpfh([pr], eng, voxel_size=vox, radius=5 * vox, hypotheses=1024)          # today's path needs the pyramid
    pred, stats, corr = register_fpfh([pr], eng, voxel_size=vox, radius=5 * vox, max_nn=100, normal_radius=2 * vox, normal_max_nn=30,
                                      search="grid", hypotheses=1024, want_corr=True)
    T = pred[0, 0]
    assert pred.shape == (1, 1, 3, 4) and np.isfinite(pred).all() and np.isfinite(stats).all()
    succ, rte, rre = rte_rre(T, pr["transform_gt"][0], *THRESHOLDS["3DMatch"])
    print(f"600-point pair: {len(corr[0][0])} correspondences, RTE {rte:.3e}, RRE {rre:.3e}")
    assert succ == 1.0 and stats[0, 0] == 1.0
    assert np.abs(T[:, :3] @ T[:, :3].T - np.eye(3)).max() < 1e-5 and len(corr[0][0]) > 300
    assert not corr[0][1].any() and not corr[0][2].any()
    # two pairs with different viewpoints in one batch: the normals go cloud by cloud over slices of the batch CSR - the same bits
    pr2 = F.bumpy_pair(4, 600)
    both, _ = register_fpfh([pr, pr2], eng, voxel_size=vox, radius=5 * vox, max_nn=100, normal_radius=2 * vox, normal_max_nn=30,
                            search="grid", hypotheses=1024, batch=2)
    assert np.array_equal(_bits(both[0]), _bits(pred[0]))
    assert rte_rre(both[1, 0], pr2["transform_gt"][0], *THRESHOLDS["3DMatch"])[0] == 1.0


def test_csr_of_cloud_slices_a_batch_csr(eng):
    from deepsir_amd.harness import csr_of_cloud
    x = torch.from_numpy(np.stack([F.jittered_surface(300, 51)[0], F.jittered_surface(300, 52)[0], F.jittered_surface(300, 53)[0]])).cuda()
    batch = eng.radius_neighbors(x, 0.4)
    bounds = batch[0][::300].cpu().numpy()
    for b in range(3):
        alone = eng.radius_neighbors(x[b:b + 1].contiguous(), 0.4)
        for got in (csr_of_cloud(batch, b, 300), csr_of_cloud(batch, b, 300, bounds)):
            assert torch.equal(got[0], alone[0]) and torch.equal(got[1], alone[1]) and got[1].numel() > 300
