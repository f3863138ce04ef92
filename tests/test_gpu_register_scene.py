"""harness.register_scene on the MI355X: one synthetic cloud of deepsir_amd.synth cut into 6 overlapping fragments (slabs along x of
about 1500 points) with known poses; candidate edges (i, i+1) certain and (i, i+2) uncertain are the ground truth perturbed by
2 degrees / 2 cm, plus two uncertain edges with unrelated transforms.  The cloud has empty strips, wider than the correspondence
radius, at the planes the slabs are cut at: a source point then has either its own copy in the other fragment or nothing within
the radius, so the true pose is a fixed point of the ICP and the pair poses are consistent up to fp32 rounding - which is what lets
the optimised poses be held to "no worse than the ICP pose by more than the ulp spread".  Nothing here exists before this change."""
import numpy as np
import pytest

from deepsir_amd import harness as H
from deepsir_amd import pose_graph as PG
from deepsir_amd.metrics import THRESHOLDS, rte_rre
from deepsir_amd.synth import make_pair, se3_inv as inv, se3_mul as mul, se3_random as pose

pytestmark = pytest.mark.gpu
VOXEL = 0.03                 # correspondence radius 2 x VOXEL = 0.06 m
STEP, WIDTH, STRIP = 0.3, 1.2, 0.07


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    from deepsir_amd.weights import generate_state_dict
    cfg = NetConfig()
    e = Engine(cfg, 0, max_points=2048, max_pairs=1)
    e.load_state_dict(generate_state_dict(cfg, 0))
    yield e
    e.close()


def _scene():
    rng = np.random.default_rng(5)
    cloud = make_pair(4900, 11)["points_ref"][0, :, :3].astype(np.float64)           # uniform in the 3 m room
    cloud = cloud[np.abs(cloud[:, 0] / STEP - np.round(cloud[:, 0] / STEP)) * STEP > STRIP / 2]   # empty strips at the cut planes
    X = np.stack([np.eye(3, 4)] + [pose(rng, 1.0, 1.0) for _ in range(5)])           # fragment -> scene
    frags = []
    for i in range(6):
        p = cloud[(cloud[:, 0] >= STEP * i) & (cloud[:, 0] <= STEP * i + WIDTH)]
        frags.append(((p - X[i][:, 3]) @ X[i][:, :3]).astype(np.float32))           # X_i^-1 p
    gt = {(s, t): mul(inv(X[t]), X[s]) for s in range(6) for t in range(s + 1, 6)}
    edges = [(s, t, mul(pose(rng, np.deg2rad(2.0), 0.02), gt[(s, t)]), t != s + 1) for s in range(6) for t in (s + 1, s + 2) if t < 6]
    false = [(0, 4, pose(rng, 2.5, 1.0), True), (1, 5, pose(rng, 2.5, 1.0), True)]
    return frags, X, gt, edges + false, len(edges)


def test_gpu_register_scene(eng):
    frags, Xgt, gt, edges, n_true = _scene()
    assert all(1300 < len(f) < 1700 for f in frags)
    res = H.register_scene(frags, eng, edges, voxel_size=VOXEL)
    rows = res["edges"]
    for r in rows:
        print(f"edge {r['s']}->{r['t']} uncertain {int(r['uncertain'])} count {r['count']} l {r['line']:.3g} dropped {r['dropped']}")
    print("stats", [s.tolist() for s in res["stats"]], H.summarize_scene(res, gt))
    assert all(r["dropped"] in ("overlap", "line") for r in rows[n_true:])            # both false edges go
    assert all(r["dropped"] is None for r in rows[:n_true])                          # no true edge goes
    assert res["X"][0].tobytes() == np.eye(3, 4).tobytes()
    keep = [r for r in rows if r["dropped"] is None]
    # the spread of tests/test_gpu_pose_graph.py for this scene: the host rule of the graph stage - poses chained from the edges, then
    # optimize_host - when every edge_T entry moves by +-1 fp32 ulp (the ICP poses are fp32 numbers: that is their own rounding)
    def host_stage(Ts):
        X0 = H._chain_poses(6, [(r["s"], r["t"], T, r["uncertain"]) for r, T in zip(keep, Ts)], 0)
        g = PG.PoseGraph(X0, [(r["s"], r["t"]) for r in keep], Ts, [r["info"] for r in keep], [r["uncertain"] for r in keep],
                         PG.line_process_weight([r["info"] for r in keep], [r["uncertain"] for r in keep], 2 * VOXEL))
        return PG.optimize_host(g)[0]

    Ts = np.array([r["T"] for r in keep])
    base, rng, spread = host_stage(Ts), np.random.default_rng(0), 0.0
    for _ in range(4):
        ulp = np.spacing(np.abs(Ts).astype(np.float32)).astype(np.float64)
        spread = max(spread, np.abs(host_stage(Ts + rng.choice([-1.0, 1.0], Ts.shape) * ulp) - base).max())
    assert np.abs(res["X"] - base).max() <= 4 * spread                                    # the device stage against the host stage
    rte_t, rre_t = THRESHOLDS["3DMatch"]
    for r in rows[:n_true]:
        T_gt = gt[(r["s"], r["t"])]
        ok, rte, rre = rte_rre(H.implied_pose(res["X"], r["s"], r["t"]), T_gt, rte_t, rre_t)
        rte_icp = rte_rre(r["T"], T_gt, rte_t, rre_t)[1]
        print(f"edge {r['s']}->{r['t']}: implied RTE {rte:.3e} RRE {rre:.3e} deg, ICP RTE {rte_icp:.3e}, spread {spread:.3e}")
        assert ok and rte <= rte_icp + spread
    s = H.summarize_scene(res, gt)
    assert s["dropped_overlap"] + s["dropped_line"] == 2 and s["recall_optimized"] == 1.0


def test_gpu_scene_edges_fpfh_table(eng):
    frags = _scene()[0]
    table = H.scene_edges_fpfh(frags[:2], eng, voxel_size=VOXEL, hypotheses=256)             # two fragments, all pairs: one certain edge
    assert [(s, t, u) for s, t, _, u in table] == [(0, 1, False)]
    table = H.scene_edges_fpfh([frags[0], frags[2]], eng, pairs=[(1, 0)], voxel_size=VOXEL, hypotheses=256)   # a given list: t != s + 1
    assert [(s, t, u) for s, t, _, u in table] == [(1, 0, True)]
    assert all(T.shape == (3, 4) and T.dtype == np.float64 for _, _, T, _ in table)
