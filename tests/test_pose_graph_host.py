"""The host rules of scene registration (deepsir_amd/pose_graph.py, metrics.info_rmse): no GPU.  The graphs built here are the
ones tests/test_gpu_pose_graph.py hands to the device."""
import numpy as np
import pytest

from deepsir_amd import metrics as M
from deepsir_amd import pose_graph as PG
from deepsir_amd.synth import POSE_GRAPH_RADIUS as RADIUS, make_pose_graph as make_graph, se3_inv as inv, se3_mul as mul, se3_random as pose

def outlier_graph():
    """12 nodes, 6 true loops, 3 false loops; 2 mrad / 5 mm noise on the true edges"""
    return make_graph(12, 77, loops=6, noise=(0.002, 0.005), start=(0.05, 0.05), false_edges=3)


def pose_err(X, Y):
    return max(np.abs(np.asarray(X) - np.asarray(Y)).max(), 0.0)


# ---------------------------------------------------------------------------------------------------------------------- information
def test_information_matrix_host_against_the_literal_rows():
    rng = np.random.default_rng(3)
    ref = rng.uniform(-2, 5, (257, 6)).astype(np.float32)
    idx = rng.integers(-1, 257, 300)
    A = PG.information_matrix_host(ref, idx)
    lit, mag = np.zeros((6, 6)), np.zeros((6, 6))
    for i in idx[idx >= 0]:
        x, y, z = (float(v) for v in ref[i, :3])
        for row in ([0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]):
            r = np.array(row)
            lit += np.outer(r, r)
            mag += np.abs(np.outer(r, r))
    n = int((idx >= 0).sum())
    bound = 2 * (n - 1) * 2.0 ** -53 * mag          # both sides are fp64 sums of the same terms in their own order
    assert n > 200 and (np.abs(A - lit) <= bound).all()
    assert np.array_equal(A, A.T) and A[3, 3] == n and (A[3:, 3:] == n * np.eye(3)).all()
    assert not PG.information_matrix_host(ref, np.full(10, -1)).any()


def test_line_process_weight_is_the_stated_product():
    info = np.zeros((3, 6, 6))
    info[:, 3, 3] = [100.0, 200.0, 400.0]
    assert PG.line_process_weight(info, [0, 1, 1], 0.1, preference=2.0) == pytest.approx(2.0 * 0.01 * 300.0)
    assert PG.line_process_weight(info, [0, 0, 0], 0.1) == 1.0


# ---------------------------------------------------------------------------------------------------------------------- optimize_host
@pytest.mark.parametrize("N,ref", [(2, 0), (7, 3), (12, 11)])
def test_noise_free_ring_recovers_the_generating_poses(N, ref):
    g, Xt, _ = make_graph(N, 10 + N, ref=ref)
    trace = []
    X, line, stats = PG.optimize_host(g, trace=trace)
    print(f"N={N}: F {stats[0]:.3e} -> {stats[1]:.3e} in {int(stats[2])} solves, status {int(stats[3])}, pose error {pose_err(X, Xt):.2e}")
    assert stats[3] == 0 and stats[2] < PG.MAX_ITER
    assert pose_err(X, Xt) < 1e-6          # the rule stops on a relative step of 1e-6 of a pose scale >= 1: no finer is promised
    assert X[ref].tobytes() == np.ascontiguousarray(g.X0, np.float64)[ref].tobytes()        # the fixed node is untouched
    assert all(b <= a for a, b in zip([stats[0]] + trace, trace))                           # F never rises over accepted steps
    assert stats[1] == (trace[-1] if trace else stats[0]) and (line > 0.99).all()


def test_wrong_loop_edges_are_switched_off():
    """Achieved on this graph (12 nodes, 11 odometry + 6 true loops + 3 false loops, mu = RADIUS^2 x 200): the smallest l of a true
    uncertain edge is 0.99, the largest l of a false one 2.2e-08 - the condition l_false < 0.25 < l_true holds with a wide gap."""
    g, Xt, false = outlier_graph()
    X, line, stats = PG.optimize_host(g)
    unc = np.asarray(g.uncertain).astype(bool)
    print(f"min true l {line[unc & ~false].min():.3g}, max false l {line[false].max():.3g}, solves {int(stats[2])}, status {int(stats[3])}, "
          f"pose error {pose_err(X, Xt):.3g}")
    assert (line[false] < PG.PRUNE_LINE).all() and (line[~false] > PG.PRUNE_LINE).all() and (line[~unc] == 1.0).all()
    assert stats[1] < stats[0] and pose_err(X, Xt) < 0.02


def test_status_codes_of_bad_graphs():
    g, _, _ = make_graph(7, 5)
    bad = PG.PoseGraph(g.X0, g.st, g.T, g.info.copy(), g.uncertain, g.mu, 0)
    bad.info[2, 1, 1] = np.nan
    X, line, st = PG.optimize_host(bad)
    assert st[3] == PG.ST_NON_FINITE and X.tobytes() == np.ascontiguousarray(g.X0).tobytes() and (line == 1).all()
    idx = PG.PoseGraph(g.X0, g.st.copy(), g.T, g.info, g.uncertain, g.mu, 0)
    idx.st[1, 1] = 7
    assert PG.optimize_host(idx)[2][3] == PG.ST_EDGE_INDEX
    flat = PG.PoseGraph(g.X0, g.st, g.T, np.zeros_like(g.info), g.uncertain, g.mu, 0)
    assert PG.optimize_host(flat)[2][3] == PG.ST_PIVOT
    one = PG.PoseGraph(g.X0[:1], np.zeros((0, 2), np.int32), np.zeros((0, 3, 4)), np.zeros((0, 6, 6)), np.zeros(0, np.uint8))
    X, line, st = PG.optimize_host(one)
    assert X.tobytes() == np.ascontiguousarray(g.X0[:1]).tobytes() and not st.any()


def test_refusals():
    g, _, _ = make_graph(7, 5)
    PG.pack_graphs([g])
    with pytest.raises(ValueError, match="disconnected"):
        PG.pack_graphs([PG.PoseGraph(g.X0, g.st[[0, 1, 3, 4, 5]], g.T[[0, 1, 3, 4, 5]], g.info[[0, 1, 3, 4, 5]], g.uncertain[[0, 1, 3, 4, 5]])])
    with pytest.raises(ValueError, match="disconnected"):
        PG.pack_graphs([PG.PoseGraph(g.X0, np.zeros((0, 2)), np.zeros((0, 3, 4)), np.zeros((0, 6, 6)), np.zeros(0))])
    with pytest.raises(ValueError, match="reference_node"):
        PG.pack_graphs([PG.PoseGraph(g.X0, g.st, g.T, g.info, g.uncertain, reference_node=7)])
    big, _, _ = make_graph(129, 1, loops=0)
    with pytest.raises(ValueError, match="DSIR_POSE_GRAPH_MAX_NODES"):
        PG.pack_graphs([g, big])
    p = PG.pack_graphs([g, make_graph(128, 1, loops=0)[0]])
    assert p["node_off"].tolist() == [0, 7, 135] and p["edge_off"].tolist() == [0, len(g.st), len(g.st) + 127]


# ---------------------------------------------------------------------------------------------------------------------- info_rmse
def test_info_rmse_hand_worked():
    T = pose(np.random.default_rng(1), 1.0, 1.0)
    info = np.diag([50.0, 50, 50, 7, 8, 9])
    p, ok = M.info_rmse(T, T, info)
    assert p == 0.0 and ok
    d = np.array([0.03, -0.04, 0.12])                                    # |d|^2 = 0.0169 <= 0.04
    Tp = mul(T, np.hstack([np.eye(3), d[:, None]]))                      # E = T_gt^-1 T_pred = the pure translation d
    p, ok = M.info_rmse(Tp, T, 123.0 * np.eye(6))
    assert p == pytest.approx(d @ d, rel=1e-12) and ok
    p, ok = M.info_rmse(mul(T, np.hstack([np.eye(3), 3 * d[:, None]])), T, 123.0 * np.eye(6))
    assert p == pytest.approx(9 * d @ d, rel=1e-12) and not ok
