"""dsir_pose_graph_optimize (csrc/pose_graph.hip) on the MI355X against pose_graph.optimize_host, on the graphs of
tests/test_pose_graph_host.py.  Sizes straddle the factorisation's 32-wide panel: N = 2 (6 unknowns), 7 (36: one past a panel),
12 (66), and once N = 128 (762, the largest accepted).

Tolerance of the poses: the device differs from the host rule only in summation and elimination order, so it is allowed 4 x the
host rule's own spread when every edge_T entry moves by +-1 fp32 ulp (as tests/test_gpu_icp_plane.py measures its tolerance).
Measured spread (max |X - X'| over 4 draws): N=2 2.6e-07, N=7 5.6e-07, N=12 7.6e-07, N=128 (4 solves, 2 draws) 1.1e-06;
the device was within 3e-15 of the host on all four.
`Engine.pose_graph_optimize` does not exist before this change, so every test fails without it."""
import numpy as np
import pytest

from deepsir_amd import pose_graph as PG
from deepsir_amd.synth import make_pose_graph as make_graph
from test_pose_graph_host import outlier_graph, pose_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), 0, max_points=1024, max_pairs=1)
    yield e
    e.close()


def _ulp_spread(g, max_iter, draws=4):
    """max |X - X'| of optimize_host when every edge_T entry is moved by +-1 fp32 ulp"""
    X = PG.optimize_host(g, max_iter)[0]
    rng = np.random.default_rng(0)
    T = np.asarray(g.T, np.float64)
    worst = 0.0
    for _ in range(draws):
        ulp = np.spacing(np.abs(T).astype(np.float32)).astype(np.float64)
        moved = PG.PoseGraph(g.X0, g.st, T + rng.choice([-1.0, 1.0], T.shape) * ulp, g.info, g.uncertain, g.mu, g.reference_node)
        worst = max(worst, pose_err(PG.optimize_host(moved, max_iter)[0], X))
    return worst


_CASES = {}


def _case(N):
    if N not in _CASES:
        if N == 128:
            g = make_graph(128, 9, loops=40, noise=(0.002, 0.005), start=(0.02, 0.02))[0]
            it = 4                                              # a few iterations: the host reference is the slow side
        else:
            g = make_graph(N, 20 + N, loops=4, noise=(0.002, 0.005), start=(0.1, 0.1), ref=N // 2)[0]
            it = PG.MAX_ITER
        _CASES[N] = (g, it, PG.optimize_host(g, it), _ulp_spread(g, it, 2 if N == 128 else 4))
    return _CASES[N]


@pytest.mark.parametrize("N", [2, 7, 12, 128])
def test_gpu_pose_graph_against_host(eng, N):
    g, it, (Xh, lh, sh), spread = _case(N)
    (X, line, st), = eng.pose_graph_optimize([g], max_iter=it)
    err = pose_err(X, Xh)
    print(f"N={N}: host F {sh[0]:.4e} -> {sh[1]:.4e} in {int(sh[2])} solves (status {int(sh[3])}); device F {st[0]:.4e} -> {st[1]:.4e} in "
          f"{int(st[2])} (status {int(st[3])}); |X - X_host| {err:.3e}, ulp spread {spread:.3e}, |line - line_host| {np.abs(line - lh).max():.3e}")
    assert X.dtype == np.float64 and X.shape == Xh.shape and line.shape == lh.shape
    assert st[3] == sh[3] and abs(st[2] - sh[2]) <= 1
    assert err <= 4 * spread
    assert st[0] == pytest.approx(sh[0], rel=1e-12) and st[1] <= st[0]
    ref = int(g.reference_node)
    assert X[ref].tobytes() == np.ascontiguousarray(g.X0, np.float64)[ref].tobytes()
    (X2, line2, st2), = eng.pose_graph_optimize([g], max_iter=it)                          # two runs, equal bytes
    assert X2.tobytes() == X.tobytes() and line2.tobytes() == line.tobytes() and st2.tobytes() == st.tobytes()


def test_gpu_pose_graph_switches_off_wrong_loops(eng):
    g, Xt, false = outlier_graph()
    (X, line, st), = eng.pose_graph_optimize([g])
    Xh, lh, sh = PG.optimize_host(g)
    unc = np.asarray(g.uncertain).astype(bool)
    print(f"device: min true l {line[unc & ~false].min():.3g}, max false l {line[false].max():.3g}, status {int(st[3])}")
    assert (line[false] < PG.PRUNE_LINE).all() and (line[~false] > PG.PRUNE_LINE).all() and (line[~unc] == 1.0).all()
    assert np.array_equal(line < PG.PRUNE_LINE, lh < PG.PRUNE_LINE) and st[3] == sh[3]
    assert pose_err(X, Xt) < 0.02


def test_gpu_pose_graph_batch_is_the_separate_calls(eng):
    a, b = _case(7)[0], _case(12)[0]
    both = eng.pose_graph_optimize([a, b])
    for got, g in zip(both, (a, b)):
        (X, line, st), = eng.pose_graph_optimize([g])
        assert got[0].tobytes() == X.tobytes() and got[1].tobytes() == line.tobytes() and got[2].tobytes() == st.tobytes()


def test_gpu_pose_graph_nan_stays_in_its_graph(eng):
    a, b = _case(7)[0], _case(12)[0]
    bad = PG.PoseGraph(a.X0, a.st, a.T, np.array(a.info, np.float64).copy(), a.uncertain, a.mu, a.reference_node)
    bad.info[3, 2, 4] = np.nan
    (Xa, la, sa), (Xb, lb, sb) = eng.pose_graph_optimize([bad, b])
    assert int(sa[3]) == PG.ST_NON_FINITE and Xa.tobytes() == np.ascontiguousarray(a.X0, np.float64).tobytes() and (la == 1.0).all()
    (X, line, st), = eng.pose_graph_optimize([b])
    assert Xb.tobytes() == X.tobytes() and lb.tobytes() == line.tobytes() and sb.tobytes() == st.tobytes()
    one = PG.PoseGraph(a.X0[:1], np.zeros((0, 2), np.int32), np.zeros((0, 3, 4)), np.zeros((0, 6, 6)), np.zeros(0, np.uint8))
    (X1, l1, s1), = eng.pose_graph_optimize([one])                                          # N = 1 returns its input
    assert X1.tobytes() == np.ascontiguousarray(a.X0[:1], np.float64).tobytes() and not s1.any() and len(l1) == 0


def test_gpu_pose_graph_refusals(eng):
    from deepsir_amd.engine import EngineError
    g = _case(7)[0]
    with pytest.raises((ValueError, EngineError), match="DSIR_POSE_GRAPH_MAX_NODES"):
        eng.pose_graph_optimize([make_graph(129, 1, loops=0)[0]])
    with pytest.raises((ValueError, EngineError), match="reference_node"):
        eng.pose_graph_optimize([PG.PoseGraph(g.X0, g.st, g.T, g.info, g.uncertain, g.mu, -1)])
    keep = [0, 1, 2, 3, 4]                                       # the chain 0 .. 5 alone: node 6 is cut off
    with pytest.raises((ValueError, EngineError), match="disconnected"):
        eng.pose_graph_optimize([PG.PoseGraph(g.X0, g.st[keep], g.T[keep], g.info[keep], g.uncertain[keep], g.mu, 0)])
    # the C entry refuses by itself, too: more nodes than it takes, without a launch
    import ctypes as C
    no, eo, rf = (np.array(v, np.int32) for v in ([0, 129], [0, 128], [0]))
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    assert eng.lib.dsir_pose_graph_scratch_bytes(1, p(no), p(eo), p(rf)) == 0
    assert eng.lib.dsir_pose_graph_optimize(eng.h, 1, p(no), p(eo), None, None, None, None, None, None, p(rf), 10, None, None, None, None) != 0
    assert b"DSIR_POSE_GRAPH_MAX_NODES" in eng.lib.dsir_last_error(eng.h)
