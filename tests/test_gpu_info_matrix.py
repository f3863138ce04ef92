"""dsir_information_matrix (csrc/info_matrix.hip) on the MI355X against the host rule of deepsir_amd/pose_graph.py: P = 4 pairs
(plain, no correspondence, non-finite rows on both sides, offset by 1e3 m), J = 300, K = 257, strides 3 and 6.  The entry and
`Engine.information_matrix` do not exist before this change, so every test fails without it."""
import math

import numpy as np
import pytest

from deepsir_amd import pose_graph as PG

pytestmark = pytest.mark.gpu
P, J, K, R = 4, 300, 257, 0.15


@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), 0, max_points=4096, max_pairs=4)
    yield e
    e.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _case(stride):
    rng = np.random.default_rng(41 + stride)
    ref = rng.uniform(0, 1.5, (P, K, stride)).astype(np.float32)
    src = np.stack([ref[p][rng.integers(0, K, J)] + rng.normal(0, 0.03, (J, stride)).astype(np.float32) for p in range(P)]).astype(np.float32)
    src[1, :, :3] += 50.0                                   # pair 1: nothing within the radius
    src[2, ::7, 0] = np.nan                                 # pair 2: non-finite rows on both sides
    src[2, 5::11, 2] = np.inf
    ref[2, ::5, 1] = np.nan
    ref[2, 3::9, 0] = -np.inf
    src[3, :, :3] += 1000.0                                 # pair 3: a kilometre from the origin
    ref[3, :, :3] += 1000.0
    T = np.tile(np.eye(3, 4, dtype=np.float32), (P, 1, 1))
    T[0, :, 3] = [0.01, -0.02, 0.005]
    return src, ref, T


def _run(eng, src, ref, T, search="brute"):
    info, cnt = eng.information_matrix(_dev(src), _dev(ref), _dev(T), R, search=search)
    return info.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("stride", [3, 6])
def test_gpu_information_matrix(eng, stride):
    src, ref, T = _case(stride)
    idx = eng.icp_correspondences(_dev(src), _dev(ref), _dev(T), R)[0].cpu().numpy()
    info, cnt = _run(eng, src, ref, T)
    assert info.dtype == np.float64 and info.shape == (P, 6, 6) and cnt.dtype == np.int32
    assert np.array_equal(cnt, (idx >= 0).sum(1))
    assert cnt[1] == 0 and not info[1].any() and info[1].tobytes() == bytes(288)
    assert cnt[0] > 100 and 0 < cnt[2] < J and cnt[3] > 100
    for p in range(P):
        host = PG.information_matrix_host(ref[p], idx[p])
        q = ref[p][idx[p][idx[p] >= 0], :3].astype(np.float64)
        n = len(q)
        assert np.isfinite(info[p]).all() and np.array_equal(info[p], info[p].T)          # exact symmetry
        # every entry against the exactly rounded sum of its terms (math.fsum), within (n - 1) 2^-53 sum |term|: the bound of a
        # floating-point sum of n terms in any order.  The terms of an entry are the products of the three rows' columns.
        worst = 0.0
        for a in range(6):
            for b in range(6):
                terms = []
                for x, y, z in q:
                    rows = ((0.0, z, -y, 1.0, 0.0, 0.0), (-z, 0.0, x, 0.0, 1.0, 0.0), (y, -x, 0.0, 0.0, 0.0, 1.0))
                    terms += [r[a] * r[b] for r in rows if r[a] != 0.0 and r[b] != 0.0]
                exact, mag = math.fsum(terms), math.fsum(abs(t) for t in terms)
                bound = max(n - 1, 0) * 2.0 ** -53 * mag
                assert abs(info[p, a, b] - exact) <= bound, (p, a, b, info[p, a, b], exact, bound)
                assert abs(host[a, b] - exact) <= bound
                worst = max(worst, abs(info[p, a, b] - exact) / bound if bound else 0.0)
        print(f"stride {stride} pair {p}: count {n}, worst |device - exact| / bound = {worst:.3g}")
    # the same bytes: two runs, the cell index, a pair alone
    again = _run(eng, src, ref, T)
    grid = _run(eng, src, ref, T, "grid")
    assert again[0].tobytes() == info.tobytes() and np.array_equal(again[1], cnt)
    assert grid[0].tobytes() == info.tobytes() and np.array_equal(grid[1], cnt)
    for p in range(P):
        one = _run(eng, src[p:p + 1], ref[p:p + 1], T[p:p + 1])
        assert one[0].tobytes() == info[p].tobytes() and one[1][0] == cnt[p]


def test_gpu_information_matrix_refusals(eng):
    src, ref, T = _case(3)
    from deepsir_amd.engine import EngineError
    with pytest.raises(ValueError):
        eng.information_matrix(_dev(src), _dev(ref), _dev(T), R, search="kd")
    with pytest.raises(EngineError):
        eng.information_matrix(_dev(src), _dev(ref), _dev(T), -1.0)
