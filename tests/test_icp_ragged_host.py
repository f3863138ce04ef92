"""ICP and edge information on batches of clouds of unequal sizes, the host side: ``harness.pad_clouds``, the batching plan of
``register_scene`` (``harness.scene_batches``, a pure function), and the argument checks of ``Engine.icp_refine``,
``icp_correspondences`` and ``information_matrix`` for ``counts_src`` / ``counts_ref``.  Those checks must fire before any library
call, so they are exercised on an Engine whose library raises on every access.  No GPU."""
import numpy as np
import pytest
import torch

from deepsir_amd import harness as H
from deepsir_amd.engine import Engine, pair_counts


# ------------------------------------------------------------------ pad_clouds
@pytest.mark.parametrize("stride", [3, 6])
def test_pad_clouds_shapes_counts_and_nan_padding(stride):
    rng = np.random.default_rng(stride)
    sizes = [5, 1, 9, 9, 0, 3]
    clouds = [rng.standard_normal((n, stride)).astype(np.float32) for n in sizes]
    out, counts = H.pad_clouds(clouds)
    assert tuple(out.shape) == (len(sizes), 9, stride) and out.dtype == torch.float32 and out.is_contiguous()
    assert counts.dtype == torch.int32 and counts.tolist() == sizes
    for i, (c, n) in enumerate(zip(clouds, sizes)):
        assert out[i, :n].numpy().tobytes() == c.tobytes()                     # the rows, bit for bit
        assert torch.isnan(out[i, n:]).all()                                   # every padding value is NaN, all columns
    t_out, t_counts = H.pad_clouds([torch.from_numpy(c) for c in clouds])      # tensors in, the same out
    assert t_out.numpy().tobytes() == out.numpy().tobytes() and t_counts.tolist() == sizes


def test_pad_clouds_equal_sizes_have_no_padding_and_empty_input_is_refused():
    a = np.arange(12, dtype=np.float32).reshape(4, 3)
    out, counts = H.pad_clouds([a, a + 1])
    assert tuple(out.shape) == (2, 4, 3) and not torch.isnan(out).any() and counts.tolist() == [4, 4]
    out, counts = H.pad_clouds([np.zeros((0, 3), np.float32)])                 # capacity is at least one row: the C ABI refuses 0
    assert tuple(out.shape) == (1, 1, 3) and counts.tolist() == [0] and torch.isnan(out).all()
    with pytest.raises(ValueError):
        H.pad_clouds([])
    with pytest.raises(ValueError):
        H.pad_clouds([np.zeros((2, 3), np.float32), np.zeros((2, 6), np.float32)])


# ------------------------------------------------------------------ the batching plan
@pytest.mark.parametrize("batch", [1, 2, 4, 7, 15, 100])
def test_scene_batches_cover_every_edge_once_in_stable_size_order(batch):
    rng = np.random.default_rng(11)
    sizes = [(int(a), int(b)) for a, b in rng.integers(1, 6, (15, 2))]         # few distinct sums: ties are certain
    plan = H.scene_batches(sizes, batch)
    flat = [k for kb in plan for k in kb]
    assert sorted(flat) == list(range(15))                                     # every edge in exactly one batch
    assert all(len(kb) == batch for kb in plan[:-1]) and 1 <= len(plan[-1]) <= batch and len(plan) == -(-15 // batch)
    key = [sizes[k][0] + sizes[k][1] for k in flat]
    assert key == sorted(key)                                                  # ascending n_s + n_t ..
    assert all(a < b for a, b, ka, kb_ in zip(flat, flat[1:], key, key[1:]) if ka == kb_)   # .. and input order among equals (stable)
    assert len({k for k in key}) < 15                                          # the ties the line above speaks of exist


def test_scene_batches_edge_cases():
    assert H.scene_batches([], 4) == []
    assert H.scene_batches([(3, 3)], 4) == [[0]]
    assert H.scene_batches([(9, 9), (1, 1), (5, 5)], 2) == [[1, 2], [0]]
    with pytest.raises(ValueError):
        H.scene_batches([(1, 1)], 0)


# ------------------------------------------------------------------ the Engine methods' argument checks, before any library call
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name}) before the arguments were checked")


@pytest.fixture()
def eng():
    e = Engine.__new__(Engine)                                                 # no context, no library: only the checks can run
    e.lib = _NoLibrary()
    e.h = None
    e.device = torch.device("cpu")
    return e


P, J, K = 3, 5, 7
_CALLS = {
    "icp_refine": lambda e, s, **kw: e.icp_refine(torch.zeros(P, J, s), torch.zeros(P, K, s), torch.zeros(P, 3, 4), 0.1, **kw),
    "icp_correspondences": lambda e, s, **kw: e.icp_correspondences(torch.zeros(P, J, s), torch.zeros(P, K, s), torch.zeros(P, 3, 4), 0.1, **kw),
    "information_matrix": lambda e, s, **kw: e.information_matrix(torch.zeros(P, J, s), torch.zeros(P, K, s), torch.zeros(P, 3, 4), 0.1, **kw),
}
_BAD = [
    dict(counts_src=[1, 2, J + 1]),                                            # above the capacity
    dict(counts_src=[-1, 2, 3]),                                               # negative
    dict(counts_ref=[1, K + 1, 0]),
    dict(counts_ref=[0, 0, -2]),
    dict(counts_src=[1, 2]),                                                   # not one per pair
    dict(counts_ref=[[1, 2, 3]]),
    dict(counts_src=[1.0, 2.0, 3.0]),                                          # not integers
    dict(counts_src=torch.tensor([1, 2, J + 1], dtype=torch.int32)),           # a tensor is checked as well
    dict(counts_src=[1, 2, 3], counts_ref=np.array([1, 2, K + 1])),
]


@pytest.mark.parametrize("method", sorted(_CALLS))
@pytest.mark.parametrize("bad", _BAD)
def test_bad_counts_are_a_value_error_before_any_launch(eng, method, bad):
    with pytest.raises(ValueError, match="counts_(src|ref)"):
        _CALLS[method](eng, 3, **bad)


@pytest.mark.parametrize("method", sorted(_CALLS))
def test_good_counts_pass_the_checks(eng, method):
    """the boundary values 0 and the capacity are accepted: the call then goes on to the tensor checks (EngineError: no CUDA
    tensor here), not to a ValueError"""
    from deepsir_amd.engine import EngineError
    with pytest.raises(EngineError):
        _CALLS[method](eng, 3, counts_src=[0, J, 1], counts_ref=torch.tensor([K, 0, 1], dtype=torch.int32))


def test_plane_with_counts_needs_normals(eng):
    with pytest.raises(ValueError, match="normals"):                           # the dense pyramid cannot estimate them: say so
        _CALLS["icp_refine"](eng, 3, estimator="plane", counts_src=[1, 2, 3], counts_ref=[1, 2, 3])
    with pytest.raises(ValueError, match="normals"):
        _CALLS["icp_refine"](eng, 3, estimator="plane", counts_ref=[1, 2, 3])
    from deepsir_amd.engine import EngineError
    with pytest.raises(EngineError):                                           # rows that carry normals pass this check ..
        _CALLS["icp_refine"](eng, 6, estimator="plane", counts_ref=[1, 2, 3])
    with pytest.raises(EngineError):                                           # .. and so do given normals
        eng.icp_refine(torch.zeros(P, J, 3), torch.zeros(P, K, 3), torch.zeros(P, 3, 4), 0.1, estimator="plane",
                       normals_ref=torch.zeros(P, K, 3), counts_ref=[1, 2, 3])


def test_pair_counts_returns_int32_host_array_or_none():
    assert pair_counts(None, 3, 5, "counts_src") is None
    a = pair_counts((0, 5, 2), 3, 5, "counts_src")
    assert a.dtype == np.int32 and a.tolist() == [0, 5, 2] and a.flags["C_CONTIGUOUS"]
    assert pair_counts(torch.tensor([1, 2, 3]), 3, 5, "counts_ref").dtype == np.int32     # int64 in, int32 out
