"""ScanAlignmentLoss with its pose-error term (wt_pose_loss > 0, reference network/loss.py:830-842): dsir_align_loss_backward3.
Fixture: tests/golden/align_pose_loss_cases.npz, the imported reference's float32 autograd on five cases inside a conditioning cap
(tools/gen_golden_align_pose_loss.py).  Second yardstick and edge-rule oracle: tests/align_pose_host.py, the same chain in float64
under torch's autograd.  CPU: the restatement against the fixture, the lifted guard, the corner rules.  GPU: the kernel against both."""
import ctypes
import functools
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import align_pose_host as host
from conftest import GOLD


@functools.lru_cache(maxsize=None)
def _fixture():
    g = np.load(os.path.join(GOLD, "align_pose_loss_cases.npz"))
    return [{k[len(f"c{c}_"):]: g[k] for k in g.files if k.startswith(f"c{c}_")} for c in range(int(g["n_cases"]))]


@functools.lru_cache(maxsize=None)
def _restated(c):
    """(values, per-pair values, gradient, transforms) of case c from the float64 restatement; computed once, never written to."""
    d = _fixture()[c]
    w = d["weights"]
    out = host.loss_and_grad(d["src"], d["ref"], d["idx"], d["logits"], d["labels"], d["gt"], str(d["loss_type"]), w[0], w[1], w[2], w[3])
    for a in (out[2], out[3]):
        a.setflags(write=False)
    return out


def _want(d):
    names = [str(n) for n in d["loss_names"]]
    return dict(zip(names, d["loss_values"])), dict(zip(names, d["loss_per_pair"]))


def _kw(d, pose=True):
    w = d["weights"]
    return dict(loss_type=str(d["loss_type"]), wt_ptDist_loss=float(w[0]), wt_inlier_loss=float(w[1]), loss_discount_factor=float(w[3]),
                wt_pose_loss=float(w[2]) if pose else 0.0)


def _cu(d):
    f = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(dtype=dt).cuda() if dt else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return f(d["src"]), f(d["ref"]), f(d["idx"], torch.int32), f(d["logits"]), f(d["labels"]), f(d["gt"])


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_guard_is_lifted_and_bad_weights_are_rejected():
    from deepsir_amd.autograd import ScanAlignmentLoss
    from deepsir_amd.engine import EngineError, check_pose_weight
    f = ScanAlignmentLoss(None, SimpleNamespace(wt_pose_loss=0.5))            # raised NotImplementedError before the term existed
    assert f.wt_pose_loss == 0.5
    assert ScanAlignmentLoss(None, SimpleNamespace()).wt_pose_loss == 0.0     # the reference's default
    assert check_pose_weight(0.0) == 0.0 and check_pose_weight(2) == 2.0
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(EngineError, match="wt_pose_loss"):
            check_pose_weight(bad)


def test_fixture_meets_the_conditioning_cap():
    cases = _fixture()
    assert [(d["src"].shape[0], d["src"].shape[1], d["ref"].shape[1], d["idx"].shape[0], str(d["loss_type"]), *d["weights"][:3]) for d in cases] == \
        [(2, 600, 600, 3, "mae", 1, 1, 0.5), (3, 257, 300, 2, "mse", 1, 1, 2.0), (1, 100, 130, 1, "mae", 0, 0, 1.0),
         (1, 1500, 1700, 5, "mae", 1, 1, 1.0), (2, 320, 320, 8, "mae", 1, 0, 0.25)]
    for d in cases:
        assert d["err_r"].min() >= 0.05 and d["err_r"].max() <= math.pi - 0.05 and d["err_t"].min() >= 1e-2
        assert any(n.startswith("poseError_") for n in map(str, d["loss_names"]))


def test_restatement_matches_reference_autograd():
    """Bounds of tests/test_align_loss.py for the same chain on the CPU: values 1e-6 max(1, |v|), gradient 2e-4 of its scale.
    Measured on the five cases: values <= 5.7e-7, gradient <= 2.0e-6 of the scale, transforms <= 5.9e-7."""
    for c, d in enumerate(_fixture()):
        vals, _, grad, T = _restated(c)
        want, _ = _want(d)
        assert set(vals) == set(want)
        ev = max(abs(vals[k] - want[k]) / max(1.0, abs(want[k])) for k in want)
        scale = np.abs(d["grad_logits"]).max()
        eg = np.abs(grad - d["grad_logits"]).max() / scale
        print(f"[pose-loss host] case {c}: values {ev:.2e}, gradient {eg:.2e} of scale {scale:.2e}, transforms {np.abs(T - d['transforms']).max():.2e}")
        assert ev <= 1e-6, (c, ev)
        assert eg <= 2e-4, (c, eg)
        np.testing.assert_allclose(T, d["transforms"], atol=2e-6)


def _one_pair(gt_rot):
    """One pair whose prediction is the identity by construction (ref = src, identity correspondences, equal weights)."""
    rng = np.random.Generator(np.random.Philox(key=7))
    src = rng.uniform(-1, 1, (1, 64, 3))
    gt = np.concatenate([gt_rot, np.zeros((3, 1))], 1)[None]
    idx = np.arange(64)[None, None]
    return src, src.copy(), idx, np.zeros((1, 1, 64)), gt


def test_edge_rules():
    """|tc - t_gt| == 0: zero translation gradient; 1 - s^2 <= 0: value acos(clamp(s)), zero rotation gradient (include/dsir.h)."""
    for R, want_r in ((np.eye(3), 0.0), (np.diag([1.0, -1.0, -1.0]), math.pi)):
        # the rule itself, on exact poses
        gt = torch.from_numpy(np.concatenate([R, np.zeros((3, 1))], 1)[None])
        Tc = torch.cat([torch.eye(3, dtype=torch.float64), torch.zeros(3, 1, dtype=torch.float64)], 1)[None].requires_grad_(True)
        er, et = host.pose_errors(Tc, gt)
        (er.sum() + et.sum()).backward()
        assert float(er.detach()) == want_r and float(et.detach()) == 0.0
        assert torch.equal(Tc.grad, torch.zeros_like(Tc.grad))
        # and through the whole chain: finite values and gradients (the solve returns the identity to rounding only)
        src, ref, idx, logits, g = _one_pair(R)
        vals, pp, grad, T = host.loss_and_grad(src, ref, idx, logits, None, g, "mae", 1.0, 0.0, 1.0, 0.5)
        assert np.isfinite(list(vals.values())).all() and np.isfinite(grad).all()
        assert abs(vals["poseError_0"] - want_r) <= 1e-6 and abs(pp["poseError_0"][0] - want_r) <= 1e-6


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def eng():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    e = Engine(NetConfig(), 0, max_points=2048, max_pairs=4)
    yield e
    e.close()


@pytest.mark.gpu
def test_gpu_align_loss_backward3_matches_reference(eng):
    """Values 2e-6 max(1, |v|) and transforms 5e-6 against the fixture; gradient 2e-5 of its scale against the float64 restatement
    (the kernel's existing bound), and against the reference's float32 autograd that plus the restatement's own distance from it."""
    from deepsir_amd.engine import EngineError
    for c, d in enumerate(_fixture()):
        want, want_pp = _want(d)
        _, _, g64, _ = _restated(c)
        out = eng.align_loss_backward(*_cu(d), per_pair=True, **_kw(d))
        got, got_pp = out["losses"], out["losses_per_pair"]
        assert set(got) == set(want) and set(got_pp) == set(want_pp)
        ev = max(abs(got[k] - want[k]) / max(1.0, abs(want[k])) for k in want)
        ep = max(np.max(np.abs(got_pp[k] - want_pp[k]) / np.maximum(1.0, np.abs(want_pp[k]))) for k in want_pp)
        eT = np.abs(out["transforms"].cpu().numpy() - d["transforms"]).max()
        g = out["grad_logits"].cpu().numpy()
        scale = np.abs(d["grad_logits"]).max()
        e64, e32, host32 = np.abs(g - g64).max(), np.abs(g - d["grad_logits"]).max(), np.abs(g64 - d["grad_logits"]).max()
        print(f"[pose-loss] case {c}: total {got['total']:.6f} (reference {want['total']:.6f}); values {ev:.2e}, per pair {ep:.2e}, "
              f"transforms {eT:.2e}; gradient vs float64 {e64 / scale:.2e}, vs reference {e32 / scale:.2e} (restatement to reference "
              f"{host32 / scale:.2e}) of scale {scale:.2e}")
        assert ev <= 2e-6, (c, ev)
        assert ep <= 2e-6, (c, ep)
        assert eT <= 5e-6, (c, eT)
        assert e64 <= 2e-5 * scale, (c, e64 / scale)
        assert e32 <= host32 + 2e-5 * scale, (c, e32 / scale)
        # without the term: the reference's keys but the pose ones, and the older entry's result
        off = eng.align_loss_backward(*_cu(d), per_pair=True, **_kw(d, pose=False))
        no_pose = {k for k in want if not k.startswith("poseError_")}
        assert set(off["losses"]) == no_pose and set(off["losses_per_pair"]) == no_pose
    for bad in (-1.0, float("nan")):
        with pytest.raises(EngineError, match="wt_pose_loss"):
            eng.align_loss_backward(*_cu(_fixture()[2]), **{**_kw(_fixture()[2]), "wt_pose_loss": bad})
    # the C entry's own check
    s, r, ix, lg, lb, gt = _cu(_fixture()[2])
    grad = torch.empty_like(lg)
    for bad in (-1.0, float("nan"), float("inf")):
        rc = eng.lib.dsir_align_loss_backward3(eng.h, s.data_ptr(), r.data_ptr(), ix.data_ptr(), lg.data_ptr(), None, gt.data_ptr(), 1, 100, 130, 1,
                                               0, 1.0, 0.0, 0.5, bad, None, None, grad.data_ptr(), None)
        assert rc != 0 and b"wt_pose_loss" in eng.lib.dsir_last_error(eng.h)


@pytest.mark.gpu
def test_gpu_nothing_else_moved(eng):
    cases = _fixture()
    # weight 0 through the new entry == dsir_align_loss_backward2, bit for bit
    d = cases[0]
    s, r, ix, lg, lb, gt = _cu(d)
    n, P, J = lg.shape
    K = r.shape[1]
    res = []
    for entry, cols in ((eng.lib.dsir_align_loss_backward2, 2), (eng.lib.dsir_align_loss_backward3, 3)):
        T, grad = torch.zeros(P, n, 3, 4, device="cuda"), torch.zeros(n, P, J, device="cuda")
        losses, pp = (ctypes.c_double * (cols * n))(), (ctypes.c_double * (cols * n * P))()
        a = [eng.h, s.data_ptr(), r.data_ptr(), ix.data_ptr(), lg.data_ptr(), lb.data_ptr(), gt.data_ptr(), P, J, K, n, 0, 1.0, 1.0, 0.5]
        a += [0.0] if cols == 3 else []
        assert entry(*a, T.data_ptr(), losses, grad.data_ptr(), pp) == 0, eng.lib.dsir_last_error(eng.h)
        torch.cuda.synchronize()
        res.append((T.cpu().numpy(), grad.cpu().numpy(), np.array(losses).reshape(n, cols), np.array(pp).reshape(P, n, cols)))
    (T2, g2, l2, p2), (T3, g3, l3, p3) = res
    assert T2.tobytes() == T3.tobytes() and g2.tobytes() == g3.tobytes()
    assert l2.tobytes() == l3[:, :2].tobytes() and p2.tobytes() == np.ascontiguousarray(p3[:, :, :2]).tobytes()
    assert not l3[:, 2].any() and not p3[:, :, 2].any()
    # two runs with the term on: same bytes (no atomics; the pairs are added in pair order)
    runs = [eng.align_loss_backward(*_cu(cases[1]), per_pair=True, **_kw(cases[1])) for _ in range(2)]
    assert torch.equal(runs[0]["grad_logits"], runs[1]["grad_logits"]) and torch.equal(runs[0]["transforms"], runs[1]["transforms"])
    assert runs[0]["losses"] == runs[1]["losses"]
    assert all(np.array_equal(runs[0]["losses_per_pair"][k], runs[1]["losses_per_pair"][k]) for k in runs[0]["losses_per_pair"])
    # pair 0 alone.  Every term of a pair's workgroup is linear in 1 / P and reads no other pair, so a pair run alone gives
    # P x its gradient in the batch and the same per-pair values; with P = 2 the factor is a power of two, every product and sum
    # scales exactly, and the relation holds bit for bit (for other P it holds to rounding).
    both = eng.align_loss_backward(s, r, ix, lg, lb, gt, per_pair=True, **_kw(d))
    one = eng.align_loss_backward(s[:1].contiguous(), r[:1].contiguous(), ix[:, :1].contiguous(), lg[:, :1].contiguous(), lb[:, :1].contiguous(),
                                  gt[:1].contiguous(), per_pair=True, **_kw(d))
    assert P == 2
    assert torch.equal(one["grad_logits"][:, 0], 2.0 * both["grad_logits"][:, 0])
    assert torch.equal(one["transforms"][0], both["transforms"][0])
    for k, v in one["losses_per_pair"].items():
        assert v[0] == both["losses_per_pair"][k][0], k
        assert one["losses"][k] == v[0], k          # one pair: its own value is the batch mean


@pytest.mark.gpu
def test_gpu_edge_rules_give_finite_gradients(eng):
    """The two corner problems of test_edge_rules on the device: prediction = ground truth, and a pure 180 degree error."""
    for R, want_r in ((np.eye(3), 0.0), (np.diag([1.0, -1.0, -1.0]), math.pi)):
        src, ref, idx, logits, gt = _one_pair(R)
        f = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
        out = eng.align_loss_backward(f(src), f(ref), f(idx, torch.int32), f(logits), None, f(gt), per_pair=True, wt_ptDist_loss=1.0,
                                      wt_inlier_loss=0.0, wt_pose_loss=1.0)
        assert torch.isfinite(out["grad_logits"]).all()
        assert all(math.isfinite(v) for v in out["losses"].values())
        assert abs(out["losses"]["poseError_0"] - want_r) <= 1e-3        # the float32 solve returns the identity to rounding only
