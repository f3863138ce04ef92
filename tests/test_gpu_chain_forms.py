"""The two fused MLP kernels of the registration path - the aggregation chain and the per-point head - in their two forms
(fp16-split default, exact fp32): the claims their comments make about one another.

  * the fp32 forms are bit-identical to the layer-by-layer launches they replace (DSIR_NO_AGG / DSIR_NO_HEAD);
  * a point's chain does not depend on the blocking (64 or 128 rows per workgroup), in either form;
  * the split head stays within its bounds of the fp32 head at a ragged row count."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cu(a, dtype=None):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU-only hosts)")
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(torch.device("cuda", 0))


@pytest.mark.parametrize("pairs,points,iters", [(1, 1357, 2), (12, 1357, 2)])
def test_fp32_forms_equal_the_unfused_launches(tmp_path, pairs, points, iters):
    """The exact-fp32 chain and head (DSIR_AGG_F32) contract every layer in the k order of the kernel they replace: a registration
    through them equals, bit for bit, the one through the six + four separate launches (DSIR_NO_AGG=1 DSIR_NO_HEAD=1; read once per
    process, hence two processes).  1 x 1357: ragged rows, the 64-row chain, heads of 19 classes and of one logit;
    12 x 1357: 24 clouds x 11 blocks of 128 rows = 264 >= 256 workgroups, the 128-row chain."""
    outs = []
    for name, extra in (("fused", {}), ("unfused", {"DSIR_NO_AGG": "1", "DSIR_NO_HEAD": "1"})):
        out = str(tmp_path / f"{name}.npz")
        env = dict(os.environ, DSIR_TUNING="1", DSIR_AGG_F32="1", **extra)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "register_dump.py"), out, str(pairs), str(points), str(iters)],
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(np.load(out))
    a, b = outs
    for k in ("idx", "logits", "transforms"):
        assert np.array_equal(a[k], b[k]), f"{k} differs between the fp32 fused kernels and the unfused launches"


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("clouds,n", [(24, 1357), (8, 4100)])
def test_agg_chain_bits_do_not_depend_on_the_blocking(clouds, n, split):
    """ceil(n / 128) x clouds >= 256 workgroups selects 128 rows per workgroup, fewer select 64: cloud 0 of the large launch
    (24 x 11 = 8 x 33 = 264 workgroups) and cloud 0 alone (64-row workgroups) give the same descriptors, bit for bit."""
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    from deepsir_amd.weights import generate_state_dict
    assert (n + 127) // 128 * clouds >= 256 > (n + 127) // 128
    cfg = NetConfig(feat_len=3)
    eng = Engine(cfg, 0, max_points=max(n, 1024), max_pairs=(clouds + 1) // 2)
    eng.load_state_dict(generate_state_dict(cfg, 1))
    rng = np.random.Generator(np.random.Philox(key=n + clouds))
    xyz = cu(rng.uniform(0.0, 3.0, (clouds, n, 3)).astype(np.float32))
    feat = cu(rng.standard_normal((clouds, n, 64)).astype(np.float32))
    score = cu(rng.uniform(0, 1, (clouds, n)).astype(np.float32))
    eng.enable_agg_split(split)
    many = eng.aggregate(xyz, feat, score)[0].clone()
    one = eng.aggregate(xyz[:1].contiguous(), feat[:1].contiguous(), score[:1].contiguous())[0]
    assert torch.isfinite(many).all()
    assert torch.equal(many, one)
    eng.close()


@pytest.mark.parametrize("which", ["feat_extractor", "inlier_model"])
def test_head_split_matches_fp32_head_at_a_ragged_tail(which):
    """test_gpu_parity.py::test_head_split_matches_fp32_head at n = 1357 (85 row tiles, the last with 13 rows): the same
    relative bounds, 1e-5 of the scale of the feature and of the logits."""
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    from deepsir_amd.synth import make_pair
    from deepsir_amd.weights import generate_state_dict
    n = 1357
    cfg = NetConfig(feat_len=3)
    eng = Engine(cfg, 0, max_points=2048, max_pairs=1)
    eng.load_state_dict(generate_state_dict(cfg, 2))
    raw = make_pair(n, 31, 3)
    pts = cu(np.concatenate([raw["points_src"], raw["points_ref"]], 0))
    xyz, neigh, sub, interp = eng.knn_pyramid(pts)
    if which == "feat_extractor":
        feats = pts
    else:
        rng = np.random.Generator(np.random.Philox(key=n))
        feats = cu(rng.uniform(0, 3, (2, n, 6)).astype(np.float32))
    eng.enable_agg_split(False)
    f0, l0 = eng.randla_forward(which, feats, xyz, neigh, sub, interp)
    f0, l0 = f0.clone(), l0.clone()
    eng.enable_agg_split(True)
    f1, l1 = eng.randla_forward(which, feats, xyz, neigh, sub, interp)
    ef = float((f1.double() - f0.double()).abs().max() / f0.double().abs().max())
    el = float((l1.double() - l0.double()).abs().max() / l0.double().abs().max())
    print(f"[head-split] n {n} {which}: feat rel err {ef:.2e} (scale {float(f0.abs().max()):.2f}), logits rel err {el:.2e} (scale {float(l0.abs().max()):.2f})")
    assert torch.isfinite(f1).all() and torch.isfinite(l1).all()
    assert ef <= 1e-5 and el <= 1e-5
    assert not torch.equal(l0, l1)            # different arithmetic: identical bits would mean the switch is dead
    eng.close()
