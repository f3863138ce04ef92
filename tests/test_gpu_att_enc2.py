"""lfa.mlp2 of pyramid level 0 as a second product of the block's first attentive pooling (csrc/att_pool.hip, the producing variant of
att_pool16_kernel) instead of a row-streaming launch of its own (csrc/pw_stream.hip, loader S_UV): same product per element, same
sums per statistic - the same bits, in the layer and in everything downstream.  Level 1 keeps its own launch."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from att_enc2_dump import FEAT_LEN, ITERS, KEYS, PAIRS, POINTS  # noqa: E402


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """Both schedules' registrations of every case, one child process per setting (the switch is read once per process)."""
    d = tmp_path_factory.mktemp("att_enc2")
    outs = []
    # launches this small keep the two-launch schedule by default (the producing launch's grid is fixed by n and would not fill the
    # chip): DSIR_ATT_ENC2_MIN_BLOCKS=0 hands them to the producing variant all the same
    for name, extra in (("fused", {"DSIR_TUNING": "1", "DSIR_ATT_ENC2_MIN_BLOCKS": "0"}),
                        ("separate", {"DSIR_TUNING": "1", "DSIR_NO_ATT_ENC2": "1"})):
        out = str(d / f"{name}.npz")
        env = dict(os.environ, **extra)
        if name == "fused":
            env.pop("DSIR_NO_ATT_ENC2", None)
        else:
            env.pop("DSIR_ATT_ENC2_MIN_BLOCKS", None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "att_enc2_dump.py"), out], env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(np.load(out))
    return outs


# n = 1024: the smallest cloud the pyramid takes; 1027, 1100: n no multiple of level 0's four-point unit (padded tail units).
# n_iter = 1: no cache, arena buffers; 3: the cache is filled by the producing launch and read by iterations 1 and 2.
@pytest.mark.parametrize("feat_len", FEAT_LEN)
@pytest.mark.parametrize("n_iter", ITERS)
@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("n", POINTS)
def test_registration_is_the_same_bits_with_and_without_the_producing_pooling(dumps, n, pairs, n_iter, feat_len):
    a, b = dumps
    for k in KEYS:
        key = f"{feat_len}_{n}_{pairs}_{n_iter}_{k}"
        x, y = torch.from_numpy(a[key]), torch.from_numpy(b[key])
        assert x.numel() > 0 and torch.equal(x, y), f"{key} differs between the two schedules"


def test_the_fused_child_ran_the_producing_launch(dumps):
    """The comparison above means something only if the two children ran different schedules: the captured registration of the fused
    child holds two kernel nodes fewer - level 0's lfa.mlp2 launch of the feature pass and of the first inlier pass."""
    a, b = dumps
    assert int(a["census_kernels"]) > 0 and int(a["census_kernels"]) == int(b["census_kernels"]) - 2


@pytest.fixture(scope="module")
def probe_engine():
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    from deepsir_amd.synth import make_batch
    from deepsir_amd.weights import generate_state_dict, to_torch_state_dict
    cfg = NetConfig(feat_len=3)
    eng = Engine(cfg, 0, max_points=1027, max_pairs=2)
    eng.load_state_dict(to_torch_state_dict(generate_state_dict(cfg, 3)))
    b = make_batch(1027, [700, 701], 3)
    pts = torch.from_numpy(np.concatenate([b["points_src"], b["points_ref"][:1]], 0)).cuda()      # 3 clouds
    xyz, neigh, _, _ = eng.knn_pyramid(pts)
    yield eng, xyz, neigh
    eng.close()


@pytest.mark.parametrize("which", ["feat_extractor", "inlier_model"])
def test_layer_rows_and_statistics_bitwise_level0(probe_engine, which):
    """The layer itself, 3 clouds of 1027 points: every raw row of lfa.mlp2 and both statistics words (each as its two limbs) from the
    pooling launch equal those of the row-streaming launch."""
    eng, xyz, neigh = probe_engine
    rows_s, stats_s = eng.lfa_enc2_probe(which, 0, False, xyz, neigh, 1027)
    rows_f, stats_f = eng.lfa_enc2_probe(which, 0, True, xyz, neigh, 1027)
    assert rows_s.shape == (3, 16 * 1027, 8) and float(rows_s.abs().max()) > 0
    assert torch.equal(rows_f.view(torch.int32), rows_s.view(torch.int32))
    assert float(stats_s.abs().max()) > 0
    assert torch.equal(stats_f.view(torch.int64), stats_s.view(torch.int64))


def test_level1_keeps_its_own_launch(probe_engine):
    """Level 1's pooling has no producing variant: the probe says so instead of producing something else; the row-streaming launch
    still serves the level.  Why none: att_full_kernel<32, true> holds 160 VGPRs at its three-wave floor (168), and its LDS (53760 B x 3
    workgroups per CU) leaves 853 B.  Three forms of the variant were compiled, none without spill: accumulators in registers, weights
    from memory: 168 VGPRs, 6 spilled, 28 B scratch per lane; accumulators in the LDS tile's pad columns: 3 spilled, 16 B; that with a
    scheduling fence before the second product: 12 spilled, 20 B (profiles/README.md)."""
    from deepsir_amd.engine import EngineError
    eng, xyz, neigh = probe_engine
    rows_s, stats_s = eng.lfa_enc2_probe("feat_extractor", 1, False, xyz, neigh, 1027)
    assert rows_s.shape == (3, 16 * (1027 // 4), 32) and float(stats_s.abs().max()) > 0
    with pytest.raises(EngineError, match="does not produce"):
        eng.lfa_enc2_probe("feat_extractor", 1, True, xyz, neigh, 1027)
