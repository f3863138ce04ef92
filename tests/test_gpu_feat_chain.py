"""mlp_feat (64 -> 64 -> 128 -> 64) of Network.aggregation in one launch (csrc/feat_chain.hip) instead of three point-wise launches
(csrc/pw_stream.hip twice, csrc/pw_tile.hip): every element is the same chain of operations, so the layer - and every descriptor,
arg-min and transform downstream - is the same bits.  All comparisons are torch.equal."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from feat_chain_dump import KEYS  # noqa: E402

# fewer rows than a 16-row tile, a tile's edges, ragged tails, more tiles than one workgroup's eight waves (257 x 3 clouds: 51 tiles);
# 337: above the 320 rows up to which the three launches' last layer is pw_tile_small_kernel - there it is pw_tile_kernel, as at the
# production shapes.  The launch's own grid gives every wave ONE tile at all these sizes (a workgroup per 8 tiles, up to one per CU:
# a second tile per wave needs 32768 rows): the steady-state walk is what the capped cases below run.
SIZES = (1, 15, 16, 17, 33, 257, 337)
NMAX = max(SIZES)


@pytest.fixture(scope="module", params=["plain", "separated"])
def probe(request):
    """An engine per weight variant and the inputs of every case: 4 clouds of NMAX rows, cut down per case."""
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    from deepsir_amd.weights import generate_state_dict, to_torch_state_dict
    cfg = NetConfig(feat_len=3)
    eng = Engine(cfg, 0, max_points=1024, max_pairs=2)
    eng.load_state_dict(to_torch_state_dict(generate_state_dict(cfg, 3, request.param)))
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4, NMAX, 64, generator=g)
    inputs = {"normal": x, "negative": -x.abs() - 1e-3, "scaled": x * 1e3}
    yield eng, {k: v.cuda() for k, v in inputs.items()}
    eng.close()


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("kind", ["normal", "negative", "scaled"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("clouds", [1, 3])
def test_fused_launch_is_the_three_launches_bit_for_bit(probe, clouds, n, kind):
    eng, inputs = probe
    x = inputs[kind][:clouds, :n].contiguous()
    ref = eng.mlp_feat_probe(x, 0)
    got = eng.mlp_feat_probe(x, 1)
    assert ref.shape == (clouds, n, 64) and bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
    assert torch.equal(_bits(got), _bits(ref))


@pytest.mark.parametrize("n", [257, 337])
@pytest.mark.parametrize("clouds", [1, 3])
@pytest.mark.parametrize("cap", [1, 2])
def test_a_wave_walks_several_tiles(probe, cap, clouds, n):
    """The grid capped at one or two workgroups (dsir_mlp_feat_probe, max_workgroups): 17 - 66 tiles on 8 or 16 waves, so every wave
    runs the loop two to nine times - the stride walk, the prefetched next rows, the wave's LDS tile reused, clouds changing between a
    wave's tiles and a ragged last tile per cloud - against the three launches."""
    eng, inputs = probe
    x = inputs["normal"][:clouds, :n].contiguous()
    ref = eng.mlp_feat_probe(x, 0)
    got = eng.mlp_feat_probe(x, 1, max_workgroups=cap)
    assert float(ref.abs().max()) > 0
    assert torch.equal(_bits(got), _bits(ref))


@pytest.mark.parametrize("n", [257, 337])
@pytest.mark.parametrize("cap", [1, 2])
def test_two_output_launch_with_several_tiles_per_wave(probe, cap, n):
    """The two-output form under the same cap: 4 clouds, 68 or 88 tiles dealt round-robin to 8 or 16 waves, so every wave's walk
    crosses from the first output base to the second - against the three launches on all four clouds."""
    eng, inputs = probe
    x = inputs["normal"][:, :n].contiguous()
    ref = eng.mlp_feat_probe(x, 0)
    got = eng.mlp_feat_probe(x, 2, max_workgroups=cap)
    assert torch.equal(_bits(got), _bits(ref))


@pytest.mark.parametrize("n", [17, 257])
def test_two_output_launch_gives_each_side_its_own_bytes(probe, n):
    """P = 2: src and ref sides in one launch over 4 clouds with two output bases, against one fused launch per side."""
    eng, inputs = probe
    x = inputs["normal"][:, :n].contiguous()
    both = eng.mlp_feat_probe(x, 2)
    for side in (0, 1):
        alone = eng.mlp_feat_probe(x[2 * side:2 * side + 2].contiguous(), 1)
        assert float(alone.abs().max()) > 0
        assert torch.equal(_bits(both[2 * side:2 * side + 2]), _bits(alone))


@pytest.mark.parametrize("n", [33, 337])
def test_exact_fp32_switch_follows_the_unfused_last_layer(probe, n):
    """dsir_enable_agg_split(0): the three launches run the last layer in exact fp32 (pw_tile.hip's k order; n = 337: pw_tile_kernel,
    not the small-M kernel) - so does the fused one, on its own grid and with several tiles per wave."""
    eng, inputs = probe
    x = inputs["normal"][:3, :n].contiguous()
    split = eng.mlp_feat_probe(x, 0)
    eng.enable_agg_split(False)
    try:
        ref = eng.mlp_feat_probe(x, 0)
        got = eng.mlp_feat_probe(x, 1)
        capped = eng.mlp_feat_probe(x, 1, max_workgroups=1)
    finally:
        eng.enable_agg_split(True)
    assert torch.equal(_bits(got), _bits(ref))
    assert torch.equal(_bits(capped), _bits(ref))
    assert not torch.equal(_bits(ref), _bits(split)), "the switch did not change the last layer's arithmetic"


@pytest.fixture(scope="module")
def whole_path(tmp_path_factory):
    """The same registration in three fresh child processes (the switches are read once per process): mlp_feat fused, as three
    launches, and under the default rule."""
    d = tmp_path_factory.mktemp("feat_chain")
    outs = []
    # a registration this small keeps the three launches by default (csrc/schedule.hip, feat_chain_wanted):
    # DSIR_FEAT_CHAIN_MIN_BLOCKS=0 hands it to the fused launch all the same
    for name, extra in (("fused", {"DSIR_TUNING": "1", "DSIR_FEAT_CHAIN_MIN_BLOCKS": "0"}),
                        ("unfused", {"DSIR_TUNING": "1", "DSIR_NO_FEAT_CHAIN": "1"}),
                        ("default", {})):
        out = str(d / f"{name}.npz")
        env = {k: v for k, v in os.environ.items() if k not in ("DSIR_TUNING", "DSIR_NO_FEAT_CHAIN", "DSIR_FEAT_CHAIN_MIN_BLOCKS")}
        env.update(extra)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "feat_chain_dump.py"), out], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(np.load(out))
    return outs


def test_registration_is_the_same_bits_with_and_without_the_fused_launch(whole_path):
    """2 pairs x 257 points, 2 iterations: transforms, idx and both sides' descriptors."""
    a, b, c = whole_path
    for k in KEYS:
        x, y, z = torch.from_numpy(a[k]), torch.from_numpy(b[k]), torch.from_numpy(c[k])
        assert x.numel() > 0 and torch.equal(x, y) and torch.equal(z, y), f"{k} differs between the schedules"


def test_the_children_ran_different_schedules(whole_path):
    """The comparison means something only if the children ran different schedules: the captured registration of the fused child
    holds five kernel nodes fewer - one launch for both sides instead of three per side.  The default rule leaves a registration of
    this size on the three launches."""
    a, b, c = whole_path
    assert int(a["census_kernels"]) > 0 and int(a["census_kernels"]) == int(b["census_kernels"]) - 5
    assert int(c["census_kernels"]) == int(b["census_kernels"])
