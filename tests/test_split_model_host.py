"""No GPU: what the fp16 operand split (csrc/split_f16.h) promises on paper, and the conditions under which the tolerances of
tests/test_gpu_split_magnitudes.py mean something.  The split itself is dsir_split_f16, the host entry of the library."""
import numpy as np
import pytest
import torch

import split_cases as sc

SCALES = (0, -6, -10, -14, 10)


@pytest.mark.parametrize("K", [32, 64, 256])
@pytest.mark.parametrize("e", SCALES)
@pytest.mark.parametrize("side", ["weights", "activations"])
def test_emulated_split_contraction_stays_under_its_bound(K, e, side):
    """al.bh + ah.bl + ah.bh on the parts of dsir_split_f16, summed in float64, against the float64 dot product of the fp32
    operands: within B(a, b) for every row, at every operand scale."""
    a, w = sc.dot_operands(K, 2000, 1)
    if side == "weights":
        w = sc._mul(w, e)
    else:
        a = sc._mul(a, e)
    assert np.abs(a).max() <= 65504 and np.abs(w).max() <= 65504
    err = np.abs(sc.split_dot(a, w[None]) - (a.astype(np.float64) * w.astype(np.float64)).sum(-1))
    B = sc.split_bound(a, w[None])
    mag = np.linalg.norm(a.astype(np.float64), axis=1) * np.linalg.norm(w.astype(np.float64))
    print(f"[split-bound] K {K} {side} x 2^{e}: worst err {float((err / mag).max()):.2e} |a||w|, worst err / B {float((err / B).max()):.3f}")
    assert (err <= B).all()


def test_split_error_grows_as_the_operand_shrinks():
    """What "fp32 accuracy" does and does not mean for the raw rule: at weights x 2^-10 (K = 256, activations ~ N(0, 1)) the low
    part is sub-normal and the split's worst error is more than 16 x that of a plain fp32 dot product on the same operands;
    at x 1 the two are within that factor of each other."""
    a, w = sc.dot_operands(256, 2000, 2)
    out = {}
    for e in (0, -10):
        ws = sc._mul(w, e)
        exact = (a.astype(np.float64) * ws.astype(np.float64)).sum(-1)
        mag = np.linalg.norm(a.astype(np.float64), axis=1) * np.linalg.norm(ws.astype(np.float64))
        es = float((np.abs(sc.split_dot(a, ws[None]) - exact) / mag).max())
        ef = float((np.abs(sc.fp32_dot(a, ws[None]).astype(np.float64) - exact) / mag).max())
        print(f"[split-vs-fp32] weights x 2^{e}: split {es:.2e}, fp32 dot {ef:.2e} (of |a||w|)")
        out[e] = (es, ef)
    assert out[-10][0] > 16 * out[-10][1]
    assert out[0][0] <= 16 * out[0][1]


# ------------------------------------------------------------------ the fp32 oracle has headroom at every GPU case
def _headroom(got32, ref64, tol, what):
    r = sc.worst_ratio(got32, ref64, tol)
    print(f"[oracle-headroom] {what}: fp32 oracle at {r:.3f} of the tolerance")
    assert r <= 0.1, what


@pytest.mark.parametrize("kind,e", [(k, e) for k in sc.AGG_KINDS for e in sc.AGG_E] + [sc.RANGE_END])
def test_fp32_oracle_headroom_aggregation(kind, e):
    """Every rescaled dict of the aggregation cases (the range end included): the fp32 OracleNet within a tenth of the
    descriptor tolerance of the float64 OracleNet.  No exponent had to be dropped."""
    for n in sc.AGG_N if (kind, e) != sc.RANGE_END else (257,):
        got = sc.oracle_aggregate(sc.agg_dict(kind, e), sc.agg_inputs(n), torch.float32)
        _headroom(got, sc.ref_aggregate(kind, e, n), sc.DESC_TOL, f"{kind} 2^{e} n {n}")


@pytest.mark.parametrize("feat_e", sc.ACT_FEAT_E)
def test_fp32_oracle_headroom_activations(feat_e):
    got = sc.oracle_aggregate(sc.base_sd(), sc.act_inputs(feat_e), torch.float32)
    _headroom(got, sc.ref_aggregate("act", 0, 257, feat_e), sc.DESC_TOL, f"feat0 x 2^{feat_e}")


@pytest.mark.parametrize("kind,e", [("gn", e) for e in sc.ENC_GN_E] + [("fc", e) for e in sc.ENC_FC_E] + [("head", e) for e in sc.HEAD_E])
@pytest.mark.parametrize("which", sc.NETS)
def test_fp32_oracle_headroom_encoder(which, kind, e):
    """GroupNorm's eps against the 2^-20 variance of scale_conv_gn at e = -10 changes the function, for both oracles alike."""
    f32, l32 = sc.oracle_randla(sc.enc_dict(kind, e), which, torch.float32)
    f64, l64 = sc.ref_randla(kind, e, which)
    s = 2.0 ** e if kind == "head" else 1.0
    ltol = sc.FEAT_TOL if which == "feat_extractor" else sc.INLIER_TOL
    _headroom(f32, f64, sc.FEAT_TOL, f"{which} {kind} 2^{e} features")
    _headroom(l32, l64, (ltol[0], ltol[1] * s), f"{which} {kind} 2^{e} logits")


# ------------------------------------------------------------------ the rescalings preserve the function
@pytest.mark.parametrize("i", [1, 2, 3])
@pytest.mark.parametrize("e", [-6, -10, -14, 20])
def test_mlp1d_pair_leaves_the_fp64_descriptors_unchanged(i, e):
    inputs = sc.agg_inputs(257)
    ref = sc.oracle_aggregate(sc.base_sd(), inputs)
    got = sc.oracle_aggregate(sc.scale_mlp1d_pair(sc.base_sd(), "mlp_att", i, e), inputs)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("e", [-6, -10, -14])
def test_scaled_mlp_proj_leaves_the_fp64_descriptors_unchanged(e):
    inputs = sc.agg_inputs(257)
    ref = sc.oracle_aggregate(sc.base_sd(), inputs)
    got = sc.oracle_aggregate(sc.scale_last(sc.base_sd(), "mlp_proj", e), inputs)
    d = float(np.abs(got - ref).max())
    print(f"[mlp_proj x 2^{e}] max |d desc| {d:.2e}")
    assert d <= 1e-12


def test_rescalings_touch_what_they_say():
    sd = sc.base_sd()
    gn = sc.scale_conv_gn(sd, sc.is_encoder_conv, -6)
    changed = {k for k in sd if not np.array_equal(gn[k], sd[k])}
    assert len(changed) == 2 * 2 * 4 * 7                                   # weight + bias, two networks, four levels, seven mlp2d layers
    assert all(".dilated_res_blocks." in k and ".conv." in k for k in changed)
    fc = sc.scale_att_fc(sd, 4)
    assert sum(not np.array_equal(fc[k], sd[k]) for k in sd) == 2 * 4 * 2
    hd = sc.scale_last(sd, "fc_label", -10)
    assert {k for k in sd if not np.array_equal(hd[k], sd[k])} == {f"{n}.fc_label.6.{p}" for n in sc.NETS for p in ("weight", "bias")}
    big = sc.scale_mlp1d_pair(sd, "mlp_att", 3, 20)
    s = big["mlp_att.10.weight"].astype(np.float64) / np.sqrt(big["mlp_att.10.running_var"].astype(np.float64) + 1e-5)
    assert float(np.abs(big["mlp_att.9.weight"][:, :, 0].astype(np.float64) * s[:, None]).max()) > 65504
