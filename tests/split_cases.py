"""Shared by tests/test_split_model_host.py (no GPU) and tests/test_gpu_split_magnitudes.py: the cases at which the fp16-split
layers (csrc/split_f16.h) are checked away from the one magnitude band that generate_state_dict draws from.

Three things live here, and no fixtures:
  * rescalings of a generated state dict by exact powers of two (most of them leave the network's function unchanged);
  * the per-output error bound of one split contraction, in float64, from the parts that dsir_split_f16 returns;
  * the seeded input builders, the case tables and the float64 oracle references both test files walk.
"""
from collections import OrderedDict

import numpy as np
import torch

from conftest import build_case

# ------------------------------------------------------------------ tolerances: test_stages_vs_oracle_and_golden's, (rtol, atol)
DESC_TOL = (1e-4, 2e-5)
FEAT_TOL = (2e-4, 2e-4)
INLIER_TOL = (5e-4, 5e-4)

STAGE = "stage_n1024_s1"
ENCODER_LAYERS = (".mlp1.", ".lfa.", ".mlp2.", ".mlp_skip.")


def worst_ratio(got, ref, tol):
    """max |got - ref| / (atol + rtol |ref|): <= 1 is numpy's assert_allclose; non-finite values give inf."""
    rtol, atol = tol
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())


# ------------------------------------------------------------------ rescalings
def _copy(sd):
    return OrderedDict((k, np.array(v)) for k, v in sd.items())


def _mul(a, e):
    return (a * np.float32(2.0) ** np.float32(e)).astype(np.float32)


def scale_conv_gn(sd, prefix_filter, e):
    """conv.weight and conv.bias times 2^e in every mlp2d layer (a conv followed by GroupNorm) whose prefix passes the filter.
    GroupNorm divides the factor out again: the function is unchanged apart from its eps."""
    out = _copy(sd)
    for k in sd:
        if k.endswith(".conv.weight") and k[:-len("conv.weight")] + "norm.weight" in sd and prefix_filter(k[:-len(".conv.weight")]):
            out[k] = _mul(sd[k], e)
            b = k[:-len("weight")] + "bias"
            out[b] = _mul(sd[b], e)
    return out


def scale_att_fc(sd, e):
    """Every att_pooling_*.fc.weight times 2^e: the softmax over the neighbours gets softer or sharper (the function changes)."""
    out = _copy(sd)
    hit = 0
    for k in sd:
        if ".att_pooling_" in k and k.endswith(".fc.weight"):
            out[k] = _mul(sd[k], e)
            hit += 1
    assert hit > 0
    return out


def scale_mlp1d_pair(sd, chain, i, e):
    """Gain and bias of the BatchNorm after layer i of an mlp1d chain times 2^e, layer i + 1's conv weight times 2^-e.
    LeakyReLU is positively homogeneous, so the function is unchanged (in fp32 bit for bit, barring under- and overflow)."""
    out = _copy(sd)
    for k in (f"{chain}.{3 * i + 1}.weight", f"{chain}.{3 * i + 1}.bias"):
        assert sd[k].ndim == 1, k
        out[k] = _mul(sd[k], e)
    k = f"{chain}.{3 * i + 3}.weight"
    assert sd[k].ndim == 3, k
    out[k] = _mul(sd[k], -e)
    return out


def scale_last(sd, key, e):
    """Weight and bias of the bare last layer of every mlp1d chain called `key` (mlp_proj, fc_label) times 2^e: the chain's
    output scales with it; mlp_proj's is normalised afterwards, so the descriptors do not change."""
    out = _copy(sd)
    hit = 0
    for k in sd:
        parts = k.split(".")
        if len(parts) >= 3 and parts[-3] == key and parts[-1] == "weight" and sd[k].ndim == 3:
            if f"{'.'.join(parts[:-2])}.{int(parts[-2]) + 1}.running_var" in sd:
                continue                                 # followed by a BatchNorm: not the last layer
            out[k] = _mul(sd[k], e)
            b = k[:-len("weight")] + "bias"
            out[b] = _mul(sd[b], e)
            hit += 1
    assert hit > 0, key
    return out


def is_encoder_conv(prefix):
    return ".dilated_res_blocks." in prefix and any(s in prefix + "." for s in ENCODER_LAYERS)


# ------------------------------------------------------------------ the split contraction and its bound
def split_parts(x):
    """x (float32) -> (hi, lo, r) in float64: the two fp16 parts dsir_split_f16 makes of it and r = |x - hi - lo|."""
    from deepsir_amd import _lib
    lib = _lib.load()
    x = np.ascontiguousarray(x, np.float32)
    hi = np.zeros(x.shape, np.uint16)
    lo = np.zeros(x.shape, np.uint16)
    lib.dsir_split_f16(x.ctypes.data, x.size, hi.ctypes.data, lo.ctypes.data)
    h, l = hi.view(np.float16).astype(np.float64), lo.view(np.float16).astype(np.float64)
    return h, l, np.abs(x.astype(np.float64) - h - l)


def split_dot(a, b):
    """The split contraction over the last axis, al.bh + ah.bl + ah.bh, with the three sums in float64: the operand error
    alone, none from accumulation."""
    ah, al, _ = split_parts(a)
    bh, bl, _ = split_parts(b)
    return (al * bh).sum(-1) + (ah * bl).sum(-1) + (ah * bh).sum(-1)


def split_bound(a, b):
    """B(a, b) of csrc/split_f16.h per output: sum_k (ra_k |b_k| + |a_k| rb_k + |al_k| |bl_k|) for the dropped terms plus
    (K / 16 + 1) 2^-24 sum_k |a_k b_k| for the matrix core's fp32 accumulation (<= 12 roundings per 192 products,
    tests/test_gpu_screen_bound.py)."""
    _, al, ra = split_parts(a)
    _, bl, rb = split_parts(b)
    a64, b64 = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(b, np.float64))
    K = a64.shape[-1]
    return (ra * b64 + a64 * rb + np.abs(al) * np.abs(bl)).sum(-1) + (K / 16.0 + 1.0) * 2.0 ** -24 * (a64 * b64).sum(-1)


def fp32_dot(a, b):
    """A plain fp32 dot product over the last axis: one fp32 multiply and one fp32 add per term, in order."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros(np.broadcast_shapes(a.shape, b.shape)[:-1], np.float32)
    for k in range(a.shape[-1]):
        acc = (acc + a[..., k] * b[..., k]).astype(np.float32)
    return acc


def dot_operands(K, rows, seed):
    """Activations ~ N(0, 1) [rows, K] against one He-normal weight row [K]."""
    rng = np.random.Generator(np.random.Philox(key=1000 * K + seed))
    return rng.standard_normal((rows, K)).astype(np.float32), (rng.standard_normal(K) * np.sqrt(2.0 / K)).astype(np.float32)


# ------------------------------------------------------------------ state dicts and inputs
def base_sd():
    return stage_case()[3]


def stage_case():
    return build_case(STAGE)


def agg_inputs(n, clouds=2, feat_e=0, score_hi=1.0, extent=3.0):
    """xyz [c, n, 3], feat0 [c, n, 64], score [c, n] as dsir_aggregate takes them."""
    rng = np.random.Generator(np.random.Philox(key=7919 * n + clouds))
    xyz = rng.uniform(-extent if extent > 3 else 0.0, extent, (clouds, n, 3)).astype(np.float32)
    feat = _mul(rng.standard_normal((clouds, n, 64)).astype(np.float32), feat_e)
    score = rng.uniform(0, score_hi, (clouds, n)).astype(np.float32)
    return xyz, feat, score


def oracle_aggregate(sd, inputs, dtype=torch.float64):
    from oracle.network import OracleNet
    xyz, feat, score = (torch.from_numpy(a).to(dtype) for a in inputs)
    with torch.no_grad():
        d = OracleNet(stage_case()[2], sd, dtype).aggregate(xyz.permute(0, 2, 1), feat.permute(0, 2, 1), score)
    return d.permute(0, 2, 1).contiguous().numpy()


def encoder_inputs(which):
    """The golden stage pyramid: feat_extractor on both clouds, inlier_model on the source cloud with the golden
    iteration-0 correspondences (as test_stages_vs_oracle_and_golden feeds them).  numpy: feats, xyz, neigh, sub, interp."""
    g, m, cfg, _, data = stage_case()
    cat = lambda k: np.concatenate([data["points_src" + k], data["points_ref" + k]], 0)
    xyz, neigh, sub, interp = cat("_xyz"), cat("_neigh_idx"), cat("_sub_idx"), cat("_interp_idx")
    if which == "feat_extractor":
        return cat(""), xyz, neigh, sub, interp
    N = m["n"]
    i0 = g["idx"][0, 0].astype(np.int64)
    feats = np.concatenate([data["points_src_xyz"][0, :N], data["points_ref_xyz"][0, :N][i0]], 1)[None].astype(np.float32)
    return feats, xyz[:1], neigh[:1], sub[:1], interp[:1]


def oracle_randla(sd, which, dtype=torch.float64):
    """-> feat [c, n, 64], logits [c, n, ncls] (numpy), OracleNet in `dtype` on encoder_inputs(which)."""
    from oracle.network import OracleNet
    feats, xyz, neigh, sub, interp = encoder_inputs(which)
    f = lambda a: torch.from_numpy(a).to(dtype)
    i = lambda a: torch.from_numpy(a).long()
    with torch.no_grad():
        feat, _, logits = OracleNet(stage_case()[2], sd, dtype).randla(which, f(feats), f(xyz), i(neigh), i(sub), i(interp))
    return feat.permute(0, 2, 1).contiguous().numpy(), logits.permute(0, 2, 1).contiguous().numpy()


# ------------------------------------------------------------------ the case tables of tests/test_gpu_split_magnitudes.py
AGG_N = (257, 1357)                 # one 128-point block plus a tail, several blocks; both ragged
AGG_E = (0, -6, -10, -14)
AGG_KINDS = ("pair1", "pair2", "pair3", "proj")
RANGE_END = ("pair3", 20)           # folded mlp_att layer 3 above 65504
ACT_FEAT_E = (-12, 0, 10)
ENC_GN_E = (0, -6, -10)
ENC_FC_E = (-8, 0, 4)
HEAD_E = (-10, 0)
NETS = ("feat_extractor", "inlier_model")


def agg_dict(kind, e):
    sd = base_sd()
    if kind == "proj":
        return scale_last(sd, "mlp_proj", e)
    return scale_mlp1d_pair(sd, "mlp_att", int(kind[-1]), e)


def act_inputs(feat_e):
    return agg_inputs(257, 2, feat_e=feat_e, score_hi=2.0 ** -8, extent=50.0)


def enc_dict(kind, e):
    sd = base_sd()
    if kind == "gn":
        return scale_conv_gn(sd, is_encoder_conv, e)
    if kind == "fc":
        return scale_att_fc(sd, e)
    assert kind == "head"
    return scale_last(sd, "fc_label", e)


_REF = {}


def ref_aggregate(kind, e, n, feat_e=None):
    """float64 oracle descriptors of an aggregation case (computed once)."""
    k = ("agg", kind, e, n, feat_e)
    if k not in _REF:
        sd = base_sd() if kind == "act" else agg_dict(kind, e)
        _REF[k] = oracle_aggregate(sd, act_inputs(feat_e) if kind == "act" else agg_inputs(n))
    return _REF[k]


def ref_randla(kind, e, which):
    k = ("enc", kind, e, which)
    if k not in _REF:
        _REF[k] = oracle_randla(enc_dict(kind, e), which)
    return _REF[k]
