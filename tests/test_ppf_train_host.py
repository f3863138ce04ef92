"""The host restatement of the use_ppf front end's backward (deepsir_amd/ppf.py::ppf_pre_backward) against the reference's autograd
(tests/golden/ppf_train_front_n1024.npz, tools/gen_golden_ppf_train.py).  No GPU."""
import json
import os

import numpy as np

from deepsir_amd import ppf
from deepsir_amd.arch import NetConfig
from deepsir_amd.weights import generate_state_dict

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("conv.weight", "conv.bias", "norm.weight", "norm.bias")


def front_case():
    """rows, neigh, the four mlp_pre tensors, the upstream gradient and the reference's four gradients of fixture (a)."""
    front = np.load(os.path.join(GOLD, "ppf_front_n1024.npz"))
    tr = np.load(os.path.join(GOLD, "ppf_train_front_n1024.npz"))
    meta = json.loads(str(tr["meta"]))
    sd = generate_state_dict(NetConfig(feat_len=6, use_ppf=True), meta["wseed"])
    w = [np.asarray(sd["feat_extractor.mlp_pre." + k], np.float32) for k in NAMES]
    return front["rows"], front["neigh_idx"].astype(np.int32), w, tr["G"], [tr["g_" + k].astype(np.float64) for k in NAMES]


def relative_distance(got, ref):
    """max |got - ref| over the tensor, in units of the reference tensor's largest magnitude"""
    return float(np.abs(np.asarray(got, np.float64).reshape(-1) - ref.reshape(-1)).max() / np.abs(ref).max())


def test_restated_backward_matches_reference_autograd():
    """The four gradients of the fp64-accumulating restatement vs torch autograd through the reference's feat_grouping + mlp_pre +
    mean (fp32 throughout).  The distance printed here is the yardstick of the device test (tests/test_gpu_ppf_train.py): measured
    4.3e-6 (conv.weight), 4.9e-6 (conv.bias), 1.9e-6 (norm.weight), 2.4e-6 (norm.bias) of each tensor's maximum - far inside the
    project's 2e-3 rule, so the device test keeps that rule."""
    rows, neigh, w, G, ref = front_case()
    dW, db, dgamma, dbeta = ppf.ppf_pre_backward(rows, neigh, *w, G)
    for name, got, want in zip(NAMES, (dW, db, dgamma, dbeta), ref):
        d = relative_distance(got, want)
        print(f"restatement vs reference autograd, mlp_pre.{name}: {d:.3e} of max |g| = {np.abs(want).max():.4f}")
        assert d <= 2e-3 + 1e-6 / np.abs(want).max(), name          # the project's rule for gradient comparisons (tests/test_train.py)
        # the reference sums 32 768 fp32 terms per channel: at most 32 768 x 2^-24 = 2e-3 of the sum of magnitudes, ~ sqrt of that
        # count in practice (1e-5); the restatement's fp64 sums add nothing to it
        assert d <= 1e-4, name


def test_restated_backward_is_per_cloud_and_forward_is_unchanged():
    rows, neigh, w, G, _ = front_case()
    full = ppf.ppf_pre_backward(rows, neigh, *w, G, per_cloud=True)
    one = ppf.ppf_pre_backward(rows[1:], neigh[1:], *w, G[1:], per_cloud=True)
    assert np.array_equal(full[4][1], one[4][0]) and np.array_equal(full[5][1], one[5][0])
    front = np.load(os.path.join(GOLD, "ppf_front_n1024.npz"))
    out = ppf.ppf_pre(rows, neigh, *w).transpose(0, 2, 1)
    assert np.abs(out - front["front"]).max() <= 1e-5 * np.abs(front["front"]).max() + 1e-6
