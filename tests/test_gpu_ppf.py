"""use_ppf on the device, through the C ABI (include/dsir.h: dsir_create_ex + DSIR_FLAG_PPF, dsir_ppf_pre, dsir_estimate_normals,
dsir_forward_pair, dsir_register): the point-pair-feature input layer against vectors from the imported reference
(tools/gen_golden_ppf.py) and against its host restatement (deepsir_amd/ppf.py); the normals against the fp64 host rule.
Every test here fails on an engine that refuses ``use_ppf``."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_ppf_host import line_angle, normal_filters

pytestmark = pytest.mark.gpu

_ENGINES = {}


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ppf_cfg(pipeline="align", num_sub=-1):
    from deepsir_amd.arch import NetConfig
    return NetConfig(feat_len=6, use_ppf=True, pipeline=pipeline, num_sub=num_sub)


def engine_for(tag, cfg, wseed, variant="plain", max_points=1100, max_pairs=2):
    from deepsir_amd.engine import Engine
    from deepsir_amd.weights import generate_state_dict
    if tag not in _ENGINES:
        sd = generate_state_dict(cfg, wseed, variant)
        eng = Engine(cfg, max_points=max_points, max_pairs=max_pairs)
        eng.load_state_dict(sd)
        assert len(eng.expected_keys()) == len(sd)
        _ENGINES[tag] = (eng, sd)
    return _ENGINES[tag]


def restated(sd, rows, nb, which="feat_extractor"):
    from deepsir_amd import ppf
    p = which + ".mlp_pre."
    return ppf.ppf_pre(rows, nb, sd[p + "conv.weight"], sd[p + "conv.bias"], sd[p + "norm.weight"], sd[p + "norm.bias"])


# --------------------------------------------------------------------------- front end
def test_front_end_matches_reference_and_restatement():
    g, m = load_golden("ppf_front_n1024")
    eng, sd = engine_for("front", ppf_cfg(), m["wseed"])
    rows, nb = g["rows"], g["neigh_idx"].astype(np.int32)
    out = eng.ppf_pre("feat_extractor", cu(rows), cu(nb)).cpu().numpy()
    want = np.transpose(g["front"], (0, 2, 1))
    host = restated(sd, rows, nb.astype(np.int64))
    print("front end: max |hip - reference| =", np.abs(out - want).max(), " max |hip - restatement| =", np.abs(out - host).max())
    np.testing.assert_allclose(out, want, rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(out, host, rtol=1e-3, atol=1e-4)
    # the inlier model's own mlp_pre through the same entry point
    out_i = eng.ppf_pre("inlier_model", cu(rows), cu(nb)).cpu().numpy()
    np.testing.assert_allclose(out_i, restated(sd, rows, nb.astype(np.int64), "inlier_model"), rtol=1e-3, atol=1e-4)
    assert np.abs(out_i - out).max() > 1e-2


def test_front_end_ragged_multi_cloud_independent_and_repeatable():
    """N = 1100 (no multiple of the 64 points of a workgroup, of a wave's 4 or of anything else), 3 clouds per call, rows of 7
    columns (the last one ignored): against the restatement; per-cloud statistics do not mix - cloud 0 is the same bytes alone
    and inside the batch; two runs write the same bytes."""
    eng, sd = engine_for("front", ppf_cfg(), 7)
    rng = np.random.Generator(np.random.Philox(key=41))
    n = 1100
    xyz = rng.uniform(-2.0, 2.0, (3, n, 3)) * np.array([1.0, 3.0, 0.5])[None, None] + np.arange(3)[:, None, None]
    nrm = rng.standard_normal((3, n, 3))
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    rows = np.concatenate([xyz, nrm, rng.uniform(0, 1, (3, n, 1))], 2).astype(np.float32)
    rows_d = cu(rows)
    _, neigh, _, _ = eng.knn_pyramid(rows_d)
    out = eng.ppf_pre("feat_extractor", rows_d, neigh)
    host = restated(sd, rows, neigh[:, :n].cpu().numpy().astype(np.int64))
    print("ragged: max |hip - restatement| =", np.abs(out.cpu().numpy() - host).max())
    np.testing.assert_allclose(out.cpu().numpy(), host, rtol=1e-3, atol=1e-4)
    again = eng.ppf_pre("feat_extractor", rows_d, neigh)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    alone = eng.ppf_pre("feat_extractor", rows_d[:1].contiguous(), neigh[:1].contiguous())
    assert torch.equal(out[:1].view(torch.int32), alone.view(torch.int32))
    assert (out[0] - out[1]).abs().max() > 1e-2


# --------------------------------------------------------------------------- feat / label pipelines
def _check_selection(pt, score, g_pt, g_score, tag, num_sub):
    """tests/test_pipelines.py: torch.topk leaves the order of equal scores open - scores at 1e-5 / 1e-7, the selection as a set
    through them, identical points wherever a score is not tied with a neighbour."""
    np.testing.assert_allclose(score, g_score, rtol=1e-5, atol=1e-7, err_msg=tag)
    s = g_score[0]
    strict = np.ones(len(s), bool)
    strict[1:] &= s[1:] < s[:-1] * (1 - 1e-5)
    strict[:-1] &= s[:-1] * (1 - 1e-5) > s[1:]
    assert strict.mean() > 0.5, "fixture is degenerate"
    np.testing.assert_array_equal(pt[0][:, strict], g_pt[0][:, strict], err_msg=tag)


@pytest.mark.parametrize("name", ["ppf_label_n1024", "ppf_feat_n1100_sub256"])
def test_pipelines_match_reference(name):
    g, m = load_golden(name)
    eng, _ = engine_for(name, ppf_cfg(m["pipeline"], m["num_sub"]), m["wseed"], max_points=m["n"], max_pairs=1)
    out = eng.forward_pair(cu(g["points_src"]), cu(g["points_ref"]), m["num_sub"])          # pyramids built on device
    for s in ("src", "ref"):
        o = out[s]
        logits = o["logits"].permute(0, 2, 1).cpu().numpy()
        print(name, s, "max |logits - reference| =", np.abs(logits - g[f"logits_{s}"]).max())
        np.testing.assert_allclose(logits, g[f"logits_{s}"], rtol=1e-3, atol=2e-4)
        pt = o["xyz"].permute(0, 2, 1).cpu().numpy()
        feat = o["feat"].permute(0, 2, 1).cpu().numpy()
        if m["pipeline"] == "feat":
            _check_selection(pt, o["score"].cpu().numpy(), g[f"pt_{s}"], g[f"score_{s}"], name + s, m["num_sub"])
            idx = o["index"].cpu().numpy().astype(np.int64)
            assert len(np.unique(idx[0])) == m["num_sub"]
            np.testing.assert_array_equal(pt[0].T, g[f"points_{s}"][0][idx[0], :3])
        same = np.all(pt == g[f"pt_{s}"], axis=1)[0]
        assert same.mean() > 0.9
        np.testing.assert_allclose(feat[0][:, same], g[f"feat_{s}"][0][:, same], rtol=1e-3, atol=1e-4)
        np.testing.assert_allclose(np.linalg.norm(feat[0], axis=0), 1.0, atol=1e-5)


# --------------------------------------------------------------------------- align
def _rot_angle(Ra, Rb):
    """The rotation distance of tests/test_gpu_parity.py (rad): atan2(|vee(skew(Ra^T Rb))|, (tr - 1) / 2) in fp64.  arccos of the
    trace alone cannot serve: two fp32 matrices that differ in their last bit leave the trace 1e-7 short of 3, which arccos
    turns into 3e-4 rad."""
    D = Ra.T @ Rb
    v = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(np.linalg.norm(v), 0.5 * (np.trace(D) - 1.0)))


def _pose_close(T, G, rot_tol, t_tol, tag):
    T, G = np.asarray(T, np.float64).reshape(-1, 3, 4), np.asarray(G, np.float64).reshape(-1, 3, 4)
    worst_a = worst_d = 0.0
    for a, b in zip(T, G):
        ang, d = _rot_angle(a[:, :3], b[:, :3]), float(np.linalg.norm(a[:, 3] - b[:, 3]))
        worst_a, worst_d = max(worst_a, ang), max(worst_d, d)
        assert ang < rot_tol and d < t_tol, (tag, ang, d)
    print(f"[pose] {tag}: worst rot diff {worst_a:.2e} rad, worst trans diff {worst_d:.2e} (tol {rot_tol:g} / {t_tol:g})")


def test_register_teacher_forced_matches_reference():
    """forward_align_4 under use_ppf with the reference's own correspondences forced (the rule of
    tests/test_gpu_parity.py::test_register_teacher_forced_matches_reference): the inlier model's front end is fed [moved src ;
    matched ref] anew every iteration; (R, t) per iteration within 1e-4, logits at 2e-3."""
    g, m = load_golden("ppf_e2e_n1024")
    eng, _ = engine_for("e2e", ppf_cfg(), m["wseed"], m["variant"], max_points=1024, max_pairs=2)
    forced = cu(np.transpose(g["idx"].astype(np.int32), (1, 0, 2)))           # [n_iter, P, J]
    out = eng.register(cu(g["points_src"]), cu(g["points_ref"]), m["n_iter"], forced_idx=forced)
    lg = np.transpose(out["logits"].cpu().numpy(), (1, 0, 2))
    print("teacher-forced: max |logits - reference| =", np.abs(lg - g["logits"]).max())
    _pose_close(out["transforms"].cpu().numpy(), g["transforms"], 1e-4, 1e-4, "ppf_e2e")
    np.testing.assert_allclose(lg, g["logits"], rtol=2e-3, atol=2e-3)
    assert not out["invalid"].cpu().numpy().any() and not bool(g["invalid"])
    np.testing.assert_allclose(out["pt_ref_new"].cpu().numpy(), g["pt_ref_new"], rtol=0, atol=0)


def test_register_free_running_batch_equals_each_pair_alone():
    """No teacher forcing, pyramids on the device, under the rules of tests/test_gpu_parity.py: iteration 0
    agrees with the reference's arg-min on more than 99 % of the rows; poses are asserted (1e-4) only through the iterations in
    which EVERY arg-min agrees; at the first iteration that disagrees, every disagreeing row is a near-tie by the reference's own
    recorded fp64 top-2 gap: the engine's pick is at least that gap above the minimum, and a correct arg-min on descriptors within
    eps of the reference's cannot be more than 2 eta + e32 above it, eta = 2 (eps_src + eps_ref) + e32, with that file's e32 = 2e-6
    and its ceiling eps = 2e-4 per side, relative to 1 + |d_min| as there.  Both pairs in one call equal each pair alone, bit
    for bit (transforms, arg-mins, logits)."""
    g, m = load_golden("ppf_e2e_n1024")
    eng, _ = engine_for("e2e", ppf_cfg(), m["wseed"], m["variant"], max_points=1024, max_pairs=2)
    src, ref = cu(g["points_src"]), cu(g["points_ref"])
    both = eng.register(src, ref, m["n_iter"])
    both = {k: both[k].clone() for k in ("transforms", "idx", "logits")}
    idx = np.transpose(both["idx"].cpu().numpy(), (1, 0, 2))                  # [P, n_iter, J]
    T = both["transforms"].cpu().numpy()
    e32, eps = 2e-6, 2e-4
    tau = 2.0 * (2.0 * (eps + eps) + e32) + e32
    for p in range(2):
        agree = [(idx[p, i] == g["idx"][p, i]).mean() for i in range(m["n_iter"])]
        print(f"pair {p}: arg-min agreement per iteration {['%.4f' % a for a in agree]}")
        assert agree[0] > 0.99
        for i in range(m["n_iter"]):
            if all(a == 1.0 for a in agree[: i + 1]):
                _pose_close(T[p, i], g["transforms"][p, i], 1e-4, 1e-4, f"pair {p} iter {i}")
        first = next((i for i, a in enumerate(agree) if a < 1.0), None)
        if first is not None:
            bad = idx[p, first] != g["idx"][p, first]
            gap, dmin = g["top2_gap"][p, first][bad], g["top2_min"][p, first][bad]
            print(f"pair {p} iteration {first}: {int(bad.sum())} rows differ, largest recorded top-2 gap among them {gap.max():.3e} "
                  f"(admissible {tau:.2e} (1 + |d|); median gap of all rows {np.median(g['top2_gap'][p, first]):.3e})")
            assert np.all(gap <= tau * (1.0 + np.abs(dmin))), "a disagreeing row is not a near-tie"
        R = T[p, -1][:, :3].astype(np.float64)
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-5)
    for p in range(2):
        one = eng.register(src[p:p + 1].contiguous(), ref[p:p + 1].contiguous(), m["n_iter"])
        assert torch.equal(one["transforms"][0].view(torch.int32), both["transforms"][p].view(torch.int32)), p
        assert torch.equal(one["idx"][:, 0], both["idx"][:, p]), p
        assert torch.equal(one["logits"][:, 0].view(torch.int32), both["logits"][:, p].view(torch.int32)), p


# --------------------------------------------------------------------------- normals
@pytest.mark.parametrize("n,seed", [(1024, 21), (2048, 22)])
def test_normals_match_the_host_rule(n, seed):
    """Angle <= 1e-5 rad with equal sign on every point with a separated smallest eigenvalue ((l1 - l0) / l2 >= 0.05) and a decided
    orientation (|cos(n, v - p)| >= 1e-2); the filters leave out at most 1 % (asserted); flags equal everywhere.  The bound: an
    fp32-covariance variant of the rule sits 1.5e-7 rad from the fp64 one on these clouds, the device rule is fp64, two orders of
    magnitude are left for the Jacobi solver, a wrong eigenvector is pi / 2 away."""
    from deepsir_amd import ppf
    eng, _ = engine_for("normals", ppf_cfg("label"), 1, max_points=2048, max_pairs=1)
    pts = ppf.analytic_normals_cloud(n, seed)
    d = cu(pts[None])
    _, neigh, _, _ = eng.knn_pyramid(d)
    got, flags = eng.estimate_normals(d, neigh)
    nb = neigh[0, :n].cpu().numpy().astype(np.int64)
    want, wflags = ppf.estimate_normals(pts[None], nb[None])
    q = pts.astype(np.float64)[nb]
    e = q - q.mean(1, keepdims=True)
    w = np.linalg.eigvalsh(np.einsum("nka,nkb->nab", e, e))
    keep = normal_filters(pts, want[0].astype(np.float64), w)
    assert 1.0 - keep.mean() <= 0.01, keep.mean()
    np.testing.assert_array_equal(flags.cpu().numpy(), wflags)
    a, b = got[0].cpu().numpy().astype(np.float64), want[0].astype(np.float64)
    ang = line_angle(a, b)
    print(f"normals n={n}: max angle on the kept points = {ang[keep].max():.3e} rad, left out {1 - keep.mean():.4f}")
    assert ang[keep].max() <= 1e-5
    assert np.all((a * b).sum(1)[keep] > 0)


def test_normals_of_coincident_points_are_zero_and_flagged():
    """16 coincident points padded to N with a regular cloud: their normals are exactly 0 and flagged, nothing else is; the front
    end downstream stays finite (angle of a zero vector is 0)."""
    from deepsir_amd import ppf
    eng, sd = engine_for("front", ppf_cfg(), 7)
    pts = ppf.analytic_normals_cloud(1024, 23)
    pts[:16] = np.array([0.25, -1.5, 2.0], np.float32)
    d = cu(pts[None])
    _, neigh, _, _ = eng.knn_pyramid(d)
    nb = neigh[0, :1024].cpu().numpy()
    assert np.all(np.sort(nb[:16], axis=1) == np.arange(16)[None])          # each other's 16 nearest: distance 0
    normals, flags = eng.estimate_normals(d, neigh)
    f = flags[0].cpu().numpy()
    assert f[:16].all() and not f[16:].any()
    assert not normals[0, :16].cpu().numpy().any()
    rows = torch.cat([d, normals], 2).contiguous()
    out = eng.ppf_pre("feat_extractor", rows, neigh)
    assert torch.isfinite(out).all()
    np.testing.assert_allclose(out.cpu().numpy(), restated(sd, rows.cpu().numpy(), nb[None].astype(np.int64)), rtol=1e-3, atol=1e-4)


# --------------------------------------------------------------------------- Python surface
def _args(pipeline, num_sub=-1, **kw):
    return SimpleNamespace(pipeline=pipeline, num_sub=num_sub, feat_len=6, num_knn=16, out_feat_dim=64, d_out=[16, 64, 128, 256],
                           sub_sampling_ratio=[4, 4, 4, 4], clip_weight_thresh=0.0, use_ppf=True, num_reg_iter=3, **kw)


def test_network_loads_ppf_state_dict_and_reproduces_label_golden():
    from deepsir_amd.model import Network
    from deepsir_amd.weights import generate_state_dict, to_torch_state_dict
    g, m = load_golden("ppf_label_n1024")
    net = Network(_args("label"))
    net.load_state_dict(to_torch_state_dict(generate_state_dict(ppf_cfg("label"), m["wseed"])), strict=True)
    net = net.cuda().eval()
    none, ep = net({"points_src": cu(g["points_src"]), "points_ref": cu(g["points_ref"])})
    assert none is None and sorted(ep.keys()) == m["keys"]
    for k in m["keys"]:
        assert tuple(ep[k].shape) == g[k].shape, k
    np.testing.assert_allclose(ep["logits_src"].cpu().numpy(), g["logits_src"], rtol=1e-3, atol=2e-4)
    np.testing.assert_allclose(ep["feat_ref"].cpu().numpy(), g["feat_ref"], rtol=1e-3, atol=1e-4)
    # the reference's assertion for rows without normals
    with pytest.raises(AssertionError, match="feature dimension error"):
        net({"points_src": cu(g["points_src"][:, :, :3]), "points_ref": cu(g["points_ref"][:, :, :3])})
    with pytest.raises(NotImplementedError, match="use_ppf"):
        net.train_step({"points_src": cu(g["points_src"]), "points_ref": cu(g["points_ref"])})


def test_harness_align_with_estimated_normals():
    """3-column clouds + args.ppf_estimate_normals: finite poses, byte for byte those of Engine.estimate_normals followed by
    6-column rows."""
    from deepsir_amd.harness import inference_align
    from deepsir_amd.model import Network
    from deepsir_amd.weights import generate_state_dict, to_torch_state_dict
    g, m = load_golden("ppf_e2e_n1024")
    sd = to_torch_state_dict(generate_state_dict(ppf_cfg(), m["wseed"], m["variant"]))
    eye = np.eye(4, dtype=np.float32)[None, :3]

    def run(pairs, **kw):
        net = Network(_args("align", **kw))
        net.load_state_dict(sd, strict=True)
        return inference_align(pairs, net.cuda().eval(), num_reg_iter=m["n_iter"])[0]

    bare = [{"points_src": g["points_src"][p:p + 1, :, :3], "points_ref": g["points_ref"][p:p + 1, :, :3], "transform_gt": eye} for p in range(2)]
    pred = run(bare, ppf_estimate_normals=True)
    assert pred.shape == (2, m["n_iter"] + 1, 3, 4) and np.isfinite(pred).all()
    eng, _ = engine_for("e2e", ppf_cfg(), m["wseed"], m["variant"], max_points=1024, max_pairs=2)
    full = []
    for pr in bare:
        row = {"transform_gt": eye}
        for s in ("points_src", "points_ref"):
            d = cu(pr[s])
            normals, _ = eng.estimate_normals(d, eng.knn_pyramid(d)[1])
            row[s] = torch.cat([d, normals], 2).cpu().numpy()
        full.append(row)
    assert np.array_equal(pred.view(np.uint32), run(full).view(np.uint32))
    with pytest.raises(AssertionError, match="feature dimension error"):
        run(bare)


# --------------------------------------------------------------------------- limits
def test_create_ex_limits():
    from deepsir_amd import _lib
    lib = _lib.load()
    c = _lib.dsir_cfg()
    c.feat_len, c.num_knn, c.num_layers = 6, 16, 4
    for i, (r, d) in enumerate(zip((4, 4, 4, 4), (16, 64, 128, 256))):
        c.sub_sampling_ratio[i], c.d_out[i] = r, d
    c.out_feat_dim, c.num_classes, c.max_pairs, c.pipeline = 64, 19, 1, 0
    limit = lib.dsir_max_points_limit_ex(C.byref(c), _lib.DSIR_FLAG_PPF)
    assert 1024 <= limit <= 1 << 20
    assert lib.dsir_gn_contributions_ex(C.byref(c), _lib.DSIR_FLAG_PPF, limit) <= lib.dsir_gn_contribution_limit()
    h = C.c_void_p()
    c.max_points = limit + 1
    assert lib.dsir_create_ex(0, C.byref(c), _lib.DSIR_FLAG_PPF, C.byref(h)) != 0
    msg = lib.dsir_last_error(None).decode()
    assert "max_points" in msg, msg
    c.max_points, c.feat_len = 1024, 5
    assert lib.dsir_create_ex(0, C.byref(c), _lib.DSIR_FLAG_PPF, C.byref(h)) != 0
    msg = lib.dsir_last_error(None).decode()
    assert "feature dimension error" in msg and "RandLANet.py:325" in msg, msg
    assert lib.dsir_create_ex(0, C.byref(c), 0, C.byref(h)) == 0          # the same cfg without the flag is an ordinary network
    lib.dsir_destroy(h)
