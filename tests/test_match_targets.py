"""Ground-truth matches and inlier targets of the `align` training step (csrc/match_targets.hip, include/dsir_train.h).

The distance rule is owned by the engine (open3d, whose KD-tree radius search builds the reference's data['matches'], is not
installable: parity unpinned).  ``rule32`` below restates it in float32 numpy, operation by operation:

    c_r = ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3];  d = ref - c;  d2 = (dx dx + dy dy) + dz dz;  match <=> d2 < r r

1. CPU: the rule is geometrically right - against a float64 brute force ``d2_64 < r^2``; pairs with |d2_64 - r^2| <= 1e-3 r^2 may
   go either way and are left out; at most 1 % of the float64 matches may lie in that band (the rounding of the fp32 rule is
   ~1e-6 relative, the band a thousand times wider: what falls inside is a property of the data, 0.07 - 0.16 % on these inputs).
2. GPU: ``Engine.radius_matches`` equals ``rule32`` exactly - counts, columns, ascending order -, twice with the same bytes.
3. GPU: ``inlier_targets_matches`` equals ``train.find_correct_correspondence`` (the host restatement of the reference) exactly.
4. GPU: ``inlier_targets_radius`` equals operator 3 fed with ``radius_matches`` of the same radius, exactly.
6. The C ABI exports the new symbols with the documented argument lists; the new source holds no floating-point atomics.
"""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

# (shape, points, radius, partial overlap) - the four inputs; match counts of seed 11 (computed on the CPU by rule32)
INPUTS = [("3dmatch", 5000, 0.09, True), ("3dmatch", 2048, 0.3, False), ("kitti", 18000, 0.9, True), ("kitti", 18000, 3.0, True)]
SEED11_MATCHES = [5152, 17492, 23056, 466782]


def _pair(shape, n, seed, partial):
    from deepsir_amd.synth import make_pair
    d = make_pair(n, seed, 3, shape, partial)
    return d["points_src"][0], d["points_ref"][0], d["transform_gt"][0]


def rule32(src, ref, T, r, want64=False, chunk=256):
    """The engine's rule in float32 numpy -> (counts [J] i64, cols i64: per row ascending).  want64: also the float64 brute force
    -> (n64, n_band, n_disagree_outside_band, n_disagree_anywhere)."""
    f = np.float32
    s, q, T = src[:, :3].astype(f), ref[:, :3].astype(f), T.astype(f)
    c = np.stack([((T[k, 0] * s[:, 0] + T[k, 1] * s[:, 1]) + T[k, 2] * s[:, 2]) + T[k, 3] for k in range(3)], 1)
    assert c.dtype == f
    r2 = f(r) * f(r)
    counts, cols = np.zeros(len(s), np.int64), []
    stats = np.zeros(4, np.int64)
    if want64:
        T64 = T.astype(np.float64)
        c64 = s.astype(np.float64) @ T64[:, :3].T + T64[:, 3]
        q64, r2_64 = q.astype(np.float64), float(r) * float(r)
    for a in range(0, len(s), chunk):
        b = min(len(s), a + chunk)
        dx = q[None, :, 0] - c[a:b, None, 0]
        dy = q[None, :, 1] - c[a:b, None, 1]
        dz = q[None, :, 2] - c[a:b, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == f
        m = d2 < r2
        counts[a:b] = m.sum(1)
        cols.append(np.nonzero(m)[1])
        if want64:
            e = q64[None, :, :] - c64[a:b, None, :]
            d64 = (e * e).sum(2)
            m64 = d64 < r2_64
            band = np.abs(d64 - r2_64) <= 1e-3 * r2_64
            stats += (m64.sum(), (m64 & band).sum(), ((m != m64) & ~band).sum(), (m != m64).sum())
    cols = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    return (counts, cols, stats) if want64 else (counts, cols)


@pytest.mark.parametrize("case", range(4))
def test_rule_is_geometrically_right(case):
    shape, n, r, partial = INPUTS[case]
    src, ref, T = _pair(shape, n, 11, partial)
    counts, cols, (n64, n_band, bad_outside, bad_any) = rule32(src, ref, T, r, want64=True)
    print(f"{shape} n={n} r={r}: fp32 matches {counts.sum()}, fp64 {n64}, in band {n_band} ({100.0 * n_band / n64:.2f} %), "
          f"disagree outside band {bad_outside}, anywhere {bad_any}")
    assert counts.sum() == SEED11_MATCHES[case] == len(cols)
    assert n_band <= 0.01 * n64
    assert bad_outside == 0


def test_cabi_exports_the_match_operators_with_documented_arguments():
    import ctypes as C
    from deepsir_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "dsir_train.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    ctype = {"void*": C.c_void_p, "const void*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p, "const int32_t*": C.c_void_p,
             "int32_t*": C.c_void_p, "const int64_t*": C.c_void_p, "int64_t*": C.c_void_p, "int": C.c_int, "float": C.c_float,
             "int64_t": C.c_int64}
    names = ["dsir_t_radius_matches_scratch", "dsir_t_radius_matches_count", "dsir_t_radius_matches_fill", "dsir_t_inlier_targets_radius",
             "dsir_t_match_keys_scratch", "dsir_t_match_keys", "dsir_t_inlier_targets_matches"]
    for name in names:
        m = re.search(r"(size_t|int)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/dsir_train.h"
        assert hasattr(lib, name), f"{name} is not exported"
        args = [ctype[re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*")] for a in m.group(2).split(",")]
        res, bound = _lib.SYMBOLS[name]
        assert res is (C.c_size_t if m.group(1) == "size_t" else C.c_int), name
        assert bound == args, f"{name}: ctypes binding {bound} != header {args}"
    # host-only entry points: shapes that would overflow the int32 offsets get no scratch (the launchers then refuse them)
    assert lib.dsir_t_radius_matches_scratch(4, 18000, 18000) > 0
    assert lib.dsir_t_radius_matches_scratch(8, 18000, 18000) == 0
    assert lib.dsir_t_match_keys_scratch(0, 1) == 0 and lib.dsir_t_match_keys_scratch(1000, 3) > 0


def test_match_source_has_no_float_atomics():
    src = open(os.path.join(ROOT, "deepsir_amd", "csrc", "match_targets.hip")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    assert "tomicAdd" not in src and "atomic" not in src.lower()


def test_as_reference_matches_layout():
    import torch
    from deepsir_amd.train import as_reference_matches
    off = torch.tensor([0, 2, 2, 3, 3, 5, 6], dtype=torch.int32)          # P = 2, J = 3
    cols = torch.tensor([4, 7, 1, 0, 2, 9], dtype=torch.int32)
    m = as_reference_matches(off, cols, 2, 3)
    assert [x.tolist() for x in m] == [[[0, 4], [0, 7], [2, 1]], [[1, 0], [1, 2], [2, 9]]]
    assert all(x.dtype == np.int64 and x.shape[1] == 2 for x in m)
    e = as_reference_matches(torch.zeros(4, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), 1, 3)
    assert e[0].shape == (0, 2)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _dev():
    import torch
    return torch.device("cuda", 0)


_ENG = {}


def _engine(n, pairs=2):
    """One engine per size with plain generated weights (for real ``register`` correspondences)."""
    from deepsir_amd.arch import NetConfig
    from deepsir_amd.engine import Engine
    from deepsir_amd.weights import generate_state_dict
    if (n, pairs) not in _ENG:
        cfg = NetConfig(feat_len=3)
        eng = Engine(cfg, 0, max_points=n, max_pairs=pairs)
        eng.load_state_dict(generate_state_dict(cfg, 3, "plain"))
        _ENG[(n, pairs)] = eng
    return _ENG[(n, pairs)]


def _batch(case, seeds):
    import torch
    shape, n, r, partial = INPUTS[case]
    raws = [_pair(shape, n, s, partial) for s in seeds]
    t = lambda i: torch.from_numpy(np.stack([x[i] for x in raws])).to(_dev())
    return raws, t(0), t(1), t(2), r


def _check_csr(raws, off, cols, r, J):
    off, cols = off.cpu().numpy().astype(np.int64), cols.cpu().numpy().astype(np.int64)
    assert off[0] == 0 and off[-1] == len(cols)
    for p, (s, q, T) in enumerate(raws):
        counts, want = rule32(s, q, T, r)
        o = off[p * J:(p + 1) * J + 1]
        assert (np.diff(o) == counts).all(), f"pair {p}: row counts differ"
        assert (cols[o[0]:o[-1]] == want).all(), f"pair {p}: columns differ"
    return int(off[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(4))
def test_radius_matches_equals_the_float32_restatement(case):
    import torch
    raws, src, ref, gt, r = _batch(case, (11, 12))
    J = src.shape[1]
    eng = _engine(1024, 1)
    off, cols = eng.radius_matches(src, ref, gt, r)
    total = _check_csr(raws, off, cols, r, J)
    print(f"{INPUTS[case]}: {total} matches in 2 pairs")
    assert int(off[J]) == SEED11_MATCHES[case]
    off2, cols2 = eng.radius_matches(src, ref, gt, r)
    assert torch.equal(off, off2) and torch.equal(cols, cols2)


@pytest.mark.gpu
def test_radius_matches_ragged_strided_empty_and_full():
    import torch
    from deepsir_amd.synth import make_pair
    from deepsir_amd.train import as_reference_matches
    eng = _engine(1024, 1)
    dev = _dev()
    # J != K, stride 4 (a feature channel rides along)
    raws = []
    for s in (21, 22, 23):
        d = make_pair(3000, s, 4, "3dmatch", True)
        raws.append((d["points_src"][0][:2777], d["points_ref"][0], d["transform_gt"][0]))
    t = lambda i: torch.from_numpy(np.stack([x[i] for x in raws])).to(dev)
    off, cols = eng.radius_matches(t(0), t(1), t(2), 0.12)
    assert t(0).shape == (3, 2777, 4) and t(1).shape == (3, 3000, 4)
    assert _check_csr(raws, off, cols, 0.12, 2777) > 1000
    m = as_reference_matches(off, cols, 3, 2777)
    assert sum(len(x) for x in m) == len(cols) and all((x[:, 0] < 2777).all() and (x[:, 1] < 3000).all() for x in m)
    # nothing matches
    off, cols = eng.radius_matches(t(0), t(1), t(2), 1e-6)
    assert cols.numel() == 0 and int(off.abs().max()) == 0
    # everything matches: identity transform, ref = src, a cloud smaller than the radius
    rng = np.random.Generator(np.random.Philox(key=5))
    pts = torch.from_numpy(rng.uniform(0, 0.1, (2, 1024, 3)).astype(np.float32)).to(dev)
    eye = torch.eye(4, device=dev)[:3].repeat(2, 1, 1).contiguous()
    off, cols = eng.radius_matches(pts, pts, eye, 1.0)
    assert cols.numel() == 2 * 1024 * 1024
    assert torch.equal(off, (torch.arange(2 * 1024 + 1, device=dev) * 1024).int())
    assert torch.equal(cols.view(2 * 1024, 1024), torch.arange(1024, device=dev).int().expand(2 * 1024, 1024))


@pytest.mark.gpu
def test_inlier_targets_matches_equals_the_host_function():
    import torch
    from deepsir_amd.train import as_reference_matches, find_correct_correspondence
    raws, src, ref, gt, r = _batch(1, (11, 12, 13))                       # 3 pairs of 2048 points, r 0.3
    P, J = 3, src.shape[1]
    eng = _engine(2048, 3)
    idx = eng.register(src, ref, 5)["idx"]
    assert tuple(idx.shape) == (5, P, J)
    lists = as_reference_matches(*eng.radius_matches(src, ref, gt, r), P, J)
    rng = np.random.Generator(np.random.Philox(key=77))
    m0 = lists[0][rng.permutation(len(lists[0]))]                         # random order
    m0 = np.concatenate([m0, m0[:500], m0[100:300]])                      # duplicated entries
    m1 = np.zeros((0, 2), np.int64)                                       # an empty list
    hit = idx[0, 2].cpu().numpy().astype(np.int64)
    alias = np.stack([J + np.arange(40), hit[:40] - 1], 1)                # src >= J: key (J + a) + (b - 1) J aliases the pair (a, b)
    alias = alias[alias[:, 1] >= 0]
    m2 = np.concatenate([lists[2][rng.permutation(len(lists[2]))], alias])
    matches = [m0, m1, m2]
    rand_idx = torch.from_numpy(rng.integers(0, J, (5, P, J)).astype(np.int32)).to(_dev())
    for name, ix in (("register", idx), ("register, 1 iteration", idx[:1].contiguous()), ("random", rand_idx), ("random, 1 iteration", rand_idx[2:3].contiguous())):
        keys = eng.match_keys(matches, J)
        got = eng.inlier_targets_matches(keys, ix).cpu().numpy()
        want = find_correct_correspondence(matches, ix, J)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert (got == want).all(), f"{name}: {int((got != want).sum())} targets differ"
        print(f"{name}: {int(want.sum())} of {want.size} targets are 1")
        assert want[:, 1].sum() == 0
    want = find_correct_correspondence(matches, idx, J)
    assert want[0, 2, alias[:, 0] - J].all() and 0 < want.sum() < want.size    # the aliased entries hit, as on the host
    # torch tensors (host or device) are taken like arrays
    keys_t = eng.match_keys([torch.from_numpy(m).to(_dev()) for m in matches], J)
    assert torch.equal(keys_t.keys, eng.match_keys(matches, J).keys)


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(4))
def test_inlier_targets_radius_equals_targets_from_radius_matches(case):
    import torch
    raws, src, ref, gt, r = _batch(case, (11, 12))
    P, J = 2, src.shape[1]
    eng = _engine(18000, 2)
    idx = eng.register(src, ref, 5)["idx"]
    off, cols = eng.radius_matches(src, ref, gt, r)
    # a second set of correspondences that certainly holds matches: every row's first match where it has one, else its register index
    o = off.long()
    first = cols[o[:-1].clamp(max=max(cols.numel() - 1, 0))].view(P, J)
    has = (o[1:] > o[:-1]).view(P, J)
    mixed = torch.where(has, first, idx[0]).unsqueeze(0).contiguous()
    from deepsir_amd.train import MatchKeys, as_reference_matches
    keys = eng.match_keys(as_reference_matches(off, cols, P, J), J)
    assert isinstance(keys, MatchKeys)
    for name, ix in (("register", idx), ("first match", mixed)):
        a = eng.inlier_targets_radius(src, ref, ix, gt, r)
        b = eng.inlier_targets_matches(keys, ix)
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} targets differ"
        print(f"{INPUTS[case]} {name}: {int(a.sum())} of {a.numel()} targets are 1")
    assert torch.equal(a[0].bool(), has)
