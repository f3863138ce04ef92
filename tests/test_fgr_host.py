"""The host restatement of the FGR pose rule (deepsir_amd/fgr.py) on its own: the tuple selection against a plain loop, the key
scheme against ransac.py's, normalise -> un-normalise, recovery on the synthetic problems the rule was probed with, the no-pose cases,
and header / binding / constants.  The recovery bar - 1 degree and max_dist (0.05 m) - is ten times what the probe measured (under
0.1 degree and 6 mm at 5 mm noise, outlier shares 0.5 - 0.8, M = 64 .. 1025)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from deepsir_amd import fgr as F
from deepsir_amd import ransac as R

THR = 0.05


def _f32(x):
    return np.float32(x)


def _plain_tuple_rows(cs, cq, count, seed, p, tuple_scale, max_tuples, max_trials):
    ts2 = _f32(_f32(tuple_scale) * _f32(tuple_scale))
    rows = []
    n = min(100 * count, max_trials)
    for t in range(n):
        r = R.sample_rows(seed, p, [t], 3, count)[0, :3]
        ok = True
        with np.errstate(over="ignore", invalid="ignore"):
            for a, b in ((0, 1), (0, 2), (1, 2)):
                d2 = []
                for pts in (cs, cq):
                    d = [_f32(pts[r[a]][c] - pts[r[b]][c]) for c in range(3)]
                    d2.append(_f32(_f32(_f32(d[0] * d[0]) + _f32(d[1] * d[1])) + _f32(d[2] * d[2])))
                ok = ok and bool(_f32(d2[0] * ts2) < d2[1]) and bool(_f32(d2[1] * ts2) < d2[0])
        if ok:
            rows.extend(int(x) for x in r)
            if len(rows) == 3 * max_tuples:
                break
    return np.array(rows, np.int32), n


@pytest.mark.parametrize("count,max_tuples,max_trials", [(40, 1000, 1 << 20), (40, 7, 1 << 20), (40, 1000, 500), (3, 5, 100), (0, 5, 100)])
def test_tuple_selection_against_a_plain_loop(count, max_tuples, max_trials):
    pr = R.make_problem(40, 0.5, 0.005, 9)
    pr["ref"][4] = np.nan                                                           # a parked row fails by itself
    cs, cq, count, _ = R.gather(pr["src"], pr["ref"], pr["corr"], count)
    got, trials = F.tuple_rows(cs, cq, count, 77, 2, 0.95, max_tuples, max_trials)
    want, n = _plain_tuple_rows(cs, cq, count, 77, 2, 0.95, max_tuples, max_trials)
    assert trials == n == F.trials_of(count, max_trials) and np.array_equal(got, want)
    assert not (got == 4).any() and len(got) <= 3 * max_tuples


def test_key_scheme_is_ransacs():
    for seed, p, count in ((0, 0, 17), (0xDEADBEEF12345678, 3, 5000), (5, 1, 1)):
        t = np.arange(300)
        want = R.sample_rows(seed, p, t, 3, count)[:, :3]
        cs = np.zeros((count, 3), np.float32)
        rows, _ = F.tuple_trials(cs, cs, count, seed, p, 0.95, t)
        assert np.array_equal(rows, want) and rows.max() < count
        # pair p of a call is pair 0 of a call with seed ^ (p << 40)
        assert np.array_equal(R.sample_rows(seed ^ (p << 40), 0, t, 3, count)[:, :3], want)


def test_normalise_unnormalise_is_the_identity_on_a_known_pose():
    pr = R.make_problem(200, 0.0, 0.0, 5)
    s, q = pr["src"].astype(np.float64), pr["ref"].astype(np.float64)
    ms, mq, scale = F.normalise(s, q)
    assert scale == max(np.linalg.norm(s - ms, axis=1).max(), np.linalg.norm(q - mq, axis=1).max())
    Rg, tg = pr["T_gt"][:, :3], pr["T_gt"][:, 3]
    T_norm = np.concatenate([Rg, ((Rg @ ms + tg - mq) / scale)[:, None]], 1)       # the ground truth in the normalised frame
    assert np.abs(F.unnormalise(T_norm, ms, mq, scale) - pr["T_gt"]).max() < 1e-14
    sn, qn = (s - ms) / scale, (q - mq) / scale
    assert np.abs(sn @ Rg.T + T_norm[:, 3] - qn).max() < 1e-6                        # fp32 rounding of ref, in units of scale


@pytest.mark.parametrize("tuple_test", [True, False])
@pytest.mark.parametrize("share", [0.5, 0.8])
@pytest.mark.parametrize("M", [64, 257, 1025])
def test_recovery(M, share, tuple_test):
    pr = R.make_problem(M, share, 0.005, 7 + M)
    out = F.fgr_pair(pr["src"], pr["ref"], pr["corr"], max_dist=THR, tuple_test=tuple_test, seed=3)
    rot, tr = R.pose_error(out["T"], pr["T_gt"])
    print(f"RECOVERY M={M} share {share} tuple_test {tuple_test}: {out['n_rows']} rows, {np.degrees(rot):.3f} deg {tr:.4f} m")
    assert out["iters_run"] == 64 and rot < np.radians(1.0) and tr < THR
    assert out["stats"][2] == 0 and out["stats"][3] == 1 and out["stats"][4] >= 0.9 * pr["inlier"].sum()


def test_no_pose():
    T_init = np.arange(12, dtype=np.float32).reshape(3, 4)
    pr = R.make_problem(64, 0.0, 0.005, 31)
    cases = [dict(count=2), dict(count=2, tuple_test=False)]
    for kw in cases:                                                                # M < 3
        out = F.fgr_pair(pr["src"], pr["ref"], pr["corr"], max_dist=THR, T_init=T_init, **kw)
        assert out["T_candidate"] is None and np.array_equal(out["T"], T_init) and np.array_equal(out["stats"], [0, 0, -1, 0, 0])
    out = F.fgr_pair(pr["src"], (2.0 * pr["ref"]).astype(np.float32), pr["corr"], max_dist=THR)   # every edge twice as long
    assert out["n_rows"] == 0 and out["trials"] == 6400 and out["T_candidate"] is None and np.array_equal(out["T"], R.IDENTITY)
    same = np.full((64, 3), 0.5, np.float32)                                        # all coincident: no tuple, and scale == 0 without the test
    for tt in (True, False):
        out = F.fgr_pair(same, same, pr["corr"], max_dist=THR, tuple_test=tt)
        assert out["T_candidate"] is None and out["n_rows"] == (0 if tt else 64) and np.array_equal(out["stats"], [0, 0, -1, 0, 0])
    for kw in (dict(tuple_scale=0.0), dict(tuple_scale=1.5), dict(max_tuples=0), dict(max_trials=0), dict(iterations=0),
               dict(iterations=F.MAX_ITERS + 1)):
        with pytest.raises(ValueError):
            F.fgr_pair(pr["src"], pr["ref"], pr["corr"], max_dist=THR, **kw)


def test_solve_is_the_headers():
    """fgr.solve against numpy's on a well-conditioned system, and its refusals (fewer than 6 rows, a zero diagonal entry)."""
    rng = np.random.default_rng(0)
    J = rng.normal(size=(50, 6))
    A, b = J.T @ J, rng.normal(size=6)
    x, ok = F.solve(A, b, 50.0)
    assert ok and np.abs(x - np.linalg.solve(A, -b)).max() < 1e-12
    assert not F.solve(A, b, 5.0)[1]
    A[0, :] = 0
    A[:, 0] = 0
    assert not F.solve(A, b, 50.0)[1]


def test_header_binding_and_limits_agree():
    from deepsir_amd import _lib
    from deepsir_amd.engine import Engine
    h = open(os.path.join(ROOT, "include", "dsir.h")).read()
    for name, val, eng in (("TUPLES", F.MAX_TUPLES, Engine.FGR_MAX_TUPLES), ("TRIALS", F.MAX_TRIALS, Engine.FGR_MAX_TRIALS),
                           ("ITERS", F.MAX_ITERS, Engine.FGR_MAX_ITERS)):
        m = re.search(rf"#define DSIR_FGR_MAX_{name} (\(1 << (\d+)\)|\d+)", h)
        assert (1 << int(m.group(2)) if m.group(2) else int(m.group(1))) == val == eng
    fh = open(os.path.join(ROOT, "deepsir_amd", "csrc", "fgr.h")).read()
    assert int(re.search(r"kFgrTrialsPerRow = (\d+)", fh).group(1)) == F.TRIALS_PER_ROW
    assert "int dsir_fgr_correspondence(" in h and len(_lib.SYMBOLS["dsir_fgr_correspondence"][1]) == 24
    assert ctypes.sizeof(_lib.dsir_fgr_diag) == 8 * 8
    lib = _lib.load()
    assert lib.dsir_fgr_correspondence(None, None, None, 1, 1, 1, 3, None, None, 1, ctypes.c_float(0.1), 1, ctypes.c_float(0.95), 1000,
                                       1000, 64, ctypes.c_float(1.4), 2, 0, None, None, None, None, None) != 0


def test_host_only_fgr_check(tmp_path):
    """csrc/fgr.h (the trial key, the trial count, the row-list bounds, the scratch layout) compiles as plain host C++; its stand-alone
    check (tools/fgr_check.cpp; the sanitizer command is in its header) passes."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "fgr_check")
    r = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "deepsir_amd", "csrc"),
                        os.path.join(ROOT, "tools", "fgr_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "fgr: " in r.stdout, r.stdout + r.stderr
    # the draws the header makes are the restatement's
    want = R.sample_rows(12345, 3, [0, 1, 777], 3, 1000)[:, :3].reshape(-1).tolist()
    assert [int(v) for v in re.search(r"rows: ([\d ]+)", r.stdout).group(1).split()] == want
