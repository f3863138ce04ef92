"""interp_idx read off the finished 16-NN lists (csrc/knn.hip, interp_lists_kernel) against the searches it replaces: Engine.knn_pyramid,
all four outputs, bit for bit against (a) a child process with DSIR_NO_INTERP_LISTS set - the switch is read once per process, the
child is a fresh process running tools/interp_lists_dump.py - which runs the parent's launches (the kind-0 jobs, grid_nn1_kernel,
copy_sub_levels_kernel), and (b) oracle.knn.knn_pyramid.  The clouds (tools/interp_lists_dump.py, cases()): 3 x 1027 (levels
1027 / 256 / 64 / 16), 16 x 4224 (the launch size at which the parent walked the grid), 2 x 5000, a cloud sorted along x (most queries
take the cooperative scan), a lattice with every point duplicated (ties at d2 = 0 and at equal positive d2 across every prefix
boundary), and a cloud with non-finite rows (expected: what the searches give).  And one registration with the switch on and off."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import interp_lists_dump as dump  # noqa: E402

pytestmark = pytest.mark.gpu

_RUN = {}


def _both(tmp_path_factory):
    """(this process, the child with the searches): computed once, never changed"""
    if not _RUN:
        d = tmp_path_factory.mktemp("interp")
        mine, theirs = str(d / "lists.npz"), str(d / "search.npz")
        dump.run(mine)
        env = dict(os.environ, DSIR_TUNING="1", DSIR_NO_INTERP_LISTS="1")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "interp_lists_dump.py"), theirs], env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        _RUN["mine"], _RUN["theirs"] = dict(np.load(mine)), dict(np.load(theirs))
    return _RUN["mine"], _RUN["theirs"]


CASES = ["r1027", "r4224", "r5000", "sorted1100", "dups1100", "nonfinite1100"]


def test_cases_are_the_dump_s():
    assert sorted(CASES) == sorted(dump.cases())


@pytest.mark.parametrize("name", CASES)
def test_same_bits_as_the_searches(tmp_path_factory, name):
    mine, theirs = _both(tmp_path_factory)
    for k in ("xyz", "neigh", "sub", "interp"):
        a, b = mine[f"{name}.{k}"], theirs[f"{name}.{k}"]
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, k)


@pytest.mark.parametrize("name", [c for c in CASES if c != "nonfinite1100"])
def test_same_as_oracle(tmp_path_factory, name):
    from oracle.knn import knn_pyramid
    mine, _ = _both(tmp_path_factory)
    pts, with_oracle = dump.cases()[name]
    assert with_oracle
    for c in range(len(pts)):
        want = knn_pyramid(pts[c], 16, (4, 4, 4, 4))
        assert mine[f"{name}.xyz"][c].tobytes() == want["xyz"].tobytes(), (name, c)
        for k, w in (("neigh", "neigh_idx"), ("sub", "sub_idx"), ("interp", "interp_idx")):
            assert np.array_equal(mine[f"{name}.{k}"][c], want[w]), (name, c, k)


def test_registration_same_transforms(tmp_path_factory):
    mine, theirs = _both(tmp_path_factory)
    a, b = torch.from_numpy(mine["transforms"]), torch.from_numpy(theirs["transforms"])
    assert a.shape[0] == 2 and torch.isfinite(a).all()
    assert torch.equal(a, b)
