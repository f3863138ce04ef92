"""The host restatement of the spatial-consensus pose rule (deepsir_amd/consensus.py; the device side is csrc/consensus.hip): its
packed-bit form against a plain dense one, the tie rules, the degenerate inputs, and what the stage is for - poses from
correspondence sets that are 90 % and 95 % wrong.  No GPU."""
import numpy as np
import pytest

from deepsir_amd import consensus as Cn
from deepsir_amd import ransac as R

THR = 0.05


def _dense_float64(cs, cq, compat):
    """The rule once more, entry by entry: C and S2 as plain integer loops over float64 lengths."""
    M = cs.shape[0]
    live = ~R.is_parked(cs, cq)
    s, q = cs.astype(np.float64), cq.astype(np.float64)
    C = np.zeros((M, M), np.int64)
    for i in range(M):
        for j in range(M):
            if i != j and live[i] and live[j]:
                a, b = s[i] - s[j], q[i] - q[j]
                ls = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
                lq = np.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])
                C[i, j] = abs(ls - lq) < compat
    S2 = C * (C @ C.T)
    return C.astype(bool), S2


def test_packed_bits_against_the_dense_restatement():
    pr = R.make_problem(130, 0.5, 0.005, 7)
    pr["src"][11] = np.nan                                                          # one parked row
    out = Cn.consensus_pair(pr["src"], pr["ref"], pr["corr"], 125, max_dist=THR)
    C, S2 = _dense_float64(out["cs"], out["cq"], Cn.compat_dist_of(None, THR))
    assert out["bits"].shape == (130, 3) and out["bits"].dtype == np.uint64
    assert np.array_equal(out["C"], C) and np.array_equal(out["C"], out["C"].T) and not out["C"].diagonal().any()
    assert np.array_equal(Cn.unpack_bits(out["bits"], 130), C)
    assert not Cn.unpack_bits(out["bits"], 192)[:, 130:].any()
    assert np.array_equal(out["S2"], S2) and np.array_equal(Cn.second_order_packed(out["bits"]), S2)
    assert np.array_equal(out["score"], S2.sum(1))
    assert not out["C"][11].any() and not out["C"][125:].any() and not out["band"].any()
    for i, j in ((0, 1), (5, 70), (129, 64)):                                       # bit j % 64 of word j // 64 of row i
        assert bool((int(out["bits"][i, j // 64]) >> (j % 64)) & 1) == bool(C[i, j])
    assert Cn.compat_dist_of(0.0, THR) == Cn.compat_dist_of(-1.0, THR) == float(np.float32(THR)) != Cn.compat_dist_of(0.1, THR)


def test_selection_rules():
    assert Cn.select_seeds([5, 9, 9, 0, 5], 3).tolist() == [1, 2, 0]                # score descending, ties to the lower index
    assert Cn.select_seeds([5, 9, 9, 0, 5], 8).tolist() == [1, 2, 0, 4, -1, -1, -1, -1]          # only rows with score > 0
    assert Cn.select_members([0, 4, 7, 4, 4, 0, 9], 0, 4).tolist() == [0, 1, 2, 6]   # the seed, then (S2, lower j): 6, 2, 1
    assert Cn.select_members([0, 4, 7, 4, 4, 0, 9], 5, 8).tolist() == [1, 2, 3, 4, 5, 6, -1, -1]  # S2 > 0 only, ascending
    assert Cn.select_members([0, 0, 3], 0, 3).tolist() == [0, 2, -1]


def test_ties_on_duplicated_rows():
    # two copies of one noise-free structure: row i and row i + 100 have the same score and the same S2 values
    a = R.make_problem(100, 0.3, 0.0, 60)
    src, ref = np.concatenate([a["src"], a["src"]]), np.concatenate([a["ref"], a["ref"]])
    corr = np.stack([np.arange(200), np.arange(200)], 1).astype(np.int32)
    out = Cn.consensus_pair(src, ref, corr, max_dist=THR, seeds=8, members=9)
    sc, seed = out["score"], out["seed"]
    assert np.array_equal(sc[:100], sc[100:])
    assert (np.diff(sc[seed]) <= 0).all() and len(set(sc[seed])) < 8                       # descending, with ties among the 8
    assert all(seed[r] < seed[r + 1] for r in range(7) if sc[seed[r]] == sc[seed[r + 1]])  # seeds: ties to the lower index
    assert seed[0] < 100 and seed[1] == seed[0] + 100                                      # a row comes before its copy
    assert (sc[np.setdiff1d(np.arange(200), seed)] <= sc[seed[-1]]).all()
    for r, i in enumerate(seed):
        row = out["S2"][i]
        mem = out["seed_members"][r]
        mem = mem[mem >= 0]
        assert len(mem) == 9 and i in mem and (np.diff(mem) > 0).all()
        rest = mem[mem != i]
        t = row[rest].min()
        assert (row[np.setdiff1d(np.arange(200), mem)] <= t).all()
        tied = np.nonzero(row == t)[0]
        tied = tied[tied != i]
        taken = np.isin(tied, mem)
        assert len(tied) > taken.sum() > 0 and taken[:taken.sum()].all()                   # members: ties to the lower index
    assert out["seed_valid"].all() and (out["seed_count"] == out["seed_count"][0]).all()
    assert out["h"] == 0 and out["stats"][2] == 0                                          # winner: equal counts, the lower rank
    assert out["stats"][4] == 2 * a["inlier"].sum()


def test_degenerate_inputs_return_t_init():
    T_init = np.array([[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3]], np.float32)
    pr = R.make_problem(64, 0.0, 0.0, 3)
    for count in (0, 1, 2):                                                         # fewer than 3 live rows
        out = Cn.consensus_pair(pr["src"], pr["ref"], pr["corr"], count, max_dist=THR, T_init=T_init)
        assert out["h"] == -1 and np.array_equal(out["T"], T_init) and np.array_equal(out["stats"], [0, 0, -1, 0, 0])
        assert not out["seed_valid"].any()
    src = pr["src"].copy()
    src[2] = np.inf                                                                 # 3 rows, one of them parked
    out = Cn.consensus_pair(src, pr["ref"], pr["corr"], 3, max_dist=THR, T_init=T_init)
    assert out["h"] == -1 and np.array_equal(out["T"], T_init) and not out["C"][2].any() and not out["C"][:, 2].any()
    out = Cn.consensus_pair(pr["src"], pr["ref"], pr["corr"], 0, max_dist=THR)
    assert np.array_equal(out["T"], R.IDENTITY)
    out = Cn.consensus_pair(pr["src"], pr["ref"], pr["corr"], 3, max_dist=THR, T_init=T_init)       # three live rows are enough
    assert out["h"] == 0 and out["stats"][4] == 3
    for kw in (dict(seeds=0), dict(seeds=Cn.MAX_SEEDS + 1), dict(members=2), dict(members=Cn.MAX_MEMBERS + 1)):
        with pytest.raises(ValueError):
            Cn.consensus_pair(pr["src"], pr["ref"], pr["corr"], max_dist=THR, **kw)


@pytest.mark.parametrize("frac", [0.9, 0.95])
@pytest.mark.parametrize("seed", [100, 101, 102])
def test_recovery_where_sampling_fails(frac, seed):
    pr = R.make_problem(1000, frac, 0.005, seed)
    out = Cn.consensus_pair(pr["src"], pr["ref"], pr["corr"], max_dist=THR)
    rot, tr = R.pose_error(out["T"], pr["T_gt"])
    print(f"RECOVERY {frac} seed {seed}: inliers {int(out['stats'][4])} of {int(pr['inlier'].sum())} true, {rot:.1e} rad {tr:.1e} m")
    assert rot < 5e-3 and tr < 5e-3
    assert not out["band"].any()


def test_header_binding_and_limits_agree():
    import os
    import re
    from conftest import ROOT
    from deepsir_amd import _lib
    h = open(os.path.join(ROOT, "include", "dsir.h")).read()
    for name, val in (("SEEDS", Cn.MAX_SEEDS), ("MEMBERS", Cn.MAX_MEMBERS), ("M", Cn.MAX_M)):
        assert int(re.search(rf"#define DSIR_CONSENSUS_MAX_{name} (\d+)", h).group(1)) == val
    assert Cn.MAX_M ** 2 < 2 ** 31 and Cn.MAX_M < 2 ** 16                           # int32 scores, uint16 second-order counts
    assert "int dsir_consensus_correspondence(" in h and len(_lib.SYMBOLS["dsir_consensus_correspondence"][1]) == 20
    import ctypes
    assert ctypes.sizeof(_lib.dsir_consensus_diag) == 7 * 8
