"""Host restatement of the spatial-consensus pose rule of ``csrc/consensus.hip`` (include/dsir.h, dsir_consensus_correspondence).

Neither the reference nor open3d has this stage (the idea is the second-order spatial compatibility of SC2-PCR), so parity is
unpinned and the engine owns the rule.  This module states it a second time in numpy, the way ``ransac.py`` does for RANSAC: the
tests compare the device against it, the product path never calls it.  There is no seed and no random number.

The rule, per pair (the header of csrc/consensus.hip has the full text):

* gather as RANSAC's (``ransac.gather``): clamp, park non-finite rows and rows beyond ``count``; a parked row is compatible with nothing;
* ``C[i][j] = 1`` iff ``i != j``, neither parked and ``| |s_i - s_j| - |q_i - q_j| | < compat_dist`` in float64 on the fp32
  coordinates, ``|d| = sqrt((dx dx + dy dy) + dz dz)``; packed as ``W = ceil(M / 64)`` words a row, bit ``j % 64`` of word ``j // 64``;
* ``S2[i][j] = C[i][j] * popcount(row_i & row_j)``, ``score[i] = sum_j S2[i][j]``: integers;
* seeds: the ``seeds`` rows of the largest ``(score, lower index)`` with ``score > 0``;
* members of seed ``i``: ``i`` and the ``members - 1`` rows of the largest ``(S2[i][j], lower j)`` with ``S2[i][j] > 0``, in ascending
  index; fewer than 3: invalid;
* fit: ``ransac.kabsch64`` of the members in member order, rounded to fp32 once;
* the seed poses are scored, picked (largest count, ties to the lower seed rank), refitted and finished as RANSAC's hypotheses.

``band`` marks the entries with ``| |ds - dq| - compat_dist | < 1e-12 max(1, compat_dist)``: the only places where a last-bit
difference of the device's float64 ``sqrt`` could move a bit.  ``second_order`` takes ``C @ C`` in float32 BLAS: the counts are
below ``M <= 4096 < 2^24`` and therefore exact; ``second_order_packed`` is the plain popcount form for small problems.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from . import ransac as R

MAX_SEEDS = 256          # DSIR_CONSENSUS_MAX_SEEDS of include/dsir.h
MAX_MEMBERS = 128        # DSIR_CONSENSUS_MAX_MEMBERS
MAX_M = 24576            # DSIR_CONSENSUS_MAX_M
HOST_MAX_M = 4096        # the float32 product below is exact up to here (and far beyond: counts < 2^24)

_POP8 = np.array([bin(v).count("1") for v in range(256)], np.uint8)


def compat_dist_of(compat_dist, max_dist) -> float:
    """The threshold the device compares against: the fp32 argument widened (``<= 0`` / None: ``max_dist``)."""
    cd = max_dist if compat_dist is None or not compat_dist > 0 else compat_dist
    return float(np.float32(cd))


def compat_matrix(cs, cq, compat: float):
    """(C [M, M] bool, band [M, M] bool) of the gathered rows."""
    live = ~R.is_parked(cs, cq)
    s, q = np.asarray(cs, np.float64), np.asarray(cq, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        ds = s[:, None, :] - s[None, :, :]
        ls = np.sqrt((ds[..., 0] * ds[..., 0] + ds[..., 1] * ds[..., 1]) + ds[..., 2] * ds[..., 2])
        del ds
        dq = q[:, None, :] - q[None, :, :]
        lq = np.sqrt((dq[..., 0] * dq[..., 0] + dq[..., 1] * dq[..., 1]) + dq[..., 2] * dq[..., 2])
        del dq
        diff = np.abs(ls - lq)
    ok = live[:, None] & live[None, :]
    np.fill_diagonal(ok, False)
    C = ok & (diff < compat)
    with np.errstate(invalid="ignore"):
        band = ok & (np.abs(diff - compat) < 1e-12 * max(1.0, compat))
    return C, band


def pack_bits(C) -> np.ndarray:
    """[M, M] bool -> [M, W] uint64, bit j % 64 of word j // 64."""
    C = np.asarray(C, bool)
    M = C.shape[0]
    W = (M + 63) // 64
    padded = np.zeros((M, W * 64), np.uint8)
    padded[:, :C.shape[1]] = C
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(M, W).astype(np.uint64)


def unpack_bits(bits, M: int) -> np.ndarray:
    b = np.ascontiguousarray(np.asarray(bits).astype("<u8")).view(np.uint8).reshape(bits.shape[0], -1)
    return np.unpackbits(b, axis=1, bitorder="little")[:, :M].astype(bool)


def second_order(C) -> np.ndarray:
    """S2 [M, M] int32 through one float32 product (exact: every count is an integer below 2^24)."""
    M = C.shape[0]
    if M > HOST_MAX_M:
        raise ValueError(f"the host restatement takes M <= {HOST_MAX_M}")
    f = np.asarray(C, np.float32)
    return np.where(C, np.rint(f @ f.T), 0).astype(np.int32)


def second_order_packed(bits) -> np.ndarray:
    """The same from the packed rows, literally: S2[i][j] = C[i][j] popcount(row_i & row_j).  O(M^2 W) numpy: small M only."""
    bits = np.asarray(bits, np.uint64)
    M, W = bits.shape
    out = np.zeros((M, M), np.int32)
    for i in range(M):
        both = (bits[i][None, :] & bits).view(np.uint8).reshape(M, W * 8)
        pc = _POP8[both].sum(1, dtype=np.int64)
        gate = (bits[i][np.arange(M) // 64] >> (np.arange(M) % 64).astype(np.uint64)) & np.uint64(1)
        out[i] = np.where(gate.astype(bool), pc, 0)
    return out


def select_seeds(score, seeds: int) -> np.ndarray:
    """[seeds] int32: rows by (score descending, index ascending) with score > 0, -1 padded."""
    score = np.asarray(score, np.int64)
    order = np.lexsort((np.arange(score.shape[0]), -score))
    order = order[score[order] > 0][:seeds]
    out = np.full(seeds, -1, np.int32)
    out[:len(order)] = order
    return out


def select_members(s2_row, i: int, members: int) -> np.ndarray:
    """[members] int32: i and the members - 1 rows of the largest (S2, lower j) with S2 > 0, ascending, -1 padded."""
    row = np.asarray(s2_row, np.int64)
    order = np.lexsort((np.arange(row.shape[0]), -row))
    order = order[row[order] > 0][:members - 1]
    mem = np.sort(np.concatenate([order[order != i], [i]]))
    out = np.full(members, -1, np.int32)
    out[:len(mem)] = mem
    return out


def fit_members(cs, cq, mem):
    """(T [3, 4] fp32 - zeros if fewer than 3 members -, valid, singular values [3]) of one member list (-1 padded)."""
    mem = np.asarray(mem)
    mem = mem[mem >= 0]
    if len(mem) < 3:
        return np.zeros((3, 4), np.float32), False, np.zeros(3)
    T64, S = R.kabsch64(cs[mem], cq[mem])
    with np.errstate(over="ignore", invalid="ignore"):
        T = T64.astype(np.float32)
    return T, bool(np.isfinite(T).all()), S


def consensus_pair(points_src, points_ref, corr, count: Optional[int] = None, max_dist: float = 0.05, compat_dist=None,
                   seeds: int = 64, members: int = 32, refine_iters: int = 2, T_init=None) -> Dict[str, np.ndarray]:
    """One pair through the whole rule."""
    if not 1 <= seeds <= MAX_SEEDS:
        raise ValueError("seeds out of range")
    if not 3 <= members <= MAX_MEMBERS:
        raise ValueError("members out of range")
    cs, cq, count, invalid = R.gather(points_src, points_ref, corr, count)
    M = cs.shape[0]
    thr2 = R.thr2_of(max_dist)
    C, band = compat_matrix(cs, cq, compat_dist_of(compat_dist, max_dist))
    S2 = second_order(C)
    score = S2.sum(1, dtype=np.int64)
    seed = select_seeds(score, seeds)
    mem = np.full((seeds, members), -1, np.int32)
    seed_T = np.zeros((seeds, 3, 4), np.float32)
    valid = np.zeros(seeds, bool)
    sigma = np.zeros((seeds, 3))
    for r, i in enumerate(seed):
        if i >= 0:
            mem[r] = select_members(S2[i], int(i), members)
            seed_T[r], valid[r], sigma[r] = fit_members(cs, cq, mem[r])
    cnt = np.zeros(seeds, np.int64)
    if valid.any():
        cnt[valid] = R.count_inliers(seed_T[valid], cs, cq, count, thr2)
    h = R.pick(valid, cnt)
    out = {"C": C, "band": band, "bits": pack_bits(C), "S2": S2, "score": score, "seed": seed, "seed_members": mem, "seed_T": seed_T,
           "seed_valid": valid, "seed_count": cnt, "sigma": sigma, "invalid": invalid, "h": h, "cs": cs, "cq": cq, "count": count, "M": M}
    if h < 0:
        T0 = R.IDENTITY.copy() if T_init is None else np.asarray(T_init, np.float32).reshape(3, 4)
        out.update(T=T0, T_winner=T0, stats=np.array([0.0, 0.0, -1.0, 0.0, 0.0]))
        return out
    Ts, cnts = R.refit_sequence(seed_T[h], cs, cq, count, thr2, refine_iters)
    T, stats = R.finish(Ts, cnts, cs, cq, count, thr2, h, int(valid.sum()))
    out.update(T=T, T_winner=seed_T[h], stats=stats, refit_counts=np.array(cnts))
    return out


def consensus(points_src, points_ref, corr, counts=None, T_init=None, **kw):
    """The batch: a list of ``consensus_pair`` results (pairs are independent)."""
    return [consensus_pair(points_src[p], points_ref[p], corr[p], None if counts is None else int(counts[p]),
                           T_init=None if T_init is None else T_init[p], **kw) for p in range(len(points_src))]
