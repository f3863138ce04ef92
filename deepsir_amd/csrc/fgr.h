// Fast global registration (fgr.hip): what the host has to agree with the kernels about - the key of a tuple trial, the number
// of trials, the bounds of the row list, and the scratch - as plain C++ that compiles for the host and the device alike, so that it
// can be exercised from a host-only program: tools/fgr_check.cpp, built with the address and undefined-behaviour sanitizers and run
// on the CPU (its header gives the command).  The rule itself is stated in the header of fgr.hip and restated in deepsir_amd/fgr.py.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "icp_plane.h"    // DSIR_HD, the 6 x 6 solve and the update the optimisation shares with the point-to-plane ICP
#include "op_layouts.h"   // PoseLayout and CandLayout: the head and the end of every pose-from-correspondences stage's scratch

namespace dsir {

constexpr int kFgrBlock = 256;        // trials (tuple_test == 0: rows) one selection workgroup evaluates; also the optimise workgroup
constexpr int kFgrTrialsPerRow = 100; // trials = min(kFgrTrialsPerRow x count, max_trials)
constexpr int kFgrSums = 29;          // A (21, upper triangle by rows: icp_plane_tri), b (6), the energy, the rows

// splitmix64 (Vigna) as device_utils.h states it for the kernels, here for both sides; the static_assert pins the published vector
DSIR_HD constexpr uint64_t fgr_mix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static_assert(fgr_mix64(0) == 0xE220A8397B1DCDAFull, "splitmix64");

// the key scheme of dsir_ransac_correspondence, a trial in the place of a hypothesis
DSIR_HD constexpr uint64_t fgr_pair_key(uint64_t seed, int pair) { return fgr_mix64(seed ^ ((uint64_t)pair << 40)); }
DSIR_HD constexpr int fgr_trial_row(uint64_t pair_key, int trial, int k, int count) {
  return (int)(((fgr_mix64(pair_key ^ ((uint64_t)trial << 8) ^ (uint64_t)k) >> 32) * (uint64_t)(count < 0 ? 0 : count)) >> 32);
}

// trials of a pair with `count` live rows
DSIR_HD constexpr int fgr_trials(int count, int max_trials) {
  const int64_t t = (int64_t)kFgrTrialsPerRow * (count < 0 ? 0 : count);
  return (int)(t < (int64_t)max_trials ? t : (int64_t)max_trials);
}
// what the selection walks per pair: trials (the largest any pair can have), or with tuple_test == 0 the M rows themselves
DSIR_HD constexpr int fgr_candidates(int tuple_test, int M, int max_trials) { return tuple_test ? fgr_trials(M, max_trials) : M; }
DSIR_HD constexpr int fgr_blocks(int candidates) { return (int)(((int64_t)candidates + kFgrBlock - 1) / kFgrBlock); }
// rows an accepted candidate adds to the list, the most candidates a list takes, and the list's length in rows
DSIR_HD constexpr int fgr_rows_per(int tuple_test) { return tuple_test ? 3 : 1; }
DSIR_HD constexpr int fgr_accept_cap(int tuple_test, int M, int max_tuples) { return tuple_test ? max_tuples : M; }
DSIR_HD constexpr int64_t fgr_list_rows(int tuple_test, int M, int max_tuples) {
  return (int64_t)fgr_rows_per(tuple_test) * fgr_accept_cap(tuple_test, M, max_tuples);
}
// rows of a pair's list, from the number of candidates it accepted
DSIR_HD constexpr int64_t fgr_n_rows(int tuple_test, int M, int max_tuples, int64_t accepted) {
  const int64_t cap = fgr_accept_cap(tuple_test, M, max_tuples);
  return (int64_t)fgr_rows_per(tuple_test) * (accepted < cap ? accepted : cap);
}

// What dsir_fgr_correspondence and launch_fgr take: the selection grids carry the pairs on grid.y (pairs <= 65535), and one int32
// prefix sum ranks the accepted candidates of ALL pairs over blocks of kFgrBlock trials (or, without the tuple test, rows)
DSIR_HD constexpr bool fgr_shape_ok(int pairs, int M, int max_trials) {
  return pairs <= 65535 && (int64_t)pairs * ((int64_t)max_trials + kFgrBlock) <= 0x7fffffffll && pose_corr_shape_ok(pairs, M);
}

// launch_fgr: the PoseLayout head, then rows [P][L] int32, the selection's block counts and their exclusive prefix [P x blocks]
// int32, the scan's temporary, the normalised points [P][L][6] float64 and the single candidate pose of the tail
struct FgrLayout {
  PoseLayout pose;
  size_t rows, blk_cnt, blk_pre, tmp, npts;
  CandLayout hyp;
  size_t bytes;
  FgrLayout(int pairs, int M, int tuple_test, int max_tuples, int max_trials, int refine_iters, size_t scan_tmp)
      : pose(pairs, M, refine_iters) {
    const size_t P = (size_t)pairs, L = (size_t)fgr_list_rows(tuple_test, M, max_tuples);
    const size_t NB = (size_t)fgr_blocks(fgr_candidates(tuple_test, M, max_trials));
    Carve c{pose.bytes};
    rows = c.take(P * L * 4);
    blk_cnt = c.take(P * NB * 4); blk_pre = c.take(P * NB * 4);
    tmp = c.take(scan_tmp);
    npts = c.take(P * L * 48);
    hyp.take(c, P, 1);
    bytes = c.p;
  }
};

}  // namespace dsir
