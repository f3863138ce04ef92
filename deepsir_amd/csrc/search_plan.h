// Host-side decisions of the descriptor search (search.hip): which of the arg-min paths a launch takes, and the sizes of the operand
// set it needs; and the launch geometry and scratch layout of the exact search (nn_match.hip, nn_topk.hip).  Plain C++, no device
// code, so that the thresholds can be exercised from a host-only program: tools/search_plan_check.cpp, built with the address and undefined-behaviour sanitizers and run on the CPU (its header gives the
// command).  Every mode returns the same bits (tests/test_gpu_parity.py, tests/test_gpu_search_sites.py), so the choice is free.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dsir {

enum class SearchMode {
  forced,       // caller-supplied correspondences: no search, the indices are clamped into [0, K)
  exhaustive,   // the single exhaustive fp32 kernel (nn_match.hip)
  screened,     // fp16-screened arg-min (nn_screen.hip): split descriptors, norms, candidate scratch; decided in exact fp32
  pruned        // the screened search over row / column orders and tile lists (nn_prune.hip)
};

// the context's switches the choice depends on
struct SearchSwitches {
  int screen_mode;              // dsir_enable_screen / DSIR_NO_SCREEN: 0 = the exhaustive fp32 kernel throughout (A/B switch)
  int prune_min_points;         // pruned search for ref clouds of that many points and more; 0 = off
  long long prune_min_rows;     // ... in launches of that many src rows (pairs x points) and more
  long long screen_min_work;    // DSIR_SCREEN_MIN_WORK (A/B hook): P J K from which a registration screens
};
constexpr long long kScreenMinWork = 100000000ll;

// Both searches return the same bits: small problems (latency-bound, e.g. one pair in flight) take the single exhaustive kernel,
// large ones the three-kernel screened path.
// The pruned search is for long ref ranges (column order + tile bounds once, row order + tile lists per iteration) ... and only with
// enough rows in the launch to fill the chip with items (128 row blocks): below that the search lasts as long as its longest item
// either way and the preparation is pure cost (one 16384-point pair: 5.18 -> 5.59 ms per registration with it).
// prune_supported: nn_prune_supported(P, J, K), the kernels' own envelope.
inline SearchMode search_mode(const SearchSwitches& s, int P, int J, int K, bool forced_idx, bool prune_supported) {
  if (forced_idx) return SearchMode::forced;
  if (!s.screen_mode || (int64_t)P * J * K < s.screen_min_work) return SearchMode::exhaustive;
  const bool prune = s.prune_min_points > 0 && K >= s.prune_min_points && (int64_t)P * J >= s.prune_min_rows && prune_supported;
  return prune ? SearchMode::pruned : SearchMode::screened;
}
inline bool search_screens(SearchMode m) { return m == SearchMode::screened || m == SearchMode::pruned; }

// the operand set of the screened / pruned search: fp16 high and low parts of both sides ([rows][64] halves each) and the rows'
// squared norms; the other modes take none of it
struct SearchOperandBytes { size_t a_half, b_half, sa, sb; };
inline SearchOperandBytes search_operand_bytes(SearchMode m, int P, int J, int K) {
  if (!search_screens(m)) return {0, 0, 0, 0};
  return {(size_t)P * J * 64 * 2, (size_t)P * K * 64 * 2, (size_t)P * J * sizeof(float), (size_t)P * K * sizeof(float)};
}

// ------------------------------------------------------------------ the exact search (exact_search_body.h): geometry and scratch
// Workgroups of 4 waves, each wave rt row tiles of 16 src rows: rb_count row blocks of 64 rt rows per pair, the ref range cut into
// `splits` runs of cols_per_split columns (whole 64-column tiles); one workgroup per (pair, split, row block).
struct ExactPlan {
  int rt, rb_count, splits, cols_per_split;
  int64_t blocks(int P) const { return (int64_t)rb_count * splits * P; }
};
constexpr int kExactTile = 64;        // ref columns per LDS tile (BC of exact_search_body.h)
constexpr int kExactMinTiles = 8;     // tiles per split that keep the A-fragment preload amortised
constexpr int kExactMaxSplits = 16;

// The arg-min's candidate split counts sp = 1, 2, .. (16 at the most, while a split keeps 8 tiles): f(sp, tiles per split, splits that
// leaves after rounding to whole tiles)
template <class F>
inline void match_split_candidates(int tiles, F f) {
  for (int sp = 1; sp <= kExactMaxSplits && sp <= tiles; ++sp) {
    const int tiles_per = (tiles + sp - 1) / sp;
    if (sp > 1 && tiles_per < kExactMinTiles) break;
    f(sp, tiles_per, (tiles + tiles_per - 1) / tiles_per);
  }
}
// Column splits by residency balance: the grid as close as possible to a whole number of residency rounds (`resident` workgroups at
// once), times the padding of the last split.  base = pairs x row blocks.
inline int match_splits_balance(int64_t base, int tiles, int resident) {
  int splits = 1;
  double best_eff = -1.0;
  match_split_candidates(tiles, [&](int sp, int tiles_per, int nsp) {
    const int64_t blocks = base * nsp, rounds = (blocks + resident - 1) / resident;
    const double eff = (double)blocks / (double)(rounds * resident) * ((double)tiles / (double)(tiles_per * nsp));
    if (eff > best_eff + 1e-9) { best_eff = eff; splits = sp; }
  });
  return splits;
}
// A launch that fits the chip in ONE residency round (a single pair: 79 row blocks) is bound by the CU that gets the most
// workgroups: its matrix pipe serves ceil(blocks / 256) of them, each tiles_per tiles long plus ~2 tiles' worth of prologue /
// epilogue; one or two workgroups per CU run no faster than three (their load latencies no longer overlap).  (Measured at
// 1 x 5000 x 5000: 9 splits - this model's choice - 3.595 ms per registration, 10 splits - what match_splits_balance picks - 3.627,
// 12: 3.60, 8: 3.613, 4: 3.69.)
inline int match_splits_one_round(int64_t base, int tiles) {
  int splits = 1;
  double best_cost = 1e30;
  match_split_candidates(tiles, [&](int sp, int tiles_per, int nsp) {
    const int64_t per_cu = (base * nsp + 255) / 256;
    const double cost = (double)(per_cu < 3 ? 3 : per_cu) * (tiles_per + 2);
    if (cost < best_cost - 1e-9) { best_cost = cost; splits = sp; }
  });
  return splits;
}
// Geometry of the arg-min (nn_match.hip): 2 row tiles per wave (128-row blocks) once there is enough work, else 64-row blocks.
// rowlist_rows > 0: the row-list launch of the screening's fallback, every pair at most that many listed rows (and at most J) - few
// rows per pair: small row blocks, the ref range split as far as it goes.  force_rt (1, 2, 4) / force_splits (> 0): the tuning
// hooks DSIR_MATCH_RT / DSIR_MATCH_SPLITS, read by the launcher.
inline ExactPlan nn_match_plan(int P, int J, int K, int rowlist_rows, int force_rt, int force_splits) {
  ExactPlan p;
  p.rt = (int64_t)P * ((J + 127) / 128) >= 256 ? 2 : 1;
  if (force_rt == 1 || force_rt == 2 || force_rt == 4) p.rt = force_rt;
  if (rowlist_rows > 0) p.rt = 1;
  const int rows_per_block = 64 * p.rt;
  const int resident = p.rt == 4 ? 768 : 1024;   // workgroups the chip holds at once (VGPR- resp. LDS-limited: 256 CUs x 3 or 4)
  const int rows = rowlist_rows > 0 && rowlist_rows < J ? rowlist_rows : J;
  p.rb_count = (rows + rows_per_block - 1) / rows_per_block;
  const int64_t base = (int64_t)P * p.rb_count;
  const int tiles = (K + kExactTile - 1) / kExactTile;
  int max_nsp = 1;                               // the most splits a candidate leaves
  match_split_candidates(tiles, [&](int, int, int nsp) { max_nsp = nsp; });
  int splits;
  if (rowlist_rows > 0) splits = tiles / kExactMinTiles < 1 ? 1 : (tiles / kExactMinTiles > kExactMaxSplits ? kExactMaxSplits : tiles / kExactMinTiles);
  else if (base * max_nsp <= resident) splits = match_splits_one_round(base, tiles);
  else splits = match_splits_balance(base, tiles, resident);
  if (force_splits > 0) splits = force_splits < tiles ? force_splits : tiles;
  p.cols_per_split = ((tiles + splits - 1) / splits) * kExactTile;
  p.splits = (K + p.cols_per_split - 1) / p.cols_per_split;
  return p;
}

// Geometry of the top-k search (nn_topk.hip) for lists of kk = 2, 4 or 8 keys per row.  Row tiles per wave: 2 (128-row blocks) once
// that still leaves a workgroup per CU and the lists fit beside two sets of A fragments (kk <= 4), else 1.  Column splits: at least
// two workgroups per CU (512 in all) where the problem allows it, every split 8 tiles of 64 columns or longer so that the A-fragment
// preload and the 16-lane merge stay amortised, 16 splits at the most (the merge kernel reads them all per row).
inline ExactPlan nn_topk_plan(int P, int J, int K, int kk) {
  ExactPlan p;
  p.rt = (kk <= 4 && (int64_t)P * ((J + 127) / 128) >= 256) ? 2 : 1;
  const int rows_per_block = 64 * p.rt;
  p.rb_count = (J + rows_per_block - 1) / rows_per_block;
  const int64_t base = (int64_t)P * p.rb_count;
  const int tiles = (K + 63) / 64;
  int64_t want = (512 + base - 1) / base;
  if (want > tiles / 8) want = tiles / 8;
  if (want > 16) want = 16;
  if (want < 1) want = 1;
  const int tiles_per = (tiles + (int)want - 1) / (int)want;
  p.cols_per_split = tiles_per * 64;
  p.splits = (tiles + tiles_per - 1) / tiles_per;
  return p;
}
inline int topk_kk(int k) { return k <= 2 ? 2 : (k <= 4 ? 4 : 8); }   // list length of the kernel that serves k

// The scratch of both searches, byte offsets: sa [P J] floats | sb [P K] floats | pad to 4 floats | tail (8-byte words) of tail_bytes.
// A closed form of its own (no 256-byte parts): the arena-size refusals depend on `bytes`, and the aggregation epilogue writes the
// src norms and the arg-min's packed slots through nn_match_scratch_layout.
struct ExactScratch {
  size_t sa, sb, tail, bytes;
  ExactScratch(int P, int J, int K, size_t tail_bytes)
      : sa(0), sb((size_t)P * J * 4), tail((((size_t)P * J + (size_t)P * K + 3) & ~(size_t)3) * 4), bytes(tail + tail_bytes) {}
};
// arg-min: the tail is the packed (distance bits << 32 | index) result slots, u64 [P][J]
inline ExactScratch nn_match_scratch(int P, int J, int K) { return ExactScratch(P, J, K, (size_t)P * J * 8); }
// top-k: the tail is the splits' partial lists, u64 [P][splits][J][kk]
inline ExactScratch nn_topk_scratch(int P, int J, int K, int k) {
  const int kk = topk_kk(k);
  return ExactScratch(P, J, K, (size_t)P * nn_topk_plan(P, J, K, kk).splits * J * kk * 8);
}

}  // namespace dsir
