// Host-side decisions of the descriptor search (search.hip): which of the arg-min paths a launch takes, and the sizes of the operand
// set it needs.  Plain C++, no device code, so that the thresholds can be exercised from a host-only program:
// tools/search_plan_check.cpp, built with the address and undefined-behaviour sanitizers and run on the CPU (its header gives the
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

// Geometry of the top-k search (nn_topk.hip) for lists of kk = 2, 4 or 8 keys per row.  Row tiles per wave: 2 (128-row blocks) once
// that still leaves a workgroup per CU and the lists fit beside two sets of A fragments (kk <= 4), else 1.  Column splits: at least
// two workgroups per CU (512 in all) where the problem allows it, every split 8 tiles of 64 columns or longer so that the A-fragment
// preload and the 16-lane merge stay amortised, 16 splits at the most (the merge kernel reads them all per row).
struct TopkPlan { int rt, rb_count, splits, cols_per_split; };
inline TopkPlan nn_topk_plan(int P, int J, int K, int kk) {
  TopkPlan p;
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

}  // namespace dsir
