// Stand-alone host check of deepsir_amd/csrc/search_plan.h (which arg-min path a registration's descriptor search takes, and the
// byte sizes of its operand set) under AddressSanitizer + UndefinedBehaviorSanitizer: host code only, runs on the CPU, no GPU and
// no Python loader involved.
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Ideepsir_amd/csrc tools/search_plan_check.cpp -o /tmp/search_plan_check && /tmp/search_plan_check
// (any host C++17 compiler with -fsanitize=address,undefined does as well: the header has no device code.  The sanitizer run is this
// manual command; tests/test_cabi.py::test_host_only_plan_checks builds this file and tools/ppf_plan_check.cpp as plain host C++,
// without a sanitizer, and runs them - the first test hook either plan check has.)
// The mode function is walked across each of its edges - the screening threshold on P J K, prune_min_points on K, prune_min_rows on P J, an unsupported shape, forced correspondences, screening switched
// off - and at every stop the operand sizes must be the registration's: P J 64 2 bytes per src half, P K 64 2 per ref half, one float
// per row for the norms, nothing outside the screened modes.  The geometry of the exact search (nn_match_plan, nn_topk_plan) is held
// to recorded values at the shapes the project runs and at its edges - the two-row-tile threshold, the 8-tiles-per-split edge, the row
// list, forced row tiles and splits - with the grid's invariants checked at every stop.  Failures exit non-zero (no assert: the checks hold under NDEBUG too).
#include <cstdio>
#include <cstdlib>
#include "search_plan.h"
using namespace dsir;

static int checks = 0;
#define CHECK(x) do { ++checks; if (!(x)) { std::fprintf(stderr, "search_plan_check: %s failed (line %d)\n", #x, __LINE__); std::exit(1); } } while (0)

static SearchMode mode_and_sizes(const SearchSwitches& s, int P, int J, int K, bool forced, bool supported) {
  const SearchMode m = search_mode(s, P, J, K, forced, supported);
  const SearchOperandBytes b = search_operand_bytes(m, P, J, K);
  if (m == SearchMode::screened || m == SearchMode::pruned) {
    CHECK(search_screens(m));
    CHECK(b.a_half == (size_t)P * J * 64 * 2 && b.b_half == (size_t)P * K * 64 * 2);
    CHECK(b.a_half == (size_t)P * J * 128 && b.b_half == (size_t)P * K * 128);      // the stand-alone entry points' spelling
    CHECK(b.sa == (size_t)P * J * 4 && b.sb == (size_t)P * K * 4);
  } else {
    CHECK(!search_screens(m));
    CHECK(b.a_half == 0 && b.b_half == 0 && b.sa == 0 && b.sb == 0);
  }
  return m;
}

// ---- geometry of the exact search: nn_match_plan / nn_topk_plan.  The expected values are what the launchers' own arithmetic gave
// before it moved into search_plan.h (computed once by a host program holding that arithmetic verbatim): the plan must not move.
struct PlanCase { int P, J, K, rowlist_rows, force_rt, force_splits, rt, rb_count, splits, cols; };

static void plan_invariants(const ExactPlan& p, int P, int rows, int K, bool forced_splits) {
  CHECK(p.rt == 1 || p.rt == 2 || p.rt == 4);
  CHECK(p.cols_per_split > 0 && p.cols_per_split % 64 == 0);
  CHECK((int64_t)p.splits * p.cols_per_split >= K && K > (int64_t)(p.splits - 1) * p.cols_per_split);   // every split holds a column
  CHECK(p.splits >= 1 && (forced_splits || p.splits <= 16));
  CHECK((int64_t)p.rb_count * 64 * p.rt >= rows && (int64_t)(p.rb_count - 1) * 64 * p.rt < rows);
  CHECK(p.blocks(P) == (int64_t)P * p.rb_count * p.splits && p.blocks(P) > 0);
}

static void check_exact_plans() {
  const int gm5000 = 5000 / 4 + 1;   // the row-list launch's gate_min as nn_screen.hip passes it: J / 4 + 1 (or DSIR_SCREEN_OVF_MIN)
  const PlanCase match[] = {
      // dense
      {1, 5000, 5000, 0, 0, 0, 1, 79, 9, 576},        // one residency round: the cost model's 9 splits, not the balance formula's 10 (below)
      {2, 5000, 5000, 0, 0, 0, 1, 79, 6, 896},
      {128, 5000, 5000, 0, 0, 0, 2, 40, 1, 5056},
      {256, 5000, 5000, 0, 0, 0, 2, 40, 1, 5056},
      {1, 1, 1, 0, 0, 0, 1, 1, 1, 64},
      {1, 70, 63, 0, 0, 0, 1, 2, 1, 64},
      {128, 129, 70, 0, 0, 0, 2, 2, 1, 128},          // tests/test_gpu_exact_search_rt2.py: two row tiles at the threshold itself
      {127, 129, 70, 0, 0, 0, 1, 3, 1, 128},          // one pair fewer: one row tile
      // the 8-tiles-per-split edge
      {1, 5000, 511, 0, 0, 0, 1, 79, 1, 512},
      {1, 5000, 512, 0, 0, 0, 1, 79, 1, 512},
      {1, 5000, 513, 0, 0, 0, 1, 79, 1, 576},
      {1, 5000, 1023, 0, 0, 0, 1, 79, 2, 512},
      {1, 5000, 1024, 0, 0, 0, 1, 79, 2, 512},
      {1, 5000, 1025, 0, 0, 0, 1, 79, 2, 576},
      {128, 5000, 511, 0, 0, 0, 2, 40, 1, 512},
      {128, 5000, 512, 0, 0, 0, 2, 40, 1, 512},
      {128, 5000, 513, 0, 0, 0, 2, 40, 1, 576},
      {128, 5000, 1023, 0, 0, 0, 2, 40, 1, 1024},
      {128, 5000, 1024, 0, 0, 0, 2, 40, 1, 1024},
      {128, 5000, 1025, 0, 0, 0, 2, 40, 1, 1088},
      // the largest accepted launch: products in 64 bits
      {4096, 1 << 20, 1 << 20, 0, 0, 0, 2, 8192, 1, 1 << 20},
      // row list: gate_min = J / 4 + 1 below J, equal to J (J = 1), and forced above J
      {1, 5000, 5000, gm5000, 0, 0, 1, 20, 9, 576},
      {128, 5000, 5000, gm5000, 0, 0, 1, 20, 9, 576},
      {1, 1, 1, 1, 0, 0, 1, 1, 1, 64},
      {1, 70, 63, 18, 0, 0, 1, 1, 1, 64},
      {128, 129, 70, 33, 0, 0, 1, 1, 1, 128},
      {2, 16384, 16384, 4097, 0, 0, 1, 65, 16, 1024},
      {1, 5000, 1024, gm5000, 0, 0, 1, 20, 2, 512},
      {2, 70, 5000, 100, 0, 0, 1, 2, 9, 576},
      {2, 5000, 5000, gm5000, 4, 3, 1, 20, 3, 1728},  // a row list keeps one row tile whatever DSIR_MATCH_RT says
      // forced row tiles (3 is no value: ignored)
      {1, 5000, 5000, 0, 1, 0, 1, 79, 9, 576},
      {128, 5000, 5000, 0, 1, 0, 1, 79, 1, 5056},
      {1, 5000, 5000, 0, 2, 0, 2, 40, 10, 512},
      {128, 5000, 5000, 0, 2, 0, 2, 40, 1, 5056},
      {1, 5000, 5000, 0, 4, 0, 4, 20, 10, 512},
      {128, 5000, 5000, 0, 4, 0, 4, 20, 3, 1728},
      {1, 5000, 5000, 0, 3, 0, 1, 79, 9, 576},
      {128, 5000, 5000, 0, 3, 0, 2, 40, 1, 5056},
      // forced splits, up to and above the tile count (79 tiles)
      {1, 5000, 5000, 0, 0, 1, 1, 79, 1, 5056},
      {1, 5000, 5000, 0, 0, 9, 1, 79, 9, 576},
      {1, 5000, 5000, 0, 0, 16, 1, 79, 16, 320},
      {1, 5000, 5000, 0, 0, 79, 1, 79, 79, 64},
      {1, 5000, 5000, 0, 0, 80, 1, 79, 79, 64},
      {1, 5000, 5000, 0, 0, 1000, 1, 79, 79, 64},
      {1, 70, 63, 0, 0, 5, 1, 2, 1, 64},
  };
  for (const PlanCase& c : match) {
    const ExactPlan p = nn_match_plan(c.P, c.J, c.K, c.rowlist_rows, c.force_rt, c.force_splits);
    CHECK(p.rt == c.rt && p.rb_count == c.rb_count && p.splits == c.splits && p.cols_per_split == c.cols);
    plan_invariants(p, c.P, c.rowlist_rows > 0 && c.rowlist_rows < c.J ? c.rowlist_rows : c.J, c.K, c.force_splits > 0);
  }
  {
    const ExactPlan p = nn_match_plan(4096, 1 << 20, 1 << 20, 0, 1, 1 << 20);   // 2^12 pairs x 2^14 row blocks x 2^14 one-tile splits
    CHECK(p.rt == 1 && p.rb_count == 16384 && p.splits == 16384 && p.cols_per_split == 64 && p.blocks(4096) == ((int64_t)1 << 40));
  }
  // the two split rules at one pair of 5000 x 5000 (79 row blocks, 79 tiles): the note beside match_splits_one_round
  CHECK(match_splits_balance(79, 79, 1024) == 10 && match_splits_one_round(79, 79) == 9);

  // top-k: {P, J, K, kk, rt, rb_count, splits, cols}
  const int topk[][8] = {
      {1, 5000, 5000, 2, 1, 79, 7, 768},     {1, 5000, 5000, 8, 1, 79, 7, 768},     {2, 5000, 5000, 2, 1, 79, 4, 1280},
      {128, 5000, 5000, 2, 2, 40, 1, 5056},  {128, 5000, 5000, 4, 2, 40, 1, 5056},  {128, 5000, 5000, 8, 1, 79, 1, 5056},
      {256, 5000, 5000, 2, 2, 40, 1, 5056},  {1, 1, 1, 2, 1, 1, 1, 64},             {1, 1, 1, 8, 1, 1, 1, 64},
      {1, 70, 63, 2, 1, 2, 1, 64},           {128, 129, 70, 2, 2, 2, 1, 128},       {128, 129, 70, 8, 1, 3, 1, 128},
      {64, 385, 70, 2, 2, 4, 1, 128},        {64, 385, 70, 4, 2, 4, 1, 128},        {64, 385, 70, 8, 1, 7, 1, 128},   // test_gpu_exact_search_rt2.py
      {63, 385, 70, 2, 1, 7, 1, 128},        {64, 384, 70, 4, 1, 6, 1, 128},
      {1, 5000, 1023, 2, 1, 79, 2, 512},     {1, 5000, 1025, 8, 1, 79, 2, 576},     {128, 5000, 1025, 2, 2, 40, 1, 1088},
      {4096, 1 << 20, 1 << 20, 2, 2, 8192, 1, 1 << 20}, {4096, 1 << 20, 1 << 20, 8, 1, 16384, 1, 1 << 20},
  };
  for (const auto& c : topk) {
    const ExactPlan p = nn_topk_plan(c[0], c[1], c[2], c[3]);
    CHECK(p.rt == c[4] && p.rb_count == c[5] && p.splits == c[6] && p.cols_per_split == c[7]);
    plan_invariants(p, c[0], c[1], c[2], false);
    CHECK(p.rt == 1 || c[3] <= 4);                     // two row tiles only beside lists of 2 or 4
  }
  CHECK(topk_kk(1) == 2 && topk_kk(2) == 2 && topk_kk(3) == 4 && topk_kk(4) == 4 && topk_kk(5) == 8 && topk_kk(8) == 8);
}

int main() {
  const SearchSwitches dflt = {1, 8192, 65536, kScreenMinWork};
  CHECK(kScreenMinWork == 100000000ll);
  // the screening threshold: P J K one below and at it (P J K = 2 x 5000 x 10000 = 1e8)
  CHECK(mode_and_sizes(dflt, 2, 5000, 9999, false, true) == SearchMode::exhaustive);
  CHECK((long long)2 * 5000 * 9999 == kScreenMinWork - 10000);
  CHECK(mode_and_sizes(dflt, 2, 5000, 10000, false, true) == SearchMode::screened);     // P J = 10000 < prune_min_rows
  {
    const SearchSwitches s = {1, 8192, 65536, 1001};      // an exact edge: 1 x 7 x 143 = 1001
    CHECK(mode_and_sizes(s, 1, 7, 143, false, true) == SearchMode::screened);
    CHECK(mode_and_sizes(s, 1, 7, 142, false, true) == SearchMode::exhaustive);
    const SearchSwitches t = {1, 8192, 65536, 1002};
    CHECK(mode_and_sizes(t, 1, 7, 143, false, true) == SearchMode::exhaustive);          // one below the threshold
  }
  // K one below and at prune_min_points (rows and work far above their thresholds)
  CHECK(mode_and_sizes(dflt, 16, 8192, 8191, false, true) == SearchMode::screened);
  CHECK(mode_and_sizes(dflt, 16, 8192, 8192, false, true) == SearchMode::pruned);
  // P J one below and at prune_min_rows: 65535 = 3 x 21845, 65536 = 4 x 16384
  CHECK(mode_and_sizes(dflt, 3, 21845, 16384, false, true) == SearchMode::screened);
  CHECK(mode_and_sizes(dflt, 4, 16384, 16384, false, true) == SearchMode::pruned);
  // the kernels' own envelope says no
  CHECK(mode_and_sizes(dflt, 4, 16384, 16384, false, false) == SearchMode::screened);
  // forced correspondences win over everything
  CHECK(mode_and_sizes(dflt, 4, 16384, 16384, true, true) == SearchMode::forced);
  CHECK(mode_and_sizes(dflt, 1, 1024, 1024, true, false) == SearchMode::forced);
  // screening switched off: exhaustive throughout, pruning included
  {
    const SearchSwitches off = {0, 8192, 65536, kScreenMinWork};
    CHECK(mode_and_sizes(off, 4, 16384, 16384, false, true) == SearchMode::exhaustive);
    CHECK(mode_and_sizes(off, 4, 16384, 16384, true, true) == SearchMode::forced);
  }
  // pruning switched off (prune_min_points = 0), and the lowered thresholds of the tests' hooks
  {
    const SearchSwitches nop = {1, 0, 65536, kScreenMinWork};
    CHECK(mode_and_sizes(nop, 4, 16384, 16384, false, true) == SearchMode::screened);
    const SearchSwitches low = {1, 1024, 0, 1};
    CHECK(mode_and_sizes(low, 2, 1100, 1024, false, true) == SearchMode::pruned);
    CHECK(mode_and_sizes(low, 2, 1100, 1023, false, true) == SearchMode::screened);
    CHECK(mode_and_sizes(low, 1, 1, 1, false, false) == SearchMode::screened);
  }
  // the largest accepted launch: the products stay in 64 bits (max_points 2^20, 4096 pairs)
  CHECK(mode_and_sizes(dflt, 4096, 1 << 20, 1 << 20, false, false) == SearchMode::screened);
  CHECK(search_operand_bytes(SearchMode::screened, 4096, 1 << 20, 1 << 20).a_half == ((size_t)1 << 39));
  check_exact_plans();
  std::printf("search_plan: %d checks passed\n", checks);
  return 0;
}
