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
// per row for the norms, nothing outside the screened modes.  Failures exit non-zero (no assert: the checks hold under NDEBUG too).
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
  std::printf("search_plan: %d checks passed\n", checks);
  return 0;
}
