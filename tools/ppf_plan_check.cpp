// Stand-alone host check of deepsir_amd/csrc/ppf_plan.h (the launch and scratch-size arithmetic of dsir_t_ppf_fwd / dsir_t_ppf_bwd)
// under AddressSanitizer + UndefinedBehaviorSanitizer: host code only, runs on the CPU, no GPU and no Python loader involved.
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Ideepsir_amd/csrc tools/ppf_plan_check.cpp -o /tmp/ppf_plan_check && /tmp/ppf_plan_check
// (any host C++17 compiler with -fsanitize=address,undefined does as well: the header has no device code.)  Every extreme of
// (clouds, n) - negative, zero, INT_MAX, the 4096-workgroup limit and its neighbours - must be refused with size 0 or give offsets
// that tile the scratch buffer exactly.  Last run: clean, "90 shapes accepted".
#include <cassert>
#include <cstdio>
#include <climits>
#include "ppf_plan.h"
using namespace dsir;
int main() {
  const int ns[] = {INT_MIN, -1, 0, 1, 16, 63, 64, 65, 70, 1024, 1100, 5000, 262143, 262144, 262145, INT_MAX};
  const int cs[] = {INT_MIN, -1, 0, 1, 2, 3, 8, 64, 8191, 8192, 1 << 20, INT_MAX};
  long ok = 0;
  for (int n : ns) for (int c : cs) {
    const bool fits = ppf_shape_ok(c, n);
    const size_t f = ppf_fwd_scratch_bytes(c, n), b = ppf_bwd_scratch_bytes(c, n);
    const PpfBwdPlan p = ppf_bwd_plan(c, n);
    if (!fits) { assert(f == 0 && b == 0 && p.total == 0); continue; }
    ++ok;
    assert(p.bpc == (n + 63) / 64 && p.bpc <= kPpfMaxBlocks);
    assert(f == (size_t)c * 128);
    assert(p.sums == 0 && p.part_a == (size_t)c * 24 && p.part_b == p.part_a + (size_t)c * p.bpc * 24);
    assert(p.total == p.part_b + (size_t)c * p.bpc * 132 && b == p.total * 8);
    assert((int64_t)p.bpc * c <= 0x7fffffffll);
  }
  assert(ppf_blocks(INT_MAX) == 33554432 && ppf_blocks(70) == 2);
  std::printf("ppf_plan: %ld shapes accepted, all offsets consistent\n", ok);
  return 0;
}
