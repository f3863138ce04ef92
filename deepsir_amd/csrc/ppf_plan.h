// Host-side sizes of the point-pair-feature layer's launches and scratch (ppf.hip): plain C++, no device code, so that the arithmetic
// can be exercised from a host-only program: tools/ppf_plan_check.cpp, built with the address and undefined-behaviour sanitizers and
// run on the CPU (its header gives the command).  A workgroup owns kPpfPts consecutive points of one cloud (16 rows each), a function of
// n alone: it fixes the partition - hence the summation order - of the forward statistics and of both backward passes.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dsir {

constexpr int kPpfPts = 64;           // points per workgroup (four rows per lane)
constexpr int kPpfSaved = 32;         // floats per cloud kept for the backward: scale[12], shift[12], {mean, rstd}[4]
constexpr int kPpfSums = 24;          // pass A, per cloud: d beta[12], d gamma[12] (fp64)
constexpr int kPpfDw = 132;           // pass B: dW [12][10] then db [12] (fp64 partials)
constexpr int kPpfMaxBlocks = 1 << 12;   // kGnMaxContrib: the forward statistics' exact limbs hold for that many contributions

inline int ppf_blocks(int n) { return n <= 0 ? 0 : (int)(((int64_t)n + kPpfPts - 1) / kPpfPts); }

// does (clouds, n) fit the launches?  (one workgroup per 64 points and cloud in a 1-D grid)
inline bool ppf_shape_ok(int clouds, int n) {
  if (clouds < 1 || n < 1) return false;
  const int bpc = ppf_blocks(n);
  return bpc <= kPpfMaxBlocks && (int64_t)bpc * clouds <= 0x7fffffffll;
}

// forward: the statistics' limb slots, [clouds][4 groups][4 words] doubles
inline size_t ppf_fwd_scratch_bytes(int clouds, int n) {
  return ppf_shape_ok(clouds, n) ? (size_t)clouds * 16 * sizeof(double) : 0;
}

// backward, in doubles: sums [clouds][24] | partial A [clouds][bpc][24] | partial B [clouds][bpc][132]
struct PpfBwdPlan { int bpc; size_t sums, part_a, part_b, total; };      // offsets and total in doubles
inline PpfBwdPlan ppf_bwd_plan(int clouds, int n) {
  PpfBwdPlan p = {0, 0, 0, 0, 0};
  if (!ppf_shape_ok(clouds, n)) return p;
  p.bpc = ppf_blocks(n);
  const size_t blocks = (size_t)clouds * (size_t)p.bpc;
  p.sums = 0;
  p.part_a = (size_t)clouds * kPpfSums;
  p.part_b = p.part_a + blocks * kPpfSums;
  p.total = p.part_b + blocks * kPpfDw;
  return p;
}
inline size_t ppf_bwd_scratch_bytes(int clouds, int n) { return ppf_bwd_plan(clouds, n).total * sizeof(double); }

}  // namespace dsir
