// The arithmetic of the screened descriptor search's bound, L <= D <= U = L + 2 d, once: the screening (nn_screen.hip), its
// diagnostic kernel and the bound pass of the pruned search (nn_prune.hip) all evaluate it through this header, so that
// tests/test_gpu_screen_bound.py, which proves the inequality entry by entry for screen_bounds_kernel, proves it for all of them.
// (nn_screen.hip's header derives S, d and the operand split.)
//
// Error budget, in units of M = |a|^2 + |b|^2 (|a||b| <= M/2): representation 2^-22 per element (3 2^-22 M with the
// dropped al.bl term); fp32 accumulation: both high parts are stored pre-scaled by 2^11 (exact) and the kernel forms
// z' = 2^22 (c + ah.bh) + 2^11 (ah.bl + al.bh) = 2^22 z in ONE chain of six MFMAs (192 exact fp16 products + the seed;
// a pure power-of-two scaling: the roundings are those of the unscaled sum), pessimistically one fp32 rounding per
// addition relative to the sum of the magnitudes (|a||b| + |b|^2 / 2) <= M: 198 2^-24 M on z, 2^-15.4 M after the factor 2; the reference's own
// fmaf chain 64 * 2^-24 * 2 |a||b| <= 2^-18 M; final roundings 2^-22 M: 2.8e-5 M against 2^-15 M = 3.05e-5 M (measured on
// unit descriptors: < 1e-6 against 6e-5).  Elements below 2^-25 lose their low part
// (fp16 underflow): <= 2^-25 per element, 2^-21 (|a| + |b|) <= 2^-21 (1 + M/2) on the distance: the constant term 2^-20.
// MEASURED on the matrix core (round 3; tests/test_gpu_screen_bound.py through dsir_screen_bounds, which runs screen_chain
// on the screening's operands and returns L, U and the exact D of EVERY (row, column)): 19 input regimes chosen against the
// bound - same-sign components (no cancellation in the accumulator), constant vectors / 64 identical products, components on
// fp16 rounding ties, |x| = 16, norms 1e-3 .. 30, one-hot, sparse, below the fp16 normal range, near-duplicates, geometric
// decay - x three shapes, 4.4 M entries: no entry outside [L, U]; worst |D - (L + U) / 2| = 0.066 of the half width (a margin
// of 15 on d); the accumulation error of the six chained MFMAs against an fp64 sum of the same fp16 products never exceeded
// 11.9 fp32 roundings of the magnitude sum, against the 198 budgeted above: the v_mfma_f32_16x16x32_f16 adder of gfx950 rounds
// far less often than once per product (and not by truncation: same-sign inputs err LESS than signed ones).  The bound is
// kept at its pessimistic width; the test asserts a margin of 2 so that a different stepping would be noticed.
// Elements with |x| > 16 (the 2^11 pre-scaling of the high part must stay inside fp16: 2^15 < 65504) or not finite: split16_kernel
// raises a flag and every pair is searched exhaustively (the engine's descriptors are L2-normalised, model.py:232-233,
// and never take that path).
#pragma once
#include "device_utils.h"
#include "exact_search_body.h"

namespace dsir {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

#ifndef DSIR_SCREEN_BC
#define DSIR_SCREEN_BC 64
#endif
constexpr int SBC = DSIR_SCREEN_BC;   // ref columns per LDS tile of the screening = per tile of the pruned search's column order
constexpr int kMaxBoundTiles = 4096;        // tiles of a pruned search's column order (LDS: tile flags of the bound pass, an item's tile list)
constexpr float kC1 = 1.0f / 32768.0f;      // bound width: d = kC1 (|a|^2 + |b|^2) + kC0
constexpr float kC0 = 1.0f / 1048576.0f;
constexpr float kW = 2.0f * 1.015625f;      // upper - lower bound = 2 d, with slack for the rounding of its own evaluation
constexpr float kSeedScale = -2097152.f;                // seed = 2^22 c, c = -(|b|^2 - d_b) / 2
constexpr float kLowerScale = -4.76837158203125e-7f;    // z' = 2^22 z: L = slo - 2 z = slo - 2^-21 z'
// margins of the pruned search (fp32 evaluation errors stay below 4e-6 (1 + ...); domain: see row_prep_kernel)
constexpr float kMarginExact = 2e-5f;       // (1 + |a|^2 + |b|^2): on an exact fp32 distance used as a row's upper bound T
constexpr float kMarginCentroid = 1e-5f;    // (1 + |a|^2 + |c|^2): D(a, c) against the true |a - c|^2, under the lower bound L
constexpr float kMarginRoot = 1.00002f;     // on sqrt(T) and the tile radius: the factor 1 / 0.99999 on sqrt(L) and the rounding of sqrtf

// the accumulator seed of a column: the chain's first C operand.  A column that is not live takes -INFINITY instead and never wins;
// the callers select (a flag passed through here costs the dense screen_kernel 2 VGPRs: its short-circuit is no longer threaded)
__device__ __forceinline__ float screen_seed(float sb) { return kSeedScale * (sb - kC1 * sb); }
// the row term |a|^2 - d_a
__device__ __forceinline__ float screen_slo(float sa) { return sa - kC1 * sa - kC0; }
__device__ __forceinline__ float screen_lower(float z, float slo) { return fmaf(z, kLowerScale, slo); }
__device__ __forceinline__ float screen_upper(float l, float sa, float sb) { return l + kW * (kC1 * (sa + sb) + kC0); }

// a lane's share of one 16-row (A) or 16-column (B) MFMA operand: halves 32 c + 8 fq .. +7 of `row`'s high and low parts
struct ScreenFrag { h8 h[2], l[2]; };
__device__ __forceinline__ ScreenFrag screen_frag(const _Float16* __restrict__ hi, const _Float16* __restrict__ lo, int64_t row, int fq) {
  ScreenFrag f;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    f.h[c] = *reinterpret_cast<const h8*>(hi + row * 64 + 32 * c + 8 * fq);
    f.l[c] = *reinterpret_cast<const h8*>(lo + row * 64 + 32 * c + 8 * fq);
  }
  return f;
}

// z' of 16 rows x 16 columns: THE operand order of the bound, (ah0,bh0) (ah1,bh1) (ah0,bl0) (al0,bh0) (ah1,bl1) (al1,bh1)
__device__ __forceinline__ f32x4 screen_chain(const ScreenFrag& a, const ScreenFrag& b, float seed) {
  f32x4 z = f32x4{seed, seed, seed, seed};
  z = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.h[0], b.h[0], z, 0, 0, 0);
  z = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.h[1], b.h[1], z, 0, 0, 0);
  z = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.h[0], b.l[0], z, 0, 0, 0);
  z = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.l[0], b.h[0], z, 0, 0, 0);
  z = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.h[1], b.l[1], z, 0, 0, 0);
  z = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.l[1], b.h[1], z, 0, 0, 0);
  return z;
}

// exact D(a, b) by THE RULE of exact_search_body.h in scalar code: the k-ordered fmaf chain of v_mfma_f32_16x16x4_f32 from a zero
// accumulator, then dist_from_dot.  a: the row as float4 [16] in registers, or a const float4* to it
template <typename A>
__device__ __forceinline__ float exact_dist(const A& a, const float* __restrict__ b, float san, float sbn) {
  float acc = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const float4 u = a[q], v = reinterpret_cast<const float4*>(b)[q];
    acc = fmaf(u.x, v.x, acc); acc = fmaf(u.y, v.y, acc); acc = fmaf(u.z, v.z, acc); acc = fmaf(u.w, v.w, acc);
  }
  return dist_from_dot(acc, san, sbn);
}

}  // namespace dsir
