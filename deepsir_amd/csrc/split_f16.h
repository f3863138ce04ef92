// The fp16 operand split: fp32 contractions on the fp16 matrix pipe, at fp32 accuracy.
//
// gfx950 has no TF32, and v_mfma_f32_16x16x4_f32 is the slowest matrix rate of the chip (157 TFLOP/s); its fp16 MFMA runs
// 16 x faster and accumulates in fp32.  So each fp32 operand is split into two fp16 numbers,
//       x = xh + xl + r,   xh = fp16(x),  xl = fp16(x - xh),   |r| <= max(2^-22 |x|, 2^-25)
// (x - xh is exact in fp32; fp16 subnormals are honoured by the matrix core - tools/ubench/mfma_denorm.hip), and
//       a.b = ah.bh + ah.bl + al.bh  (+ al.bl + r-terms <= 4 2^-22 |a||b| + 2^-25 (|a|_1 + |b|_1): dropped)
// is three v_mfma_f32_16x16x32_f16 (every product of two fp16 numbers is exact in fp32; the sum is accumulated in fp32 by
// the matrix core, whose accumulation error was measured at <= 12 fp32 roundings per 192 products,
// tests/test_gpu_screen_bound.py).  Per dot product that is the error fp32 arithmetic itself makes in a 64..256-term sum
// (K 2^-24 |a||b|), at 3/16 of the fp32 MFMA time.
// "fp32 accuracy" holds in one magnitude band only.  Per output the error is at most
//       B(a, b) = sum_k (ra_k |b_k| + |a_k| rb_k + |al_k| |bl_k|) + (K / 16 + 1) 2^-24 sum_k |a_k b_k|,
// and the floor 2^-25 of r is ABSOLUTE (the fp16 sub-normal spacing): below |x| ~ 2^-3 the low part is sub-normal and the
// product's relative error grows like 1 / |x| (weights x 2^-10 at K = 256: 5e-5 of |a||b| against fp32's 1e-7;
// tests/test_split_model_host.py).  |x| > 65504 (or a non-finite x) makes the result non-finite.
// Domain, weights: a matrix is contracted split only if all its entries are within the fp16 range and its two parts carry it
// to 2^-19 of its Frobenius norm (split_in_domain, weights.hip, decided at load).  Any other matrix runs in its layer's
// exact-fp32 kernel; agg_chain.hip and head_mlp.hip take all their matrices split or none.  He-normal matrices and trained
// ones of like size are inside; the same matrices times 2^-6 or 2^+20 are outside.  tests/test_gpu_split_magnitudes.py pins the result:
// rescalings of a state dict that preserve its function keep every output within the oracle tolerances.
// The one exception is att_pool.hip's score contraction, which has no fp32 twin: its scores feed a softmax, where the absolute
// error counts, and that stays <= 2^-25 |f|_1 however small fc is; an fc entry above 65504 gives non-finite output.
// Domain, activations (split in the kernels, as they are): the same floor.  Every split layer reads either GroupNorm / LeakyReLU
// outputs of O(1) or caller-supplied rows (dsir_aggregate's feat0: pinned at 2^-12 .. 2^10 times N(0, 1)) whose product is added
// to a bias of O(0.1), against which 2^-25 |w|_1 is nothing.  A chain whose INNER activations are tiny or beyond 65504 by a
// BatchNorm gain has a matrix outside the weight domain next to them, and runs in fp32 for that reason.
//
// The order of the three products decides bits: every kernel that contracts split operands issues them through mma3.
// Weights are split once at load (split_weights_f16, weights.hip: the same rule on the host).
// screen_split4 (device_utils.h) is a DIFFERENT rule - pre-scaled parts, no subnormals in the high part - for the screened search.
#pragma once
#include "device_utils.h"

namespace dsir {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

// the rule, per element
__device__ __forceinline__ void split1(const float x, _Float16& h, _Float16& l) {
  h = (_Float16)x;
  l = (_Float16)(x - (float)h);
}

template <int N, class V>
__device__ __forceinline__ void split_n(const float* x, V& h, V& l) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    _Float16 t, u;
    split1(x[k], t, u);
    h[k] = t;
    l[k] = u;
  }
}
__device__ __forceinline__ void split8(const float* x, h8& h, h8& l) { split_n<8>(x, h, l); }
__device__ __forceinline__ void split8(const float4 u, const float4 v, h8& h, h8& l) {
  const float f[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
  split_n<8>(f, h, l);
}
__device__ __forceinline__ void split4(const float4 v, h4& h, h4& l) {
  const float f[4] = {v.x, v.y, v.z, v.w};
  split_n<4>(f, h, l);
}

// acc += a.b over one 32-channel k-step of split operands: al.bh, ah.bl, ah.bh, in that order
__device__ __forceinline__ void mma3(f32x4& acc, const h8 ah, const h8 al, const h8 bh, const h8 bl) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc, 0, 0, 0);
}

}  // namespace dsir
