// Fused per-point head of RandLA.forward (reference network/RandLANet.py:363-367):
//   feat   = mlp_out(x)              32 -> 64, no bias, no norm        (x = last decoder block, GroupNorm+LeakyReLU lazy)
//   logits = fc_label(feat)          64 -> 64 -> 32 -> ncls, eval-BatchNorm folded, LeakyReLU(0.2) between
// Four row-wise GEMMs whose 64/64/32-wide intermediates never leave the CU, at ~1/4 of the HBM traffic and 1/4 of the
// launches.  The walk is head_mlp_body.h; this file is its two arithmetics and the launch rule.
//
// SplitOps (default): the four layers on the fp16 matrix pipe at fp32 accuracy, by the operand split of split_f16.h.  The
//   fp32 form issues 136 - 144 v_mfma_f32_16x16x4_f32 per 16 points (4.4 - 4.6 k cycles of the matrix pipe: it is bound by
//   it); this one 51 - 54 fp16 MFMAs (0.8 k cycles) plus ~6 VALU instructions per activation for the split.  Weights are
//   split once at load (dsir_finalize_weights); activations are split when they are read back as the next layer's A
//   fragments (lane (fr, fq): row fr, channels 8 fq .. + 7 of each 32-channel k-step).  Results are within ~1e-6
//   (relative to the layer's scale) of the fp32 form's.
// F32Ops (dsir_enable_agg_split(0) / DSIR_AGG_F32=1): exact-fp32 MFMAs in the k order pw_stream.hip uses for the same shapes
//   (lane (r,q) holds channels [q*C/4,(q+1)*C/4) of row r), so the results are bit-identical to the four separate
//   launches this kernel replaces (DSIR_NO_HEAD=1; tests/test_gpu_chain_forms.py).  The reference of the split form.
#include <hip/hip_fp16.h>

#include "head_mlp_body.h"
#include "split_f16.h"

namespace dsir {

namespace {

struct F32Ops {
  template <int K> struct A { float v[K / 4]; };   // channels (K / 4) fq .. of the lane's row
  template <int K> struct W { float v[K / 4]; };   // the same channels of one weight row

  template <int K>
  static __device__ __forceinline__ void load(const HeadArgs& p, int layer, int col, int ncols, int fq, W<K>& w) {
    const float* Wm = layer == 0 ? p.W1 : layer == 1 ? p.W2 : layer == 2 ? p.W3 : p.W4;
    if (col < ncols) {
#pragma unroll
      for (int i = 0; i < K / 16; ++i) {
        const float4 t = *reinterpret_cast<const float4*>(Wm + (int64_t)col * K + (K / 4) * fq + 4 * i);
        w.v[4 * i] = t.x; w.v[4 * i + 1] = t.y; w.v[4 * i + 2] = t.z; w.v[4 * i + 3] = t.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < K / 4; ++i) w.v[i] = 0.f;
    }
  }
  static __device__ __forceinline__ void pack(const float (&v)[8], A<32>& a) {
#pragma unroll
    for (int j = 0; j < 8; ++j) a.v[j] = v[j];
  }
  template <int K>
  static __device__ __forceinline__ void read(const float* Trow, int fq, A<K>& a) {
#pragma unroll
    for (int i = 0; i < K / 16; ++i) {
      const float4 v = *reinterpret_cast<const float4*>(Trow + (K / 4) * fq + 4 * i);
      a.v[4 * i] = v.x; a.v[4 * i + 1] = v.y; a.v[4 * i + 2] = v.z; a.v[4 * i + 3] = v.w;
    }
  }
  template <int K, int NTL>
  static __device__ __forceinline__ void mma(f32x4 (&acc)[NTL], const A<K>& a, const W<K> (&w)[NTL]) {
#pragma unroll
    for (int s = 0; s < K / 4; ++s)
#pragma unroll
      for (int t = 0; t < NTL; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[s], w[t].v[s], acc[t], 0, 0, 0);
  }
};

struct SplitOps {
  template <int K> struct A { h8 h[K / 32], l[K / 32]; };   // k-step s: channels 32 s + 8 fq .. + 7 of the lane's row, high / low
  template <int K> struct W { h8 h[K / 32], l[K / 32]; };   // the same channels of one weight row

  template <int K>
  static __device__ __forceinline__ void load(const HeadArgs& p, int layer, int col, int ncols, int fq, W<K>& w) {
    const _Float16* Wh = reinterpret_cast<const _Float16*>(p.Wh[layer]);
    const _Float16* Wl = reinterpret_cast<const _Float16*>(p.Wl[layer]);
#pragma unroll
    for (int s = 0; s < K / 32; ++s) {
      if (col < ncols) {
        w.h[s] = *reinterpret_cast<const h8*>(Wh + (int64_t)col * K + 32 * s + 8 * fq);
        w.l[s] = *reinterpret_cast<const h8*>(Wl + (int64_t)col * K + 32 * s + 8 * fq);
      } else {
        w.h[s] = h8{0, 0, 0, 0, 0, 0, 0, 0};
        w.l[s] = h8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
  }
  static __device__ __forceinline__ void pack(const float (&v)[8], A<32>& a) { split8(v, a.h[0], a.l[0]); }
  template <int K>
  static __device__ __forceinline__ void read(const float* Trow, int fq, A<K>& a) {
#pragma unroll
    for (int s = 0; s < K / 32; ++s) {
      const float4* q = reinterpret_cast<const float4*>(Trow + 32 * s + 8 * fq);
      split8(q[0], q[1], a.h[s], a.l[s]);
    }
  }
  template <int K, int NTL>
  static __device__ __forceinline__ void mma(f32x4 (&acc)[NTL], const A<K>& a, const W<K> (&w)[NTL]) {
#pragma unroll
    for (int t = 0; t < NTL; ++t)
#pragma unroll
      for (int s = 0; s < K / 32; ++s) mma3(acc[t], a.h[s], a.l[s], w[t].h[s], w[t].l[s]);
  }
};

template <int NT4>
__global__ __launch_bounds__(256) void head_mlp_kernel(const HeadArgs p) { headm::head_mlp_body<F32Ops, NT4>(p); }
template <int NT4>
__global__ __launch_bounds__(256) void head_mlp_h_kernel(const HeadArgs p) { headm::head_mlp_body<SplitOps, NT4>(p); }

}  // namespace

bool launch_head_mlp(const HeadArgs& a, bool split, hipStream_t st) {
  if (a.M <= 0 || a.clouds <= 0) return true;
  if (a.in.C != 32 || (a.in.ld % 4) != 0 || (a.in.cloud_stride % 4) != 0 || a.in.idx) return false;
  if (a.ncls < 1 || a.ncls > 32 || !a.logits_out) return false;
  if (reinterpret_cast<uintptr_t>(a.in.x) % 16) return false;
  if (split) {
    for (int k = 0; k < 4; ++k)
      if (!a.Wh[k] || !a.Wl[k]) return false;
  } else if ((reinterpret_cast<uintptr_t>(a.W1) | reinterpret_cast<uintptr_t>(a.W2) | reinterpret_cast<uintptr_t>(a.W3) |
              reinterpret_cast<uintptr_t>(a.W4)) % 16) {
    return false;
  }
  const int ntiles = (a.M + 15) / 16;
  int blocks = (ntiles + 31) / 32;              // ~8 tiles per wave: the weight fragments are loaded once per wave
  if (blocks < 16) blocks = (ntiles + 3) / 4 < 16 ? (ntiles + 3) / 4 : 16;
  if (blocks < 1) blocks = 1;
  const dim3 grid(blocks, a.clouds);
  const bool wide = a.ncls > 16;
  auto k = split ? (wide ? head_mlp_h_kernel<2> : head_mlp_h_kernel<1>) : (wide ? head_mlp_kernel<2> : head_mlp_kernel<1>);
  hipLaunchKernelGGL(k, grid, dim3(256), 0, st, a);
  return true;
}

}  // namespace dsir
