// The walk of the fused per-point head (head_mlp.hip), once for both arithmetics.
//
// A wave owns 16-row tiles (persistent: tile, tile + waves, ..., the next tile's rows in flight during the current one's
// MFMAs); the weight fragments of all four layers stay in registers for the whole kernel; between layers the 16 x C
// accumulator tile is transposed through a wave-private LDS tile (C layout -> row-per-lane A fragments).
// Ops is the arithmetic: A<K> / W<K>, the fragments of a lane's row / of one weight row over K input channels, with their
// load, read-back and contraction.
#pragma once
#include "kernels.h"
#include "device_utils.h"

namespace dsir {
namespace headm {

constexpr int LDT = 64 + 4;   // transposition tile row (floats): 16-byte aligned rows, conflict-free both ways

template <class Ops, int NT4>
__device__ __forceinline__ void head_mlp_body(const HeadArgs& p) {
  __shared__ float s_sc[32], s_sh[32];
  __shared__ float s_T[4][16 * LDT];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int cloud = blockIdx.y;

  if (tid < 32) {
    float scale = 1.f, shift = 0.f;
    const Seg& s = p.in;
    if (s.gn.stats) {
      const int g = tid / (32 / s.gn.groups);
      const double* st = s.gn.stats + ((int64_t)cloud * s.gn.groups + g) * kGnWords;
      const double mean = gn_stat_get(st) * s.gn.inv_count;
      double var = gn_stat_get(st + 2) * s.gn.inv_count - mean * mean;
      var = var > 0.0 ? var : 0.0;
      const double rstd = gn_rstd(var);
      const double scd = (double)s.gn.gamma[tid] * rstd;
      scale = (float)scd;
      shift = (float)((double)s.gn.beta[tid] - mean * scd);
    }
    s_sc[tid] = scale;
    s_sh[tid] = shift;
  }
  __syncthreads();

  // weight fragments of the four layers (zero past the layer's columns) and their biases
  typename Ops::template W<32> w1[4], w4[NT4];
  typename Ops::template W<64> w2[4], w3[2];
  float b2[4], b3[2], b4[NT4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    Ops::load(p, 0, 16 * t + fr, 64, fq, w1[t]);
    Ops::load(p, 1, 16 * t + fr, 64, fq, w2[t]);
    b2[t] = p.b2[16 * t + fr];
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    Ops::load(p, 2, 16 * t + fr, 32, fq, w3[t]);
    b3[t] = p.b3[16 * t + fr];
  }
#pragma unroll
  for (int t = 0; t < NT4; ++t) {
    Ops::load(p, 3, 16 * t + fr, p.ncls, fq, w4[t]);
    b4[t] = (16 * t + fr) < p.ncls ? p.b4[16 * t + fr] : 0.f;
  }
  float sc[8], sh[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { sc[j] = s_sc[8 * fq + j]; sh[j] = s_sh[8 * fq + j]; }
  const float slope = p.in.act ? 0.2f : 1.f;
  float* T = s_T[w];
  const float* X = p.in.x + cloud * p.in.cloud_stride;
  float* feat = p.feat_out ? p.feat_out + (int64_t)cloud * p.M * 64 : nullptr;
  float* logit = p.logits_out + (int64_t)cloud * p.M * p.ncls;

  // C-layout accumulators (col = lane & 15, row = 4 (lane >> 4) + reg) -> T[row][col]
  auto spill = [&](const auto& acc) {
    constexpr int NTL = sizeof(acc) / sizeof(acc[0]);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t = 0; t < NTL; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) T[(4 * fq + r) * LDT + 16 * t + fr] = acc[t][r];
    __builtin_amdgcn_wave_barrier();
  };
  auto zero = [&](auto& acc) {
#pragma unroll
    for (size_t t = 0; t < sizeof(acc) / sizeof(acc[0]); ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  };
  auto bias_act = [&](auto& acc, const auto& b) {
#pragma unroll
    for (size_t t = 0; t < sizeof(acc) / sizeof(acc[0]); ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) { const float v = acc[t][r] + b[t]; acc[t][r] = v < 0.f ? v * 0.2f : v; }
  };

  const int ntiles = (p.M + 15) >> 4;
  const int nwaves = gridDim.x * 4;
  float4 x0, x1, x0n, x1n;
  auto load_a0 = [&](int tile, float4& u, float4& v) {
    const int row = min(tile * 16 + fr, p.M - 1);        // clamped, not predicated (results of padded rows are dropped)
    const float* src = X + (int64_t)row * p.in.ld + 8 * fq;
    u = *reinterpret_cast<const float4*>(src);
    v = *reinterpret_cast<const float4*>(src + 4);
  };
  int tile = blockIdx.x * 4 + w;
  if (tile < ntiles) load_a0(tile, x0, x1);
  for (; tile < ntiles; tile += nwaves) {
    if (tile + nwaves < ntiles) load_a0(tile + nwaves, x0n, x1n);
    typename Ops::template A<32> a0;
    {
      float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float u = fmaf(v[j], sc[j], sh[j]);
        v[j] = fmaxf(u, slope * u);
      }
      Ops::pack(v, a0);
    }
    const int rbase = tile * 16 + 4 * fq;
    // ---- mlp_out: 32 -> 64 (no bias)
    f32x4 c1[4];
    zero(c1);
    Ops::mma(c1, a0, w1);
    if (feat) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (rbase + r < p.M) feat[(int64_t)(rbase + r) * 64 + 16 * t + fr] = c1[t][r];
    }
    spill(c1);
    typename Ops::template A<64> a1;
    Ops::read(T + fr * LDT, fq, a1);
    // ---- fc_label.0 (+ folded BN): 64 -> 64, LeakyReLU
    f32x4 c2[4];
    zero(c2);
    Ops::mma(c2, a1, w2);
    bias_act(c2, b2);
    spill(c2);
    typename Ops::template A<64> a2;
    Ops::read(T + fr * LDT, fq, a2);
    // ---- fc_label.3 (+ folded BN): 64 -> 32, LeakyReLU
    f32x4 c3[2];
    zero(c3);
    Ops::mma(c3, a2, w3);
    bias_act(c3, b3);
    spill(c3);
    typename Ops::template A<32> a3;
    Ops::read(T + fr * LDT, fq, a3);
    // ---- fc_label.6: 32 -> ncls
    f32x4 c4[NT4];
    zero(c4);
    Ops::mma(c4, a3, w4);
#pragma unroll
    for (int t = 0; t < NT4; ++t) {
      const int col = 16 * t + fr;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (rbase + r < p.M && col < p.ncls) logit[(int64_t)(rbase + r) * p.ncls + col] = c4[t][r] + b4[t];
    }
    x0 = x0n; x1 = x1n;
  }
}

}  // namespace headm
}  // namespace dsir
