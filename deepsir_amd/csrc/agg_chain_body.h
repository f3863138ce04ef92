// The walk of the fused aggregation chain (agg_chain.hip), once for both arithmetics.
//
// A block owns 64 RT points (4 waves x RT row tiles of 16) and walks the whole chain:
//   * activations never leave the CU: a layer's accumulators (C layout) are transposed through a wave-private LDS tile
//     into the A fragments (registers) of the next layer; the 256-wide layer is produced 64 columns at a time and
//     consumed immediately as one K chunk of the following 256 -> 64 layer;
//   * weights stream through a double-buffered LDS tile of 64 columns x 64 channels shared by the four waves: 16 chunks
//     per block, fetched Ops::LOOKAHEAD chunks before they are staged.
// Ops is the arithmetic: the LDS tile of a weight chunk and its fetch / stage, the A fragment and its read-back from the
// transposition tile, the contraction of one chunk.  Nothing here depends on which one it is.
#pragma once
#include "kernels.h"
#include "device_utils.h"

namespace dsir {
namespace aggc {

// ---- the 16 weight chunks, in the order the walk consumes them
struct Chunk { int layer, ld, col0, k0, nk; };   // layer 0 .. 4 = W2 .. W6; leading dimension; first column, first channel, channels
__device__ __forceinline__ Chunk chunk_of(int i) {
  if (i == 0) return {0, 32, 0, 0, 32};                        // layer 2
  if (i <= 2) return {1, 64, 64 * (i - 1), 0, 64};             // layer 3: two column halves
  if (i == 15) return {4, 64, 0, 0, 64};                       // mlp_proj
  const int j = (i - 3) / 3, u = (i - 3) % 3;                  // column chunk j: layer 4's two K chunks, then K chunk j of layer 5
  if (u < 2) return {2, 128, 64 * j, 64 * u, 64};
  return {3, 256, 0, 64 * j, 64};
}
constexpr int kChunks = 16;

// where a fragment sits in the chain: layer 2's 32 input channels, the 64-channel chunks in between, mlp_proj's input
enum Stage { L2, MID, PROJ };

template <class Ops, int RT>
__device__ __forceinline__ void agg_chain_body(const AggArgs& p) {
  constexpr int LDT = Ops::LDT;
  using AFrag = typename Ops::AFrag;
  __shared__ typename Ops::WTile Ws;
  __shared__ float Ts[4][RT][16 * LDT];

  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int cloud = blockIdx.y;
  const int r0 = blockIdx.x * (64 * RT) + 16 * RT * w;      // first row of this wave

  Ops ops(p, Ws, tid, fr, fq);
  int buf = 0, ci = 0;
  // finish chunk ci: stage chunk ci + 1 (in registers) into the other buffer, barrier, flip, fetch the chunk LOOKAHEAD ahead
  auto next_chunk = [&]() {
    if (ci + 1 < kChunks) ops.lstore(buf ^ 1, ci + 1);
    __syncthreads();
    buf ^= 1;
    ++ci;
    if (ci + Ops::LOOKAHEAD < kChunks) ops.gload(ci + Ops::LOOKAHEAD);
  };

  ops.gload(0);
  ops.lstore(0, 0);
#pragma unroll
  for (int i = 1; i <= Ops::LOOKAHEAD; ++i) ops.gload(i);

  // ---- layer 1: [xyz ; score] (4) -> 32 in exact fp32, weights in registers (one MFMA k-step, k = q)
  {
    float w1[2], b1[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) { w1[t] = p.W1[(16 * t + fr) * 4 + fq]; b1[t] = p.b1[16 * t + fr]; }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int row = min(r0 + 16 * rt + fr, p.n - 1);
      const float a = Ops::input(fq < 3 ? p.xyz[cloud * p.xyz_cs + (int64_t)row * 3 + fq] : p.score[(int64_t)cloud * p.n + row]);
      float* T = Ts[w][rt];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4 c = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w1[t], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = c[r] + b1[t];
          v = v < 0.f ? v * 0.2f : v;
          T[(4 * fq + r) * LDT + 16 * t + fr] = v;
        }
      }
    }
  }
  __syncthreads();   // chunk 0 staged (and T written)

  // C-layout accumulators (+ bias, LeakyReLU) -> LDS tile, from which the next layer's A fragments are read back
  auto spill = [&](float* T, const f32x4 (&acc)[4], const float* bias, bool act) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float b = bias[16 * t + fr];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[t][r] + b;
        if (act) v = v < 0.f ? v * 0.2f : v;
        T[(4 * fq + r) * LDT + 16 * t + fr] = v;
      }
    }
    __builtin_amdgcn_wave_barrier();
  };
  auto zero = [&](f32x4 (&acc)[RT][4]) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  };

  // ---- layer 2: 32 -> 64 (chunk 0)
  AFrag a3[RT];
  {
    AFrag a2[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) ops.template read<L2>(Ts[w][rt], a2[rt]);
    f32x4 acc[RT][4];
    zero(acc);
    ops.template mma<L2, RT>(acc, a2, buf);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      spill(Ts[w][rt], acc[rt], p.b2, true);
      ops.template read<MID>(Ts[w][rt], a3[rt]);
    }
    next_chunk();
  }

  // ---- layer 3: 64 -> 128 (chunks 1, 2 = column halves); its output is layer 4's A operand
  AFrag a4[2][RT];   // [k half][row tile]
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    f32x4 acc[RT][4];
    zero(acc);
    ops.template mma<MID, RT>(acc, a3, buf);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      spill(Ts[w][rt], acc[rt], p.b3 + 64 * c, true);
      ops.template read<MID>(Ts[w][rt], a4[c][rt]);
    }
    next_chunk();
  }

  // ---- layers 4 + 5 interleaved: column chunk j of 128 -> 256 (two K chunks), activated, becomes K chunk j of 256 -> 64
  f32x4 acc5[RT][4];
  zero(acc5);
  float fpre[RT][4][4];      // the mlp_feat rows the epilogue adds (model.py:226): fetched during the last column chunk, not in front of their use
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f32x4 acc[RT][4];
    zero(acc);
    if (j == 3) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = min(r0 + 16 * rt + 4 * fq + r, p.n - 1);
          const float* f = p.F + ((int64_t)cloud * p.n + row) * 64 + fr;
#pragma unroll
          for (int t = 0; t < 4; ++t) fpre[rt][r][t] = f[16 * t];
        }
    }
    ops.template mma<MID, RT>(acc, a4[0], buf);
    next_chunk();
    ops.template mma<MID, RT>(acc, a4[1], buf);
    AFrag a5[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      spill(Ts[w][rt], acc[rt], p.b4 + 64 * j, true);
      ops.template read<MID>(Ts[w][rt], a5[rt]);
    }
    next_chunk();
    ops.template mma<MID, RT>(acc5, a5, buf);
    next_chunk();
  }

  // ---- layer 5 epilogue (bias, + F) -> layer 6 (mlp_proj) -> L2 normalise -> store
  {
    AFrag a6[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      float* T = Ts[w][rt];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int t = 0; t < 4; ++t) T[(4 * fq + r) * LDT + 16 * t + fr] = (acc5[rt][t][r] + p.b5[16 * t + fr]) + fpre[rt][r][t];
      }
      __builtin_amdgcn_wave_barrier();
      ops.template read<PROJ>(T, a6[rt]);
    }
    f32x4 acc[RT][4];
    zero(acc);
    ops.template mma<PROJ, RT>(acc, a6, buf);
    float bv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) bv[t] = p.b6[16 * t + fr];
    float* Y = p.desc + (int64_t)cloud * p.n * 64;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      float ss[4] = {0.f, 0.f, 0.f, 0.f};
      float v[4][4];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[t][r] = acc[rt][t][r] + bv[t];
          ss[r] += v[t][r] * v[t][r];
        }
      const bool extras = Ops::EXTRAS && (p.sq || p.hi || p.packed_init);      // block-uniform
      float* T = Ts[w][rt];
      if (extras) __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ss[r] += __shfl_xor(ss[r], 1); ss[r] += __shfl_xor(ss[r], 2);
        ss[r] += __shfl_xor(ss[r], 4); ss[r] += __shfl_xor(ss[r], 8);
        const float den = fmaxf(__fsqrt_rn(ss[r]), 1e-12f);
        const int row = r0 + 16 * rt + 4 * fq + r;
        if (extras) {
#pragma unroll
          for (int t = 0; t < 4; ++t) T[(4 * fq + r) * LDT + 16 * t + fr] = v[t][r] / den;
        } else if (row < p.n) {
#pragma unroll
          for (int t = 0; t < 4; ++t) Y[(int64_t)row * 64 + 16 * t + fr] = v[t][r] / den;
        }
      }
      if constexpr (Ops::EXTRAS) {
        if (extras) {
          // The descriptors go back through the wave's LDS tile into the row layout the search's preparation kernels read them in (16
          // lanes per row, four consecutive channels each): |desc|^2 in THEIR summation order (sqnorm_row16: the value enters the
          // distance every arg-min is decided on), the screening's fp16 operand pair by THEIR split - same bits, one pass less over
          // the descriptors (and 16-byte descriptor stores instead of 4-byte ones).
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int lr = 4 * q + fq, row = r0 + 16 * rt + lr;           // lane group fq takes row 4 q + fq, lane fr its channels 4 fr ..
            const float4 d4 = *reinterpret_cast<const float4*>(T + lr * LDT + 4 * fr);
            const float s2 = sqnorm_row16(d4);
            if (row < p.n) {
              const int64_t gr = (int64_t)cloud * p.n + row;
              *reinterpret_cast<float4*>(Y + (int64_t)row * 64 + 4 * fr) = d4;
              if (p.hi) {
                dsir_h4 hh, ll;
                screen_split4(d4, hh, ll, nullptr);
                *reinterpret_cast<dsir_h4*>(reinterpret_cast<_Float16*>(p.hi) + gr * 64 + 4 * fr) = hh;
                *reinterpret_cast<dsir_h4*>(reinterpret_cast<_Float16*>(p.lo) + gr * 64 + 4 * fr) = ll;
              }
              if (fr == 0) {
                if (p.sq) p.sq[gr] = s2;
                if (p.packed_init) p.packed_init[gr] = ~0ull;
              }
            }
          }
        }
      }
    }
  }
}

}  // namespace aggc
}  // namespace dsir
