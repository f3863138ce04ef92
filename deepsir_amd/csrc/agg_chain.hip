// The per-iteration half of Network.aggregation (reference network/model.py:223-233) in ONE launch:
//   g    = mlp_att([xyz ; score])        4 -> 32 -> 64 -> 128 -> 256 -> 64   (Conv1d + eval-BatchNorm folded + LeakyReLU 0.2,
//                                                                             last layer bare; RandLANet.py:34-55)
//   desc = normalize(mlp_proj(F + g))    64 -> 64, L2 over channels           (F = mlp_feat(feat0): loop invariant, hoisted)
// Unfused these are six launches whose 32..256-wide intermediates make a round trip through HBM (4.3 kB per point per
// iteration) and whose K loops are only 1..8 chunks long, so prologue / epilogue dominate.  The walk that keeps them on the
// CU is agg_chain_body.h; this file is its two arithmetics and the launch rule.
//
// SplitOps (default): the five wide layers on the fp16 matrix pipe at fp32 accuracy, by the operand split of split_f16.h.
//   The chain is the one MFMA-bound stage of the path besides the descriptor search: 127 kFLOP per point, 77 % of it in
//   128 -> 256 -> 64; the fp32 MFMA keeps its pipe 75 % busy, three fp16 MFMAs per product take 3/16 of that time.
//   Activations are split when they are read back from the transposition tile, weights were split at load and stream
//   through {high, low} tiles.  Descriptors differ from the fp32 form's by ~1e-7 (asserted <= 2e-6 by
//   tests/test_gpu_parity.py::test_agg_chain_split_matches_fp32_chain; the reference's own thread-count noise on these
//   descriptors is of the same size).  Domain: |activation| <= 65504 (fp16 range); larger values (or non-finite
//   ones) make that point's descriptor non-finite, which the pose solve reports as the pair's `invalid` bit 0 - the same
//   outcome as a non-finite input point.
// F32Ops (DSIR_AGG_F32=1 / dsir_enable_agg_split(0)): exact-fp32 MFMA (v_mfma_f32_16x16x4_f32), every layer in the SAME k
//   order as the kernel it replaces (pw_stream.hip for 4->32, 32->64 and 64->64, pw_tile.hip for the wide ones), so
//   descriptors are bit-identical to the unfused path (DSIR_NO_AGG=1; tests/test_gpu_chain_forms.py).  The reference of the
//   split form.
#include <hip/hip_fp16.h>

#include "agg_chain_body.h"
#include "split_f16.h"

namespace dsir {

namespace {

using aggc::Chunk;
using aggc::chunk_of;
using aggc::Stage;

struct F32Ops {
  static constexpr int LDW = 66;   // weight tile row (floats): fragment reads (row r, k = 4 s + q) hit banks 2 r + q
  static constexpr int LDT = 66;   // transposition tile row
  static constexpr int LOOKAHEAD = 1;
  static constexpr bool EXTRAS = false;
  struct WTile { alignas(16) float w[2][64 * LDW]; };
  struct AFrag { float v[16]; };
  // lane (r, q) holds, as k-step s of its fragment, channel KQ q + KS s: the k order of pw_stream<8,...> for layer 2, the natural
  // order (pw_tile) in the middle, the k order of pw_stream<16,...> for mlp_proj
  template <Stage ST> static constexpr int steps() { return ST == aggc::L2 ? 8 : 16; }
  template <Stage ST> static constexpr int kq() { return ST == aggc::L2 ? 8 : ST == aggc::MID ? 1 : 16; }
  template <Stage ST> static constexpr int ks() { return ST == aggc::MID ? 4 : 1; }

  const AggArgs& p;
  WTile& Ws;
  const int fr, fq, srow, sk;
  float4 rw[4];

  __device__ __forceinline__ F32Ops(const AggArgs& p_, WTile& Ws_, int tid, int fr_, int fq_)
      : p(p_), Ws(Ws_), fr(fr_), fq(fq_), srow(tid >> 4), sk((tid & 15) * 4) {}

  // the unfused first layer reads its input through the lazy-GroupNorm prologue with scale 1, shift 0
  static __device__ __forceinline__ float input(float x) { return fmaf(x, 1.f, 0.f); }

  __device__ __forceinline__ void gload(int i) {
    const Chunk c = chunk_of(i);
    const float* W = c.layer == 0 ? p.W2 : c.layer == 1 ? p.W3 : c.layer == 2 ? p.W4 : c.layer == 3 ? p.W5 : p.W6;
    const int k = min(sk, c.nk - 4);
#pragma unroll
    for (int u = 0; u < 4; ++u) rw[u] = *reinterpret_cast<const float4*>(W + (int64_t)(c.col0 + srow + 16 * u) * c.ld + c.k0 + k);
  }
  __device__ __forceinline__ void lstore(int buf, int i) {
    const int k = min(sk, chunk_of(i).nk - 4);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float2* d = reinterpret_cast<float2*>(&Ws.w[buf][(srow + 16 * u) * LDW + k]);
      d[0] = make_float2(rw[u].x, rw[u].y);
      d[1] = make_float2(rw[u].z, rw[u].w);
    }
  }
  template <Stage ST>
  __device__ __forceinline__ void read(const float* T, AFrag& a) const {
#pragma unroll
    for (int s = 0; s < steps<ST>(); ++s) a.v[s] = T[fr * LDT + kq<ST>() * fq + ks<ST>() * s];
  }
  template <Stage ST, int RT>
  __device__ __forceinline__ void mma(f32x4 (&acc)[RT][4], const AFrag (&a)[RT], int buf) const {
    const float* Wt = Ws.w[buf];
#pragma unroll
    for (int s = 0; s < steps<ST>(); ++s) {
      float b[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) b[t] = Wt[(16 * t + fr) * LDW + kq<ST>() * fq + ks<ST>() * s];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt].v[s], b[t], acc[rt][t], 0, 0, 0);
    }
  }
};

struct SplitOps {
  static constexpr int SRS = 80;   // halfs per LDS weight row: 64 + 16 pad (the fragment layout of nn_screen.hip's ref tile)
  static constexpr int LDT = 68;   // floats per row of the transposition tile: 16-byte aligned rows, conflict-free both ways
  // Two register sets: chunk i travels in set i & 1 and is fetched TWO chunks before it is staged.  A chunk's 48 - 96 MFMAs (0.3 - 0.6 us
  // with two workgroups per CU) hide a fraction of one L2 round trip: with one chunk of lookahead (round 3) the sixteen chunks of a
  // workgroup each waited for their weights (1.8 us per chunk, matrix pipe 36 % busy).
  static constexpr int LOOKAHEAD = 2;
  static constexpr bool EXTRAS = true;   // the epilogue can write the search's operands (AggArgs::sq, hi / lo, packed_init)
  struct WTile { alignas(16) _Float16 b[2][2][64 * SRS]; };     // [buffer][high | low]
  struct AFrag { h8 h[2], l[2]; };                              // one row tile x 64 channels: k-steps 0 / 1, high / low parts

  const AggArgs& p;
  WTile& Ws;
  const int tid, fr, fq;
  h8 rwh[LOOKAHEAD][2], rwl[LOOKAHEAD][2];

  __device__ __forceinline__ SplitOps(const AggArgs& p_, WTile& Ws_, int tid_, int fr_, int fq_) : p(p_), Ws(Ws_), tid(tid_), fr(fr_), fq(fq_) {}

  static __device__ __forceinline__ float input(float x) { return x; }

  __device__ __forceinline__ void gload(int i) {
    const Chunk c = chunk_of(i);
    const _Float16* Wh = reinterpret_cast<const _Float16*>(p.Wh[c.layer]);
    const _Float16* Wl = reinterpret_cast<const _Float16*>(p.Wl[c.layer]);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int f = tid + 256 * u;
      const int piece = min(f & 7, c.nk / 8 - 1);
      const int64_t o = (int64_t)(c.col0 + (f >> 3)) * c.ld + c.k0 + 8 * piece;
      rwh[i % LOOKAHEAD][u] = *reinterpret_cast<const h8*>(Wh + o);
      rwl[i % LOOKAHEAD][u] = *reinterpret_cast<const h8*>(Wl + o);
    }
  }
  __device__ __forceinline__ void lstore(int buf, int i) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int f = tid + 256 * u;
      *reinterpret_cast<h8*>(&Ws.b[buf][0][(f >> 3) * SRS + 8 * (f & 7)]) = rwh[i % LOOKAHEAD][u];
      *reinterpret_cast<h8*>(&Ws.b[buf][1][(f >> 3) * SRS + 8 * (f & 7)]) = rwl[i % LOOKAHEAD][u];
    }
  }
  // row fr, channels 8 fq .. and 32 + 8 fq .. (layer 2's 32 channels are one k-step)
  template <Stage ST>
  __device__ __forceinline__ void read(const float* T, AFrag& a) const {
    const float4* q = reinterpret_cast<const float4*>(T + fr * LDT + 8 * fq);
    split8(q[0], q[1], a.h[0], a.l[0]);
    if (ST != aggc::L2) split8(q[8], q[9], a.h[1], a.l[1]);
  }
  template <Stage ST, int RT>
  __device__ __forceinline__ void mma(f32x4 (&acc)[RT][4], const AFrag (&a)[RT], int buf) const {
    const _Float16* bh = &Ws.b[buf][0][fr * SRS + 8 * fq];
    const _Float16* bl = &Ws.b[buf][1][fr * SRS + 8 * fq];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int s = 0; s < (ST == aggc::L2 ? 1 : 2); ++s) {
        const h8 vh = *reinterpret_cast<const h8*>(bh + 16 * t * SRS + 32 * s);
        const h8 vl = *reinterpret_cast<const h8*>(bl + 16 * t * SRS + 32 * s);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) mma3(acc[rt][t], a[rt].h[s], a[rt].l[s], vh, vl);
      }
    }
  }
};

template <int RT>
__global__ __launch_bounds__(256, 2) void agg_chain_kernel(const AggArgs p) { aggc::agg_chain_body<F32Ops, RT>(p); }
template <int RT>
__global__ __launch_bounds__(256, 2) void agg_chain_h_kernel(const AggArgs p) { aggc::agg_chain_body<SplitOps, RT>(p); }

}  // namespace

bool launch_agg_chain(const AggArgs& a, bool split, hipStream_t st) {
  if (a.n <= 0 || a.clouds <= 0) return true;
  if (split)
    for (int l = 0; l < 5; ++l)
      if (!a.Wh[l] || !a.Wl[l]) return false;
  // every point's chain is independent of the blocking, so the rows per workgroup follow the launch size: 128 (two row
  // tiles per wave, weights re-read once per 128 points) when that already fills the chip, 64 for a few clouds in flight
  // (batch-1 latency: twice the workgroups, half the chain per wave) - same bits either way (tests/test_gpu_chain_forms.py)
  const bool big = (int64_t)((a.n + 127) / 128) * a.clouds >= 256;
  const int rows = big ? 128 : 64;
  const dim3 grid((a.n + rows - 1) / rows, a.clouds);
  auto k = split ? (big ? agg_chain_h_kernel<2> : agg_chain_h_kernel<1>) : (big ? agg_chain_kernel<2> : agg_chain_kernel<1>);
  hipLaunchKernelGGL(k, grid, dim3(256), 0, st, a);
  return true;
}

}  // namespace dsir
