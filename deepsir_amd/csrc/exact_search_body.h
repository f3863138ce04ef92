// Device body of the exact-fp32 descriptor search: the one tile walk and the one distance expression behind the arg-min
// (nn_match.hip, also the fallback of nn_screen.hip / nn_prune.hip) and the top-k lists (nn_topk.hip) - same instructions on the same
// operands, same bits.  What a kernel does with a distance (running minimum, sorted list) is its own; everything before is here.
//
// THE RULE of the exact distance of src row j to ref column c (reference network/matchnet.py:96-113 square_distance_V2):
//   dot        a_j.b_c from the v_mfma_f32_16x16x4_f32 chain: 16 MFMAs from a ZERO accumulator, k-step s = 0..15 ascending, inside a
//              step the matrix core's k order - a k-ordered fmaf chain over channels 0..63 ascending (screen_bound.h::exact_dist is
//              the same chain in scalar code).
//   distance   d = fl(fl(-2 dot + |a_j|^2) + |b_c|^2): two roundings (-2 dot is exact, so the fused form rounds exactly like the
//              reference's multiply and add).  dist_from_dot() is its one spelling.  The norms are launch_sqnorm's (sqnorm_row16).
//   ties       a lane meets its columns in ascending order and every consumer compares strictly (d < held), so an equal distance
//              stays behind the lower column; across lanes and workgroups the packed key order_bits(d) << 32 | c decides.
//   non-finite nothing is filtered here: a NaN or +inf distance reaches visit() and fails the consumer's `d < held` against a
//              held value that starts at +inf, so it never enters a result.  Columns at c_end and beyond are never visited.
#pragma once
#include "device_utils.h"

namespace dsir {

constexpr int BC = 64;        // ref columns per LDS tile
constexpr int LDB = 64 + 2;   // padded tile row (floats): fragment reads are conflict free

__device__ __forceinline__ float dist_from_dot(float dot, float san, float sbn) { return __fadd_rn(__fmaf_rn(dot, -2.f, san), sbn); }

// One wave's share of a workgroup (4 waves, all 256 threads call it: the body has barriers) streaming ref columns [c_begin, c_end)
// of one pair past RT row tiles of 16 src rows.  Bs / sbs: the calling kernel's __shared__ double-buffered ref tile and its norms.
// Ap / Bp: the pair's descriptors [.][64]; sa_pair / sb_pair: their squared norms.  The wave's virtual rows are row0 .. row0 + 16 RT;
// rowof(v) is the src row behind virtual row v, or -1 for none (its fragments are zero, its distances are the caller's to drop).
// visit(rt, r, d, col) is called for every live column col and the lane's 4 rows r of row tile rt (virtual row
// row0 + 16 rt + 4 (lane >> 4) + r), rt and r compile-time constants after unrolling; col = c0 + 16 t + (lane & 15) ascends per lane.
template <int RT, typename RowOf, typename Visit>
__device__ __forceinline__ void exact_search_stream(float (*Bs)[BC * LDB], float (*sbs)[BC], const float* __restrict__ Ap,
                                                    const float* __restrict__ Bp, const float* __restrict__ sa_pair,
                                                    const float* __restrict__ sb_pair, const int row0, RowOf rowof, const int c_begin,
                                                    const int c_end, Visit visit) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int fr = lane & 15, fq = lane >> 4;
  // A fragments: lane holds A[row = fr][k = 4 s + fq], resident for the whole column range
  float af[RT][16];
  float san[RT][4];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int row = rowof(row0 + rt * 16 + fr);
#pragma unroll
    for (int s = 0; s < 16; ++s) af[rt][s] = row >= 0 ? Ap[(int64_t)row * 64 + 4 * s + fq] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = rowof(row0 + rt * 16 + 4 * fq + r);
      san[rt][r] = rr >= 0 ? sa_pair[rr] : 0.f;
    }
  }
  // Pipeline: the next 64-column ref tile is fetched into registers while the MFMAs of the current
  // tile run, then written to the other LDS buffer; one barrier per tile.
  float4 pre[4];
  float pre_sb = 0.f;
  auto gload = [&](int c0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int f = tid + 256 * i;
      const int r = f >> 4, c4 = f & 15;
      pre[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c0 + r < c_end) pre[i] = *reinterpret_cast<const float4*>(Bp + (int64_t)(c0 + r) * 64 + c4 * 4);
    }
    if (tid < BC) pre_sb = (c0 + tid < c_end) ? sb_pair[c0 + tid] : 0.f;
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int f = tid + 256 * i;
      const int r = f >> 4, c4 = f & 15;
      float2* dst = reinterpret_cast<float2*>(&Bs[buf][r * LDB + c4 * 4]);
      dst[0] = make_float2(pre[i].x, pre[i].y);
      dst[1] = make_float2(pre[i].z, pre[i].w);
    }
    if (tid < BC) sbs[buf][tid] = pre_sb;
  };
  gload(c_begin);
  lstore(0);
  __syncthreads();
  int buf = 0;
  for (int c0 = c_begin; c0 < c_end; c0 += BC) {
    const bool has_next = c0 + BC < c_end;
    if (has_next) gload(c0 + BC);
    const float* Bt = Bs[buf];
#pragma unroll
    for (int t = 0; t < BC / 16; ++t) {
      f32x4 acc[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const float b = Bt[(16 * t + fr) * LDB + 4 * s + fq];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[rt][s], b, acc[rt], 0, 0, 0);
      }
      const int col = c0 + 16 * t + fr;
      const float sbv = sbs[buf][16 * t + fr];
      if (col < c_end) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) visit(rt, r, dist_from_dot(acc[rt][r], san[rt][r], sbv), col);
      }
    }
    if (has_next) lstore(buf ^ 1);   // last readers of that buffer finished before the previous barrier
    __syncthreads();
    buf ^= 1;
  }
}

}  // namespace dsir
