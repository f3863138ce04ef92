// mlp_feat of Network.aggregation (reference network/model.py:160-162, :218) in one launch:
//   F = W3 lrelu(W2 lrelu(W1 x + b1) + b2) + b3        64 -> 64 -> 128 -> 64, eval-BatchNorm folded, LeakyReLU(0.2)
// Three point-wise layers with nothing between them that crosses a row: the 64- and 128-wide intermediates stay on the CU
// (the three launches this replaces wrote them to memory and read them back: 1.3 GB per 128 x 5000 points against the
// 328 MB the chain itself needs).
//
// Every output element is the chain of operations the three launches give it (run_mlp_feat, schedule.hip), bit for bit:
//   layers 1, 2   pw_stream.hip, KQ = 16: exact-fp32 v_mfma_f32_16x16x4_f32, lane (r, q) holds channels [16 q, 16 q + 16) of
//                 row r, k-step s contracts channels {16 q + s}; epilogue v = acc + b, v < 0 ? 0.2 v : v
//   layer 3       pw_tile.hip.  SPLIT: the fp16 operand split of split_f16.h, one mma3 per 32-channel chunk, chunks ascending,
//                 lane (r, q) holds channels 32 s + 8 q .. + 7.  Otherwise (dsir_enable_agg_split(0), DSIR_AGG_F32,
//                 DSIR_TILE_F32) exact fp32 in that kernel's k order: step S contracts channels {4 S + q}.  Epilogue v = acc + b.
// The producers' input transform of those kernels (fmaf(x, 1, 0), max(v, 1 v): no GroupNorm, no activation pending) is the
// identity up to the sign of a zero, which no sum that starts from +0 can see.
//
// Workgroup = 8 waves, persistent: one per CU (LDS).  W2 (fp32) and W3 (fp16 high / low parts, or fp32) are staged in LDS
// once per workgroup in the order the fragments are read; W1 stays in registers.  A wave owns 16-row tiles of the flattened
// (cloud, tile) range - no cross-workgroup reduction, so any assignment gives the same bits - and walks the three layers;
// between layers the C-layout accumulators go through a wave-private LDS tile to become the next layer's A fragments.
// LDS layouts are blocked by the lane quarter q (the 16-lane groups of ds_read_b128 mix two quarters: a quarter's block
// starts at a multiple of the bank row, rows inside it are an odd number of 16-byte slots apart).
#include <hip/hip_fp16.h>

#include "kernels.h"
#include "device_utils.h"
#include "split_f16.h"

namespace dsir {

namespace {

constexpr int kWaves = 8;
constexpr int kDefaultCUs = 256;   // MI355X; used only where the device does not say
constexpr int W2_LD = 20;          // s_w2 [q][128 columns][16 + 4]: channels 16 q .. of a column
constexpr int T1_LD = 20;          // layer 1 -> 2 tile [q][16 rows][16 + 4]
constexpr int T2_LD = 36;          // layer 2 -> 3 tile [q][16 rows][4 chunks x 8 + 4]: channels 32 s + 8 q .. at 8 s
constexpr int W3_LD = 128 + 4;     // exact-fp32 layer 3: s_w3 [64 columns][128 + 4]
constexpr int T_WORDS = 4 * 16 * T2_LD;

template <bool SPLIT>
__global__ __launch_bounds__(64 * kWaves) void feat_chain_kernel(const FeatChainArgs p) {
  __shared__ __attribute__((aligned(16))) float s_w2[4 * 128 * W2_LD];
  // SPLIT: 16-byte slots [high | low][chunk s][q][64 columns] = 8 halfs of channels 32 s + 8 q ..; else fp32 rows
  __shared__ __attribute__((aligned(16))) float s_w3[SPLIT ? 2 * 16 * 64 * 4 : 64 * W3_LD];
  __shared__ __attribute__((aligned(16))) float s_T[kWaves][T_WORDS];

  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;

  // ---- W1 fragments and the biases: registers
  float w1[4][16], b1[4], b2[8], b3[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 v = *reinterpret_cast<const float4*>(p.W1 + (16 * t + fr) * 64 + 16 * fq + 4 * i);
      w1[t][4 * i] = v.x; w1[t][4 * i + 1] = v.y; w1[t][4 * i + 2] = v.z; w1[t][4 * i + 3] = v.w;
    }
    b1[t] = p.b1 ? p.b1[16 * t + fr] : 0.f;
    b3[t] = p.b3 ? p.b3[16 * t + fr] : 0.f;
  }
#pragma unroll
  for (int t = 0; t < 8; ++t) b2[t] = p.b2 ? p.b2[16 * t + fr] : 0.f;

  // ---- W2, W3 -> LDS
  for (int i = tid; i < 128 * 16; i += 64 * kWaves) {
    const int col = i >> 4, q4 = i & 15;       // channels 4 q4 .. of column col: quarter q4 / 4, offset 4 (q4 % 4)
    *reinterpret_cast<float4*>(&s_w2[((q4 >> 2) * 128 + col) * W2_LD + 4 * (q4 & 3)]) = *reinterpret_cast<const float4*>(p.W2 + col * 64 + 4 * q4);
  }
  if constexpr (SPLIT) {
    const uint4* gh = reinterpret_cast<const uint4*>(p.W3h);
    const uint4* gl = reinterpret_cast<const uint4*>(p.W3l);
    uint4* d = reinterpret_cast<uint4*>(s_w3);
    for (int i = tid; i < 64 * 16; i += 64 * kWaves) {
      const int col = i >> 4, u = i & 15;      // halfs 8 u .. of column col: chunk u / 4, quarter u % 4
      d[u * 64 + col] = gh[i];
      d[(16 + u) * 64 + col] = gl[i];
    }
  } else {
    for (int i = tid; i < 64 * 32; i += 64 * kWaves) {
      const int col = i >> 5, c4 = i & 31;
      *reinterpret_cast<float4*>(&s_w3[col * W3_LD + 4 * c4]) = *reinterpret_cast<const float4*>(p.W3 + col * 128 + 4 * c4);
    }
  }
  __syncthreads();

  float* T = s_T[w];
  const int ntiles = (p.n + 15) >> 4;
  const int total = p.clouds * ntiles, stride = gridDim.x * kWaves;

  float4 x[4], xn[4];
  auto load_x = [&](int g, float4 (&v)[4]) {
    const int cloud = g / ntiles, tile = g - cloud * ntiles;
    const int row = min(tile * 16 + fr, p.n - 1);          // clamped, not predicated (results of padded rows are dropped)
    const float* src = p.X + ((int64_t)cloud * p.n + row) * 64 + 16 * fq;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const float4*>(src + 4 * i);
  };
  int g = blockIdx.x * kWaves + w;
  if (g < total) load_x(g, x);
  for (; g < total; g += stride) {
    if (g + stride < total) load_x(g + stride, xn);
    const int cloud = g / ntiles, tile = g - cloud * ntiles;

    // ---- mlp_feat.0 (+ folded BN): 64 -> 64, LeakyReLU
    f32x4 c1[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) c1[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float a[4] = {x[i].x, x[i].y, x[i].z, x[i].w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) c1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], w1[t][4 * i + j], c1[t], 0, 0, 0);
    }
    // C layout (col = lane & 15, row = 4 (lane >> 4) + reg) -> T[quarter t of the next layer][row][col & 15]
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = c1[t][r] + b1[t];
        if (v < 0.f) v *= 0.2f;
        T[(t * 16 + 4 * fq + r) * T1_LD + fr] = v;
      }
    __builtin_amdgcn_wave_barrier();
    float4 a1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a1[i] = *reinterpret_cast<const float4*>(&T[(fq * 16 + fr) * T1_LD + 4 * i]);

    // ---- mlp_feat.3 (+ folded BN): 64 -> 128, LeakyReLU
    f32x4 c2[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) c2[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float4 b[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) b[t] = *reinterpret_cast<const float4*>(&s_w2[(fq * 128 + 16 * t + fr) * W2_LD + 4 * i]);
      const float a[4] = {a1[i].x, a1[i].y, a1[i].z, a1[i].w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const float bj = j == 0 ? b[t].x : (j == 1 ? b[t].y : (j == 2 ? b[t].z : b[t].w));
          c2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], bj, c2[t], 0, 0, 0);
        }
    }
    // -> T[quarter (col % 32) / 8][row][8 (col / 32) + col % 8]
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = c2[t][r] + b2[t];
        if (v < 0.f) v *= 0.2f;
        T[((2 * (t & 1) + (fr >> 3)) * 16 + 4 * fq + r) * T2_LD + 8 * (t >> 1) + (fr & 7)] = v;
      }
    __builtin_amdgcn_wave_barrier();

    // ---- mlp_feat.6: 128 -> 64
    f32x4 c3[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) c3[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (SPLIT) {
      h8 ah[4], al[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float4* q = reinterpret_cast<const float4*>(&T[(fq * 16 + fr) * T2_LD + 8 * s]);
        split8(q[0], q[1], ah[s], al[s]);
      }
      const h8* wh = reinterpret_cast<const h8*>(s_w3);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s)
          mma3(c3[t], ah[s], al[s], wh[(4 * s + fq) * 64 + 16 * t + fr], wh[(16 + 4 * s + fq) * 64 + 16 * t + fr]);
    } else {
#pragma unroll
      for (int S = 0; S < 32; ++S) {
        // channel 4 S + q: chunk S / 8, quarter (S % 8) / 2, offset 4 (S % 2) + q
        const float a = T[(((S & 7) >> 1) * 16 + fr) * T2_LD + 8 * (S >> 3) + 4 * (S & 1) + fq];
#pragma unroll
        for (int t = 0; t < 4; ++t)
          c3[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, s_w3[(16 * t + fr) * W3_LD + 4 * S + fq], c3[t], 0, 0, 0);
      }
    }
    float* Y = cloud < p.split_cloud ? p.out0 + (int64_t)cloud * p.n * 64 : p.out1 + (int64_t)(cloud - p.split_cloud) * p.n * 64;
    const int rbase = tile * 16 + 4 * fq;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (rbase + r < p.n) Y[(int64_t)(rbase + r) * 64 + 16 * t + fr] = c3[t][r] + b3[t];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = xn[i];
  }
}

}  // namespace

long long feat_chain_blocks(int clouds, int n) { return ((long long)clouds * ((n + 15) / 16) + kWaves - 1) / kWaves; }

bool launch_feat_chain(const FeatChainArgs& a, hipStream_t st) {
  if (a.n <= 0 || a.clouds <= 0) return true;
  // the three launches' arithmetic is reproduced for the default dispatch of launch_pw_gemm only: pw_stream.hip (vector loader:
  // aligned rows) for the two 64-channel layers, pw_tile.hip for the last
  static const bool other = tuning_flag("DSIR_NO_STREAM") || tuning_flag("DSIR_NO_TILE") || tuning_int("DSIR_TILE_MIN_COUT", 32) > 64;
  if (other) return false;
  if (!a.X || !a.W1 || !a.W2 || !a.W3 || !a.out0 || (a.split_cloud < a.clouds && !a.out1) || a.split_cloud < 0) return false;
  if ((reinterpret_cast<uintptr_t>(a.X) | reinterpret_cast<uintptr_t>(a.W1) | reinterpret_cast<uintptr_t>(a.W2) |
       reinterpret_cast<uintptr_t>(a.W3)) % 16)
    return false;
  static const bool tile_f32 = tuning_flag("DSIR_TILE_F32");   // pw_tile.hip's own switch: its exact-fp32 kernels although split weights exist
  const bool split = a.W3h && a.W3l && !tile_f32;
  if (split && (reinterpret_cast<uintptr_t>(a.W3h) | reinterpret_cast<uintptr_t>(a.W3l)) % 16) return false;
  const int64_t total = (int64_t)a.clouds * ((a.n + 15) / 16);
  if (total > 0x7fffffffll - 64 * 1024) return false;
  // one workgroup per CU holds the weights in LDS (the device's CU count, asked once); a small launch (the captured one-pair
  // registration) gets one tile per wave
  static const int cus = [] {
    int dev = 0, n = 0;
    const bool ok = hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess;
    return ok && n > 0 ? n : kDefaultCUs;
  }();
  const int64_t want = feat_chain_blocks(a.clouds, a.n);
  const int64_t most = a.max_blocks > 0 && a.max_blocks < cus ? a.max_blocks : cus;
  const int blocks = (int)(want < most ? want : most);
  if (split) hipLaunchKernelGGL(feat_chain_kernel<true>, dim3(blocks), dim3(64 * kWaves), 0, st, a);
  else hipLaunchKernelGGL(feat_chain_kernel<false>, dim3(blocks), dim3(64 * kWaves), 0, st, a);
  return true;
}

}  // namespace dsir
