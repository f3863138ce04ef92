// Point-pair-feature input layer of RandLA (args.use_ppf; reference network/RandLANet.py:110-137 feat_grouping, :324-332,
// network/matchnet.py:11-30 angle) and the normals it needs, from the level-0 neighbour lists.
//
// ---- The front end: feat_grouping -> mlp_pre (conv 1x1 10 -> 12 + bias, GroupNorm(4), LeakyReLU(0.2)) -> mean over the 16 neighbours.
// Two launches, both one lane per (point i, neighbour slot k) row; neither the ten-channel code nor the 12-channel activations are
// stored: the statistics pass commits the four groups' sum / sum of squares, the consumer pass rebuilds the row, normalises and
// averages.  Rebuilding costs ~120 FMA + 3 atan2f + 2 sqrtf per row against a 48-byte store and load.
//
// ARITHMETIC RULE (restated on the host in deepsir_amd/ppf.py).  All fp32, every operation rounded once, NO contraction except where
// an fma is written.  With j = neigh[i][k], p = point row, n = normal row:
//   d        = p_j - p_i                                     (three subtractions)
//   cross(a, b) = (a1 b2 - a2 b1,  a2 b0 - a0 b2,  a0 b1 - a1 b0)        (two products, one subtraction each)
//   dot(a, b)   = ((+0 + a0 b0) + a1 b1) + a2 b2        (from +0, as torch.sum: a zero vector times negative numbers gives -0 products, and
//                                                     atan2f(0, -0) is pi where the reference has 0)
//   norm(a)     = sqrtf((a0 a0 + a1 a1) + a2 a2)
//   angle(a, b) = atan2f(norm(cross(a, b)), dot(a, b))        (atan2f(0, 0) = 0: self neighbour, duplicate points, zero normals)
//   x[0..10) = [p_i(3), d(3), angle(n_i, d), angle(n_j, d), angle(n_i, n_j), norm(d)]
//   y[c]     = fma(W[c][9], x[9], ... fma(W[c][1], x[1], fma(W[c][0], x[0], b[c])))          (the ONE place contraction is allowed,
//              besides the GroupNorm scale / shift below: an fma chain in ascending input channel)
//   GroupNorm: group g = channels 3g .. 3g + 2 over all n x 16 rows of the cloud; sums of y and y^2 (the square an fp32 product)
//              in fp64; mean / variance / scale = gamma rstd / shift = beta - mean scale in fp64 as every other layer (pw_gemm.hip),
//              scale and shift rounded to fp32; z = fma(y, scale, shift); z < 0 -> 0.2 z
//   mean over k: a 16-lane butterfly (partners 1, 2, 4, 8), then x 1/16 (exact)
// The statistics meet across workgroups through the exact order-independent limbs of device_utils.h (no floating-point atomics on
// raw sums): a workgroup owns kPts consecutive points of one cloud - a function of n alone - sums its rows in fp64 in a fixed order
// (per lane: its four rows ascending; block_sum) and commits one contribution per statistic: ceil(n / kPts) contributions per
// (cloud, group), ppf_gn_contributions.  Same bytes on every run and for a cloud alone or inside a batch.
//
// ---- Normals (dsir_estimate_normals; open3d is unpinned: THE RULE IS OWNED HERE, restated in deepsir_amd/ppf.py).  One lane per point.
//   neighbourhood = the point's 16 level-0 neighbours in list order (self included, as the pyramid has it)
//   m   = (sum_k (double)q_k) / 16                            q_k: the fp32 coordinates, summed in fp64 in list order
//   C   = sum_k (q_k - m)(q_k - m)^T                          fp64, list order, upper triangle mirrored
//   (S, V) = svd3(C) (svd3.h; for a symmetric PSD matrix the SVD is the eigen-decomposition, S descending); normal = V[:, 2]
//   normalised in fp64, oriented, rounded to fp32 once
//   orientation: t = n . (v - p) in fp64 (v: the viewpoint, default origin; p: the point itself); t < 0: n = -n; t == 0: the sign
//   that makes the component of largest magnitude positive (ties: the lower axis)
//   degenerate (S[0] == 0: all neighbours coincide; or anything non-finite): normal (0, 0, 0), flag 1 - angle() then yields 0
//   dsir_estimate_normals_csr: the same arithmetic over the entries of a CSR row in row order (the divisor is the row's length); a row
//   of fewer than 3 entries is degenerate too
//
// ---- Training (dsir_t_ppf_fwd / dsir_t_ppf_bwd, include/dsir_train.h).  The rows are data in every pipeline, so the front end has
// four trainable tensors: W [12][10], b, gamma, beta.  The taped forward IS the two launches above (same bits); the consumer pass
// also writes, per cloud, the fp32 scale / shift it applied and {mean, rstd} per group (kPpfSaved floats).  Nothing of size n x 16 is
// kept: the backward rebuilds every row through ppf_row and z = fma(y, scale, shift) from the SAVED scale / shift, so the LeakyReLU
// branch is the forward's.  With g = dOut[i][c] / 16 * (z < 0 ? 0.2 : 1), yh = (y - mean) rstd, m = 3 n 16:
//   pass A, per cloud:   d beta_c = sum g,  d gamma_c = sum g yh;   per group  S1 = sum_c gamma_c d beta_c,  S2 = sum_c gamma_c d gamma_c
//   pass B:              dy = rstd (g gamma_c - S1 / m - yh S2 / m);   dW[c][q] += sum dy x[q],  db[c] += sum dy   (all clouds)
// Reductions: no floating-point atomics.  The partition is the forward's (a workgroup = 64 consecutive points of a cloud); a workgroup
// writes ONE fp64 partial per quantity; a second stage adds a cloud's partials in a fixed order (eight lanes, partials j, j + 8, ...
// ascending, then an xor tree) and the clouds in ascending order.  Same bytes on every run; a cloud's d gamma / d beta contribution is
// the same alone or inside a batch.  Within a workgroup pass A sums fp64 per lane and block_sum; pass B forms the 12 x 11 products
// [dy]^T [x | 1] of a wave's 64 rows on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation over the wave's 256 rows), the
// four waves' tiles meet in fp64 in wave order.
#include "device_utils.h"
#include "kernels.h"
#include "ppf_plan.h"
#include "svd3.h"
#include "dsir_train.h"

namespace dsir {

namespace {

constexpr int kPts = kPpfPts;      // points per workgroup (four rows per lane)

__device__ __forceinline__ float ppf_norm3(float x, float y, float z) {
  return __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));
}
__device__ __forceinline__ float ppf_angle(float ax, float ay, float az, float bx, float by, float bz) {
  const float cx = __fsub_rn(__fmul_rn(ay, bz), __fmul_rn(az, by));
  const float cy = __fsub_rn(__fmul_rn(az, bx), __fmul_rn(ax, bz));
  const float cz = __fsub_rn(__fmul_rn(ax, by), __fmul_rn(ay, bx));
  const float dp = __fadd_rn(__fadd_rn(__fadd_rn(0.f, __fmul_rn(ax, bx)), __fmul_rn(ay, by)), __fmul_rn(az, bz));
  return atan2f(ppf_norm3(cx, cy, cz), dp);
}

// the ten input channels x and the 12 raw conv outputs y of row (i, k); wb (LDS): W [12][10] then b [12].  The ONE statement of a row:
// the forward's two passes and the backward's two rebuild through it.
__device__ __forceinline__ void ppf_row(const PpfArgs& p, int cloud, int i, int k, const float* wb, float (&x)[10], float (&y)[12]) {
  int j = p.neigh[cloud * p.neigh_cs + (int64_t)i * kKnn + k];
  j = min(max(j, 0), p.n - 1);                      // a bad neighbour index can never leave the cloud
  const float* xyz = p.xyz + cloud * p.xyz_cs;
  const float* pi = xyz + (int64_t)i * p.xyz_ld;
  const float* pj = xyz + (int64_t)j * p.xyz_ld;
  int ri = i, rj = j;
  if (p.nrm_idx) { const int32_t* t = p.nrm_idx + cloud * p.nrm_idx_cs; ri = t[i]; rj = t[j]; }
  const float* ni = p.nrm + cloud * p.nrm_cs + (int64_t)ri * p.nrm_ld;
  const float* nj = p.nrm + cloud * p.nrm_cs + (int64_t)rj * p.nrm_ld;
  x[0] = pi[0]; x[1] = pi[1]; x[2] = pi[2];
  x[3] = __fsub_rn(pj[0], x[0]); x[4] = __fsub_rn(pj[1], x[1]); x[5] = __fsub_rn(pj[2], x[2]);
  const float a0 = ni[0], a1 = ni[1], a2 = ni[2], b0 = nj[0], b1 = nj[1], b2 = nj[2];
  x[6] = ppf_angle(a0, a1, a2, x[3], x[4], x[5]);
  x[7] = ppf_angle(b0, b1, b2, x[3], x[4], x[5]);
  x[8] = ppf_angle(a0, a1, a2, b0, b1, b2);
  x[9] = ppf_norm3(x[3], x[4], x[5]);
#pragma unroll
  for (int c = 0; c < 12; ++c) {
    float acc = wb[120 + c];
#pragma unroll
    for (int q = 0; q < 10; ++q) acc = fmaf(wb[c * 10 + q], x[q], acc);
    y[c] = acc;
  }
}

__device__ __forceinline__ void ppf_load_weights(const PpfArgs& p, float* wb) {
  if (threadIdx.x < 120) wb[threadIdx.x] = p.W[threadIdx.x];
  else if (threadIdx.x < 132) wb[threadIdx.x] = p.b[threadIdx.x - 120];
}

__global__ __launch_bounds__(256) void ppf_stats_kernel(const PpfArgs p, int bpc) {
  __shared__ float wb[132];
  __shared__ double sh[4 * 8 + 8];
  const int cloud = blockIdx.x / bpc, blk = blockIdx.x % bpc;
  ppf_load_weights(p, wb);
  __syncthreads();
  const int k = threadIdx.x & 15;
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // {sum, sum of squares} of groups 0 .. 3
  for (int it = 0; it < kPts / 16; ++it) {
    const int i = blk * kPts + it * 16 + (threadIdx.x >> 4);
    if (i >= p.n) continue;
    float x[10], y[12];
    ppf_row(p, cloud, i, k, wb, x, y);
#pragma unroll
    for (int c = 0; c < 12; ++c) {
      s[(c / 3) * 2] += (double)y[c];
      s[(c / 3) * 2 + 1] += (double)__fmul_rn(y[c], y[c]);
    }
  }
  block_sum<4, 8>(s, sh);
  if (threadIdx.x < 16) {                   // (group, statistic, limb): the slot layout of gn_block_commit
    const int g = threadIdx.x >> 2, stat = (threadIdx.x >> 1) & 1, limb = threadIdx.x & 1;
    unsafeAtomicAdd(p.stats + ((int64_t)cloud * 4 + g) * kGnWords + 2 * stat + limb, gn_stat_limb(sh[4 * 8 + g * 2 + stat], limb));
  }
}

__global__ __launch_bounds__(256) void ppf_apply_kernel(const PpfArgs p, int bpc) {
  __shared__ float wb[132];
  __shared__ float s_sc[12], s_sh[12];
  const int cloud = blockIdx.x / bpc, blk = blockIdx.x % bpc;
  ppf_load_weights(p, wb);
  if (threadIdx.x >= 192 && threadIdx.x < 204) {
    const int c = threadIdx.x - 192;
    const double inv_count = 1.0 / (3.0 * (double)p.n * (double)kKnn);
    const double* st = p.stats + ((int64_t)cloud * 4 + c / 3) * kGnWords;
    const double mean = gn_stat_get(st) * inv_count;
    double var = gn_stat_get(st + 2) * inv_count - mean * mean;
    var = var > 0.0 ? var : 0.0;
    const double sc = (double)p.gamma[c] * gn_rstd(var);
    s_sc[c] = (float)sc;
    s_sh[c] = (float)((double)p.beta[c] - mean * sc);
    if (p.saved && blk == 0) {              // the taped forward: what the backward rebuilds z and yh from
      float* sv = p.saved + (int64_t)cloud * kPpfSaved;
      sv[c] = s_sc[c];
      sv[12 + c] = s_sh[c];
      if (c % 3 == 0) { sv[24 + 2 * (c / 3)] = (float)mean; sv[25 + 2 * (c / 3)] = (float)gn_rstd(var); }
    }
  }
  __syncthreads();
  const int k = threadIdx.x & 15;
  float* out = p.out + cloud * p.out_cs;
  for (int it = 0; it < kPts / 16; ++it) {
    const int i = blk * kPts + it * 16 + (threadIdx.x >> 4);
    const bool live = i < p.n;              // uniform over the 16 lanes of a point; the butterfly runs in every lane
    float x[10], y[12];
    if (live) ppf_row(p, cloud, i, k, wb, x, y);
    float mine = 0.f;
#pragma unroll
    for (int c = 0; c < 12; ++c) {
      float z = live ? fmaf(y[c], s_sc[c], s_sh[c]) : 0.f;
      z = z < 0.f ? __fmul_rn(0.2f, z) : z;
      z = __fadd_rn(z, __shfl_xor(z, 1)); z = __fadd_rn(z, __shfl_xor(z, 2));
      z = __fadd_rn(z, __shfl_xor(z, 4)); z = __fadd_rn(z, __shfl_xor(z, 8));
      if (k == c) mine = z;
    }
    if (live && k < 12) out[(int64_t)i * 12 + k] = __fmul_rn(mine, 0.0625f);
  }
}

// ---- the backward (the rule: the header's training paragraph).  Grid and row ownership are those of the forward's two launches.
// g and yh of one rebuilt row; sv: the cloud's saved floats (LDS copy): scale[12], shift[12], {mean, rstd}[4]
__device__ __forceinline__ void ppf_row_grad(const float (&y)[12], const float* sv, const float* dout_i, float (&g)[12], float (&yh)[12]) {
#pragma unroll
  for (int c = 0; c < 12; ++c) {
    const float z = fmaf(y[c], sv[c], sv[12 + c]);                     // the forward's own z: its branch
    const float gd = __fmul_rn(dout_i[c], 0.0625f);
    g[c] = z < 0.f ? __fmul_rn(0.2f, gd) : gd;
    yh[c] = __fmul_rn(__fsub_rn(y[c], sv[24 + 2 * (c / 3)]), sv[25 + 2 * (c / 3)]);
  }
}

// pass A: partial[cloud][blk][24] = this workgroup's {sum g [12], sum g yh [12]}
__global__ __launch_bounds__(256) void ppf_bwd_a_kernel(const PpfArgs p, int bpc, const float* __restrict__ saved,
                                                        const float* __restrict__ dOut, double* __restrict__ partial) {
  __shared__ float wb[132];
  __shared__ float sv[kPpfSaved];
  __shared__ double sh[4 * kPpfSums + kPpfSums];
  const int cloud = blockIdx.x / bpc, blk = blockIdx.x % bpc;
  ppf_load_weights(p, wb);
  if (threadIdx.x >= 192 && threadIdx.x < 192 + kPpfSaved) sv[threadIdx.x - 192] = saved[(int64_t)cloud * kPpfSaved + threadIdx.x - 192];
  __syncthreads();
  const int k = threadIdx.x & 15;
  const float* dO = dOut + (int64_t)cloud * p.n * 12;
  double s[kPpfSums];
#pragma unroll
  for (int q = 0; q < kPpfSums; ++q) s[q] = 0.0;
  for (int it = 0; it < kPts / 16; ++it) {
    const int i = blk * kPts + it * 16 + (threadIdx.x >> 4);
    if (i >= p.n) continue;                 // no cross-lane step inside the loop
    float x[10], y[12], g[12], yh[12];
    ppf_row(p, cloud, i, k, wb, x, y);
    ppf_row_grad(y, sv, dO + (int64_t)i * 12, g, yh);
#pragma unroll
    for (int c = 0; c < 12; ++c) {
      s[c] += (double)g[c];
      s[12 + c] += (double)g[c] * (double)yh[c];
    }
  }
  block_sum<4, kPpfSums>(s, sh);
  if (threadIdx.x < kPpfSums) partial[((int64_t)cloud * bpc + blk) * kPpfSums + threadIdx.x] = sh[4 * kPpfSums + threadIdx.x];
}

// A cloud's partials of one quantity, by the eight lanes of an aligned group: lane j adds the blocks j, j + 8, ... ascending, then a
// fixed xor tree.  Every lane of the group returns the total.
__device__ __forceinline__ double ppf_cloud_total(const double* __restrict__ part, int bpc, int width, int q, int j, bool live) {
  double a = 0.0;
  if (live)
    for (int b = j; b < bpc; b += 8) a += part[(int64_t)b * width + q];
  a += __shfl_xor(a, 1); a += __shfl_xor(a, 2); a += __shfl_xor(a, 4);
  return a;
}

// second stage of pass A, ONE workgroup: sums[cloud][24] = the cloud's totals; then d beta / d gamma += the clouds in ascending order
__global__ __launch_bounds__(256) void ppf_bwd_a_final_kernel(const double* __restrict__ partial, int bpc, int clouds,
                                                              double* __restrict__ sums, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta) {
  const int j = threadIdx.x & 7;
  const int total = clouds * kPpfSums;
  for (int o0 = 0; o0 < total; o0 += 32) {              // uniform trip count: the shuffles run in every lane
    const int o = o0 + (threadIdx.x >> 3);
    const bool live = o < total;
    const int cloud = live ? o / kPpfSums : 0, q = live ? o % kPpfSums : 0;
    const double a = ppf_cloud_total(partial + (int64_t)cloud * bpc * kPpfSums, bpc, kPpfSums, q, j, live);
    if (live && j == 0) sums[o] = a;
  }
  __syncthreads();                                      // one workgroup: its own global writes are visible to it after the barrier
  if (threadIdx.x < kPpfSums) {
    double a = 0.0;
    for (int cl = 0; cl < clouds; ++cl) a += sums[cl * kPpfSums + threadIdx.x];
    if (threadIdx.x < 12) dbeta[threadIdx.x] += (float)a;
    else dgamma[threadIdx.x - 12] += (float)a;
  }
}

// pass B: partial[cloud][blk][132] = this workgroup's sum over its rows of dy[c] x[q] ([12][10]) and of dy[c] ([12])
constexpr int kTLd = 16;       // LDS row of a wave's [64 rows][16] tiles: the MFMA operand reads of a step are 64 consecutive floats
__global__ __launch_bounds__(256) void ppf_bwd_b_kernel(const PpfArgs p, int bpc, const float* __restrict__ saved,
                                                        const float* __restrict__ dOut, const double* __restrict__ sums,
                                                        double* __restrict__ partial) {
  __shared__ float wb[132];
  __shared__ float sv[kPpfSaved];
  __shared__ float gm[8];                                                   // per group: S1 / m, S2 / m
  __shared__ __attribute__((aligned(16))) float dyT[4][64 * kTLd];          // per wave: row-major [row][channel], channels 12 .. 15 zero
  __shared__ __attribute__((aligned(16))) float xT[4][64 * kTLd];           // per wave: [row][x 0 .. 9, 1, 0 ...]
  __shared__ float tile[4][16 * 16];
  const int cloud = blockIdx.x / bpc, blk = blockIdx.x % bpc;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  ppf_load_weights(p, wb);
  if (threadIdx.x >= 192 && threadIdx.x < 192 + kPpfSaved) sv[threadIdx.x - 192] = saved[(int64_t)cloud * kPpfSaved + threadIdx.x - 192];
  if (threadIdx.x >= 224 && threadIdx.x < 232) {
    const int g = (threadIdx.x - 224) >> 1, which = (threadIdx.x - 224) & 1;
    const double* sm = sums + (int64_t)cloud * kPpfSums + 12 * which;       // d beta (S1) or d gamma (S2) of the cloud
    double a = 0.0;
    for (int c = 3 * g; c < 3 * g + 3; ++c) a += (double)p.gamma[c] * sm[c];
    gm[2 * g + which] = (float)(a / (3.0 * (double)p.n * (double)kKnn));
  }
  __syncthreads();
  const int k = threadIdx.x & 15;
  const float* dO = dOut + (int64_t)cloud * p.n * 12;
  float* myd = &dyT[w][lane * kTLd];
  float* myx = &xT[w][lane * kTLd];
  const int fr = lane & 15, fq = lane >> 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int it = 0; it < kPts / 16; ++it) {
    const int i = blk * kPts + it * 16 + (threadIdx.x >> 4);
    const bool live = i < p.n;              // dead lanes hand the product rows of zeros
    float dy[16], xx[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) { dy[c] = 0.f; xx[c] = 0.f; }
    if (live) {
      float x[10], y[12], g[12], yh[12];
      ppf_row(p, cloud, i, k, wb, x, y);
      ppf_row_grad(y, sv, dO + (int64_t)i * 12, g, yh);
#pragma unroll
      for (int c = 0; c < 12; ++c) {
        const int gr = c / 3;
        const float t = __fsub_rn(__fsub_rn(__fmul_rn(g[c], p.gamma[c]), gm[2 * gr]), __fmul_rn(yh[c], gm[2 * gr + 1]));
        dy[c] = __fmul_rn(sv[25 + 2 * gr], t);
      }
#pragma unroll
      for (int q = 0; q < 10; ++q) xx[q] = x[q];
      xx[10] = 1.f;                         // the bias column
    }
#pragma unroll
    for (int c = 0; c < 16; c += 4) {
      *reinterpret_cast<float4*>(myd + c) = make_float4(dy[c], dy[c + 1], dy[c + 2], dy[c + 3]);
      *reinterpret_cast<float4*>(myx + c) = make_float4(xx[c], xx[c + 1], xx[c + 2], xx[c + 3]);
    }
    __syncthreads();
    // D[c][q] += sum over the wave's 64 rows of dy[row][c] xx[row][q]: 16 steps of four rows, rows ascending
#pragma unroll
    for (int s4 = 0; s4 < 16; ++s4)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dyT[w][(4 * s4 + fq) * kTLd + fr], xT[w][(4 * s4 + fq) * kTLd + fr], acc, 0, 0, 0);
    __syncthreads();                        // the tiles are rewritten by the next trip
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) tile[w][(4 * fq + r) * 16 + fr] = acc[r];     // D layout: row 4 (lane >> 4) + r, column lane & 15
  __syncthreads();
  if (threadIdx.x < kPpfDw) {
    const int c = threadIdx.x < 120 ? threadIdx.x / 10 : threadIdx.x - 120, q = threadIdx.x < 120 ? threadIdx.x % 10 : 10;
    double a = 0.0;
    for (int ww = 0; ww < 4; ++ww) a += (double)tile[ww][c * 16 + q];
    partial[((int64_t)cloud * bpc + blk) * kPpfDw + threadIdx.x] = a;
  }
}

// second stage of pass B: eight lanes per output; per cloud the fixed-order total, the clouds added in ascending order
__global__ __launch_bounds__(256) void ppf_bwd_b_final_kernel(const double* __restrict__ partial, int bpc, int clouds,
                                                              float* __restrict__ dW, float* __restrict__ db) {
  const int o = blockIdx.x * 32 + (threadIdx.x >> 3), j = threadIdx.x & 7;
  const bool live = o < kPpfDw;
  double a = 0.0;
  for (int cl = 0; cl < clouds; ++cl) a += ppf_cloud_total(partial + (int64_t)cl * bpc * kPpfDw, bpc, kPpfDw, live ? o : 0, j, live);
  if (!live || j != 0) return;
  if (o < 120) dW[o] += (float)a;
  else db[o - 120] += (float)a;
}

// The normal of point i of cloud P [n][stride] from the `cnt` entries of its list nb, in list order; cnt < 3 (a CSR row too short to
// span a plane): normal 0, flag 1.  One body for the fixed 16-entry lists and the CSR rows: the same bytes where the lists agree.
__device__ __forceinline__ void normal_of_list(const float* __restrict__ P, int stride, int n, int i, const int32_t* __restrict__ nb, int cnt,
                                               float vx, float vy, float vz, float* __restrict__ o, int32_t* __restrict__ flag_out) {
  double m[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < cnt; ++k) {
    const int j = min(max(nb[k], 0), n - 1);
    for (int a = 0; a < 3; ++a) m[a] += (double)P[(int64_t)j * stride + a];
  }
  for (int a = 0; a < 3; ++a) m[a] = m[a] / (double)cnt;
  double Cm[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int k = 0; k < cnt; ++k) {         // the neighbours are read a second time (cache hits) instead of held in 96 registers
    const int j = min(max(nb[k], 0), n - 1);
    double e[3];
    for (int a = 0; a < 3; ++a) e[a] = (double)P[(int64_t)j * stride + a] - m[a];
    for (int a = 0; a < 3; ++a)
      for (int b = a; b < 3; ++b) Cm[a][b] += e[a] * e[b];
  }
  Cm[1][0] = Cm[0][1]; Cm[2][0] = Cm[0][2]; Cm[2][1] = Cm[1][2];
  bool finite = cnt >= 3;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) finite = finite && isfinite(Cm[a][b]);
  double nv[3] = {0.0, 0.0, 0.0};
  int flag = 1;
  if (finite) {
    double U[3][3], S[3], V[3][3];
    svd3(Cm, U, S, V);
    const double len = sqrt(V[0][2] * V[0][2] + V[1][2] * V[1][2] + V[2][2] * V[2][2]);
    if (S[0] > 0.0 && len > 0.0 && isfinite(len)) {
      for (int a = 0; a < 3; ++a) nv[a] = V[a][2] / len;
      const double t = nv[0] * ((double)vx - (double)P[(int64_t)i * stride]) + nv[1] * ((double)vy - (double)P[(int64_t)i * stride + 1]) +
                       nv[2] * ((double)vz - (double)P[(int64_t)i * stride + 2]);
      bool flip = t < 0.0;
      if (t == 0.0) {
        int mx = 0;
        if (fabs(nv[1]) > fabs(nv[mx])) mx = 1;
        if (fabs(nv[2]) > fabs(nv[mx])) mx = 2;
        flip = nv[mx] < 0.0;
      }
      if (!(t == t)) { nv[0] = nv[1] = nv[2] = 0.0; }      // a non-finite point or viewpoint: degenerate
      else {
        if (flip) for (int a = 0; a < 3; ++a) nv[a] = -nv[a];
        flag = 0;
      }
    }
  }
  o[0] = (float)nv[0]; o[1] = (float)nv[1]; o[2] = (float)nv[2];
  if (flag_out) *flag_out = flag;
}

__global__ __launch_bounds__(256) void estimate_normals_kernel(const float* __restrict__ pts, int64_t pts_cs, int stride,
                                                               const int32_t* __restrict__ neigh, int64_t neigh_cs, int n, float vx,
                                                               float vy, float vz, float* __restrict__ normals,
                                                               int32_t* __restrict__ flags) {
  const int cloud = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t r = (int64_t)cloud * n + i;
  normal_of_list(pts + cloud * pts_cs, stride, n, i, neigh + cloud * neigh_cs + (int64_t)i * kKnn, kKnn, vx, vy, vz, normals + r * 3,
                 flags ? flags + r : nullptr);
}

// the same over a CSR with cloud-local columns (dsir_fpfh's csr form): row (cloud, i) = cols[offsets[cloud n + i] .. offsets[cloud n + i + 1])
__global__ __launch_bounds__(256) void estimate_normals_csr_kernel(const float* __restrict__ pts, int64_t pts_cs, int stride,
                                                                   const int32_t* __restrict__ offsets, const int32_t* __restrict__ cols, int n,
                                                                   float vx, float vy, float vz, float* __restrict__ normals,
                                                                   int32_t* __restrict__ flags) {
  const int cloud = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t r = (int64_t)cloud * n + i;
  const int b = offsets[r], cnt = max(offsets[r + 1] - b, 0);
  normal_of_list(pts + cloud * pts_cs, stride, n, i, cols + b, cnt, vx, vy, vz, normals + r * 3, flags ? flags + r : nullptr);
}

}  // namespace

static_assert(kPpfMaxBlocks == kGnMaxContrib, "ppf_plan.h bounds the workgroups per cloud by the exact limbs' contribution limit");
int ppf_gn_contributions(int n) { return ppf_blocks(n); }

bool launch_ppf_pre(const PpfArgs& a, hipStream_t st) {
  if (a.n <= 0 || a.clouds <= 0) return true;
  if (!a.xyz || !a.nrm || !a.neigh || !a.W || !a.b || !a.gamma || !a.beta || !a.stats || !a.out) return false;
  const int bpc = ppf_gn_contributions(a.n);
  if (bpc > kGnMaxContrib || (int64_t)bpc * a.clouds > 0x7fffffffll) return false;
  const dim3 grid((unsigned)((int64_t)bpc * a.clouds));
  hipLaunchKernelGGL(ppf_stats_kernel, grid, dim3(256), 0, st, a, bpc);
  hipLaunchKernelGGL(ppf_apply_kernel, grid, dim3(256), 0, st, a, bpc);
  return true;
}

void launch_estimate_normals(const float* pts, int64_t pts_cs, int stride, const int32_t* neigh, int64_t neigh_cs, int n, int clouds,
                             float vx, float vy, float vz, float* normals, int32_t* flags, hipStream_t st) {
  if (n <= 0 || clouds <= 0) return;
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)clouds);
  hipLaunchKernelGGL(estimate_normals_kernel, grid, dim3(256), 0, st, pts, pts_cs, stride, neigh, neigh_cs, n, vx, vy, vz, normals, flags);
}

void launch_estimate_normals_csr(const float* pts, int64_t pts_cs, int stride, const int32_t* offsets, const int32_t* cols, int n, int clouds,
                                 float vx, float vy, float vz, float* normals, int32_t* flags, hipStream_t st) {
  if (n <= 0 || clouds <= 0) return;
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)clouds);
  hipLaunchKernelGGL(estimate_normals_csr_kernel, grid, dim3(256), 0, st, pts, pts_cs, stride, offsets, cols, n, vx, vy, vz, normals, flags);
}

}  // namespace dsir

using namespace dsir;

namespace {
// rows [clouds][n][stride]: columns 0 - 2 the point, 3 - 5 its normal; neigh [clouds][n][16]
PpfArgs ppf_train_args(const float* rows, int stride, const int32_t* neigh, int clouds, int n, const float* W, const float* b,
                       const float* gamma, const float* beta) {
  PpfArgs a;
  a.xyz = rows; a.xyz_cs = (int64_t)n * stride; a.xyz_ld = stride;
  a.nrm = rows + 3; a.nrm_cs = (int64_t)n * stride; a.nrm_ld = stride;
  a.neigh = neigh; a.neigh_cs = (int64_t)n * kKnn;
  a.W = W; a.b = b; a.gamma = gamma; a.beta = beta;
  a.n = n; a.clouds = clouds;
  return a;
}
}  // namespace

extern "C" {

size_t dsir_t_ppf_fwd_scratch(int clouds, int n) { return ppf_fwd_scratch_bytes(clouds, n); }

int dsir_t_ppf_fwd(void* stream, const float* rows, int stride, const int32_t* neigh, int clouds, int n, const float* W, const float* b,
                   const float* gamma, const float* beta, float* out, float* saved, void* scratch) {
  if (!rows || !neigh || !W || !b || !gamma || !beta || !out || !saved || !scratch || stride < 6 || !ppf_shape_ok(clouds, n))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  PpfArgs a = ppf_train_args(rows, stride, neigh, clouds, n, W, b, gamma, beta);
  a.stats = reinterpret_cast<double*>(scratch);
  a.out = out; a.out_cs = (int64_t)n * 12;
  a.saved = saved;
  if (hipError_t e = hipMemsetAsync(scratch, 0, ppf_fwd_scratch_bytes(clouds, n), st)) return (int)e;
  if (!launch_ppf_pre(a, st)) return (int)hipErrorInvalidValue;
  return (int)hipGetLastError();
}

size_t dsir_t_ppf_bwd_scratch(int clouds, int n) { return ppf_bwd_scratch_bytes(clouds, n); }

int dsir_t_ppf_bwd(void* stream, const float* rows, int stride, const int32_t* neigh, int clouds, int n, const float* W, const float* b,
                   const float* gamma, const float* beta, const float* saved, const float* dOut, float* dW, float* db, float* dgamma,
                   float* dbeta, void* scratch) {
  if (!rows || !neigh || !W || !b || !gamma || !beta || !saved || !dOut || !dW || !db || !dgamma || !dbeta || !scratch || stride < 6 ||
      !ppf_shape_ok(clouds, n))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const PpfArgs a = ppf_train_args(rows, stride, neigh, clouds, n, W, b, gamma, beta);
  const PpfBwdPlan pl = ppf_bwd_plan(clouds, n);
  double* base = reinterpret_cast<double*>(scratch);
  const dim3 grid((unsigned)((int64_t)pl.bpc * clouds));
  hipLaunchKernelGGL(ppf_bwd_a_kernel, grid, dim3(256), 0, st, a, pl.bpc, saved, dOut, base + pl.part_a);
  hipLaunchKernelGGL(ppf_bwd_a_final_kernel, dim3(1), dim3(256), 0, st, base + pl.part_a, pl.bpc, clouds, base + pl.sums, dgamma, dbeta);
  hipLaunchKernelGGL(ppf_bwd_b_kernel, grid, dim3(256), 0, st, a, pl.bpc, saved, dOut, base + pl.sums, base + pl.part_b);
  hipLaunchKernelGGL(ppf_bwd_b_final_kernel, dim3((kPpfDw + 31) / 32), dim3(256), 0, st, base + pl.part_b, pl.bpc, clouds, dW, db);
  return (int)hipGetLastError();
}

}  // extern "C"
