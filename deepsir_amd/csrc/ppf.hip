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
#include "device_utils.h"
#include "kernels.h"
#include "svd3.h"

namespace dsir {

namespace {

constexpr int kPts = 64;      // points per workgroup (four rows per lane)

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

// the 12 raw conv outputs of row (i, k); wb (LDS): W [12][10] then b [12]
__device__ __forceinline__ void ppf_row(const PpfArgs& p, int cloud, int i, int k, const float* wb, float (&y)[12]) {
  int j = p.neigh[cloud * p.neigh_cs + (int64_t)i * kKnn + k];
  j = min(max(j, 0), p.n - 1);                      // a bad neighbour index can never leave the cloud
  const float* xyz = p.xyz + cloud * p.xyz_cs;
  const float* pi = xyz + (int64_t)i * p.xyz_ld;
  const float* pj = xyz + (int64_t)j * p.xyz_ld;
  int ri = i, rj = j;
  if (p.nrm_idx) { const int32_t* t = p.nrm_idx + cloud * p.nrm_idx_cs; ri = t[i]; rj = t[j]; }
  const float* ni = p.nrm + cloud * p.nrm_cs + (int64_t)ri * p.nrm_ld;
  const float* nj = p.nrm + cloud * p.nrm_cs + (int64_t)rj * p.nrm_ld;
  float x[10];
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
    float y[12];
    ppf_row(p, cloud, i, k, wb, y);
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
  }
  __syncthreads();
  const int k = threadIdx.x & 15;
  float* out = p.out + cloud * p.out_cs;
  for (int it = 0; it < kPts / 16; ++it) {
    const int i = blk * kPts + it * 16 + (threadIdx.x >> 4);
    const bool live = i < p.n;              // uniform over the 16 lanes of a point; the butterfly runs in every lane
    float y[12];
    if (live) ppf_row(p, cloud, i, k, wb, y);
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

__global__ __launch_bounds__(256) void estimate_normals_kernel(const float* __restrict__ pts, int64_t pts_cs, int stride,
                                                               const int32_t* __restrict__ neigh, int64_t neigh_cs, int n, float vx,
                                                               float vy, float vz, float* __restrict__ normals,
                                                               int32_t* __restrict__ flags) {
  const int cloud = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* P = pts + cloud * pts_cs;
  const int32_t* nb = neigh + cloud * neigh_cs + (int64_t)i * kKnn;
  double m[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < kKnn; ++k) {
    const int j = min(max(nb[k], 0), n - 1);
    for (int a = 0; a < 3; ++a) m[a] += (double)P[(int64_t)j * stride + a];
  }
  for (int a = 0; a < 3; ++a) m[a] = m[a] / 16.0;
  double Cm[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int k = 0; k < kKnn; ++k) {        // the neighbours are read a second time (cache hits) instead of held in 96 registers
    const int j = min(max(nb[k], 0), n - 1);
    double e[3];
    for (int a = 0; a < 3; ++a) e[a] = (double)P[(int64_t)j * stride + a] - m[a];
    for (int a = 0; a < 3; ++a)
      for (int b = a; b < 3; ++b) Cm[a][b] += e[a] * e[b];
  }
  Cm[1][0] = Cm[0][1]; Cm[2][0] = Cm[0][2]; Cm[2][1] = Cm[1][2];
  bool finite = true;
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
  float* o = normals + ((int64_t)cloud * n + i) * 3;
  o[0] = (float)nv[0]; o[1] = (float)nv[1]; o[2] = (float)nv[2];
  if (flags) flags[(int64_t)cloud * n + i] = flag;
}

}  // namespace

int ppf_gn_contributions(int n) { return (n + kPts - 1) / kPts; }

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

}  // namespace dsir
