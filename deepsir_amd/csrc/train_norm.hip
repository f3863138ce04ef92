// Training operators, normalisation (include/dsir_train.h): GroupNorm / BatchNorm1d(training) forward and backward in two deterministic
// reduction stages (row chunks: gn_chunks, train_layouts.h), the BatchNorm running statistics, L2 normalisation over channels.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include <cstdlib>

#include "device_utils.h"
#include "dsir_train.h"
#include "kernels.h"
#include "train_ops.h"

namespace dsir {
namespace {

// ---- GroupNorm / BatchNorm(train) -------------------------------------------------------------------------------------
// stage 1: one block per (row chunk, group, cloud): sum and sum of squares over its rows x gw channels, fp64
__global__ __launch_bounds__(256) void t_gn_stats_kernel(const float* __restrict__ Y, int M, int C, int groups, int rows_per_chunk,
                                                         double* __restrict__ partial) {
  const int chunk = blockIdx.x, g = blockIdx.y, cloud = blockIdx.z, gw = C / groups, nchunks = gridDim.x;
  const int r0 = chunk * rows_per_chunk, r1 = min(M, r0 + rows_per_chunk);
  const float* base = Y + ((int64_t)cloud * M + r0) * C + g * gw;
  double s1 = 0.0, s2 = 0.0;
  const int64_t total = (int64_t)max(r1 - r0, 0) * gw;
  for (int64_t e = threadIdx.x; e < total; e += 256) {
    const float v = base[(e / gw) * C + (e % gw)];
    s1 += v; s2 += (double)v * v;
  }
  s1 = wave_sum(s1); s2 = wave_sum(s2);
  __shared__ double sh[2][4];
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s1; sh[1][threadIdx.x >> 6] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = partial + (((int64_t)cloud * groups + g) * nchunks + chunk) * 2;
    o[0] = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
    o[1] = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
  }
}

// stage 2: mean, 1 / sqrt(var + eps).  Eight lanes per (cloud, group): lane j adds the chunks j, j + 8, ... in order, then a fixed
// xor tree - deterministic, and 32 dependent loads instead of 256 on the large layers
__global__ __launch_bounds__(256) void t_gn_stats_final_kernel(const double* __restrict__ partial, int nchunks, int count, double inv_total,
                                                               float* __restrict__ stats) {
  const int i = blockIdx.x * 32 + (threadIdx.x >> 3);      // cloud * groups + g
  const int j = threadIdx.x & 7;
  double a = 0.0, b = 0.0;
  if (i < count)
    for (int c = j; c < nchunks; c += 8) { a += partial[((int64_t)i * nchunks + c) * 2]; b += partial[((int64_t)i * nchunks + c) * 2 + 1]; }
  a += __shfl_xor(a, 1); b += __shfl_xor(b, 1);
  a += __shfl_xor(a, 2); b += __shfl_xor(b, 2);
  a += __shfl_xor(a, 4); b += __shfl_xor(b, 4);
  if (i >= count || j != 0) return;
  const double mean = a * inv_total;
  double var = b * inv_total - mean * mean;
  var = var > 0.0 ? var : 0.0;
  stats[2 * i] = (float)mean;
  stats[2 * i + 1] = (float)(1.0 / sqrt(var + 1e-5));
}

__global__ void t_gn_apply_kernel(const float* __restrict__ Y, const float* __restrict__ stats, int M, int C, int groups,
                                  const float* __restrict__ gamma, const float* __restrict__ beta, int act, float* __restrict__ out,
                                  int64_t total) {
  const int gw = C / groups;
  if ((C & 3) == 0 && ((reinterpret_cast<uintptr_t>(Y) | reinterpret_cast<uintptr_t>(out)) & 15) == 0) {
    // four consecutive channels of one row per trip (C % 4 == 0: a float4 never straddles rows), same arithmetic per element
    for (int64_t e = 4 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x); e < total; e += 4 * (int64_t)gridDim.x * blockDim.x) {
      const int c = (int)(e % C);
      const int64_t cloud = e / ((int64_t)M * C);
      const float4 y4 = *reinterpret_cast<const float4*>(Y + e);
      const float yv[4] = {y4.x, y4.y, y4.z, y4.w};
      float o[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float* st = stats + (cloud * groups + (c + u) / gw) * 2;
        float v = (yv[u] - st[0]) * st[1] * gamma[c + u] + beta[c + u];
        if (act && !(v > 0.f)) v *= 0.2f;
        o[u] = v;
      }
      *reinterpret_cast<float4*>(out + e) = make_float4(o[0], o[1], o[2], o[3]);
    }
    return;
  }
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const int64_t cloud = e / ((int64_t)M * C);
    const float* st = stats + (cloud * groups + c / gw) * 2;
    float v = (Y[e] - st[0]) * st[1] * gamma[c] + beta[c];
    if (act && !(v > 0.f)) v *= 0.2f;
    out[e] = v;
  }
}

// stage 1, per (cloud, row chunk, channel): s1 = sum_r g, s2 = sum_r g xhat, g = dOut * slope(v); block = 32 channels x 8 row lanes
__global__ __launch_bounds__(256) void t_gn_bwd_sums_kernel(const float* __restrict__ dOut, const float* __restrict__ Y,
                                                            const float* __restrict__ stats, int M, int C, int groups,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, int act,
                                                            int rows_per_chunk, float* __restrict__ partial) {
  const int cloud = blockIdx.z, chunk = blockIdx.y, nchunks = gridDim.y;
  const int c = blockIdx.x * 32 + (threadIdx.x & 31), ry = threadIdx.x >> 5;
  const int gw = C / groups;
  const int r0 = chunk * rows_per_chunk, r1 = min(M, r0 + rows_per_chunk);
  double s1 = 0.0, s2 = 0.0;
  if (c < C) {
    const float* st = stats + ((int64_t)cloud * groups + c / gw) * 2;
    const float mean = st[0], rstd = st[1], ga = gamma[c], be = beta[c];
    for (int r = r0 + ry; r < r1; r += 8) {
      const int64_t e = ((int64_t)cloud * M + r) * C + c;
      const float xh = (Y[e] - mean) * rstd;
      float g = dOut[e];
      if (act && !(xh * ga + be > 0.f)) g *= 0.2f;
      s1 += g; s2 += (double)g * xh;
    }
  }
  __shared__ double sh[2][8][32];
  sh[0][ry][threadIdx.x & 31] = s1; sh[1][ry][threadIdx.x & 31] = s2;
  __syncthreads();
  if (ry == 0 && c < C) {
    double a = 0.0, b = 0.0;
    for (int i = 0; i < 8; ++i) { a += sh[0][i][threadIdx.x]; b += sh[1][i][threadIdx.x]; }
    float* o = partial + (((int64_t)cloud * nchunks + chunk) * C + c) * 2;
    o[0] = (float)a; o[1] = (float)b;
  }
}

// stage 2: sums[cloud][C][2]; eight lanes per output as in t_gn_stats_final_kernel
__global__ __launch_bounds__(256) void t_gn_bwd_sums_final_kernel(const float* __restrict__ partial, int nchunks, int C, int64_t count,
                                                                  float* __restrict__ sums) {
  const int64_t i = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);     // (cloud * C + c) * 2 + which
  const int j = threadIdx.x & 7;
  double a = 0.0;
  if (i < count) {
    const int64_t cloud = i / (2 * C), rest = i % (2 * C);
    for (int k = j; k < nchunks; k += 8) a += partial[(cloud * nchunks + k) * 2 * C + rest];
  }
  a += __shfl_xor(a, 1); a += __shfl_xor(a, 2); a += __shfl_xor(a, 4);
  if (i < count && j == 0) sums[i] = (float)a;
}

// dY = rstd (gamma g - mean_group(gamma g) - xhat mean_group(gamma g xhat)); one block per (row range, cloud)
__global__ __launch_bounds__(256) void t_gn_bwd_apply_kernel(const float* __restrict__ dOut, const float* __restrict__ Y,
                                                             const float* __restrict__ stats, const float* __restrict__ sums, int M,
                                                             int C, int groups, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, int act, float* __restrict__ dY,
                                                             int rows_per_block, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  extern __shared__ float gm[];   // [groups][2]: mean(gamma g), mean(gamma g xhat)
  const int cloud = blockIdx.y, gw = C / groups;
  // the parameter gradients (sums over the clouds, in cloud order) ride along in the first workgroup: one launch less per layer
  if (blockIdx.x == 0 && blockIdx.y == 0)
    for (int c = threadIdx.x; c < C; c += 256) {
      float a = 0.f, b = 0.f;
      for (int i = 0; i < (int)gridDim.y; ++i) { a += sums[((int64_t)i * C + c) * 2]; b += sums[((int64_t)i * C + c) * 2 + 1]; }
      dbeta[c] += a;
      dgamma[c] += b;
    }
  for (int g = threadIdx.x; g < groups; g += 256) {
    double a = 0.0, b = 0.0;
    for (int c = g * gw; c < (g + 1) * gw; ++c) {
      a += (double)gamma[c] * sums[((int64_t)cloud * C + c) * 2];
      b += (double)gamma[c] * sums[((int64_t)cloud * C + c) * 2 + 1];
    }
    const double inv = 1.0 / ((double)M * gw);
    gm[2 * g] = (float)(a * inv); gm[2 * g + 1] = (float)(b * inv);
  }
  __syncthreads();
  const int r0 = blockIdx.x * rows_per_block;
  const int64_t n = (int64_t)min(rows_per_block, M - r0) * C;
  const int64_t base = ((int64_t)cloud * M + r0) * C;
  // C a power of two <= 1024 (every layer of the network): a thread's four consecutive channels are the same in every trip
  // (4 tid + 1024 k mod C), so their parameters are loaded once and the tensors travel as float4 - same arithmetic per element
  if ((C & 3) == 0 && (1024 % C) == 0 && ((reinterpret_cast<uintptr_t>(Y) | reinterpret_cast<uintptr_t>(dOut) | reinterpret_cast<uintptr_t>(dY)) & 15) == 0) {
    const int c0 = (4 * threadIdx.x) % C;
    float mean[4], rstd[4], ga[4], be[4], g0[4], g1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c0 + u, g = c / gw;
      const float* st = stats + ((int64_t)cloud * groups + g) * 2;
      mean[u] = st[0]; rstd[u] = st[1]; ga[u] = gamma[c]; be[u] = beta[c]; g0[u] = gm[2 * g]; g1[u] = gm[2 * g + 1];
    }
    for (int64_t i = 4 * (int64_t)threadIdx.x; i < n; i += 1024) {
      const float4 y4 = *reinterpret_cast<const float4*>(Y + base + i);
      const float4 d4 = *reinterpret_cast<const float4*>(dOut + base + i);
      const float yv[4] = {y4.x, y4.y, y4.z, y4.w};
      float dv[4] = {d4.x, d4.y, d4.z, d4.w};
      float o[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float xh = (yv[u] - mean[u]) * rstd[u];
        if (act && !(xh * ga[u] + be[u] > 0.f)) dv[u] *= 0.2f;
        o[u] = rstd[u] * (ga[u] * dv[u] - g0[u] - xh * g1[u]);
      }
      *reinterpret_cast<float4*>(dY + base + i) = make_float4(o[0], o[1], o[2], o[3]);
    }
    return;
  }
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const int64_t e = base + i;
    const int c = (int)(e % C), g = c / gw;
    const float* st = stats + ((int64_t)cloud * groups + g) * 2;
    const float xh = (Y[e] - st[0]) * st[1];
    float d = dOut[e];
    if (act && !(xh * gamma[c] + beta[c] > 0.f)) d *= 0.2f;
    dY[e] = st[1] * (gamma[c] * d - gm[2 * g] - xh * gm[2 * g + 1]);
  }
}

// running statistics of nn.BatchNorm1d in training mode: running = (1 - momentum) running + momentum batch, the variance
// unbiased (M / (M - 1)); stats [C][2] = {mean, rstd} of dsir_t_gn_fwd with groups = C
__global__ void t_bn_running_kernel(const float* __restrict__ stats, int C, double M, float momentum, float* __restrict__ rmean,
                                    float* __restrict__ rvar) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double mean = stats[2 * c], rstd = stats[2 * c + 1];
  const double var = fmax(1.0 / (rstd * rstd) - 1e-5, 0.0) * (M > 1.0 ? M / (M - 1.0) : 1.0);
  rmean[c] = (float)((1.0 - momentum) * rmean[c] + momentum * mean);
  rvar[c] = (float)((1.0 - momentum) * rvar[c] + momentum * var);
}

// ---- L2 normalisation over channels (F.normalize, p = 2, eps 1e-12) -------------------------------------------------
__global__ void t_l2norm_fwd_kernel(const float* __restrict__ x, int64_t rows, int C, float* __restrict__ y, float* __restrict__ nrm) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += x[r * C + c] * x[r * C + c];
    const float n = fmaxf(sqrtf(s), 1e-12f);
    nrm[r] = n;
    for (int c = 0; c < C; ++c) y[r * C + c] = x[r * C + c] / n;
  }
}
__global__ void t_l2norm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ nrm, int64_t rows,
                                    int C, float* __restrict__ dx) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
    float dot = 0.f;
    for (int c = 0; c < C; ++c) dot += y[r * C + c] * dy[r * C + c];
    const float inv = 1.f / nrm[r];
    for (int c = 0; c < C; ++c) dx[r * C + c] = (dy[r * C + c] - y[r * C + c] * dot) * inv;
  }
}

}  // namespace
}  // namespace dsir

using namespace dsir;

extern "C" {

size_t dsir_t_gn_scratch(int clouds, int M, int C) { return gn_scratch_bytes(clouds, M, C); }

int dsir_t_gn_fwd(void* stream, const float* Y, int clouds, int M, int C, int groups, const float* gamma, const float* beta, int act,
                  float* out, float* stats, void* scratch) {
  if (!Y || !gamma || !beta || !out || !stats || !scratch || clouds < 1 || M < 1 || C < 1 || groups < 1 || C % groups)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int nch = gn_chunks(M), rpc = (M + nch - 1) / nch;
  double* partial = at<double>(scratch, GnFwdLayout(clouds, M, C, groups).partial);
  hipLaunchKernelGGL(t_gn_stats_kernel, dim3(nch, groups, clouds), dim3(256), 0, st, Y, M, C, groups, rpc, partial);
  hipLaunchKernelGGL(t_gn_stats_final_kernel, dim3((clouds * groups + 31) / 32), dim3(256), 0, st, partial, nch, clouds * groups,
                     1.0 / ((double)M * (C / groups)), stats);
  const int64_t total = (int64_t)clouds * M * C;
  hipLaunchKernelGGL(t_gn_apply_kernel, dim3(grid1((C & 3) == 0 ? total / 4 : total)), dim3(256), 0, st, Y, stats, M, C, groups, gamma, beta, act, out, total);
  return done();
}

int dsir_t_gn_bwd(void* stream, const float* dOut, const float* Y, const float* stats, int clouds, int M, int C, int groups,
                  const float* gamma, const float* beta, int act, float* dY, float* dgamma, float* dbeta, void* scratch) {
  if (!dOut || !Y || !stats || !gamma || !beta || !dY || !dgamma || !dbeta || !scratch || clouds < 1 || M < 1 || C < 1 || groups < 1 ||
      C % groups || groups > 4096)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int nch = gn_chunks(M), rpc = (M + nch - 1) / nch;
  const GnBwdLayout lay(clouds, M, C);
  float* partial = at<float>(scratch, lay.partial);
  float* sums = at<float>(scratch, lay.sums);
  hipLaunchKernelGGL(t_gn_bwd_sums_kernel, dim3((C + 31) / 32, nch, clouds), dim3(256), 0, st, dOut, Y, stats, M, C, groups, gamma, beta, act,
                     rpc, partial);
  const int64_t cnt = (int64_t)clouds * C * 2;
  hipLaunchKernelGGL(t_gn_bwd_sums_final_kernel, dim3((unsigned)((cnt + 31) / 32)), dim3(256), 0, st, partial, nch, C, cnt, sums);
  // elements per block: 16 k on the large layers, down to 4 k where that is needed for ~1000 workgroups (a block first forms the
  // group means from `sums`: C loads - not less than that many elements per thread-block pass)
  const int64_t total = (int64_t)clouds * M * C;
  int64_t per = total / 1024;
  per = per < 4096 ? 4096 : (per > 16384 ? 16384 : per);
  int rpb = (int)((per + C - 1) / C);
  rpb = rpb < 1 ? 1 : rpb;
  hipLaunchKernelGGL(t_gn_bwd_apply_kernel, dim3((M + rpb - 1) / rpb, clouds), dim3(256), (size_t)groups * 2 * sizeof(float), st, dOut, Y,
                     stats, sums, M, C, groups, gamma, beta, act, dY, rpb, dgamma, dbeta);
  return done();
}

int dsir_t_bn_running(void* stream, const float* stats, int C, int64_t M, float momentum, float* running_mean, float* running_var) {
  if (!stats || !running_mean || !running_var || C < 1 || M < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(t_bn_running_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, stats, C, (double)M, momentum,
                     running_mean, running_var);
  return done();
}

int dsir_t_l2norm_fwd(void* stream, const float* x, int64_t rows, int C, float* y, float* norms) {
  if (!x || !y || !norms || rows < 1 || C < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(t_l2norm_fwd_kernel, dim3(grid1(rows)), dim3(256), 0, (hipStream_t)stream, x, rows, C, y, norms);
  return done();
}

int dsir_t_l2norm_bwd(void* stream, const float* dy, const float* y, const float* norms, int64_t rows, int C, float* dx) {
  if (!dy || !y || !norms || !dx || rows < 1 || C < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(t_l2norm_bwd_kernel, dim3(grid1(rows)), dim3(256), 0, (hipStream_t)stream, dy, y, norms, rows, C, dx);
  return done();
}

}  // extern "C"
