// Training operators, row gathers and pooling (include/dsir_train.h): gather and its backward as an ordered sum through the scatter plan,
// relative position encoding, the inlier model's input, attentive pooling and max pooling, each with its backward.
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

// ---- gathers ----------------------------------------------------------------------------------------------------------
__global__ void t_gather_kernel(const float* __restrict__ X, int n, int C, const int32_t* __restrict__ idx, int m, float* __restrict__ Y,
                                int ldy, int col_off, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const int64_t j = e / C;                 // cloud * m + j
    const int64_t cloud = j / m;
    int i = idx[j];
    i = i < 0 ? 0 : (i >= n ? n - 1 : i);
    Y[j * ldy + col_off + c] = X[(cloud * n + i) * C + c];
  }
}

// backward of a gather: dX[d][c] = sum of dY over the sources of destination row d, in ascending source order (the plan of
// launch_scatter_plan): every sum has one order - no float atomics, same bits every run
__global__ void t_scatter_sum_kernel(const float* __restrict__ dY, int ldy, int col_off, const int32_t* __restrict__ order,
                                     const int32_t* __restrict__ offsets, float* __restrict__ dX, int C, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const int64_t d = e / C;                 // cloud * n + i
    float s = 0.f;
    for (int q = offsets[d]; q < offsets[d + 1]; ++q) s += dY[(int64_t)order[q] * ldy + col_off + c];
    dX[e] = s;
  }
}

__global__ void t_relpos_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ idx, int n, int k, float* __restrict__ out,
                                int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = e / k;                 // cloud * n + i
    const int64_t cloud = p / n;
    int j = idx[e];
    j = j < 0 ? 0 : (j >= n ? n - 1 : j);
    const float* pi = xyz + p * 3;
    const float* pj = xyz + (cloud * n + j) * 3;
    const float dx = pj[0] - pi[0], dy = pj[1] - pi[1], dz = pj[2] - pi[2];
    float* o = out + e * 10;
    o[0] = sqrtf(dx * dx + dy * dy + dz * dz);
    o[1] = dx; o[2] = dy; o[3] = dz;
    o[4] = pi[0]; o[5] = pi[1]; o[6] = pi[2];
    o[7] = pj[0]; o[8] = pj[1]; o[9] = pj[2];
  }
}

// the inlier model's input of one registration iteration (model.py:571-573 with :587): [T x_src ; x_ref[idx]]
__global__ void t_inlier_input_kernel(const float* __restrict__ xs, const float* __restrict__ xr, const int32_t* __restrict__ idx,
                                      const float* __restrict__ T, int t_stride, int J, int K, float* __restrict__ out, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t pair = e / J;
    const float* p = xs + e * 3;
    float x = p[0], y = p[1], z = p[2];
    if (T) {
      const float* t = T + pair * t_stride;
      const float a = t[0] * x + t[1] * y + t[2] * z + t[3];
      const float b = t[4] * x + t[5] * y + t[6] * z + t[7];
      const float c = t[8] * x + t[9] * y + t[10] * z + t[11];
      x = a; y = b; z = c;
    }
    int i = idx[e];
    i = i < 0 ? 0 : (i >= K ? K - 1 : i);
    const float* q = xr + (pair * K + i) * 3;
    float* o = out + e * 6;
    o[0] = x; o[1] = y; o[2] = z; o[3] = q[0]; o[4] = q[1]; o[5] = q[2];
  }
}

// ---- attentive pooling ------------------------------------------------------------------------------------------------
// k = 16 neighbours (the network's only value): a point's column of scores and features lives in registers - one read of S and
// cat and one exp per element instead of three reads and two exps; same operations in the same order (same bits)
__global__ void t_attpool_fwd_kernel(const float* __restrict__ cat, float* __restrict__ S, int k, int C, float* __restrict__ out,
                                     int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const int64_t p = e / C;
    const int64_t b = p * k * C + c;
    if (k == 16) {
      float sv[16], cv[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) { sv[t] = S[b + (int64_t)t * C]; cv[t] = cat[b + (int64_t)t * C]; }
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < 16; ++t) mx = fmaxf(mx, sv[t]);
      float se = 0.f;
#pragma unroll
      for (int t = 0; t < 16; ++t) { sv[t] = expf(sv[t] - mx); se += sv[t]; }
      const float inv = 1.f / se;
      float o = 0.f;
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const float a = sv[t] * inv;
        S[b + (int64_t)t * C] = a;
        o += a * cv[t];
      }
      out[e] = o;
      continue;
    }
    float mx = -INFINITY;
    for (int t = 0; t < k; ++t) mx = fmaxf(mx, S[b + (int64_t)t * C]);
    float se = 0.f;
    for (int t = 0; t < k; ++t) se += expf(S[b + (int64_t)t * C] - mx);
    const float inv = 1.f / se;
    float o = 0.f;
    for (int t = 0; t < k; ++t) {
      const float a = expf(S[b + (int64_t)t * C] - mx) * inv;
      S[b + (int64_t)t * C] = a;
      o += a * cat[b + (int64_t)t * C];
    }
    out[e] = o;
  }
}

__global__ void t_attpool_bwd_kernel(const float* __restrict__ dOut, const float* __restrict__ cat, const float* __restrict__ A, int k,
                                     int C, float* __restrict__ dCat, float* __restrict__ dS, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const int64_t p = e / C;
    const int64_t b = p * k * C + c;
    const float g = dOut[e];
    if (k == 16) {
      float av[16], cv[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) { av[t] = A[b + (int64_t)t * C]; cv[t] = cat[b + (int64_t)t * C]; }
      float dot = 0.f;
#pragma unroll
      for (int t = 0; t < 16; ++t) dot += av[t] * cv[t];
      dot *= g;
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        dCat[b + (int64_t)t * C] = av[t] * g;
        dS[b + (int64_t)t * C] = av[t] * (cv[t] * g - dot);
      }
      continue;
    }
    float dot = 0.f;
    for (int t = 0; t < k; ++t) dot += A[b + (int64_t)t * C] * cat[b + (int64_t)t * C];
    dot *= g;                                // sum_t a_t (cat_t g)
    for (int t = 0; t < k; ++t) {
      const float a = A[b + (int64_t)t * C];
      dCat[b + (int64_t)t * C] = a * g;
      dS[b + (int64_t)t * C] = a * (cat[b + (int64_t)t * C] * g - dot);
    }
  }
}

__global__ void t_maxpool_fwd_kernel(const float* __restrict__ X, int n, int C, const int32_t* __restrict__ pool, int m, int k,
                                     float* __restrict__ out, int32_t* __restrict__ arg, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const int64_t j = e / C;                 // cloud * m + j
    const int64_t cloud = j / m;
    float best = -INFINITY;
    int bi = 0;
    for (int t = 0; t < k; ++t) {
      int i = pool[j * k + t];
      i = i < 0 ? 0 : (i >= n ? n - 1 : i);
      const float v = X[(cloud * n + i) * C + c];
      if (t == 0 || v > best) { best = v; bi = i; }
    }
    out[e] = best;
    arg[e] = bi;
  }
}

// backward of the max over k pooled rows: dX[i][c] = sum of dOut[j][c] over the pooled outputs j whose winner for channel c was row i,
// walked through the inverse of the pool index in ascending (j, t) order; a row listed twice by one output counts once
__global__ void t_maxpool_bwd_kernel(const float* __restrict__ dOut, const int32_t* __restrict__ arg, const int32_t* __restrict__ order,
                                     const int32_t* __restrict__ offsets, int m, int k, int C, float* __restrict__ dX, int n, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const int64_t d = e / C;                 // cloud * n + i
    const int i = (int)(d % n);
    float s = 0.f;
    int64_t prev = -1;
    for (int q = offsets[d]; q < offsets[d + 1]; ++q) {
      const int64_t j = (int64_t)order[q] / k;           // cloud * m + output row
      if (j != prev && arg[j * C + c] == i) s += dOut[j * C + c];
      prev = j;
    }
    dX[e] = s;
  }
}

}  // namespace
}  // namespace dsir

using namespace dsir;

extern "C" {

int dsir_t_gather(void* stream, const float* X, int n, int C, const int32_t* idx, int m, int clouds, float* Y, int ldy, int col_off) {
  if (!X || !idx || !Y || n < 1 || C < 1 || m < 1 || clouds < 1) return (int)hipErrorInvalidValue;
  const int64_t total = (int64_t)clouds * m * C;
  hipLaunchKernelGGL(t_gather_kernel, dim3(grid1(total)), dim3(256), 0, (hipStream_t)stream, X, n, C, idx, m, Y, ldy, col_off, total);
  return done();
}

size_t dsir_t_scatter_plan_scratch(int64_t total) { return total > 0 && total <= 0x7fffffffll ? scatter_plan_scratch_bytes(total) : 0; }

int dsir_t_scatter_plan(void* stream, const int32_t* idx, int m, int clouds, int n, int32_t* order, int32_t* offsets, void* scratch) {
  if (!idx || !order || !offsets || !scratch || m < 1 || clouds < 1 || n < 1) return (int)hipErrorInvalidValue;
  if (int r = launch_scatter_plan(idx, m, clouds, n, order, offsets, scratch, (hipStream_t)stream)) return r;
  return done();
}

int dsir_t_scatter_add(void* stream, const float* dY, int ldy, int col_off, const int32_t* order, const int32_t* offsets, int clouds,
                       float* dX, int n, int C) {
  if (!dY || !order || !offsets || !dX || n < 1 || C < 1 || clouds < 1) return (int)hipErrorInvalidValue;
  const int64_t total = (int64_t)clouds * n * C;
  hipLaunchKernelGGL(t_scatter_sum_kernel, dim3(grid1(total)), dim3(256), 0, (hipStream_t)stream, dY, ldy, col_off, order, offsets, dX, C, total);
  return done();
}

int dsir_t_relpos(void* stream, const float* xyz, const int32_t* idx, int n, int k, int clouds, float* out) {
  if (!xyz || !idx || !out || n < 1 || k < 1 || clouds < 1) return (int)hipErrorInvalidValue;
  const int64_t total = (int64_t)clouds * n * k;
  hipLaunchKernelGGL(t_relpos_kernel, dim3(grid1(total)), dim3(256), 0, (hipStream_t)stream, xyz, idx, n, k, out, total);
  return done();
}

int dsir_t_inlier_input(void* stream, const float* xyz_src, const float* xyz_ref, const int32_t* idx, const float* T, int t_stride,
                        int pairs, int J, int K, float* out) {
  if (!xyz_src || !xyz_ref || !idx || !out || pairs < 1 || J < 1 || K < 1) return (int)hipErrorInvalidValue;
  const int64_t total = (int64_t)pairs * J;
  hipLaunchKernelGGL(t_inlier_input_kernel, dim3(grid1(total)), dim3(256), 0, (hipStream_t)stream, xyz_src, xyz_ref, idx, T, t_stride, J, K,
                     out, total);
  return done();
}

int dsir_t_attpool_fwd(void* stream, const float* cat, float* S, int64_t points, int k, int C, float* out) {
  if (!cat || !S || !out || points < 1 || k < 1 || C < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(t_attpool_fwd_kernel, dim3(grid1(points * C)), dim3(256), 0, (hipStream_t)stream, cat, S, k, C, out, points * C);
  return done();
}

int dsir_t_attpool_bwd(void* stream, const float* dOut, const float* cat, const float* A, int64_t points, int k, int C, float* dCat,
                       float* dS) {
  if (!dOut || !cat || !A || !dCat || !dS || points < 1 || k < 1 || C < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(t_attpool_bwd_kernel, dim3(grid1(points * C)), dim3(256), 0, (hipStream_t)stream, dOut, cat, A, k, C, dCat, dS,
                     points * C);
  return done();
}

int dsir_t_maxpool_fwd(void* stream, const float* X, int n, int C, const int32_t* pool, int m, int k, int clouds, float* out,
                       int32_t* arg) {
  if (!X || !pool || !out || !arg || n < 1 || C < 1 || m < 1 || k < 1 || clouds < 1) return (int)hipErrorInvalidValue;
  const int64_t total = (int64_t)clouds * m * C;
  hipLaunchKernelGGL(t_maxpool_fwd_kernel, dim3(grid1(total)), dim3(256), 0, (hipStream_t)stream, X, n, C, pool, m, k, out, arg, total);
  return done();
}

int dsir_t_maxpool_bwd(void* stream, const float* dOut, const int32_t* arg, const int32_t* order, const int32_t* offsets, int m, int k, int C,
                       int clouds, float* dX, int n) {
  if (!dOut || !arg || !order || !offsets || !dX || n < 1 || C < 1 || m < 1 || k < 1 || clouds < 1) return (int)hipErrorInvalidValue;
  const int64_t total = (int64_t)clouds * n * C;
  hipLaunchKernelGGL(t_maxpool_bwd_kernel, dim3(grid1(total)), dim3(256), 0, (hipStream_t)stream, dOut, arg, order, offsets, m, k, C, dX, n, total);
  return done();
}

}  // extern "C"
