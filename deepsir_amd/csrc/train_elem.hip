// Training operators, element-wise (include/dsir_train.h): add + LeakyReLU, dropout mask, sigmoid, axpy, Adam, the NaN flag, and the
// top-k entry (select.hip's launch_topk).
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

__global__ void t_add_leaky_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n, float* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    float v = a[e] + b[e];
    if (!(v > 0.f)) v *= 0.2f;
    out[e] = v;
  }
}
__global__ void t_add_leaky_bwd_kernel(const float* __restrict__ dOut, const float* __restrict__ out, int64_t n, float* __restrict__ d) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
    d[e] = out[e] > 0.f ? dOut[e] : 0.2f * dOut[e];
}
__global__ void t_mul_mask_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask, float scale, int64_t n,
                                  float* __restrict__ y) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
    y[e] = mask[e] ? x[e] * scale : 0.f;
}
__global__ void t_sigmoid_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ y) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) y[e] = 1.f / (1.f + expf(-x[e]));
}
__global__ void t_axpy_kernel(float a, const float* __restrict__ x, int64_t n, float* __restrict__ y) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) y[e] += a * x[e];
}
__global__ void t_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                              int64_t n, float b1, float b2, float eps, float step_size, float inv_sqrt_bc2) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const float gi = g[e];
    const float mi = b1 * m[e] + (1.f - b1) * gi;
    const float vi = b2 * v[e] + (1.f - b2) * gi * gi;
    m[e] = mi; v[e] = vi;
    p[e] -= step_size * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
  }
}

// flag[0] = 1 when any element is NaN (train.py:437-441: the step is skipped then)
__global__ void t_any_nan_kernel(const float* __restrict__ x, int64_t n, int32_t* __restrict__ flag) {
  bool bad = false;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) bad |= x[e] != x[e];
  if (__any(bad) && (threadIdx.x & 63) == 0) flag[0] = 1;
}

}  // namespace
}  // namespace dsir

using namespace dsir;

extern "C" {

int dsir_t_add_leaky_fwd(void* stream, const float* a, const float* b, int64_t n, float* out) {
  if (!a || !b || !out || n < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(t_add_leaky_fwd_kernel, dim3(grid1(n)), dim3(256), 0, (hipStream_t)stream, a, b, n, out);
  return done();
}

int dsir_t_add_leaky_bwd(void* stream, const float* dOut, const float* out, int64_t n, float* d) {
  if (!dOut || !out || !d || n < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(t_add_leaky_bwd_kernel, dim3(grid1(n)), dim3(256), 0, (hipStream_t)stream, dOut, out, n, d);
  return done();
}

int dsir_t_mul_mask(void* stream, const float* x, const uint8_t* mask, float scale, int64_t n, float* y) {
  if (!x || !mask || !y || n < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(t_mul_mask_kernel, dim3(grid1(n)), dim3(256), 0, (hipStream_t)stream, x, mask, scale, n, y);
  return done();
}

size_t dsir_t_topk_scratch(int clouds, int n) { return topk_scratch_bytes(clouds, n); }

int dsir_t_topk(void* stream, const float* score, int clouds, int n, int k, int32_t* idx, float* score_out, void* scratch) {
  if (!score || !idx || !score_out || !scratch || clouds < 1 || n < 1 || k < 1 || k > n) return (int)hipErrorInvalidValue;
  if (int r = launch_topk(score, clouds, n, k, idx, score_out, scratch, (hipStream_t)stream)) return r;
  return done();
}

int dsir_t_sigmoid(void* stream, const float* x, int64_t n, float* y) {
  if (!x || !y || n < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(t_sigmoid_kernel, dim3(grid1(n)), dim3(256), 0, (hipStream_t)stream, x, n, y);
  return done();
}

int dsir_t_axpy(void* stream, float a, const float* x, int64_t n, float* y) {
  if (!x || !y || n < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(t_axpy_kernel, dim3(grid1(n)), dim3(256), 0, (hipStream_t)stream, a, x, n, y);
  return done();
}

int dsir_t_any_nan(void* stream, const float* x, int64_t n, int32_t* flag) {
  if (!x || !flag || n < 1) return (int)hipErrorInvalidValue;
  (void)hipMemsetAsync(flag, 0, sizeof(int32_t), (hipStream_t)stream);
  hipLaunchKernelGGL(t_any_nan_kernel, dim3(grid1(n)), dim3(256), 0, (hipStream_t)stream, x, n, flag);
  return done();
}

int dsir_t_adam(void* stream, float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps,
                int step) {
  if (!p || !g || !m || !v || n < 1 || step < 1) return (int)hipErrorInvalidValue;
  const double bc1 = 1.0 - pow((double)b1, step), bc2 = 1.0 - pow((double)b2, step);
  hipLaunchKernelGGL(t_adam_kernel, dim3(grid1(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, b1, b2, eps, (float)(lr / bc1),
                     (float)(1.0 / sqrt(bc2)));
  return done();
}

}  // extern "C"
