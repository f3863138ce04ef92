// Training operators (include/dsir_train.h): forward-with-saved-activations and backward of the ATen calls RandLA.forward
// makes (reference network/RandLANet.py:140-230, :311-408), point-major fp32.  The inference engine (schedule.hip) fuses and
// never materialises most of these tensors; a training step needs them all, so this path is layer by layer: one
// exact-fp32 MFMA GEMM for every 1x1 convolution (forward, d input, d weight), and row-streaming kernels around it
// (train_norm.hip, train_gather.hip, train_loss.hip, train_elem.hip).
// This file: the GEMMs - t_gemm_kernel behind dsir_t_gemm and launch_t_gemm, the split weight-gradient GEMM and its reduction.
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

constexpr int TLD = TK + 2;   // LDS row (floats): fragment reads (row r, k = 4 s + q) hit banks 2 r + q

// Y[r][n] = beta Y[r][n] + bias[n] + sum_k X[r][k] W[n wn + k wk]; block = 4 waves, wave w owns rows 16 w .. 16 w + 15
__global__ __launch_bounds__(256) void t_gemm_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ W, int wn, int wk,
                                                     const float* __restrict__ bias, float* __restrict__ Y, int ldy, int64_t rows,
                                                     int K, int N, float beta) {
  __shared__ float Xs[2][TB * TLD];
  __shared__ float Ws[2][TB * TLD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * TB;
  const int n0 = blockIdx.y * TB;
  const int sr = tid >> 2, sk = (tid & 3) * 4;          // staging: row / column sr, four consecutive k
  const int64_t xr = m0 + sr;
  const int wc = n0 + sr;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  // rows of X (and of W when it is k-contiguous) are read as one 16-byte load per thread where alignment allows
  const bool xv = (ldx & 3) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
  const bool wv = wk == 1 && (wn & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;
  // the next K chunk is fetched into registers while the MFMAs of the current one run, then written to the other LDS buffer:
  // one barrier per chunk and no exposed load latency (round 3; the deep layers - 40 workgroups, K = 512 - were a chain of 32
  // fetch -> barrier -> 4 MFMAs -> barrier steps, 43 us)
  float xq[4], wq[4];
  auto gload = [&](int k0) {
    const int kb = k0 + sk;
    if (xv && xr < rows && kb + 3 < K) {
      const float4 v = *reinterpret_cast<const float4*>(X + xr * ldx + kb);
      xq[0] = v.x; xq[1] = v.y; xq[2] = v.z; xq[3] = v.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) xq[u] = (xr < rows && kb + u < K) ? X[xr * ldx + kb + u] : 0.f;
    }
    if (wv && wc < N && kb + 3 < K) {
      const float4 v = *reinterpret_cast<const float4*>(W + (int64_t)wc * wn + kb);
      wq[0] = v.x; wq[1] = v.y; wq[2] = v.z; wq[3] = v.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) wq[u] = (wc < N && kb + u < K) ? W[(int64_t)wc * wn + (int64_t)(kb + u) * wk] : 0.f;
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 4; ++u) { Xs[buf][sr * TLD + sk + u] = xq[u]; Ws[buf][sr * TLD + sk + u] = wq[u]; }
  };
  gload(0);
  sstore(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = 0; k0 < K; k0 += TK) {
    const bool more = k0 + TK < K;
    if (more) gload(k0 + TK);
#pragma unroll
    for (int s = 0; s < TK / 4; ++s) {
      const float a = Xs[buf][(16 * w + fr) * TLD + 4 * s + fq];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Ws[buf][(16 * t + fr) * TLD + 4 * s + fq], acc[t], 0, 0, 0);
    }
    if (more) sstore(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int n = n0 + 16 * t + fr;
    if (n >= N) continue;
    const float bv = bias ? bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = m0 + 16 * w + 4 * fq + r;
      if (row < rows) {
        float v = acc[t][r] + bv;
        if (beta != 0.f) v += beta * Y[row * ldy + n];
        Y[row * ldy + n] = v;
      }
    }
  }
}

// partial[split][n][k'] = sum over the split's rows of dY[r][n] X'[r][k'], X' = [X, 1] when the bias column is wanted
constexpr int DLD = TB + 16;   // LDS row of the transposed-use tiles: (k-row q, column fr) -> banks 16 q + fr
__global__ __launch_bounds__(256) void t_gemm_dw_kernel(const float* __restrict__ dY, int ldy, const float* __restrict__ X, int ldx,
                                                        int64_t rows, int64_t rows_per_split, int N, int K, int Kp,
                                                        float* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float As[2][TK * DLD];
  __shared__ __attribute__((aligned(16))) float Bs[2][TK * DLD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int n0 = blockIdx.x * TB, k0 = blockIdx.y * TB;
  const int64_t r_begin = (int64_t)blockIdx.z * rows_per_split;
  const int64_t r_end = min(rows, r_begin + rows_per_split);
  const int sr = tid >> 4, sc = (tid & 15) * 4;         // staging: row sr of the chunk, four consecutive columns
  const bool av = (ldy & 3) == 0 && (reinterpret_cast<uintptr_t>(dY) & 15) == 0;
  const bool bv = (ldx & 3) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  // as in t_gemm_kernel: the next 16-row chunk travels to registers during the MFMAs of the current one; one barrier per chunk
  float4 aq, bq;
  auto gload = [&](int64_t r0) {
    const int64_t r = r0 + sr;
    const bool rin = r < r_end;
    if (av && rin && n0 + sc + 3 < N) {
      aq = *reinterpret_cast<const float4*>(dY + r * ldy + n0 + sc);
    } else {
      float t[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) t[u] = (rin && n0 + sc + u < N) ? dY[r * ldy + n0 + sc + u] : 0.f;
      aq = make_float4(t[0], t[1], t[2], t[3]);
    }
    if (bv && rin && k0 + sc + 3 < K) {
      bq = *reinterpret_cast<const float4*>(X + r * ldx + k0 + sc);
    } else {
      float t[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = k0 + sc + u;
        t[u] = !rin ? 0.f : (k < K ? X[r * ldx + k] : (k == K && Kp > K ? 1.f : 0.f));
      }
      bq = make_float4(t[0], t[1], t[2], t[3]);
    }
  };
  auto sstore = [&](int buf) {
    *reinterpret_cast<float4*>(&As[buf][sr * DLD + sc]) = aq;
    *reinterpret_cast<float4*>(&Bs[buf][sr * DLD + sc]) = bq;
  };
  int buf = 0;
  if (r_begin < r_end) {
    gload(r_begin);
    sstore(0);
  }
  __syncthreads();
  for (int64_t r0 = r_begin; r0 < r_end; r0 += TK) {
    const bool more = r0 + TK < r_end;
    if (more) gload(r0 + TK);
#pragma unroll
    for (int s = 0; s < TK / 4; ++s) {
      const float a = As[buf][(4 * s + fq) * DLD + 16 * w + fr];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[buf][(4 * s + fq) * DLD + 16 * t + fr], acc[t], 0, 0, 0);
    }
    if (more) sstore(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
  float* P = partial + (int64_t)blockIdx.z * N * Kp;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int k = k0 + 16 * t + fr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + 16 * w + 4 * fq + r;
      if (n < N && k < Kp) P[(int64_t)n * Kp + k] = acc[t][r];
    }
  }
}

// block = 32 consecutive elements x 8 split lanes: lane (el, sl) adds the splits sl, sl + 8, ... of its element in order - a wave reads
// two 128-byte runs per trip instead of 64 scattered floats -, then the 8 lanes of an element meet in LDS in a fixed order
// (deterministic)
__global__ __launch_bounds__(256) void t_gemm_dw_reduce_kernel(const float* __restrict__ partial, int splits, int N, int K, int Kp,
                                                               float* __restrict__ dW, float* __restrict__ db) {
  __shared__ float sh[8][32];
  const int el = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int64_t e = (int64_t)blockIdx.x * 32 + el;
  const int64_t total = (int64_t)N * Kp;
  float s = 0.f;
  if (e < total) {
#pragma unroll 4
    for (int i = sl; i < splits; i += 8) s += partial[(int64_t)i * total + e];
  }
  sh[sl][el] = s;
  __syncthreads();
  if (sl != 0 || e >= total) return;
  float a = sh[0][el];
#pragma unroll
  for (int q = 1; q < 8; ++q) a += sh[q][el];
  const int n = (int)(e / Kp), k = (int)(e % Kp);
  if (k < K) dW[(int64_t)n * K + k] += a;
  else if (db) db[n] += a;
}

}  // namespace

void launch_t_gemm(hipStream_t st, const float* X, int ldx, const float* W, int wn, int wk, const float* bias, float* Y, int ldy,
                   int64_t rows, int K, int N, float beta) {
  const dim3 grid((unsigned)((rows + TB - 1) / TB), (unsigned)((N + TB - 1) / TB));
  hipLaunchKernelGGL(t_gemm_kernel, grid, dim3(256), 0, st, X, ldx, W, wn, wk, bias, Y, ldy, rows, K, N, beta);
}

}  // namespace dsir

using namespace dsir;

extern "C" {

int dsir_t_gemm(void* stream, const float* X, int ldx, const float* W, int wn, int wk, const float* bias, float* Y, int ldy,
                int64_t rows, int K, int N, float beta) {
  if (!X || !W || !Y || rows < 1 || K < 1 || N < 1) return (int)hipErrorInvalidValue;
  launch_t_gemm((hipStream_t)stream, X, ldx, W, wn, wk, bias, Y, ldy, rows, K, N, beta);
  return done();
}

size_t dsir_t_gemm_dw_scratch(int64_t rows, int N, int K) { return DwLayout(rows, N, K).bytes; }

int dsir_t_gemm_dw(void* stream, const float* dY, int ldy, const float* X, int ldx, int64_t rows, int N, int K, float* dW, float* db,
                   void* scratch) {
  if (!dY || !X || !dW || !scratch || rows < 1 || K < 1 || N < 1) return (int)hipErrorInvalidValue;
  const DwPlan p = dw_plan(rows, N, K, db != nullptr);
  float* partial = at<float>(scratch, DwLayout(rows, N, K).partial);
  const dim3 grid((unsigned)((N + TB - 1) / TB), (unsigned)((p.Kp + TB - 1) / TB), (unsigned)p.splits);
  hipLaunchKernelGGL(t_gemm_dw_kernel, grid, dim3(256), 0, (hipStream_t)stream, dY, ldy, X, ldx, rows, p.rows_per_split, N, K, p.Kp,
                     partial);
  hipLaunchKernelGGL(t_gemm_dw_reduce_kernel, dim3((unsigned)(((int64_t)N * p.Kp + 31) / 32)), dim3(256), 0, (hipStream_t)stream, partial, p.splits, N, K,
                     p.Kp, dW, db);
  return done();
}

}  // extern "C"
