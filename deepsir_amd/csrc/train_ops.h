// What the training-operator files share (train_gemm.hip, train_norm.hip, train_gather.hip, train_loss.hip, train_elem.hip): the
// plans and scratch layouts (train_layouts.h, with the GEMM tile TB / TK), the 1-D grid rule, the launch status, and the launcher
// of the forward GEMM, which the detection loss calls as well.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "train_layouts.h"

namespace dsir {

inline unsigned grid1(int64_t n) { const int64_t g = (n + 255) / 256; return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g)); }
inline int done() { return (int)hipGetLastError(); }

// train_gemm.hip, t_gemm_kernel on its grid: Y[r][n] = beta Y[r][n] + bias[n] + sum_k X[r][k] W[n wn + k wk]
void launch_t_gemm(hipStream_t st, const float* X, int ldx, const float* W, int wn, int wk, const float* bias, float* Y, int ldy,
                   int64_t rows, int K, int N, float beta);

}  // namespace dsir
