// The stages of ransac.hip that consensus.hip runs as well (the rule of each is stated in ransac.hip's header): the gather of
// the matched points, the float64 fit of a handful of rows, and everything after the candidate poses exist - scoring, pick, refit
// rounds, finish.  The kernels stay file-local to ransac.hip; these are their launchers and the two device helpers both files share.
#pragma once
#include <cfloat>
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "op_layouts.h"
#include "svd3.h"

namespace dsir {

__device__ __forceinline__ int live_count(const int32_t* counts, int pair, int M) {
  return counts ? max(0, min(counts[pair], M)) : M;
}

__device__ __forceinline__ bool parked(const float* s, const float* q) {
  return q[0] == FLT_MAX && q[1] == FLT_MAX && q[2] == FLT_MAX && s[0] == 0.f && s[1] == 0.f && s[2] == 0.f;
}

// Unweighted Kabsch of n matched rows, row k at ps(k) / pq(k) (three fp32 each): centroids and covariance as float64 sums in row
// order, svd3.h, the reflection fix, t = cq - R cs in float64, T rounded to fp32 once.
template <class PS, class PQ>
__device__ inline void fit_rows64(int n, PS ps, PQ pq, float* T) {
  double ms[3] = {0, 0, 0}, mq[3] = {0, 0, 0};
  for (int k = 0; k < n; ++k)
    for (int c = 0; c < 3; ++c) { ms[c] += (double)ps(k)[c]; mq[c] += (double)pq(k)[c]; }
  for (int c = 0; c < 3; ++c) { ms[c] /= (double)n; mq[c] /= (double)n; }
  double Hm[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int k = 0; k < n; ++k)
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) Hm[a][b] += ((double)ps(k)[a] - ms[a]) * ((double)pq(k)[b] - mq[b]);
  double U[3][3], S[3], V[3][3], R[3][3];
  svd3(Hm, U, S, V);
  procrustes_rotation(U, V, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[r * 4 + c] = (float)R[r][c];
    T[r * 4 + 3] = (float)(mq[r] - ((R[r][0] * ms[0] + R[r][1] * ms[1]) + R[r][2] * ms[2]));
  }
}

// the parts of PoseLayout (op_layouts.h: the head of both pose stages' scratch) as the pointers the launchers below read
struct PoseParts {
  float *cs, *cq, *w, *Tcand;
  int32_t *cnt, *info;
  PoseParts(void* scratch, const PoseLayout& l)
      : cs(at<float>(scratch, l.cs)), cq(at<float>(scratch, l.cq)), w(at<float>(scratch, l.w)), Tcand(at<float>(scratch, l.Tcand)),
        cnt(at<int32_t>(scratch, l.cnt)), info(at<int32_t>(scratch, l.info)) {}
};

// clamp, flag (bit 2 of invalid, zeroed here), gather, park
void launch_ransac_gather(const float* src, const float* ref, int pairs, int J, int K, int stride, const int32_t* corr,
                          const int32_t* counts, int M, const PoseParts& s, int32_t* invalid, hipStream_t st);
// H candidate poses per pair (hyp_T [P][H][12], hyp_valid [P][H]) -> their inlier counts (hyp_count [P][H], zeroed here), the pick
// (largest count, ties to the lower h), R refit rounds, T_out and stats
void launch_ransac_tail(const PoseParts& s, const int32_t* counts, int pairs, int M, const float* hyp_T, const int32_t* hyp_valid,
                        int32_t* hyp_count, int H, int R, float thr2, const float* T_init, float* T_out, double* stats, hipStream_t st);

}  // namespace dsir
