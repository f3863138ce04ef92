// RANSAC pose from correspondences (the third branch of DGR's pose stage, next to icp.hip and finetune.hip): the reference's
//   registration_ransac_based_on_correspondence   network/DGR.py:26-36
//   registration_ransac_based_on_feature_matching network/DGR.py:7-24     (DGR.safeguard_registration, :249-306)
// are open3d calls.  open3d cannot be imported here, so parity at this boundary is UNPINNED: the engine owns the rule, states it
// here once, and deepsir_amd/ransac.py restates it on the host for the tests.
//
// THE RULE.  Front (gather and park) and tail (scoring, pick and its tie-break, refit rounds, finish and the stats columns): the head
// of pose_corr.hip.  The middle, ransac_hyp_kernel, one lane per hypothesis h of H per pair p:
//   hypothesis h of H, sample of n in {3, 4} rows:   draw k:  d = splitmix64(splitmix64(seed ^ (p << 40)) ^ (h << 8) ^ k),
//       row_k = ((d >> 32) * count) >> 32.  Nothing else enters: the same (seed, p, h, k) is the same row in every batch, for every H
//       and launch geometry (pair p of a call with seed s is pair 0 of a call with seed s ^ (p << 40)).
//       Rejected: count < n, a repeated row, a parked row.
//   fit: unweighted Kabsch of the n pairs: centroids and covariance H[a][b] = sum (s_a - cs_a)(q_b - cq_b) as float64 sums of the fp32
//       coordinates in sample order, svd3.h, R = V diag(1, 1, d) U^T (the reflection fix of kabsch.hip), t = cq - R cs in float64;
//       T rounded to fp32 ONCE (fit_rows64, pose_corr.h).  A non-finite T is rejected.
//   checks: edge lengths (open3d CorrespondenceCheckerBasedOnEdgeLength): for every sample pair (i, j), in float64,
//       |s_i - s_j| >= edge_sim |q_i - q_j| and |q_i - q_j| >= edge_sim |s_i - s_j|   (edge_sim <= 0: no check);
//       distance: every sample member has d2 < thr^2 under T (pose_d2 and corr_thr2 of pose_corr.h: the tail's residual and threshold).
//   stats columns 2 and 3: the winning h or -1, the valid hypotheses.
// Three deliberate deviations from open3d: samples with a repeated row are rejected (open3d draws with replacement and lets the
// checkers sort it out); the tie-break is the count alone (open3d: lower RMSE - a float sum whose value depends on the order of
// addition; the refit makes the choice among equal counts irrelevant); no early exit on a confidence bound (every hypothesis is
// scored: H x M independent products are what the device is for, and the result does not depend on H for the hypotheses shared).
#include <cfloat>

#include "kernels.h"
#include "device_utils.h"
#include "pose_corr.h"
#include "dsir.h"

namespace dsir {

namespace {

constexpr int HB = 128;                 // hypotheses per fitting workgroup

// one lane per hypothesis: draw, gather, fit, check.  hyp_T [P][H][12], hyp_valid [P][H]; sample (optional) [P][H][4]
__global__ __launch_bounds__(HB) void ransac_hyp_kernel(const float* __restrict__ cs, const float* __restrict__ cq,
                                                        const int32_t* __restrict__ counts, int M, int H, int n, uint64_t seed,
                                                        float thr2, float edge_sim, float* __restrict__ hyp_T,
                                                        int32_t* __restrict__ hyp_valid, int32_t* __restrict__ sample) {
  const int pair = blockIdx.y;
  const int h = blockIdx.x * HB + threadIdx.x;
  if (h >= H) return;
  const int count = live_count(counts, pair, M);
  const uint64_t key = splitmix64(seed ^ ((uint64_t)pair << 40));
  int row[4] = {-1, -1, -1, -1};
  for (int k = 0; k < n; ++k) {
    const uint64_t d = splitmix64(key ^ ((uint64_t)h << 8) ^ (uint64_t)k);
    row[k] = (int)(((d >> 32) * (uint64_t)count) >> 32);
  }
  if (sample)
    for (int k = 0; k < 4; ++k) sample[((int64_t)pair * H + h) * 4 + k] = row[k];
  bool ok = count >= n;
  for (int a = 0; a < n; ++a)
    for (int b = a + 1; b < n; ++b) ok = ok && row[a] != row[b];
  float T[12];
  for (int k = 0; k < 12; ++k) T[k] = 0.f;
  if (ok) {
    float s[4][3], q[4][3];
    for (int k = 0; k < n; ++k) {
      const float* ps = cs + ((int64_t)pair * M + row[k]) * 3;
      const float* pq = cq + ((int64_t)pair * M + row[k]) * 3;
      for (int c = 0; c < 3; ++c) { s[k][c] = ps[c]; q[k][c] = pq[c]; }
      ok = ok && !parked(s[k], q[k]);
    }
    if (ok) {
      fit_rows64(n, [&](int k) { return s[k]; }, [&](int k) { return q[k]; }, T);
      for (int k = 0; k < 12; ++k) ok = ok && isfinite(T[k]);
      if (edge_sim > 0.f) {
        for (int a = 0; a < n; ++a)
          for (int b = a + 1; b < n; ++b) {
            double ls = 0.0, lq = 0.0;
            for (int c = 0; c < 3; ++c) {
              const double ds = (double)s[a][c] - (double)s[b][c], dq = (double)q[a][c] - (double)q[b][c];
              ls += ds * ds; lq += dq * dq;
            }
            ls = sqrt(ls); lq = sqrt(lq);
            ok = ok && ls >= (double)edge_sim * lq && lq >= (double)edge_sim * ls;
          }
      }
      for (int k = 0; k < n; ++k) ok = ok && pose_d2(T, s[k][0], s[k][1], s[k][2], q[k][0], q[k][1], q[k][2]) < thr2;
    }
  }
  float* o = hyp_T + ((int64_t)pair * H + h) * 12;
  for (int k = 0; k < 12; ++k) o[k] = T[k];
  hyp_valid[(int64_t)pair * H + h] = ok ? 1 : 0;
}

}  // namespace

size_t ransac_scratch_bytes(int pairs, int M, int H, int refine_iters) { return RansacLayout(pairs, M, H, refine_iters).bytes; }

int launch_ransac(const RansacArgs& a, void* scratch, hipStream_t st) {
  const CorrProblem& p = a.p;
  const int P = p.pairs, M = p.M, H = a.hypotheses;
  if (!pose_corr_shape_ok(P, M)) return 1;
  const RansacLayout lay(P, M, H, p.refine_iters);
  const PoseParts s(scratch, lay.pose);
  const CandSet hyp(scratch, lay.hyp, H);

  launch_pose_front(p, s, st);
  hipLaunchKernelGGL(ransac_hyp_kernel, dim3((H + HB - 1) / HB, P), dim3(HB), 0, st, s.cs, s.cq, p.counts, M, H, a.n, a.seed, corr_thr2(p),
                     a.edge_sim, hyp.T, hyp.valid, a.diag_sample);
  launch_pose_tail(p, s, hyp, st);
  copy_candidates(hyp, P, a.diag_T, a.diag_valid, a.diag_count, st);
  return 0;
}

}  // namespace dsir
