// Pose from a correspondence list: what ransac.hip, consensus.hip and fgr.hip share.  Each of them is a MIDDLE - it turns the
// gathered points into candidate poses - between one front and one tail; front, tail and their rule live in pose_corr.hip.  Here: the
// problem all three are handed, the candidates they hand on, the scratch head, and the device helpers for the gathered points.
#pragma once
#include <cfloat>
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "device_utils.h"
#include "op_layouts.h"
#include "svd3.h"

namespace dsir {

// the arguments every dsir_*_correspondence entry takes
struct CorrProblem {
  const float* src; const float* ref;   // [pairs][J][stride], [pairs][K][stride], xyz first
  int pairs, J, K, stride;
  const int32_t* corr;                  // [pairs][M][2] (src index, ref index)
  const int32_t* counts;                // [pairs] or nullptr (M)
  int M;
  float max_dist; int refine_iters;
  const float* T_init;                  // [pairs][3][4] or nullptr (identity)
  float* T_out; double* stats; int32_t* invalid;   // [pairs][3][4], [pairs][5], [pairs]
};

// the inlier threshold of every stage: an fp32 product (the build keeps contraction off)
inline float corr_thr2(const CorrProblem& p) { return p.max_dist * p.max_dist; }

// H candidate poses per pair: T [P][H][12], valid [P][H], count [P][H] (the tail's inlier counts)
struct CandSet {
  float* T; int32_t* valid; int32_t* count; int H;
  CandSet(void* scratch, const CandLayout& l, int H_) : T(at<float>(scratch, l.T)), valid(at<int32_t>(scratch, l.valid)),
                                                        count(at<int32_t>(scratch, l.count)), H(H_) {}
};

// the parts of PoseLayout (op_layouts.h: the head of every stage's scratch) as pointers
struct PoseParts {
  float *cs, *cq, *w, *Tcand;
  int32_t *cnt, *info;
  PoseParts(void* scratch, const PoseLayout& l)
      : cs(at<float>(scratch, l.cs)), cq(at<float>(scratch, l.cq)), w(at<float>(scratch, l.w)), Tcand(at<float>(scratch, l.Tcand)),
        cnt(at<int32_t>(scratch, l.cnt)), info(at<int32_t>(scratch, l.info)) {}
};

// front: invalid zeroed, then clamp, flag (bit 2 of invalid), gather into s.cs / s.cq, park
void launch_pose_front(const CorrProblem& p, const PoseParts& s, hipStream_t st);
// tail: the candidates' inlier counts (c.count, zeroed here), the pick, p.refine_iters refit rounds, T_out and stats
void launch_pose_tail(const CorrProblem& p, const PoseParts& s, const CandSet& c, hipStream_t st);
// the optional diagnostic copies of a candidate set, after the tail (nullptr: not wanted)
void copy_candidates(const CandSet& c, int pairs, float* T, int32_t* valid, int32_t* count, hipStream_t st);

// The three middles: the problem, the middle's own parameters, its optional diagnostics.  All pairs at once; 0 on success.
struct RansacArgs {          // ransac.hip (network/DGR.py:7-36, :249-306 / open3d registration_ransac_*)
  CorrProblem p;
  int n; float edge_sim; int hypotheses; uint64_t seed;
  int32_t* diag_sample; float* diag_T; int32_t* diag_valid; int32_t* diag_count;
};
size_t ransac_scratch_bytes(int pairs, int M, int H, int refine_iters);
int launch_ransac(const RansacArgs& a, void* scratch, hipStream_t st);

struct ConsensusArgs {       // consensus.hip (second-order spatial compatibility)
  CorrProblem p;
  float compat_dist; int seeds, members;
  uint64_t* diag_bits; int32_t* diag_score; int32_t* diag_seed; int32_t* diag_members;
  float* diag_T; int32_t* diag_valid; int32_t* diag_count;
};
size_t consensus_scratch_bytes(int pairs, int M, int seeds, int refine_iters);
int launch_consensus(const ConsensusArgs& a, void* scratch, hipStream_t st);

struct FgrArgs {             // fgr.hip (tuple pre-filter, graduated Gauss-Newton); shape limits: fgr_shape_ok (fgr.h)
  CorrProblem p;
  int tuple_test; float ts2; int max_tuples, max_trials, iterations; float division_factor; uint64_t seed;
  int32_t* diag_rows; int32_t* diag_n_rows; int32_t* diag_trials; double* diag_norm;
  double* diag_iter_T; double* diag_iter_mu; double* diag_iter_energy; int32_t* diag_iters_run;
};
size_t fgr_scratch_bytes(int pairs, int M, int tuple_test, int max_tuples, int max_trials, int refine_iters);
int launch_fgr(const FgrArgs& a, void* scratch, hipStream_t st);

__device__ __forceinline__ int live_count(const int32_t* counts, int pair, int M) {
  return counts ? max(0, min(counts[pair], M)) : M;
}

__device__ __forceinline__ bool parked(const float* s, const float* q) {
  return q[0] == FLT_MAX && q[1] == FLT_MAX && q[2] == FLT_MAX && s[0] == 0.f && s[1] == 0.f && s[2] == 0.f;
}

// squared residual of one correspondence under T: THE fp32 rounding sequence of the rule (checks, scores, weights and stats share it)
__device__ __forceinline__ float pose_d2(const float* T, float sx, float sy, float sz, float qx, float qy, float qz) {
  const float dx = __fsub_rn(se3_row(T, 0, sx, sy, sz), qx);
  const float dy = __fsub_rn(se3_row(T, 1, sx, sy, sz), qy);
  const float dz = __fsub_rn(se3_row(T, 2, sx, sy, sz), qz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
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

}  // namespace dsir
