// Fast global registration pose from correspondences: the fifth pose stage, beside ransac.hip, consensus.hip, icp.hip and
// finetune.hip (FGR: Zhou, Park, Koltun, ECCV 2016; open3d registration_fgr_based_on_feature_matching).  open3d cannot be imported
// here, so parity is UNPINNED: the engine owns the rule, states it here once, and deepsir_amd/fgr.py restates it on the host for
// the tests.  No hypotheses and no quadratic memory: a tuple pre-filter, then a few dozen 6 x 6 Gauss-Newton steps under a graduated
// robust weight - O(rows x iterations) per pair.
//
// THE RULE.  Front (step 1) and tail (step 6) are those of every pose-from-correspondences stage: the head of pose_corr.hip states
// them.  Per pair p:
//   1 gather: the shared front: clamp with bit 2 of invalid, park non-finite rows and rows >= count at s = 0, q = FLT_MAX.  A parked
//     row enters nothing below.
//   2 tuple test (tuple_test != 0): trial t of min(100 count, max_trials) draws three rows with RANSAC's key scheme, a trial in the
//     place of a hypothesis:  row_k = ((splitmix64(splitmix64(seed ^ (p << 40)) ^ (t << 8) ^ k) >> 32) * count) >> 32,  k = 0, 1, 2.
//     It is accepted iff for each of the edges (0,1), (0,2), (1,2):  d2s ts2 < d2q  and  d2q ts2 < d2s,  all in fp32 with every
//     operation rounded on its own: d = a - b per coordinate, d2 = (dx dx + dy dy) + dz dz on the gathered points, ts2 =
//     fp32(tuple_scale^2) rounded once on the host.  Equal rows (0 < 0), parked rows (d2q = 0 or +inf) and NaNs fail by themselves.
//     The row list is the three rows of each of the FIRST max_tuples accepted trials in trial order, duplicates kept: a
//     correspondence that sits in many tuples weighs more.  tuple_test == 0: the list is every live row that is not parked, ascending.
//     Fewer than 3 listed rows: no pose.
//   3 normalise, float64: ms, mq = the means of the listed rows' points (duplicates count); scale = the largest distance of a listed
//     point from its own side's mean, sqrt((dx dx + dy dy) + dz dz); scale == 0 or not finite: no pose.
//     s^ = (s - ms) / scale, q^ = (q - mq) / scale.
//   4 optimise, float64, every operation rounded on its own: T = I, mu = 1, floor = (max_dist / scale)^2; for it = 0 .. iterations - 1:
//       per listed row  u_c = ((T_c0 s^_0 + T_c1 s^_1) + T_c2 s^_2) + T_c3,  r = q^ - u,  rr = (r_0 r_0 + r_1 r_1) + r_2 r_2,
//       w = mu / (mu + rr),  l = w w;  for c = 0, 1, 2 with c1 = (c + 1) % 3, c2 = (c + 2) % 3 the Jacobian row J_c has
//       J_c[c1] = -u[c2], J_c[c2] = u[c1], J_c[3 + c] = -1, zeros elsewhere;
//       A += l J_c J_c^T (the 21 sums of icp_plane_tri), b += l J_c r_c, energy += l rr + mu (1 - sqrt(l))^2, rows += 1;
//       x = icp_plane_solve(A, b, rows) (icp_plane.h, as it is).  A refusal ends the loop, keeps T and is recorded;
//       T <- M(x) T with icp_plane_transform (Rz Ry Rx, translation x_3..5);
//       if division_factor > 1 and it % 4 == 0 and mu > floor: mu <- mu / division_factor.
//   5 un-normalise, float64: R = T_R, t = scale T_t + mq - R ms; rounded to fp32 once.  A non-finite pose is no pose.
//   6 tail: that pose is the single candidate (H = 1) of the shared tail (launch_pose_tail): inlier count under max_dist, refine_iters
//     refits on all inliers, T_out and stats {fitness, inlier RMSE, 0 or -1, 1 or 0, inliers}.  No pose: T_out = T_init (identity if
//     NULL), stats {0, 0, -1, 0, 0} - not an error.
// Where the rule leaves open3d's: open3d normalises the two whole clouds (here the listed correspondences alone: the stage reads
// nothing but its correspondence list, like its siblings); open3d draws tuples with rand() and keeps at most max_tuples of them as
// they come (here: keyed draws, first max_tuples in trial order); open3d compares edge LENGTHS with tuple_scale (here squared
// lengths with tuple_scale^2: no square root, the same verdict up to rounding); open3d solves with a plain LDL^T and no singularity
// test; open3d returns the optimised pose (here it goes through the siblings' scoring and refit tail).
//
// KERNELS.
//   fgr_select_kernel<TUPLE, FILL>: count -> hipCUB exclusive scan -> fill, over blocks of kFgrBlock trials across the whole grid
//     (the shape of dsir_t_radius_matches_count / _fill).  Every trial is evaluated in both passes; the count pass leaves one number
//     per block, the scan turns them into the block's first position, the fill pass ranks the accepted trials inside the block by
//     ballot + prefix and writes those below the cap.  No atomics: the same bytes on every run, and "the first max_tuples accepted in
//     trial order" whatever the grid.
//   fgr_optimize_kernel: one workgroup of kFgrBlock threads per pair through steps 3 - 5, no host round trip.  Thread i takes rows
//     i, i + kFgrBlock, ...; 29 float64 sums per thread go through the wave butterfly and then the waves in ascending order in LDS
//     (block_sum of device_utils.h): the order of every addition is a function of the row count alone.  One lane solves and composes.
//     The normalised points are written once to scratch as float64 (48 bytes a row; each thread reads back only what it wrote) and
//     stream from L2 every iteration: at the default 3000 rows that is 144 KB per pair, which no LDS holds in float64, and the fp32
//     originals in LDS (72 KB) would pay two subtractions and two divisions per coordinate per iteration instead.
#include <cfloat>
#include <hipcub/hipcub.hpp>

#include "kernels.h"
#include "device_utils.h"
#include "pose_corr.h"
#include "fgr.h"
#include "dsir.h"

namespace dsir {

namespace {

constexpr int FB = kFgrBlock;
constexpr int FW = FB / 64;

__device__ __forceinline__ float fgr_d2(const float* a, const float* b) {
  const float dx = __fsub_rn(a[0], b[0]), dy = __fsub_rn(a[1], b[1]), dz = __fsub_rn(a[2], b[2]);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// candidate t of a pair: its rows and its verdict.  S, Q: the pair's gathered points [M][3]
template <bool TUPLE>
__device__ __forceinline__ bool fgr_candidate(const float* __restrict__ S, const float* __restrict__ Q, int count, uint64_t key, int t,
                                              float ts2, int (&row)[3]) {
  if (!TUPLE) {
    row[0] = t; row[1] = -1; row[2] = -1;
    if (t >= count) return false;
    return !parked(S + (int64_t)t * 3, Q + (int64_t)t * 3);
  }
  float s[3][3], q[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    row[k] = fgr_trial_row(key, t, k, count);                   // < count <= M
#pragma unroll
    for (int c = 0; c < 3; ++c) { s[k][c] = S[(int64_t)row[k] * 3 + c]; q[k][c] = Q[(int64_t)row[k] * 3 + c]; }
  }
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = a + 1; b < 3; ++b) {
      const float d2s = fgr_d2(s[a], s[b]), d2q = fgr_d2(q[a], q[b]);
      ok = ok && __fmul_rn(d2s, ts2) < d2q && __fmul_rn(d2q, ts2) < d2s;
    }
  return ok;
}

// grid (blocks of FB candidates, pairs).  !FILL: blk_cnt [P][NB] = accepted candidates of the block.  FILL: blk_pre = the exclusive
// prefix of blk_cnt over the whole [P x NB] array; rows [P][L] (preset to -1) receive the rows of the accepted candidates whose rank
// in the pair is below cap.
template <bool TUPLE, bool FILL>
__global__ __launch_bounds__(FB) void fgr_select_kernel(const float* __restrict__ cs, const float* __restrict__ cq,
                                                        const int32_t* __restrict__ counts, int M, int max_trials, uint64_t seed, float ts2,
                                                        int NB, int cap, int64_t L, int32_t* __restrict__ blk_cnt,
                                                        const int32_t* __restrict__ blk_pre, int32_t* __restrict__ rows) {
  __shared__ int wt[FW];
  const int pair = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int count = live_count(counts, pair, M);
  const int n = TUPLE ? fgr_trials(count, max_trials) : count;
  const int t = blockIdx.x * FB + tid;
  int base = 0;
  if (FILL) {
    base = blk_pre[(int64_t)pair * NB + blockIdx.x] - blk_pre[(int64_t)pair * NB];
    if (base >= cap) return;                                    // block-uniform
  }
  int row[3] = {-1, -1, -1};
  bool ok = false;
  if (t < n)
    ok = fgr_candidate<TUPLE>(cs + (int64_t)pair * M * 3, cq + (int64_t)pair * M * 3, count, fgr_pair_key(seed, pair), t, ts2, row);
  const unsigned long long bal = __ballot(ok);
  if (lane == 0) wt[wave] = __popcll(bal);
  __syncthreads();
  if (!FILL) {
    if (tid == 0) {
      int c = 0;
      for (int w = 0; w < FW; ++w) c += wt[w];
      blk_cnt[(int64_t)pair * NB + blockIdx.x] = c;
    }
    return;
  }
  int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) pos += wt[w];
  if (ok && pos < cap) {
    constexpr int per = TUPLE ? 3 : 1;
    int32_t* o = rows + (int64_t)pair * L + (int64_t)pos * per;  // pos < cap: per x pos + per <= L
#pragma unroll
    for (int k = 0; k < per; ++k) o[k] = row[k];
  }
}

struct FgrDiagPtrs {
  int32_t *n_rows, *trials, *iters_run;
  double *norm, *iter_T, *iter_mu, *iter_energy;
};

__device__ __forceinline__ double wave_max64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// One workgroup per pair: steps 3 - 5 of the rule.  rows [P][L]; npts [P][L][6] float64 scratch; hyp_T [P][12], hyp_valid [P].
__global__ __launch_bounds__(FB) void fgr_optimize_kernel(const float* __restrict__ cs, const float* __restrict__ cq,
                                                          const int32_t* __restrict__ counts, int M, const int32_t* __restrict__ rows,
                                                          int64_t L, const int32_t* __restrict__ blk_cnt,
                                                          const int32_t* __restrict__ blk_pre, int NB, int tuple_test, int max_tuples,
                                                          int max_trials, double max_dist, int iterations, double division_factor,
                                                          double* __restrict__ npts, float* __restrict__ hyp_T,
                                                          int32_t* __restrict__ hyp_valid, FgrDiagPtrs dg) {
  __shared__ double sh[FW * kFgrSums + kFgrSums];
  __shared__ double sT[12];
  __shared__ double s_mu;
  __shared__ int s_stop;
  const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* S = cs + (int64_t)pair * M * 3;
  const float* Q = cq + (int64_t)pair * M * 3;
  const int32_t* R = rows + (int64_t)pair * L;
  double* N = npts + (int64_t)pair * L * 6;
  const int64_t last = (int64_t)pair * NB + NB - 1;
  const int64_t accepted = (int64_t)blk_pre[last] + blk_cnt[last] - blk_pre[(int64_t)pair * NB];
  const int n = (int)fgr_n_rows(tuple_test, M, max_tuples, accepted);    // <= L

  // diag rows of iterations that do not run are zero
  if (dg.iter_T)
    for (int k = tid; k < iterations * 12; k += FB) dg.iter_T[(int64_t)pair * iterations * 12 + k] = 0.0;
  if (dg.iter_mu)
    for (int k = tid; k < iterations; k += FB) dg.iter_mu[(int64_t)pair * iterations + k] = 0.0;
  if (dg.iter_energy)
    for (int k = tid; k < iterations; k += FB) dg.iter_energy[(int64_t)pair * iterations + k] = 0.0;
  if (tid == 0) {
    if (dg.n_rows) dg.n_rows[pair] = n;
    if (dg.trials) dg.trials[pair] = tuple_test ? fgr_trials(live_count(counts, pair, M), max_trials) : 0;
  }

  // 3 normalise
  double ms[3] = {0, 0, 0}, mq[3] = {0, 0, 0}, scale = 0.0;
  bool pose = n >= 3;                                           // block-uniform throughout
  if (pose) {
    double v[6] = {0, 0, 0, 0, 0, 0};
    for (int i = tid; i < n; i += FB) {
      const int r = R[i];
#pragma unroll
      for (int c = 0; c < 3; ++c) { v[c] += (double)S[(int64_t)r * 3 + c]; v[3 + c] += (double)Q[(int64_t)r * 3 + c]; }
    }
    block_sum<FW>(v, sh);
#pragma unroll
    for (int c = 0; c < 3; ++c) { ms[c] = v[c] / (double)n; mq[c] = v[3 + c] / (double)n; }
    double far2 = 0.0;
    for (int i = tid; i < n; i += FB) {
      const int r = R[i];
      double ds[3], dq[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) { ds[c] = (double)S[(int64_t)r * 3 + c] - ms[c]; dq[c] = (double)Q[(int64_t)r * 3 + c] - mq[c]; }
      far2 = fmax(far2, fmax((ds[0] * ds[0] + ds[1] * ds[1]) + ds[2] * ds[2], (dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2]));
    }
    far2 = wave_max64(far2);
    __syncthreads();                                            // block_sum's reads of sh are done
    if (lane == 0) sh[wave] = far2;
    __syncthreads();
    far2 = sh[0];
    for (int w = 1; w < FW; ++w) far2 = fmax(far2, sh[w]);
    scale = sqrt(far2);
    pose = scale > 0.0 && scale <= DBL_MAX;
    __syncthreads();                                            // sh is free again
  }
  if (dg.norm && tid == 0) {
    double* o = dg.norm + (int64_t)pair * 8;
    for (int c = 0; c < 3; ++c) { o[c] = ms[c]; o[3 + c] = mq[c]; }
    o[6] = scale; o[7] = 0.0;
  }
  int iters_run = 0;
  if (pose) {
    for (int i = tid; i < n; i += FB) {                         // thread i reads back below only what it writes here
      const int r = R[i];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        N[(int64_t)i * 6 + c] = ((double)S[(int64_t)r * 3 + c] - ms[c]) / scale;
        N[(int64_t)i * 6 + 3 + c] = ((double)Q[(int64_t)r * 3 + c] - mq[c]) / scale;
      }
    }
    // 4 optimise
    if (tid == 0) {
      for (int k = 0; k < 12; ++k) sT[k] = (k == 0 || k == 5 || k == 10) ? 1.0 : 0.0;
      s_mu = 1.0; s_stop = 0;
    }
    __syncthreads();
    const double floor_mu = (max_dist / scale) * (max_dist / scale);
    for (int it = 0; it < iterations; ++it) {
      double T[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) T[k] = sT[k];
      const double mu = s_mu;
      double v[kFgrSums];
#pragma unroll
      for (int k = 0; k < kFgrSums; ++k) v[k] = 0.0;
      for (int i = tid; i < n; i += FB) {
        const double* p = N + (int64_t)i * 6;
        const double s0 = p[0], s1 = p[1], s2 = p[2];
        double u[3], r[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          u[c] = ((T[c * 4] * s0 + T[c * 4 + 1] * s1) + T[c * 4 + 2] * s2) + T[c * 4 + 3];
          r[c] = p[3 + c] - u[c];
        }
        const double rr = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
        const double w = mu / (mu + rr), l = w * w;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
          double J[6] = {0, 0, 0, 0, 0, 0};
          J[c1] = -u[c2]; J[c2] = u[c1]; J[3 + c] = -1.0;
#pragma unroll
          for (int a = 0; a < 6; ++a) {                           // the structural zeros of J_c add nothing: skipped at compile time
            if (a != c1 && a != c2 && a != 3 + c) continue;
#pragma unroll
            for (int b = a; b < 6; ++b)
              if (b == c1 || b == c2 || b == 3 + c) v[icp_plane_tri(a, b)] += l * J[a] * J[b];
            v[21 + a] += l * J[a] * r[c];
          }
        }
        const double e = 1.0 - sqrt(l);
        v[27] += l * rr + mu * (e * e);
        v[28] += 1.0;
      }
      block_sum<FW>(v, sh);
      if (tid == 0) {
        if (dg.iter_mu) dg.iter_mu[(int64_t)pair * iterations + it] = mu;
        if (dg.iter_energy) dg.iter_energy[(int64_t)pair * iterations + it] = v[27];
        double x[6], Mx[12], Tn[12];
        if (!icp_plane_solve(v, v + 21, v[28], x)) {
          s_stop = 1;
        } else {
          icp_plane_transform(x, Mx);
          for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 4; ++b)
              Tn[a * 4 + b] = (Mx[a * 4] * T[b] + Mx[a * 4 + 1] * T[4 + b]) + Mx[a * 4 + 2] * T[8 + b];
            Tn[a * 4 + 3] += Mx[a * 4 + 3];
          }
          for (int k = 0; k < 12; ++k) sT[k] = Tn[k];
          if (dg.iter_T)
            for (int k = 0; k < 12; ++k) dg.iter_T[((int64_t)pair * iterations + it) * 12 + k] = Tn[k];
          if (division_factor > 1.0 && it % 4 == 0 && mu > floor_mu) s_mu = mu / division_factor;
        }
      }
      __syncthreads();
      if (s_stop) { iters_run = -(it + 1); break; }             // block-uniform
      iters_run = it + 1;
    }
  }
  if (tid == 0) {
    if (dg.iters_run) dg.iters_run[pair] = iters_run;
    // 5 un-normalise
    float o[12];
    bool ok = pose;
    for (int k = 0; k < 12; ++k) o[k] = 0.f;
    if (pose) {
      for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) o[a * 4 + b] = (float)sT[a * 4 + b];
        const double Rm = (sT[a * 4] * ms[0] + sT[a * 4 + 1] * ms[1]) + sT[a * 4 + 2] * ms[2];
        o[a * 4 + 3] = (float)((scale * sT[a * 4 + 3] + mq[a]) - Rm);
      }
      for (int k = 0; k < 12; ++k) ok = ok && isfinite(o[k]);
      if (!ok)
        for (int k = 0; k < 12; ++k) o[k] = 0.f;
    }
    for (int k = 0; k < 12; ++k) hyp_T[(int64_t)pair * 12 + k] = o[k];
    hyp_valid[pair] = ok ? 1 : 0;
  }
}

size_t fgr_scan_tmp_bytes(int64_t n) {
  size_t b = 0;
  hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const int32_t*)nullptr, (int32_t*)nullptr, (int)n);
  return b;
}

template <bool TUPLE>
void launch_select(const FgrArgs& a, const PoseParts& s, float ts2, int NB, int cap, int64_t L, int32_t* blk_cnt, int32_t* blk_pre,
                   int32_t* rows, bool fill, hipStream_t st) {
  const CorrProblem& p = a.p;
  const dim3 grid(NB, p.pairs);
  if (!fill)
    hipLaunchKernelGGL((fgr_select_kernel<TUPLE, false>), grid, dim3(FB), 0, st, s.cs, s.cq, p.counts, p.M, a.max_trials, a.seed, ts2, NB,
                       cap, L, blk_cnt, blk_pre, rows);
  else
    hipLaunchKernelGGL((fgr_select_kernel<TUPLE, true>), grid, dim3(FB), 0, st, s.cs, s.cq, p.counts, p.M, a.max_trials, a.seed, ts2, NB,
                       cap, L, blk_cnt, blk_pre, rows);
}

}  // namespace

size_t fgr_scratch_bytes(int pairs, int M, int tuple_test, int max_tuples, int max_trials, int refine_iters) {
  const int64_t nb = (int64_t)pairs * fgr_blocks(fgr_candidates(tuple_test, M, max_trials));
  return FgrLayout(pairs, M, tuple_test, max_tuples, max_trials, refine_iters, fgr_scan_tmp_bytes(nb)).bytes;
}

int launch_fgr(const FgrArgs& a, void* scratch, hipStream_t st) {
  const CorrProblem& p = a.p;
  const int P = p.pairs, M = p.M, tt = a.tuple_test ? 1 : 0;
  if (!fgr_shape_ok(P, M, a.max_trials)) return 1;
  const int NB = fgr_blocks(fgr_candidates(tt, M, a.max_trials));
  const int cap = fgr_accept_cap(tt, M, a.max_tuples);
  const int64_t L = fgr_list_rows(tt, M, a.max_tuples);
  size_t tmp = fgr_scan_tmp_bytes((int64_t)P * NB);
  const FgrLayout lay(P, M, tt, a.max_tuples, a.max_trials, p.refine_iters, tmp);
  const PoseParts s(scratch, lay.pose);
  const CandSet hyp(scratch, lay.hyp, 1);
  int32_t *rows = at<int32_t>(scratch, lay.rows), *blk_cnt = at<int32_t>(scratch, lay.blk_cnt), *blk_pre = at<int32_t>(scratch, lay.blk_pre);
  double* npts = at<double>(scratch, lay.npts);

  launch_pose_front(p, s, st);
  hipMemsetAsync(rows, 0xFF, (size_t)P * L * 4, st);
  if (tt) launch_select<true>(a, s, a.ts2, NB, cap, L, blk_cnt, blk_pre, rows, false, st);
  else launch_select<false>(a, s, a.ts2, NB, cap, L, blk_cnt, blk_pre, rows, false, st);
  if (hipcub::DeviceScan::ExclusiveSum(at<char>(scratch, lay.tmp), tmp, blk_cnt, blk_pre, P * NB, st) != hipSuccess) return 2;
  if (tt) launch_select<true>(a, s, a.ts2, NB, cap, L, blk_cnt, blk_pre, rows, true, st);
  else launch_select<false>(a, s, a.ts2, NB, cap, L, blk_cnt, blk_pre, rows, true, st);
  const FgrDiagPtrs dg{a.diag_n_rows, a.diag_trials, a.diag_iters_run, a.diag_norm, a.diag_iter_T, a.diag_iter_mu, a.diag_iter_energy};
  hipLaunchKernelGGL(fgr_optimize_kernel, dim3(P), dim3(FB), 0, st, s.cs, s.cq, p.counts, M, rows, L, blk_cnt, blk_pre, NB, tt, a.max_tuples,
                     a.max_trials, (double)p.max_dist, a.iterations, (double)a.division_factor, npts, hyp.T, hyp.valid, dg);
  launch_pose_tail(p, s, hyp, st);
  if (a.diag_rows) hipMemcpyAsync(a.diag_rows, rows, (size_t)P * L * 4, hipMemcpyDeviceToDevice, st);
  return 0;
}

}  // namespace dsir
