// Point-to-point ICP refinement of a registration result: the `use_icp` branch of the reference's
// pose_optimization (test.py:241-258), which hands the predicted pose to open3d's
//   registration_icp(src, tgt, max_correspondence_distance, T_init, TransformationEstimationPointToPoint())
// with the default convergence criteria (relative_fitness = relative_rmse = 1e-6, max_iteration = 30).  The branch is
// switched off in the reference (`use_icp = False`, test.py:216) and open3d is not installable here, so parity at this
// boundary is unpinned: the algorithm restated (and mirrored in oracle/icp.py) is open3d's RegistrationICP loop —
//   result = correspondences(T·src, tgt)                       nearest target within the radius, fitness, inlier RMSE
//   repeat: update = Kabsch(correspondences); T = update·T; src = update·src; result' = correspondences(...)
//           stop when |fitness' - fitness| < relative_fitness and |rmse' - rmse| < relative_rmse
// run for all pairs of a batch at once, entirely on device (no host round trip per iteration): a per-pair `done` flag
// turns the remaining iterations into no-ops.  Nearest neighbours: exact brute force in fp32 (squared distance
// (dx*dx + dy*dy) + dz*dz without FMA contraction, ties to the lower index), support staged through LDS.
// IcpSearch::Grid runs the same loop with the cell index of icp_grid.hip at the search sites: the same neighbour and the same d2
// bits, so the same pose and statistics byte for byte, without the J x K product per iteration.  One call path: IcpArgs (kernels.h)
// in, IcpLayout (icp_layout.h) for the scratch, the estimator as a step (step_point / step_plane) of one loop body.
//
// ---- Point-to-plane estimator (dsir_icp_refine_ex, estimator 1): open3d's TransformationEstimationPointToPlane in the same loop.
// open3d is not installable here: parity is unpinned, THE RULE IS OWNED HERE and restated in tests/icp_plane_host.py.  The first
// search, fitness, inlier RMSE (from point distances), the convergence test, the `done` flag and max_iter are the loop above;
// only the update differs.  Over the correspondences (s = moved source point, t = its target point, n = the target's normal,
// all fp32 values taken to fp64):
//   r = ((s-t).x n.x + (s-t).y n.y) + (s-t).z n.z,   J = [s x n ; n]  (6),   A = sum J J^T (21 distinct sums),   b = sum J r (6)
//   solve A x = -b in fp64;  update R = Rz(x2) Ry(x1) Rx(x0), t = (x3, x4, x5)  (open3d's TransformVector6dToMatrix4d),
//   rounded to fp32 once, applied to the moved points and composed onto T exactly as the Kabsch step's transform is.
// A correspondence whose normal is (0,0,0) (dsir_estimate_normals' degenerate output), or whose normal or target coordinates are
// not finite, contributes nothing and is not counted as a row.  The update is the IDENTITY - the moved points and T keep their
// bits, and the pair's fifth statistic counts it - when fewer than 6 rows entered the sums, when the system is singular
// (icp_plane.h: LDL^T without pivoting of the matrix scaled to unit diagonal, a pivot below kIcpPlanePivotMin; a diagonal entry
// that is zero or not finite is singular), or when any of the pair's moved source points is not finite.
// Kernels: icp_plane_accum_kernel, one workgroup per (chunk of kIcpPlaneChunk source points, pair), writes the chunk's 29 fp64 sums
// (wave butterflies, then the waves in order: no atomics) to its own slot; icp_plane_step_kernel, one workgroup per 256 source
// points and pair, adds the pair's slots in chunk order (every workgroup for itself: the same bits in each), solves, and moves its
// points; its first workgroup composes T and hands the pair's `done` flag to the next search.  The partition depends on J alone,
// so a pair's result depends neither on the run nor on the other pairs of the call.  An iteration is four launches, as in the
// point-to-point loop (flags, Kabsch, search, statistics there; sums, step, search, statistics here).
//
// ---- Clouds of unequal sizes (IcpArgs::counts_src / counts_ref, dsir_icp_refine_ex3 and dsir_icp_correspondences_ex): J and K are the
// row capacities of the arrays and the strides of every scratch part; pair p works on its first Jp = pair_rows(counts_src, p, J)
// source and Kp = pair_rows(counts_ref, p, K) reference rows.  Every kernel stops at the pair's own count - the apply, the search
// (slices of Kp; query blocks beyond Jp write "no correspondence" and leave block-uniformly), the statistics (fitness = matched / Jp,
// 0 for Jp == 0), the Kabsch kernels (KabschArgs::counts), the plane sums and the move (chunks of Jp: last = min(Jp, first +
// kIcpPlaneChunk), icp_plane_chunks(Jp) slots added) - so a padding row is never read into anything that reaches an output, and
// every partition is the one the pair has in a call of its own: pair p gets, byte for byte, what the dense call on its first Jp
// and Kp rows alone writes.  A pair with Jp == 0 or Kp == 0 has no correspondence: identity updates (the Kabsch kernels' frozen step,
// the plane step's "fewer than 6 rows"), T carried over bit for bit, fitness and RMSE 0, frozen by the first convergence test.
// As before: no floating-point atomics, no scratch shared between pairs, the same bytes on every run, and a pair's bytes do not
// depend on the other pairs of the call - their counts included.  Without counts every launch, grid and byte is what it was.
//
// ---- Robust loss kernels (IcpArgs::kernel / kernel_scale, dsir_icp_refine_ex4): open3d's `robust_kernel` of both estimators.  open3d is
// not installable here: parity is unpinned, THE RULE IS OWNED HERE (icp_robust.h holds the arithmetic) and restated in
// tests/icp_robust_host.py.  The weight of a correspondence is a function of its squared residual q = r^2 and the scale k > 0, in fp64,
// one correctly rounded operation after the other in the order written (k^2 = k * k first):
//   l2 (0): 1    huber (1): q <= k^2 ? 1 : k / sqrt(q)    cauchy (2): 1 / (1 + q / k^2)    gm (3): k / ((k + q) * (k + q))
//   tukey (4): q <= k^2 ? (1 - q / k^2)^2 : 0
// Point-to-point: q = the fp32 squared point distance d2 of the search, w = (float)weight((double)d2, k) rounded once, written by
// icp_stats_kernel<true> where the l2 loop writes 1; the weighted Kabsch step is the one the l2 loop runs.  A weight 0 on a matched
// row leaves its index alone.  A pair whose weights are all 0 takes the frozen step (KabschArgs::zero_freeze; why: icp_robust.h): the
// identity update, T carried over bit for bit.  Point-to-plane: q = r * r of the fp64 plane residual, wr = weight(q, k),
// A += (wr J[a]) J[b], b += (wr J[a]) r in icp_plane_accum_kernel<true>; a row whose weight is not > 0 contributes nothing and is not
// counted, then "fewer than 6 rows" and the singular-system rule apply as they are.
// The kernel acts on the estimator ALONE, as in open3d: the search, the fitness, the inlier RMSE (unweighted point distances), the
// convergence test, max_iter, the done flags, the stats columns and the information matrix do not see it.  l2 runs the <false>
// instantiations of both kernels - the code they were - and zero_freeze = 0: the same bytes as before.  As before: no atomics, the same
// bytes on every run, a pair's bytes independent of the other pairs, of the counts' padding and of the search.
#include "kernels.h"
#include "device_utils.h"
#include "icp_layout.h"
#include "icp_robust.h"

namespace dsir {

namespace {

constexpr int QB = 64;      // queries per block (one per lane)
constexpr int NW = 4;       // waves per block = support slices
constexpr int TILE = 256;   // support points staged per wave per step

// cur[pair][j] = T[pair] * src[pair][j] for the pair's own rows (J: the row capacity)
__global__ void icp_apply_kernel(const float* __restrict__ src, int stride, int J, const int32_t* __restrict__ counts_src,
                                 const float* __restrict__ T, float* __restrict__ cur) {
  const int pair = blockIdx.y;
  const float* t = T + (int64_t)pair * 12;
  const int Jp = pair_rows(counts_src, pair, J);
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < Jp; j += gridDim.x * blockDim.x) {
    const float* p = src + ((int64_t)pair * J + j) * stride;
    const float x = p[0], y = p[1], z = p[2];
    float* o = cur + ((int64_t)pair * J + j) * 3;
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = se3_row(t, r, x, y, z);
  }
}

__global__ __launch_bounds__(QB * NW) void icp_nn_kernel(const float* __restrict__ cur, const float* __restrict__ ref,
                                                         int ref_stride, int J, int K, const int32_t* __restrict__ counts_src,
                                                         const int32_t* __restrict__ counts_ref, float r2,
                                                         int32_t* __restrict__ idx, float* __restrict__ d2,
                                                         const int32_t* __restrict__ skip) {
  // a converged pair keeps the correspondences of its last search: its points no longer move (block-uniform exit)
  if (skip && skip[blockIdx.y]) return;
  __shared__ float4 tile[NW][TILE];
  __shared__ float md[NW][QB];
  __shared__ int mi[NW][QB];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int pair = blockIdx.y;
  const int Jp = pair_rows(counts_src, pair, J), Kp = pair_rows(counts_ref, pair, K);   // the pair's own rows; J, K: the capacities
  const float* Q = cur + (int64_t)pair * J * 3;
  const float* S = ref + (int64_t)pair * K * ref_stride;
  const int q = blockIdx.x * QB + lane;
  if (blockIdx.x * QB >= Jp) {   // a block of padding rows only: "no correspondence", and out before the first barrier (block-uniform)
    if (w == 0 && q < J) { idx[(int64_t)pair * J + q] = -1; d2[(int64_t)pair * J + q] = 0.f; }
    return;
  }
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (q < Jp) { qx = Q[(int64_t)q * 3]; qy = Q[(int64_t)q * 3 + 1]; qz = Q[(int64_t)q * 3 + 2]; }
  // the slices are a function of Kp alone (block-uniform trip counts); the arg-min with ties to the lower index does not depend on them
  const int slice = (Kp + NW - 1) / NW;
  const int s_begin = w * slice, s_end = min(Kp, s_begin + slice);
  float bd = INFINITY;
  int bi = -1;
  for (int t0 = 0; t0 < slice; t0 += TILE) {
#pragma unroll
    for (int r = 0; r < TILE / 64; ++r) {
      const int j = s_begin + t0 + r * 64 + lane;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j < s_end) { v.x = S[(int64_t)j * ref_stride]; v.y = S[(int64_t)j * ref_stride + 1]; v.z = S[(int64_t)j * ref_stride + 2]; }
      tile[w][r * 64 + lane] = v;
    }
    __syncthreads();
    const int cnt = max(0, min(TILE, s_end - (s_begin + t0)));
    for (int j = 0; j < cnt; ++j) {
      const float d = dist2_rn(tile[w][j], qx, qy, qz);
      if (d < bd) { bd = d; bi = s_begin + t0 + j; }
    }
    __syncthreads();
  }
  md[w][lane] = bd; mi[w][lane] = bi;
  __syncthreads();
  if (w == 0 && q < J) {
#pragma unroll
    for (int s = 1; s < NW; ++s) {
      const float d = md[s][lane];
      if (d < bd) { bd = d; bi = mi[s][lane]; }   // slices are ascending in index: strict < keeps the lower index on a tie
    }
    const bool in = q < Jp && bi >= 0 && bd <= r2;            // a padding row of the last block: -1 and 0, whatever it met
    idx[(int64_t)pair * J + q] = in ? bi : -1;
    d2[(int64_t)pair * J + q] = in ? bd : 0.f;
  }
}

// per pair: fitness = |corr| / Jp (0 for a pair without source rows), inlier RMSE = sqrt(sum d2 / |corr|); convergence test against
// the previous values; correspondences turned into (clamped index, 0/1 weight) for the Kabsch kernel.  state = {fitness, rmse, done,
// iterations}.  Jp = the pair's own rows of the capacity J; the rows beyond are neither read nor written.
// ROBUST: the weight of a matched row is the kernel's (icp_robust.h) of its squared point distance, rounded once to fp32 - possibly 0,
// the index stays; count, sums and the convergence test do not see it.  ROBUST = false is the least-squares loop's kernel as it was.
template <bool ROBUST>
__global__ __launch_bounds__(256) void icp_stats_kernel(int32_t* __restrict__ idx, const float* __restrict__ d2,
                                                        float* __restrict__ w, int J, const int32_t* __restrict__ counts_src, int check,
                                                        float rel_fitness, float rel_rmse, double* __restrict__ state, int kernel, double kscale) {
  __shared__ double s_cnt[4], s_sse[4];
  const int pair = blockIdx.x;
  double* st = state + (int64_t)pair * 4;
  if (st[2] != 0.0) return;   // converged earlier: frozen (block-uniform)
  const int Jp = pair_rows(counts_src, pair, J);
  double cnt = 0.0, sse = 0.0;
  for (int j = threadIdx.x; j < Jp; j += 256) {
    const int64_t o = (int64_t)pair * J + j;
    const int i = idx[o];
    const bool in = i >= 0;
    if (ROBUST) w[o] = in ? (float)icp_robust_weight(kernel, (double)d2[o], kscale) : 0.f;
    else w[o] = in ? 1.f : 0.f;
    if (!in) idx[o] = 0;
    cnt += in ? 1.0 : 0.0;
    sse += in ? (double)d2[o] : 0.0;
  }
  cnt = wave_sum(cnt); sse = wave_sum(sse);
  if ((threadIdx.x & 63) == 0) { s_cnt[threadIdx.x >> 6] = cnt; s_sse[threadIdx.x >> 6] = sse; }
  __syncthreads();
  if (threadIdx.x == 0) {
    cnt = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    sse = s_sse[0] + s_sse[1] + s_sse[2] + s_sse[3];
    const double fitness = Jp > 0 ? cnt / (double)Jp : 0.0;
    const double rmse = cnt > 0.0 ? sqrt(sse / cnt) : 0.0;
    if (check) {
      st[3] += 1.0;
      if (fabs(st[0] - fitness) < (double)rel_fitness && fabs(st[1] - rmse) < (double)rel_rmse) st[2] = 1.0;
    }
    st[0] = fitness; st[1] = rmse;
  }
}

// one search step's {fitness, inlier RMSE} in icp_stats_kernel's summation order, the correspondences left as the search wrote them
__global__ __launch_bounds__(256) void icp_corr_stats_kernel(const int32_t* __restrict__ idx, const float* __restrict__ d2, int J,
                                                             const int32_t* __restrict__ counts_src, double* __restrict__ out) {
  __shared__ double s_cnt[4], s_sse[4];
  const int pair = blockIdx.x;
  const int Jp = pair_rows(counts_src, pair, J);
  double cnt = 0.0, sse = 0.0;
  for (int j = threadIdx.x; j < Jp; j += 256) {
    const int64_t o = (int64_t)pair * J + j;
    const bool in = idx[o] >= 0;
    cnt += in ? 1.0 : 0.0;
    sse += in ? (double)d2[o] : 0.0;
  }
  cnt = wave_sum(cnt); sse = wave_sum(sse);
  if ((threadIdx.x & 63) == 0) { s_cnt[threadIdx.x >> 6] = cnt; s_sse[threadIdx.x >> 6] = sse; }
  __syncthreads();
  if (threadIdx.x == 0) {
    cnt = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    sse = s_sse[0] + s_sse[1] + s_sse[2] + s_sse[3];
    out[(int64_t)pair * 2] = Jp > 0 ? cnt / (double)Jp : 0.0;
    out[(int64_t)pair * 2 + 1] = cnt > 0.0 ? sqrt(sse / cnt) : 0.0;
  }
}

__global__ void icp_done_flags_kernel(const double* __restrict__ state, int pairs, int32_t* __restrict__ skip) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < pairs) skip[p] = state[(int64_t)p * 4 + 2] != 0.0 ? 1 : 0;
}

// ---- point-to-plane update (the rule: this file's header)
constexpr int PT = 256;    // threads of both plane kernels (kIcpPlaneChunk / PT points per thread in the sums)

// C = T o P for row-major 3x4 transforms, (R_T R_P, R_T t_P + t_T), in the rounding sequence kabsch_solve composes the cumulative pose by
__device__ __forceinline__ void se3_compose(const float* T, const float* P, float* C) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c)
      C[r * 4 + c] = fmaf(T[r * 4 + 2], P[2 * 4 + c], fmaf(T[r * 4 + 1], P[1 * 4 + c], __fmul_rn(T[r * 4 + 0], P[c])));
    const float rt = fmaf(T[r * 4 + 2], P[2 * 4 + 3], fmaf(T[r * 4 + 1], P[1 * 4 + 3], __fmul_rn(T[r * 4 + 0], P[3])));
    C[r * 4 + 3] = __fadd_rn(rt, T[r * 4 + 3]);
  }
}

// normals of pair `pair`: N + pair * cs, `ld` floats between points ([P][K][3], or columns 3..5 of the reference rows)
struct PlaneNormals { const float* N; int64_t cs; int ld; };

// ROBUST: a row enters the sums with the kernel's weight (icp_robust.h) of its squared plane residual, wr = weight(r * r, k) in fp64:
// A += (wr J[a]) J[b], b += (wr J[a]) r; a weight that is not > 0 contributes nothing and is not a row.  The fp32 array w only says
// "has a correspondence" here: under every kernel the plane loop runs icp_stats_kernel<false>, which writes 1 or 0 (the kernel's
// argument is the plane residual, not the point distance).  ROBUST = false is the least-squares kernel as it was.
template <bool ROBUST>
__global__ __launch_bounds__(PT) void icp_plane_accum_kernel(const float* __restrict__ cur, const float* __restrict__ ref, int ref_stride,
                                                             PlaneNormals nrm, const int32_t* __restrict__ idx,
                                                             const float* __restrict__ w, int J, int K, const int32_t* __restrict__ counts_src,
                                                             const double* __restrict__ state, double* __restrict__ part, int kernel, double kscale) {
  __shared__ double sh[(PT / 64 + 1) * kIcpPlaneSums];
  const int pair = blockIdx.y, ch = blockIdx.x;
  if (state[(int64_t)pair * 4 + 2] != 0.0) return;   // converged: the step is the identity (block-uniform)
  const int Jp = pair_rows(counts_src, pair, J);
  if (ch >= icp_plane_chunks(Jp)) return;            // a chunk of padding rows only: no slot of the pair's sum (block-uniform)
  const float* S = ref + (int64_t)pair * K * ref_stride;
  const float* N = nrm.N + pair * nrm.cs;
  const int first = ch * kIcpPlaneChunk, last = min(Jp, first + kIcpPlaneChunk);
  double v[kIcpPlaneSums];
#pragma unroll
  for (int k = 0; k < kIcpPlaneSums; ++k) v[k] = 0.0;
  for (int j = first + threadIdx.x; j < last; j += PT) {
    const int64_t o = (int64_t)pair * J + j;
    const float sx = cur[o * 3], sy = cur[o * 3 + 1], sz = cur[o * 3 + 2];
    if (!(isfinite(sx) && isfinite(sy) && isfinite(sz))) v[28] += 1.0;
    if (w[o] == 0.f) continue;                        // no correspondence (icp_stats_kernel: weight 0, index clamped)
    const int64_t i = idx[o];
    const float tx = S[i * ref_stride], ty = S[i * ref_stride + 1], tz = S[i * ref_stride + 2];
    const float nx = N[i * nrm.ld], ny = N[i * nrm.ld + 1], nz = N[i * nrm.ld + 2];
    if (!(isfinite(tx) && isfinite(ty) && isfinite(tz) && isfinite(nx) && isfinite(ny) && isfinite(nz))) continue;
    if (nx == 0.f && ny == 0.f && nz == 0.f) continue;
    const double s[3] = {(double)sx, (double)sy, (double)sz}, n[3] = {(double)nx, (double)ny, (double)nz};
    const double r = ((s[0] - (double)tx) * n[0] + (s[1] - (double)ty) * n[1]) + (s[2] - (double)tz) * n[2];
    const double Jr[6] = {s[1] * n[2] - s[2] * n[1], s[2] * n[0] - s[0] * n[2], s[0] * n[1] - s[1] * n[0], n[0], n[1], n[2]};
    int k = 0;
    if (ROBUST) {
      const double wr = icp_robust_weight(kernel, r * r, kscale);
      if (!(wr > 0.0)) continue;
      double wJ[6];
#pragma unroll
      for (int a = 0; a < 6; ++a) wJ[a] = wr * Jr[a];
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) v[k++] += wJ[a] * Jr[b];
#pragma unroll
      for (int a = 0; a < 6; ++a) v[21 + a] += wJ[a] * r;
    } else {
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) v[k++] += Jr[a] * Jr[b];
#pragma unroll
      for (int a = 0; a < 6; ++a) v[21 + a] += Jr[a] * r;
    }
    v[27] += 1.0;
  }
  block_sum<PT / 64>(v, sh);
  if (threadIdx.x < kIcpPlaneSums)
    part[((int64_t)pair * gridDim.x + ch) * kIcpPlaneSlots + threadIdx.x] = sh[(PT / 64) * kIcpPlaneSums + threadIdx.x];
}

// nch: the slots a pair has (the capacity's chunks); the pair's sum adds the icp_plane_chunks(Jp) of them that its own rows fill
__global__ __launch_bounds__(PT) void icp_plane_step_kernel(float* __restrict__ cur, int J, const int32_t* __restrict__ counts_src, int nch,
                                                            const double* __restrict__ part,
                                                            const double* __restrict__ state, const float* __restrict__ T_prev,
                                                            float* __restrict__ T_cum, double* __restrict__ nsing,
                                                            int32_t* __restrict__ skip) {
  __shared__ double tot[kIcpPlaneSlots];
  __shared__ float sT[12];
  __shared__ int s_move;
  const int pair = blockIdx.y;
  const bool lead = blockIdx.x == 0 && threadIdx.x == 0;   // the one thread that writes the pair's transform, counter and flag
  const bool done = state[(int64_t)pair * 4 + 2] != 0.0;   // block-uniform
  if (lead) skip[pair] = done ? 1 : 0;                      // the search after this step leaves a converged pair alone
  if (done) {
    if (lead)
      for (int k = 0; k < 12; ++k) T_cum[pair * 12 + k] = T_prev[pair * 12 + k];
    return;
  }
  const int Jp = pair_rows(counts_src, pair, J);
  if (threadIdx.x < kIcpPlaneSums) {
    double s = 0.0;
    const int used = icp_plane_chunks(Jp);
    for (int c = 0; c < used; ++c) s += part[((int64_t)pair * nch + c) * kIcpPlaneSlots + threadIdx.x];   // chunk order
    tot[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double x[6], Td[12];
    const bool ok = tot[28] == 0.0 && icp_plane_solve(tot, tot + 21, tot[27], x);
    bool move = ok;
    if (ok) {
      icp_plane_transform(x, Td);
      for (int k = 0; k < 12; ++k) {
        sT[k] = (float)Td[k];
        move = move && isfinite(sT[k]);
      }
    }
    s_move = move ? 1 : 0;
    if (lead) {
      const float* P = T_prev + pair * 12;
      float C[12];
      if (move) se3_compose(sT, P, C);
      for (int k = 0; k < 12; ++k) T_cum[pair * 12 + k] = move ? C[k] : P[k];
      if (!move) nsing[pair] += 1.0;
    }
  }
  __syncthreads();
  if (!s_move) return;                                      // identity update: the points keep their bits (block-uniform)
  const int j = blockIdx.x * PT + threadIdx.x;
  if (j < Jp) {
    float* p = cur + ((int64_t)pair * J + j) * 3;
    const float x = p[0], y = p[1], z = p[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = se3_row(sT, r, x, y, z);
  }
}

// stats [pairs][5] = the four values of the loop's state, then the identity updates taken for a singular system (0 without counters)
__global__ void icp_stats5_kernel(const double* __restrict__ state, const double* __restrict__ nsing, int pairs, double* __restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pairs) return;
  for (int k = 0; k < 4; ++k) out[(int64_t)p * 5 + k] = state[(int64_t)p * 4 + k];
  out[(int64_t)p * 5 + 4] = nsing ? nsing[p] : 0.0;
}

// the loop's scratch as pointers: IcpLayout's parts
struct IcpParts {
  float* cur; int32_t* idx; float* d2; float* w; float* Ta; float* Tb; double* state; int32_t* skip; float* Tstep;
  double* part; double* nsing; void* grid;
  IcpParts(const IcpLayout& l, void* scratch, bool plane) {
    char* b = reinterpret_cast<char*>(scratch);
    cur = reinterpret_cast<float*>(b + l.cur); idx = reinterpret_cast<int32_t*>(b + l.idx); d2 = reinterpret_cast<float*>(b + l.d2);
    w = reinterpret_cast<float*>(b + l.w); Ta = reinterpret_cast<float*>(b + l.Ta); Tb = reinterpret_cast<float*>(b + l.Tb);
    state = reinterpret_cast<double*>(b + l.state); skip = reinterpret_cast<int32_t*>(b + l.skip);
    Tstep = reinterpret_cast<float*>(b + l.Tstep);
    part = plane ? reinterpret_cast<double*>(b + l.part) : nullptr;
    nsing = plane ? reinterpret_cast<double*>(b + l.nsing) : nullptr;
    grid = b + l.grid;
  }
};

size_t grid_bytes(const IcpArgs& a) { return a.search != IcpSearch::Brute ? icp_grid_scratch_bytes(a.pairs, a.J, a.K) : 0; }
IcpLayout layout(const IcpArgs& a) { return IcpLayout(a.pairs, a.J, a.estimator == 1, grid_bytes(a)); }

// the point-to-point update: the pairs' done flags, then Kabsch on the correspondences (moves cur, composes Tn = step o Tp)
void step_point(const IcpArgs& a, const IcpParts& s, const float* Tp, float* Tn, hipStream_t st) {
  hipLaunchKernelGGL(icp_done_flags_kernel, dim3((a.pairs + 255) / 256), dim3(256), 0, st, s.state, a.pairs, s.skip);
  KabschArgs k{};
  k.src = s.cur; k.ref = a.ref; k.idx = s.idx; k.w = s.w; k.src_stride = (int64_t)a.J * 3; k.ref_stride = (int64_t)a.K * a.stride;
  k.ref_ld = a.stride; k.sigmoid = 0; k.pairs = a.pairs; k.m = a.J; k.T = s.Tstep; k.invalid = nullptr;
  k.src_out = s.cur; k.src_out_stride = (int64_t)a.J * 3; k.T_prev = Tp; k.T_cum = Tn; k.T_stride = 12; k.skip = s.skip;
  k.counts = a.counts_src; k.ref_counts = a.counts_ref;   // a pair without a source or a reference row: the frozen step, no row of it read
  k.zero_freeze = a.kernel != kIcpL2;                      // a robust kernel may leave a pair without a non-zero weight: the frozen step too
  launch_kabsch(k, st);
}

// the point-to-plane update: the chunks' sums, then the solve and the move (its first workgroup composes Tn and writes the flags)
void step_plane(const IcpArgs& a, const IcpParts& s, const float* Tp, float* Tn, hipStream_t st) {
  const int nch = icp_plane_chunks(a.J);
  const auto accum = a.kernel != kIcpL2 ? icp_plane_accum_kernel<true> : icp_plane_accum_kernel<false>;
  hipLaunchKernelGGL(accum, dim3(nch, a.pairs), dim3(PT), 0, st, (const float*)s.cur, a.ref, a.stride,
                     PlaneNormals{a.normals, a.normals_cs, a.normals_ld}, (const int32_t*)s.idx, (const float*)s.w, a.J, a.K,
                     a.counts_src, (const double*)s.state, s.part, a.kernel, (double)a.kernel_scale);
  hipLaunchKernelGGL(icp_plane_step_kernel, dim3((a.J + PT - 1) / PT, a.pairs), dim3(PT), 0, st, s.cur, a.J, a.counts_src, nch, (const double*)s.part,
                     (const double*)s.state, Tp, Tn, s.nsing, s.skip);
}

// the search of cur [pairs][J][3]: the grid's kernel with an index (built by the caller), else the brute force
void search(const IcpArgs& a, const IcpGrid* grid, const float* cur, float r2, int32_t* idx, float* d2, const int32_t* skip, hipStream_t st) {
  if (grid) { launch_icp_nn_grid(*grid, cur, a.pairs, a.J, a.K, a.counts_src, a.counts_ref, r2, idx, d2, skip, st); return; }
  hipLaunchKernelGGL(icp_nn_kernel, dim3((a.J + QB - 1) / QB, a.pairs), dim3(QB * NW), 0, st, cur, a.ref, a.stride, a.J, a.K, a.counts_src, a.counts_ref,
                     r2, idx, d2, skip);
}

// the statistics of a search and the weights of the next update: the kernel's weights for the point estimator under a robust kernel,
// else 1 / 0 (the plane sums weigh by the plane residual themselves)
void stats(const IcpArgs& a, const IcpParts& s, int check, hipStream_t st) {
  const auto k = a.kernel != kIcpL2 && a.estimator == 0 ? icp_stats_kernel<true> : icp_stats_kernel<false>;
  hipLaunchKernelGGL(k, dim3(a.pairs), dim3(256), 0, st, s.idx, (const float*)s.d2, s.w, a.J, a.counts_src, check, a.rel_fitness, a.rel_rmse, s.state,
                     a.kernel, (double)a.kernel_scale);
}

}  // namespace

size_t icp_scratch_bytes(const IcpArgs& a) { return layout(a).bytes; }

// The first search under T_init, then max_iter times: the estimator's step, the search, the statistics with the convergence test.
// With a cell index (search != Brute) it is built once after the points are moved by T_init and serves every search.
int launch_icp_refine(const IcpArgs& a, void* scratch, hipStream_t st) {
  const bool plane = a.estimator == 1;
  const IcpParts s(layout(a), scratch, plane);
  const int pairs = a.pairs, J = a.J;
  if (plane) hipMemsetAsync(s.nsing, 0, (size_t)pairs * 8, st);
  const float r2 = a.max_corr_dist * a.max_corr_dist;
  hipMemsetAsync(s.state, 0, (size_t)pairs * 32, st);
  hipMemcpyAsync(s.Ta, a.T_init, (size_t)pairs * 48, hipMemcpyDeviceToDevice, st);
  hipLaunchKernelGGL(icp_apply_kernel, dim3((J + 255) / 256, pairs), dim3(256), 0, st, a.src, a.stride, J, a.counts_src, s.Ta, s.cur);
  IcpGrid grid{};
  const IcpGrid* g = a.search != IcpSearch::Brute ? &grid : nullptr;
  if (g)
    if (const int e = icp_grid_build(a.ref, a.stride, s.cur, pairs, J, a.K, a.counts_src, a.counts_ref, a.max_corr_dist, a.search == IcpSearch::Grid, s.grid, st, &grid)) return e;
  search(a, g, s.cur, r2, s.idx, s.d2, nullptr, st);
  stats(a, s, 0, st);
  float *Tp = s.Ta, *Tn = s.Tb;
  for (int it = 0; it < a.max_iter; ++it) {
    if (plane) step_plane(a, s, Tp, Tn, st);
    else step_point(a, s, Tp, Tn, st);
    search(a, g, s.cur, r2, s.idx, s.d2, s.skip, st);
    stats(a, s, 1, st);
    float* t = Tp; Tp = Tn; Tn = t;
  }
  hipMemcpyAsync(a.T_out, Tp, (size_t)pairs * 48, hipMemcpyDeviceToDevice, st);
  if (a.stats_out) hipMemcpyAsync(a.stats_out, s.state, (size_t)pairs * 32, hipMemcpyDeviceToDevice, st);
  if (a.stats5_out)
    hipLaunchKernelGGL(icp_stats5_kernel, dim3((pairs + 255) / 256), dim3(256), 0, st, (const double*)s.state, (const double*)s.nsing, pairs,
                       a.stats5_out);
  return 0;
}

size_t icp_corr_scratch_bytes(const IcpArgs& a) { return IcpCorrLayout(a.pairs, a.J, grid_bytes(a)).bytes; }

// one search step under a.T_init: the apply and the search of the loop's first three launches, and their statistics
int launch_icp_correspondences(const IcpArgs& a, int32_t* idx_out, float* d2_out, double* stats_out, void* scratch, hipStream_t st) {
  const IcpCorrLayout l(a.pairs, a.J, grid_bytes(a));
  float* cur = reinterpret_cast<float*>(reinterpret_cast<char*>(scratch) + l.cur);
  hipLaunchKernelGGL(icp_apply_kernel, dim3((a.J + 255) / 256, a.pairs), dim3(256), 0, st, a.src, a.stride, a.J, a.counts_src, a.T_init, cur);
  IcpGrid grid{};
  const IcpGrid* g = a.search != IcpSearch::Brute ? &grid : nullptr;
  if (g)
    if (const int e = icp_grid_build(a.ref, a.stride, cur, a.pairs, a.J, a.K, a.counts_src, a.counts_ref, a.max_corr_dist, a.search == IcpSearch::Grid,
                                     reinterpret_cast<char*>(scratch) + l.grid, st, &grid))
      return e;
  search(a, g, cur, a.max_corr_dist * a.max_corr_dist, idx_out, d2_out, nullptr, st);
  if (stats_out) hipLaunchKernelGGL(icp_corr_stats_kernel, dim3(a.pairs), dim3(256), 0, st, (const int32_t*)idx_out, (const float*)d2_out, a.J, a.counts_src, stats_out);
  return 0;
}

}  // namespace dsir
