// Plane segmentation of a batch of clouds: dsir_segment_plane (include/dsir.h), Engine.segment_plane.  What open3d's
// segment_plane(distance_threshold, ransac_n = 3, num_iterations) and PCL's SACSegmentation do in front of a lidar registration (the
// road of a KITTI scan, floor and walls of a 3DMatch fragment).  open3d cannot be imported here, so parity is UNPINNED and THE RULE IS
// OWNED HERE; deepsir_amd/plane.py restates it in numpy (segment_plane_host).
//
// ---- THE RULE.  Inputs per cloud c: points [clouds][cap][stride >= 3] fp32 (xyz first); counts [clouds] i32 or none: the cloud has
// n = clamp(counts[c], 0, cap) rows (none: cap), rows at and past n are never read.  A row is LIVE iff it is below n, its three
// coordinates are finite and no plane has taken it yet.  Rounds j = 0 .. max_planes - 1; n_live = the live rows of the round:
//   1 draw, hypothesis h < H, k = 0, 1, 2:  d = splitmix64(splitmix64(seed ^ (id_c << 40)) ^ (j << 32) ^ (h << 8) ^ k),
//       r_k = ((d >> 32) * n_live) >> 32, the row is the r_k-th live row in ascending row order.  id_c = cloud_ids[c], or c without
//       cloud_ids: cloud c of a batch is cloud 0 of a call with seed ^ (c << 40) (the device of ransac.hip).  Rejected: n_live < 3, a
//       repeated row.
//   2 fit, fp64 from the fp32 coordinates a, b, c of the rows: u = b - a, v = c - a, m = u x v (each component one product minus the
//       other), len2 = (mx mx + my my) + mz mz; rejected unless len2 > 0 and finite; n = m / sqrt(len2).  The candidate is the normal n
//       and the anchor a, both rounded to fp32 ONCE.  With an axis (a unit vector made on the host, 3 fp32; all zero: none) rejected
//       unless |(nx ax + ny ay) + nz az| >= cos_min, in fp64 before the rounding.
//   3 score, fp32, every operation rounded on its own (no contraction, no fma):  e = ((nx (x - ax)) + (ny (y - ay))) + (nz (z - az)),
//       inlier iff |e| < thr, strict; the score is the INTEGER count over the live rows.  The anchored form is deliberate: n.p + d
//       cancels the cloud's offset (1e2 .. 1e5 m in a world frame) against the threshold in fp32.
//   4 pick: the largest count, ties to the lower h (the key count << 32 | (0xFFFFFFFF - h), plane.h).  The cloud is FINISHED with
//       num_planes = j if no hypothesis is valid or the winning count is below min_inliers (>= 3).
//   5 refit, refine_iters rounds on the plane kept so far: the fp64 centroid of its inliers, then - a second pass - their fp64
//       covariance sums about it; both in an order that depends on the rows alone (below).  Normal = svd3's singular vector of the
//       smallest singular value, anchor = the centroid, both rounded to fp32 once, recounted.  The result replaces the kept plane iff
//       it is finite, passes the axis test and its count is at least the kept one's (the last largest count, as pose_corr.hip).
//   6 finish: the kept plane's inliers get labels = j and stop being live; planes[c][j] = (nx, ny, nz, d), d = -((nx ax + ny ay) +
//       nz az) in fp64 from the fp32 values, rounded; anchors[c][j], plane_counts[c][j].  Orientation is applied once, here, by exact
//       negation of n and d: with an axis n.axis >= 0 (fp64), without d >= 0; on an exact zero the first non-zero component of n is
//       positive.  A zero d and a zero component of n are written as +0 (a negation leaves -0 behind).
//   Outputs: labels [clouds][cap] i32, -1 for every row no plane took (non-finite rows, rows past n - written, never read - and the
//   rows of a finished cloud); num_planes [clouds]; planes, anchors, plane_counts and stats at and behind num_planes are 0;
//   stats [clouds][max_planes][4] = {winning h, valid hypotheses, count before the refits, refits kept}.  A cloud with no live row is
//   no error.
//   Departures from open3d: a draw with a repeated row is rejected; every hypothesis is scored (no early exit on a confidence bound);
//   the tie-break is by h; several planes in one call; the angle constraint.
//
// ---- KERNELS (plane.h: draw and key arithmetic, geometry, limits, scratch layout).  Per round, in stream order, no host
// synchronisation, nothing allocated; done[c] makes every later launch of a finished cloud a no-op (the ICP loop's device):
//   plane_live_kernel<false>: live rows per block of 256 rows (ballot, popcount);  plane_live_kernel<true>: integer prefix of the
//     block counts, ballot ranks inside the block -> live [n_live] rows ascending and pts4, their (x, y, z, -) packed 16 B: no sort,
//     no atomics.
//   plane_hyp_kernel: one lane per h - draw, three 16-byte gathers through the live list's packed copy, fit, verdict.
//   plane_score_kernel, the hot path (H x n_live tests): a workgroup owns 512 candidates, TWO per lane (12 floats in registers),
//     and a slice of the live points staged through LDS in chunks of 256, one ds_read_b128 per point that every lane reads at the
//     SAME address (a broadcast); the next chunk's global loads are issued before the current one is consumed; per-lane integer
//     counters end in one integer atomicAdd per candidate and slice - exact, so arrival order cannot matter.  Two candidates per
//     lane because one test is 9 dependent-free VALU operations plus compare and add (about 24 issue cycles per wave) against a
//     4-cycle b128 LDS read shared by 4 SIMDs: with one candidate per lane the LDS pipe would be ~2/3 busy; two halve the reads
//     per test and leave the loop VALU-bound.  Four would halve them again for nothing and leave H = 1024 with one workgroup
//     column.  The same kernel with H = 1 recounts a refit.  Not the body of pose_score_kernel: residual and layout differ.
//   plane_pick_kernel: one workgroup per cloud, u64 max by butterflies.
//   plane_refit_sum_kernel<1|2>: grid (slices of 4096 live rows, clouds); position q of the live list belongs to lane q % 256, a lane
//     adds its 16 rows in ascending order, wave butterflies, the 4 wave sums added in wave order; plane_refit_solve_kernel adds the
//     slices in slice order (pass 2 forms the centroid the same way), svd3, verdict; plane_refit_keep_kernel.
//   plane_finish_kernel: labels through the live list, and the round's output row.
// Integer atomics only; no floating-point atomic anywhere.
// Build (-Rpass-analysis=kernel-resource-usage, gfx950; VGPRs, SGPRs, LDS, scratch):
//   plane_live_kernel<false>     6 VGPRs, 24 SGPRs,   16 B LDS, no scratch, 8 waves per SIMD
//   plane_live_kernel<true>     20 VGPRs, 33 SGPRs, 2064 B LDS, no scratch, 8 waves per SIMD
//   plane_hyp_kernel            32 VGPRs, 31 SGPRs,    0 B LDS, no scratch, 8 waves per SIMD
//   plane_score_kernel          50 VGPRs, 27 SGPRs, 4352 B LDS, no scratch, 8 waves per SIMD
//   plane_pick_kernel           16 VGPRs, 36 SGPRs,   48 B LDS, no scratch, 8 waves per SIMD
//   plane_refit_sum_kernel<1>   24 VGPRs, 28 SGPRs,  160 B LDS, no scratch, 8 waves per SIMD
//   plane_refit_sum_kernel<2>   32 VGPRs, 34 SGPRs,  264 B LDS, no scratch, 8 waves per SIMD
//   plane_refit_solve_kernel    91 VGPRs, 32 SGPRs,    0 B LDS, no scratch, 5 waves per SIMD (one lane per cloud)
//   plane_refit_keep_kernel     14 VGPRs, 14 SGPRs,    0 B LDS, no scratch, 8 waves per SIMD
//   plane_finish_kernel         12 VGPRs, 44 SGPRs,    0 B LDS, no scratch, 8 waves per SIMD
// Open costs: nine small launches per round beside the scoring; the live list is rebuilt from all rows every round; the prefix of
// the block counts is re-summed by every block (cap / 256 integers each).
#include <cmath>

#include "device_utils.h"
#include "kernels.h"
#include "plane.h"
#include "svd3.h"

namespace dsir {

namespace {

constexpr int RB = kPlaneRowBlock, SL = kPlaneScoreLanes, CPL = kPlaneCandPerLane;
static_assert(RB == 256 && SL == 256 && kPlaneRefitSlice % 256 == 0, "the kernels below are written for 256-thread workgroups");

struct Axis { float x, y, z; int on; double cos_min; };

// the rule's step 3, one test
__device__ __forceinline__ bool plane_inlier(const float* c, float x, float y, float z, float thr) {
  const float e = ((c[0] * (x - c[3])) + (c[1] * (y - c[4]))) + (c[2] * (z - c[5]));
  return fabsf(e) < thr;
}
__device__ __forceinline__ bool axis_ok(const Axis& ax, double nx, double ny, double nz) {
  if (!ax.on) return true;
  const double dot = (nx * (double)ax.x + ny * (double)ax.y) + nz * (double)ax.z;
  return fabs(dot) >= ax.cos_min;
}

// COMPACT = false: blocks[c][b] = live rows of block b.  COMPACT = true: the live list and its packed copy.
template <bool COMPACT>
__global__ __launch_bounds__(RB) void plane_live_kernel(const float* __restrict__ pts, int64_t pts_cs, int pts_ld,
                                                        const int32_t* __restrict__ counts, int cap, const int32_t* __restrict__ labels,
                                                        const int32_t* __restrict__ done, int32_t* __restrict__ blocks,
                                                        int32_t* __restrict__ live, float4* __restrict__ pts4, int32_t* __restrict__ n_live) {
  __shared__ int32_t wave_cnt[RB / 64];
  __shared__ int32_t red[2][RB];
  const int cloud = blockIdx.y, b = blockIdx.x, t = threadIdx.x, nb = gridDim.x;
  if (done[cloud]) return;
  const int n = pair_rows(counts, cloud, cap);
  const int i = b * RB + t;
  float x = 0.f, y = 0.f, z = 0.f;
  bool keep = false;
  if (i < n && labels[(int64_t)cloud * cap + i] < 0) {
    const float* p = pts + (int64_t)cloud * pts_cs + (int64_t)i * pts_ld;
    x = p[0]; y = p[1]; z = p[2];
    keep = isfinite(x) && isfinite(y) && isfinite(z);
  }
  const unsigned long long m = __ballot(keep);
  if ((t & 63) == 0) wave_cnt[t >> 6] = (int32_t)__popcll(m);
  int32_t* bc = blocks + (int64_t)cloud * nb;
  if (!COMPACT) {
    __syncthreads();
    if (t == 0) bc[b] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    return;
  }
  int32_t before = 0, all = 0;                                 // integer sums: any order gives the same total
  for (int k = t; k < nb; k += RB) {
    const int32_t v = bc[k];
    all += v;
    if (k < b) before += v;
  }
  red[0][t] = before; red[1][t] = all;
  __syncthreads();
  for (int o = RB / 2; o > 0; o >>= 1) {
    if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; }
    __syncthreads();
  }
  int32_t pos = red[0][0] + (int32_t)__popcll(m & ((1ull << (t & 63)) - 1ull));
  for (int w = 0; w < (t >> 6); ++w) pos += wave_cnt[w];
  if (keep && pos < cap) {                                     // pos < total <= cap by construction
    live[(int64_t)cloud * cap + pos] = i;
    pts4[(int64_t)cloud * cap + pos] = make_float4(x, y, z, 0.f);
  }
  if (b == nb - 1 && t == 0) n_live[cloud] = red[1][0];
}

// one lane per hypothesis: draw, gather, fit, verdict.  hyp [clouds][H][6], hyp_ok / hyp_cnt [clouds][H] (the count zeroed here)
__global__ __launch_bounds__(kPlaneHypBlock) void plane_hyp_kernel(const float4* __restrict__ pts4, const int32_t* __restrict__ n_live,
                                                                   const int32_t* __restrict__ done, const int32_t* __restrict__ cloud_ids,
                                                                   int cap, int H, int round, uint64_t seed, Axis ax,
                                                                   float* __restrict__ hyp, int32_t* __restrict__ hyp_ok,
                                                                   int32_t* __restrict__ hyp_cnt) {
  const int cloud = blockIdx.y;
  const int h = blockIdx.x * kPlaneHypBlock + threadIdx.x;
  if (h >= H || done[cloud]) return;
  const int n = n_live[cloud];
  const uint64_t key = plane_cloud_key(seed, cloud_ids ? (uint32_t)cloud_ids[cloud] : (uint32_t)cloud);
  uint32_t r[3];
  for (int k = 0; k < 3; ++k) r[k] = plane_draw(key, round, h, k, (uint32_t)(n > 0 ? n : 0));
  bool ok = n >= 3 && r[0] != r[1] && r[0] != r[2] && r[1] != r[2];
  float o[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (ok) {                                                    // r_k < n_live <= cap
    const float4* P = pts4 + (int64_t)cloud * cap;
    const float4 a = P[r[0]], b = P[r[1]], c = P[r[2]];
    const double ux = (double)b.x - (double)a.x, uy = (double)b.y - (double)a.y, uz = (double)b.z - (double)a.z;
    const double vx = (double)c.x - (double)a.x, vy = (double)c.y - (double)a.y, vz = (double)c.z - (double)a.z;
    const double mx = uy * vz - uz * vy, my = uz * vx - ux * vz, mz = ux * vy - uy * vx;
    const double len2 = (mx * mx + my * my) + mz * mz;
    ok = len2 > 0.0 && isfinite(len2);
    if (ok) {
      const double s = sqrt(len2);
      const double nx = mx / s, ny = my / s, nz = mz / s;
      ok = axis_ok(ax, nx, ny, nz);
      if (ok) { o[0] = (float)nx; o[1] = (float)ny; o[2] = (float)nz; o[3] = a.x; o[4] = a.y; o[5] = a.z; }
    }
  }
  const int64_t s = (int64_t)cloud * H + h;
  for (int k = 0; k < 6; ++k) hyp[s * 6 + k] = o[k];
  hyp_ok[s] = ok ? 1 : 0;
  hyp_cnt[s] = 0;
}

// Inlier counts of H candidates per cloud over the live rows.  cand [clouds][H][6], ok / out [clouds][H]: with H = 1 the same kernel
// recounts a refit.  grid (candidate blocks of 512, slices, clouds); a slice is cps chunks of 256 live points.  out is zeroed by
// whoever wrote the candidates.
__global__ __launch_bounds__(SL) void plane_score_kernel(const float4* __restrict__ pts4, const int32_t* __restrict__ n_live,
                                                         const int32_t* __restrict__ done, int cap, const float* __restrict__ cand,
                                                         const int32_t* __restrict__ ok, int H, int cps, float thr,
                                                         int32_t* __restrict__ out) {
  __shared__ float4 sP[SL];
  const int cloud = blockIdx.z, tid = threadIdx.x;
  if (done[cloud]) return;
  const int n = min(n_live[cloud], cap);
  const int begin = blockIdx.y * cps * SL;
  const int end = min(n, begin + cps * SL);
  if (begin >= end) return;                                    // block-uniform: the slice lies beyond the cloud's live rows
  float c[CPL][6];
  bool good[CPL];
  int64_t slot[CPL];
  bool any = false;
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int h = (blockIdx.x * CPL + q) * SL + tid;
    slot[q] = (int64_t)cloud * H + (h < H ? h : 0);
    good[q] = h < H && ok[slot[q]] != 0;
    any = any || good[q];
#pragma unroll
    for (int k = 0; k < 6; ++k) c[q][k] = good[q] ? cand[slot[q] * 6 + k] : 0.f;
  }
  if (!__syncthreads_or(any ? 1 : 0)) return;                  // block-uniform: nothing to score here
  const bool wave_any = __ballot(any) != 0ull;                 // a wholly rejected wave stages its share and skips the tests
  const float4* P = pts4 + (int64_t)cloud * cap;
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (begin + tid < end) r = P[begin + tid];
  int cnt[CPL];
#pragma unroll
  for (int q = 0; q < CPL; ++q) cnt[q] = 0;
  for (int c0 = begin; c0 < end; c0 += SL) {
    sP[tid] = r;
    __syncthreads();
    const int nx = c0 + SL + tid;                              // the next chunk's loads fly while this one is consumed
    if (nx < end) r = P[nx];
    const int m = min(SL, end - c0);
    if (wave_any) {
#pragma unroll 4
      for (int j = 0; j < m; ++j) {
        const float4 a = sP[j];
#pragma unroll
        for (int q = 0; q < CPL; ++q) cnt[q] += plane_inlier(c[q], a.x, a.y, a.z, thr) ? 1 : 0;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < CPL; ++q)
    if (good[q] && cnt[q]) atomicAdd(out + slot[q], cnt[q]);
}

// per cloud: the valid hypothesis with the largest count, ties to the lower h; the stop; the state of the refit rounds
__global__ __launch_bounds__(256) void plane_pick_kernel(const float* __restrict__ hyp, const int32_t* __restrict__ hyp_ok,
                                                         const int32_t* __restrict__ hyp_cnt, int H, int min_inliers,
                                                         int32_t* __restrict__ done, int32_t* __restrict__ info,
                                                         int32_t* __restrict__ first_cnt, float* __restrict__ cur,
                                                         int32_t* __restrict__ cur_cnt, int32_t* __restrict__ kept) {
  __shared__ unsigned long long s_key[4];
  __shared__ int s_nv[4];
  const int cloud = blockIdx.x;
  if (done[cloud]) return;
  unsigned long long key = 0ull;
  int nv = 0;
  for (int h = threadIdx.x; h < H; h += 256) {
    if (hyp_ok[(int64_t)cloud * H + h]) {
      ++nv;
      const unsigned long long k = plane_pick_key((uint32_t)hyp_cnt[(int64_t)cloud * H + h], (uint32_t)h);
      key = k > key ? k : key;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long k = __shfl_xor(key, o);
    key = k > key ? k : key;
    nv += __shfl_xor(nv, o);
  }
  if ((threadIdx.x & 63) == 0) { s_key[threadIdx.x >> 6] = key; s_nv[threadIdx.x >> 6] = nv; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) { key = s_key[w] > key ? s_key[w] : key; nv += s_nv[w]; }
    const int count = (int)plane_key_count(key);
    if (key == 0ull || count < min_inliers) { done[cloud] = 1; return; }
    const int h = (int)plane_key_h(key);
    for (int k = 0; k < 6; ++k) cur[(int64_t)cloud * 6 + k] = hyp[((int64_t)cloud * H + h) * 6 + k];
    cur_cnt[cloud] = count; first_cnt[cloud] = count; kept[cloud] = 0;
    info[(int64_t)cloud * 2] = h; info[(int64_t)cloud * 2 + 1] = nv;
  }
}

// the slices of sum1 added in slice order: {count, centroid}
__device__ inline void plane_centroid(const double* __restrict__ s1, int used, double* out) {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < used; ++k)
    for (int q = 0; q < 4; ++q) s[q] += s1[(int64_t)k * 4 + q];
  out[0] = s[0];
  for (int q = 1; q < 4; ++q) out[q] = s[q] / s[0];
}

// PASS 1: sum1[c][slice] = {count, sum x, sum y, sum z} of the kept plane's inliers in the slice; PASS 2: sum2[c][slice] =
// {xx, xy, xz, yy, yz, zz} of their fp64 offsets from the centroid.  Position q of the live list: slice q / 4096, lane q % 256.
template <int PASS>
__global__ __launch_bounds__(256) void plane_refit_sum_kernel(const float4* __restrict__ pts4, const int32_t* __restrict__ n_live,
                                                              const int32_t* __restrict__ done, int cap, const float* __restrict__ cur,
                                                              float thr, int slices, double* __restrict__ sum1,
                                                              double* __restrict__ sum2) {
  constexpr int NV = PASS == 1 ? 4 : 6;
  __shared__ double sh[4 * NV + NV];
  __shared__ double cen[4];
  const int cloud = blockIdx.y, t = threadIdx.x;
  if (done[cloud]) return;
  const int n = min(n_live[cloud], cap);
  const int begin = blockIdx.x * kPlaneRefitSlice;
  if (begin >= n) return;                                      // block-uniform; the solve adds the slices below n alone
  const int end = min(n, begin + kPlaneRefitSlice);
  if (PASS == 2) {
    if (t == 0) plane_centroid(sum1 + (int64_t)cloud * slices * 4, (n + kPlaneRefitSlice - 1) / kPlaneRefitSlice, cen);
    __syncthreads();
  }
  float c[6];
  for (int k = 0; k < 6; ++k) c[k] = cur[(int64_t)cloud * 6 + k];
  const float4* P = pts4 + (int64_t)cloud * cap;
  double v[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = 0.0;
  for (int q = begin + t; q < end; q += 256) {
    const float4 p = P[q];
    if (!plane_inlier(c, p.x, p.y, p.z, thr)) continue;
    if (PASS == 1) {
      v[0] += 1.0; v[1] += (double)p.x; v[2] += (double)p.y; v[3] += (double)p.z;
    } else {
      const double dx = (double)p.x - cen[1], dy = (double)p.y - cen[2], dz = (double)p.z - cen[3];
      v[0] += dx * dx; v[1] += dx * dy; v[2] += dx * dz; v[3] += dy * dy; v[4] += dy * dz; v[5] += dz * dz;
    }
  }
  block_sum<4, NV>(v, sh);
  double* o = (PASS == 1 ? sum1 : sum2) + ((int64_t)cloud * slices + blockIdx.x) * NV;
  if (t < NV) o[t] = v[t];
}

// per cloud: slices in slice order -> covariance sums -> normal and anchor of the refit, its verdict; trial_cnt zeroed
__global__ __launch_bounds__(64) void plane_refit_solve_kernel(const int32_t* __restrict__ n_live, const int32_t* __restrict__ done, int cap,
                                                               int clouds, int slices, const double* __restrict__ sum1,
                                                               const double* __restrict__ sum2, Axis ax, float* __restrict__ trial,
                                                               int32_t* __restrict__ trial_ok, int32_t* __restrict__ trial_cnt) {
  const int cloud = blockIdx.x * 64 + threadIdx.x;
  if (cloud >= clouds || done[cloud]) return;
  const int n = min(n_live[cloud], cap);
  const int used = (n + kPlaneRefitSlice - 1) / kPlaneRefitSlice;
  double cen[4], s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  plane_centroid(sum1 + (int64_t)cloud * slices * 4, used, cen);
  for (int k = 0; k < used; ++k)
    for (int q = 0; q < 6; ++q) s[q] += sum2[((int64_t)cloud * slices + k) * 6 + q];
  const double A[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
  double U[3][3], S[3], V[3][3];
  svd3(A, U, S, V);
  const double nx = V[0][2], ny = V[1][2], nz = V[2][2];
  const float o[6] = {(float)nx, (float)ny, (float)nz, (float)cen[1], (float)cen[2], (float)cen[3]};
  bool ok = cen[0] >= 3.0 && axis_ok(ax, nx, ny, nz);
  for (int k = 0; k < 6; ++k) { ok = ok && isfinite(o[k]); trial[(int64_t)cloud * 6 + k] = o[k]; }
  ok = ok && (o[0] != 0.f || o[1] != 0.f || o[2] != 0.f);
  trial_ok[cloud] = ok ? 1 : 0;
  trial_cnt[cloud] = 0;
}

// the refit replaces the kept plane iff it is valid and counts at least as many
__global__ __launch_bounds__(64) void plane_refit_keep_kernel(const int32_t* __restrict__ done, int clouds, const float* __restrict__ trial,
                                                              const int32_t* __restrict__ trial_ok, const int32_t* __restrict__ trial_cnt,
                                                              float* __restrict__ cur, int32_t* __restrict__ cur_cnt,
                                                              int32_t* __restrict__ kept) {
  const int cloud = blockIdx.x * 64 + threadIdx.x;
  if (cloud >= clouds || done[cloud]) return;
  if (!trial_ok[cloud] || trial_cnt[cloud] < cur_cnt[cloud]) return;
  for (int k = 0; k < 6; ++k) cur[(int64_t)cloud * 6 + k] = trial[(int64_t)cloud * 6 + k];
  cur_cnt[cloud] = trial_cnt[cloud];
  kept[cloud] += 1;
}

// the kept plane's inliers take the label `round`; block 0 writes the round's output row
__global__ __launch_bounds__(RB) void plane_finish_kernel(const float4* __restrict__ pts4, const int32_t* __restrict__ live,
                                                          const int32_t* __restrict__ n_live, const int32_t* __restrict__ done, int cap,
                                                          int round, int max_planes, float thr, Axis ax, const float* __restrict__ cur,
                                                          const int32_t* __restrict__ cur_cnt, const int32_t* __restrict__ info,
                                                          const int32_t* __restrict__ first_cnt, const int32_t* __restrict__ kept,
                                                          int32_t* __restrict__ labels, int32_t* __restrict__ num_planes,
                                                          float* __restrict__ planes, float* __restrict__ anchors,
                                                          int32_t* __restrict__ plane_counts, int32_t* __restrict__ stats) {
  const int cloud = blockIdx.y;
  if (done[cloud]) return;
  const int n = min(n_live[cloud], cap);
  float c[6];
  for (int k = 0; k < 6; ++k) c[k] = cur[(int64_t)cloud * 6 + k];
  const int q = blockIdx.x * RB + threadIdx.x;
  if (q < n) {
    const float4 p = pts4[(int64_t)cloud * cap + q];
    const int row = live[(int64_t)cloud * cap + q];
    if (plane_inlier(c, p.x, p.y, p.z, thr) && row >= 0 && row < cap) labels[(int64_t)cloud * cap + row] = round;
  }
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double d = -(((double)c[0] * (double)c[3] + (double)c[1] * (double)c[4]) + (double)c[2] * (double)c[5]);
  const double s = ax.on ? ((double)c[0] * (double)ax.x + (double)c[1] * (double)ax.y) + (double)c[2] * (double)ax.z : d;
  const float first = c[0] != 0.f ? c[0] : (c[1] != 0.f ? c[1] : c[2]);
  const bool flip = s < 0.0 || (s == 0.0 && first < 0.f);
  // a product with -1 is the exact negation.  Kept free of branches on purpose: as `if (flip) { c[0] = -c[0]; ... }` the compiler
  // merged the tails of the two flip conditions and left c[2] un-negated on the exact-zero path (seen in the ISA and on the lattice case)
  const float sg = flip ? -1.f : 1.f;
  for (int k = 0; k < 3; ++k) {
    const float v = c[k] * sg;
    c[k] = v == 0.f ? 0.f : v;                                 // -0 is written as +0, in the normal and in d
  }
  d = d * (double)sg;
  if (d == 0.0) d = 0.0;
  const int64_t o = (int64_t)cloud * max_planes + round;
  planes[o * 4] = c[0]; planes[o * 4 + 1] = c[1]; planes[o * 4 + 2] = c[2]; planes[o * 4 + 3] = (float)d;
  anchors[o * 3] = c[3]; anchors[o * 3 + 1] = c[4]; anchors[o * 3 + 2] = c[5];
  plane_counts[o] = cur_cnt[cloud];
  stats[o * 4] = info[(int64_t)cloud * 2]; stats[o * 4 + 1] = info[(int64_t)cloud * 2 + 1];
  stats[o * 4 + 2] = first_cnt[cloud]; stats[o * 4 + 3] = kept[cloud];
  num_planes[cloud] = round + 1;
}

}  // namespace

size_t plane_scratch_bytes(int clouds, int cap, int H) { return PlaneLayout(clouds, cap, H).bytes; }

bool launch_segment_plane(const PlaneArgs& a, hipStream_t st) {
  const int C = a.clouds, cap = a.cap, H = a.H;
  if (!plane_shape_ok(C, cap, H) || a.max_planes < 1 || a.max_planes > kPlaneMaxPlanes || a.min_inliers < kPlaneMinInliers ||
      a.refine_iters < 0 || a.refine_iters > kPlaneMaxRefits || !(a.thr > 0.f) || !std::isfinite(a.thr))
    return false;
  if (!a.pts || !a.scratch || !a.labels || !a.num_planes || !a.planes || !a.anchors || !a.plane_counts || !a.stats) return false;
  const PlaneLayout lay(C, cap, H);
  void* s = a.scratch;
  float4* pts4 = at<float4>(s, lay.pts4);
  int32_t *live = at<int32_t>(s, lay.live), *blocks = at<int32_t>(s, lay.blocks), *n_live = at<int32_t>(s, lay.n_live);
  int32_t *done = at<int32_t>(s, lay.done), *hyp_ok = at<int32_t>(s, lay.hyp_ok), *hyp_cnt = at<int32_t>(s, lay.hyp_cnt);
  int32_t *info = at<int32_t>(s, lay.info), *first_cnt = at<int32_t>(s, lay.first_cnt), *cur_cnt = at<int32_t>(s, lay.cur_cnt);
  int32_t *trial_cnt = at<int32_t>(s, lay.trial_cnt), *trial_ok = at<int32_t>(s, lay.trial_ok), *kept = at<int32_t>(s, lay.kept);
  float *hyp = at<float>(s, lay.hyp), *cur = at<float>(s, lay.cur), *trial = at<float>(s, lay.trial);
  double *sum1 = at<double>(s, lay.sum1), *sum2 = at<double>(s, lay.sum2);
  Axis ax;
  ax.x = a.axis[0]; ax.y = a.axis[1]; ax.z = a.axis[2]; ax.cos_min = a.cos_min;
  ax.on = (a.axis[0] != 0.f || a.axis[1] != 0.f || a.axis[2] != 0.f) ? 1 : 0;

  const size_t rows = (size_t)C * cap, P = (size_t)C * a.max_planes;
  hipMemsetAsync(a.labels, 0xFF, rows * 4, st);                // -1
  hipMemsetAsync(a.num_planes, 0, (size_t)C * 4, st);
  hipMemsetAsync(a.planes, 0, P * 16, st);
  hipMemsetAsync(a.anchors, 0, P * 12, st);
  hipMemsetAsync(a.plane_counts, 0, P * 4, st);
  hipMemsetAsync(a.stats, 0, P * 16, st);
  hipMemsetAsync(done, 0, (size_t)C * 4, st);

  const dim3 grows((unsigned)lay.row_blocks, (unsigned)C), ghyp((unsigned)((H + kPlaneHypBlock - 1) / kPlaneHypBlock), (unsigned)C);
  const int hb = plane_hyp_blocks(H), cps = plane_chunks_per_slice(cap, hb, C), cps1 = plane_chunks_per_slice(cap, 1, C);
  const dim3 gscore((unsigned)hb, (unsigned)plane_score_slices(cap, cps), (unsigned)C);
  const dim3 gscore1(1u, (unsigned)plane_score_slices(cap, cps1), (unsigned)C);
  const dim3 gsum((unsigned)lay.slices, (unsigned)C), gcloud((unsigned)((C + 63) / 64));
  for (int j = 0; j < a.max_planes; ++j) {
    hipLaunchKernelGGL(plane_live_kernel<false>, grows, dim3(RB), 0, st, a.pts, a.pts_cs, a.pts_ld, a.counts, cap, (const int32_t*)a.labels,
                       (const int32_t*)done, blocks, live, pts4, n_live);
    hipLaunchKernelGGL(plane_live_kernel<true>, grows, dim3(RB), 0, st, a.pts, a.pts_cs, a.pts_ld, a.counts, cap, (const int32_t*)a.labels,
                       (const int32_t*)done, blocks, live, pts4, n_live);
    hipLaunchKernelGGL(plane_hyp_kernel, ghyp, dim3(kPlaneHypBlock), 0, st, (const float4*)pts4, (const int32_t*)n_live, (const int32_t*)done,
                       a.cloud_ids, cap, H, j, a.seed, ax, hyp, hyp_ok, hyp_cnt);
    hipLaunchKernelGGL(plane_score_kernel, gscore, dim3(SL), 0, st, (const float4*)pts4, (const int32_t*)n_live, (const int32_t*)done, cap,
                       (const float*)hyp, (const int32_t*)hyp_ok, H, cps, a.thr, hyp_cnt);
    hipLaunchKernelGGL(plane_pick_kernel, dim3((unsigned)C), dim3(256), 0, st, (const float*)hyp, (const int32_t*)hyp_ok,
                       (const int32_t*)hyp_cnt, H, a.min_inliers, done, info, first_cnt, cur, cur_cnt, kept);
    for (int r = 0; r < a.refine_iters; ++r) {
      hipLaunchKernelGGL(plane_refit_sum_kernel<1>, gsum, dim3(256), 0, st, (const float4*)pts4, (const int32_t*)n_live, (const int32_t*)done,
                         cap, (const float*)cur, a.thr, lay.slices, sum1, sum2);
      hipLaunchKernelGGL(plane_refit_sum_kernel<2>, gsum, dim3(256), 0, st, (const float4*)pts4, (const int32_t*)n_live, (const int32_t*)done,
                         cap, (const float*)cur, a.thr, lay.slices, sum1, sum2);
      hipLaunchKernelGGL(plane_refit_solve_kernel, gcloud, dim3(64), 0, st, (const int32_t*)n_live, (const int32_t*)done, cap, C, lay.slices,
                         (const double*)sum1, (const double*)sum2, ax, trial, trial_ok, trial_cnt);
      hipLaunchKernelGGL(plane_score_kernel, gscore1, dim3(SL), 0, st, (const float4*)pts4, (const int32_t*)n_live, (const int32_t*)done, cap,
                         (const float*)trial, (const int32_t*)trial_ok, 1, cps1, a.thr, trial_cnt);
      hipLaunchKernelGGL(plane_refit_keep_kernel, gcloud, dim3(64), 0, st, (const int32_t*)done, C, (const float*)trial,
                         (const int32_t*)trial_ok, (const int32_t*)trial_cnt, cur, cur_cnt, kept);
    }
    hipLaunchKernelGGL(plane_finish_kernel, grows, dim3(RB), 0, st, (const float4*)pts4, (const int32_t*)live, (const int32_t*)n_live,
                       (const int32_t*)done, cap, j, a.max_planes, a.thr, ax, (const float*)cur, (const int32_t*)cur_cnt,
                       (const int32_t*)info, (const int32_t*)first_cnt, (const int32_t*)kept, a.labels, a.num_planes, a.planes, a.anchors,
                       a.plane_counts, a.stats);
  }
  return true;
}

}  // namespace dsir
