// Pose from a correspondence list: the front and the tail that ransac.hip, consensus.hip and fgr.hip share, and the rule of both.
// A stage is front -> MIDDLE -> tail: only the middle - how the candidate poses come about - is the stage's own, stated in its file's
// header.  Parity is UNPINNED (open3d cannot be imported): the rule is stated here once and restated in deepsir_amd/ransac.py.
//
// THE SHARED RULE.  Per pair p: points_src [J][stride], points_ref [K][stride] (xyz first), corr [M][2] int32 (src index, ref index),
// count = counts[p] clamped to [0, M] (counts == NULL: M).
//   front: indices are clamped into range; a clamp of a live row raises bit 2 of invalid[p].  The matched points are gathered once,
//       s_i = src[corr_i0], q_i = ref[corr_i1]; a row that holds a non-finite coordinate, and every row >= count, is PARKED at s = 0,
//       q = FLT_MAX (all three): finite, so it adds exact zeros to a refit at weight 0, and never an inlier (its squared residual
//       overflows to +inf under every pose a middle can produce).
//   middle: H candidate poses T_h [3][4] fp32 with a verdict valid_h each.
//   residual, fp32, every operation rounded on its own except where se3_row (device_utils.h) fuses (pose_d2, pose_corr.h):
//       c_r = se3_row(T, r, s) = fma(z, T_r2, fma(y, T_r1, x T_r0)) + T_r3;   d = c - q;   d2 = (dx dx + dy dy) + dz dz
//   score: the INTEGER count of live rows with d2 < thr^2, thr^2 = max_dist * max_dist in fp32 (corr_thr2).  Winner: the valid
//       candidate with the largest count, ties to the lower h - integers, so the winner cannot depend on the order workgroups arrive in.
//   refit, refine_iters rounds: T_{r+1} = Kabsch(all inliers of T_r) through launch_kabsch with 0/1 weights on the gathered points,
//       recount; the result is the LAST element with the largest count of T_0 .. T_r: a refit that keeps the count replaces the pose
//       of a small sample by the fit of all its inliers (which makes the tie-break above irrelevant), one that loses inliers is dropped.
//   finish: T_out, stats {fitness = inliers / count, inlier RMSE (the fp32 residuals summed in float64 in a fixed order), winning h
//       or -1, valid candidates, inliers}.  No valid candidate: T_out = T_init (identity if NULL), stats {0, 0, -1, 0, 0}: no error.
//
// KERNELS.  pose_gather_kernel (clamp, flag, gather, park) -> the middle -> pose_score_kernel (the hot path: a workgroup owns 256
// candidates, one per lane with its T in 12 registers, and a slice of the correspondences staged through LDS in chunks of
// DSIR_RANSAC_CHUNK; every lane reads the SAME LDS address each step - a broadcast, no bank conflict - laid out as one 16-byte
// {sx, sy, sz, qx} and one 8-byte {qy, qz} read; the next chunk's global loads are issued before the current chunk is consumed;
// per-lane integer counters end in one integer atomicAdd per candidate and slice: exact, so order cannot matter) ->
// pose_pick_kernel (max of count << 32 | (0xFFFFFFFF - h)) -> per round pose_weights_kernel, launch_kabsch, the scoring kernel with
// H = 1 -> pose_finish_kernel.  No host synchronisation between them, nothing allocated.
// No MFMA form of the scoring: d2 as a bilinear form <phi(h), psi(i)> cancels terms of 1e2..1e4 m^2 against thresholds of
// 1e-3..1e-1 m^2 in fp32 and would give up the exact counts.
//
// corr_compact_kernel PRODUCES such lists: the mutual-nearest-neighbour list of dsir_feature_correspondences - one workgroup per
// pair, ballot + LDS block scan in ascending src index, no atomics: the same bytes every run.
#include <cfloat>

#include "kernels.h"
#include "device_utils.h"
#include "pose_corr.h"
#include "dsir.h"

namespace dsir {

namespace {

constexpr int CH = DSIR_RANSAC_CHUNK;   // correspondences per LDS chunk
constexpr int SB = 256;                 // hypotheses per scoring workgroup (one per lane)
static_assert(CH == SB, "a scoring workgroup stages one correspondence per thread and chunk");

// cs / cq [P][M][3]: the matched points, gathered once; dead rows (>= count) and rows with a non-finite coordinate are parked
__global__ __launch_bounds__(256) void pose_gather_kernel(const float* __restrict__ src, const float* __restrict__ ref, int J, int K,
                                                          int stride, const int32_t* __restrict__ corr,
                                                          const int32_t* __restrict__ counts, int M, float* __restrict__ cs,
                                                          float* __restrict__ cq, int32_t* __restrict__ invalid) {
  const int pair = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const int count = live_count(counts, pair, M);
  float s[3] = {0.f, 0.f, 0.f}, q[3] = {FLT_MAX, FLT_MAX, FLT_MAX};
  if (i < count) {
    const int a = corr[((int64_t)pair * M + i) * 2], b = corr[((int64_t)pair * M + i) * 2 + 1];
    const int ac = min(max(a, 0), J - 1), bc = min(max(b, 0), K - 1);
    if (ac != a || bc != b) atomicOr(invalid + pair, 2);   // idempotent: the flag does not depend on who arrives first
    const float* ps = src + ((int64_t)pair * J + ac) * stride;
    const float* pq = ref + ((int64_t)pair * K + bc) * stride;
    const float v[6] = {ps[0], ps[1], ps[2], pq[0], pq[1], pq[2]};
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) fin = fin && isfinite(v[k]);
    if (fin) { s[0] = v[0]; s[1] = v[1]; s[2] = v[2]; q[0] = v[3]; q[1] = v[4]; q[2] = v[5]; }
  }
  float* os = cs + ((int64_t)pair * M + i) * 3;
  float* oq = cq + ((int64_t)pair * M + i) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) { os[k] = s[k]; oq[k] = q[k]; }
}

// Inlier counts of H transforms per pair over the live correspondences.  T [P][H][12], valid / out [P][H]: with H = 1 the same
// kernel recounts the one refitted transform of every pair.
// grid (hypothesis blocks, slices, pairs); a slice is cps chunks of CH correspondences.  out is zeroed by the caller.
__global__ __launch_bounds__(SB) void pose_score_kernel(const float* __restrict__ cs, const float* __restrict__ cq,
                                                        const int32_t* __restrict__ counts, int M, const float* __restrict__ T,
                                                        const int32_t* __restrict__ valid, int H, int cps,
                                                        float thr2, int32_t* __restrict__ out) {
  __shared__ float4 sA[CH];   // {sx, sy, sz, qx}: one ds_read_b128
  __shared__ float2 sB[CH];   // {qy, qz}:         one ds_read_b64
  const int pair = blockIdx.z, tid = threadIdx.x;
  const int h = blockIdx.x * SB + tid;
  const int count = live_count(counts, pair, M);
  const int begin = blockIdx.y * cps * CH;
  const int end = min(count, begin + cps * CH);
  if (begin >= end) return;                                   // block-uniform: the slice lies beyond the pair's live rows
  const bool ok = h < H && valid[(int64_t)pair * H + h] != 0;
  if (!__syncthreads_or(ok ? 1 : 0)) return;                  // block-uniform: nothing to score here
  const bool wave_ok = __ballot(ok) != 0ull;                  // a wholly rejected wave stages its share and skips the products
  float t[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) t[k] = ok ? T[((int64_t)pair * H + h) * 12 + k] : 0.f;
  const float* S = cs + (int64_t)pair * M * 3;
  const float* Q = cq + (int64_t)pair * M * 3;
  float r[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (begin + tid < end) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { r[k] = S[(int64_t)(begin + tid) * 3 + k]; r[3 + k] = Q[(int64_t)(begin + tid) * 3 + k]; }
  }
  int cnt = 0;
  for (int c0 = begin; c0 < end; c0 += CH) {
    sA[tid] = make_float4(r[0], r[1], r[2], r[3]);
    sB[tid] = make_float2(r[4], r[5]);
    __syncthreads();
    const int nx = c0 + CH + tid;                             // the next chunk's loads fly while this one is consumed
    if (nx < end) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { r[k] = S[(int64_t)nx * 3 + k]; r[3 + k] = Q[(int64_t)nx * 3 + k]; }
    }
    const int m = min(CH, end - c0);
    if (wave_ok) {
#pragma unroll 4
      for (int j = 0; j < m; ++j) {
        const float4 a = sA[j];
        const float2 b = sB[j];
        cnt += pose_d2(t, a.x, a.y, a.z, a.w, b.x, b.y) < thr2 ? 1 : 0;
      }
    }
    __syncthreads();
  }
  if (ok && cnt) atomicAdd(out + (int64_t)pair * H + h, cnt);
}

// per pair: the valid hypothesis with the largest count, ties to the lower h; state of the refit rounds.
// Tcand [R+1][P][12], cnt [R+1][P], info [4][P] = {winning h or -1, valid hypotheses, found, skip (= !found, for launch_kabsch)}
__global__ __launch_bounds__(256) void pose_pick_kernel(const float* __restrict__ hyp_T, const int32_t* __restrict__ hyp_valid,
                                                        const int32_t* __restrict__ hyp_count, int H,
                                                        const float* __restrict__ T_init, float* __restrict__ Tcand,
                                                        int P, int32_t* __restrict__ cnt, int32_t* __restrict__ info) {
  __shared__ unsigned long long s_key[4];
  __shared__ int s_nv[4];
  const int pair = blockIdx.x;
  unsigned long long key = 0ull;
  int nv = 0;
  for (int h = threadIdx.x; h < H; h += 256) {
    if (hyp_valid[(int64_t)pair * H + h]) {
      ++nv;
      const unsigned long long k = ((unsigned long long)(uint32_t)hyp_count[(int64_t)pair * H + h] << 32) | (0xFFFFFFFFu - (uint32_t)h);
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
    const bool found = key != 0ull;                           // a valid hypothesis has h < 2^32 - 1: its key is never 0
    const int h = found ? (int)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull)) : -1;
    info[pair] = h; info[P + pair] = nv; info[2 * P + pair] = found ? 1 : 0; info[3 * P + pair] = found ? 0 : 1;
    cnt[pair] = found ? (int32_t)(key >> 32) : 0;
    const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    for (int k = 0; k < 12; ++k)
      Tcand[(int64_t)pair * 12 + k] = found ? hyp_T[((int64_t)pair * H + h) * 12 + k] : (T_init ? T_init[(int64_t)pair * 12 + k] : I[k]);
  }
}

// the 0/1 inlier weights of T for the refit, w [P][M] (rows >= count: 0)
__global__ __launch_bounds__(256) void pose_weights_kernel(const float* __restrict__ cs, const float* __restrict__ cq,
                                                           const int32_t* __restrict__ counts, int M, const float* __restrict__ T,
                                                           float thr2, float* __restrict__ w) {
  const int pair = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const float* t = T + (int64_t)pair * 12;
  const float* s = cs + ((int64_t)pair * M + i) * 3;
  const float* q = cq + ((int64_t)pair * M + i) * 3;
  const bool in = i < live_count(counts, pair, M) && pose_d2(t, s[0], s[1], s[2], q[0], q[1], q[2]) < thr2;
  w[(int64_t)pair * M + i] = in ? 1.f : 0.f;
}

// per pair: the last largest count of T_0 .. T_R, its transform, and the stats row (inlier RMSE: the fp32 residuals summed in
// float64 in a fixed order)
__global__ __launch_bounds__(256) void pose_finish_kernel(const float* __restrict__ cs, const float* __restrict__ cq,
                                                          const int32_t* __restrict__ counts, int M, int P, int R,
                                                          const float* __restrict__ Tcand, const int32_t* __restrict__ cnt,
                                                          const int32_t* __restrict__ info, float thr2, float* __restrict__ T_out,
                                                          double* __restrict__ stats) {
  __shared__ double sh[4 * 2 + 2];
  const int pair = blockIdx.x;
  const int count = live_count(counts, pair, M);
  const bool found = info[2 * P + pair] != 0;
  int best = 0;
  for (int r = 1; r <= R; ++r)
    if (cnt[(int64_t)r * P + pair] >= cnt[(int64_t)best * P + pair]) best = r;
  if (!found) best = 0;
  const float* t = Tcand + ((int64_t)best * P + pair) * 12;
  double v[2] = {0.0, 0.0};
  if (found)
    for (int i = threadIdx.x; i < count; i += 256) {
      const float* s = cs + ((int64_t)pair * M + i) * 3;
      const float* q = cq + ((int64_t)pair * M + i) * 3;
      const float d2 = pose_d2(t, s[0], s[1], s[2], q[0], q[1], q[2]);
      if (d2 < thr2) { v[0] += 1.0; v[1] += (double)d2; }
    }
  block_sum<4>(v, sh);
  if (threadIdx.x == 0) {
    for (int k = 0; k < 12; ++k) T_out[(int64_t)pair * 12 + k] = t[k];
    double* o = stats + (int64_t)pair * 5;
    o[0] = found && count > 0 ? v[0] / (double)count : 0.0;
    o[1] = v[0] > 0.0 ? sqrt(v[1] / v[0]) : 0.0;
    o[2] = (double)info[pair];
    o[3] = (double)info[P + pair];
    o[4] = v[0];
  }
}

// mutual-nearest-neighbour list: row j of the pair survives when mutual == 0 or ba[ab[j]] == j; survivors in ascending j,
// corr [P][J][2] = (j, ab[j]), rows beyond counts[p] = -1
__global__ __launch_bounds__(256) void corr_compact_kernel(const int32_t* __restrict__ ab, const int32_t* __restrict__ ba, int J, int K,
                                                           int mutual, int32_t* __restrict__ corr, int32_t* __restrict__ counts) {
  __shared__ int wt[4];
  const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int32_t* A = ab + (int64_t)pair * J;
  const int32_t* B = ba + (int64_t)pair * K;
  int32_t* out = corr + (int64_t)pair * J * 2;
  int base = 0;
  for (int j0 = 0; j0 < J; j0 += 256) {
    const int j = j0 + tid;
    int k = 0;
    bool keep = false;
    if (j < J) {
      k = min(max(A[j], 0), K - 1);
      keep = !mutual || B[k] == j;
    }
    const unsigned long long bal = __ballot(keep);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wt[w] = __popcll(bal);
    __syncthreads();
    int off = base;
    for (int ww = 0; ww < w; ++ww) off += wt[ww];
    if (keep) { out[(int64_t)(off + before) * 2] = j; out[(int64_t)(off + before) * 2 + 1] = k; }
    base += wt[0] + wt[1] + wt[2] + wt[3];
    __syncthreads();
  }
  for (int i = base + tid; i < J; i += 256) { out[(int64_t)i * 2] = -1; out[(int64_t)i * 2 + 1] = -1; }
  if (tid == 0) counts[pair] = base;
}

// slices of a scoring launch: at least two workgroups per CU where the problem allows it, whole chunks per slice
inline int chunks_per_slice(int M, int hyp_blocks, int pairs) {
  const int nch = (M + CH - 1) / CH;
  const int64_t wgs = (int64_t)hyp_blocks * pairs;
  int want = (int)((512 + wgs - 1) / wgs);
  want = want < 1 ? 1 : (want > nch ? nch : want);
  return (nch + want - 1) / want;
}

void launch_score(const float* cs, const float* cq, const int32_t* counts, int pairs, int M, const float* T, const int32_t* valid,
                  int H, float thr2, int32_t* out, hipStream_t st) {
  const int hb = (H + SB - 1) / SB;
  const int cps = chunks_per_slice(M, hb, pairs);
  const int nch = (M + CH - 1) / CH;
  const dim3 grid(hb, (nch + cps - 1) / cps, pairs);
  hipLaunchKernelGGL(pose_score_kernel, grid, dim3(SB), 0, st, cs, cq, counts, M, T, valid, H, cps, thr2, out);
}

}  // namespace

void launch_pose_front(const CorrProblem& p, const PoseParts& s, hipStream_t st) {
  hipMemsetAsync(p.invalid, 0, (size_t)p.pairs * 4, st);
  hipLaunchKernelGGL(pose_gather_kernel, dim3((p.M + 255) / 256, p.pairs), dim3(256), 0, st, p.src, p.ref, p.J, p.K, p.stride, p.corr,
                     p.counts, p.M, s.cs, s.cq, p.invalid);
}

void launch_pose_tail(const CorrProblem& p, const PoseParts& s, const CandSet& c, hipStream_t st) {
  const int P = p.pairs, M = p.M, H = c.H, R = p.refine_iters;
  const float thr2 = corr_thr2(p);
  const dim3 gm((M + 255) / 256, P);
  hipMemsetAsync(c.count, 0, (size_t)P * H * 4, st);
  hipMemsetAsync(s.cnt, 0, (size_t)P * (R + 1) * 4, st);
  launch_score(s.cs, s.cq, p.counts, P, M, c.T, c.valid, H, thr2, c.count, st);
  hipLaunchKernelGGL(pose_pick_kernel, dim3(P), dim3(256), 0, st, c.T, c.valid, c.count, H, p.T_init, s.Tcand, P, s.cnt, s.info);
  for (int r = 0; r < R; ++r) {
    float* Tr = s.Tcand + (size_t)r * P * 12;
    float* Tn = s.Tcand + (size_t)(r + 1) * P * 12;
    hipLaunchKernelGGL(pose_weights_kernel, gm, dim3(256), 0, st, s.cs, s.cq, p.counts, M, Tr, thr2, s.w);
    KabschArgs k{};
    k.src = s.cs; k.ref = s.cq; k.idx = nullptr; k.w = s.w; k.src_stride = (int64_t)M * 3; k.ref_stride = (int64_t)M * 3;
    k.sigmoid = 0; k.pairs = P; k.m = M; k.T = Tn; k.invalid = nullptr;
    k.skip = s.info + 3 * P;   // a pair without a valid candidate: identity step, and its recount is gated by `found`
    launch_kabsch(k, st);
    launch_score(s.cs, s.cq, p.counts, P, M, Tn, s.info + 2 * P, 1, thr2, s.cnt + (size_t)(r + 1) * P, st);
  }
  hipLaunchKernelGGL(pose_finish_kernel, dim3(P), dim3(256), 0, st, s.cs, s.cq, p.counts, M, P, R, s.Tcand, s.cnt, s.info, thr2, p.T_out,
                     p.stats);
}

void copy_candidates(const CandSet& c, int pairs, float* T, int32_t* valid, int32_t* count, hipStream_t st) {
  const size_t n = (size_t)pairs * c.H;
  if (T) hipMemcpyAsync(T, c.T, n * 48, hipMemcpyDeviceToDevice, st);
  if (valid) hipMemcpyAsync(valid, c.valid, n * 4, hipMemcpyDeviceToDevice, st);
  if (count) hipMemcpyAsync(count, c.count, n * 4, hipMemcpyDeviceToDevice, st);
}

void launch_corr_compact(const int32_t* ab, const int32_t* ba, int pairs, int J, int K, int mutual, int32_t* corr, int32_t* counts,
                         hipStream_t st) {
  hipLaunchKernelGGL(corr_compact_kernel, dim3(pairs), dim3(256), 0, st, ab, ba, J, K, mutual, corr, counts);
}

}  // namespace dsir
