// ISS keypoints (intrinsic shape signatures; open3d compute_iss_keypoints, Zhong ICCV-W 2009) from two CSR neighbour lists of a dense
// cloud batch: dsir_iss_keypoints (include/dsir.h), Engine.iss_keypoints.  open3d cannot be imported here, so parity is unpinned and
// THE RULE IS OWNED HERE; deepsir_amd/iss.py restates it in numpy (iss_saliency_host, iss_select_host, iss_keypoints_host).
//
// ---- THE RULE.  Inputs: points [clouds][n][stride >= 3] fp32; a salient CSR and a non-max CSR, each (offsets [clouds n + 1] i32, cols
// i32) with cloud-local columns, ascending per row, self included (what dsir_t_nn_radius_fill writes, what dsir_fpfh and
// dsir_estimate_normals_csr take); gamma_21, gamma_32 (fp64), min_neighbors.  A column index is clamped into [0, n - 1] before any use.
//   Stage 1, saliency of point i whose salient row has cnt entries q_0 .. q_(cnt - 1) (row order):
//     cnt < min_neighbors:  s_i = 0
//     m = (sum_k (double)q_k) / cnt;   C = (sum_k (q_k - m)(q_k - m)^T) / cnt      fp64, the six entries of the upper triangle, mirrored
//       SUMMATION ORDER (part of the rule): the row is dealt to kGroup = 16 lanes, lane l takes entries l, l + 16, l + 32, ... and adds
//       them in ascending order from +0; the 16 partials of every quantity meet in an xor butterfly with partners 1, 2, 4, 8 in that
//       order (a = a + partner's a; IEEE addition commutes, so the 16 lanes hold the same bits after every step).  The mean's three sums
//       are complete and divided by cnt before the first covariance term is formed: two passes over the row, (q_k - m) one fp64
//       subtraction, every product and sum rounded once (no contraction).  The six totals are divided by cnt after the butterfly.
//       Nothing in this depends on the launch, the batch or on timing.
//     an entry of C is not finite, or all are zero:  s_i = 0
//     (e1 >= e2 >= e3) = S of svd3(C) (svd3.h: for a symmetric PSD matrix the singular values are the eigenvalues)
//     e1 > 0, e2 > 0, e2 / e1 < gamma_21 and e3 / e2 < gamma_32 (fp64 divisions, strict):  s_i = (float)e3, rounded once;  else s_i = 0
//     (a value that rounds to 0.0f is thereby no candidate)
//   Stage 2, selection of point i with non-max row R_i: i is a keypoint iff  s_i > 0,  |R_i| >= min_neighbors,  no j in R_i has
//     s_j > s_i,  and no j in R_i has s_j == s_i with j < i.  The tie clause is a departure from open3d, which keeps both points of a
//     tie: exact duplicate points have identical rows, hence identical saliency bits, and yield ONE keypoint here, the lower index.
//   Outputs: saliency [clouds][n] f32, mask [clouds][n] i32 (0 / 1), index [clouds][n] i32: the cloud's keypoints in ascending point
//     index, -1 beyond its count, counts [clouds] i32.
//
// ---- Kernel shapes.
// iss_saliency_kernel: a group of 16 lanes per point, 16 points per 256-thread workgroup, grid (ceil(n / 16), clouds).  Why 16: the
//   salient rows at 6 x resolution hold on the order of a hundred entries (a disc of radius 6 cells on a surface: ~113) with a wide
//   spread (borders, density).  One lane per point (normal_of_list's shape) chains ~100 dependent gathered loads per lane twice and
//   diverges on the row length.  A whole wave per row leaves 3/4 of its lanes idle on the 16-entry rows near a border, pays six
//   butterfly steps on nine fp64 values and still parks 63 lanes during the svd3.  8 lanes: 13+ dependent loads per pass on a 100-entry
//   row.  16 lanes: 7 loads per lane per pass on such a row, one partly filled trip on anything up to 16, four butterfly steps, four
//   points per wave so four lanes run the svd3 side by side, and a group's 16 consecutive column reads share cache lines.  The second pass
//   re-reads the row (cache hits) instead of holding it in registers, as normal_of_list does.  The covariance body is written again
//   here, not factored out of ppf.hip: normal_of_list is a one-lane serial sum whose order is the normals' rule, this one is a
//   16-lane partition with another order; sharing the few lines would tie two rules together for no saved work.
// iss_select_kernel: one lane per point, grid (ceil(n / 256), clouds): the row scan over the fp32 saliencies with early exit, the
//   mask, and the workgroup's keypoint count by ballot + popcount.  iss_compact_kernel, same grid: the workgroup's base = the counts of
//   the workgroups before it in its cloud (added in workgroup order), ranks by wave ballots in row order, index written; rows at and
//   past the cloud's total get -1, the last workgroup writes counts.  This is crop.hip's compaction shape, written again locally:
//   crop's two kernels rank `kept(key, mode, key_lo)` over slices of 2048 rows of a ragged cloud and copy whole rows, all of it tied to
//   its CropState; a shared body would have to take the predicate, the slice and the payload as parameters and crop.hip would be
//   rebuilt around it, with its tests' bytes at stake for ~25 lines.
// No atomics anywhere: the same bytes on every run, and for a cloud alone or inside a batch (a cloud's workgroups read that cloud only).
#include "device_utils.h"
#include "kernels.h"
#include "svd3.h"

namespace dsir {

namespace {

constexpr int kGroup = 16;                  // lanes per salient row
constexpr int kSalPts = 256 / kGroup;       // points per workgroup of the saliency kernel
constexpr int kSelT = 256;                  // threads (= points) per workgroup of the selection and the compaction

__device__ __forceinline__ double group_sum(double a) {
  a += __shfl_xor(a, 1); a += __shfl_xor(a, 2); a += __shfl_xor(a, 4); a += __shfl_xor(a, 8);
  return a;
}

__global__ __launch_bounds__(256) void iss_saliency_kernel(const float* __restrict__ pts, int64_t pts_cs, int stride,
                                                           const int32_t* __restrict__ offsets, const int32_t* __restrict__ cols, int n,
                                                           double gamma_21, double gamma_32, int min_neighbors, float* __restrict__ saliency) {
  const int cloud = blockIdx.y;
  const int i = blockIdx.x * kSalPts + (int)(threadIdx.x / kGroup), l = threadIdx.x % kGroup;
  const bool live = i < n;                  // uniform over a group; every lane of the wave runs the butterflies
  const int64_t r = (int64_t)cloud * n + (live ? i : 0);
  const int b = offsets[r];
  int cnt = live ? max(offsets[r + 1] - b, 0) : 0;
  if (cnt < min_neighbors) cnt = 0;         // s = 0 without reading the row
  const float* P = pts + cloud * pts_cs;
  const int32_t* nb = cols + b;
  double m[3] = {0.0, 0.0, 0.0};
  for (int k = l; k < cnt; k += kGroup) {
    const int j = min(max(nb[k], 0), n - 1);
    for (int a = 0; a < 3; ++a) m[a] += (double)P[(int64_t)j * stride + a];
  }
  const double dc = (double)(cnt > 0 ? cnt : 1);
  for (int a = 0; a < 3; ++a) m[a] = group_sum(m[a]) / dc;
  double c6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // xx xy xz yy yz zz
  for (int k = l; k < cnt; k += kGroup) {             // the row a second time: cache hits
    const int j = min(max(nb[k], 0), n - 1);
    double e[3];
    for (int a = 0; a < 3; ++a) e[a] = (double)P[(int64_t)j * stride + a] - m[a];
    c6[0] += e[0] * e[0]; c6[1] += e[0] * e[1]; c6[2] += e[0] * e[2];
    c6[3] += e[1] * e[1]; c6[4] += e[1] * e[2]; c6[5] += e[2] * e[2];
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) c6[q] = group_sum(c6[q]) / dc;
  if (!live || l != 0) return;
  float s = 0.f;
  bool finite = cnt > 0, any = false;
#pragma unroll
  for (int q = 0; q < 6; ++q) { finite = finite && isfinite(c6[q]); any = any || c6[q] != 0.0; }
  if (finite && any) {
    const double Cm[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
    double U[3][3], S[3], V[3][3];
    svd3(Cm, U, S, V);
    if (S[0] > 0.0 && S[1] > 0.0 && S[1] / S[0] < gamma_21 && S[2] / S[1] < gamma_32) s = (float)S[2];
  }
  saliency[r] = s;
}

__device__ __forceinline__ void block_ballot_counts(bool keep, int32_t* wave_sum, unsigned long long& m) {
  m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = (int32_t)__popcll(m);
  __syncthreads();
}

__global__ __launch_bounds__(kSelT) void iss_select_kernel(const float* __restrict__ saliency, const int32_t* __restrict__ offsets,
                                                           const int32_t* __restrict__ cols, int n, int min_neighbors,
                                                           int32_t* __restrict__ mask, int32_t* __restrict__ block_counts) {
  __shared__ int32_t wave_sum[kSelT / 64];
  const int cloud = blockIdx.y, i = blockIdx.x * kSelT + (int)threadIdx.x;
  const float* sal = saliency + (int64_t)cloud * n;
  bool keep = false;
  if (i < n) {
    const int64_t r = (int64_t)cloud * n + i;
    const float si = sal[i];
    const int b = offsets[r], cnt = max(offsets[r + 1] - b, 0);
    keep = si > 0.f && cnt >= min_neighbors;
    for (int k = 0; keep && k < cnt; ++k) {
      const int j = min(max(cols[b + k], 0), n - 1);
      const float sj = sal[j];
      if (sj > si || (sj == si && j < i)) keep = false;
    }
    mask[r] = keep ? 1 : 0;
  }
  unsigned long long m;
  block_ballot_counts(keep, wave_sum, m);
  if (threadIdx.x == 0) {
    int32_t s = 0;
    for (int w = 0; w < kSelT / 64; ++w) s += wave_sum[w];
    block_counts[(int64_t)cloud * gridDim.x + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kSelT) void iss_compact_kernel(const int32_t* __restrict__ mask, const int32_t* __restrict__ block_counts, int n,
                                                            int32_t* __restrict__ index, int32_t* __restrict__ counts) {
  __shared__ int32_t red[2][kSelT];
  __shared__ int32_t wave_sum[kSelT / 64];
  const int cloud = blockIdx.y, b = blockIdx.x, t = threadIdx.x, blocks = gridDim.x;
  const int32_t* bc = block_counts + (int64_t)cloud * blocks;
  int32_t before = 0, all = 0;              // integer sums: any order gives the same total
  for (int k = t; k < blocks; k += kSelT) {
    const int32_t v = bc[k];
    all += v;
    if (k < b) before += v;
  }
  red[0][t] = before; red[1][t] = all;
  __syncthreads();
  for (int o = kSelT / 2; o > 0; o >>= 1) {
    if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; }
    __syncthreads();
  }
  const int32_t base = red[0][0], total = red[1][0];
  const int i = b * kSelT + t;
  const bool keep = i < n && mask[(int64_t)cloud * n + i] != 0;
  unsigned long long m;
  block_ballot_counts(keep, wave_sum, m);
  const int lane = t & 63, wave = t >> 6;
  int32_t pos = base + (int32_t)__popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) pos += wave_sum[w];
  int32_t* out = index + (int64_t)cloud * n;
  if (keep && pos < n) out[pos] = i;        // pos < total <= n by construction
  if (i < n && i >= total) out[i] = -1;     // rows [0, total) are written by the ranked keypoints alone
  if (b == blocks - 1 && t == 0) counts[cloud] = total;
}

}  // namespace

static int iss_blocks(int n) { return (n + kSelT - 1) / kSelT; }

size_t iss_scratch_bytes(int clouds, int n) { return (size_t)clouds * (size_t)iss_blocks(n) * sizeof(int32_t); }

bool launch_iss_keypoints(const IssArgs& a, hipStream_t st) {
  if (a.n < 1 || a.clouds < 1 || a.clouds > 65535 || (int64_t)a.clouds * a.n > 0x7fffffffll - 1) return false;
  if (!a.pts || !a.sal_offsets || !a.sal_cols || !a.nms_offsets || !a.nms_cols || !a.saliency || !a.mask || !a.index || !a.counts ||
      !a.block_counts)
    return false;
  const dim3 gs((unsigned)((a.n + kSalPts - 1) / kSalPts), (unsigned)a.clouds), gb((unsigned)iss_blocks(a.n), (unsigned)a.clouds);
  hipLaunchKernelGGL(iss_saliency_kernel, gs, dim3(256), 0, st, a.pts, a.pts_cs, a.pts_ld, a.sal_offsets, a.sal_cols, a.n, a.gamma_21,
                     a.gamma_32, a.min_neighbors, a.saliency);
  hipLaunchKernelGGL(iss_select_kernel, gb, dim3(kSelT), 0, st, (const float*)a.saliency, a.nms_offsets, a.nms_cols, a.n, a.min_neighbors,
                     a.mask, a.block_counts);
  hipLaunchKernelGGL(iss_compact_kernel, gb, dim3(kSelT), 0, st, (const int32_t*)a.mask, (const int32_t*)a.block_counts, a.n, a.index,
                     a.counts);
  return true;
}

}  // namespace dsir
