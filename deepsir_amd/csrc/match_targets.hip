// Ground-truth matches and inlier targets of the `align` training step, on the device (include/dsir_train.h, "ground-truth matches").
//
// The reference builds data['matches'] in its loader: per source point an open3d KD-tree radius search around T_gt src_i among the
// reference points (dataloader/data_base.py:436-449 get_matching_indices with K = None, radius = voxel_size *
// positive_pair_radius_multiplier), in a Python loop; ScanAlignmentLoss.find_correct_correspondence (network/loss.py:723-749) then
// asks on the host, per registration iteration, whether the predicted pair (j, idx[j]) is in that list - the 0/1 targets of the
// confidence term.  With K = None the list holds EVERY (i, k) inside the radius, so "in the list" is the distance test itself.
//
// open3d is not installable here, so parity at this boundary is unpinned (like the ICP and the voxel grid).  The rule owned here, in
// fp32 with every operation rounded on its own (no fused multiply-add):
//     c_r = ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3]                      the source point moved by T_gt
//     d2  = (dx dx + dy dy) + dz dz,  d = ref - c                                 as csrc/icp.hip forms it
//     match  <=>  d2 < r r                                                        r r one fp32 product
// The comparison is strict, as nanoflann's radius result set (which open3d's KD-tree search uses) compares - from memory: neither
// library is available to check against.  Every operator below decides through match_rule(), so they agree bit for bit, and numpy in
// float32 restates the rule exactly (tests/test_match_targets.py).
//
// No atomics: counts are per lane, the order of a row's columns is fixed by construction (reference slices in ascending order, one
// lane walks a slice in ascending order), two runs write the same bytes.  Scans and sorts are library calls (hipCUB).
#include <hipcub/hipcub.hpp>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsir_train.h"
#include "op_layouts.h"
#include "seg_sort.h"
#include "train_ops.h"

namespace dsir {
namespace {

constexpr int QB = 64;          // source points per block: one per lane
constexpr int NW = 4;           // waves per block, each on its own part of the block's reference slice
constexpr int TILE = 256;       // reference points a wave stages per step
constexpr int MAX_SPLIT = 16;   // reference slices across the grid (blockIdx.y)

struct Pt { float x, y, z; };

// T_gt [3][4] row-major applied to (x, y, z)
__device__ __forceinline__ Pt match_move(const float* __restrict__ T, float x, float y, float z) {
  Pt c;
  c.x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[0], x), __fmul_rn(T[1], y)), __fmul_rn(T[2], z)), T[3]);
  c.y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[4], x), __fmul_rn(T[5], y)), __fmul_rn(T[6], z)), T[7]);
  c.z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[8], x), __fmul_rn(T[9], y)), __fmul_rn(T[10], z)), T[11]);
  return c;
}

__device__ __forceinline__ bool match_near(const Pt c, float rx, float ry, float rz, float r2) {
  const float dx = __fsub_rn(rx, c.x), dy = __fsub_rn(ry, c.y), dz = __fsub_rn(rz, c.z);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)) < r2;
}

// THE rule: is reference point (rx, ry, rz) a ground-truth match of source point (x, y, z) under T?  r2 = radius * radius in fp32.
__device__ __forceinline__ bool match_rule(const float* __restrict__ T, float x, float y, float z, float rx, float ry, float rz, float r2) {
  return match_near(match_move(T, x, y, z), rx, ry, rz, r2);
}

// Brute force, the layout of icp_nn_kernel: a lane owns one source point, wave w of block (bx, by, pair) walks part by * NW + w of the
// pair's reference points, staged through LDS and read as broadcasts.  FILL = false: part[row][by * NW + w] = matches in that part.
// FILL = true: the part's matching indices go to cols from offsets[row] + part[row][by * NW + w] on (part now holds the exclusive
// prefix within the row, row_prefix_kernel), never past the part's own end nor n_cols.
template <bool FILL>
__global__ __launch_bounds__(QB * NW) void radius_matches_kernel(const float* __restrict__ src, const float* __restrict__ ref, int stride,
                                                                 const float* __restrict__ Tgt, int J, int K, float r2, int parts,
                                                                 int32_t* __restrict__ part, const int32_t* __restrict__ offsets,
                                                                 int32_t* __restrict__ cols, int64_t n_cols) {
  __shared__ float4 tile[NW][TILE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int pair = blockIdx.z;
  const float* S = ref + (int64_t)pair * K * stride;
  const int q = blockIdx.x * QB + lane;
  const int64_t row = (int64_t)pair * J + q;
  Pt c{0.f, 0.f, 0.f};
  if (q < J) {
    const float* p = src + row * stride;
    c = match_move(Tgt + (int64_t)pair * 12, p[0], p[1], p[2]);
  }
  const int slot = blockIdx.y * NW + w;
  const int len = (K + parts - 1) / parts;                    // the same for every part: the loops below are block-uniform
  const int s_begin = min(K, slot * len), s_end = min(K, s_begin + len);
  int64_t pos = 0, end = 0;
  if (FILL && q < J) {
    const int64_t base = offsets[row];
    pos = base + part[row * parts + slot];
    end = slot + 1 < parts ? base + part[row * parts + slot + 1] : (int64_t)offsets[row + 1];
    end = end < n_cols ? end : n_cols;
  }
  int cnt = 0;
  for (int t0 = 0; t0 < len; t0 += TILE) {
#pragma unroll
    for (int r = 0; r < TILE / 64; ++r) {
      const int j = s_begin + t0 + r * 64 + lane;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j < s_end) { v.x = S[(int64_t)j * stride]; v.y = S[(int64_t)j * stride + 1]; v.z = S[(int64_t)j * stride + 2]; }
      tile[w][r * 64 + lane] = v;
    }
    __syncthreads();
    const int n = max(0, min(TILE, s_end - (s_begin + t0)));
    for (int j = 0; j < n; ++j) {
      const float4 s = tile[w][j];
      const bool in = match_near(c, s.x, s.y, s.z, r2);
      if (FILL) {
        if (in && pos < end) cols[pos++] = s_begin + t0 + j;
      } else {
        cnt += in ? 1 : 0;
      }
    }
    __syncthreads();
  }
  if (!FILL && q < J) part[row * parts + slot] = cnt;
}

// per source row: counts[row] = sum of its parts, part[row][.] <- exclusive prefix within the row
__global__ void row_prefix_kernel(int32_t* __restrict__ part, int parts, int64_t rows, int32_t* __restrict__ counts) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
    int32_t* p = part + r * parts;
    int acc = 0;
    for (int s = 0; s < parts; ++s) { const int v = p[s]; p[s] = acc; acc += v; }
    counts[r] = acc;
  }
}

__global__ void targets_radius_kernel(const float* __restrict__ src, const float* __restrict__ ref, int stride, const int32_t* __restrict__ idx,
                                      const float* __restrict__ Tgt, int P, int J, int K, float r2, float* __restrict__ labels, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = e % ((int64_t)P * J);                 // labels / idx [n_iter][P][J]
    const int pair = (int)(row / J);
    const int k = min(max(idx[e], 0), K - 1);
    const float* s = src + row * stride;
    const float* r = ref + ((int64_t)pair * K + k) * stride;
    labels[e] = match_rule(Tgt + (int64_t)pair * 12, s[0], s[1], s[2], r[0], r[1], r[2], r2) ? 1.f : 0.f;
  }
}

// ScanAlignmentLoss._hash (network/loss.py:280-294): key = src + ref * hash_seed in int64
__global__ void match_keys_kernel(const int32_t* __restrict__ matches, int64_t n, int64_t hash_seed, int64_t* __restrict__ keys) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
    keys[e] = (int64_t)matches[2 * e] + (int64_t)matches[2 * e + 1] * hash_seed;
}

// np.isin(j + idx * hash_seed, keys of the pair): binary search in the pair's sorted segment.  idx is NOT clamped: it only enters
// the key arithmetic, exactly as on the host.
__global__ void targets_matches_kernel(const int64_t* __restrict__ keys, const int32_t* __restrict__ seg, const int32_t* __restrict__ idx,
                                       int P, int J, int64_t hash_seed, float* __restrict__ labels, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = e % ((int64_t)P * J);
    const int pair = (int)(row / J);
    const int64_t key = (row - (int64_t)pair * J) + (int64_t)idx[e] * hash_seed;
    int lo = seg[pair], hi = seg[pair + 1];                   // first position whose key is >= key
    const int last = hi;
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (keys[mid] < key) lo = mid + 1; else hi = mid; }
    labels[e] = (lo < last && keys[lo] == key) ? 1.f : 0.f;
  }
}


// reference slices across the grid: enough blocks to fill the chip (about 2048 of 4 waves), no part shorter than one tile
inline int match_split(int pairs, int J, int K) {
  const int64_t row_blocks = (int64_t)pairs * ((J + QB - 1) / QB);
  int64_t s = (2048 + row_blocks - 1) / row_blocks;
  const int64_t cap = K / (NW * TILE);
  s = s > cap ? cap : s;
  return (int)(s < 1 ? 1 : (s > MAX_SPLIT ? MAX_SPLIT : s));
}

inline bool match_shape_ok(int pairs, int J, int K, int stride) {
  return pairs >= 1 && pairs <= 65535 && J >= 1 && K >= 1 && stride >= 3 && (int64_t)pairs * J * K <= 0x7fffffffll;
}

size_t scan_tmp_bytes(int64_t rows) {
  size_t b = 0;
  hipcub::DeviceScan::InclusiveSum(nullptr, b, (const int32_t*)nullptr, (int32_t*)nullptr, (int)rows);
  return b;
}
inline BufferTmpLayout radius_layout(int pairs, int J, int K) {
  const size_t rows = (size_t)pairs * J;
  return BufferTmpLayout(rows * match_split(pairs, J, K) * NW * sizeof(int32_t), scan_tmp_bytes((int64_t)rows));
}
inline BufferTmpLayout keys_layout(int64_t n_matches, size_t sort_tmp) { return BufferTmpLayout((size_t)n_matches * sizeof(int64_t), sort_tmp); }

}  // namespace
}  // namespace dsir

using namespace dsir;

extern "C" {

size_t dsir_t_radius_matches_scratch(int pairs, int J, int K) {
  return match_shape_ok(pairs, J, K, 3) ? radius_layout(pairs, J, K).bytes : 0;
}

int dsir_t_radius_matches_count(void* stream, const float* src, const float* ref, int stride, const float* transform_gt, int pairs, int J,
                                int K, float radius, int32_t* counts, int32_t* offsets, void* scratch) {
  if (!src || !ref || !transform_gt || !counts || !offsets || !scratch || !match_shape_ok(pairs, J, K, stride) || !(radius >= 0.f))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)pairs * J;
  const int split = match_split(pairs, J, K), parts = split * NW;
  const BufferTmpLayout lay = radius_layout(pairs, J, K);
  int32_t* part = at<int32_t>(scratch, lay.buf);
  const float r2 = radius * radius;
  hipLaunchKernelGGL(radius_matches_kernel<false>, dim3((J + QB - 1) / QB, split, pairs), dim3(QB * NW), 0, st, src, ref, stride, transform_gt, J,
                     K, r2, parts, part, (const int32_t*)nullptr, (int32_t*)nullptr, (int64_t)0);
  hipLaunchKernelGGL(row_prefix_kernel, dim3(grid1(rows)), dim3(256), 0, st, part, parts, rows, counts);
  if (hipMemsetAsync(offsets, 0, sizeof(int32_t), st) != hipSuccess) return (int)hipGetLastError();
  size_t tb = scan_tmp_bytes(rows);
  if (hipcub::DeviceScan::InclusiveSum(at<char>(scratch, lay.tmp), tb, counts, offsets + 1, (int)rows, st) != hipSuccess)
    return (int)hipErrorUnknown;
  return done();
}

int dsir_t_radius_matches_fill(void* stream, const float* src, const float* ref, int stride, const float* transform_gt, int pairs, int J,
                               int K, float radius, const int32_t* offsets, const void* scratch, int32_t* cols, int64_t n_cols) {
  if (!src || !ref || !transform_gt || !offsets || !scratch || !match_shape_ok(pairs, J, K, stride) || !(radius >= 0.f) || n_cols < 0 ||
      (n_cols > 0 && !cols))
    return (int)hipErrorInvalidValue;
  if (n_cols == 0) return 0;
  const int split = match_split(pairs, J, K), parts = split * NW;
  const float r2 = radius * radius;
  int32_t* part = const_cast<int32_t*>(at<int32_t>(scratch, radius_layout(pairs, J, K).buf));
  hipLaunchKernelGGL(radius_matches_kernel<true>, dim3((J + QB - 1) / QB, split, pairs), dim3(QB * NW), 0, (hipStream_t)stream, src, ref, stride,
                     transform_gt, J, K, r2, parts, part, offsets, cols, n_cols);
  return done();
}

int dsir_t_inlier_targets_radius(void* stream, const float* src, const float* ref, int stride, const int32_t* idx, const float* transform_gt,
                                 int n_iter, int pairs, int J, int K, float radius, float* labels) {
  if (!src || !ref || !idx || !transform_gt || !labels || n_iter < 1 || pairs < 1 || J < 1 || K < 1 || stride < 3 || !(radius >= 0.f))
    return (int)hipErrorInvalidValue;
  const int64_t total = (int64_t)n_iter * pairs * J;
  hipLaunchKernelGGL(targets_radius_kernel, dim3(grid1(total)), dim3(256), 0, (hipStream_t)stream, src, ref, stride, idx, transform_gt, pairs, J,
                     K, radius * radius, labels, total);
  return done();
}

size_t dsir_t_match_keys_scratch(int64_t n_matches, int pairs) {
  return n_matches < 1 || n_matches > 0x7fffffffll || pairs < 1 ? 0 : keys_layout(n_matches, seg_sort_keys_i64_tmp_bytes(n_matches, pairs)).bytes;
}

int dsir_t_match_keys(void* stream, const int32_t* matches, const int32_t* pair_offsets, int64_t n_matches, int pairs, int64_t hash_seed,
                      int64_t* keys, void* scratch) {
  if (pairs < 1 || n_matches < 0 || n_matches > 0x7fffffffll || !pair_offsets) return (int)hipErrorInvalidValue;
  if (n_matches == 0) return 0;
  if (!matches || !keys || !scratch) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  size_t sort_tmp = seg_sort_keys_i64_tmp_bytes(n_matches, pairs);
  const BufferTmpLayout lay = keys_layout(n_matches, sort_tmp);
  int64_t* raw = at<int64_t>(scratch, lay.buf);
  hipLaunchKernelGGL(match_keys_kernel, dim3(grid1(n_matches)), dim3(256), 0, st, matches, n_matches, hash_seed, raw);
  if (hipcub::DeviceSegmentedRadixSort::SortKeys(at<char>(scratch, lay.tmp), sort_tmp, (const int64_t*)raw, keys, (int)n_matches, pairs, pair_offsets,
                                                 pair_offsets + 1, 0, 64, st) != hipSuccess)
    return (int)hipErrorUnknown;
  return done();
}

int dsir_t_inlier_targets_matches(void* stream, const int64_t* keys, const int32_t* pair_offsets, const int32_t* idx, int n_iter, int pairs,
                                  int J, int64_t hash_seed, float* labels) {
  if (!pair_offsets || !idx || !labels || n_iter < 1 || pairs < 1 || J < 1) return (int)hipErrorInvalidValue;
  const int64_t total = (int64_t)n_iter * pairs * J;
  hipLaunchKernelGGL(targets_matches_kernel, dim3(grid1(total)), dim3(256), 0, (hipStream_t)stream, keys, pair_offsets, idx, pairs, J, hash_seed,
                     labels, total);
  return done();
}

}  // extern "C"
