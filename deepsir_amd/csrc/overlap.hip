// Fragment overlap: the radius-bounded nearest neighbour of one ragged cloud in another, over a sparse cell index
// (include/dsir_train.h, "fragment overlap").
//
// The reference makes its 3DMatch training tables offline (dataloader/3DMatch_preprocess.py:82-89, :107-131): for every fragment pair
// i < j of a scene, cv2.BFMatcher(NORM_L2).match(anc, pos) - the nearest pos point of every anc point, brute force - kept where
// distance < voxel size; the share of kept points is the overlap ratio, the kept (i, j) are the key-point pairs.  cv2 is not
// installable here, so parity at this boundary is unpinned (like the voxel grid, the ICP and the match lists); the rule owned here:
//     d2 = (dx dx + dy dy) + dz dz,  d = b - a          fp32, every operation rounded on its own (csrc/match_targets.hip, csrc/icp.hip)
//     the neighbour of a is the b with the smallest d2; ties go to the LOWER ORIGINAL INDEX of b
//     match  <=>  d2 < r r                               strict, r r one fp32 product (BFMatcher's distance < r on the square root)
//     a query with a non-finite coordinate matches nothing; a non-finite b is never a neighbour; an empty a or b gives count 0
//     with a pose T [3][4] per job the query is moved first: c_r = ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3] (match_move of
//     csrc/match_targets.hip; the identity is a separate case there too: poses == NULL reads the unmoved bits)
// deepsir_amd/overlap.py::nn_within_host restates it in numpy float32; the tests compare bit for bit.
//
// The lattice, one per call: origin o = the minimum over all finite points (the caller's bounds), cell edge h = r (1 + 2^-10) in fp64,
// cell coordinate c(a) = floor(((double)a - (double)o) / h) per axis, in fp64 from the fp32 values.  Why no b that satisfies the rule
// can lie outside the 27 cells around c(a): the argument of csrc/cell_index.h with the strict `<` - fl(dx dx) <= d2 < fl(r r) gives
// |b - a| < r (1 + 2^-21) per axis (a dx dx that underflows has |dx| < 2^-63: smaller still), so |b - a| / h < 1 - 2^-11.  An extent
// of more than 2^21 - 2 cells on an axis is refused before any launch, so c + 1 still fits the 21 bits an axis has in the key
// x | y << 21 | z << 42.
//
// The index is sparse - workspace linear in the point count, never in the box's cells (a 5 m fragment at 0.03 m spans 5 10^6 cells,
// a scene has hundreds of fragments): per fragment the points sorted by key (hipCUB segmented radix sort, a library step), xyz and the
// original index as one float4, and the fragment's cell box.  A non-finite point gets the key ~0, sorts last and is in no interval.
// At h = the voxel size the clouds were thinned with a cell holds about one point, so the sorted keys themselves are searched: a
// table of run starts would take a compaction pass and save no probe.  The search compares (d2, original index) lexicographically,
// so the tie rule does not rest on the order inside a cell.
//
// nn_within_kernel, the hot path: one lane per query, queries in the query fragment's own cell order (a wave's lanes walk the same
// or adjacent parts of the target's keys), results written in original numbering.  Per query 9 lookups (dy, dz) in {-1, 0, 1}^2,
// each the key interval [key(cx - 1), key(cx + 1)]: a binary search (up to 15 dependent global loads at 16384 target points) and a
// scan of the run.  What bounds it is that latency, about 9 x 15 dependent probes per lane, hidden by occupancy: the build reports
// 29 VGPRs, 70 SGPRs, no LDS, no scratch, 8 waves per SIMD.  A query whose cell is outside the target's cell box grown by one, and a block
// whose whole job has disjoint boxes, end without a search.  Jobs are ragged: block -> (job, query block) through a prefix over
// the jobs' block counts, made on the host with the validation.  Counts meet in integer atomics (order-independent); nothing else
// is shared, so two runs write the same bytes and a job's bytes do not depend on the rest of the list.
#include <hipcub/hipcub.hpp>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "cell_index.h"
#include "seg_sort.h"
#include "dsir_train.h"

namespace dsir {
namespace {

constexpr int NN_BLOCK = 256;                       // queries per block: one per lane, 4 waves
constexpr int64_t MAX_CELLS = (1ll << 21) - 2;      // per axis
constexpr int64_t MAX_POINTS = 1ll << 30;
constexpr int MAX_FRAGMENTS = 1 << 20;

// enc [6]: min xyz, max xyz of the finite rows, as ordered integers (integer atomics: order-independent)
__global__ void finite_bounds_kernel(const float* __restrict__ pts, int stride, int64_t n, uint32_t* __restrict__ enc) {
  finite_bounds_accumulate(pts, stride, n, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, enc, enc + 3);
}
__global__ void finite_bounds_decode_kernel(const uint32_t* enc, float* out) {
  const int a = threadIdx.x < 6 ? threadIdx.x : 0;                // enc and out may be the same 24 bytes: read all, then write
  const float v = enc[0] > enc[3] ? 0.f : ord2f(enc[a]);           // min > max: no finite row at all
  __syncthreads();
  if (threadIdx.x < 6) out[a] = v;
}

// keys [total], vals [total] = the row's index inside its fragment; frag found by binary search over off [F + 1]
__global__ void nn_key_kernel(const float* __restrict__ pts, int stride, const int32_t* __restrict__ off, int F, int64_t total, CellLattice L,
                              uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int lo = 0, hi = F;                                            // the last f with off[f] <= i
    while (hi - lo > 1) { const int mid = lo + ((hi - lo) >> 1); if ((int64_t)off[mid] <= i) lo = mid; else hi = mid; }
    const float* p = pts + i * stride;
    keys[i] = point_key(p[0], p[1], p[2], L);
    vals[i] = (uint32_t)(i - off[lo]);
  }
}

// sorted [total] = (x, y, z, original index) in key order
__global__ void nn_gather_kernel(const float* __restrict__ pts, int stride, const int32_t* __restrict__ off, int F, int64_t total,
                                 const uint32_t* __restrict__ vals, float4* __restrict__ sorted) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int lo = 0, hi = F;
    while (hi - lo > 1) { const int mid = lo + ((hi - lo) >> 1); if ((int64_t)off[mid] <= i) lo = mid; else hi = mid; }
    const uint32_t v = vals[i];
    const float* p = pts + ((int64_t)off[lo] + v) * stride;
    sorted[i] = gather_xyzi(p, v);
  }
}

// box [F][6]: min / max cell coordinate of the fragment's finite points (from the sorted keys); empty: min = MAXC + 8, max = -8
__global__ __launch_bounds__(256) void nn_box_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ off, int32_t* __restrict__ box) {
  __shared__ int red[4][6];
  const int f = blockIdx.x;
  const int b = off[f], e = off[f + 1];
  int lo[3] = {MAXC + 8, MAXC + 8, MAXC + 8}, hi[3] = {-8, -8, -8};
  for (int i = b + threadIdx.x; i < e; i += blockDim.x) {
    const uint64_t k = keys[i];
    if (k == KEY_NONE) continue;
#pragma unroll
    for (int a = 0; a < 3; ++a) { const int c = (int)((k >> (21 * a)) & (uint64_t)MAXC); lo[a] = min(lo[a], c); hi[a] = max(hi[a], c); }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    for (int s = 32; s > 0; s >>= 1) { lo[a] = min(lo[a], __shfl_xor(lo[a], s)); hi[a] = max(hi[a], __shfl_xor(hi[a], s)); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][a] = lo[a]; red[threadIdx.x >> 6][3 + a] = hi[a]; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = threadIdx.x;
    int v = red[0][a];
    for (int w = 1; w < 4; ++w) v = a < 3 ? min(v, red[w][a]) : max(v, red[w][a]);
    box[f * 6 + a] = v;
  }
}

// tab: off [F + 1] | jobs [n][2] | blk [n + 1] (prefix of the jobs' block counts) | row [n + 1] (prefix of the jobs' query rows)
__global__ __launch_bounds__(NN_BLOCK) void nn_within_kernel(const uint64_t* __restrict__ keys, const float4* __restrict__ sorted,
                                                             const int32_t* __restrict__ box, const int32_t* __restrict__ off,
                                                             const int32_t* __restrict__ jobs, const int32_t* __restrict__ blk,
                                                             const int32_t* __restrict__ row, int n_jobs, const float* __restrict__ poses,
                                                             float r2, CellLattice L, int32_t* __restrict__ counts, int32_t* __restrict__ nn) {
  int jlo = 0, jhi = n_jobs;                                       // the last job with blk[job] <= blockIdx.x: block-uniform
  while (jhi - jlo > 1) { const int mid = jlo + ((jhi - jlo) >> 1); if (blk[mid] <= (int)blockIdx.x) jlo = mid; else jhi = mid; }
  const int job = jlo;
  const int qf = jobs[2 * job], tf = jobs[2 * job + 1];
  const int qb = off[qf], nq = off[qf + 1] - qb, tb = off[tf], nt = off[tf + 1] - tb;
  const int s = ((int)blockIdx.x - blk[job]) * NN_BLOCK + (int)threadIdx.x;
  const bool active = s < nq;
  int tlo[3], thi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { tlo[a] = box[tf * 6 + a] - 1; thi[a] = box[tf * 6 + 3 + a] + 1; }
  bool apart = nt == 0;                                            // block-uniform: the whole job has nothing to find
  if (!poses) {
#pragma unroll
    for (int a = 0; a < 3; ++a) apart = apart || box[qf * 6 + a] > thi[a] || box[qf * 6 + 3 + a] < tlo[a];
  }
  int best_i = -1, orig = 0;
  if (active) {
    const float4 p = sorted[qb + s];
    orig = (int)__float_as_uint(p.w);
    float x = p.x, y = p.y, z = p.z;
    if (poses) {
      const float* T = poses + (int64_t)job * 12;
      const float mx = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[0], x), __fmul_rn(T[1], y)), __fmul_rn(T[2], z)), T[3]);
      const float my = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[4], x), __fmul_rn(T[5], y)), __fmul_rn(T[6], z)), T[7]);
      const float mz = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[8], x), __fmul_rn(T[9], y)), __fmul_rn(T[10], z)), T[11]);
      x = mx; y = my; z = mz;
    }
    if (!apart && finite3(x, y, z)) {
      const int cx = cell_of(x, L.ox, L.h), cy = cell_of(y, L.oy, L.h), cz = cell_of(z, L.oz, L.h);
      if (cx >= tlo[0] && cx <= thi[0] && cy >= tlo[1] && cy <= thi[1] && cz >= tlo[2] && cz <= thi[2]) {
        const uint64_t* K = keys + tb;
        const float4* S = sorted + tb;
        float best = INFINITY;
        walk_key_intervals(cx, cy, cz, tlo[1], thi[1], tlo[2], thi[2], [&](uint64_t klo, uint64_t khi) {   // tlo / thi: the box grown by one
          for (int i = key_lower_bound(K, nt, klo); i < nt && K[i] <= khi; ++i) {
            const float4 t = S[i];
            const float d2 = dist2_rn(t, x, y, z);
            const int ti = (int)__float_as_uint(t.w);
            if (d2 < r2 && (d2 < best || (d2 == best && ti < best_i))) { best = d2; best_i = ti; }
          }
        });
      }
    }
    if (nn) nn[(int64_t)row[job] + orig] = best_i;
  }
  const int hits = __popcll(__ballot(active && best_i >= 0));
  if ((threadIdx.x & 63) == 0 && hits) atomicAdd(counts + job, hits);
}

inline unsigned grid1(int64_t n) { const int64_t g = (n + 255) / 256; return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g)); }
inline IndexLayout layout(int64_t total, int F) { return IndexLayout(total, F, seg_sort_tmp_bytes(total, F)); }

inline bool index_shape_ok(int64_t total, int F) { return total >= 0 && total <= MAX_POINTS && F >= 1 && F <= MAX_FRAGMENTS; }

const char* check(const int64_t* offsets, int F, const int32_t* jobs, int64_t n_jobs, float radius, const float* bounds) {
  if (!offsets || !bounds) return "nn_within: offsets and bounds are required";
  if (!(radius > 0.f) || !isfinite(radius) || !(radius * radius > 0.f) || !isfinite(radius * radius))
    return "nn_within: the radius must be positive and finite (and its fp32 square too)";
  if (F < 1 || F > MAX_FRAGMENTS) return "nn_within: between 1 and 2^20 fragments";
  if (offsets[0] != 0) return "nn_within: offsets must start at 0";
  for (int f = 0; f < F; ++f)
    if (offsets[f + 1] < offsets[f]) return "nn_within: offsets must ascend";
  if (offsets[F] > MAX_POINTS) return "nn_within: more than 2^30 points in one call";
  const double h = nn_cell_edge(radius);
  for (int a = 0; a < 3; ++a) {
    if (!isfinite(bounds[a]) || !isfinite(bounds[3 + a]) || bounds[a] > bounds[3 + a]) return "nn_within: bounds must be finite, min <= max";
    if (floor(((double)bounds[3 + a] - (double)bounds[a]) / h) + 1.0 > (double)MAX_CELLS)
      return "nn_within: the extent needs more than 2^21 - 2 cells of the radius on an axis";
  }
  if (n_jobs < 0 || n_jobs > 0x3fffffffll) return "nn_within: between 0 and 2^30 - 1 jobs";
  if (n_jobs > 0 && jobs) {
    int64_t rows = 0, blocks = 0;
    for (int64_t j = 0; j < n_jobs; ++j) {
      const int32_t q = jobs[2 * j], t = jobs[2 * j + 1];
      if (q < 0 || q >= F || t < 0 || t >= F) return "nn_within: job index out of range";
      const int64_t nq = offsets[q + 1] - offsets[q];
      rows += nq;
      blocks += (nq + NN_BLOCK - 1) / NN_BLOCK;
    }
    if (rows > 0x7fffffffll || blocks > 0x7fffffffll) return "nn_within: more than 2^31 - 1 query rows in one job list: split it";
  }
  return nullptr;
}

}  // namespace
}  // namespace dsir

using namespace dsir;

extern "C" {

const char* dsir_t_nn_within_check(const int64_t* offsets, int fragments, const int32_t* jobs, int64_t n_jobs, float radius,
                                   const float* bounds) {
  return check(offsets, fragments, jobs, n_jobs, radius, bounds);
}

int dsir_t_finite_bounds(void* stream, const float* points, int stride, int64_t n, float* bounds_dev) {
  if (!bounds_dev || n < 0 || stride < 3 || (n > 0 && !points)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  // the ordered-integer accumulators live in the output's own 24 bytes until the decode
  uint32_t* enc = reinterpret_cast<uint32_t*>(bounds_dev);
  if (hipMemsetAsync(enc, 0xff, 3 * sizeof(uint32_t), st) != hipSuccess || hipMemsetAsync(enc + 3, 0, 3 * sizeof(uint32_t), st) != hipSuccess)
    return (int)hipGetLastError();
  if (n > 0) hipLaunchKernelGGL(finite_bounds_kernel, dim3(grid1(n) > 1024 ? 1024 : grid1(n)), dim3(256), 0, st, points, stride, n, enc);
  hipLaunchKernelGGL(finite_bounds_decode_kernel, dim3(1), dim3(64), 0, st, enc, bounds_dev);
  return (int)hipGetLastError();
}

size_t dsir_t_nn_index_scratch(int64_t total, int fragments) {
  if (!index_shape_ok(total, fragments)) return 0;
  return layout(total, fragments).bytes;
}

int dsir_t_nn_index_build(void* stream, const float* points, int stride, const int64_t* offsets, int fragments, float radius,
                          const float* bounds, void* index) {
  if (!index || stride < 3 || check(offsets, fragments, nullptr, 0, radius, bounds)) return (int)hipErrorInvalidValue;
  const int64_t total = offsets[fragments];
  if (total > 0 && !points) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const IndexLayout lay = layout(total, fragments);
  char* base = reinterpret_cast<char*>(index);
  uint64_t* keys = reinterpret_cast<uint64_t*>(base + lay.keys);
  float4* sorted = reinterpret_cast<float4*>(base + lay.sorted);
  int32_t* box = reinterpret_cast<int32_t*>(base + lay.box);
  int32_t* off = reinterpret_cast<int32_t*>(base + lay.off);
  uint64_t* keys_raw = reinterpret_cast<uint64_t*>(base + lay.keys_raw);
  uint32_t* vals_raw = reinterpret_cast<uint32_t*>(base + lay.vals_raw);
  uint32_t* vals = reinterpret_cast<uint32_t*>(base + lay.vals);
  std::vector<int32_t> off32((size_t)fragments + 1);
  for (int f = 0; f <= fragments; ++f) off32[f] = (int32_t)offsets[f];
  if (hipMemcpyAsync(off, off32.data(), off32.size() * sizeof(int32_t), hipMemcpyHostToDevice, st) != hipSuccess) return (int)hipGetLastError();
  if (total > 0) {
    hipLaunchKernelGGL(nn_key_kernel, dim3(grid1(total)), dim3(256), 0, st, points, stride, off, fragments, total, nn_lattice(bounds, radius),
                       keys_raw, vals_raw);
    size_t tb = lay.tmp_bytes;
    if (hipcub::DeviceSegmentedRadixSort::SortPairs(base + lay.tmp, tb, (const uint64_t*)keys_raw, keys, (const uint32_t*)vals_raw, vals,
                                                    (int)total, fragments, (const int32_t*)off, (const int32_t*)(off + 1), 0, 64, st) != hipSuccess)
      return (int)hipErrorUnknown;
    hipLaunchKernelGGL(nn_gather_kernel, dim3(grid1(total)), dim3(256), 0, st, points, stride, off, fragments, total, vals, sorted);
  }
  hipLaunchKernelGGL(nn_box_kernel, dim3(fragments), dim3(256), 0, st, keys, off, box);
  return (int)hipGetLastError();
}

size_t dsir_t_nn_within_scratch(int64_t n_jobs) {
  if (n_jobs < 0 || n_jobs > 0x3fffffffll) return 0;
  Carve c;
  c.take((size_t)(4 * n_jobs + 2) * sizeof(int32_t));
  return c.p;
}

int dsir_t_nn_within(void* stream, const void* index, const int64_t* offsets, int fragments, const int32_t* jobs, int64_t n_jobs,
                     const float* poses, float radius, const float* bounds, int32_t* counts, int32_t* nn, void* job_scratch) {
  if (!index || (n_jobs > 0 && (!jobs || !counts || !job_scratch)) || check(offsets, fragments, jobs, n_jobs, radius, bounds))
    return (int)hipErrorInvalidValue;
  if (n_jobs == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = offsets[fragments];
  const IndexLayout lay = layout(total, fragments);
  const char* base = reinterpret_cast<const char*>(index);
  // jobs [n][2] | blk [n + 1] | row [n + 1]
  std::vector<int32_t> tab((size_t)(4 * n_jobs + 2));
  int32_t* blk = tab.data() + 2 * n_jobs;
  int32_t* row = blk + n_jobs + 1;
  blk[0] = 0; row[0] = 0;
  for (int64_t j = 0; j < n_jobs; ++j) {
    tab[2 * j] = jobs[2 * j]; tab[2 * j + 1] = jobs[2 * j + 1];
    const int64_t nq = offsets[jobs[2 * j] + 1] - offsets[jobs[2 * j]];
    blk[j + 1] = blk[j] + (int32_t)((nq + NN_BLOCK - 1) / NN_BLOCK);
    row[j + 1] = row[j] + (int32_t)nq;
  }
  const int blocks = blk[n_jobs];
  int32_t* dtab = reinterpret_cast<int32_t*>(job_scratch);
  if (hipMemcpyAsync(dtab, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, st) != hipSuccess) return (int)hipGetLastError();
  if (hipMemsetAsync(counts, 0, (size_t)n_jobs * sizeof(int32_t), st) != hipSuccess) return (int)hipGetLastError();
  if (blocks > 0)
    hipLaunchKernelGGL(nn_within_kernel, dim3(blocks), dim3(NN_BLOCK), 0, st, reinterpret_cast<const uint64_t*>(base + lay.keys),
                       reinterpret_cast<const float4*>(base + lay.sorted), reinterpret_cast<const int32_t*>(base + lay.box),
                       reinterpret_cast<const int32_t*>(base + lay.off), dtab, dtab + 2 * n_jobs, dtab + 3 * n_jobs + 1, (int)n_jobs, poses,
                       radius * radius, nn_lattice(bounds, radius), counts, nn);
  return (int)hipGetLastError();
}

}  // extern "C"
