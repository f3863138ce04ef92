// Half-space crop on the device (include/dsir_train.h, "half-space crop"): Transforms.RandomCrop.crop of the reference
// (dataloader/transformation.py:121-145) as the Oxford loader applies it twice to one scan (dataloader/oxford_loader.py:141-153).
//
// The rule is owned here and written down once on the host in deepsir_amd/crop.py, which the tests compare against bit for bit:
//     d_j = ((px - mx) ux + (py - my) uy) + (pz - mz) uz      fp32, every operation rounded on its own, m the fp32-rounded centroid
//     v = (n - 1) * (((1 - p_keep) * 100) / 100) in float64, lo = floor(v);  row j is kept iff d_j > d_(lo), -0 == +0
//     p_keep == 0.5: d_j > 0;  p_keep >= 1: every row;  a non-finite d_j is dropped, counts in n and sorts last
//     per-cloud refusals (count 0): no rows (bit 0), non-finite centroid or a non-finite d_(lo) (bit 1); nothing kept sets bit 0
//
// Three steps over a 32-bit order-preserving key of d_j kept in scratch:
//   project  one lane per row writes the key (non-finite: 0xFFFFFFFF) and takes the histogram of its top byte;
//   select   radix select of the lo-th smallest key, four 8-bit digits from the top: a histogram launch over the rows that still match the
//            prefix (passes 1-3; pass 0 rides on the projection), then one small launch that adds the workgroups' histograms in
//            workgroup order, scans the 256 bins and fixes the digit.  No sort.  The histograms are integer LDS atomics: the sums do not
//            depend on arrival order;
//   compact  mask = key > key_lo: per-workgroup counts (ballot + popcount), then every workgroup adds the counts of the workgroups before it
//            in its cloud, ranks its own rows by wave ballots in row order and copies whole rows.  No atomic decides a position.
//
// Work split: a cloud is cut into slices of ROWS = 2048 rows, one 256-thread workgroup per slice, grid (slices, clouds).  The shapes this
// is for are 16 clouds x 40000 rows and 64 x 20000: one workgroup per cloud would put 16 (or 64) workgroups on 256 compute units and
// walk 40000 keys five times in each, where the split form gives 320 and 640 workgroups whose slice of keys (8 KiB) stays in cache between
// the passes.  The price is the per-slice histogram (1 KiB) that the digit launch adds up in slice order: 20 rows of 256 integers per
// cloud.  A workgroup's LDS is 1 KiB of bins, so occupancy is bounded by waves, not by LDS.  By construction the call is bounded by the
// key traffic: 4 B written and five times read per row, plus one copy of the kept rows; at the two shapes above that is tens of MB, and
// the measured call is bound by its ten launches instead (profiles/README.md, "Half-space crop").
//
// Same inputs, same bytes; a cloud's output depends on its own rows, direction and p_keep alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "dsir_train.h"
#include "device_utils.h"
#include "scratch.h"
#include "train_ops.h"

namespace dsir {
namespace {

constexpr int CT = 256;                 // threads of a workgroup
constexpr int ROWS = 2048;              // rows of a slice
constexpr int WAVES = CT / 64;
constexpr uint32_t kNonFinite = 0xFFFFFFFFu;
constexpr uint32_t kZeroKey = 0x80000000u;     // key of +0
enum Mode : int32_t { MODE_SELECT = 0, MODE_THRESHOLD = 1, MODE_ALL = 2, MODE_REFUSED = 3 };

// one cloud's select state: prefix = the digits fixed so far (finally key_lo), rank = the rank still to find among the rows matching it
struct CropState {
  uint32_t prefix, rank;
  int32_t mode, bits;
};

inline int slices_of(int cap) { return (cap + ROWS - 1) / ROWS; }

struct Layout {
  size_t keys, hist, state, q, block_counts, total;
};
inline Layout layout(int clouds, int cap) {
  Layout l;
  const size_t nb = (size_t)slices_of(cap);
  Carve c;
  l.keys = c.take((size_t)clouds * cap * 4);
  l.hist = c.take((size_t)clouds * nb * 256 * 4);
  l.state = c.take((size_t)clouds * sizeof(CropState));
  l.q = c.take((size_t)clouds * 2 * sizeof(double));
  l.block_counts = c.take((size_t)clouds * nb * 4);
  l.total = c.p;
  return l;
}

__device__ __forceinline__ uint32_t order_key(float d) {
  if (!isfinite(d)) return kNonFinite;
  const uint32_t b = __float_as_uint(__fadd_rn(d, 0.f));          // -0 + 0 = +0
  return (b >> 31) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ int cloud_rows(const int32_t* counts, int c, int cap) { return max(0, min(counts[c], cap)); }

// ---- project: keys of the slice's rows, histogram of their top byte
__global__ __launch_bounds__(CT) void crop_project_kernel(const float* __restrict__ in, const int32_t* __restrict__ counts, int cap, int stride,
                                                          const float* __restrict__ dirs, const double* __restrict__ centroids,
                                                          uint32_t* __restrict__ keys, uint32_t* __restrict__ hist) {
  __shared__ uint32_t bins[256];
  const int c = blockIdx.y, b = blockIdx.x;
  const int n = cloud_rows(counts, c, cap);
  bins[threadIdx.x] = 0;
  __syncthreads();
  const float mx = (float)centroids[c * 3], my = (float)centroids[c * 3 + 1], mz = (float)centroids[c * 3 + 2];
  const float ux = dirs[c * 3], uy = dirs[c * 3 + 1], uz = dirs[c * 3 + 2];
  const int hi = min(n, (b + 1) * ROWS);
  for (int i = b * ROWS + (int)threadIdx.x; i < hi; i += CT) {
    const float* p = in + ((int64_t)c * cap + i) * stride;
    const float d = __fadd_rn(__fadd_rn(__fmul_rn(__fsub_rn(p[0], mx), ux), __fmul_rn(__fsub_rn(p[1], my), uy)),
                              __fmul_rn(__fsub_rn(p[2], mz), uz));
    const uint32_t k = order_key(d);
    keys[(int64_t)c * cap + i] = k;
    atomicAdd(&bins[k >> 24], 1u);
  }
  __syncthreads();
  hist[((int64_t)c * gridDim.x + b) * 256 + threadIdx.x] = bins[threadIdx.x];
}

// ---- select, passes 1-3: histogram of digit `pass` over the slice's rows whose higher digits equal the prefix
__global__ __launch_bounds__(CT) void crop_hist_kernel(const uint32_t* __restrict__ keys, const int32_t* __restrict__ counts, int cap, int pass,
                                                       const CropState* __restrict__ state, uint32_t* __restrict__ hist) {
  __shared__ uint32_t bins[256];
  const int c = blockIdx.y, b = blockIdx.x;
  if (state[c].mode != MODE_SELECT) return;           // uniform over the workgroup; the digit launch skips this cloud too
  const int n = cloud_rows(counts, c, cap);
  const uint32_t prefix = state[c].prefix;
  const int high = 32 - 8 * pass, low = 24 - 8 * pass;
  bins[threadIdx.x] = 0;
  __syncthreads();
  const int hi = min(n, (b + 1) * ROWS);
  for (int i = b * ROWS + (int)threadIdx.x; i < hi; i += CT) {
    const uint32_t k = keys[(int64_t)c * cap + i];
    if ((k >> high) == prefix) atomicAdd(&bins[(k >> low) & 255u], 1u);
  }
  __syncthreads();
  hist[((int64_t)c * gridDim.x + b) * 256 + threadIdx.x] = bins[threadIdx.x];
}

// ---- select: one workgroup per cloud adds the slices' histograms in slice order, scans the bins and fixes digit `pass`.
// Pass 0 also forms the state: the refusals, the mode and the rank lo from n and q = ((1 - p_keep) * 100) / 100.
__global__ __launch_bounds__(256) void crop_digit_kernel(const uint32_t* __restrict__ hist, int slices, const int32_t* __restrict__ counts, int cap,
                                                         const double* __restrict__ q, const double* __restrict__ centroids, int pass,
                                                         CropState* __restrict__ state) {
  __shared__ uint32_t scan[256];
  __shared__ CropState st;
  const int c = blockIdx.x, t = threadIdx.x;
  const int n = cloud_rows(counts, c, cap);
  if (t == 0) {
    if (pass == 0) {
      const double pk = q[2 * c + 1];
      const bool fin = isfinite(centroids[c * 3]) && isfinite(centroids[c * 3 + 1]) && isfinite(centroids[c * 3 + 2]);
      st.prefix = 0; st.rank = 0; st.bits = 0;
      if (n == 0) { st.mode = MODE_REFUSED; st.bits = 1; }
      else if (!fin) { st.mode = MODE_REFUSED; st.bits = 2; }
      else if (pk >= 1.0) st.mode = MODE_ALL;
      else if (pk == 0.5) { st.mode = MODE_THRESHOLD; st.prefix = kZeroKey; }
      else {
        const double v = (double)(n - 1) * q[2 * c];
        const long long lo = (long long)floor(v);
        st.mode = MODE_SELECT;
        st.rank = (uint32_t)(lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo));
      }
    } else {
      st = state[c];
    }
  }
  __syncthreads();
  if (st.mode != MODE_SELECT) {
    if (pass == 0 && t == 0) state[c] = st;
    return;
  }
  uint32_t h = 0;
  const int used = min(slices, (n + ROWS - 1) / ROWS);           // the slices past the cloud's rows hold zeros
  for (int b = 0; b < used; ++b) h += hist[((int64_t)c * slices + b) * 256 + t];
  scan[t] = h;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {                            // inclusive scan of the 256 bins
    const uint32_t add = t >= o ? scan[t - o] : 0u;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  const uint32_t below = scan[t] - h;
  if (st.rank >= below && st.rank < scan[t]) {                   // exactly one bin: the rank is below the total by construction
    CropState o = st;
    o.prefix = (st.prefix << 8) | (uint32_t)t;
    o.rank = st.rank - below;
    if (pass == 3 && o.prefix == kNonFinite) { o.mode = MODE_REFUSED; o.bits = 2; }      // d_(lo) is not finite
    state[c] = o;
  }
}

__device__ __forceinline__ bool kept(uint32_t k, int mode, uint32_t key_lo) {
  return mode == MODE_ALL || (mode != MODE_REFUSED && k != kNonFinite && k > key_lo);
}

// ---- compact, step 1: kept rows of every slice
__global__ __launch_bounds__(CT) void crop_count_kernel(const uint32_t* __restrict__ keys, const int32_t* __restrict__ counts, int cap,
                                                        const CropState* __restrict__ state, int32_t* __restrict__ block_counts) {
  __shared__ int32_t wave_sum[WAVES];
  const int c = blockIdx.y, b = blockIdx.x;
  const int n = cloud_rows(counts, c, cap);
  const int mode = state[c].mode;
  const uint32_t key_lo = state[c].prefix;
  const int hi = min(n, (b + 1) * ROWS);
  int32_t mine = 0;
  for (int i = b * ROWS + (int)threadIdx.x; i < hi; i += CT) mine += kept(keys[(int64_t)c * cap + i], mode, key_lo) ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t s = 0;
    for (int w = 0; w < WAVES; ++w) s += wave_sum[w];
    block_counts[(int64_t)c * gridDim.x + b] = s;
  }
}

// ---- compact, step 2: the slice's base = the counts of the slices before it; rows ranked by ballots in row order; whole rows copied
__global__ __launch_bounds__(CT) void crop_scatter_kernel(const float* __restrict__ in, const uint32_t* __restrict__ keys,
                                                          const int32_t* __restrict__ counts, int cap, int stride,
                                                          const CropState* __restrict__ state, const int32_t* __restrict__ block_counts,
                                                          int out_cap, float* __restrict__ out, int32_t* __restrict__ out_counts,
                                                          int32_t* __restrict__ invalid) {
  __shared__ int32_t red[CT];
  __shared__ int32_t wave_sum[WAVES];
  const int c = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
  const int slices = gridDim.x;
  const int n = cloud_rows(counts, c, cap);
  const int mode = state[c].mode;
  const uint32_t key_lo = state[c].prefix;
  int32_t s = 0;
  for (int k = t; k < b; k += CT) s += block_counts[(int64_t)c * slices + k];
  red[t] = s;
  __syncthreads();
  for (int o = CT / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  int32_t base = red[0];
  if (b == slices - 1 && t == 0) {
    const int32_t total = base + block_counts[(int64_t)c * slices + b];
    out_counts[c] = total;
    invalid[c] = state[c].bits | (total == 0 && state[c].bits == 0 ? 1 : 0);
  }
  const int lane = t & 63, wave = t >> 6;
  const int lo_row = b * ROWS, hi = min(n, lo_row + ROWS);
  for (int r0 = lo_row; r0 < hi; r0 += CT) {                      // uniform trip count over the workgroup
    const int i = r0 + t;
    const bool keep = i < hi && kept(keys[(int64_t)c * cap + i], mode, key_lo);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_sum[wave] = (int32_t)__popcll(m);
    __syncthreads();
    int32_t pos = base + (int32_t)__popcll(m & ((1ull << lane) - 1ull));
    int32_t all = 0;
    for (int w = 0; w < WAVES; ++w) {
      if (w < wave) pos += wave_sum[w];
      all += wave_sum[w];
    }
    if (keep && pos < out_cap) {
      const float* p = in + ((int64_t)c * cap + i) * stride;
      float* o = out + ((int64_t)c * out_cap + pos) * stride;
      for (int ch = 0; ch < stride; ++ch) o[ch] = p[ch];
    }
    base += all;
    __syncthreads();
  }
}

inline bool shape_ok(int clouds, int cap, int stride) {
  return clouds >= 1 && cap >= 1 && stride >= 3 && (int64_t)clouds * cap <= 0x7fffffffll && clouds <= 65535;
}

}  // namespace
}  // namespace dsir

using namespace dsir;

extern "C" {

size_t dsir_t_halfspace_crop_scratch(int clouds, int cap) { return shape_ok(clouds, cap, 3) ? layout(clouds, cap).total : 0; }

int dsir_t_halfspace_crop(void* stream, const float* in, const int32_t* counts, int clouds, int cap, int stride, const float* dirs,
                          const double* p_keep, const double* centroids, int out_cap, float* out, int32_t* out_counts, int32_t* invalid,
                          void* scratch) {
  if (!in || !counts || !dirs || !p_keep || !centroids || !out || !out_counts || !invalid || !scratch || !shape_ok(clouds, cap, stride) ||
      out_cap < 1 || (int64_t)clouds * out_cap > 0x7fffffffll)
    return (int)hipErrorInvalidValue;
  std::vector<double> q((size_t)clouds * 2);
  for (int c = 0; c < clouds; ++c) {
    const double p = p_keep[c];
    if (!(p > 0.0) || std::isinf(p)) return (int)hipErrorInvalidValue;       // NaN, <= 0 or infinite: no such share of a cloud
    q[2 * c] = ((1.0 - p) * 100) / 100;
    q[2 * c + 1] = p;
  }
  hipStream_t st = (hipStream_t)stream;
  const Layout lay = layout(clouds, cap);
  char* base = reinterpret_cast<char*>(scratch);
  uint32_t* keys = reinterpret_cast<uint32_t*>(base + lay.keys);
  uint32_t* hist = reinterpret_cast<uint32_t*>(base + lay.hist);
  CropState* state = reinterpret_cast<CropState*>(base + lay.state);
  double* qd = reinterpret_cast<double*>(base + lay.q);
  int32_t* block_counts = reinterpret_cast<int32_t*>(base + lay.block_counts);
  if (hipMemcpyAsync(qd, q.data(), q.size() * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess) return (int)hipGetLastError();
  const int slices = slices_of(cap);
  const dim3 grid(slices, clouds);
  hipLaunchKernelGGL(crop_project_kernel, grid, dim3(CT), 0, st, in, counts, cap, stride, dirs, centroids, keys, hist);
  hipLaunchKernelGGL(crop_digit_kernel, dim3(clouds), dim3(256), 0, st, (const uint32_t*)hist, slices, counts, cap, (const double*)qd, centroids, 0,
                     state);
  for (int pass = 1; pass < 4; ++pass) {
    hipLaunchKernelGGL(crop_hist_kernel, grid, dim3(CT), 0, st, (const uint32_t*)keys, counts, cap, pass, (const CropState*)state, hist);
    hipLaunchKernelGGL(crop_digit_kernel, dim3(clouds), dim3(256), 0, st, (const uint32_t*)hist, slices, counts, cap, (const double*)qd, centroids,
                       pass, state);
  }
  hipLaunchKernelGGL(crop_count_kernel, grid, dim3(CT), 0, st, (const uint32_t*)keys, counts, cap, (const CropState*)state, block_counts);
  hipLaunchKernelGGL(crop_scatter_kernel, grid, dim3(CT), 0, st, in, (const uint32_t*)keys, counts, cap, stride, (const CropState*)state,
                     (const int32_t*)block_counts, out_cap, out, out_counts, invalid);
  return done();
}

}  // extern "C"
