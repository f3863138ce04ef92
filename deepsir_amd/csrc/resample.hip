// Every cloud of a padded batch [clouds][cap][stride] resampled to exactly k rows (reference dataloader/transformation.py:72-93
// Resampler / FixedResampler), once, for the engine (dsir_resample) and the training loader (dsir_t_resample_keyed).  The rule,
// restated in oracle/preprocess.py and deepsir_amd/augment.py:
//     n = min(counts[c], cap) live rows; n <= 0: the cloud's k rows are zeros (rows: 0)
//     key of live row i = splitmix64(perm_base ^ i) >> 1 (63 bits), all-ones for padding; a stable segmented sort by key gives the
//     cloud's permutation perm (ties by index, padding last)
//     mode 0 (Resampler):       row j = perm[j] for j < n, then top-up with replacement: splitmix64(topup_base ^ j) % n
//     mode 1 (FixedResampler):  row j = j % n, no draw
//     mode 2 (the loader's permutation, then FixedResampler): row j = perm[j % n]
// What differs between the two entries is where a cloud's (perm_base, topup_base, mode) come from - the `Draws` of the kernels:
//     SeedDraws   (seed ^ c << 40, ~seed ^ c << 40, the call's mode): position c in the call is part of the draw
//     KeyedDraws  (key ^ STREAM_PERM, key ^ STREAM_TOPUP, prm[c].rmode): the cloud's own key, never its position in a batch
// The segmented sort is a library call (hipCUB), skipped when no cloud of the call reads perm.
#include <hipcub/hipcub.hpp>

#include "kernels.h"
#include "device_utils.h"
#include "augment_params.h"
#include "op_layouts.h"
#include "seg_sort.h"
#include "dsir_train.h"

namespace dsir {

namespace {

constexpr uint64_t kPadKey = ~0ull;

struct CloudDraws { uint64_t perm_base, topup_base; int mode; };

struct SeedDraws {
  uint64_t seed; int mode;
  __device__ CloudDraws operator()(int c) const { return {seed ^ ((uint64_t)c << 40), ~seed ^ ((uint64_t)c << 40), mode}; }
};
struct KeyedDraws {
  const AugParams* prm;
  __device__ CloudDraws operator()(int c) const { return {prm[c].key ^ STREAM_PERM, prm[c].key ^ STREAM_TOPUP, (int)prm[c].rmode}; }
};

inline int grid_for(int64_t n) { const int64_t g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g)); }

template <class Draws>
__global__ void resample_key_kernel(const int32_t* __restrict__ counts, Draws draws, int clouds, int cap, uint64_t* __restrict__ keys,
                                    uint32_t* __restrict__ vals) {
  const int64_t total = (int64_t)clouds * cap;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(e / cap), i = (int)(e % cap);
    const int n = min(counts[c], cap);
    keys[e] = i < n ? (splitmix64(draws(c).perm_base ^ (uint64_t)i) >> 1) : kPadKey;   // top bit clear: padding sorts last
    vals[e] = (uint32_t)i;
  }
}

// out [clouds][k][stride]; rows (optional) [clouds][k]: the source row of every output row
template <class Draws>
__global__ void resample_gather_kernel(const float* __restrict__ in, const int32_t* __restrict__ counts, Draws draws,
                                       const uint32_t* __restrict__ perm, int clouds, int cap, int stride, int k, float* __restrict__ out,
                                       int32_t* __restrict__ rows) {
  const int64_t total = (int64_t)clouds * k;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(e / k), j = (int)(e % k);
    const int n = min(counts[c], cap);
    float* o = out + e * stride;
    if (n <= 0) {
      for (int ch = 0; ch < stride; ++ch) o[ch] = 0.f;
      if (rows) rows[e] = 0;
      continue;
    }
    const CloudDraws d = draws(c);
    int srow;
    if (d.mode == 1) srow = j % n;                                                   // FixedResampler: tile / prefix
    else if (d.mode == 2) srow = (int)perm[(int64_t)c * cap + j % n];                // the loader's permutation, then FixedResampler
    else if (j < n) srow = (int)perm[(int64_t)c * cap + j];                          // Resampler: random order, no repeats
    else srow = (int)(splitmix64(d.topup_base ^ (uint64_t)j) % (uint64_t)n);         // top-up with replacement
    const float* s = in + ((int64_t)c * cap + srow) * stride;
    for (int ch = 0; ch < stride; ++ch) o[ch] = s[ch];
    if (rows) rows[e] = srow;
  }
}

inline size_t sort_tmp_bytes(int clouds, int cap) { return seg_sort_tmp_bytes((int64_t)clouds * cap, clouds); }
inline size_t scratch_bytes(int clouds, int cap) { return SegSortLayout(clouds, cap, 8, sort_tmp_bytes(clouds, cap)).bytes; }

// offsets, keys, sort (only when `sort`: some cloud reads perm), gather; false: the sort failed
template <class Draws>
bool resample(const Draws& draws, const float* in, const int32_t* counts, int clouds, int cap, int stride, int k, bool sort, float* out,
              int32_t* rows, void* scratch, hipStream_t st) {
  const int64_t total = (int64_t)clouds * cap;
  size_t tb = sort_tmp_bytes(clouds, cap);
  const SegSortLayout lay(clouds, cap, 8, tb);
  uint64_t *k0 = at<uint64_t>(scratch, lay.k0), *k1 = at<uint64_t>(scratch, lay.k1);
  uint32_t *v0 = at<uint32_t>(scratch, lay.v0), *v1 = at<uint32_t>(scratch, lay.v1);
  int* seg = at<int>(scratch, lay.seg);
  if (sort) {
    launch_seg_offsets(seg, clouds, cap, st);
    hipLaunchKernelGGL(resample_key_kernel<Draws>, dim3(grid_for(total)), dim3(256), 0, st, counts, draws, clouds, cap, k0, v0);
    if (hipcub::DeviceSegmentedRadixSort::SortPairs(at<char>(scratch, lay.tmp), tb, k0, k1, v0, v1, (int)total, clouds, seg, seg + 1, 0, 64, st) !=
        hipSuccess)
      return false;
  }
  hipLaunchKernelGGL(resample_gather_kernel<Draws>, dim3(grid_for((int64_t)clouds * k)), dim3(256), 0, st, in, counts, draws, (const uint32_t*)v1,
                     clouds, cap, stride, k, out, rows);
  return true;
}

}  // namespace

size_t resample_scratch_bytes(int clouds, int cap) { return scratch_bytes(clouds, cap); }

int launch_resample(const float* in, const int32_t* counts, int clouds, int cap, int stride, int k, int mode, uint64_t seed,
                    float* out, void* scratch, hipStream_t st) {
  const int64_t total = (int64_t)clouds * cap;
  if (total <= 0 || total > 0x7fffffffll || k < 1 || stride < 1) return 1;
  return resample(SeedDraws{seed, mode}, in, counts, clouds, cap, stride, k, mode == 0, out, nullptr, scratch, st) ? 0 : 2;
}

}  // namespace dsir

using namespace dsir;

extern "C" {

size_t dsir_t_resample_keyed_scratch(int clouds, int cap) { return aug_shape_ok(clouds, cap, 3) ? scratch_bytes(clouds, cap) : 0; }

int dsir_t_resample_keyed(void* stream, const float* in, const int32_t* counts, int clouds, int cap, int stride, int k, const void* params,
                          int need_perm, float* out, int32_t* rows, void* scratch) {
  if (!in || !counts || !params || !out || !scratch || !aug_shape_ok(clouds, cap, stride) || k < 1 || (int64_t)clouds * k > 0x7fffffffll)
    return (int)hipErrorInvalidValue;
  if (!resample(KeyedDraws{reinterpret_cast<const AugParams*>(params)}, in, counts, clouds, cap, stride, k, need_perm != 0, out, rows, scratch,
                (hipStream_t)stream))
    return (int)hipErrorUnknown;
  return (int)hipGetLastError();
}

}  // extern "C"
