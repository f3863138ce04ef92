// seg_sort.h: uniform segment offsets and the temporary sizes of hipCUB's segmented radix sorts (library calls, not the hot path).
#include <hipcub/hipcub.hpp>

#include "seg_sort.h"

namespace dsir {

namespace {

__global__ void seg_offsets_kernel(int* seg, int segments, int len) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= segments; i += gridDim.x * blockDim.x) seg[i] = i * len;
}

template <class K, class V>
size_t pairs_tmp_bytes(int64_t total, int segments) {
  size_t b = 0;
  hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, b, (const K*)nullptr, (K*)nullptr, (const V*)nullptr, (V*)nullptr, (int)total, segments,
                                              (const int*)nullptr, (const int*)nullptr);
  return b;
}

}  // namespace

void launch_seg_offsets(int* seg, int segments, int len, hipStream_t st) {
  hipLaunchKernelGGL(seg_offsets_kernel, dim3(1), dim3(256), 0, st, seg, segments, len);
}

size_t seg_sort_pairs_u32_tmp_bytes(int64_t total, int segments) { return pairs_tmp_bytes<uint32_t, uint32_t>(total, segments); }
size_t seg_sort_tmp_bytes(int64_t total, int segments) { return pairs_tmp_bytes<uint64_t, uint32_t>(total, segments); }

size_t seg_sort_keys_desc_tmp_bytes(int64_t total, int segments) {
  size_t b = 0;
  hipcub::DeviceSegmentedRadixSort::SortKeysDescending(nullptr, b, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)total,
                                                       segments, (const int*)nullptr, (const int*)nullptr);
  return b;
}

size_t seg_sort_keys_i64_tmp_bytes(int64_t total, int segments) {
  size_t b = 0;
  hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, b, (const int64_t*)nullptr, (int64_t*)nullptr, (int)total, segments, (const int*)nullptr,
                                             (const int*)nullptr);
  return b;
}

}  // namespace dsir
