// What the users of hipCUB's segmented radix sort share (seg_sort.hip): the offsets of equal-length segments and the sorts' temporary
// sizes.  The sorts, their bit ranges and their place on the stream stay with select, resample, consensus, match_targets, icp_grid, overlap.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace dsir {

// seg[i] = i * len for i in [0, segments]: one block, before the sort on `st`
void launch_seg_offsets(int* seg, int segments, int len, hipStream_t st);

// temporary bytes of a sort of `total` items in `segments` segments
size_t seg_sort_pairs_u32_tmp_bytes(int64_t total, int segments);   // SortPairs, (uint32 key, uint32 value)
size_t seg_sort_tmp_bytes(int64_t total, int segments);             // SortPairs, (uint64 key, uint32 value)
size_t seg_sort_keys_desc_tmp_bytes(int64_t total, int segments);   // SortKeysDescending, 64-bit unsigned keys
size_t seg_sort_keys_i64_tmp_bytes(int64_t total, int segments);    // SortKeys, int64 keys

}  // namespace dsir
