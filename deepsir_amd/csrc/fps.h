// Farthest-point sampling (fps.hip): what the kernel, its launcher, the entry and tools/fps_check.cpp share - the candidate key, the
// row-to-lane map, the tiers and the scratch layout.  Plain C++ that compiles for the host too.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "scratch.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSIR_FPS_HD __host__ __device__ inline
#else
#define DSIR_FPS_HD inline
#endif

namespace dsir {

constexpr int kFpsMaxRows = 65536;          // rows per cloud the entry takes (the streaming tier's 64 rows per lane x 1024 lanes)
constexpr int kFpsRegisterRows = 8192;      // up to here coordinates and dist stay in registers (8 rows per lane x 1024 lanes)
constexpr int kFpsSmallRows = 1024;         // up to here a 256-thread workgroup (4 rows per lane)

// ---- The candidate key.  dist >= 0 (or +inf), so its fp32 bit pattern orders as an unsigned integer; the low word puts the lower
// index on top among equal dist.  The maximum key of a cloud is the rule's arg-max with its tie-break.  A row that is no candidate
// carries key 0, below every candidate's: i <= 65535 < 0xffffffff leaves a candidate's low word non-zero.
DSIR_FPS_HD unsigned long long fps_key(uint32_t dist_bits, uint32_t i) { return ((unsigned long long)dist_bits << 32) | (0xffffffffu - i); }
DSIR_FPS_HD uint32_t fps_key_index(unsigned long long key) { return 0xffffffffu - (uint32_t)key; }
DSIR_FPS_HD uint32_t fps_key_dist_bits(unsigned long long key) { return (uint32_t)(key >> 32); }
// step 0 runs through the same reduction: every finite row has dist = +inf, and the row `start` - if it is one of them - a high word
// one above +inf's, so the maximum is `start`, else the lowest finite row
constexpr uint32_t kFpsInfBits = 0x7f800000u, kFpsStartBits = 0x7f800001u;

// ---- Tiers: a function of the row capacity alone (never of a cloud's own count: the key makes the bytes independent of it anyway).
struct FpsPlan {
  int threads = 0;      // workgroup size T; row i lives in lane i % T, register slot i / T
  int slots = 0;        // register slots R per lane: T * R >= cap
  bool stream = false;  // coordinates re-read every step from the float4-packed copy (FpsLayout) instead of held in registers
};
inline FpsPlan fps_plan(int cap) {
  FpsPlan p;
  if (cap < 1 || cap > kFpsMaxRows) return p;               // threads == 0: refused
  if (cap <= kFpsSmallRows) { p.threads = 256; p.slots = 4; }
  else if (cap <= kFpsRegisterRows) { p.threads = 1024; p.slots = 8; }
  else { p.threads = 1024; p.slots = 64; p.stream = true; }
  return p;
}
DSIR_FPS_HD int fps_row(int lane, int slot, int threads) { return lane + threads * slot; }
DSIR_FPS_HD int fps_live_slots(int n, int threads) { return (n + threads - 1) / threads; }   // slots that hold a row of a cloud of n rows

// the streaming tier handles its slots in groups of kFpsStreamGroup (that many 16 B loads in flight per lane) and loads a whole group
// without a per-row test: a cloud's slice of the packed copy holds whole groups of slots, zero rows past the cloud's count
constexpr int kFpsStreamGroup = 4;
DSIR_FPS_HD int fps_stream_slots(int live) { return (live + kFpsStreamGroup - 1) / kFpsStreamGroup * kFpsStreamGroup; }
DSIR_FPS_HD int fps_stream_rows(int cap) { return fps_stream_slots(fps_live_slots(cap, 1024)) * 1024; }

// ---- Scratch of one call: the streaming tier's packed copy, xyz4 [clouds][fps_stream_rows(cap)] float4 = (x, y, z, unused); cloud c's
// workgroup writes the slots it will load (fps_stream_slots of its live slots) of its own slice before its first step and reads nothing else of it.  The register tiers take no scratch.
struct FpsLayout {
  size_t xyz4 = 0, bytes = 0;
  FpsLayout(int clouds, int cap) {
    Carve c;
    if (fps_plan(cap).stream) xyz4 = c.take((size_t)clouds * (size_t)fps_stream_rows(cap) * 16);
    bytes = c.p;
  }
};

}  // namespace dsir
