// Plane segmentation (plane.hip): what the kernels, the launcher, the entry and tools/plane_check.cpp share - the draw arithmetic, the
// pick key, the launch geometry that depends on the shape alone, the limits and the scratch layout.  Plain C++ that compiles for the
// host too.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "scratch.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSIR_PLANE_HD __host__ __device__ inline
#else
#define DSIR_PLANE_HD inline
#endif

namespace dsir {

// ---- Limits: the entry refuses, and does not clamp, what lies outside them.
constexpr int kPlaneMaxClouds = 65535;            // grid.y / grid.z
constexpr int kPlaneMaxHyp = 1 << 20;             // h << 8 stays below the round's field (j << 32) of the draw key
constexpr int kPlaneMaxPlanes = 8;
constexpr int kPlaneMinInliers = 3;
constexpr int kPlaneMaxRefits = 8;

DSIR_PLANE_HD bool plane_shape_ok(int clouds, int cap, int H) {
  return clouds >= 1 && clouds <= kPlaneMaxClouds && cap >= 1 && (int64_t)clouds * cap < ((int64_t)1 << 31) && H >= 1 && H <= kPlaneMaxHyp;
}

// ---- Draws.  splitmix64 (Vigna), the generator of device_utils.h, restated so that the host check can call it.
DSIR_PLANE_HD uint64_t plane_mix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the cloud's key: cloud `id` of a call with seed s is cloud 0 of a call with seed s ^ (id << 40)
DSIR_PLANE_HD uint64_t plane_cloud_key(uint64_t seed, uint32_t id) { return plane_mix64(seed ^ ((uint64_t)id << 40)); }
// draw k of hypothesis h in round j among n_live rows: a position in the live list, in [0, n_live)
DSIR_PLANE_HD uint32_t plane_draw(uint64_t cloud_key, int j, int h, int k, uint32_t n_live) {
  const uint64_t d = plane_mix64(cloud_key ^ ((uint64_t)j << 32) ^ ((uint64_t)h << 8) ^ (uint64_t)k);
  return (uint32_t)(((d >> 32) * (uint64_t)n_live) >> 32);
}

// ---- The pick key: the largest count wins, ties to the lower h.  A scored hypothesis has h < 2^32 - 1: its key is never 0.
DSIR_PLANE_HD unsigned long long plane_pick_key(uint32_t count, uint32_t h) { return ((unsigned long long)count << 32) | (0xFFFFFFFFu - h); }
DSIR_PLANE_HD uint32_t plane_key_h(unsigned long long key) { return 0xFFFFFFFFu - (uint32_t)key; }
DSIR_PLANE_HD uint32_t plane_key_count(unsigned long long key) { return (uint32_t)(key >> 32); }

// ---- Geometry, a function of the shape alone (never of a cloud's own count).
constexpr int kPlaneRowBlock = 256;       // rows per workgroup of the live-list and label kernels
constexpr int kPlaneHypBlock = 128;       // hypotheses per fitting workgroup, one per lane
constexpr int kPlaneScoreLanes = 256;     // lanes of a scoring workgroup = live points per LDS chunk
constexpr int kPlaneCandPerLane = 2;      // candidates a scoring lane holds: one LDS read serves two tests
constexpr int kPlaneScoreCands = kPlaneScoreLanes * kPlaneCandPerLane;
constexpr int kPlaneRefitSlice = 4096;    // live rows per workgroup of the refit sums: row q of the live list belongs to slice
                                          // q / 4096, lane q % 256, and a lane adds its 16 rows in ascending order
inline int plane_row_blocks(int cap) { return (cap + kPlaneRowBlock - 1) / kPlaneRowBlock; }
inline int plane_hyp_blocks(int H) { return (H + kPlaneScoreCands - 1) / kPlaneScoreCands; }
inline int plane_refit_slices(int cap) { return (cap + kPlaneRefitSlice - 1) / kPlaneRefitSlice; }
// chunks of 256 live points per scoring slice: about two workgroups per CU where the problem allows it, whole chunks per slice
inline int plane_chunks_per_slice(int cap, int hyp_blocks, int clouds) {
  const int nch = (cap + kPlaneScoreLanes - 1) / kPlaneScoreLanes;
  const int64_t wgs = (int64_t)hyp_blocks * clouds;
  int want = (int)((512 + wgs - 1) / wgs);
  want = want < 1 ? 1 : (want > nch ? nch : want);
  return (nch + want - 1) / want;
}
inline int plane_score_slices(int cap, int cps) { return ((cap + kPlaneScoreLanes - 1) / kPlaneScoreLanes + cps - 1) / cps; }

// ---- Scratch of one call.  Per cloud c:
//   live      [cap] i32     the live rows in ascending order, rebuilt every round; the first n_live[c] are meaningful
//   pts4      [cap] float4  (x, y, z, unused) of the live rows, in the live list's order: what the draws and the scoring read
//   blocks    [row blocks] i32   live rows per block of 256 rows
//   n_live, done, cur_cnt, trial_cnt, trial_ok, kept   [1] i32
//   hyp       [H][6] f32    (nx, ny, nz, ax, ay, az);  hyp_ok, hyp_cnt [H] i32
//   info      [2] i32       {winning h, valid hypotheses};  first_cnt [1] i32: the count before the refits
//   cur, trial [6] f32      the kept plane of the round and the refit under test
//   sum1      [slices][4] f64   {count, sum x, sum y, sum z} of the inliers, per refit slice
//   sum2      [slices][6] f64   {xx, xy, xz, yy, yz, zz} about the centroid
struct PlaneLayout {
  size_t live = 0, pts4 = 0, blocks = 0, n_live = 0, done = 0, hyp = 0, hyp_ok = 0, hyp_cnt = 0, info = 0, first_cnt = 0, cur = 0, cur_cnt = 0,
         trial = 0, trial_cnt = 0, trial_ok = 0, kept = 0, sum1 = 0, sum2 = 0, bytes = 0;
  int row_blocks = 0, slices = 0;
  PlaneLayout(int clouds, int cap, int H) {
    Carve c;
    const size_t C = (size_t)clouds;
    row_blocks = plane_row_blocks(cap);
    slices = plane_refit_slices(cap);
    pts4 = c.take(C * (size_t)cap * 16);
    live = c.take(C * (size_t)cap * 4);
    blocks = c.take(C * (size_t)row_blocks * 4);
    n_live = c.take(C * 4); done = c.take(C * 4);
    hyp = c.take(C * (size_t)H * 24); hyp_ok = c.take(C * (size_t)H * 4); hyp_cnt = c.take(C * (size_t)H * 4);
    info = c.take(C * 8); first_cnt = c.take(C * 4);
    cur = c.take(C * 24); cur_cnt = c.take(C * 4);
    trial = c.take(C * 24); trial_cnt = c.take(C * 4); trial_ok = c.take(C * 4); kept = c.take(C * 4);
    sum1 = c.take(C * (size_t)slices * 32); sum2 = c.take(C * (size_t)slices * 48);
    bytes = c.p;
  }
};

}  // namespace dsir
