// The sparse cell index's shared pieces: the cell coordinate and 64-bit key of a point, the order-preserving fp32 <-> uint32 map of
// the integer min / max, and the gather of a point into (x, y, z, original index).  overlap.hip (one lattice per call, strict `<`,
// its header holds the containment argument) and icp_grid.hip (one lattice per pair on the device, `<=`, argument restated there)
// both build on these.  cell_of and cell_key are plain C++ that compile for the host as well: tools/icp_grid_check.cpp and
// csrc/icp_grid.h use them there.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSIR_CELL_HD __host__ __device__ __forceinline__
#else
#define DSIR_CELL_HD inline
#endif

namespace dsir {

constexpr int MAXC = (1 << 21) - 1;                 // largest coordinate a key holds
constexpr uint64_t KEY_NONE = ~0ull;                // a non-finite point: sorts last, lies in no interval

// the cell coordinate of a finite fp32 value, clamped so that a moved query far outside the lattice stays a valid int
DSIR_CELL_HD int cell_of(float a, double o, double h) {
  double u = floor(((double)a - o) / h);
  u = u < -2.0 ? -2.0 : (u > (double)(MAXC + 2) ? (double)(MAXC + 2) : u);
  return (int)u;
}
DSIR_CELL_HD uint64_t cell_key(int x, int y, int z) { return (uint64_t)x | ((uint64_t)y << 21) | ((uint64_t)z << 42); }
DSIR_CELL_HD bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

#if defined(__HIPCC__) || defined(__CUDACC__)
// order-preserving map fp32 -> uint32, for integer min / max
__device__ __forceinline__ uint32_t f2ord(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float ord2f(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// (x, y, z, original index): the point a sorted position stands for, its index carried as the fourth float's bits
__device__ __forceinline__ float4 gather_xyzi(const float* __restrict__ p, uint32_t v) { return make_float4(p[0], p[1], p[2], __uint_as_float(v)); }
#endif

}  // namespace dsir
