// The sparse cell index, stated once for overlap.hip (one lattice per call, one lane per query) and icp_grid.hip (one lattice per pair
// made on the device, eight lanes per query): lattice, cell coordinate, key and overlap.hip's layout (carved with scratch.h) as plain C++ that
// compiles for the host too (tools/icp_grid_check.cpp); for the device the bounds accumulation, gather, distance rule and key walk.
//
// Why the 27 cells around c(a) hold every b the rule accepts for a query a - the part both users share.  The rule is
//     d = b - a,  d2 = (dx dx + dy dy) + dz dz      fp32, every operation rounded on its own (dist2_rn)
// and b is accepted when d2 is below fl(r r), strictly or not.  Every term of d2 is non-negative and rounding is monotone, so
// fl(dx dx) <= d2; with d2 bounded by fl(r r) that gives dx^2 bounded by r^2 (1 + 2^-24) / (1 - 2^-24) and, dx = fl(b - a) being
// within 2^-24 of b - a, |b - a| bounded by r (1 + 2^-21) per axis in exact arithmetic.  With a cell edge h >= r (1 + 2^-10),
// |b - a| / h is bounded by (1 + 2^-21) / (1 + 2^-10) < 1 - 2^-11.  The cell coordinate c(a) = floor(((double)a - (double)o) / h)
// is computed in fp64 from the fp32 values: subtraction and division carry a relative error of 2^-52 on quotients below 2^21 + 2
// (the clamp of cell_of), less than 2^-29 absolute, so the two computed quotients differ by less than 1 and their floors by at
// most 1.  What differs between the users is the inequality and how c + 1 is kept inside a key's 21 bits per axis: overlap.hip
// accepts with a strict `<` and refuses an extent of more than 2^21 - 2 cells; icp_grid.hip accepts with `<=` and coarsens the
// edge instead.  Each file's header has its own two lines on that.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "scratch.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSIR_CELL_HD __host__ __device__ __forceinline__
#else
#define DSIR_CELL_HD inline
#endif

namespace dsir {

constexpr int MAXC = (1 << 21) - 1;                 // largest coordinate a key holds
constexpr uint64_t KEY_NONE = ~0ull;                // a non-finite point: sorts last, lies in no interval

struct CellLattice { double ox, oy, oz, h; };       // origin and cell edge

// the cell coordinate of a finite fp32 value, clamped so that a moved query far outside the lattice stays a valid int
DSIR_CELL_HD int cell_of(float a, double o, double h) {
  double u = floor(((double)a - o) / h);
  u = u < -2.0 ? -2.0 : (u > (double)(MAXC + 2) ? (double)(MAXC + 2) : u);
  return (int)u;
}
DSIR_CELL_HD uint64_t cell_key(int x, int y, int z) { return (uint64_t)x | ((uint64_t)y << 21) | ((uint64_t)z << 42); }
DSIR_CELL_HD bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// the key an indexed point is sorted by: its cell, every coordinate clamped into the key's 21 bits; KEY_NONE for a non-finite point
DSIR_CELL_HD uint64_t point_key(float x, float y, float z, const CellLattice& L) {
  if (!finite3(x, y, z)) return KEY_NONE;
  const int cx = cell_of(x, L.ox, L.h), cy = cell_of(y, L.oy, L.h), cz = cell_of(z, L.oz, L.h);
  return cell_key(cx < 0 ? 0 : (cx > MAXC ? MAXC : cx), cy < 0 ? 0 : (cy > MAXC ? MAXC : cy), cz < 0 ? 0 : (cz > MAXC ? MAXC : cz));
}

// the lattice of overlap.hip's index (searched by radius_nn.hip too): the cell edge r (1 + 2^-10) in fp64, the origin the bounds' minimum
inline double nn_cell_edge(float r) { return (double)r * (1.0 + 1.0 / 1024.0); }
inline CellLattice nn_lattice(const float* bounds, float r) { return CellLattice{(double)bounds[0], (double)bounds[1], (double)bounds[2], nn_cell_edge(r)}; }

// overlap.hip's index inside its one allocation, from (total, fragments) and the sort's temporary size: _scratch, _build, _within
struct IndexLayout {
  size_t keys, sorted, box, off, keys_raw, vals_raw, vals, tmp, tmp_bytes, bytes;
  IndexLayout(int64_t total, int F, size_t sort_tmp_bytes) {
    const size_t n = (size_t)(total < 1 ? 1 : total);
    Carve c;
    keys = c.take(n * sizeof(uint64_t));
    sorted = c.take(n * 16);                        // (x, y, z, original index) in key order
    box = c.take((size_t)F * 6 * sizeof(int32_t));
    off = c.take((size_t)(F + 1) * sizeof(int32_t));
    keys_raw = c.take(n * sizeof(uint64_t));
    vals_raw = c.take(n * sizeof(uint32_t));
    vals = c.take(n * sizeof(uint32_t));
    tmp_bytes = sort_tmp_bytes;
    tmp = c.take(tmp_bytes < 256 ? 256 : tmp_bytes);
    bytes = c.p;
  }
};

#if defined(__HIPCC__) || defined(__CUDACC__)
// order-preserving map fp32 -> uint32, for integer min / max
__device__ __forceinline__ uint32_t f2ord(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float ord2f(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// min / max xyz of the finite rows start, start + step, .. below n, as ordered integers: the thread's rows, the wave's butterfly,
// then lane 0's integer atomics (order-independent) on enc_lo [3] / enc_hi [3].  Every lane of the wave must call it.
__device__ __forceinline__ void finite_bounds_accumulate(const float* __restrict__ rows, int stride, int64_t n, int64_t start, int64_t step,
                                                         uint32_t* __restrict__ enc_lo, uint32_t* __restrict__ enc_hi) {
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  for (int64_t i = start; i < n; i += step) {
    const float* p = rows + i * stride;
    const float v[3] = {p[0], p[1], p[2]};
    if (!finite3(v[0], v[1], v[2])) continue;
#pragma unroll
    for (int a = 0; a < 3; ++a) { const uint32_t o = f2ord(v[a]); lo[a] = min(lo[a], o); hi[a] = max(hi[a], o); }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    for (int s = 32; s > 0; s >>= 1) { lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], s)); hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], s)); }
    if ((threadIdx.x & 63) == 0) { atomicMin(enc_lo + a, lo[a]); atomicMax(enc_hi + a, hi[a]); }
  }
}

// (x, y, z, original index): the point a sorted position stands for, its index carried as the fourth float's bits
__device__ __forceinline__ float4 gather_xyzi(const float* __restrict__ p, uint32_t v) { return make_float4(p[0], p[1], p[2], __uint_as_float(v)); }

// the rule's squared distance from (x, y, z) to t: d = t - (x, y, z), (dx dx + dy dy) + dz dz, every operation rounded on its own
__device__ __forceinline__ float dist2_rn(const float4& t, float x, float y, float z) {
  const float dx = __fsub_rn(t.x, x), dy = __fsub_rn(t.y, y), dz = __fsub_rn(t.z, z);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// the first position of the ascending keys [n] whose key is >= klo
__device__ __forceinline__ int key_lower_bound(const uint64_t* __restrict__ keys, int n, uint64_t klo) {
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (keys[mid] < klo) lo = mid + 1; else hi = mid; }
  return lo;
}

// the 27 cells around (cx, cy, cz) as nine key intervals, one per (dy, dz) in {-1, 0, 1}^2: f(klo, khi) with klo = key(cx - 1, y, z),
// khi = key(cx + 1, y, z), x clamped into the key.  Rows outside the key's range or the open box ylo < y < yhi, zlo < z < zhi are left out.
template <class F>
__device__ __forceinline__ void walk_key_intervals(int cx, int cy, int cz, int ylo, int yhi, int zlo, int zhi, F&& f) {
  const int x0 = max(cx - 1, 0), x1 = min(cx + 1, MAXC);
  if (x1 < x0) return;
  for (int dz = -1; dz <= 1; ++dz) {
    const int zz = cz + dz;
    if (zz < 0 || zz > MAXC || zz <= zlo || zz >= zhi) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = cy + dy;
      if (yy < 0 || yy > MAXC || yy <= ylo || yy >= yhi) continue;
      f(cell_key(x0, yy, zz), cell_key(x1, yy, zz));
    }
  }
}
#endif

}  // namespace dsir
