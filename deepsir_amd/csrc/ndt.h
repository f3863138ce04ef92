// NDT registration (ndt.hip): the per-pair lattice, the score constants, the partition of a pair's source points and the scratch
// layout - plain C++ that compiles for the host and the device alike, so that the arithmetic can be exercised from a host-only
// program: tools/ndt_check.cpp, built with the address and undefined-behaviour sanitizers and run on the CPU (its header gives the
// command).  The rule itself is stated in the header of ndt.hip and restated in deepsir_amd/ndt.py.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "cell_index.h"
#include "icp_plane.h"

namespace dsir {

constexpr int kNdtChunk = kIcpPlaneChunk;   // source points per accumulating workgroup: a constant, so the partition - hence the
                                            // summation order - of a pair depends on Jp alone (the chunks are icp_plane_chunks')
constexpr int kNdtSums = 31;                // A (21, upper triangle by rows), b (6), score, matched points, contributing visits (rows),
                                            // source points that are not finite
constexpr int kNdtSlots = 32;               // doubles per (pair, chunk) partial
constexpr int kNdtScore = 27, kNdtMatched = 28, kNdtRows = 29, kNdtBad = 30;
constexpr int kNdtMinPoints = 6;            // a cell of fewer points has no Gaussian (PCL's min_points_per_voxel)
constexpr double kNdtEigMult = 0.01;        // lambda_i' = max(lambda_i, 0.01 lambda_1) (PCL's min_covar_eigvalue_mult)
constexpr int kNdtRecord = 10;              // doubles per cell record: mu (3), B (6: 00 01 02 11 12 22), n
constexpr double kNdtMaxCells = 1048576.0;  // 2^20: cells the longest axis may span, so every coordinate fits a key's 21 bits
constexpr int kNdtState = 4;                // doubles per pair: iterations run, identity updates (done has its own ping-pong flags)

// h = max((double)res, longest axis extent / 2^20) in fp64: no margin, NDT has no radius to contain
DSIR_CELL_HD double ndt_cell_edge(float res, double extent) {
  const double h = (double)res, coarse = extent / kNdtMaxCells;
  return coarse > h ? coarse : h;
}

// lo / hi: the minimum and maximum of the pair's finite reference rows; any = false (no finite row): origin 0, edge res, no cell
DSIR_CELL_HD CellLattice ndt_lattice(float res, const float* lo, const float* hi, bool any) {
  CellLattice L{0.0, 0.0, 0.0, 0.0};
  double ext = 0.0;
  if (any) {
    L.ox = (double)lo[0]; L.oy = (double)lo[1]; L.oz = (double)lo[2];
    for (int a = 0; a < 3; ++a) {
      const double e = (double)hi[a] - (double)lo[a];
      ext = e > ext ? e : ext;
    }
  }
  L.h = ndt_cell_edge(res, ext);
  return L;
}

// PCL's score constants from the outlier ratio o and the resolution, in fp64 on the host; passed to the kernels as doubles
struct NdtConstants { double d1, d2, d3; };
inline NdtConstants ndt_constants(double outlier_ratio, float res) {
  const double r = (double)res;
  const double c1 = 10.0 * (1.0 - outlier_ratio), c2 = outlier_ratio / (r * r * r);
  NdtConstants k;
  k.d3 = -log(c2);
  k.d1 = -log(c1 + c2) - k.d3;
  k.d2 = -2.0 * log((-log(c1 * exp(-0.5) + c2) - k.d3) / k.d1);
  return k;
}

inline bool ndt_positive_finite(float v) { return v > 0.f && v - v == 0.f; }
inline bool ndt_shape_ok(int pairs, int J, int K) {
  return pairs >= 1 && J >= 1 && K >= 1 && (int64_t)pairs * J <= 0x7fffffffll && (int64_t)pairs * K <= 0x7fffffffll;
}
// resolution and step_tol positive and finite, outlier_ratio inside (0, 1) with constants that are finite and a positive d2,
// neighbors 1 or 7
inline bool ndt_args_ok(float res, int neighbors, float step_tol, float outlier_ratio) {
  if (!ndt_positive_finite(res) || !ndt_positive_finite(step_tol)) return false;
  if (!(outlier_ratio > 0.f && outlier_ratio < 1.f)) return false;
  if (neighbors != 1 && neighbors != 7) return false;
  const NdtConstants k = ndt_constants((double)outlier_ratio, res);
  return k.d1 - k.d1 == 0.0 && k.d3 - k.d3 == 0.0 && k.d2 > 0.0 && k.d2 - k.d2 == 0.0;
}

// Why the cells (cx - 1, cx, cx + 1) of one (y, z) are ONE key interval: a key is x | y << 21 | z << 42 with 0 <= x <= MAXC, so for a
// fixed (y, z) the key is (y << 21 | z << 42) + x, increasing in x, and every key of another (y', z') differs in the bits above 21 -
// it is below key(0, y, z) or above key(MAXC, y, z).  So the sorted keys in [key(x0, y, z), key(x1, y, z)] are exactly the cells
// x0 .. x1 of that (y, z), in ascending x: one lower bound, then at most three runs (tools/ndt_check.cpp counts it out).
DSIR_CELL_HD bool ndt_in_key(int c) { return c >= 0 && c <= MAXC; }

// The map's and the loop's parts inside one piece of scratch: a function of (pairs, J, K) and the sort's temporary size alone, shared
// by the size function and the launchers.  Every part starts on 256 bytes; part p of every array belongs to pair p.  J = 0: the map alone.
struct NdtLayout {
  size_t lat, enc, off_ref, keys, vals, runs, records, keys_raw, vals_raw, tmp, tmp_bytes, cur, Ta, Tb, part, state, done, bytes;
  NdtLayout(int pairs, int J, int K, size_t sort_tmp_bytes) {
    const size_t P = (size_t)pairs, nj = P * (size_t)J, nk = P * (size_t)K;
    Carve c;
    lat = c.take(P * sizeof(CellLattice));
    enc = c.take(P * 6 * sizeof(uint32_t));                       // [3 P] minima, then [3 P] maxima, as ordered integers
    off_ref = c.take((P + 1) * sizeof(int32_t));                  // p K
    keys = c.take(nk * sizeof(uint64_t));                         // the reference keys, sorted per pair
    vals = c.take(nk * sizeof(uint32_t));                         // the original index of every sorted position
    runs = c.take(nk * sizeof(int32_t));                          // at a run's first position its length, else 0
    records = c.take(nk * kNdtRecord * sizeof(double));           // at a valid cell's first position its record, else 0
    keys_raw = c.take(nk * sizeof(uint64_t));
    vals_raw = c.take(nk * sizeof(uint32_t));
    tmp_bytes = sort_tmp_bytes;
    tmp = c.take(tmp_bytes < 256 ? 256 : tmp_bytes);
    cur = c.take(nj * 12);                                        // the source points under the current pose [pairs][J][3]
    Ta = c.take(P * 48);                                          // the cumulative pose, ping
    Tb = c.take(P * 48);                                          // and pong
    part = c.take(P * (size_t)icp_plane_chunks(J) * kNdtSlots * sizeof(double));
    state = c.take(P * kNdtState * sizeof(double));
    done = c.take(2 * P * sizeof(int32_t));                       // the pairs' done flags, ping [P] and pong [P]
    bytes = c.p;
  }
};

}  // namespace dsir
