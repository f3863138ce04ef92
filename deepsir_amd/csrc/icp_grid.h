// Cell-indexed ICP search (icp_grid.hip): the per-pair lattice rule and the scratch layout - plain C++ that compiles for the host and
// the device alike, so that the arithmetic can be exercised from a host-only program: tools/icp_grid_check.cpp, built with the
// address and undefined-behaviour sanitizers and run on the CPU (its header gives the command).  The search rule and the containment
// argument are stated in the header of icp_grid.hip; deepsir_amd/icp.py restates the lattice in numpy.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "cell_index.h"

namespace dsir {

constexpr double kIcpGridMargin = 1.0 + 1.0 / 1024.0;   // cell edge over radius: the 2^-10 of overlap.hip's cell_edge
constexpr double kIcpGridMinEdge = 0x1p-60;              // floor of the edge: covers a radius whose fp32 square underflows
constexpr double kIcpGridMaxCells = 1048576.0;           // 2^20: cells the longest axis may span, so c + 1 fits a key's 21 bits

using IcpLattice = CellLattice;                          // one per pair, in device memory

// h = max(r (1 + 2^-10), 2^-60, longest axis extent / 2^20) in fp64
DSIR_CELL_HD double icp_grid_cell_edge(float r, double extent) {
  double h = (double)r * kIcpGridMargin;
  if (!(h >= kIcpGridMinEdge)) h = kIcpGridMinEdge;
  const double coarse = extent / kIcpGridMaxCells;
  return coarse > h ? coarse : h;
}

// lo / hi: the minimum and maximum of the pair's finite reference points; any = false (no finite point): origin 0, extent 0
DSIR_CELL_HD IcpLattice icp_grid_lattice(float r, const float* lo, const float* hi, bool any) {
  IcpLattice L{0.0, 0.0, 0.0, 0.0};
  double ext = 0.0;
  if (any) {
    L.ox = (double)lo[0]; L.oy = (double)lo[1]; L.oz = (double)lo[2];
    for (int a = 0; a < 3; ++a) {
      const double e = (double)hi[a] - (double)lo[a];
      ext = e > ext ? e : ext;
    }
  }
  L.h = icp_grid_cell_edge(r, ext);
  return L;
}

// the grid is refused for a radius whose fp32 square is not finite (the brute search then accepts every point; no lattice of this
// rule has an edge for that)
inline bool icp_grid_radius_ok(float r) { const float r2 = r * r; return r > 0.f && r2 - r2 == 0.f; }
inline bool icp_grid_shape_ok(int pairs, int J, int K) {
  return pairs >= 1 && J >= 1 && K >= 1 && (int64_t)pairs * J <= 0x7fffffffll && (int64_t)pairs * K <= 0x7fffffffll;
}

// the index's parts inside its one piece of scratch: a function of (pairs, J, K) and the sort's temporary size alone, shared by the
// size function and the build.  Every part starts on 256 bytes.  Per pair nothing is shared: part p of every array belongs to pair p.
struct IcpGridLayout {
  size_t lat, enc, off_ref, off_qry, keys, sorted, perm, keys_raw, vals_raw, vals, keys_qry, tmp, tmp_bytes, bytes;
  IcpGridLayout(int pairs, int J, int K, size_t sort_tmp_bytes) {
    const size_t P = (size_t)pairs, nj = P * (size_t)J, nk = P * (size_t)K, nm = nj > nk ? nj : nk;
    Carve c;
    lat = c.take(P * sizeof(IcpLattice));
    enc = c.take(P * 6 * sizeof(uint32_t));          // [3 P] minima, then [3 P] maxima, as ordered integers
    off_ref = c.take((P + 1) * sizeof(int32_t));     // p K
    off_qry = c.take((P + 1) * sizeof(int32_t));     // p J
    keys = c.take(nk * sizeof(uint64_t));            // the reference keys, sorted per pair
    sorted = c.take(nk * 16);                        // (x, y, z, original index) in key order
    perm = c.take(nj * sizeof(int32_t));             // the queries in cell order
    keys_raw = c.take(nm * sizeof(uint64_t));
    vals_raw = c.take(nm * sizeof(uint32_t));
    vals = c.take(nk * sizeof(uint32_t));
    keys_qry = c.take(nj * sizeof(uint64_t));
    tmp_bytes = sort_tmp_bytes;
    tmp = c.take(tmp_bytes < 256 ? 256 : tmp_bytes);
    bytes = c.p;
  }
};

}  // namespace dsir
