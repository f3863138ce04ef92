// The scratch of the ICP loop and of the single search step (icp.hip) as offsets into one piece, read by the size function and the
// launcher alike: plain host C++ (tools/icp_grid_check.cpp lays it out on the CPU).  The cell index's part (IcpGridLayout) comes in as a size.
#pragma once
#include "cell_index.h"
#include "icp_plane.h"

namespace dsir {

// launch_icp_refine: a part that is not needed (the plane estimator's, the grid's) takes no bytes and its offset is not read
struct IcpLayout {
  size_t cur, idx, d2, w, Ta, Tb, state, skip, Tstep, part, nsing, grid, bytes;
  IcpLayout(int pairs, int J, bool plane, size_t grid_bytes) {
    const size_t P = (size_t)pairs, n = P * (size_t)J;
    Carve c;
    cur = c.take(n * 12);                                    // the source points under the current pose [pairs][J][3]
    idx = c.take(n * 4);                                     // the correspondences of the last search
    d2 = c.take(n * 4);
    w = c.take(n * 4);                                       // 0 / 1 weights of the estimators
    Ta = c.take(P * 48);                                     // the cumulative pose, ping
    Tb = c.take(P * 48);                                     // and pong
    state = c.take(P * 32);                                  // {fitness, rmse, done, iterations} doubles
    skip = c.take(P * 4);                                    // the pair's `done` as the flag the update and the search read
    Tstep = c.take(P * 48);                                  // the Kabsch step's own transform
    part = c.take(plane ? icp_plane_part_bytes(pairs, J) : 0);   // [pairs][chunks][kIcpPlaneSlots] partial sums
    nsing = c.take(plane ? P * sizeof(double) : 0);          // identity updates taken for a singular system
    grid = c.take(grid_bytes);                               // the cell index (IcpGridLayout), 0 for the brute search
    bytes = c.p;
  }
};

// launch_icp_correspondences: the moved points, then the cell index
struct IcpCorrLayout {
  size_t cur, grid, bytes;
  IcpCorrLayout(int pairs, int J, size_t grid_bytes) {
    Carve c;
    cur = c.take((size_t)pairs * (size_t)J * 12);
    grid = c.take(grid_bytes);
    bytes = c.p;
  }
};

}  // namespace dsir
