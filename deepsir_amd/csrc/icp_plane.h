// Point-to-plane ICP update (icp.hip): the partition of a pair's correspondences, the scratch it needs, and the 6 x 6 solve with its
// singularity test - plain C++ that compiles for the host and the device alike, so that the arithmetic can be exercised from a
// host-only program: tools/icp_plane_check.cpp, built with the address and undefined-behaviour sanitizers and run on the CPU (its
// header gives the command).  The rule itself is stated in the header of icp.hip and restated in tests/icp_plane_host.py.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSIR_HD __host__ __device__
#else
#define DSIR_HD
#endif

namespace dsir {

constexpr int kIcpPlaneChunk = 1024;   // source points per accumulating workgroup: a function of nothing, so the partition - hence
                                       // the summation order - of a pair depends on J alone
constexpr int kIcpPlaneSums = 29;      // A (21, upper triangle by rows), b (6), rows used, source points that are not finite
constexpr int kIcpPlaneSlots = 32;     // doubles per (pair, chunk) partial

// A pivot of the LDL^T factorisation (no pivoting) of the normal matrix scaled to unit diagonal, D^-1/2 A D^-1/2, below this is
// "singular".  Why this value: pivot k of that matrix is 1 - (squared multiple correlation of parameter k with parameters 0..k-1),
// a number in [0, 1] whatever the units of the cloud, and every pivot is >= the smallest eigenvalue, so a system whose scaled
// condition number is below 1e10 is never refused (scanned surfaces measure 1e2 .. 1e3).  The sums carry a relative rounding error
// of about rows x 2^-53 (1e-11 at 1e5 rows): a pivot below 1e-10 is within a factor ten of that noise, and a solve through it
// would lose more than ten of fp64's sixteen digits.
constexpr double kIcpPlanePivotMin = 1e-10;

DSIR_HD inline int icp_plane_chunks(int J) { return J <= 0 ? 0 : (int)(((int64_t)J + kIcpPlaneChunk - 1) / kIcpPlaneChunk); }

// scratch the plane estimator needs beyond the point-to-point loop's parts (IcpLayout, icp_layout.h): partials [pairs][chunks][kIcpPlaneSlots] doubles, then the
// identity-update counters [pairs] doubles; both pieces padded to 256 bytes.  0 for shapes that are not positive.
inline size_t icp_plane_part_bytes(int pairs, int J) {
  if (pairs < 1 || J < 1) return 0;
  const size_t b = (size_t)pairs * (size_t)icp_plane_chunks(J) * kIcpPlaneSlots * sizeof(double);
  return (b + 255) & ~(size_t)255;
}
inline size_t icp_plane_extra_bytes(int pairs, int J) {
  if (pairs < 1 || J < 1) return 0;
  return icp_plane_part_bytes(pairs, J) + (((size_t)pairs * sizeof(double) + 255) & ~(size_t)255);
}

DSIR_HD inline int icp_plane_tri(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }   // r <= c: index into the 21 sums

// Solve A x = -b.  A: the 21 sums (upper triangle by rows), rows: the number of correspondences that entered them.
// Returns false - x = 0, the update is the identity - when rows < 6, a diagonal entry is not a positive finite number (a zero
// diagonal entry is singular), a pivot of the scaled matrix is below kIcpPlanePivotMin or not a number, or x is not finite.
DSIR_HD inline bool icp_plane_solve(const double* A, const double* b, double rows, double* x) {
  for (int i = 0; i < 6; ++i) x[i] = 0.0;
  if (!(rows >= 6.0)) return false;
  double s[6], L[6][6], D[6], y[6];
  for (int i = 0; i < 6; ++i) {
    const double d = A[icp_plane_tri(i, i)];
    if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) return false;
    s[i] = 1.0 / sqrt(d);
  }
  for (int j = 0; j < 6; ++j) {
    double d = 1.0;
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k] * D[k];
    if (!(d >= kIcpPlanePivotMin)) return false;
    D[j] = d;
    for (int i = j + 1; i < 6; ++i) {
      double v = A[icp_plane_tri(j, i)] * s[i] * s[j];
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k] * D[k];
      L[i][j] = v / d;
    }
  }
  for (int i = 0; i < 6; ++i) {            // L y = -(D^-1/2 b)
    double v = -b[i] * s[i];
    for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
    y[i] = v;
  }
  for (int i = 0; i < 6; ++i) y[i] /= D[i];
  for (int i = 5; i >= 0; --i) {           // L^T z = y, x = D^-1/2 z
    double v = y[i];
    for (int k = i + 1; k < 6; ++k) v -= L[k][i] * y[k];
    y[i] = v;
  }
  bool finite = true;
  for (int i = 0; i < 6; ++i) {
    y[i] *= s[i];
    finite = finite && (y[i] - y[i] == 0.0);
  }
  if (!finite) return false;
  for (int i = 0; i < 6; ++i) x[i] = y[i];
  return true;
}

// R = Rz(x2) Ry(x1) Rx(x0), t = (x3, x4, x5): open3d's TransformVector6dToMatrix4d, row-major 3 x 4
DSIR_HD inline void icp_plane_transform(const double* x, double* T) {
  const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
  T[0] = cg * cb; T[1] = cg * sb * sa - sg * ca; T[2] = cg * sb * ca + sg * sa; T[3] = x[3];
  T[4] = sg * cb; T[5] = sg * sb * sa + cg * ca; T[6] = sg * sb * ca - cg * sa; T[7] = x[4];
  T[8] = -sb;     T[9] = cb * sa;                T[10] = cb * ca;               T[11] = x[5];
}

}  // namespace dsir
