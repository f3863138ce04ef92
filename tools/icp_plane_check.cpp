// Stand-alone host check of deepsir_amd/csrc/icp_plane.h (the 6 x 6 LDL^T solve of the point-to-plane ICP update, its singularity
// test, the Euler composition and the scratch-size arithmetic of dsir_icp_refine_ex) under AddressSanitizer +
// UndefinedBehaviorSanitizer: host code only, runs on the CPU, no GPU and no Python loader involved.
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Ideepsir_amd/csrc tools/icp_plane_check.cpp -o /tmp/icp_plane_check && /tmp/icp_plane_check
// (any host C++17 compiler with -fsanitize=address,undefined does as well.  The sanitizer run is this manual command;
// tests/test_icp_plane.py builds the file as plain host C++, without a sanitizer, and runs it.)
// Failures exit non-zero (no assert: the checks hold under NDEBUG too).
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "icp_plane.h"
using namespace dsir;

static int checks = 0;
#define CHECK(x) do { ++checks; if (!(x)) { std::fprintf(stderr, "icp_plane_check: %s failed (line %d)\n", #x, __LINE__); std::exit(1); } } while (0)

// A = sum J J^T (packed), b = -A x_true from rows J_k = f(k): a system with a known answer
static void make_system(int rows, const double* x_true, double* A, double* b, bool flat) {
  double M[6][6] = {};
  for (int k = 0; k < rows; ++k) {
    double J[6];
    for (int i = 0; i < 6; ++i) J[i] = std::sin(1.0 + 0.7 * k * (i + 1)) + (i == k % 6 ? 0.5 : 0.0);
    if (flat) J[2] = J[3] = J[4] = 0.0;          // a planar target with normals (0,0,1): rows [sy, -sx, 0, 0, 0, 1]
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) M[r][c] += J[r] * J[c];
  }
  for (int r = 0; r < 6; ++r) {
    double v = 0.0;
    for (int c = 0; c < 6; ++c) v += M[r][c] * x_true[c];
    b[r] = -v;
    for (int c = r; c < 6; ++c) A[icp_plane_tri(r, c)] = M[r][c];
  }
}

int main() {
  // the packed index covers 0..20 once, row by row
  int at = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) CHECK(icp_plane_tri(r, c) == at++);
  CHECK(at == 21 && kIcpPlaneSums == 21 + 6 + 2 && kIcpPlaneSlots >= kIcpPlaneSums);

  const double x_true[6] = {0.01, -0.02, 0.03, 0.1, -0.2, 0.05};
  double A[21], b[6], x[6];
  make_system(40, x_true, A, b, false);
  CHECK(icp_plane_solve(A, b, 40.0, x));
  for (int i = 0; i < 6; ++i) CHECK(std::fabs(x[i] - x_true[i]) < 1e-12);
  // the answer does not depend on the units of the parameters: the matrix is scaled to unit diagonal first
  {
    double As[21], bs[6], xs[6];
    const double u[6] = {1e3, 1e3, 1e3, 1e-3, 1e-3, 1e-3};
    for (int r = 0; r < 6; ++r) {
      bs[r] = b[r] * u[r];
      for (int c = r; c < 6; ++c) As[icp_plane_tri(r, c)] = A[icp_plane_tri(r, c)] * u[r] * u[c];
    }
    CHECK(icp_plane_solve(As, bs, 40.0, xs));
    for (int i = 0; i < 6; ++i) CHECK(std::fabs(xs[i] * u[i] - x_true[i]) < 1e-11);
  }
  // fewer than 6 rows, and a count that is not a number
  CHECK(!icp_plane_solve(A, b, 5.0, x));
  for (int i = 0; i < 6; ++i) CHECK(x[i] == 0.0);
  CHECK(!icp_plane_solve(A, b, std::nan(""), x));
  // a zero diagonal entry (planar target) is singular
  make_system(40, x_true, A, b, true);
  CHECK(A[icp_plane_tri(2, 2)] == 0.0 && !icp_plane_solve(A, b, 40.0, x));
  for (int i = 0; i < 6; ++i) CHECK(x[i] == 0.0);
  // rank 5 without a zero on the diagonal: column 5 = column 4 (a pivot of 0 up to rounding)
  make_system(40, x_true, A, b, false);
  for (int r = 0; r < 5; ++r) A[icp_plane_tri(r, 5)] = A[icp_plane_tri(r, 4)];
  A[icp_plane_tri(5, 5)] = A[icp_plane_tri(4, 4)];
  A[icp_plane_tri(4, 5)] = A[icp_plane_tri(4, 4)];
  CHECK(!icp_plane_solve(A, b, 40.0, x));
  // 6 rows that are the same row: rank 1
  make_system(1, x_true, A, b, false);
  CHECK(!icp_plane_solve(A, b, 6.0, x));
  // values that are not finite
  make_system(40, x_true, A, b, false);
  A[icp_plane_tri(1, 1)] = INFINITY;
  CHECK(!icp_plane_solve(A, b, 40.0, x));
  make_system(40, x_true, A, b, false);
  A[icp_plane_tri(0, 3)] = std::nan("");
  CHECK(!icp_plane_solve(A, b, 40.0, x));
  make_system(40, x_true, A, b, false);
  b[2] = std::nan("");
  CHECK(!icp_plane_solve(A, b, 40.0, x));
  for (int i = 0; i < 6; ++i) CHECK(x[i] == 0.0);
  A[icp_plane_tri(3, 3)] = -1.0; b[2] = 0.0;
  CHECK(!icp_plane_solve(A, b, 40.0, x));

  // the Euler composition: a rotation (R R^T = I, det 1), Rz Ry Rx in that order, the translation copied
  double T[12];
  icp_plane_transform(x_true, T);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double v = 0.0;
      for (int k = 0; k < 3; ++k) v += T[r * 4 + k] * T[c * 4 + k];
      CHECK(std::fabs(v - (r == c ? 1.0 : 0.0)) < 1e-15);
    }
  CHECK(T[3] == x_true[3] && T[7] == x_true[4] && T[11] == x_true[5]);
  const double only_x[6] = {0.3, 0, 0, 0, 0, 0}, only_z[6] = {0, 0, 0.3, 0, 0, 0};
  icp_plane_transform(only_x, T);
  CHECK(T[0] == 1.0 && T[5] == std::cos(0.3) && T[6] == -std::sin(0.3) && T[9] == std::sin(0.3));
  icp_plane_transform(only_z, T);
  CHECK(T[10] == 1.0 && T[0] == std::cos(0.3) && T[1] == -std::sin(0.3) && T[4] == std::sin(0.3));
  const double zero[6] = {0, 0, 0, 0, 0, 0};
  icp_plane_transform(zero, T);
  for (int k = 0; k < 12; ++k) CHECK(T[k] == (k % 5 == 0 ? 1.0 : 0.0));

  // the partition and the scratch sizes at every extreme
  const int js[] = {INT_MIN, -1, 0, 1, 37, 1023, 1024, 1025, 2500, 20000, 100000, INT_MAX};
  const int ps[] = {INT_MIN, -1, 0, 1, 3, 8, 65535, INT_MAX};
  long ok = 0;
  for (int J : js) for (int P : ps) {
    const size_t part = icp_plane_part_bytes(P, J), extra = icp_plane_extra_bytes(P, J);
    if (P < 1 || J < 1) { CHECK(part == 0 && extra == 0 && (J >= 1 || icp_plane_chunks(J) == 0)); continue; }
    ++ok;
    const size_t nch = (size_t)icp_plane_chunks(J);
    CHECK(nch == ((size_t)J + 1023) / 1024 && nch * 1024 >= (size_t)J && (nch - 1) * 1024 < (size_t)J);
    CHECK(part % 256 == 0 && part >= (size_t)P * nch * 256 && part < (size_t)P * nch * 256 + 256);
    CHECK(extra % 256 == 0 && extra >= part + (size_t)P * 8 && extra < part + (size_t)P * 8 + 256);
  }
  CHECK(icp_plane_chunks(INT_MAX) == 2097152);
  std::printf("icp_plane: %d checks passed, %ld shapes accepted\n", checks, ok);
  return 0;
}
