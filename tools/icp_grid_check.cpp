// Stand-alone host check of deepsir_amd/csrc/icp_grid.h, csrc/icp_layout.h and csrc/cell_index.h (the per-pair lattice rule of the
// cell-indexed ICP search, the cell coordinate and key, and the scratch layouts: IcpGridLayout that icp_grid_build takes its offsets
// from, IcpLayout / IcpCorrLayout of the ICP loop and the search step, IndexLayout of overlap.hip) under AddressSanitizer +
// UndefinedBehaviorSanitizer: host code only, runs on the CPU, no GPU and no Python loader.
//   hipcc -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ideepsir_amd/csrc \
//         tools/icp_grid_check.cpp -o /tmp/icp_grid_check && /tmp/icp_grid_check
// (any host C++17 compiler with -fsanitize=address,undefined does as well.  The sanitizer run is this manual command;
// tests/test_icp_search_host.py builds the file as plain host C++, without a sanitizer, and runs it.)
// Failures exit non-zero (no assert: the checks hold under NDEBUG too).
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "icp_grid.h"
#include "icp_layout.h"
using namespace dsir;

static long checks = 0;
#define CHECK(x) do { ++checks; if (!(x)) { std::fprintf(stderr, "icp_grid_check: %s failed (line %d)\n", #x, __LINE__); std::exit(1); } } while (0)

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static double uniform() {                                   // xorshift64*: the same sequence on every run
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (double)((rng_state * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
}

// the rule's d2 in fp32, every operation rounded on its own (volatile keeps a host compiler from contracting)
static float d2_rule(const float* a, const float* b) {
  volatile float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
  volatile float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  volatile float s = xx + yy;
  return s + zz;
}

// parts at[0 .. n - 1] with at[n] = the total: in order, on 256 bytes, each as large as need[k], less than 256 bytes of padding, so
// none overlaps and the total is the sum of the padded parts
static void check_parts(const size_t* at, const size_t* need, int n) {
  CHECK(at[0] == 0);
  size_t sum = 0;
  for (int k = 0; k < n; ++k) {
    CHECK(at[k] % 256 == 0 && at[k + 1] >= at[k] + need[k] && at[k + 1] < at[k] + need[k] + 256);
    sum += (need[k] + 255) / 256 * 256;
  }
  CHECK(at[n] == sum);
}

// n points in a box, every accepted pair (d2 <= fl(r r)) must be in adjacent cells; returns the accepted pairs seen
static long containment(float r, const std::vector<float>& pts) {
  const size_t n = pts.size() / 3;
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (size_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) { lo[a] = std::fmin(lo[a], pts[3 * i + a]); hi[a] = std::fmax(hi[a], pts[3 * i + a]); }
  const IcpLattice L = icp_grid_lattice(r, lo, hi, n > 0);
  const double o[3] = {L.ox, L.oy, L.oz};
  volatile float r2v = r * r;
  const float r2 = r2v;
  long hits = 0;
  for (size_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      const int c = cell_of(pts[3 * i + a], o[a], L.h);
      CHECK(c >= 0 && c <= (1 << 20));                                  // a reference cell and its neighbour fit 21 bits
    }
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j) {
      if (!(d2_rule(&pts[3 * i], &pts[3 * j]) <= r2)) continue;
      ++hits;
      for (int a = 0; a < 3; ++a) CHECK(std::abs(cell_of(pts[3 * i + a], o[a], L.h) - cell_of(pts[3 * j + a], o[a], L.h)) <= 1);
    }
  return hits;
}

int main() {
  // ---- the cell edge
  CHECK(icp_grid_cell_edge(0.2f, 0.0) == (double)0.2f * (1.0 + 1.0 / 1024.0));
  CHECK(icp_grid_cell_edge(0.2f, 100.0) == (double)0.2f * kIcpGridMargin);           // 500 cells: the radius term
  CHECK(icp_grid_cell_edge(1e-4f, 1000.0) == 1000.0 / 1048576.0);                    // 10^7 radii wide: the coarse term
  CHECK(icp_grid_cell_edge(1e-30f, 0.0) == kIcpGridMinEdge && icp_grid_cell_edge(0.f, 0.0) == kIcpGridMinEdge);
  CHECK(icp_grid_cell_edge(1e-30f, 6.8e38) == 6.8e38 / 1048576.0);
  CHECK(icp_grid_cell_edge(FLT_MAX, 0.0) > (double)FLT_MAX);                         // fp64: no overflow
  for (int k = 0; k < 2000; ++k) {
    const float r = (float)std::pow(10.0, -8.0 + 12.0 * uniform());
    const double ext = std::pow(10.0, -6.0 + 14.0 * uniform());
    const double h = icp_grid_cell_edge(r, ext);
    CHECK(h >= (double)r * kIcpGridMargin && h >= kIcpGridMinEdge && std::floor(ext / h) <= kIcpGridMaxCells);
  }
  // ---- the radius and the shapes the grid takes
  CHECK(icp_grid_radius_ok(0.2f) && icp_grid_radius_ok(1e-30f) && icp_grid_radius_ok(1.8e19f));
  CHECK(!icp_grid_radius_ok(1.9e19f) && !icp_grid_radius_ok(INFINITY) && !icp_grid_radius_ok(NAN) && !icp_grid_radius_ok(0.f) &&
        !icp_grid_radius_ok(-1.f));
  CHECK(icp_grid_shape_ok(1, 1, 1) && icp_grid_shape_ok(8, 5000, 5000) && icp_grid_shape_ok(1, INT_MAX, INT_MAX));
  CHECK(!icp_grid_shape_ok(0, 1, 1) && !icp_grid_shape_ok(1, 0, 1) && !icp_grid_shape_ok(1, 1, 0) && !icp_grid_shape_ok(2, INT_MAX, 1) &&
        !icp_grid_shape_ok(INT_MAX, 1, INT_MAX) && !icp_grid_shape_ok(-1, -1, -1));
  // ---- the lattice of a pair: origin = the minimum, the edge from the longest axis; no finite point: origin 0
  {
    const float lo[3] = {-1.f, 2.f, 1e5f}, hi[3] = {3.f, 2.f, 1e5f + 1.f};
    IcpLattice L = icp_grid_lattice(0.5f, lo, hi, true);
    CHECK(L.ox == -1.0 && L.oy == 2.0 && L.oz == 1e5 && L.h == 0.5 * kIcpGridMargin);
    L = icp_grid_lattice(1e-6f, lo, hi, true);
    CHECK(L.h == 4.0 / 1048576.0);
    L = icp_grid_lattice(0.5f, lo, hi, false);
    CHECK(L.ox == 0.0 && L.oy == 0.0 && L.oz == 0.0 && L.h == 0.5 * kIcpGridMargin);
  }
  // ---- cell_of clamps; the key keeps 21 bits per axis and stays below KEY_NONE
  CHECK(cell_of(0.f, 0.0, 1.0) == 0 && cell_of(0.999f, 0.0, 1.0) == 0 && cell_of(1.f, 0.0, 1.0) == 1 && cell_of(-0.5f, 0.0, 1.0) == -1);
  CHECK(cell_of(-1e30f, 0.0, 1.0) == -2 && cell_of(1e30f, 0.0, 1.0) == MAXC + 2 && cell_of(FLT_MAX, -(double)FLT_MAX, 0x1p-60) == MAXC + 2);
  CHECK(cell_key(1, 2, 3) == (1ull | (2ull << 21) | (3ull << 42)) && cell_key(MAXC, MAXC, MAXC) == 0x7fffffffffffffffull);
  CHECK(cell_key(MAXC, MAXC, MAXC) < KEY_NONE && cell_key(0, 1, 0) > cell_key(MAXC, 0, 0) && cell_key(0, 0, 1) > cell_key(MAXC, MAXC, 0));
  // ---- containment under `<=`: random clouds, points on cell faces and at exactly r, a coarse-edge cloud, coordinates near 1e5
  long hits = 0;
  {
    std::vector<float> p;
    for (int i = 0; i < 600; ++i) for (int a = 0; a < 3; ++a) p.push_back((float)(uniform() * 1.5));
    hits += containment(0.1f, p);
    for (float& v : p) v += 1e5f;
    hits += containment(0.1f, p);
  }
  {
    std::vector<float> p;                                   // a lattice of step r / 2 from the origin: faces, and pairs at exactly r
    for (int i = 0; i < 9; ++i) for (int j = 0; j < 9; ++j) for (int k = 0; k < 5; ++k) { p.push_back(0.25f * i); p.push_back(0.25f * j); p.push_back(0.25f * k); }
    hits += containment(0.5f, p);
    std::vector<float> q;                                   // the same on multiples of the cell edge itself, rounded to fp32
    const double h = 0.5 * kIcpGridMargin;
    for (int i = 0; i < 9; ++i) for (int j = 0; j < 9; ++j) for (int k = 0; k < 3; ++k) { q.push_back((float)(h * i)); q.push_back((float)(h * j * 0.5)); q.push_back((float)(h * k)); }
    hits += containment(0.5f, q);
  }
  {
    std::vector<float> p;                                   // clusters of width ~r spread over 10^8 radii: the coarse edge
    for (int c = 0; c < 6; ++c) {
      const float base[3] = {(float)(uniform() * 1000.0), (float)(uniform() * 1000.0), (float)(uniform() * 10.0)};
      for (int i = 0; i < 60; ++i) for (int a = 0; a < 3; ++a) p.push_back(base[a] + (float)(uniform() * 3e-5));
    }
    p[0] = 0.f; p[1] = 0.f; p[2] = 0.f; p[3] = 1000.f; p[4] = 1000.f; p[5] = 10.f;
    hits += containment(1e-5f, p);
  }
  CHECK(hits > 5000);
  // ---- the scratch layout: parts in order, on 256 bytes, large enough, none overlapping, the total the sum
  long shapes = 0;
  const int ps[] = {1, 3, 8, 65535}, ns[] = {1, 63, 65, 1000, 4096, 100000};
  const size_t tmps[] = {0, 1, 256, 777, (size_t)1 << 24};
  for (int P : ps) for (int J : ns) for (int K : ns) for (size_t tmp : tmps) {
    if (!icp_grid_shape_ok(P, J, K)) continue;
    ++shapes;
    const IcpGridLayout l(P, J, K, tmp);
    const size_t nj = (size_t)P * J, nk = (size_t)P * K, nm = nj > nk ? nj : nk;
    const size_t at[] = {l.lat, l.enc, l.off_ref, l.off_qry, l.keys, l.sorted, l.perm, l.keys_raw, l.vals_raw, l.vals, l.keys_qry, l.tmp, l.bytes};
    const size_t need[] = {(size_t)P * 32, (size_t)P * 24, (size_t)(P + 1) * 4, (size_t)(P + 1) * 4, nk * 8, nk * 16, nj * 4, nm * 8, nm * 4,
                           nk * 4, nj * 8, tmp < 256 ? 256 : tmp};
    CHECK(sizeof(IcpLattice) == 32 && sizeof(CellLattice) == 32 && l.tmp_bytes == tmp);
    check_parts(at, need, 12);
    // ---- the loop's scratch for estimator 0 / 1 and search 0 / 1: the parts, and the total against the formulas the loop grew by -
    // the point-to-point loop's sum, plus icp_plane_extra_bytes, plus the grid's piece
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    for (int estimator = 0; estimator < 2; ++estimator) for (int search = 0; search < 2; ++search) {
      const size_t grid = search ? l.bytes : 0, n = nj;
      const IcpLayout i(P, J, estimator == 1, grid);
      const size_t iat[] = {i.cur, i.idx, i.d2, i.w, i.Ta, i.Tb, i.state, i.skip, i.Tstep, i.part, i.nsing, i.grid, i.bytes};
      const size_t ineed[] = {n * 12, n * 4, n * 4, n * 4, (size_t)P * 48, (size_t)P * 48, (size_t)P * 32, (size_t)P * 4, (size_t)P * 48,
                              estimator ? (size_t)P * icp_plane_chunks(J) * kIcpPlaneSlots * 8 : 0, estimator ? (size_t)P * 8 : 0, grid};
      check_parts(iat, ineed, 12);
      const size_t point = al((size_t)P * J * 12) + 3 * al((size_t)P * J * 4) + 2 * al((size_t)P * 48) + al((size_t)P * 32) +
                           al((size_t)P * 4) + al((size_t)P * 48);
      CHECK(i.bytes == point + (estimator == 1 ? icp_plane_extra_bytes(P, J) : 0) + grid);
      const IcpCorrLayout c(P, J, grid);
      CHECK(c.cur == 0 && c.grid == al((size_t)P * J * 12) && c.bytes == al((size_t)P * J * 12) + grid);
    }
  }
  // ---- overlap.hip's index over the same table (total points, fragments)
  for (int F : ps) for (int n : ns) for (size_t tmp : tmps) {
    const int64_t total = (int64_t)n - 1;                          // 0 included: laid out as one point
    const IndexLayout l(total, F, tmp);
    const size_t m = (size_t)(total < 1 ? 1 : total);
    const size_t at[] = {l.keys, l.sorted, l.box, l.off, l.keys_raw, l.vals_raw, l.vals, l.tmp, l.bytes};
    const size_t need[] = {m * 8, m * 16, (size_t)F * 24, (size_t)(F + 1) * 4, m * 8, m * 4, m * 4, tmp < 256 ? 256 : tmp};
    CHECK(l.tmp_bytes == tmp);
    check_parts(at, need, 8);
    ++shapes;
  }
  // ---- Carve and point_key
  {
    Carve c;
    CHECK(c.take(0) == 0 && c.p == 0 && c.take(1) == 0 && c.p == 256 && c.take(256) == 256 && c.take(257) == 512 && c.p == 1024);
    const CellLattice L{0.0, 0.0, 0.0, 1.0};
    CHECK(point_key(1.5f, 2.5f, 3.5f, L) == cell_key(1, 2, 3) && point_key(-5.f, 0.f, 1e30f, L) == cell_key(0, 0, MAXC));
    CHECK(point_key(NAN, 0.f, 0.f, L) == KEY_NONE && point_key(0.f, INFINITY, 0.f, L) == KEY_NONE && point_key(0.f, 0.f, -INFINITY, L) == KEY_NONE);
  }
  std::printf("icp_grid: %ld checks passed, %ld shapes laid out, %ld accepted pairs contained\n", checks, shapes, hits);
  return 0;
}
