// Stand-alone host check of deepsir_amd/csrc/ndt.h (the NDT lattice, the score constants, the argument checks, the scratch layout
// and the key-interval argument behind the x triple of ndt_accum_kernel) under AddressSanitizer + UndefinedBehaviorSanitizer: host
// code only, runs on the CPU, no GPU and no Python loader involved.
//   hipcc -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ideepsir_amd/csrc \
//         tools/ndt_check.cpp -o /tmp/ndt_check && /tmp/ndt_check
// (any host C++17 compiler with -fsanitize=address,undefined does as well.  The sanitizer run is this manual command;
// tests/test_ndt_host.py builds the file as plain host C++, without a sanitizer, and runs it.)
// Failures exit non-zero (no assert: the checks hold under NDEBUG too).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ndt.h"
using namespace dsir;

static int checks = 0;
#define CHECK(x) do { ++checks; if (!(x)) { std::fprintf(stderr, "ndt_check: %s failed (line %d)\n", #x, __LINE__); std::exit(1); } } while (0)

int main() {
  // ---- lattice: the edge is the resolution, without a margin, until the extent asks for more than 2^20 cells
  CHECK(ndt_cell_edge(0.3f, 10.0) == (double)0.3f);
  CHECK(ndt_cell_edge(0.3f, 0.0) == (double)0.3f);
  CHECK(ndt_cell_edge(1.0f, 1048576.0) == 1.0);
  CHECK(ndt_cell_edge(1.0f, 4194304.0) == 4.0);
  {
    const float lo[3] = {-1.f, 2.f, 0.5f}, hi[3] = {3.f, 2.5f, 4194304.5f};
    const CellLattice L = ndt_lattice(1.0f, lo, hi, true);
    CHECK(L.ox == -1.0 && L.oy == 2.0 && L.oz == 0.5 && L.h == 4.0);
    CHECK(cell_of(hi[2], L.oz, L.h) == 1048576 && cell_of(hi[2], L.oz, L.h) <= MAXC);    // the far point still has a key
    const CellLattice N = ndt_lattice(0.25f, lo, hi, false);                               // no finite row
    CHECK(N.ox == 0.0 && N.oy == 0.0 && N.oz == 0.0 && N.h == 0.25);
  }
  // ---- cell_of clamps a moved point far outside; such a coordinate is not in a key
  CHECK(cell_of(-1e30f, 0.0, 1.0) == -2 && cell_of(1e30f, 0.0, 1.0) == MAXC + 2);
  CHECK(!ndt_in_key(-1) && ndt_in_key(0) && ndt_in_key(MAXC) && !ndt_in_key(MAXC + 1));

  // ---- constants against the closed form at o = 0.55
  for (float res : {1.0f, 0.3f}) {
    const NdtConstants k = ndt_constants(0.55, res);
    const double r = (double)res, c1 = 4.5, c2 = 0.55 / (r * r * r);
    CHECK(std::fabs(k.d3 + std::log(c2)) < 1e-15);
    CHECK(std::fabs(k.d1 - (std::log(c2) - std::log(c1 + c2))) < 1e-14);
    // the defining property: d1 exp(-d2 / 2) + d3 = -log(c1 exp(-1/2) + c2), d1 + d3 = -log(c1 + c2)
    CHECK(std::fabs(k.d1 * std::exp(-k.d2 / 2.0) + k.d3 + std::log(c1 * std::exp(-0.5) + c2)) < 1e-13);
    CHECK(k.d1 < 0.0 && k.d2 > 0.0);
  }

  // ---- argument checks
  CHECK(ndt_args_ok(0.3f, 7, 1e-4f, 0.55f) && ndt_args_ok(2.f, 1, 1e-4f, 0.1f));
  CHECK(!ndt_args_ok(0.f, 7, 1e-4f, 0.55f) && !ndt_args_ok(-1.f, 7, 1e-4f, 0.55f) && !ndt_args_ok(NAN, 7, 1e-4f, 0.55f) &&
        !ndt_args_ok(INFINITY, 7, 1e-4f, 0.55f));
  CHECK(!ndt_args_ok(0.3f, 7, 0.f, 0.55f) && !ndt_args_ok(0.3f, 7, NAN, 0.55f) && !ndt_args_ok(0.3f, 7, INFINITY, 0.55f));
  CHECK(!ndt_args_ok(0.3f, 7, 1e-4f, 0.f) && !ndt_args_ok(0.3f, 7, 1e-4f, 1.f) && !ndt_args_ok(0.3f, 7, 1e-4f, NAN) &&
        !ndt_args_ok(0.3f, 7, 1e-4f, -0.5f));
  CHECK(!ndt_args_ok(0.3f, 0, 1e-4f, 0.55f) && !ndt_args_ok(0.3f, 27, 1e-4f, 0.55f));
  CHECK(ndt_shape_ok(1, 1, 1) && !ndt_shape_ok(0, 1, 1) && !ndt_shape_ok(1, 0, 1) && !ndt_shape_ok(1, 1, 0) && !ndt_shape_ok(4, 1 << 30, 8));

  // ---- layout: parts ascend, start on 256 bytes, do not overlap, and the size is a function of the shape alone
  for (int pairs : {1, 3, 7})
    for (int J : {0, 1, 37, 1024, 1025, 100000})
      for (int K : {1, 5, 300, 4096, 100000}) {
        const NdtLayout l(pairs, J, K, 12345), l2(pairs, J, K, 12345);
        const size_t off[] = {l.lat, l.enc, l.off_ref, l.keys, l.vals, l.runs, l.records, l.keys_raw, l.vals_raw, l.tmp, l.cur, l.Ta, l.Tb,
                              l.part, l.state, l.done, l.bytes};
        const size_t P = (size_t)pairs, nk = P * (size_t)K, nj = P * (size_t)J;
        const size_t need[] = {P * 32, P * 24, (P + 1) * 4, nk * 8, nk * 4, nk * 4, nk * 80, nk * 8, nk * 4, 12345, nj * 12, P * 48, P * 48,
                               P * (size_t)icp_plane_chunks(J) * kNdtSlots * 8, P * kNdtState * 8, 2 * P * 4};
        for (int i = 0; i < 16; ++i) {
          CHECK(off[i] % 256 == 0);
          CHECK(off[i] + need[i] <= off[i + 1]);
        }
        CHECK(l.bytes == l2.bytes && l.tmp_bytes == 12345);
      }
  CHECK(icp_plane_chunks(1024) == 1 && icp_plane_chunks(1025) == 2 && icp_plane_chunks(0) == 0);
  CHECK(kNdtSums <= kNdtSlots && kNdtBad == kNdtSums - 1 && kNdtChunk == 1024);

  // ---- the x triple is one key interval: among sorted keys of random cells, those in [key(x0, y, z), key(x1, y, z)] are exactly the
  // cells x0 .. x1 of that (y, z), ascending in x
  {
    std::vector<uint64_t> keys;
    uint64_t s = 12345;
    auto rnd = [&](int n) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (int)((s >> 33) % (uint64_t)n); };
    const int edge[] = {0, 1, 2, MAXC - 2, MAXC - 1, MAXC};
    for (int i = 0; i < 4000; ++i) keys.push_back(cell_key(edge[rnd(6)], edge[rnd(6)], edge[rnd(6)]));
    for (int i = 0; i < 4000; ++i) keys.push_back(cell_key(rnd(5), rnd(5), rnd(5)));
    keys.push_back(KEY_NONE);
    std::sort(keys.begin(), keys.end());
    for (int t = 0; t < 2000; ++t) {
      const int cx = t % 2 ? edge[rnd(6)] : rnd(5), cy = t % 3 ? rnd(5) : edge[rnd(6)], cz = t % 5 ? rnd(5) : edge[rnd(6)];
      const int x0 = std::max(cx - 1, 0), x1 = std::min(cx + 1, MAXC);
      const uint64_t klo = cell_key(x0, cy, cz), khi = cell_key(x1, cy, cz);
      CHECK(klo <= khi && khi < KEY_NONE);
      size_t in = 0, want = 0;
      for (uint64_t k : keys) {
        const int x = (int)(k & MAXC), y = (int)((k >> 21) & MAXC), z = (int)((k >> 42) & MAXC);
        const bool cell = k != KEY_NONE && y == cy && z == cz && x >= x0 && x <= x1;
        want += cell;
        if (k >= klo && k <= khi) { ++in; CHECK(cell); }
      }
      CHECK(in == want);
    }
  }
  std::printf("ndt: %d checks passed\n", checks);
  return 0;
}
