// Stand-alone host check of deepsir_amd/csrc/fgr.h (the trial key of the FGR tuple test, the trial count, the bounds of the row list
// and the scratch layout of dsir_fgr_correspondence) under AddressSanitizer + UndefinedBehaviorSanitizer: host code only, runs on
// the CPU, no GPU and no Python loader involved.
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Ideepsir_amd/csrc tools/fgr_check.cpp -o /tmp/fgr_check && /tmp/fgr_check
// (any host C++17 compiler with -fsanitize=address,undefined does as well.  The sanitizer run is this manual command;
// tests/test_fgr_host.py builds the file as plain host C++, without a sanitizer, runs it and compares the rows it prints with the
// restatement's.)  Failures exit non-zero (no assert: the checks hold under NDEBUG too).
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fgr.h"
using namespace dsir;

static int checks = 0;
#define CHECK(x) do { ++checks; if (!(x)) { std::fprintf(stderr, "fgr_check: %s failed (line %d)\n", #x, __LINE__); std::exit(1); } } while (0)

int main() {
  // splitmix64: the published vectors of the generator seeded with 0 (state advances by the golden gamma)
  CHECK(fgr_mix64(0) == 0xE220A8397B1DCDAFull);
  CHECK(fgr_mix64(0x9E3779B97F4A7C15ull) == 0x6E789E6AA1B965F4ull);
  // rows stay below count for every count, extremes included; count <= 0 draws row 0 and is never evaluated
  const int counts[] = {1, 2, 3, 255, 256, 257, 5000, 1 << 20, INT_MAX};
  for (int count : counts)
    for (int t = 0; t < 2000; t += 7)
      for (int k = 0; k < 3; ++k) {
        const int r = fgr_trial_row(fgr_pair_key(0xDEADBEEFull, 5), t, k, count);
        CHECK(r >= 0 && r < count);
      }
  CHECK(fgr_trial_row(1, 0, 0, 0) == 0 && fgr_trial_row(1, 0, 0, -3) == 0);
  CHECK(fgr_pair_key(7, 0) == fgr_mix64(7) && fgr_pair_key(7, 3) == fgr_pair_key(7 ^ (3ull << 40), 0));
  // trials: 100 per live row under the cap, no overflow at the largest count
  CHECK(fgr_trials(0, 1000) == 0 && fgr_trials(-1, 1000) == 0 && fgr_trials(3, 1000) == 300 && fgr_trials(10, 1000) == 1000 &&
        fgr_trials(11, 1000) == 1000 && fgr_trials(INT_MAX, 1 << 22) == (1 << 22));
  CHECK(fgr_candidates(1, 5000, 1 << 20) == 500000 && fgr_candidates(0, 5000, 1 << 20) == 5000 && fgr_candidates(1, 1 << 20, 1 << 22) == (1 << 22));
  CHECK(fgr_blocks(0) == 0 && fgr_blocks(1) == 1 && fgr_blocks(256) == 1 && fgr_blocks(257) == 2 && fgr_blocks(INT_MAX) == (1 << 23));
  // the list: 3 rows a tuple up to the cap, or the M rows themselves
  CHECK(fgr_list_rows(1, 100, 1000) == 3000 && fgr_list_rows(0, 100, 1000) == 100 && fgr_list_rows(1, 1, 65536) == 196608);
  CHECK(fgr_n_rows(1, 100, 1000, 0) == 0 && fgr_n_rows(1, 100, 1000, 999) == 2997 && fgr_n_rows(1, 100, 1000, 1000) == 3000 &&
        fgr_n_rows(1, 100, 1000, 123456789012ll) == 3000 && fgr_n_rows(0, 100, 1000, 64) == 64 && fgr_n_rows(0, 100, 1000, 101) == 100);
  // the layout: parts in order, each on 256 bytes, none overlapping, the pose head first; every list position has its 6 doubles
  for (int tt = 0; tt < 2; ++tt)
    for (int P : {1, 4, 64})
      for (int M : {1, 3, 257, 20000}) {
        const FgrLayout l(P, M, tt, 1000, 1 << 20, 2, 777);
        const size_t L = (size_t)fgr_list_rows(tt, M, 1000), NB = (size_t)fgr_blocks(fgr_candidates(tt, M, 1 << 20));
        const size_t off[] = {l.pose.bytes, l.rows, l.blk_cnt, l.blk_pre, l.tmp, l.npts, l.hyp.T, l.hyp.valid, l.hyp.count, l.bytes};
        const size_t need[] = {0, (size_t)P * L * 4, (size_t)P * NB * 4, (size_t)P * NB * 4, 777, (size_t)P * L * 48, (size_t)P * 48, (size_t)P * 4,
                               (size_t)P * 4};
        CHECK(l.rows == l.pose.bytes);
        for (int i = 1; i < 9; ++i) CHECK(off[i] % 256 == 0 && off[i] + need[i] <= off[i + 1]);
        // walk the memory the way the kernels index it
        std::vector<unsigned char> buf(l.bytes);
        int32_t* rows = at<int32_t>(buf.data(), l.rows);
        double* npts = at<double>(buf.data(), l.npts);
        for (size_t p = 0; p < (size_t)P; p += (P > 1 ? P - 1 : 1)) {
          rows[p * L + L - 1] = -1;
          npts[(p * L + L - 1) * 6 + 5] = 1.0;
          at<int32_t>(buf.data(), l.blk_pre)[p * NB + NB - 1] = 1;
        }
        at<int32_t>(buf.data(), l.hyp.count)[P - 1] = 1;
      }
  // the solve the optimisation shares with the point-to-plane ICP refuses fewer than 6 rows: a list of one tuple moves nothing
  double A[21] = {}, b[6] = {}, x[6];
  for (int i = 0; i < 6; ++i) A[icp_plane_tri(i, i)] = 1.0;
  CHECK(!icp_plane_solve(A, b, 3.0, x) && icp_plane_solve(A, b, 6.0, x));
  std::printf("rows:");
  for (int t : {0, 1, 777})
    for (int k = 0; k < 3; ++k) std::printf(" %d", fgr_trial_row(fgr_pair_key(12345, 3), t, k, 1000));
  std::printf("\nfgr: %d checks passed\n", checks);
  return 0;
}
