// Stand-alone host check of deepsir_amd/csrc/radius_nn.h (what csrc/radius_nn.hip decides on the host: the refusals it adds, the job
// table with its row prefix, the saturating sum of the row offsets, the scratch layout, the entry order) under AddressSanitizer + UndefinedBehaviorSanitizer: host code only,
// runs on the CPU, no GPU and no Python loader.
//   hipcc -x c++ -std=c++17 -O1 -g -fno-gpu-sanitize -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ideepsir_amd/csrc \
//         tools/radius_nn_check.cpp -o /tmp/radius_nn_check && /tmp/radius_nn_check
// (any host C++17 compiler with -fsanitize=address,undefined does as well; tests/test_radius_nn_host.py runs exactly this build.)
// Failures exit non-zero (no assert: the checks hold under NDEBUG too).
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "radius_nn.h"
using namespace dsir;

static long checks = 0;
#define CHECK(x) do { ++checks; if (!(x)) { std::fprintf(stderr, "radius_nn_check: %s failed (line %d)\n", #x, __LINE__); std::exit(1); } } while (0)

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static unsigned long long draw() {                          // xorshift64*: the same sequence on every run
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return rng_state * 0x2545f4914f6cdd1dull;
}

int main() {
  // ---- the refusals on top of dsir_t_nn_within_check
  CHECK(radius_nn_refusal(0, 0) == nullptr && radius_nn_refusal(1, 1) == nullptr && radius_nn_refusal(kRadiusMaxJobs, INT_MAX) == nullptr);
  CHECK(radius_nn_refusal(1, -1) != nullptr && radius_nn_refusal(1, INT_MIN) != nullptr);
  CHECK(radius_nn_refusal(-1, 0) != nullptr && radius_nn_refusal(kRadiusMaxJobs + 1, 0) != nullptr);
  CHECK(kRadiusCap == kRadiusWave * kRadiusOwn && kRadiusCap == 512);

  CHECK(radius_nn_rows_refusal(0) == nullptr && radius_nn_rows_refusal(kRadiusMaxRows) == nullptr && radius_nn_rows_refusal(-1) != nullptr);
  CHECK(radius_nn_rows_refusal(kRadiusMaxRows + 1) != nullptr && radius_nn_rows_refusal(0x7fffffffll) != nullptr);
  CHECK((kRadiusMaxRows + 1) * kRadiusWave == (1ll << 32) && kRadiusMaxRows * kRadiusWave < (1ll << 32));   // a launch stays below 2^32 threads

  // ---- the offsets' sum: exact while it fits an int32, else -1 for good - also where the true total passes 2^32 and an int32 sum
  // would wrap back to a non-negative number
  {
    const RadiusSatAdd add;
    CHECK(add(0, 0) == 0 && add(3, 4) == 7 && add(INT_MAX, 0) == INT_MAX && add(INT_MAX - 5, 5) == INT_MAX && add(0, INT_MAX) == INT_MAX);
    CHECK(add(INT_MAX, 1) == -1 && add(1, INT_MAX) == -1 && add(INT_MAX, INT_MAX) == -1 && add(0x40000000, 0x40000000) == -1);
    CHECK(add(-1, 0) == -1 && add(0, -1) == -1 && add(-1, -1) == -1 && add(-1, INT_MAX) == -1 && add(INT_MIN, 5) == -1);
    // a scan in any grouping: sequential, pairwise tree, and blocks of 7 joined afterwards, against the 64-bit truth
    for (int rep = 0; rep < 200; ++rep) {
      const int n = 1 + (int)(draw() % 300);
      const int32_t top = rep % 4 == 0 ? 1000 : (rep % 4 == 1 ? 0x02000000 : (rep % 4 == 2 ? 0x40000000 : INT_MAX));   // totals up to 300 * 2^31: far past 2^32
      std::vector<int32_t> c(n);
      for (int i = 0; i < n; ++i) c[i] = (int32_t)(draw() % ((uint64_t)top + 1));
      std::vector<int32_t> seq(n), blk(n);
      int64_t truth = 0;
      int32_t acc = 0;
      for (int i = 0; i < n; ++i) {
        truth += c[i];
        acc = i ? add(acc, c[i]) : c[i];
        seq[i] = acc;
        CHECK(acc == (truth > INT_MAX ? -1 : (int32_t)truth));
      }
      for (int b0 = 0; b0 < n; b0 += 7) {                      // blocks scanned alone, then the carry joined from the left
        int32_t carry = b0 ? blk[b0 - 1] : 0, local = 0;
        for (int i = b0; i < n && i < b0 + 7; ++i) { local = i == b0 ? c[i] : add(local, c[i]); blk[i] = b0 ? add(carry, local) : local; }
      }
      CHECK(std::memcmp(seq.data(), blk.data(), n * sizeof(int32_t)) == 0);
      {                                                        // pairwise reduction of the total, the odd tail carried down
        std::vector<int32_t> t(c);
        int m = n;
        while (m > 1) {
          int k = 0;
          for (int i = 0; i + 1 < m; i += 2) t[k++] = add(t[i], t[i + 1]);
          if (m & 1) t[k++] = t[m - 1];
          m = k;
        }
        CHECK(t[0] == seq[n - 1]);
      }
      // the fill's row test: a row is written only between two exact, ordered offsets
      for (int i = 0; i + 1 < n; ++i) CHECK(radius_row_ok(seq[i], seq[i + 1]) == (seq[i + 1] >= 0));
    }
    // the case of the plain sum's blind spot, spelled out: 4 rows of 2^30 entries total 2^32, which an int32 sum reads as 0
    const int32_t four[] = {0x40000000, 0x40000000, 0x40000000, 0x40000000};
    int32_t acc = four[0];
    uint32_t plain = (uint32_t)four[0];
    for (int i = 1; i < 4; ++i) { acc = add(acc, four[i]); plain += (uint32_t)four[i]; }
    CHECK(plain == 0u && acc == -1);
    CHECK(radius_row_ok(0, 0) && radius_row_ok(5, 9) && !radius_row_ok(-1, -1) && !radius_row_ok(7, -1) && !radius_row_ok(-1, 3) && !radius_row_ok(9, 5));
  }

  // ---- the table: jobs copied, row = the exclusive prefix of the jobs' query rows; exactly 3 n + 1 ints are written
  {
    const int64_t off[] = {0, 0, 1, 258, 1758};              // fragments of 0, 1, 257 and 1500 points
    const int32_t jobs[] = {3, 2, 0, 3, 1, 1, 2, 0, 3, 3, 0, 0};
    const int64_t n = 6;
    std::vector<int32_t> tab(radius_nn_table_ints(n));        // exact size: an overrun is the sanitizer's to find
    CHECK(tab.size() == 19);
    CHECK(radius_nn_table(off, 4, jobs, n, tab.data()) == 1500 + 0 + 1 + 257 + 1500 + 0);
    CHECK(std::memcmp(tab.data(), jobs, sizeof(jobs)) == 0);
    const int32_t want[] = {0, 1500, 1500, 1501, 1758, 3258, 3258};
    CHECK(std::memcmp(tab.data() + 2 * n, want, sizeof(want)) == 0);
    // the kernels' block -> job search (the last job with row[job] <= block) lands on the job that owns the row, past empty jobs
    const int32_t* row = tab.data() + 2 * n;
    for (int block = 0; block < 3258; ++block) {
      int lo = 0, hi = (int)n;
      while (hi - lo > 1) { const int mid = lo + ((hi - lo) >> 1); if (row[mid] <= block) lo = mid; else hi = mid; }
      CHECK(row[lo] <= block && block < row[lo + 1]);
    }
  }
  {
    std::vector<int32_t> tab(radius_nn_table_ints(0));        // no job: one int, rows 0
    const int64_t off[] = {0, 5};
    CHECK(tab.size() == 1 && radius_nn_table(off, 1, nullptr, 0, tab.data()) == 0 && tab[0] == 0);
  }
  {
    const int64_t off[] = {0, 5, 9};                          // a job index outside [0, F): refused, offsets never read outside
    const int32_t bad[][2] = {{2, 0}, {0, 2}, {-1, 0}, {0, -1}, {INT_MAX, 0}, {0, INT_MIN}};
    for (const auto& b : bad) {
      const int32_t jobs[] = {0, 1, b[0], b[1]};
      std::vector<int32_t> tab(radius_nn_table_ints(2));
      CHECK(radius_nn_table(off, 2, jobs, 2, tab.data()) == -1);
    }
  }
  {
    const int64_t off[] = {0, 0x40000000ll};                  // 2^30 rows a job: two fit in int32, three do not
    const int32_t jobs[] = {0, 0, 0, 0, 0, 0};
    std::vector<int32_t> tab(radius_nn_table_ints(3));
    CHECK(radius_nn_table(off, 1, jobs, 1, tab.data()) == 0x40000000ll);
    CHECK(radius_nn_table(off, 1, jobs, 2, tab.data()) == -1);                 // 2^31 > 2^31 - 1
    CHECK(radius_nn_table(off, 1, jobs, 3, tab.data()) == -1);
    const int64_t off2[] = {0, 0x3fffffffll, 0x40000000ll};
    const int32_t jobs2[] = {0, 0, 0, 0, 1, 0};
    CHECK(radius_nn_table(off2, 2, jobs2, 3, tab.data()) == 0x7fffffffll && tab[2 * 3 + 3] == INT_MAX);
  }
  long tables = 0;
  for (int rep = 0; rep < 300; ++rep) {                       // random lists: the prefix against a plain sum
    const int F = 1 + (int)(draw() % 7);
    std::vector<int64_t> off(F + 1, 0);
    for (int f = 0; f < F; ++f) off[f + 1] = off[f] + (int64_t)(draw() % 5 == 0 ? 0 : draw() % 3000);
    const int64_t n = (int64_t)(draw() % 40);
    std::vector<int32_t> jobs(2 * n + 1), tab(radius_nn_table_ints(n));
    for (int64_t j = 0; j < 2 * n; ++j) jobs[j] = (int32_t)(draw() % F);
    const int64_t rows = radius_nn_table(off.data(), F, jobs.data(), n, tab.data());
    int64_t sum = 0;
    for (int64_t j = 0; j < n; ++j) { CHECK(tab[2 * n + j] == sum); sum += off[jobs[2 * j] + 1] - off[jobs[2 * j]]; }
    CHECK(rows == sum && tab[2 * n + n] == sum);
    ++tables;
  }

  // ---- the scratch layout: the table, then the scan's temporary; on 256 bytes, large enough, not overlapping
  long shapes = 0;
  const int64_t ns[] = {0, 1, 2, 21, 22, 1000, 65536, kRadiusMaxJobs};
  const size_t tmps[] = {0, 1, 255, 256, 257, 777, (size_t)1 << 24};
  for (int64_t n : ns) for (size_t tmp : tmps) {
    const RadiusNNLayout l(n, tmp);
    const size_t need = radius_nn_table_ints(n) * 4;
    CHECK(l.tab == 0 && l.tmp % 256 == 0 && l.tmp >= need && l.tmp < need + 256 && l.tmp_bytes == tmp);
    CHECK(l.bytes % 256 == 0 && l.bytes >= l.tmp + (tmp < 256 ? 256 : tmp) && l.bytes < l.tmp + (tmp < 256 ? 256 : tmp) + 256);
    ++shapes;
  }
  CHECK(RadiusNNLayout(-5, 0).bytes == RadiusNNLayout(0, 0).bytes);

  // ---- the entry: (d2 bits, index) ordered lexicographically as one integer; never the "none" pattern for a finite d2
  CHECK(radius_entry(0u, 0u) == 0ull && radius_entry(1u, 0u) > radius_entry(0u, 0xffffffffu));
  CHECK(radius_entry(0x3f800000u, 7u) < radius_entry(0x3f800000u, 8u) && radius_entry(0x3f800000u, 7u) < radius_entry(0x3f800001u, 0u));
  CHECK(radius_entry(0x7f7fffffu, 0x3fffffffu) != ~0ull && (uint32_t)radius_entry(5u, 0x80000001u) == 0x80000001u);
  CHECK((uint32_t)(radius_entry(0x12345678u, 9u) >> 32) == 0x12345678u);
  std::printf("radius_nn: %ld checks passed, %ld tables built, %ld shapes laid out\n", checks, tables, shapes);
  return 0;
}
