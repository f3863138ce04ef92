// Stand-alone host check of deepsir_amd/csrc/train_layouts.h: the row split of the weight-gradient GEMM (dw_plan), the GroupNorm row
// chunks, and the scratch layouts of train_gemm.hip, train_norm.hip and train_loss.hip.  Every layout, at edge shapes: the parts start
// on 256 bytes, lie in declaration order, do not overlap and end inside `bytes`; each part's need is spelled out below, term by term,
// from what the kernels index, not copied from the layout.
// Host code only, runs on the CPU, no GPU and no Python loader.
//   hipcc -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ideepsir_amd/csrc \
//         tools/train_layout_check.cpp -o /tmp/train_layout_check && /tmp/train_layout_check
// (any host C++17 compiler does as well.  The sanitizer run is this manual command; tests/test_cabi.py::test_host_only_plan_checks
// builds the file as plain host C++, without a sanitizer, and runs it.)  Failures exit non-zero (no assert: the checks hold under NDEBUG too).
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>
#include "train_layouts.h"
using namespace dsir;

static long checks = 0;
#define CHECK(x) do { ++checks; if (!(x)) { std::fprintf(stderr, "train_layout_check: %s failed (line %d)\n", #x, __LINE__); std::exit(1); } } while (0)

// parts at[k] of need[k] bytes each, in declaration order, the first at 0; the piece is `bytes` long
static void check_parts(const std::vector<size_t>& at, const std::vector<size_t>& need, size_t bytes) {
  CHECK(at.size() == need.size() && at[0] == 0);
  for (size_t k = 0; k < at.size(); ++k) {
    CHECK(at[k] % 256 == 0);
    const size_t end = at[k] + need[k];
    CHECK(end >= at[k]);                                               // no wrap
    CHECK(end <= (k + 1 < at.size() ? at[k + 1] : bytes));             // in order, no overlap, the last one inside the piece
  }
  CHECK(bytes % 256 == 0);
}

int main() {
  long shapes = 0;

  // ---- dw_plan and DwLayout.  t_gemm_dw_kernel: block z writes partial[z][n][k], n < N, k < Kp, for the rows
  // [z rows_per_split, min(rows, (z + 1) rows_per_split)) in chunks of TK; t_gemm_dw_reduce_kernel reads partial[i][n][k], i < splits
  std::vector<std::pair<int64_t, std::pair<int, int>>> dw = {
      {319488, {128, 128}}, {200000, {128, 128}}, {1000000, {256, 256}}, {80000, {8, 10}}, {5000, {64, 64}}, {1, {1, 1}},
      {294912, {64, 64}}, {640000, {128, 64}}};
  for (int64_t rows : {1, 15, 16, 17, 127, 128, 129})
    for (auto nk : {std::pair<int, int>{1, 1}, {64, 63}, {64, 64}, {65, 64}}) dw.push_back({rows, nk});
  for (const auto& s : dw) {
    const int64_t rows = s.first;
    const int N = s.second.first, K = s.second.second;
    ++shapes;
    size_t need = 0;
    for (bool bias : {false, true}) {
      const DwPlan p = dw_plan(rows, N, K, bias);
      CHECK(p.Kp == K + (bias ? 1 : 0));
      CHECK(p.splits >= 1 && p.splits <= 1024);
      CHECK(p.rows_per_split >= TK && p.rows_per_split % TK == 0);
      CHECK((int64_t)p.splits * p.rows_per_split >= rows);             // every row belongs to a split
      CHECK((int64_t)(p.splits - 1) * p.rows_per_split < rows);        // and no split is empty
      const size_t n = (size_t)p.splits * (size_t)N * (size_t)p.Kp * sizeof(float);
      need = n > need ? n : need;
    }
    const DwLayout L(rows, N, K);
    check_parts({L.partial}, {need}, L.bytes);
    CHECK(L.bytes < need + 256);
  }
  {
    // K = 64: the bias column is a tile column of its own (Kp = 65), K = 63 keeps both plans on one tile column
    CHECK((dw_plan(129, 64, 64, true).Kp + TB - 1) / TB == 2 && (dw_plan(129, 64, 64, false).Kp + TB - 1) / TB == 1);
    CHECK((dw_plan(129, 64, 63, true).Kp + TB - 1) / TB == 1 && (dw_plan(129, 64, 63, false).Kp + TB - 1) / TB == 1);
    const DwPlan qb = dw_plan(319488, 128, 128, true), qn = dw_plan(319488, 128, 128, false);
    CHECK(qb.splits < qn.splits);                                      // the plan without the column needs MORE partial matrices
    CHECK(DwLayout(319488, 128, 128).bytes >= (size_t)qn.splits * 128 * 128 * 4 && DwLayout(319488, 128, 128).bytes >= (size_t)qb.splits * 128 * 129 * 4);
  }

  // ---- GroupNorm.  Forward: t_gn_stats_kernel writes partial[((cloud groups + g) chunks + chunk) 2 + {0, 1}] doubles.  Backward:
  // t_gn_bwd_sums_kernel writes partial[((cloud chunks + chunk) C + c) 2 + {0, 1}] floats, the final stage sums[(cloud C + c) 2 + {0, 1}]
  for (int M : {1, 127, 128, 129, 128 * 256, 128 * 256 + 1})
    for (auto cg : {std::pair<int, int>{4, 4}, {6, 2}, {12, 3}, {256, 8}})
      for (int clouds : {1, 2, 7}) {
        const int C = cg.first, groups = cg.second;
        ++shapes;
        const int chunks = gn_chunks(M), rpc = (M + chunks - 1) / chunks;     // the launchers' rows per chunk
        CHECK(chunks >= 1 && chunks <= 256 && chunks == ((M + 127) / 128 < 256 ? (M + 127) / 128 : 256));
        CHECK((int64_t)chunks * rpc >= M);                                 // every row belongs to a chunk (a trailing chunk may be empty)
        const GnFwdLayout f(clouds, M, C, groups);
        check_parts({f.partial}, {(size_t)clouds * groups * chunks * 2 * sizeof(double)}, f.bytes);
        const GnBwdLayout b(clouds, M, C);
        check_parts({b.partial, b.sums}, {(size_t)clouds * chunks * C * 2 * sizeof(float), (size_t)clouds * C * 2 * sizeof(float)}, b.bytes);
        // the one size function covers both calls, whatever `groups` (<= C) the forward runs with, and stays within the count before the
        // layouts - (clouds chunks C 2 + clouds C 2) doubles - plus 256 bytes per part
        const size_t got = gn_scratch_bytes(clouds, M, C);
        CHECK(got >= f.bytes && got >= b.bytes && got >= GnFwdLayout(clouds, M, C, C).bytes && got >= GnFwdLayout(clouds, M, C, 1).bytes);
        CHECK(got <= ((size_t)clouds * chunks * C * 2 + (size_t)clouds * C * 2) * sizeof(double) + 2 * 256);
      }

  // ---- detection loss.  Five [P][M][M] float matrices; lse_col, rowsum, colsum [P][M] floats; coef [P][M][3] floats (t_circle_final_kernel
  // writes coef[pi 3 + {0, 1, 2}]); rows [P][M] CircleRow of 5 floats + 3 ints
  for (auto pmv : {std::pair<int, int>{1, 1}, {1, 3}, {2, 5}, {3, 64}, {8, 512}}) {
    const int P = pmv.first, M = pmv.second;
    ++shapes;
    const size_t mm = (size_t)P * M * M * 4, pm = (size_t)P * M * 4, row = 5 * sizeof(float) + 3 * sizeof(int);
    CHECK(row == kCircleRowBytes);
    const DetDesLayout L(P, M);
    check_parts({L.dot, L.dist_pc, L.dist_feat, L.Wn, L.Wnt, L.lse_col, L.coef, L.rowsum, L.colsum, L.rows},
                {mm, mm, mm, mm, mm, pm, 3 * pm, pm, pm, (size_t)P * M * row}, L.bytes);
    CHECK(L.rows % 8 == 0);                                            // (1, 3): 99 floats lie ahead of `rows`
    const size_t before = (5 * (size_t)P * M * M + 16 * (size_t)P * M) * sizeof(float) + (size_t)P * M * row + 256;
    CHECK(L.bytes <= before + 10 * 256);
  }

  // ---- weighted cross entropy: t_wce_rows_kernel's block b (256 rows) writes partial[b 4 + {0 .. 3}] doubles
  for (int64_t rows : {(int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)1 << 31}) {
    ++shapes;
    const int64_t blocks = (rows + 255) / 256;
    const WceLayout L(rows);
    CHECK(L.blocks == blocks && blocks * 256 >= rows && (blocks - 1) * 256 < rows);
    check_parts({L.partial}, {(size_t)blocks * 4 * sizeof(double)}, L.bytes);
  }
  std::printf("train_layout: %ld checks passed, %ld shapes laid out\n", checks, shapes);
  return 0;
}
