// What radius_nn.hip decides on the host, as plain C++ that compiles without a device (tools/radius_nn_check.cpp): the refusals it adds to
// dsir_t_nn_within_check, the job table the kernels read, and the scratch layout (carved with scratch.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "scratch.h"

namespace dsir {

constexpr int kRadiusWave = 64;                     // lanes per query: one wave
constexpr int kRadiusOwn = 8;                       // staged entries a lane owns
constexpr int kRadiusCap = kRadiusWave * kRadiusOwn;   // entries of a row ranked per chunk; longer rows take more chunks
constexpr int64_t kRadiusMaxJobs = 0x3fffffffll;
constexpr int64_t kRadiusMaxRows = (1ll << 26) - 1; // one 64-lane workgroup per row: a launch takes fewer than 2^32 threads

// the table on the device: jobs [n][2] | row [n + 1] (prefix of the jobs' query rows = of their blocks: one block per row)
inline size_t radius_nn_table_ints(int64_t n_jobs) { return (size_t)(3 * n_jobs + 1); }

// NULL, or why the call is refused on top of what dsir_t_nn_within_check refuses
inline const char* radius_nn_refusal(int64_t n_jobs, int max_nn) {
  if (max_nn < 0) return "nn_radius: max_nn must be 0 (the whole ball) or positive";
  if (n_jobs < 0 || n_jobs > kRadiusMaxJobs) return "nn_radius: between 0 and 2^30 - 1 jobs";
  return nullptr;
}
// the same for the query rows of a job list (radius_nn_table's result)
inline const char* radius_nn_rows_refusal(int64_t rows) {
  if (rows < 0) return "nn_radius: job index out of range, or more than 2^31 - 1 query rows";
  if (rows > kRadiusMaxRows) return "nn_radius: more than 2^26 - 1 query rows in one job list (one workgroup per row): split it";
  return nullptr;
}

// The sum the row offsets are scanned with: exact while it fits an int32, else -1, and -1 sticks.  On counts >= 0 it is associative
// (the result is -1 exactly when the true sum of the operands' rows exceeds 2^31 - 1), so a parallel scan may group it freely:
// every prefix that does not fit is -1, the total among them, whatever the true total is - 2^32 and beyond included.
struct RadiusSatAdd {
  constexpr int32_t operator()(int32_t a, int32_t b) const {
    return (a < 0 || b < 0 || a > 0x7fffffff - b) ? -1 : a + b;
  }
};
// where a row's entries go: its offsets are usable only when both are exact (no -1) and ordered
constexpr bool radius_row_ok(int32_t begin, int32_t end) { return begin >= 0 && end >= begin; }

// tab [radius_nn_table_ints(n_jobs)] from offsets [F + 1] and jobs [n][2] -> the query rows of the list, or -1 where a job index is
// outside [0, F) or the rows exceed 2^31 - 1 (dsir_t_nn_within_check refuses both first; this never reads outside offsets)
inline int64_t radius_nn_table(const int64_t* offsets, int F, const int32_t* jobs, int64_t n_jobs, int32_t* tab) {
  int32_t* row = tab + 2 * n_jobs;
  int64_t rows = 0;
  row[0] = 0;
  for (int64_t j = 0; j < n_jobs; ++j) {
    const int32_t q = jobs[2 * j], t = jobs[2 * j + 1];
    if (q < 0 || q >= F || t < 0 || t >= F) return -1;
    rows += offsets[q + 1] - offsets[q];
    if (rows < 0 || rows > 0x7fffffffll) return -1;
    tab[2 * j] = q; tab[2 * j + 1] = t;
    row[j + 1] = (int32_t)rows;
  }
  return rows;
}

// the scratch of _count / _fill: the table, then the scan's temporary
struct RadiusNNLayout {
  size_t tab, tmp, tmp_bytes, bytes;
  RadiusNNLayout(int64_t n_jobs, size_t scan_tmp_bytes) {
    Carve c;
    tab = c.take(radius_nn_table_ints(n_jobs < 0 ? 0 : n_jobs) * sizeof(int32_t));
    tmp_bytes = scan_tmp_bytes;
    tmp = c.take(tmp_bytes < 256 ? 256 : tmp_bytes);
    bytes = c.p;
  }
};

// a row's entry while it is ranked: the fp32 bits of d2 (non-negative, so ordered as integers) above the original index -
// the lexicographic order (d2, index) is the order of these integers
constexpr uint64_t radius_entry(uint32_t d2_bits, uint32_t index) { return ((uint64_t)d2_bits << 32) | index; }

}  // namespace dsir
