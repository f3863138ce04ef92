// Radius and hybrid neighbour lists over the sparse cell index of overlap.hip (include/dsir_train.h, "neighbour lists"): every
// neighbour of a query inside the radius, or the max_nn nearest of them, as a CSR.  The index is dsir_t_nn_index_build's, as it is.
//
// THE RULE - overlap.hip's with "the nearest" replaced by "all"; deepsir_amd/overlap.py::radius_neighbors_host restates it:
//     the query a is moved first by match_move, ((T0 x + T1 y) + T2 z) + T3 in fp32, when poses are given; poses == NULL reads it unmoved
//     d2 = dist2_rn(b, a) = (dx dx + dy dy) + dz dz,  d = b - a          fp32, every operation rounded on its own
//     b is a neighbour of a  <=>  d2 < fl(r r)                            strict, r r one fp32 product
//     a non-finite query has an empty row; a non-finite b is in no row; a query of the target fragment finds itself (d2 = 0)
//     max_nn = 0: the whole ball.  max_nn > 0: the max_nn smallest under the lexicographic order (d2, original index), so the row has
//     min(count, max_nn) entries and a tie at the boundary goes to the lower index, whatever the walk met first
//     in both modes a row's columns ascend by original index within the target fragment; d2 (optional) is aligned with cols
// For max_nn = 0 the CSR is byte for byte dsir_t_radius_matches_count / _fill on the same two clouds.  Containment in the 27 cells
// around c(a) is overlap.hip's argument (csrc/cell_index.h, the strict `<`); rows = the jobs' query rows in job order.
//
// SHAPE: one wave per query, one query per 64-lane workgroup, queries in the query fragment's cell order.  A row here is tens to a
// few hundred entries and the cells are r (1 + 2^-10) wide, so each of the nine key runs holds many points: with one lane per query
// (nn_within_kernel) a lane would scan ~600 candidates alone at diverging run lengths and could not hold its row; with a wave the nine
// binary searches run on nine lanes at once, the runs are laid end to end and read 64 consecutive float4 at a time (coalesced), and a
// ballot orders the hits without an atomic.  Eight lanes per query (icp_nn_grid_kernel) suit one result per query; a row needs the
// 64-wide ballot and the staging below.  What it costs: at a radius of one voxel a run holds ~3 points and most lanes idle - that
// regime is nn_within's.
//   count: one walk; counts[row] = hits, or min(hits, max_nn).
//   fill:  the row reaches index order by RANKING, not by sorting: a chunk of up to 512 entries (d2 bits << 32 | index) is staged
//          through LDS in walk order, eight per lane in registers, then the row is walked again and every hit, broadcast from its
//          lane, raises the rank of the entries it precedes.  max_nn > 0 and a full row: phase A ranks by (d2, index) and keeps the
//          entry of rank max_nn - 1 as the threshold; phase B ranks the entries at or below the threshold by index, and the rank IS the
//          position in the row.  Rows above 512 entries take further chunks, each with its own two walks; the walks re-read L1 / L2.
//          Work per row is hits^2 / 64 compares per lane - ~150 at 100 entries - against ~10 loads of the walk.
// No atomics at all, no library sort; the exclusive scan of the counts is hipCUB's with RadiusSatAdd (csrc/radius_nn.h): a prefix that
// does not fit an int32 is -1 and stays -1, so the total the caller reads is -1 for EVERY total above 2^31 - 1, and the fill writes
// nothing for a row whose offsets are not both exact.  A list of more than 2^26 - 1 rows is refused: one workgroup per row.
// Every row is written by its own wave from its own walk, so two runs write the same bytes and a job's bytes do not depend on the
// rest of the list.
// The build (hipcc -O3, gfx950) reports  nn_radius_count_kernel: 18 VGPRs, 54 SGPRs, no LDS, no scratch;  nn_radius_fill_kernel:
// 52 VGPRs, 77 SGPRs, 4096 bytes of LDS, no scratch; both 8 waves per SIMD (the LDS allows 40 workgroups per CU).
// Call times: profiles/README.md, "Radius neighbour lists" (tools/bench_radius_nn.py) - count + fill 0.06 / 0.10 / 0.30 ms at 5000 /
// 16384 / 65536 points and ~70 entries a row (0.06 / 0.12 / 0.36 ms where max_nn = 30 binds); the index build in front of them
// is 5 to 9 times that.  Kernel shares and counters
// are UNMEASURED.
#include <hipcub/hipcub.hpp>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "cell_index.h"
#include "radius_nn.h"
#include "seg_sort.h"
#include "dsir_train.h"

namespace dsir {
namespace {

// the nine key runs of a query in the target's sorted keys, laid end to end: wave-uniform (scalar registers)
struct Runs { int beg[9]; int cum[10]; };

struct Query { float x, y, z; int row; bool live; };

// block -> (job, query in cell order): the query moved, its row in the CSR, its runs; live = there is something to walk
__device__ __forceinline__ Query radius_query(const uint64_t* __restrict__ keys, const float4* __restrict__ sorted, const int32_t* __restrict__ box,
                                              const int32_t* __restrict__ off, const int32_t* __restrict__ tab, int n_jobs,
                                              const float* __restrict__ poses, const CellLattice& L, int lane, Runs& R, const float4*& S) {
  const int32_t* row = tab + 2 * (int64_t)n_jobs;
  int jlo = 0, jhi = n_jobs;                                       // the last job with row[job] <= blockIdx.x
  while (jhi - jlo > 1) { const int mid = jlo + ((jhi - jlo) >> 1); if (row[mid] <= (int)blockIdx.x) jlo = mid; else jhi = mid; }
  const int job = jlo;
  const int qf = tab[2 * job], tf = tab[2 * job + 1];
  const int qb = off[qf], tb = off[tf], nt = off[tf + 1] - tb;
  const float4 p = sorted[qb + ((int)blockIdx.x - row[job])];
  Query q;
  q.row = row[job] + (int)__float_as_uint(p.w);
  q.x = p.x; q.y = p.y; q.z = p.z;
  if (poses) {
    const float* T = poses + (int64_t)job * 12;
    q.x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[0], p.x), __fmul_rn(T[1], p.y)), __fmul_rn(T[2], p.z)), T[3]);
    q.y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[4], p.x), __fmul_rn(T[5], p.y)), __fmul_rn(T[6], p.z)), T[7]);
    q.z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[8], p.x), __fmul_rn(T[9], p.y)), __fmul_rn(T[10], p.z)), T[11]);
  }
  S = sorted + tb;
#pragma unroll
  for (int i = 0; i < 9; ++i) R.beg[i] = 0;
#pragma unroll
  for (int i = 0; i < 10; ++i) R.cum[i] = 0;
  q.live = false;
  if (nt == 0 || !finite3(q.x, q.y, q.z)) return q;
  int tlo[3], thi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { tlo[a] = box[tf * 6 + a] - 1; thi[a] = box[tf * 6 + 3 + a] + 1; }
  const int cx = cell_of(q.x, L.ox, L.h), cy = cell_of(q.y, L.oy, L.h), cz = cell_of(q.z, L.oz, L.h);
  if (cx < tlo[0] || cx > thi[0] || cy < tlo[1] || cy > thi[1] || cz < tlo[2] || cz > thi[2]) return q;
  const uint64_t* K = keys + tb;
  int k = 0;                                                       // run k's interval goes to lane k
  uint64_t klo_mine = 0, khi_mine = 0;
  walk_key_intervals(cx, cy, cz, tlo[1], thi[1], tlo[2], thi[2], [&](uint64_t klo, uint64_t khi) {
    if (lane == k) { klo_mine = klo; khi_mine = khi; }
    ++k;
  });
  int b = 0, e = 0;
  if (lane < k) { b = key_lower_bound(K, nt, klo_mine); e = key_lower_bound(K, nt, khi_mine + 1); }   // khi < 2^63: no wrap; KEY_NONE stays out
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    R.beg[i] = __builtin_amdgcn_readlane(b, i);
    R.cum[i + 1] = R.cum[i] + (__builtin_amdgcn_readlane(e, i) - R.beg[i]);
  }
  q.live = R.cum[9] > 0;
  return q;
}

// f(hit, entry) for the candidates of the runs, 64 at a time in run order; every lane of the wave calls f the same number of times
template <class F>
__device__ __forceinline__ void walk_runs(const Runs& R, const float4* __restrict__ S, const Query& q, float r2, int lane, F&& f) {
  const int total = R.cum[9];
  for (int t0 = 0; t0 < total; t0 += kRadiusWave) {
    const int t = t0 + lane;
    int p = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) if (t >= R.cum[i]) p = R.beg[i] + (t - R.cum[i]);
    bool hit = false;
    uint64_t entry = 0;
    if (t < total) {
      const float4 c = S[p];
      const float d2 = dist2_rn(c, q.x, q.y, q.z);
      hit = d2 < r2;
      entry = radius_entry(__float_as_uint(d2), __float_as_uint(c.w));
    }
    f(hit, entry);
  }
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
}

__global__ __launch_bounds__(kRadiusWave) void nn_radius_count_kernel(const uint64_t* __restrict__ keys, const float4* __restrict__ sorted,
                                                                      const int32_t* __restrict__ box, const int32_t* __restrict__ off,
                                                                      const int32_t* __restrict__ tab, int n_jobs, const float* __restrict__ poses,
                                                                      float r2, CellLattice L, int max_nn, int32_t* __restrict__ counts) {
  const int lane = threadIdx.x;
  Runs R;
  const float4* S;
  const Query q = radius_query(keys, sorted, box, off, tab, n_jobs, poses, L, lane, R, S);
  int hits = 0;
  if (q.live) walk_runs(R, S, q, r2, lane, [&](bool hit, uint64_t) { hits += __popcll(__ballot(hit)); });
  if (lane == 0) counts[q.row] = max_nn > 0 ? min(hits, max_nn) : hits;
}

// One chunk: the selected hits (entry <= bound) of walk ordinal [c0, c0 + kRadiusCap) staged through LDS into own[], eight per lane,
// then ranked against every selected hit of the row - by the whole entry (BY_ENTRY: d2, then index) or by the index alone.
// -> the selected hits of the whole row.  own[j] is entry j * 64 + lane of the chunk, ~0 where the chunk has none.
template <bool BY_ENTRY>
__device__ __forceinline__ int rank_chunk(const Runs& R, const float4* __restrict__ S, const Query& q, float r2, int lane, uint64_t bound, int c0,
                                          uint64_t* __restrict__ stage, uint64_t (&own)[kRadiusOwn], int (&rank)[kRadiusOwn]) {
  int seen = 0;
  walk_runs(R, S, q, r2, lane, [&](bool hit, uint64_t entry) {
    const bool sel = hit && entry <= bound;
    const uint64_t mask = __ballot(sel);
    const int ord = seen + __popcll(mask & ((1ull << lane) - 1ull)) - c0;
    if (sel && ord >= 0 && ord < kRadiusCap) stage[ord] = entry;
    seen += __popcll(mask);
  });
  __syncthreads();
  const int E = min(kRadiusCap, seen - c0);
#pragma unroll
  for (int j = 0; j < kRadiusOwn; ++j) {
    const int e = j * kRadiusWave + lane;
    own[j] = e < E ? stage[e] : ~0ull;
    rank[j] = 0;
  }
  __syncthreads();                                                 // the next chunk stages over these
  walk_runs(R, S, q, r2, lane, [&](bool hit, uint64_t entry) {
    uint64_t mask = __ballot(hit && entry <= bound);
    while (mask) {
      const int l = __ffsll((unsigned long long)mask) - 1;
      mask &= mask - 1;
      const uint64_t h = readlane64(entry, l);
#pragma unroll
      for (int j = 0; j < kRadiusOwn; ++j)
        if (j * kRadiusWave < E) rank[j] += BY_ENTRY ? (h < own[j] ? 1 : 0) : ((uint32_t)h < (uint32_t)own[j] ? 1 : 0);
    }
  });
  return seen;
}

__global__ __launch_bounds__(kRadiusWave) void nn_radius_fill_kernel(const uint64_t* __restrict__ keys, const float4* __restrict__ sorted,
                                                                     const int32_t* __restrict__ box, const int32_t* __restrict__ off,
                                                                     const int32_t* __restrict__ tab, int n_jobs, const float* __restrict__ poses,
                                                                     float r2, CellLattice L, int max_nn, const int32_t* __restrict__ offsets,
                                                                     int32_t* __restrict__ cols, float* __restrict__ d2_out, int64_t n_cols) {
  __shared__ uint64_t stage[kRadiusCap];
  const int lane = threadIdx.x;
  Runs R;
  const float4* S;
  const Query q = radius_query(keys, sorted, box, off, tab, n_jobs, poses, L, lane, R, S);
  const int32_t begin = offsets[q.row], end = offsets[q.row + 1];
  if (!q.live || !radius_row_ok(begin, end) || end == begin) return;   // wave-uniform; a prefix that left int32 is -1: nothing is written
  const int64_t base = begin;
  const int len = end - begin;
  uint64_t own[kRadiusOwn];
  int rank[kRadiusOwn];
  uint64_t bound = ~0ull;                                          // every hit is selected
  if (max_nn > 0 && len == max_nn) {                               // a full row: hits >= max_nn, the entry of rank max_nn - 1 bounds it
    for (int c0 = 0;; c0 += kRadiusCap) {
      const int seen = rank_chunk<true>(R, S, q, r2, lane, ~0ull, c0, stage, own, rank);
      uint64_t mine = ~0ull;
#pragma unroll
      for (int j = 0; j < kRadiusOwn; ++j)
        if (own[j] != ~0ull && rank[j] == max_nn - 1) mine = own[j];
      const uint64_t found = __ballot(mine != ~0ull);
      if (found) { bound = readlane64(mine, __ffsll((unsigned long long)found) - 1); break; }
      if (c0 + kRadiusCap >= seen) break;
    }
  }
  for (int c0 = 0; c0 < len; c0 += kRadiusCap) {
    rank_chunk<false>(R, S, q, r2, lane, bound, c0, stage, own, rank);
#pragma unroll
    for (int j = 0; j < kRadiusOwn; ++j) {
      const int64_t pos = base + rank[j];
      if (own[j] != ~0ull && rank[j] >= 0 && rank[j] < len && pos >= 0 && pos < n_cols) {
        cols[pos] = (int32_t)(uint32_t)own[j];
        if (d2_out) d2_out[pos] = __uint_as_float((uint32_t)(own[j] >> 32));
      }
    }
  }
}

size_t scan_tmp_bytes(int64_t rows) {
  size_t b = 0;
  hipcub::DeviceScan::InclusiveScan(nullptr, b, (const int32_t*)nullptr, (int32_t*)nullptr, RadiusSatAdd(), (int)(rows < 1 ? 1 : rows));
  return b;
}

struct Call { const uint64_t* keys; const float4* sorted; const int32_t *box, *off; int64_t rows; };

// the refusals, the table (host) and the index's parts; rows < 0: refused
Call prepare(const void* index, const int64_t* offsets, int fragments, const int32_t* jobs, int64_t n_jobs, float radius, const float* bounds,
             int max_nn, std::vector<int32_t>* tab) {
  Call c{nullptr, nullptr, nullptr, nullptr, -1};
  if (!index || radius_nn_refusal(n_jobs, max_nn) || (n_jobs > 0 && !jobs) ||
      dsir_t_nn_within_check(offsets, fragments, jobs, n_jobs, radius, bounds))
    return c;
  std::vector<int32_t> local;
  std::vector<int32_t>& t = tab ? *tab : local;
  t.resize(radius_nn_table_ints(n_jobs));
  c.rows = radius_nn_table(offsets, fragments, jobs, n_jobs, t.data());
  if (radius_nn_rows_refusal(c.rows)) { c.rows = -1; return c; }
  const IndexLayout lay(offsets[fragments], fragments, seg_sort_tmp_bytes(offsets[fragments], fragments));
  const char* base = reinterpret_cast<const char*>(index);
  c.keys = reinterpret_cast<const uint64_t*>(base + lay.keys);
  c.sorted = reinterpret_cast<const float4*>(base + lay.sorted);
  c.box = reinterpret_cast<const int32_t*>(base + lay.box);
  c.off = reinterpret_cast<const int32_t*>(base + lay.off);
  return c;
}

}  // namespace
}  // namespace dsir

using namespace dsir;

extern "C" {

size_t dsir_t_nn_radius_scratch(int64_t n_jobs, int64_t rows) {
  if (radius_nn_refusal(n_jobs, 0) || radius_nn_rows_refusal(rows)) return 0;
  return RadiusNNLayout(n_jobs, scan_tmp_bytes(rows)).bytes;
}

int dsir_t_nn_radius_count(void* stream, const void* index, const int64_t* offsets, int fragments, const int32_t* jobs, int64_t n_jobs,
                           const float* poses, float radius, const float* bounds, int max_nn, int32_t* counts, int32_t* row_offsets,
                           void* scratch) {
  std::vector<int32_t> tab;
  const Call c = prepare(index, offsets, fragments, jobs, n_jobs, radius, bounds, max_nn, &tab);
  if (c.rows < 0 || !row_offsets || !scratch || (c.rows > 0 && !counts)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(row_offsets, 0, sizeof(int32_t), st) != hipSuccess) return (int)hipGetLastError();
  if (c.rows == 0) return 0;
  const RadiusNNLayout lay(n_jobs, scan_tmp_bytes(c.rows));
  int32_t* dtab = at<int32_t>(scratch, lay.tab);
  if (hipMemcpyAsync(dtab, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, st) != hipSuccess) return (int)hipGetLastError();
  hipLaunchKernelGGL(nn_radius_count_kernel, dim3((unsigned)c.rows), dim3(kRadiusWave), 0, st, c.keys, c.sorted, c.box, c.off, dtab, (int)n_jobs,
                     poses, radius * radius, nn_lattice(bounds, radius), max_nn, counts);
  size_t tb = lay.tmp_bytes;
  if (hipcub::DeviceScan::InclusiveScan(at<char>(scratch, lay.tmp), tb, counts, row_offsets + 1, RadiusSatAdd(), (int)c.rows, st) != hipSuccess)
    return (int)hipErrorUnknown;
  return (int)hipGetLastError();
}

int dsir_t_nn_radius_fill(void* stream, const void* index, const int64_t* offsets, int fragments, const int32_t* jobs, int64_t n_jobs,
                          const float* poses, float radius, const float* bounds, int max_nn, const int32_t* row_offsets, const void* scratch,
                          int32_t* cols, float* d2, int64_t n_cols) {
  const Call c = prepare(index, offsets, fragments, jobs, n_jobs, radius, bounds, max_nn, nullptr);
  if (c.rows < 0 || !row_offsets || !scratch || n_cols < 0 || (n_cols > 0 && !cols)) return (int)hipErrorInvalidValue;
  if (c.rows == 0 || n_cols == 0) return 0;
  const RadiusNNLayout lay(n_jobs, scan_tmp_bytes(c.rows));
  hipLaunchKernelGGL(nn_radius_fill_kernel, dim3((unsigned)c.rows), dim3(kRadiusWave), 0, (hipStream_t)stream, c.keys, c.sorted, c.box, c.off,
                     at<int32_t>(scratch, lay.tab), (int)n_jobs, poses, radius * radius, nn_lattice(bounds, radius), max_nn, row_offsets, cols, d2,
                     n_cols);
  return (int)hipGetLastError();
}

}  // extern "C"
