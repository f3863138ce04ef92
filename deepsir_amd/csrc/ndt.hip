// NDT registration (dsir_ndt_refine, dsir_ndt_map): the normal-distributions transform of PCL / Autoware / ndt_omp for P pairs at
// once, beside the ICP loop of icp.hip and sharing none of its scratch.  The reference cloud becomes one Gaussian per occupied
// cell; the moved source points are pulled towards the Gaussians of their own and their face-adjacent cells.  No nearest-neighbour
// search in the loop, no normals.  PCL is not installable here: parity is unpinned, THE RULE IS OWNED HERE and restated in numpy
// fp64 in deepsir_amd/ndt.py (ndt_constants, ndt_lattice_host, ndt_map_host, ndt_step_host, ndt_refine_host).
//
// ---- The map, per pair, from the pair's first Kp reference rows and the resolution res (fp32, finite, > 0)
// Lattice (ndt.h): origin = the per-axis minimum of the finite rows (finite_bounds_accumulate of cell_index.h: integer atomics,
// order-independent), edge h = max((double)res, longest extent / 2^20) in fp64 - no 1 + 2^-10 margin, NDT has no radius to contain.
// No finite row: origin 0, h = res, no cell.  Keys: point_key; the per-pair sort by key carries the original index and is stable,
// so a cell's rows stand in ascending original index; non-finite rows (KEY_NONE) sort last and belong to no cell.
// A cell is a run of equal keys, n its length, valid iff n >= 6.  Per cell in fp64, in run order:
//   mu = (sum x) / n;   C = sum (x - mu)(x - mu)^T / (n - 1)   in a second pass, six sums (00 01 02 11 12 22);
//   (lambda, V) = svd3(C), descending; the cell is invalid if lambda_1 is not a positive finite number;
//   lambda_i' = max(lambda_i, 0.01 lambda_1);   B = V diag(1 / lambda') V^T, its six upper entries only:
//   B_ab = ((V_a0 (1 / l_0')) V_b0 + (V_a1 (1 / l_1')) V_b1) + (V_a2 (1 / l_2')) V_b2.
// The record of a valid cell, ten doubles (mu 3, B 6 as 00 01 02 11 12 22, n), stands at the run's first sorted position; every
// other position of `records` is zero.  A lookup is key_lower_bound on the pair's sorted keys and one equality test: no compaction
// pass, no atomics.  `runs` holds every run's length at its first position (valid or not), so that the cells x - 1, x, x + 1 of one
// (y, z) - one key interval, ndt.h - are found by ONE binary search and up to two hops.
//
// ---- Constants: PCL's, on the host in fp64 (ndt.h ndt_constants) from the outlier ratio o and res:
//   c1 = 10 (1 - o), c2 = o / res^3, d3 = -log(c2), d1 = -log(c1 + c2) - d3, d2 = -2 log((-log(c1 exp(-1/2) + c2) - d3) / d1).
//
// ---- One iteration, over the pair's first Jp moved source points (s = the fp32 moved point taken to fp64)
// Cell of s: cell_of per axis (clamped to -2 .. MAXC + 2).  A cell is looked up only if its three coordinates lie in [0, MAXC]: a
// point outside the lattice has no own cell, its in-range face neighbours are still visited.  Cells visited, in this order: own,
// -x, +x, -y, +y, -z, +z (neighbors = 7) or the own cell alone (neighbors = 1).  Per valid cell visited:
//   d = s - mu;
//   q = (((((B00 d0) d0 + (B11 d1) d1) + (B22 d2) d2) + 2 ((B01 d0) d1)) + 2 ((B02 d0) d2)) + 2 ((B12 d1) d2);
//   e = exp(-(d2 q) / 2);   the visit contributes nothing unless q >= 0 and e is finite and e > 0;
//   w = d2 e;   g = B d, g_r = (B_r0 d0 + B_r1 d1) + B_r2 d2;
//   Jac = [-[s]x | I] (3 x 6; column k < 3 is e_k x s) - the parametrisation of the plane step, J_plane = Jac^T n;
//   BJ_k = B Jac_k (rows as g);   H_ab = (Jac_a0 BJ_b0 + Jac_a1 BJ_b1) + Jac_a2 BJ_b2,  a <= b;
//   A_ab += w H_ab (21 sums);   b += w [s x g ; g] (6 sums);   score += e;   rows += 1.
// A source point is matched if at least one visit contributed; a source point that is not finite visits nothing and is counted.
// 31 fp64 sums.  Solve A x = -b with icp_plane_solve(A, b, rows, x), unchanged; the update is icp_plane_transform(x) rounded to fp32
// once, applied to the moved points (se3_row) and composed onto T (the rounding sequence of icp_plane_step_kernel).
// The update is the IDENTITY - the moved points and T keep their bits, the pair's fifth statistic counts it - when the solve
// returns false, when the rounded update is not finite, when any of the pair's moved points is not finite, and so for Jp == 0 or
// Kp == 0 (no row).  The pair is converged when sqrt(x0^2 + x1^2 + x2^2) < step_tol and sqrt(x3^2 + x4^2 + x5^2) < step_tol res
// (fp64, on the device), and after an identity update.  A converged pair's remaining iterations are no-ops behind a device flag;
// no host round trip per iteration.
// This is iteratively reweighted Gauss-Newton on PCL's score: A is positive semi-definite by construction, so there is no line
// search; with the cell visits held fixed a step is a majorise-minimise step for the exponential loss.  The visits change as the
// points move, so MONOTONE DESCENT IS NOT PROMISED.  PCL's Newton step with second derivatives and More-Thuente line search is
// deliberately not built.
// Statistics [P][5] fp32, after the last move: score / Jp, matched / Jp (both 0 for Jp == 0), converged, iterations run, identity updates.
//
// ---- Kernels
// ndt_cell_kernel: a lane per sorted position; the lane at a run's first position walks its run (runs are tens of points): the
// summation order inside a cell is the run order whatever the launch shape.
// ndt_accum_kernel: one workgroup per (chunk of kNdtChunk source points, pair) writes the chunk's 31 sums to its own slot - wave
// butterflies, then the waves in order (block_sum).  5 binary searches per point under neighbors = 7: the x triple is one.
// ndt_step_kernel: one workgroup per 256 source points and pair adds the pair's slots in chunk order (every workgroup for itself:
// the same bits in each), solves, and moves its points; workgroup 0 composes T, tests convergence and writes the NEXT iteration's
// done flag (the flags are ping-pong, like T: no workgroup reads what another of the same launch writes).
// No floating-point atomics, no scratch shared between pairs (NdtLayout, ndt.h): the same bytes on every run, and pair p of a ragged
// batch (counts_src / counts_ref; J, K the capacities) gets, byte for byte, what a dense call on its first Jp / Kp rows alone writes -
// padding rows get KEY_NONE and sort last behind the pair's own rows (stable sorts), every kernel stops at the pair's own counts,
// and the chunks are those of Jp.
#include <float.h>

#include "device_utils.h"
#include "engine_ctx.h"
#include "kernels.h"
#include "ndt.h"
#include "svd3.h"

namespace dsir {

namespace {

constexpr int PT = 256;

__global__ __launch_bounds__(256) void ndt_bounds_kernel(const float* __restrict__ ref, int stride, int K, const int32_t* __restrict__ counts_ref,
                                                         int pairs, uint32_t* __restrict__ enc) {
  const int pair = blockIdx.y;
  finite_bounds_accumulate(ref + (int64_t)pair * K * stride, stride, pair_rows(counts_ref, pair, K), (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                           (int64_t)gridDim.x * blockDim.x, enc + pair * 3, enc + (pairs + pair) * 3);
}

// the pair's lattice (ndt.h) and the offset table of the segmented sort
__global__ void ndt_lattice_kernel(const uint32_t* __restrict__ enc, int pairs, int K, float res, CellLattice* __restrict__ lat,
                                   int32_t* __restrict__ off_ref) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > pairs) return;
  off_ref[p] = p * K;
  if (p == pairs) return;
  float lo[3], hi[3];
  bool any = true;
  for (int a = 0; a < 3; ++a) {
    const uint32_t l = enc[p * 3 + a], h = enc[(pairs + p) * 3 + a];
    any = any && l <= h;                                           // min > max: no finite row at all
    lo[a] = ord2f(l); hi[a] = ord2f(h);
  }
  lat[p] = ndt_lattice(res, lo, hi, any);
}

// keys [pairs][K], vals [pairs][K] = the row's index inside its pair; a row at or beyond the pair's count is not read and gets KEY_NONE
__global__ __launch_bounds__(256) void ndt_key_kernel(const float* __restrict__ pts, int stride, int K, const int32_t* __restrict__ counts,
                                                      const CellLattice* __restrict__ lat, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int pair = blockIdx.y;
  const CellLattice L = lat[pair];
  const int np = pair_rows(counts, pair, K);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < K; i += gridDim.x * blockDim.x) {
    const int64_t o = (int64_t)pair * K + i;
    const float* p = pts + o * stride;
    keys[o] = i < np ? point_key(p[0], p[1], p[2], L) : KEY_NONE;
    vals[o] = (uint32_t)i;
  }
}

// runs and records are zero on entry; the lane at a run's first position writes the run's length and, for a valid cell, its record
__global__ __launch_bounds__(256) void ndt_cell_kernel(const float* __restrict__ ref, int stride, int K, const int32_t* __restrict__ counts_ref,
                                                       const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                       int32_t* __restrict__ runs, double* __restrict__ records) {
  const int pair = blockIdx.y;
  const int Kp = pair_rows(counts_ref, pair, K);
  const uint64_t* Kk = keys + (int64_t)pair * K;
  const uint32_t* Vv = vals + (int64_t)pair * K;
  const float* S = ref + (int64_t)pair * K * stride;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Kp; i += gridDim.x * blockDim.x) {
    const uint64_t k = Kk[i];
    if (k == KEY_NONE || (i > 0 && Kk[i - 1] == k)) continue;
    int n = 1;
    while (i + n < Kp && Kk[i + n] == k) ++n;
    runs[(int64_t)pair * K + i] = n;
    if (n < kNdtMinPoints) continue;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int j = 0; j < n; ++j) {
      const float* p = S + (int64_t)Vv[i + j] * stride;
      sx += (double)p[0]; sy += (double)p[1]; sz += (double)p[2];
    }
    const double mx = sx / (double)n, my = sy / (double)n, mz = sz / (double)n;
    double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
    for (int j = 0; j < n; ++j) {
      const float* p = S + (int64_t)Vv[i + j] * stride;
      const double dx = (double)p[0] - mx, dy = (double)p[1] - my, dz = (double)p[2] - mz;
      c00 += dx * dx; c01 += dx * dy; c02 += dx * dz; c11 += dy * dy; c12 += dy * dz; c22 += dz * dz;
    }
    const double m = (double)(n - 1);
    c00 /= m; c01 /= m; c02 /= m; c11 /= m; c12 /= m; c22 /= m;
    const double C[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}};
    double U[3][3], lam[3], V[3][3];
    svd3(C, U, lam, V);
    if (!(lam[0] > 0.0) || !(lam[0] <= DBL_MAX)) continue;
    double il[3];
    for (int a = 0; a < 3; ++a) {
      const double floor_ = kNdtEigMult * lam[0];
      il[a] = 1.0 / (lam[a] > floor_ ? lam[a] : floor_);
    }
    double* r = records + ((int64_t)pair * K + i) * kNdtRecord;
    r[0] = mx; r[1] = my; r[2] = mz;
    int e = 3;
    for (int a = 0; a < 3; ++a)
      for (int b = a; b < 3; ++b) r[e++] = ((V[a][0] * il[0]) * V[b][0] + (V[a][1] * il[1]) * V[b][1]) + (V[a][2] * il[2]) * V[b][2];
    r[9] = (double)n;
  }
}

// cur[pair][j] = T[pair] * src[pair][j] for the pair's own rows (J: the row capacity), as the ICP loop moves its points
__global__ void ndt_apply_kernel(const float* __restrict__ src, int stride, int J, const int32_t* __restrict__ counts_src,
                                 const float* __restrict__ T, float* __restrict__ cur) {
  const int pair = blockIdx.y;
  const float* t = T + (int64_t)pair * 12;
  const int Jp = pair_rows(counts_src, pair, J);
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < Jp; j += gridDim.x * blockDim.x) {
    const float* p = src + ((int64_t)pair * J + j) * stride;
    const float x = p[0], y = p[1], z = p[2];
    float* o = cur + ((int64_t)pair * J + j) * 3;
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = se3_row(t, r, x, y, z);
  }
}

// one visit of the rule (this file's header): the record at sorted position p of the pair; true if it contributed
__device__ __forceinline__ bool ndt_visit(const double* __restrict__ rec, const double (&s)[3], double d2c, double (&v)[kNdtSums]) {
  if (!(rec[9] >= (double)kNdtMinPoints)) return false;              // a zero record: no valid cell starts here
  const double d[3] = {s[0] - rec[0], s[1] - rec[1], s[2] - rec[2]};
  const double B[3][3] = {{rec[3], rec[4], rec[5]}, {rec[4], rec[6], rec[7]}, {rec[5], rec[7], rec[8]}};
  const double q = (((((B[0][0] * d[0]) * d[0] + (B[1][1] * d[1]) * d[1]) + (B[2][2] * d[2]) * d[2]) + 2.0 * ((B[0][1] * d[0]) * d[1])) +
                    2.0 * ((B[0][2] * d[0]) * d[2])) + 2.0 * ((B[1][2] * d[1]) * d[2]);
  const double e = exp(-(d2c * q) / 2.0);
  if (!(q >= 0.0) || !(e > 0.0) || !(e <= DBL_MAX)) return false;
  const double w = d2c * e;
  double g[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) g[r] = (B[r][0] * d[0] + B[r][1] * d[1]) + B[r][2] * d[2];
  const double Jc[6][3] = {{0.0, -s[2], s[1]}, {s[2], 0.0, -s[0]}, {-s[1], s[0], 0.0}, {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  double BJ[6][3];
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int r = 0; r < 3; ++r) BJ[k][r] = (B[r][0] * Jc[k][0] + B[r][1] * Jc[k][1]) + B[r][2] * Jc[k][2];
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) v[k++] += w * ((Jc[a][0] * BJ[b][0] + Jc[a][1] * BJ[b][1]) + Jc[a][2] * BJ[b][2]);
  v[21] += w * (s[1] * g[2] - s[2] * g[1]);
  v[22] += w * (s[2] * g[0] - s[0] * g[2]);
  v[23] += w * (s[0] * g[1] - s[1] * g[0]);
  v[24] += w * g[0]; v[25] += w * g[1]; v[26] += w * g[2];
  v[kNdtScore] += e;
  v[kNdtRows] += 1.0;
  return true;
}

// done: the pairs' flags of this iteration, or nullptr (the statistics' pass after the last move: every pair)
__global__ __launch_bounds__(PT) void ndt_accum_kernel(const float* __restrict__ cur, int J, int K, const int32_t* __restrict__ counts_src,
                                                       const int32_t* __restrict__ counts_ref, const uint64_t* __restrict__ keys,
                                                       const int32_t* __restrict__ runs, const double* __restrict__ records,
                                                       const CellLattice* __restrict__ lat, int neighbors, double d2c,
                                                       const int32_t* __restrict__ done, double* __restrict__ part) {
  __shared__ double sh[(PT / 64 + 1) * kNdtSums];
  const int pair = blockIdx.y, ch = blockIdx.x;
  if (done && done[pair]) return;                    // converged: the step is a no-op (block-uniform)
  const int Jp = pair_rows(counts_src, pair, J), Kp = pair_rows(counts_ref, pair, K);
  if (ch >= icp_plane_chunks(Jp)) return;            // a chunk of padding rows only: no slot of the pair's sum (block-uniform)
  const uint64_t* Kk = keys + (int64_t)pair * K;
  const int32_t* Rn = runs + (int64_t)pair * K;
  const double* Rec = records + (int64_t)pair * K * kNdtRecord;
  const CellLattice L = lat[pair];
  const int first = ch * kNdtChunk, last = min(Jp, first + kNdtChunk);
  double v[kNdtSums];
#pragma unroll
  for (int k = 0; k < kNdtSums; ++k) v[k] = 0.0;
  // the sorted position of the cell (x, y, z), or -1: outside the key's range, or no run of that key
  auto look = [&](int x, int y, int z) -> int {
    if (!ndt_in_key(x) || !ndt_in_key(y) || !ndt_in_key(z)) return -1;
    const uint64_t k = cell_key(x, y, z);
    const int p = key_lower_bound(Kk, Kp, k);
    return p < Kp && Kk[p] == k ? p : -1;
  };
  for (int j = first + threadIdx.x; j < last; j += PT) {
    const int64_t o = (int64_t)pair * J + j;
    const float sx = cur[o * 3], sy = cur[o * 3 + 1], sz = cur[o * 3 + 2];
    if (!finite3(sx, sy, sz)) { v[kNdtBad] += 1.0; continue; }
    const double s[3] = {(double)sx, (double)sy, (double)sz};
    const int cx = cell_of(sx, L.ox, L.h), cy = cell_of(sy, L.oy, L.h), cz = cell_of(sz, L.oz, L.h);
    int p0 = -1, pm = -1, pp = -1, pym = -1, pyp = -1, pzm = -1, pzp = -1;
    if (neighbors == 1) {
      p0 = look(cx, cy, cz);
    } else {
      // the cells cx - 1, cx, cx + 1 of (cy, cz) are one key interval (ndt.h): one search, then run by run
      const int x0 = max(cx - 1, 0), x1 = min(cx + 1, MAXC);
      if (ndt_in_key(cy) && ndt_in_key(cz) && x0 <= x1) {
        const uint64_t khi = cell_key(x1, cy, cz);
        int p = key_lower_bound(Kk, Kp, cell_key(x0, cy, cz));
        while (p < Kp) {
          const uint64_t k = Kk[p];
          if (k > khi) break;
          const int dx = (int)(k & (uint64_t)MAXC) - cx;
          if (dx == 0) p0 = p; else if (dx < 0) pm = p; else pp = p;
          p += max(Rn[p], 1);                            // a run's first position holds its length (>= 1)
        }
      }
      pym = look(cx, cy - 1, cz); pyp = look(cx, cy + 1, cz);
      pzm = look(cx, cy, cz - 1); pzp = look(cx, cy, cz + 1);
    }
    bool any = false;
#pragma unroll 1
    for (int c = 0; c < neighbors; ++c) {              // own, -x, +x, -y, +y, -z, +z
      const int p = c == 0 ? p0 : c == 1 ? pm : c == 2 ? pp : c == 3 ? pym : c == 4 ? pyp : c == 5 ? pzm : pzp;
      if (p < 0) continue;
      any = ndt_visit(Rec + (int64_t)p * kNdtRecord, s, d2c, v) || any;
    }
    if (any) v[kNdtMatched] += 1.0;
  }
  block_sum<PT / 64>(v, sh);
  if (threadIdx.x < kNdtSums)
    part[((int64_t)pair * gridDim.x + ch) * kNdtSlots + threadIdx.x] = sh[(PT / 64) * kNdtSums + threadIdx.x];
}

// C = T o P for row-major 3x4 transforms, in the rounding sequence of icp_plane_step_kernel's composition
__device__ __forceinline__ void ndt_compose(const float* T, const float* P, float* C) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c)
      C[r * 4 + c] = fmaf(T[r * 4 + 2], P[2 * 4 + c], fmaf(T[r * 4 + 1], P[1 * 4 + c], __fmul_rn(T[r * 4 + 0], P[c])));
    const float rt = fmaf(T[r * 4 + 2], P[2 * 4 + 3], fmaf(T[r * 4 + 1], P[1 * 4 + 3], __fmul_rn(T[r * 4 + 0], P[3])));
    C[r * 4 + 3] = __fadd_rn(rt, T[r * 4 + 3]);
  }
}

// nch: the slots a pair has (the capacity's chunks); the pair's sum adds the icp_plane_chunks(Jp) of them that its own rows fill.
// done_in: this iteration's flags (read by every workgroup), done_out: the next iteration's (written by workgroup 0 alone)
__global__ __launch_bounds__(PT) void ndt_step_kernel(float* __restrict__ cur, int J, const int32_t* __restrict__ counts_src, int nch,
                                                      const double* __restrict__ part, const float* __restrict__ T_prev,
                                                      float* __restrict__ T_cum, double* __restrict__ state,
                                                      const int32_t* __restrict__ done_in, int32_t* __restrict__ done_out, double step_tol,
                                                      double res) {
  __shared__ double tot[kNdtSlots];
  __shared__ float sT[12];
  __shared__ int s_move;
  const int pair = blockIdx.y;
  const bool lead = blockIdx.x == 0 && threadIdx.x == 0;   // the one thread that writes the pair's transform, counters and flag
  const bool done = done_in[pair] != 0;                     // block-uniform
  if (done) {
    if (lead) {
      done_out[pair] = 1;
      for (int k = 0; k < 12; ++k) T_cum[pair * 12 + k] = T_prev[pair * 12 + k];
    }
    return;
  }
  const int Jp = pair_rows(counts_src, pair, J);
  if (threadIdx.x < kNdtSums) {
    double s = 0.0;
    const int used = icp_plane_chunks(Jp);
    for (int c = 0; c < used; ++c) s += part[((int64_t)pair * nch + c) * kNdtSlots + threadIdx.x];   // chunk order
    tot[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double x[6], Td[12];
    const bool ok = tot[kNdtBad] == 0.0 && icp_plane_solve(tot, tot + 21, tot[kNdtRows], x);
    bool move = ok;
    if (ok) {
      icp_plane_transform(x, Td);
      for (int k = 0; k < 12; ++k) {
        sT[k] = (float)Td[k];
        move = move && isfinite(sT[k]);
      }
    }
    s_move = move ? 1 : 0;
    if (lead) {
      const float* P = T_prev + pair * 12;
      float C[12];
      if (move) ndt_compose(sT, P, C);
      for (int k = 0; k < 12; ++k) T_cum[pair * 12 + k] = move ? C[k] : P[k];
      const bool conv = !move || (sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) < step_tol &&
                                  sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]) < step_tol * res);
      state[pair * kNdtState] += 1.0;
      if (!move) state[pair * kNdtState + 1] += 1.0;
      done_out[pair] = conv ? 1 : 0;
    }
  }
  __syncthreads();
  if (!s_move) return;                                      // identity update: the points keep their bits (block-uniform)
  const int j = blockIdx.x * PT + threadIdx.x;
  if (j < Jp) {
    float* p = cur + ((int64_t)pair * J + j) * 3;
    const float x = p[0], y = p[1], z = p[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = se3_row(sT, r, x, y, z);
  }
}

// stats [pairs][5] fp32 from the sums of the pass after the last move: score / Jp, matched / Jp, converged, iterations, identity updates
__global__ __launch_bounds__(64) void ndt_stats_kernel(const double* __restrict__ part, int nch, int J, const int32_t* __restrict__ counts_src,
                                                       const double* __restrict__ state, const int32_t* __restrict__ done,
                                                       float* __restrict__ stats) {
  const int pair = blockIdx.x;
  const int Jp = pair_rows(counts_src, pair, J);
  if (threadIdx.x < 2) {
    double s = 0.0;
    const int used = icp_plane_chunks(Jp);
    for (int c = 0; c < used; ++c) s += part[((int64_t)pair * nch + c) * kNdtSlots + kNdtScore + threadIdx.x];   // chunk order
    stats[pair * 5 + threadIdx.x] = Jp > 0 ? (float)(s / (double)Jp) : 0.f;
  }
  if (threadIdx.x == 2) stats[pair * 5 + 2] = done[pair] ? 1.f : 0.f;
  if (threadIdx.x == 3) stats[pair * 5 + 3] = (float)state[pair * kNdtState];
  if (threadIdx.x == 4) stats[pair * 5 + 4] = (float)state[pair * kNdtState + 1];
}

inline unsigned blocks_for(int n) { const int g = (n + 255) / 256; return (unsigned)(g < 1 ? 1 : (g > 1024 ? 1024 : g)); }

NdtLayout layout(int pairs, int J, int K) { return NdtLayout(pairs, J, K, cell_sort_tmp_bytes(pairs, K)); }

// the map of every pair into the layout's parts: bounds, lattice, keys, the stable per-pair sort, the cells
int ndt_map_build(const float* ref, int stride, int pairs, int K, const int32_t* counts_ref, float res, const NdtLayout& l, void* scratch,
                  hipStream_t st) {
  uint32_t* enc = at<uint32_t>(scratch, l.enc);
  CellLattice* lat = at<CellLattice>(scratch, l.lat);
  int32_t* off_ref = at<int32_t>(scratch, l.off_ref);
  uint64_t *keys = at<uint64_t>(scratch, l.keys), *keys_raw = at<uint64_t>(scratch, l.keys_raw);
  uint32_t *vals = at<uint32_t>(scratch, l.vals), *vals_raw = at<uint32_t>(scratch, l.vals_raw);
  const size_t nk = (size_t)pairs * (size_t)K;
  if (hipMemsetAsync(enc, 0xff, (size_t)pairs * 3 * sizeof(uint32_t), st) != hipSuccess ||
      hipMemsetAsync(enc + (size_t)pairs * 3, 0, (size_t)pairs * 3 * sizeof(uint32_t), st) != hipSuccess ||
      hipMemsetAsync(at<char>(scratch, l.runs), 0, nk * sizeof(int32_t), st) != hipSuccess ||
      hipMemsetAsync(at<char>(scratch, l.records), 0, nk * kNdtRecord * sizeof(double), st) != hipSuccess)
    return (int)hipGetLastError();
  hipLaunchKernelGGL(ndt_bounds_kernel, dim3(blocks_for(K), pairs), dim3(256), 0, st, ref, stride, K, counts_ref, pairs, enc);
  hipLaunchKernelGGL(ndt_lattice_kernel, dim3((pairs + 256) / 256), dim3(256), 0, st, (const uint32_t*)enc, pairs, K, res, lat, off_ref);
  hipLaunchKernelGGL(ndt_key_kernel, dim3(blocks_for(K), pairs), dim3(256), 0, st, ref, stride, K, counts_ref, (const CellLattice*)lat, keys_raw, vals_raw);
  if (!cell_sort_pairs(at<char>(scratch, l.tmp), l.tmp_bytes, keys_raw, keys, vals_raw, vals, pairs, K, off_ref, st)) return (int)hipErrorUnknown;
  hipLaunchKernelGGL(ndt_cell_kernel, dim3(blocks_for(K), pairs), dim3(256), 0, st, ref, stride, K, counts_ref, (const uint64_t*)keys,
                     (const uint32_t*)vals, at<int32_t>(scratch, l.runs), at<double>(scratch, l.records));
  return (int)hipGetLastError();
}

}  // namespace

}  // namespace dsir

using namespace dsir;

extern "C" int dsir_ndt_map(dsir_ctx* c, const float* points_ref, int pairs, int K, int stride, const int32_t* counts_ref, float resolution,
                            double* lattice_out, uint64_t* keys_out, int32_t* index_out, double* records_out) {
  Call call(c); if (call.refused()) return 1;
  if (!points_ref || !lattice_out || !keys_out || !index_out || !records_out || stride < 3 || !ndt_shape_ok(pairs, 1, K) ||
      !ndt_positive_finite(resolution))
    return fail(c, "dsir_ndt_map: bad arguments (resolution=%g must be finite and positive, pairs x K >= 1 and below 2^31)", (double)resolution);
  const NdtLayout l = layout(pairs, 0, K);
  void* scratch = c->ws.raw(l.bytes);
  if (c->ws.overflow) return fail(c, "workspace too small for dsir_ndt_map (raise max_points / max_pairs)");
  if (const int e = ndt_map_build(points_ref, stride, pairs, K, counts_ref, resolution, l, scratch, c->stream))
    return fail(c, "dsir_ndt_map: the map build failed (HIP error %d)", e);
  const size_t nk = (size_t)pairs * (size_t)K;
  HIP_OK(c, hipMemcpyAsync(lattice_out, at<char>(scratch, l.lat), (size_t)pairs * sizeof(CellLattice), hipMemcpyDeviceToDevice, c->stream));
  HIP_OK(c, hipMemcpyAsync(keys_out, at<char>(scratch, l.keys), nk * sizeof(uint64_t), hipMemcpyDeviceToDevice, c->stream));
  HIP_OK(c, hipMemcpyAsync(index_out, at<char>(scratch, l.vals), nk * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
  HIP_OK(c, hipMemcpyAsync(records_out, at<char>(scratch, l.records), nk * kNdtRecord * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  return call.finish();
}

extern "C" int dsir_ndt_refine(dsir_ctx* c, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                               const int32_t* counts_src, const int32_t* counts_ref, const float* T_init, float resolution, int neighbors,
                               int max_iter, float step_tol, float outlier_ratio, float* T_out, float* stats) {
  Call call(c); if (call.refused()) return 1;
  if (!points_src || !points_ref || !T_init || !T_out || stride < 3 || max_iter < 0 || !ndt_shape_ok(pairs, J, K))
    return fail(c, "dsir_ndt_refine: bad arguments");
  if (!ndt_args_ok(resolution, neighbors, step_tol, outlier_ratio))
    return fail(c, "dsir_ndt_refine: bad arguments (resolution=%g and step_tol=%g must be finite and positive, outlier_ratio=%g inside "
                   "(0, 1), neighbors=%d 1 or 7)", (double)resolution, (double)step_tol, (double)outlier_ratio, neighbors);
  const NdtLayout l = layout(pairs, J, K);
  void* scratch = c->ws.raw(l.bytes);
  if (c->ws.overflow) return fail(c, "workspace too small for dsir_ndt_refine (raise max_points / max_pairs)");
  hipStream_t st = c->stream;
  if (const int e = ndt_map_build(points_ref, stride, pairs, K, counts_ref, resolution, l, scratch, st))
    return fail(c, "dsir_ndt_refine: the map build failed (HIP error %d)", e);
  const NdtConstants k = ndt_constants((double)outlier_ratio, resolution);
  float *cur = at<float>(scratch, l.cur), *Tp = at<float>(scratch, l.Ta), *Tn = at<float>(scratch, l.Tb);
  double *part = at<double>(scratch, l.part), *state = at<double>(scratch, l.state);
  int32_t *dc = at<int32_t>(scratch, l.done), *dn = dc + pairs;
  const uint64_t* keys = at<uint64_t>(scratch, l.keys);
  const int32_t* runs = at<int32_t>(scratch, l.runs);
  const double* records = at<double>(scratch, l.records);
  const CellLattice* lat = at<CellLattice>(scratch, l.lat);
  HIP_OK(c, hipMemsetAsync(state, 0, (size_t)pairs * kNdtState * sizeof(double), st));
  HIP_OK(c, hipMemsetAsync(dc, 0, (size_t)2 * pairs * sizeof(int32_t), st));
  HIP_OK(c, hipMemcpyAsync(Tp, T_init, (size_t)pairs * 48, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(ndt_apply_kernel, dim3((J + 255) / 256, pairs), dim3(256), 0, st, points_src, stride, J, counts_src, (const float*)Tp, cur);
  const int nch = icp_plane_chunks(J);
  for (int it = 0; it < max_iter; ++it) {
    hipLaunchKernelGGL(ndt_accum_kernel, dim3(nch, pairs), dim3(PT), 0, st, (const float*)cur, J, K, counts_src, counts_ref, keys, runs, records, lat,
                       neighbors, k.d2, (const int32_t*)dc, part);
    hipLaunchKernelGGL(ndt_step_kernel, dim3((J + PT - 1) / PT, pairs), dim3(PT), 0, st, cur, J, counts_src, nch, (const double*)part, (const float*)Tp,
                       Tn, state, (const int32_t*)dc, dn, (double)step_tol, (double)resolution);
    float* t = Tp; Tp = Tn; Tn = t;
    int32_t* d = dc; dc = dn; dn = d;
  }
  HIP_OK(c, hipMemcpyAsync(T_out, Tp, (size_t)pairs * 48, hipMemcpyDeviceToDevice, st));
  if (stats) {
    hipLaunchKernelGGL(ndt_accum_kernel, dim3(nch, pairs), dim3(PT), 0, st, (const float*)cur, J, K, counts_src, counts_ref, keys, runs, records, lat,
                       neighbors, k.d2, (const int32_t*)nullptr, part);
    hipLaunchKernelGGL(ndt_stats_kernel, dim3(pairs), dim3(64), 0, st, (const double*)part, nch, J, counts_src, (const double*)state, (const int32_t*)dc,
                       stats);
  }
  return call.finish();
}
