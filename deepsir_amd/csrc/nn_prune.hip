// Pruned nearest-descriptor search: which (row block, column tile) products of the screening (nn_screen.hip) can be skipped.
//
// On large clouds the arg-min is most of the path (71 % of the flops at 16 k points, 89 % at 64 k), and
// screen_kernel multiplies every block of src descriptors with every tile of ref descriptors.  A tile t of 64 ref descriptors with
// centroid c_t and radius r_t = max_{b in t} |b - c_t| bounds all its columns from BELOW,
//       D(a, b) = |a - b|^2 >= (|a - c_t| - r_t)_+^2        (triangle inequality),
// and any actual distance of a row bounds its minimum from ABOVE.  Two such distances are at hand:
//   * T_j = D(a_j, b_{p_j}), p_j the previous iteration's match (exact fp32, row_prep_kernel), and
//   * the smallest screening upper bound U = L + 2 d >= D over the columns of the tile whose centroid is nearest to a_j
//     (tile_T_kernel; available in iteration 0 as well, and tight when the previous match is stale after a large pose update).
// A tile whose lower bound exceeds min of the two for EVERY row of a block cannot hold the arg-min of any of them - nor tie with
// it: the skipped columns are strictly farther - and the block may skip it.  Nothing approximate enters a decision: the bounds
// only remove work, the surviving products go through the screening and the exact fp32 pick unchanged.
// The bounds bite when tiles are compact and a block's rows agree on which tiles matter.  Descriptors are continuous
// functions of position (model.py:209-235: per-point MLPs of xyz, score and local features), so
//   * ref columns are taken in MORTON ORDER of their points (once per registration: the ref side is loop invariant) - tile
//     radius 0.82 -> 0.39 / 0.13 on 16 k / 64 k-point clouds - and
//   * src rows in the order of their nearest-centroid tile (per iteration; centroid_argmin_kernel).
// Measured on the engine's descriptors (tools/prune_stats.py, "tileT"): 48 - 61 % of the products of the five iterations are
// visited at 16 384 points, 35 - 61 % at 65 536, ~all at 5 000 (79 tiles: the search is not worth pruning there and is not).
// All arithmetic of the bounds is fp32 with explicit safety margins (the exact distances they are compared with are fp32
// evaluations, too): margins of 2e-5 (1 + |a|^2 + |b|^2) against evaluation errors below 4e-6 (1 + ...) - see the kernels.
// The bound pass (centroid_argmin_kernel, tile_T_kernel, tile_bound_kernel) runs the screening's own MFMA chain and bound
// arithmetic: screen_bound.h, the one definition tests/test_gpu_screen_bound.py proves the inequality for.
#include <hipcub/hipcub.hpp>

#include <type_traits>

#include "kernels.h"
#include "screen_bound.h"
#include "scratch.h"

namespace dsir {

namespace {

inline int grid_for(int64_t n) { const int64_t g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 65535 ? 65535 : g)); }

// bounding box of every cloud's points: one 1024-thread block per cloud
__global__ __launch_bounds__(1024) void bbox_kernel(const float* __restrict__ xyz, int64_t cs, int n, float* __restrict__ box) {
  const int cloud = blockIdx.x;
  const float* p = xyz + cloud * cs;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = threadIdx.x; i < n; i += 1024)
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float v = p[(int64_t)i * 3 + k]; lo[k] = fminf(lo[k], v); hi[k] = fmaxf(hi[k], v); }
  __shared__ float sh[6][16];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float a = lo[k], b = hi[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a = fminf(a, __shfl_xor(a, o)); b = fmaxf(b, __shfl_xor(b, o)); }
    if ((threadIdx.x & 63) == 0) { sh[k][threadIdx.x >> 6] = a; sh[3 + k][threadIdx.x >> 6] = b; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = sh[threadIdx.x][0];
    for (int w = 1; w < 16; ++w) v = threadIdx.x < 3 ? fminf(v, sh[threadIdx.x][w]) : fmaxf(v, sh[threadIdx.x][w]);
    box[cloud * 6 + threadIdx.x] = v;
  }
}

__device__ __forceinline__ uint32_t spread3(uint32_t v) {
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

// Morton code (up to 30 bits) of every point inside its cloud's box (non-finite coordinates: key 0 - any order is a valid order)
__global__ void morton_kernel(const float* __restrict__ xyz, int64_t cs, int n, const float* __restrict__ box, int64_t total, int mbits,
                              uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int cloud = (int)(i / n), j = (int)(i % n);
    const float* p = xyz + cloud * cs + (int64_t)j * 3;
    const float* b = box + cloud * 6;
    uint32_t q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float ext = b[3 + k] - b[k];
      float t = ext > 0.f ? (p[k] - b[k]) / ext * 1023.f : 0.f;
      t = t == t ? fminf(fmaxf(t, 0.f), 1023.f) : 0.f;
      q[k] = (uint32_t)t;
    }
    // (cloud, code) in one 32-bit key - the code's low bits go when the cloud index needs them -: one device-wide sort
    const uint32_t m = spread3(q[0]) | (spread3(q[1]) << 1) | (spread3(q[2]) << 2);
    key[i] = ((uint32_t)cloud << mbits) | (m >> (30 - mbits));
    val[i] = (uint32_t)j;
  }
}

// order (position -> element) as int32, and its inverse (element -> position)
__global__ void order_kernel(const uint32_t* __restrict__ sorted_val, int n, int64_t total, bool identity, int32_t* __restrict__ order,
                             int32_t* __restrict__ inverse) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int v = identity ? (int)(i % n) : (int)sorted_val[i];
    order[i] = v;
    if (inverse) inverse[(i / n) * n + v] = (int)(i % n);
  }
}

// one wave per tile of 64 positions of the column order, lane = channel: centroid, |centroid|^2, radius (rounded UP)
__global__ __launch_bounds__(256) void tile_stats_kernel(const float* __restrict__ desc, const int32_t* __restrict__ cols, int K, int nt,
                                                         int64_t tiles_total, float* __restrict__ cen, float* __restrict__ cn2,
                                                         float* __restrict__ rad) {
  const int64_t tg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tg >= tiles_total) return;
  const int lane = threadIdx.x & 63;
  const int pair = (int)(tg / nt), t = (int)(tg % nt);
  const float* D = desc + (int64_t)pair * K * 64;
  const int32_t* C = cols + (int64_t)pair * K;
  const int n = min(SBC, K - t * SBC);
  float s = 0.f;
  for (int i = 0; i < n; ++i) s += D[(int64_t)C[t * SBC + i] * 64 + lane];
  const float c = s / (float)n;
  float r2 = 0.f;
  for (int i = 0; i < n; ++i) {
    const float d = D[(int64_t)C[t * SBC + i] * 64 + lane] - c;
    r2 = fmaxf(r2, wave_sum(d * d));
  }
  const float c2 = wave_sum(c * c);
  cen[tg * 64 + lane] = c;
  if (lane == 0) {
    cn2[tg] = c2;
    rad[tg] = sqrtf(r2) * 1.00001f + 1e-6f;          // upper bound of the radius: fp32 sum of 64 squares + sqrt, errors < 1e-6 relative
  }
}

// DOMAIN of the margins below (2e-5 (1 + |a|^2 + |b_prev|^2) on T, 1e-5 (1 + |a|^2 + |c|^2) on L): they cover the fp32 evaluation error
// of a SKIPPED column only while that column's own |b|^2 is of the order of the norms they are built from.  The pruned search is
// reachable from dsir_register alone (search_plan.h: the pruned mode requires the registration's own descriptors), and those are L2-normalised by
// the aggregation chain (model.py:232-233: |a| = |b| = 1 up to rounding); it is not offered to caller-supplied descriptors
// (dsir_nn_match searches exhaustively or through the unpruned screening, whose bound carries every column's own norm).
// per src row: the sort key of the row order (its nearest-centroid tile) and the upper bound from the previous iteration's match,
// T = D(a, b_prev) + margin, D evaluated as nn_match.hip evaluates it (exact_dist);
// iteration 0 (idx_prev == nullptr): +inf (tile_T_kernel supplies the bound)
__global__ __launch_bounds__(256) void row_prep_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       const float* __restrict__ sa, const float* __restrict__ sb,
                                                       const int32_t* __restrict__ idx_prev, const int32_t* __restrict__ tstar, int J, int K,
                                                       int tbits, int64_t total, bool keep_all, uint32_t* __restrict__ key,
                                                       uint32_t* __restrict__ val, float* __restrict__ T) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int pair = (int)(i / J);
    float bound = INFINITY;
    if (idx_prev && !keep_all) {
      int k = idx_prev[i];
      k = k < 0 ? 0 : (k >= K ? K - 1 : k);
      const float san = sa[i], sbn = sb[(int64_t)pair * K + k];
      const float d = exact_dist(reinterpret_cast<const float4*>(a + i * 64), b + ((int64_t)pair * K + k) * 64, san, sbn);
      // non-finite rows get an infinite bound (they visit every tile)
      if (d == d) bound = d + kMarginExact * (1.f + san + sbn);
    }
    T[i] = bound;
    key[i] = ((uint32_t)pair << tbits) | (uint32_t)tstar[i];
    val[i] = (uint32_t)(i % J);
  }
}

// the ref side's screening operands in column order: 16 bytes per thread (a row of 64 halves = 8 pieces, hi and lo), + the seeds
__global__ __launch_bounds__(256) void permute_ref_kernel(const uint4* __restrict__ bh, const uint4* __restrict__ bl, const float* __restrict__ sb,
                                                          const int32_t* __restrict__ cols, int K, int64_t total, uint4* __restrict__ ph,
                                                          uint4* __restrict__ pl, float* __restrict__ psb) {
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < total * 8; f += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = f >> 3;
    const int piece = (int)(f & 7);
    const int64_t src = (i / K) * K + cols[i];
    ph[f] = bh[src * 8 + piece];
    pl[f] = bl[src * 8 + piece];
    if (piece == 0) psb[i] = sb[src];
  }
}

__global__ void prune_account_kernel(const int32_t* __restrict__ tcount, int n, int nt, unsigned long long* __restrict__ acc) {
  unsigned long long kept = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) kept += (unsigned long long)tcount[i];
  kept = (unsigned long long)wave_sum((double)kept);
  if ((threadIdx.x & 63) == 0 && kept) atomicAdd(acc, kept);
  if (threadIdx.x == 0) atomicAdd(acc + 1, (unsigned long long)n * (unsigned long long)nt);
}

// ---- the bound pass on the matrix core: which column tiles must a row block visit?
// A tile t (SBC ref columns, centroid c_t, radius r_t) can be skipped by a row whose minimum is known to be <= T iff
// (|a - c_t| - r_t)_+^2 > T.  |a - c_t|^2 is bounded from BELOW by the screening's own bound (screen_bound.h): the centroids are split
// like descriptors and L(a, c_t) <= D(a, c_t) comes out of the same six-MFMA chain (rows x nt centroids: 1/64 of a search).
// Block = 8 waves x RT row tiles = one row block of the screening (rows in the given order); per 16-centroid step every lane
// tests its column against its 4 RT rows, the wave folds the answers into a 16-bit column mask, and the tiles some row needs
// are compacted into the block's list.
template <int RT>
__global__ __launch_bounds__(512) void tile_bound_kernel(const _Float16* __restrict__ Ah, const _Float16* __restrict__ Al,
                                                         const float* __restrict__ sa, const int32_t* __restrict__ rows,
                                                         const float* __restrict__ T, const _Float16* __restrict__ Ch,
                                                         const _Float16* __restrict__ Cl, const float* __restrict__ cn2,
                                                         const float* __restrict__ rad, int J, int nt, int32_t* __restrict__ tlist,
                                                         int32_t* __restrict__ tcount, int tl_stride) {
  __shared__ unsigned int flags[kMaxBoundTiles / 16];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int rb = blockIdx.x, pair = blockIdx.y, nrb = gridDim.x;
  const int64_t arow = (int64_t)pair * J;
  const int row0 = (rb * 8 + w) * (16 * RT);
  const int nsteps = (nt + 15) >> 4;
  for (int i = tid; i < nsteps; i += 512) flags[i] = 0u;
  ScreenFrag af[RT];
  // skip iff (sqrt(lo) 0.99999 - r)_+^2 > T, tested without a square root per element as lo > ((sqrt(T) + r) k)^2, k = kMarginRoot:
  // slo2 = |a|^2 - d_a - margin per row (+inf for rows past the end: they need nothing), sT = sqrt(T) k per row, r k per column
  float slo2[RT][4], sT[RT][4];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    af[rt] = screen_frag(Ah, Al, arow + rows[arow + min(row0 + rt * 16 + fr, J - 1)], fq);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int pos = row0 + rt * 16 + 4 * fq + r;
      const int re = rows[arow + min(pos, J - 1)];
      const float san = sa[arow + re];
      slo2[rt][r] = pos < J ? screen_slo(san) - kMarginCentroid * (1.f + san) : INFINITY;
      sT[rt][r] = pos < J ? sqrtf(T[arow + re]) * kMarginRoot : 0.f;      // T < 0 or NaN: NaN - the row visits every tile
    }
  }
  __syncthreads();
  const _Float16* ch = Ch + (int64_t)pair * nt * 64;
  const _Float16* cl = Cl + (int64_t)pair * nt * 64;
  // the next step's centroid fragments travel while the current step's MFMAs run (a step's own loads were exposed: 24 MFMAs
  // cannot start before four 16-byte loads and two scalars have come back)
  struct CFrag { ScreenFrag b; float c2, rad; };
  auto cload = [&](int s) {
    const int tc = min(16 * s + fr, nt - 1);
    return CFrag{screen_frag(ch, cl, tc, fq), cn2[(int64_t)pair * nt + tc], rad[(int64_t)pair * nt + tc]};
  };
  CFrag nxt = cload(0);
  for (int s = 0; s < nsteps; ++s) {
    const CFrag cur = nxt;
    if (s + 1 < nsteps) nxt = cload(s + 1);
    const float rk = cur.rad * kMarginRoot;
    const float cterm = kMarginCentroid * cur.c2;
    const float seed = 16 * s + fr < nt ? screen_seed(cur.c2) : -INFINITY;      // tiles past the end: L = +inf (their flags are not read)
    bool need = false;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const f32x4 z = screen_chain(af[rt], cur.b, seed);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // L <= D(a, c) (the screening bound), D(a, c) within kMarginCentroid (1 + |a|^2 + |c|^2) of the true |a - c|^2: a lower bound of that
        const float lo = screen_lower(z[r], slo2[rt][r]) - cterm;
        const float thr = sT[rt][r] + rk;
        need = need || !(lo > thr * thr);                                        // NaN anywhere: visit
      }
    }
    const unsigned long long m = __ballot(need);
    const unsigned int m16 = (unsigned int)((m | (m >> 16) | (m >> 32) | (m >> 48)) & 0xffffull);
    if (lane == 0 && m16) atomicOr(&flags[s], m16);
  }
  __syncthreads();
  if (tid < 64) {
    int32_t* out = tlist + ((int64_t)pair * nrb + rb) * tl_stride;
    int cnt = 0;
    for (int base = 0; base < nt; base += 64) {
      const int t = base + tid;
      const bool f = t < nt && ((flags[t >> 4] >> (t & 15)) & 1u);
      const unsigned long long m = __ballot(f);
      if (f) out[cnt + __popcll(m & ((1ull << tid) - 1ull))] = t;
      cnt += __popcll(m);
    }
    if (tid == 0) tcount[pair * nrb + rb] = cnt;
  }
}

// ---- where does a row look first?  The tile whose CENTROID is nearest (smallest screening lower bound L(a, c_t)), per src row, rows
// in their natural order.  That tile orders the rows (rows that start in the same tile sit in the same row block and agree on
// which tiles matter) and supplies an upper bound of the row's minimum that does not need a previous iteration (tile_T_kernel).
// Same MFMA chain and operands as tile_bound_kernel; L = slo_row - 2^-21 z', so the arg-min of L over t is the arg-max of z'.
template <int RT>
__global__ __launch_bounds__(512) void centroid_argmin_kernel(const _Float16* __restrict__ Ah, const _Float16* __restrict__ Al,
                                                              const _Float16* __restrict__ Ch, const _Float16* __restrict__ Cl,
                                                              const float* __restrict__ cn2, int J, int nt, int32_t* __restrict__ tstar) {
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int rb = blockIdx.x, pair = blockIdx.y;
  const int64_t arow = (int64_t)pair * J;
  const int row0 = (rb * 8 + w) * (16 * RT);
  if (row0 >= J) return;                                 // wave-uniform; no barrier in this kernel
  ScreenFrag af[RT];
  float bz[RT][4];
  int bt[RT][4];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    af[rt] = screen_frag(Ah, Al, arow + min(row0 + rt * 16 + fr, J - 1), fq);
#pragma unroll
    for (int r = 0; r < 4; ++r) { bz[rt][r] = -INFINITY; bt[rt][r] = 0; }
  }
  const _Float16* ch = Ch + (int64_t)pair * nt * 64;
  const _Float16* cl = Cl + (int64_t)pair * nt * 64;
  const int nsteps = (nt + 15) >> 4;
  for (int s = 0; s < nsteps; ++s) {
    const int t = 16 * s + fr;
    const int tc = min(t, nt - 1);
    const ScreenFrag b = screen_frag(ch, cl, tc, fq);
    const float seed = t < nt ? screen_seed(cn2[(int64_t)pair * nt + tc]) : -INFINITY;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const f32x4 z = screen_chain(af[rt], b, seed);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (z[r] > bz[rt][r]) { bz[rt][r] = z[r]; bt[rt][r] = t; }        // NaN never wins; first (lowest) tile on ties within a lane
    }
  }
  // the 16 lanes of a row group hold its column classes: larger z' wins, the lower tile on ties (any tile is a valid choice)
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float z = bz[rt][r];
      int t = bt[rt][r];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const float zo = __shfl_xor(z, o);
        const int to = __shfl_xor(t, o);
        if (zo > z || (zo == z && to < t)) { z = zo; t = to; }
      }
      const int row = row0 + rt * 16 + 4 * fq + r;
      if (fr == 0 && row < J) tstar[arow + row] = t;
    }
}

// ---- an upper bound of every row's minimum from the tiles its 16-row group points at.  One wave per 16 consecutive rows of the row
// ORDER (rows sorted by their nearest-centroid tile: a group points at one or two tiles): for every distinct tile among the
// group's rows the screening chain on (16 rows x SBC columns of the ref operands in column order), U = L + 2 d >= D(row, column)
// for every (row, column) - the screening's proven upper bound of the exact fp32 distance -, so min U over ANY columns bounds the
// row minimum from above.  T[row] = min(T[row], min U + margin): T arrives holding the bound from the previous iteration's match
// (or +inf in iteration 0) and leaves as what tile_bound_kernel prunes against.  (64-row groups - a tile's operands read once per
// 64 rows - measured twice as slow: 4 x fewer waves with 3 x longer dependent chains; the kernel is latency-, not bandwidth-bound.)
__global__ __launch_bounds__(256) void tile_T_kernel(const _Float16* __restrict__ Ah, const _Float16* __restrict__ Al,
                                                     const float* __restrict__ sa, const int32_t* __restrict__ rows,
                                                     const int32_t* __restrict__ tstar, const _Float16* __restrict__ Bh,
                                                     const _Float16* __restrict__ Bl, const float* __restrict__ sbp, int J, int K, int nt,
                                                     float* __restrict__ T) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int pair = blockIdx.y;
  const int g0 = (blockIdx.x * 4 + w) * 16;              // first position of the wave's group in the row order
  if (g0 >= J) return;                                   // wave-uniform; no barrier in this kernel
  const int64_t arow = (int64_t)pair * J, brow = (int64_t)pair * K;
  const int ra = rows[arow + min(g0 + fr, J - 1)];        // the row whose A fragment this lane holds
  const ScreenFrag af = screen_frag(Ah, Al, arow + ra, fq);
  int rowe[4];
  float san[4], slo[4], best[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    rowe[r] = rows[arow + min(g0 + 4 * fq + r, J - 1)];
    san[r] = sa[arow + rowe[r]];
    slo[r] = screen_slo(san[r]);
    best[r] = INFINITY;
  }
  int mine = tstar[arow + ra];                            // the tile this lane's row points at (lanes fr, all four fq copies)
  mine = mine < 0 ? 0 : (mine >= nt ? nt - 1 : mine);
  bool pending = g0 + fr < J;
  for (int guard = 0; guard < 16; ++guard) {              // at most 16 distinct tiles per group
    // the lowest tile some lane still waits for
    int t = pending ? mine : 0x7fffffff;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) t = min(t, __shfl_xor(t, o));
    if (t == 0x7fffffff) break;                           // wave-uniform
    if (mine == t) pending = false;
#pragma unroll
    for (int s = 0; s < SBC / 16; ++s) {
      const int pos = min(SBC * t + 16 * s + fr, K - 1);
      const bool live = SBC * t + 16 * s + fr < K;
      const float sbk = sbp[brow + pos];
      const f32x4 z = screen_chain(af, screen_frag(Bh, Bl, brow + pos, fq), screen_seed(sbk));
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // U = L + 2 d + the margin row_prep_kernel puts on an exact distance
        const float u = screen_upper(screen_lower(z[r], slo[r]), san[r], sbk) + kMarginExact * (1.f + san[r] + sbk);
        if (live) best[r] = fminf(best[r], u);           // NaN: ignored (a row without finite bound keeps +inf: it visits every tile)
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float b = best[r];
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) b = fminf(b, __shfl_xor(b, o));
    if (fr == 0 && g0 + 4 * fq + r < J) {
      const float old = T[arow + rowe[r]];
      T[arow + rowe[r]] = fminf(old, b);                   // one writer per row
    }
  }
}

// the row blocks of every pair by descending tile count (ties: by index): the persistent search takes the long items first, so
// that its last round is made of short ones (longest-processing-time-first; the tail of a launch was up to one full-length item,
// 18 % of the kernel at 65536 points).  One workgroup per pair, rank by counting - a pair has at most a few hundred row blocks
__global__ __launch_bounds__(256) void rank_blocks_kernel(const int32_t* __restrict__ tcount, int nrb, int32_t* __restrict__ rborder) {
  const int32_t* c = tcount + (int64_t)blockIdx.x * nrb;
  int32_t* out = rborder + (int64_t)blockIdx.x * nrb;
  for (int i = threadIdx.x; i < nrb; i += 256) {
    const int ci = c[i];
    int rank = 0;
    for (int j = 0; j < nrb; ++j) { const int cj = c[j]; rank += (cj > ci || (cj == ci && j < i)) ? 1 : 0; }
    out[rank] = i;
  }
}

struct Layout {
  int32_t *cols, *rows, *tlist, *tcount, *queue, *rborder, *tstar;
  float *cen, *cn2, *rad, *T, *box;
  _Float16 *ch, *cl;                   // the centroids as the screening's fp16 pairs
  _Float16 *pbh, *pbl;                 // the ref side's fp16 pairs in column order
  float* psb;
  uint32_t *k0, *k1, *v0, *v1;
  void* cub;
  size_t cub_bytes, total;
};

Layout carve(void* scratch, int pairs, int J, int K) {
  const int nt = (K + SBC - 1) / SBC;
  const int rpb = nn_screen_rows_per_block(J);
  const int nrb = (J + rpb - 1) / rpb;
  const size_t nmax = (size_t)pairs * (size_t)(J > K ? J : K);
  Carve c;
  Layout L{};
  L.cols = at<int32_t>(scratch, c.take((size_t)pairs * K * 4));
  L.rows = at<int32_t>(scratch, c.take((size_t)pairs * J * 4));
  L.tstar = at<int32_t>(scratch, c.take((size_t)pairs * J * 4));
  L.tlist = at<int32_t>(scratch, c.take((size_t)pairs * nrb * nt * 4));
  L.tcount = at<int32_t>(scratch, c.take((size_t)pairs * nrb * 4));
  L.queue = at<int32_t>(scratch, c.take(8 * 4));
  L.rborder = at<int32_t>(scratch, c.take((size_t)pairs * nrb * 4));
  L.cen = at<float>(scratch, c.take((size_t)pairs * nt * 64 * 4));
  L.ch = at<_Float16>(scratch, c.take((size_t)pairs * nt * 64 * 2));
  L.cl = at<_Float16>(scratch, c.take((size_t)pairs * nt * 64 * 2));
  L.cn2 = at<float>(scratch, c.take((size_t)pairs * nt * 4));
  L.rad = at<float>(scratch, c.take((size_t)pairs * nt * 4));
  L.T = at<float>(scratch, c.take((size_t)pairs * J * 4));
  L.box = at<float>(scratch, c.take((size_t)pairs * 6 * 4));
  L.k0 = at<uint32_t>(scratch, c.take(nmax * 4));
  L.k1 = at<uint32_t>(scratch, c.take(nmax * 4));
  L.v0 = at<uint32_t>(scratch, c.take(nmax * 4));
  L.v1 = at<uint32_t>(scratch, c.take(nmax * 4));
  L.pbh = at<_Float16>(scratch, c.take((size_t)pairs * K * 64 * 2));
  L.pbl = at<_Float16>(scratch, c.take((size_t)pairs * K * 64 * 2));
  L.psb = at<float>(scratch, c.take((size_t)pairs * K * 4));
  // temporary storage of the two radix sorts: sized for the largest sort over all 32 key bits; every sort asks again for its own
  // size and bit range and refuses to run if the answer exceeds this (sort_pairs)
  size_t tmp = 0;
  if (hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                         (int)nmax, 0, 32) != hipSuccess)
    tmp = 0;                       // no storage: sort_pairs fails, the caller reports the error
  L.cub = at<char>(scratch, c.take(tmp));
  L.cub_bytes = tmp;
  L.total = c.p;
  return L;
}

// (key, value) radix sort k0 / v0 -> k1 / v1 over key bits [0, end_bit): the library is asked for the temporary size of THIS sort first
int sort_pairs(const Layout& L, int64_t total, int end_bit, hipStream_t st) {
  size_t need = 0;
  if (hipcub::DeviceRadixSort::SortPairs(nullptr, need, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                         (int)total, 0, end_bit, st) != hipSuccess || need > L.cub_bytes || L.cub_bytes == 0)
    return 1;
  size_t tmp = L.cub_bytes;
  return hipcub::DeviceRadixSort::SortPairs(L.cub, tmp, L.k0, L.k1, L.v0, L.v1, (int)total, 0, end_bit, st) != hipSuccess;
}

inline int bits_for(int n) { int b = 0; while ((1ll << b) < n) ++b; return b; }   // smallest b with 2^b >= n

// the bound pass works on the screening's row blocks: f(its row tiles per wave for this J, as an integral constant)
template <typename F>
void with_row_tiles(int J, F&& f) {
  if (nn_screen_rows_per_block(J) == 512) f(std::integral_constant<int, 4>{});
  else                                    f(std::integral_constant<int, 2>{});
}

// nearest-centroid tile of every src row (natural row order)
void launch_centroid_argmin(const Layout& L, const _Float16* Ah, const _Float16* Al, int pairs, int J, int nrb, int nt, hipStream_t st) {
  with_row_tiles(J, [&](auto rt) {
    hipLaunchKernelGGL(centroid_argmin_kernel<decltype(rt)::value>, dim3(nrb, pairs), dim3(512), 0, st, Ah, Al, L.ch, L.cl, L.cn2, J, nt, L.tstar);
  });
}

// T[row] = min(T[row], upper bound from the tiles the row's 16-row group (in the row order) points at)
void launch_tile_T(const Layout& L, const _Float16* Ah, const _Float16* Al, const float* sa, int pairs, int J, int K, int nt, hipStream_t st) {
  hipLaunchKernelGGL(tile_T_kernel, dim3((J + 63) / 64, pairs), dim3(256), 0, st, Ah, Al, sa, L.rows, L.tstar, L.pbh, L.pbl, L.psb, J, K, nt, L.T);
}

// tile lists of every (pair, row block) for the row order L.rows and the per-row upper bounds L.T; rborder (optional): their ranking
void launch_tile_bound(const Layout& L, const _Float16* Ah, const _Float16* Al, const float* sa, int pairs, int J, int nrb, int nt,
                       int32_t* rborder, hipStream_t st) {
  with_row_tiles(J, [&](auto rt) {
    hipLaunchKernelGGL(tile_bound_kernel<decltype(rt)::value>, dim3(nrb, pairs), dim3(512), 0, st, Ah, Al, sa, L.rows, L.T, L.ch, L.cl, L.cn2,
                       L.rad, J, nt, L.tlist, L.tcount, nt);
  });
  if (rborder) hipLaunchKernelGGL(rank_blocks_kernel, dim3(pairs), dim3(256), 0, st, L.tcount, nrb, rborder);
}

}  // namespace

bool nn_prune_supported(int pairs, int J, int K) {
  if (bits_for(pairs) + bits_for(K) > 32 || bits_for(pairs) > 12) return false;     // the sorts' composite 32-bit keys
  return (K + SBC - 1) / SBC <= kMaxBoundTiles && (int64_t)pairs * (J > K ? J : K) <= 0x7fffffffll && nn_screen_rows_per_block(J) <= 512;
}

size_t nn_prune_scratch_bytes(int pairs, int J, int K) { return carve(nullptr, pairs, J, K).total; }

// once per registration: the column order (Morton order of the ref points) and the tiles' centroids / radii
int launch_prune_ref(const float* ref_xyz, int64_t xyz_cs, const float* desc_r, const void* bh, const void* bl, const float* sb, int pairs, int J,
                     int K, void* scratch, hipStream_t st) {
  const Layout L = carve(scratch, pairs, J, K);
  const int nt = (K + SBC - 1) / SBC;
  const int64_t total = (int64_t)pairs * K;
  const int pbits = bits_for(pairs);
  const int mbits = 32 - pbits < 30 ? 32 - pbits : 30;
  hipLaunchKernelGGL(bbox_kernel, dim3(pairs), dim3(1024), 0, st, ref_xyz, xyz_cs, K, L.box);
  hipLaunchKernelGGL(morton_kernel, dim3(grid_for(total)), dim3(256), 0, st, ref_xyz, xyz_cs, K, L.box, total, mbits, L.k0, L.v0);
  if (sort_pairs(L, total, mbits + pbits, st)) return 1;
  hipLaunchKernelGGL(order_kernel, dim3(grid_for(total)), dim3(256), 0, st, L.v1, K, total, false, L.cols, (int32_t*)nullptr);
  const int64_t tiles_total = (int64_t)pairs * nt;
  hipLaunchKernelGGL(tile_stats_kernel, dim3((unsigned)((tiles_total + 3) / 4)), dim3(256), 0, st, desc_r, L.cols, K, nt, tiles_total, L.cen, L.cn2,
                     L.rad);
  // the centroids in the screening's operand format (and |c|^2 in its summation order): the bound pass runs its MFMA chain
  launch_split16_norm(L.cen, tiles_total, L.ch, L.cl, L.cn2, st);
  hipLaunchKernelGGL(permute_ref_kernel, dim3(grid_for(total * 8)), dim3(256), 0, st, reinterpret_cast<const uint4*>(bh),
                     reinterpret_cast<const uint4*>(bl), sb, L.cols, K, total, reinterpret_cast<uint4*>(L.pbh), reinterpret_cast<uint4*>(L.pbl), L.psb);
  return 0;
}

// per iteration (>= 1): the row order, the rows' upper bounds and the tile lists of every row block -> ord
int launch_prune_rows(const float* desc_s, const float* desc_r, const void* ah, const void* al, const float* sa, const float* sb,
                      const int32_t* idx_prev, int pairs, int J, int K, void* scratch, hipStream_t st, ScreenOrder* ord, unsigned long long* acc) {
  const Layout L = carve(scratch, pairs, J, K);
  const int nt = (K + SBC - 1) / SBC;
  const int rpb = nn_screen_rows_per_block(J);
  const int nrb = (J + rpb - 1) / rpb;
  const int64_t total = (int64_t)pairs * J;
  const int tbits = bits_for(nt);
  static const bool id_rows = tuning_flag("DSIR_PRUNE_ID_ROWS");     // measurement hook: rows in their natural order
  static const bool no_lpt = tuning_flag("DSIR_PRUNE_NO_LPT");       // A/B hook: items in row-block order
  static const bool keep_all = tuning_flag("DSIR_PRUNE_KEEP_ALL");   // measurement hook: every tile on every list (the mechanism's own cost)
  static const bool no_tile_T = tuning_flag("DSIR_PRUNE_NO_TILE_T"); // A/B hook: upper bounds from the previous match only
  const _Float16 *Ah = reinterpret_cast<const _Float16*>(ah), *Al = reinterpret_cast<const _Float16*>(al);
  launch_centroid_argmin(L, Ah, Al, pairs, J, nrb, nt, st);
  hipLaunchKernelGGL(row_prep_kernel, dim3(grid_for(total)), dim3(256), 0, st, desc_s, desc_r, sa, sb, idx_prev, L.tstar, J, K, tbits, total,
                     keep_all, L.k0, L.v0, L.T);
  if (sort_pairs(L, total, tbits + bits_for(pairs), st)) return 1;
  hipLaunchKernelGGL(order_kernel, dim3(grid_for(total)), dim3(256), 0, st, L.v1, J, total, id_rows, L.rows, (int32_t*)nullptr);
  if (!keep_all && !no_tile_T) launch_tile_T(L, Ah, Al, sa, pairs, J, K, nt, st);
  launch_tile_bound(L, Ah, Al, sa, pairs, J, nrb, nt, no_lpt ? nullptr : L.rborder, st);
  if (acc) hipLaunchKernelGGL(prune_account_kernel, dim3(1), dim3(256), 0, st, L.tcount, pairs * nrb, nt, acc);
  ord->rows = L.rows;
  ord->cols = L.cols;
  ord->bh = L.pbh;
  ord->bl = L.pbl;
  ord->sbp = L.psb;
  ord->tlist = L.tlist;
  ord->tcount = L.tcount;
  ord->tl_stride = nt;
  (void)hipMemsetAsync(L.queue, 0, 8 * 4, st);
  ord->queue = L.queue;
  ord->rborder = no_lpt ? nullptr : L.rborder;
  return 0;
}

}  // namespace dsir
