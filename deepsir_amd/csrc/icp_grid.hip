// Cell-indexed nearest neighbour for the ICP loop (icp.hip, search = 1): the same neighbour index and the same d2 bits as the brute
// force of icp_nn_kernel, from a sparse cell index of the reference cloud that is built once per call and searched up to
// max_iter + 1 times.  The index is overlap.hip's (points sorted by a 64-bit cell key, 27 cells around the query; csrc/cell_index.h
// holds what both files share: CellLattice, point_key, the bounds accumulation, key_lower_bound, walk_key_intervals, dist2_rn);
// what differs is the rule's `<=` and a lattice that is made per pair on the device.
//
// The rule (header of icp.hip, unchanged):
//     d = ref - cur,  d2 = (dx dx + dy dy) + dz dz        fp32, every operation rounded on its own
//     the neighbour is the reference point with the smallest d2; ties go to the LOWER ORIGINAL INDEX
//     accepted  <=>  d2 <= r2,  r2 = fl(r r)              NOT the strict < of overlap.hip
//     a non-finite query matches nothing; a non-finite reference point is never a neighbour
//     outputs as icp_nn_kernel writes them: idx = the index or -1, d2 = the distance or 0.f
//
// The lattice, one per PAIR, made on the device (no host round trip): origin o = the minimum over the pair's finite reference points
// (integer atomics on the order-preserving map of cell_index.h: order-independent), cell edge
//     h = max(r (1 + 2^-10), 2^-60, longest axis extent / 2^20)      in fp64 (csrc/icp_grid.h, restated in deepsir_amd/icp.py)
// cell coordinate c(a) = floor(((double)a - (double)o) / h) per axis.  Why no reference point b that the rule accepts for a query a
// can lie outside the 27 cells around c(a): the argument of csrc/cell_index.h with `<=` - fl(dx dx) <= d2 <= fl(r r) gives
// |b - a| <= r (1 + 2^-21) per axis, and |b - a| / h <= (1 + 2^-21) / (1 + 2^-10) < 1 - 2^-11 stays strict for every h >= r (1 + 2^-10);
// a coarser h only lowers the quotient.
// Where products underflow (fl(r r) or fl(dx dx) below 2^-126) the relative bounds do not hold; then dx^2 < 2^-126 + 2^-149 + r2,
// so for r < 2^-61 |dx| < 2^-60 = the floor of h, and for r >= 2^-61 r r is a normal number and an underflowing dx dx has
// |dx| < 2^-63 < r.  The coarsened edge in place of a refused extent: the third term
// of h bounds a reference coordinate by 2^20 (extent / h <= 2^20 (1 + 2^-52)), so c + 1 fits the 21 bits an axis has in the key
// x | y << 21 | z << 42 and NO EXTENT IS REFUSED: a far-flung cloud gets coarser cells, a slower and still exact search.  A query that
// T has moved out of the lattice is clamped to -2 or 2^21 + 1 cells: more than one cell from every reference cell, and h >= the
// radius bound above, so it has no admissible neighbour and finds none.  A pair without a finite reference point has keys ~0 only,
// which lie in no interval: every query is unmatched.
//
// Index build, once per call: per-pair bounds, lattice, keys, hipCUB segmented radix sort (one segment per pair; a library step, as in
// overlap.hip; pairs of 4096 points and more go one by one through hipCUB's device-wide radix sort instead, because the segmented
// sort leaves a segment to one workgroup - both are stable, so the order is the same), gather into (x, y, z, original index) float4
// in key order.  Query order, once per call: the keys of the source
// points moved by T_init under the same lattice, one more sort, the permutation kept for the whole loop (ICP moves the points by a
// small fraction of the cloud).  Results are written in original numbering.
//
// icp_nn_grid_kernel, the hot path: a group of 8 neighbouring lanes per query, group t of a pair takes query perm[t], so a wave's
// groups sit in the same or adjacent cells and their probes and run reads meet in the same cache lines.  Per query 9 lookups
// (dy, dz) in {-1, 0, 1}^2, each the key interval [key(cx - 1), key(cx + 1)]: a binary search (every lane of the group, the same
// probes), then a scan of the run in which lane s takes positions lo + s, lo + s + 8, .. four at a time (four key loads and four
// point loads in flight per lane; a group's eight loads are neighbouring rows; positions past the interval are predicated off, and
// the first one ends the lane's run).  The lanes compare (d2, original index) lexicographically and the group's best is the minimum
// of its lanes' by the same order (three xor exchanges), so the tie rule rests neither on the order inside a cell nor on which lane
// saw a point.  Per-lane scans, not a wave-cooperative scan of the lanes' united intervals through LDS: DESIGN.md §8 gives the
// reasons and the build's figures.  The same `skip` early-out as icp_nn_kernel.
// No atomics on floating-point values, no scratch shared between pairs (csrc/icp_grid.h: part p of every array is pair p's), no
// dependence on the order of arrival: two runs write the same bytes and a pair's bytes do not depend on the other pairs of the call.
//
// Clouds of unequal sizes (counts_src / counts_ref of IcpArgs; J, K the row capacities and the strides of every part): the bounds, the
// lattice, the keys and the gather see a pair's own rows only; a padding row - reference or query - is not read and gets KEY_NONE,
// so it sorts last, behind the pair's own non-finite rows and in index order (both sorts are stable; the SEG_MAX choice stays a
// function of the capacity), and lies in no interval.  The first Kp sorted positions and the first Jp entries of the query order are
// therefore those of the pair indexed alone, and the search takes Kp as the length of the pair's keys: the same probes, the same
// runs, the same bytes as for a pair of J = Jp, K = Kp.  Query groups t >= Jp write -1 and 0.f and leave (whole groups: the xor
// exchanges stay inside a group); a pair with Kp == 0 walks nothing.  The guarantees above hold as stated, counts included.
#include <hipcub/hipcub.hpp>
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "icp_grid.h"
#include "seg_sort.h"

namespace dsir {

namespace {

constexpr int GB = 256;      // threads per block of the search: 4 waves
constexpr int SUB = 8;       // lanes per query: a full-resolution pair has about as many queries as the chip has lanes, so one
                             // lane per query leaves one wave per SIMD and nothing to hide the run's load latency behind
constexpr int UNROLL = 4;    // positions a lane has in flight
constexpr int SEG_MAX = 4095;   // longer segments are sorted pair by pair with the device-wide sort: the segmented sort gives a
                                // segment to one workgroup (10^5 keys: 3.4 ms measured on the MI355X)

// lo [3 pairs], hi [3 pairs]: min / max xyz of each pair's finite reference rows (its own rows of the capacity K), as ordered integers
__global__ __launch_bounds__(256) void icp_grid_bounds_kernel(const float* __restrict__ ref, int stride, int K, const int32_t* __restrict__ counts_ref,
                                                              int pairs, uint32_t* __restrict__ enc) {
  const int pair = blockIdx.y;
  finite_bounds_accumulate(ref + (int64_t)pair * K * stride, stride, pair_rows(counts_ref, pair, K), (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                           (int64_t)gridDim.x * blockDim.x, enc + pair * 3, enc + (pairs + pair) * 3);
}

// the pair's lattice (icp_grid.h) and both offset tables of the segmented sorts
__global__ void icp_grid_lattice_kernel(const uint32_t* __restrict__ enc, int pairs, int J, int K, float r, IcpLattice* __restrict__ lat,
                                        int32_t* __restrict__ off_ref, int32_t* __restrict__ off_qry) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > pairs) return;
  off_ref[p] = p * K;
  off_qry[p] = p * J;
  if (p == pairs) return;
  float lo[3], hi[3];
  bool any = true;
  for (int a = 0; a < 3; ++a) {
    const uint32_t l = enc[p * 3 + a], h = enc[(pairs + p) * 3 + a];
    any = any && l <= h;                                           // min > max: no finite row at all
    lo[a] = ord2f(l); hi[a] = ord2f(h);
  }
  lat[p] = icp_grid_lattice(r, lo, hi, any);
}

// keys [pairs][n], vals [pairs][n] = the row's index inside its pair; rows of `stride` floats.  A row at or beyond the pair's count
// is not read and gets KEY_NONE: the sorts are stable, so the padding sorts last, behind the pair's own non-finite rows, in index
// order, and the first count positions of the sorted pair are those of the pair sorted alone
__global__ __launch_bounds__(256) void icp_grid_key_kernel(const float* __restrict__ pts, int stride, int n, const int32_t* __restrict__ counts,
                                                           const IcpLattice* __restrict__ lat, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int pair = blockIdx.y;
  const IcpLattice L = lat[pair];
  const int np = pair_rows(counts, pair, n);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int64_t o = (int64_t)pair * n + i;
    const float* p = pts + o * stride;
    keys[o] = i < np ? point_key(p[0], p[1], p[2], L) : KEY_NONE;
    vals[o] = (uint32_t)i;
  }
}

// sorted [pairs][K] = (x, y, z, original index) in key order; of a pair with a count its first count positions, which hold its own rows
__global__ __launch_bounds__(256) void icp_grid_gather_kernel(const float* __restrict__ ref, int stride, int K, const int32_t* __restrict__ counts_ref,
                                                              const uint32_t* __restrict__ vals, float4* __restrict__ sorted) {
  const int pair = blockIdx.y;
  const int Kp = pair_rows(counts_ref, pair, K);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Kp; i += gridDim.x * blockDim.x) {
    const int64_t o = (int64_t)pair * K + i;
    const uint32_t v = vals[o];
    sorted[o] = gather_xyzi(ref + ((int64_t)pair * K + v) * stride, v);
  }
}

// J, K: the row capacities (the strides of every per-pair array); the pair searches its first Kp sorted positions for its first Jp
// queries in cell order, exactly as the kernel does for a pair of J = Jp, K = Kp alone
__global__ __launch_bounds__(GB) void icp_nn_grid_kernel(const float* __restrict__ cur, int J, int K, const int32_t* __restrict__ counts_src,
                                                         const int32_t* __restrict__ counts_ref, const uint64_t* __restrict__ keys,
                                                         const float4* __restrict__ sorted, const int32_t* __restrict__ perm,
                                                         const IcpLattice* __restrict__ lat, float r2, int32_t* __restrict__ idx,
                                                         float* __restrict__ d2, const int32_t* __restrict__ skip) {
  // a converged pair keeps the correspondences of its last search: its points no longer move (block-uniform exit)
  if (skip && skip[blockIdx.y]) return;
  const int pair = blockIdx.y;
  const int64_t g = (int64_t)blockIdx.x * GB + threadIdx.x;
  const int sub = (int)(g % SUB);
  if (g / SUB >= J) return;                                        // whole groups leave: the shuffles below stay inside a group
  const int t = (int)(g / SUB);
  const int Jp = pair_rows(counts_src, pair, J), Kp = pair_rows(counts_ref, pair, K);
  if (t >= Jp) {                                                   // a padding row (position t of the query order is row t: the padding
    if (sub == 0) { idx[(int64_t)pair * J + t] = -1; d2[(int64_t)pair * J + t] = 0.f; }   // sorts last, in index order): whole groups leave
    return;
  }
  const int q = perm ? perm[(int64_t)pair * J + t] : t;
  const float* c = cur + ((int64_t)pair * J + q) * 3;
  const float x = c[0], y = c[1], z = c[2];
  float bd = INFINITY;
  int bi = -1;
  if (finite3(x, y, z) && Kp > 0) {                                // uniform in a group
    const IcpLattice L = lat[pair];
    const int cx = cell_of(x, L.ox, L.h), cy = cell_of(y, L.oy, L.h), cz = cell_of(z, L.oz, L.h);
    const uint64_t* Kk = keys + (int64_t)pair * K;
    const float4* S = sorted + (int64_t)pair * K;
    walk_key_intervals(cx, cy, cz, -1, MAXC + 1, -1, MAXC + 1, [&](uint64_t klo, uint64_t khi) {
      // lane `sub` of the group takes positions lo + sub, lo + sub + SUB, ..: the group's loads are SUB neighbouring rows
      for (int64_t i = (int64_t)key_lower_bound(Kk, Kp, klo) + sub; i < Kp; i += UNROLL * SUB) {
        uint64_t k[UNROLL];
        float4 s[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
          const int64_t ii = min(i + (int64_t)u * SUB, (int64_t)Kp - 1);                             // never past the pair's Kp
          k[u] = Kk[ii]; s[u] = S[ii];
        }
        bool more = true;
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
          const bool in = i + (int64_t)u * SUB < Kp && k[u] <= khi;   // keys ascend: the first position outside ends the lane's run
          more = more && in;
          const float e2 = dist2_rn(s[u], x, y, z);
          const int ti = (int)__float_as_uint(s[u].w);
          if (more && e2 <= r2 && (e2 < bd || (e2 == bd && ti < bi))) { bd = e2; bi = ti; }
        }
        if (!more) break;
      }
    });
  }
  // the group's best by (d2, original index): a minimum, so the order of the exchange does not matter
#pragma unroll
  for (int o = 1; o < SUB; o <<= 1) {
    const float od = __shfl_xor(bd, o);
    const int oi = __shfl_xor(bi, o);
    if (oi >= 0 && (bi < 0 || od < bd || (od == bd && oi < bi))) { bd = od; bi = oi; }
  }
  if (sub == 0) {
    idx[(int64_t)pair * J + q] = bi;
    d2[(int64_t)pair * J + q] = bi >= 0 ? bd : 0.f;
  }
}

inline unsigned blocks_for(int n) { const int g = (n + 255) / 256; return (unsigned)(g < 1 ? 1 : (g > 1024 ? 1024 : g)); }

size_t dev_sort_tmp_bytes(int n) {
  size_t b = 0;
  hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, n);
  return b;
}

inline IcpGridLayout layout(int pairs, int J, int K) {
  const int64_t nj = (int64_t)pairs * J, nk = (int64_t)pairs * K;
  const size_t a = J > SEG_MAX ? dev_sort_tmp_bytes(J) : seg_sort_tmp_bytes(nj, pairs);
  const size_t b = K > SEG_MAX ? dev_sort_tmp_bytes(K) : seg_sort_tmp_bytes(nk, pairs);
  return IcpGridLayout(pairs, J, K, a > b ? a : b);
}

// keys / vals [pairs][n] sorted per pair (both sorts are stable radix sorts: the same order from either)
bool sort_pairs(void* tmp, size_t tmp_bytes, const uint64_t* kin, uint64_t* kout, const uint32_t* vin, uint32_t* vout, int pairs, int n,
                const int32_t* off, hipStream_t st) {
  if (n <= SEG_MAX) {
    size_t tb = tmp_bytes;
    return hipcub::DeviceSegmentedRadixSort::SortPairs(tmp, tb, kin, kout, vin, vout, (int)((int64_t)pairs * n), pairs, off, off + 1, 0, 64, st) ==
           hipSuccess;
  }
  for (int p = 0; p < pairs; ++p) {
    size_t tb = tmp_bytes;
    const int64_t o = (int64_t)p * n;
    if (hipcub::DeviceRadixSort::SortPairs(tmp, tb, kin + o, kout + o, vin + o, vout + o, n, 0, 64, st) != hipSuccess) return false;
  }
  return true;
}

}  // namespace

// the same per-pair sort for the other cell-indexed maps (ndt.hip): the SEG_MAX choice, the temporary size and the sort, as they are here
size_t cell_sort_tmp_bytes(int pairs, int n) { return n > SEG_MAX ? dev_sort_tmp_bytes(n) : seg_sort_tmp_bytes((int64_t)pairs * n, pairs); }
bool cell_sort_pairs(void* tmp, size_t tmp_bytes, const uint64_t* kin, uint64_t* kout, const uint32_t* vin, uint32_t* vout, int pairs, int n,
                     const int32_t* off, hipStream_t st) {
  return sort_pairs(tmp, tmp_bytes, kin, kout, vin, vout, pairs, n, off, st);
}

size_t icp_grid_scratch_bytes(int pairs, int J, int K) {
  if (!icp_grid_shape_ok(pairs, J, K)) return 0;
  return layout(pairs, J, K).bytes;
}

// cur [pairs][J][3]: the source points moved by T_init (the query order is taken from them; order = false: original numbering)
// counts_src / counts_ref (nullable): the pairs' own rows.  The segments of both sorts stay the capacities J and K (so does the SEG_MAX
// choice): padding rows carry KEY_NONE and both sorts are stable, so a pair's own rows come out in the order of the pair sorted alone.
int icp_grid_build(const float* ref, int stride, const float* cur, int pairs, int J, int K, const int32_t* counts_src, const int32_t* counts_ref,
                   float r, bool order, void* scratch, hipStream_t st, IcpGrid* out) {
  if (!icp_grid_shape_ok(pairs, J, K) || !icp_grid_radius_ok(r) || !scratch || !out) return (int)hipErrorInvalidValue;
  const IcpGridLayout lay = layout(pairs, J, K);
  IcpLattice* lat = at<IcpLattice>(scratch, lay.lat);
  uint32_t* enc = at<uint32_t>(scratch, lay.enc);
  int32_t* off_ref = at<int32_t>(scratch, lay.off_ref);
  int32_t* off_qry = at<int32_t>(scratch, lay.off_qry);
  uint64_t* keys = at<uint64_t>(scratch, lay.keys);
  float4* sorted = at<float4>(scratch, lay.sorted);
  int32_t* perm = at<int32_t>(scratch, lay.perm);
  uint64_t* keys_raw = at<uint64_t>(scratch, lay.keys_raw);
  uint32_t* vals_raw = at<uint32_t>(scratch, lay.vals_raw);
  uint32_t* vals = at<uint32_t>(scratch, lay.vals);
  uint64_t* keys_qry = at<uint64_t>(scratch, lay.keys_qry);
  if (hipMemsetAsync(enc, 0xff, (size_t)pairs * 3 * sizeof(uint32_t), st) != hipSuccess ||
      hipMemsetAsync(enc + (size_t)pairs * 3, 0, (size_t)pairs * 3 * sizeof(uint32_t), st) != hipSuccess)
    return (int)hipGetLastError();
  hipLaunchKernelGGL(icp_grid_bounds_kernel, dim3(blocks_for(K), pairs), dim3(256), 0, st, ref, stride, K, counts_ref, pairs, enc);
  hipLaunchKernelGGL(icp_grid_lattice_kernel, dim3((pairs + 256) / 256), dim3(256), 0, st, (const uint32_t*)enc, pairs, J, K, r, lat, off_ref,
                     off_qry);
  hipLaunchKernelGGL(icp_grid_key_kernel, dim3(blocks_for(K), pairs), dim3(256), 0, st, ref, stride, K, counts_ref, (const IcpLattice*)lat, keys_raw, vals_raw);
  if (!sort_pairs(at<char>(scratch, lay.tmp), lay.tmp_bytes, keys_raw, keys, vals_raw, vals, pairs, K, off_ref, st)) return (int)hipErrorUnknown;
  hipLaunchKernelGGL(icp_grid_gather_kernel, dim3(blocks_for(K), pairs), dim3(256), 0, st, ref, stride, K, counts_ref, (const uint32_t*)vals, sorted);
  if (order) {
    hipLaunchKernelGGL(icp_grid_key_kernel, dim3(blocks_for(J), pairs), dim3(256), 0, st, cur, 3, J, counts_src, (const IcpLattice*)lat, keys_raw, vals_raw);
    if (!sort_pairs(at<char>(scratch, lay.tmp), lay.tmp_bytes, keys_raw, keys_qry, vals_raw, reinterpret_cast<uint32_t*>(perm), pairs, J, off_qry, st))
      return (int)hipErrorUnknown;
  }
  out->keys = keys; out->sorted = sorted; out->perm = order ? perm : nullptr; out->lat = lat;
  return (int)hipGetLastError();
}

void launch_icp_nn_grid(const IcpGrid& g, const float* cur, int pairs, int J, int K, const int32_t* counts_src, const int32_t* counts_ref, float r2,
                        int32_t* idx, float* d2, const int32_t* skip, hipStream_t st) {
  hipLaunchKernelGGL(icp_nn_grid_kernel, dim3((unsigned)(((int64_t)J * SUB + GB - 1) / GB), pairs), dim3(GB), 0, st, cur, J, K, counts_src, counts_ref,
                     (const uint64_t*)g.keys,
                     reinterpret_cast<const float4*>(g.sorted), g.perm, reinterpret_cast<const IcpLattice*>(g.lat), r2, idx, d2, skip);
}

}  // namespace dsir
