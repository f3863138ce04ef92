// Fast Point Feature Histograms (dsir_fpfh): the classical descriptor of the feature-matching baseline (Rusu, Blodow, Beetz, ICRA
// 2009; PCL FPFHEstimation, open3d compute_fpfh_feature), from what the engine already has on the device: points, normals and
// neighbour lists.  open3d cannot be imported where this is tested, so parity is unpinned: THE RULE IS OWNED HERE and restated in
// numpy in deepsir_amd/fpfh.py (fpfh_host), which the tests compare against byte for byte.
//
// ARITHMETIC RULE.  All float64 on the fp32 inputs, every operation rounded once, NO contraction (the pragma below; sqrt and the
// divisions through __dsqrt_rn / __ddiv_rn).  atan2 is the one operation whose last bit may differ between host and device.
//   dot(a, b)   = (a0 b0 + a1 b1) + a2 b2
//   cross(a, b) = (a1 b2 - a2 b1,  a2 b0 - a0 b2,  a0 b1 - a1 b0)
//   A row of point i is cols[start(i) .. start(i) + deg(i)); fixed lists: start = 16 i, deg = 16; CSR: start = offsets[c n + i],
//   deg = offsets[c n + i + 1] - start (a negative deg reads as 0).  Neighbour indices are cloud-local and clamped into [0, n).
//   Pair (i, j), j in the row of i:
//     d = p_j - p_i;  L2 = dot(d, d);  L = sqrt(L2)
//     skipped: j == i, not (L2 > 0), a non-finite coordinate of p_i or p_j, a normal that is (0, 0, 0) or not finite
//     a1 = dot(n_i, d) / L;  a2 = dot(n_j, d) / L
//     |a1| < |a2|:  s = n_j, t = n_i, d = -d, f3 = -a2       else:  s = n_i, t = n_j, f3 = a1
//         (PCL compares acos|a1| with acos|a2|; acos is decreasing on [0, 1], so this is the same choice without acos)
//     v = cross(d, s);  |v| = sqrt(dot(v, v));  skipped when not (|v| > 0);  v = v / |v| (three divisions)
//     w = cross(s, v);  f2 = dot(v, t);  f1 = atan2(dot(w, t), dot(s, t))
//     b1 = clamp(floor((11 (f1 + pi)) / (2 pi)), 0, 10);  b2 = 11 + clamp(floor((11 (f2 + 1)) / 2), 0, 10);  b3 = 22 + that of f3
//   SPFH(i): INTEGER counts of b1, b2, b3 over the pairs of i that were not skipped, and their number valid(i): 34 ints per point.
//     As a value, bin = (100 count) / valid(i); all zero when valid(i) == 0.
//   FPFH(i): acc = 0;  for j in list order with L2 > 0:  acc[b] = acc[b] + SPFH_value(j)[b] / L2
//     per block of 11 bins: sum = ((acc[0] + acc[1]) + ...) ascending;  sum > 0: acc[b] = acc[b] * (100 / sum)
//     row[b] = fp32(acc[b] + SPFH_value(i)[b]), then +0 up to out_ld.  valid(i) == 0: the row is all zeros and flags[i] = 1.
//
// WHERE IT DEPARTS from PCL / open3d.  (1) The neighbourhood is a list the caller hands in (the pyramid's 16-NN rows, or a radius
// CSR), not a hybrid radius / max_nn search.  (2) PCL's f3 and f2 are not clamped before binning and an out-of-range bin is
// dropped or written out of the block; here every bin is clamped.  (3) The weight is 1 / L2 as in PCL, but every block is scaled to
// 100 BEFORE the point's own SPFH is added (PCL adds nothing of its own when the point is not in its list; open3d adds the own SPFH
// and does not rescale): a row's blocks sum to 200 wherever the point and one neighbour have a valid pair.  (4) Counts are integers
// until pass 2, so nothing depends on the order in which pairs are counted.
//
// TWO PASSES.  Pass 1 (fpfh_spfh_kernel): a group of 16 lanes per point strides over the point's row, one lane per (point, slot);
// the histogram is 34 ints per point in LDS, integer adds only; a workgroup of 256 lanes owns 16 consecutive points of one cloud and
// stores their 544 ints as one contiguous run.  Pass 2 (fpfh_gather_kernel): the same 16 lanes per point walk the row IN LIST ORDER;
// lane l carries bins l, l + 16 and (l == 0) 32 in fp64, every lane forms L2 of the current neighbour for itself (same inputs, same
// bits); a neighbour's 136-byte SPFH row is one coalesced read of the group.  The block sums are taken from LDS, each lane adding
// the 11 bins of its block in ascending order.  No floating-point atomics anywhere: two runs write the same bytes, and a cloud's
// bytes depend on nothing outside the cloud.  Both passes are launch- and latency-bound at the project's sizes (8 x 5000 points:
// 2500 workgroups; the table, 5.4 MB, stays in L2).
#include "device_utils.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace dsir {

namespace {

constexpr int kGroup = 16;                    // lanes per point
constexpr int kPtsPerBlock = 256 / kGroup;    // points per workgroup
constexpr double kPi = 3.14159265358979323846;
constexpr double kTwoPi = 2.0 * kPi;

struct Vec3 { double x, y, z; };
__device__ __forceinline__ double dot3(const Vec3& a, const Vec3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ Vec3 cross3(const Vec3& a, const Vec3& b) {
  return Vec3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ Vec3 load3(const float* p) { return Vec3{(double)p[0], (double)p[1], (double)p[2]}; }
__device__ __forceinline__ bool finite3(const Vec3& a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }
__device__ __forceinline__ bool usable_normal(const Vec3& a) { return finite3(a) && (a.x != 0.0 || a.y != 0.0 || a.z != 0.0); }
__device__ __forceinline__ int bin11(double x) {
  const double f = floor(x);
  return f < 0.0 ? 0 : (f > 10.0 ? 10 : (int)f);
}

// the row of point i of `cloud`: where it starts in cols and how many entries it has
__device__ __forceinline__ void list_of(const FpfhArgs& a, int cloud, int i, int64_t& start, int& deg) {
  if (a.offsets) {
    const int64_t r = (int64_t)cloud * a.n + i;
    const int32_t s = a.offsets[r], e = a.offsets[r + 1];
    start = s < 0 ? 0 : s;
    deg = (s < 0 || e < s) ? 0 : e - s;
  } else {
    start = cloud * a.neigh_cs + (int64_t)i * kKnn;
    deg = kKnn;
  }
}
__device__ __forceinline__ int neighbour(const FpfhArgs& a, int64_t pos) {
  return min(max(a.cols[pos], 0), a.n - 1);      // a bad neighbour index can never leave the cloud
}

// squared length of p_j - p_i, the rule's L2 (NaN or 0 where the pair does not count)
__device__ __forceinline__ double pair_l2(const Vec3& pi, const Vec3& pj, Vec3& d) {
  d = Vec3{pj.x - pi.x, pj.y - pi.y, pj.z - pi.z};
  return dot3(d, d);
}

// the three bins of pair (i, j); false: the pair is skipped
__device__ __forceinline__ bool pair_bins(const FpfhArgs& a, int cloud, int i, int j, int& b1, int& b2, int& b3) {
  if (j == i) return false;
  const float* P = a.pts + cloud * a.pts_cs;
  const float* N = a.nrm + cloud * a.nrm_cs;
  const Vec3 pi = load3(P + (int64_t)i * a.pts_ld), pj = load3(P + (int64_t)j * a.pts_ld);
  const Vec3 ni = load3(N + (int64_t)i * a.nrm_ld), nj = load3(N + (int64_t)j * a.nrm_ld);
  Vec3 d;
  const double L2 = pair_l2(pi, pj, d);
  if (!(L2 > 0.0) || !finite3(pi) || !finite3(pj) || !usable_normal(ni) || !usable_normal(nj)) return false;
  const double L = __dsqrt_rn(L2);
  const double a1 = __ddiv_rn(dot3(ni, d), L), a2 = __ddiv_rn(dot3(nj, d), L);
  const bool swap = fabs(a1) < fabs(a2);
  const Vec3 s = swap ? nj : ni, t = swap ? ni : nj;
  if (swap) d = Vec3{-d.x, -d.y, -d.z};
  const double f3 = swap ? -a2 : a1;
  Vec3 v = cross3(d, s);
  const double vn = __dsqrt_rn(dot3(v, v));
  if (!(vn > 0.0)) return false;
  v = Vec3{__ddiv_rn(v.x, vn), __ddiv_rn(v.y, vn), __ddiv_rn(v.z, vn)};
  const Vec3 w = cross3(s, v);
  const double f2 = dot3(v, t);
  const double f1 = atan2(dot3(w, t), dot3(s, t));
  b1 = bin11(__ddiv_rn(11.0 * (f1 + kPi), kTwoPi));
  b2 = 11 + bin11(__ddiv_rn(11.0 * (f2 + 1.0), 2.0));
  b3 = 22 + bin11(__ddiv_rn(11.0 * (f3 + 1.0), 2.0));
  return true;
}

// pass 1: table[cloud][i][0 .. 33) = the counts of SPFH(i), [33] = valid(i)
__global__ __launch_bounds__(256) void fpfh_spfh_kernel(const FpfhArgs a) {
  __shared__ int hist[kPtsPerBlock * kFpfhRow];
  const int cloud = blockIdx.y;
  const int g = threadIdx.x / kGroup, l = threadIdx.x % kGroup;
  const int i0 = blockIdx.x * kPtsPerBlock, i = i0 + g;
  for (int q = threadIdx.x; q < kPtsPerBlock * kFpfhRow; q += 256) hist[q] = 0;
  __syncthreads();
  if (i < a.n) {
    int64_t start; int deg;
    list_of(a, cloud, i, start, deg);
    for (int k = l; k < deg; k += kGroup) {            // no cross-lane step inside the loop
      int b1, b2, b3;
      if (!pair_bins(a, cloud, i, neighbour(a, start + k), b1, b2, b3)) continue;
      int* h = hist + g * kFpfhRow;
      atomicAdd(h + b1, 1); atomicAdd(h + b2, 1); atomicAdd(h + b3, 1); atomicAdd(h + kFpfhDim, 1);
    }
  }
  __syncthreads();
  const int live = min(kPtsPerBlock, a.n - i0) * kFpfhRow;       // the workgroup's points are consecutive: one contiguous run
  int32_t* out = a.table + ((int64_t)cloud * a.n + i0) * kFpfhRow;
  for (int q = threadIdx.x; q < live; q += 256) out[q] = hist[q];
}

// pass 2: the weighted sum of the neighbours' SPFH in list order, the block scaling, the point's own SPFH, one rounding to fp32
__global__ __launch_bounds__(256) void fpfh_gather_kernel(const FpfhArgs a) {
  __shared__ double accs[kPtsPerBlock * kFpfhDim];
  const int cloud = blockIdx.y;
  const int g = threadIdx.x / kGroup, l = threadIdx.x % kGroup;
  const int i = blockIdx.x * kPtsPerBlock + g;
  const bool live = i < a.n;
  const int32_t* table = a.table + (int64_t)cloud * a.n * kFpfhRow;
  if (live) {
    const float* P = a.pts + cloud * a.pts_cs;
    const Vec3 pi = load3(P + (int64_t)i * a.pts_ld);
    int64_t start; int deg;
    list_of(a, cloud, i, start, deg);
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;          // bins l, l + 16, 32 (lane 0)
    for (int k = 0; k < deg; ++k) {
      const int j = neighbour(a, start + k);
      Vec3 d;
      const double L2 = pair_l2(pi, load3(P + (int64_t)j * a.pts_ld), d);
      if (!(L2 > 0.0)) continue;                        // uniform over the group: every lane has the same L2
      const int32_t* row = table + (int64_t)j * kFpfhRow;
      const int valid = row[kFpfhDim];
      if (valid <= 0) continue;                         // SPFH_value(j) is all zeros: + 0 / L2 changes nothing
      const double dv = (double)valid;
      acc0 = acc0 + __ddiv_rn(__ddiv_rn(100.0 * (double)row[l], dv), L2);
      acc1 = acc1 + __ddiv_rn(__ddiv_rn(100.0 * (double)row[l + kGroup], dv), L2);
      if (l == 0) acc2 = acc2 + __ddiv_rn(__ddiv_rn(100.0 * (double)row[2 * kGroup], dv), L2);
    }
    double* mine = accs + g * kFpfhDim;
    mine[l] = acc0; mine[l + kGroup] = acc1;
    if (l == 0) mine[2 * kGroup] = acc2;
  }
  __syncthreads();
  if (!live) return;
  const int32_t* own = table + (int64_t)i * kFpfhRow;
  const int valid = own[kFpfhDim];
  float* out = a.desc + ((int64_t)cloud * a.n + i) * a.out_ld;
  const double* mine = accs + g * kFpfhDim;
  for (int b = l; b < a.out_ld; b += kGroup) {
    float r = 0.f;
    if (b < kFpfhDim && valid > 0) {
      const double* blk = mine + (b / 11) * 11;
      double sum = 0.0;
      for (int q = 0; q < 11; ++q) sum = sum + blk[q];
      double x = mine[b];
      if (sum > 0.0) x = x * __ddiv_rn(100.0, sum);
      r = (float)(x + __ddiv_rn(100.0 * (double)own[b], (double)valid));
    }
    out[b] = r;
  }
  if (a.flags && l == 0) a.flags[(int64_t)cloud * a.n + i] = valid > 0 ? 0 : 1;
}

}  // namespace

size_t fpfh_scratch_bytes(int clouds, int n) { return (size_t)clouds * (size_t)n * kFpfhRow * sizeof(int32_t); }

bool launch_fpfh(const FpfhArgs& a, hipStream_t st) {
  if (a.n < 1 || a.clouds < 1 || a.clouds > 65535 || a.out_ld < kFpfhDim) return false;
  if (!a.pts || !a.nrm || !a.cols || !a.table || !a.desc) return false;
  if ((int64_t)a.clouds * a.n > 0x7fffffffll / kFpfhRow) return false;      // CSR offsets are int32 and index clouds x n + 1 rows
  const dim3 grid((unsigned)((a.n + kPtsPerBlock - 1) / kPtsPerBlock), (unsigned)a.clouds);
  hipLaunchKernelGGL(fpfh_spfh_kernel, grid, dim3(256), 0, st, a);
  hipLaunchKernelGGL(fpfh_gather_kernel, grid, dim3(256), 0, st, a);
  return true;
}

}  // namespace dsir
