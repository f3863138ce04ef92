// Top-k descriptor search: for every src descriptor a_j its k nearest ref descriptors, with distances, and the
// correspondence lists built on them (ratio test, k candidates per src row).  The [J, K] matrix never exists.
//
// THE RULE (restated in DESIGN.md section 8 and on the host in deepsir_amd/match.py):
//   distance   d(j, c): THE RULE of exact_search_body.h, by construction dsir_nn_match's - both kernels get their distances from the
//              same exact_search_stream; the norms from launch_sqnorm (nn_match.hip's sqnorm_kernel).
//   key        order_bits(d) << 32 | c, unsigned 64 bit - the packed value nn_match_kernel minimises.
//   answer     a row's k smallest keys, ascending.  An integer rule: ties go to the lower column, nothing depends on the arrival
//              order of workgroups (no atomics anywhere; every partial list has one writer).  Rank 0 is dsir_nn_match's result.
//   non-finite as in nn_match_kernel a column enters a list only while d < +inf holds (its `d < best` from best = +inf): a NaN or
//              +inf distance never does.  A rank without an entry is index -1, distance +inf - ranks beyond K (k > K) among them -
//              except rank 0, whose index is 0 as packed_index() gives for a slot nothing ever won.
//   dist       the fp32 distance recovered from the key (unorder_bits), no second evaluation.
//   ratio test r2 = fp32(ratio * ratio) rounded once on the host; row j keeps its rank-0 match iff rank 1 is missing or
//              max(d0, 0) < r2 * max(d1, 0): one fp32 multiply, a strict comparison (d0 == d1 == 0 rejects).
//   candidates (j, c) for every rank < k of row j that has an entry; under `mutual` kept iff j is among the k smallest keys of
//              column c in the ref -> src search; output in ascending j, then ascending rank; rows beyond counts[p] are -1.
//
// nn_topk_kernel<KK, RT> walks the tiles as nn_match_kernel does (exact_search_stream: block = 4 waves, wave w owns RT row tiles),
// under the same XCD-aware work mapping with the column range split over workgroups (search_plan.h's nn_topk_plan).  Per 16x16 tile
// a lane holds 4 rows x one column; per row it keeps a sorted list of KK (distance, column) entries in registers: one comparison
// against the KK-th entry guards an unrolled compare-exchange ladder (static indices only).  A lane meets its columns in ascending order, so the strict float comparison nn_match_kernel uses puts an equal distance
// behind the earlier (lower) column: the lane's list is in key order.  (A distance is never -0: |a|^2 and |b|^2 are sums of squares,
// +0 at the least, and x + +0 is -0 only for x = -0, which (-2 dot) + |a|^2 cannot be.)  At the end of the column range the 16
// lanes that share a row merge their lists as keys in a 4-step butterfly (merge_topk: a bitonic merge of two sorted lists, static
// indices), and lane 0 of the row stores the result as the row's partial of this column split, u64 [P][splits][J][KK].
// nn_topk_merge_kernel: one lane per row merges the splits' partials with the same merge_topk and writes idx / dist.
#include "kernels.h"
#include "device_utils.h"
#include "exact_search_body.h"
#include "scratch.h"
#include "search_plan.h"

namespace dsir {

namespace {

constexpr unsigned long long kEmpty = ~0ull;

__device__ __forceinline__ void cswap(unsigned long long& a, unsigned long long& b) {
  const unsigned long long lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo; b = hi;
}

// a, b ascending lists of KK keys -> a = the KK smallest of both, ascending.  min(a[i], b[KK-1-i]) holds exactly those and is
// bitonic; log2(KK) half-cleaner stages sort it.  Keys are distinct (the column is part of the key) except kEmpty.
template <int KK>
__device__ __forceinline__ void merge_topk(unsigned long long (&a)[KK], const unsigned long long (&b)[KK]) {
#pragma unroll
  for (int i = 0; i < KK; ++i) a[i] = a[i] < b[KK - 1 - i] ? a[i] : b[KK - 1 - i];
#pragma unroll
  for (int h = KK / 2; h >= 1; h >>= 1)
#pragma unroll
    for (int i = 0; i < KK; ++i)
      if ((i & h) == 0) cswap(a[i], a[i + h]);
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o) {
  const unsigned int lo = __shfl_xor((unsigned int)(v & 0xffffffffull), o);
  const unsigned int hi = __shfl_xor((unsigned int)(v >> 32), o);
  return ((unsigned long long)hi << 32) | lo;
}

template <int KK, int RT>
__global__ __launch_bounds__(256) void nn_topk_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                      const float* __restrict__ sa, const float* __restrict__ sb, int J, int K,
                                                      int cols_per_split, int rb_count, int splits,
                                                      unsigned long long* __restrict__ partial) {
  __shared__ float Bs[2][BC * LDB];   // double-buffered ref tile
  __shared__ float sbs[2][BC];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  // XCD-aware work mapping (speed only), as in nn_match_kernel: (pair, ref split, row block), the row block fastest
  const int wi = xcd_contiguous(blockIdx.x, gridDim.x);
  const int rb = wi % rb_count;
  const int split = (wi / rb_count) % splits;
  const int pair = wi / (rb_count * splits);
  const int row0 = (rb * 4 + w) * (16 * RT);

  // the lists: ascending (distance, column), an empty entry is (+inf, -1)
  float ld[RT][4][KK];
  int lc[RT][4][KK];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int i = 0; i < KK; ++i) { ld[rt][r][i] = INFINITY; lc[rt][r][i] = -1; }

  const int c_begin = split * cols_per_split;
  const int c_end = min(K, c_begin + cols_per_split);
  exact_search_stream<RT>(
      Bs, sbs, A + (int64_t)pair * J * 64, B + (int64_t)pair * K * 64, sa + (int64_t)pair * J, sb + (int64_t)pair * K, row0,
      [&](int v) { return v < J ? v : -1; }, c_begin, c_end, [&](int rt, int r, float d, int col) __attribute__((always_inline)) {
        if (d < ld[rt][r][KK - 1]) {   // the guard: almost every candidate fails it after the first few tiles
          ld[rt][r][KK - 1] = d; lc[rt][r][KK - 1] = col;
#pragma unroll
          for (int i = KK - 1; i >= 1; --i) {
            const bool up = ld[rt][r][i] < ld[rt][r][i - 1];   // strict: an equal distance stays behind the lower column
            const float d0 = ld[rt][r][i - 1], d1 = ld[rt][r][i];
            const int c0_ = lc[rt][r][i - 1], c1_ = lc[rt][r][i];
            ld[rt][r][i - 1] = up ? d1 : d0; ld[rt][r][i] = up ? d0 : d1;
            lc[rt][r][i - 1] = up ? c1_ : c0_; lc[rt][r][i] = up ? c0_ : c1_;
          }
        }
      });
  // the 16 lanes that share a row (same fq): butterfly over fr, every lane ends with the row's merged list
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      unsigned long long key[KK], other[KK];
#pragma unroll
      for (int i = 0; i < KK; ++i)
        key[i] = lc[rt][r][i] < 0 ? kEmpty : ((unsigned long long)order_bits(ld[rt][r][i]) << 32) | (unsigned int)lc[rt][r][i];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
#pragma unroll
        for (int i = 0; i < KK; ++i) other[i] = shfl_xor_u64(key[i], o);
        merge_topk<KK>(key, other);
      }
      const int row = row0 + rt * 16 + 4 * fq + r;
      if (fr == 0 && row < J) {
        unsigned long long* dst = partial + (((int64_t)pair * splits + split) * J + row) * KK;
#pragma unroll
        for (int i = 0; i < KK; ++i) dst[i] = key[i];
      }
    }
}

// one lane per row: the splits' sorted partials -> the row's k smallest keys -> idx [rows][k], dist [rows][k] (optional)
template <int KK>
__global__ __launch_bounds__(256) void nn_topk_merge_kernel(const unsigned long long* __restrict__ partial, int pairs, int J, int splits,
                                                            int k, int32_t* __restrict__ idx, float* __restrict__ dist) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)pairs * J) return;
  const int pair = (int)(e / J), row = (int)(e % J);
  unsigned long long key[KK], other[KK];
  const unsigned long long* src = partial + ((int64_t)pair * splits * J + row) * KK;
#pragma unroll
  for (int i = 0; i < KK; ++i) key[i] = src[i];
  for (int s = 1; s < splits; ++s) {
    const unsigned long long* p = src + (int64_t)s * J * KK;
#pragma unroll
    for (int i = 0; i < KK; ++i) other[i] = p[i];
    merge_topk<KK>(key, other);
  }
#pragma unroll
  for (int i = 0; i < KK; ++i)
    if (i < k) {
      const bool empty = key[i] == kEmpty;
      idx[e * k + i] = empty ? (i == 0 ? 0 : -1) : (int32_t)(key[i] & 0xffffffffull);
      if (dist) dist[e * k + i] = empty ? INFINITY : unorder_bits((unsigned int)(key[i] >> 32));
    }
}

// Correspondences from the lists (the rule in the file's header): one workgroup per pair, entries e = j k + rank in order, ballot +
// LDS scan, no atomics.  iab / dab [P][J][sa], iba [P][K][sb_] (mutual only); ratio test (r2 > 0) with k == 1 and sa >= 2.
__global__ __launch_bounds__(256) void corr_topk_compact_kernel(const int32_t* __restrict__ iab, const float* __restrict__ dab, int sa,
                                                                const int32_t* __restrict__ iba, int sb_, int J, int K, int mutual,
                                                                int k, float r2, int32_t* __restrict__ corr,
                                                                int32_t* __restrict__ counts, float* __restrict__ corr_dist) {
  __shared__ int wt[4];
  const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int32_t* Ia = iab + (int64_t)pair * J * sa;
  const float* Da = dab + (int64_t)pair * J * sa;
  const int32_t* Ib = iba + (int64_t)pair * K * sb_;
  const int64_t M = (int64_t)J * k;
  int32_t* out = corr + (int64_t)pair * M * 2;
  float* outd = corr_dist ? corr_dist + (int64_t)pair * M : nullptr;
  int base = 0;
  for (int64_t e0 = 0; e0 < M; e0 += 256) {
    const int64_t e = e0 + tid;
    int j = 0, c = -1;
    float d = 0.f;
    bool keep = false;
    if (e < M) {
      j = (int)(e / k);
      const int rank = (int)(e % k);
      c = Ia[(int64_t)j * sa + rank];
      d = Da[(int64_t)j * sa + rank];
      keep = c >= 0 && c < K;
      if (keep && r2 > 0.f && Ia[(int64_t)j * sa + 1] >= 0) keep = fmaxf(d, 0.f) < __fmul_rn(r2, fmaxf(Da[(int64_t)j * sa + 1], 0.f));
      if (keep && mutual) {
        bool back = false;
        for (int i = 0; i < k; ++i) back = back || Ib[(int64_t)c * sb_ + i] == j;
        keep = back;
      }
    }
    const unsigned long long bal = __ballot(keep);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wt[w] = __popcll(bal);
    __syncthreads();
    int off = base;
    for (int ww = 0; ww < w; ++ww) off += wt[ww];
    if (keep) {
      out[(int64_t)(off + before) * 2] = j; out[(int64_t)(off + before) * 2 + 1] = c;
      if (outd) outd[off + before] = d;
    }
    base += wt[0] + wt[1] + wt[2] + wt[3];
    __syncthreads();
  }
  for (int64_t i = base + tid; i < M; i += 256) {
    out[i * 2] = -1; out[i * 2 + 1] = -1;
    if (outd) outd[i] = INFINITY;
  }
  if (tid == 0) counts[pair] = base;
}

// one kernel per list length KK: the main kernel at rt row tiles per wave, then the merge of the splits' partials
template <int KK>
void launch_kk(const float* a, const float* b, const float* sa, const float* sb, int pairs, int J, int K, int k, const ExactPlan& pl,
               unsigned long long* partial, int32_t* idx, float* dist, hipStream_t st) {
  const dim3 grid((unsigned)pl.blocks(pairs));
  constexpr int RT2 = KK <= 4 ? 2 : 1;   // nn_topk_plan takes two row tiles only where the lists fit beside them
  const auto kernel = pl.rt == 2 ? nn_topk_kernel<KK, RT2> : nn_topk_kernel<KK, 1>;
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, a, b, sa, sb, J, K, pl.cols_per_split, pl.rb_count, pl.splits, partial);
  const unsigned blocks = (unsigned)(((int64_t)pairs * J + 255) / 256);
  hipLaunchKernelGGL((nn_topk_merge_kernel<KK>), dim3(blocks), dim3(256), 0, st, partial, pairs, J, pl.splits, k, idx, dist);
}

}  // namespace

int nn_topk_splits(int pairs, int J, int K, int k) { return nn_topk_plan(pairs, J, K, topk_kk(k)).splits; }

size_t nn_topk_scratch_bytes(int pairs, int J, int K, int k) { return nn_topk_scratch(pairs, J, K, k).bytes; }

void launch_nn_topk(const float* a, const float* b, int pairs, int J, int K, int k, int32_t* idx, float* dist, void* scratch,
                    hipStream_t st) {
  const int kk = topk_kk(k);
  const ExactPlan pl = nn_topk_plan(pairs, J, K, kk);
  const ExactScratch L = nn_topk_scratch(pairs, J, K, k);
  float *sa = at<float>(scratch, L.sa), *sb = at<float>(scratch, L.sb);
  unsigned long long* partial = at<unsigned long long>(scratch, L.tail);
  launch_sqnorm(a, (int64_t)pairs * J, sa, st);
  launch_sqnorm(b, (int64_t)pairs * K, sb, st);
  if (kk == 2)      launch_kk<2>(a, b, sa, sb, pairs, J, K, k, pl, partial, idx, dist, st);
  else if (kk == 4) launch_kk<4>(a, b, sa, sb, pairs, J, K, k, pl, partial, idx, dist, st);
  else              launch_kk<8>(a, b, sa, sb, pairs, J, K, k, pl, partial, idx, dist, st);
}

void launch_corr_topk_compact(const int32_t* iab, const float* dab, int stride_ab, const int32_t* iba, int stride_ba, int pairs, int J,
                              int K, int mutual, int k, float r2, int32_t* corr, int32_t* counts, float* corr_dist, hipStream_t st) {
  hipLaunchKernelGGL(corr_topk_compact_kernel, dim3(pairs), dim3(256), 0, st, iab, dab, stride_ab, iba ? iba : iab, stride_ba, J, K,
                     iba ? mutual : 0, k, r2, corr, counts, corr_dist);
}

}  // namespace dsir
