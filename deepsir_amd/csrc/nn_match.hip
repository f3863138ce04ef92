// Fused nearest-descriptor search: for every src descriptor a_j the index of the ref descriptor b_k minimising the exact
// fp32 distance (reference network/matchnet.py:96-113 square_distance_V2 + .min(dim=2)[1] at network/model.py:558-569).  The
// reference materialises the [J,K] matrix in 6000-row chunks; here it never leaves the MFMA accumulators.
//
// The distance, its tile walk (block = 4 waves, RT row tiles of resident A fragments per wave, ref columns streaming through
// a double-buffered LDS tile) and THE RULE they obey are exact_search_body.h's, shared with nn_topk.hip.  This file's own:
// 4 running (min, argmin) updates per lane and 16x16 tile, a 16-lane reduce, and the ref range split over workgroups whose
// partial results meet in a packed 64-bit atomicMin (order-preserving distance bits << 32 | index), so ties go to the lower
// index regardless of arrival order (deterministic).  The launch geometry is search_plan.h's nn_match_plan.
#include "kernels.h"
#include "device_utils.h"
#include "exact_search_body.h"
#include "scratch.h"
#include "search_plan.h"
#include <cstdlib>

namespace dsir {

namespace {

// |x|^2 of every descriptor row: one wave per 4 rows... (16 lanes per row, float4 each)
// `init` (optional): the row's packed (distance, index) result slot, set to all ones here instead of by a separate memset
__global__ __launch_bounds__(256) void sqnorm_kernel(const float* __restrict__ x, int64_t rows, float* __restrict__ out,
                                                     unsigned long long* __restrict__ init) {
  const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int l = threadIdx.x & 15;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row < rows) v = *reinterpret_cast<const float4*>(x + row * 64 + l * 4);
  const float s = sqnorm_row16(v);
  if (row < rows && l == 0) {
    out[row] = s;
    if (init) init[row] = ~0ull;
  }
}

template <int RT>
__global__ __launch_bounds__(256) void nn_match_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                       const float* __restrict__ sa, const float* __restrict__ sb,
                                                       int J, int K, int cols_per_split, int rb_count, int splits,
                                                       unsigned long long* __restrict__ packed,
                                                       unsigned long long* __restrict__ tstamp,
                                                       const int32_t* __restrict__ gate, int gate_min,
                                                       const int32_t* __restrict__ rowlist) {
  // measurement hook: first-wave start / last-wave end on the device's constant-rate clock (what a kernel trace reports)
  if (tstamp && threadIdx.x == 0) atomicMin(tstamp, (unsigned long long)wall_clock64());
  __shared__ float Bs[2][BC * LDB];   // double-buffered ref tile
  __shared__ float sbs[2][BC];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform
  const int fr = lane & 15, fq = lane >> 4;
  // XCD-aware work mapping (speed only): every XCD gets a CONTIGUOUS range of work items, ordered (pair, ref split, row block)
  // with the row block fastest, so the workgroups that stream the same ref descriptors share one L2 instead of re-fetching
  // them through eight.
  const int id = blockIdx.x, wi = xcd_contiguous(id, gridDim.x);
  int rb = wi % rb_count;
  int split = (wi / rb_count) % splits;
  int pair = wi / (rb_count * splits);
  if (rowlist) {
    // row-list use: only the first row blocks of a pair have work.  Row block slowest, in plain dispatch order: the
    // working blocks come first and spread over all CUs (with the row block fastest every rb_count-th workgroup works,
    // and round-robin dispatch piles them onto a few CUs)
    const int ps = (int)(gridDim.x / rb_count);   // pairs * splits
    rb = id / ps;
    pair = (id % ps) / splits;
    split = id % splits;
  }
  // fallback use (nn_screen.hip), block-uniform exits before any barrier.  gate[pair] = src rows of the pair whose
  // screening failed.  Without a row list: all rows of the pairs with gate >= gate_min.  With one: only the listed rows
  // (rowlist[pair][0 .. gate)) of the pairs with gate < gate_min.
  int vJ = J;
  if (gate) {
    const int g = gate[pair];
    if (rowlist) {
      if (g >= gate_min || rb * (64 * RT) >= g) return;
      vJ = g;
    } else if (g < gate_min) {
      return;
    }
  }
  const int32_t* lst = rowlist ? rowlist + (int64_t)pair * J : nullptr;
  auto rowof = [&](int v) { return v < vJ ? (lst ? lst[v] : v) : -1; };
  const int row0 = (rb * 4 + w) * (16 * RT);

  float best[RT][4];
  int bidx[RT][4];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) { best[rt][r] = INFINITY; bidx[rt][r] = 0x7fffffff; }

  const int c_begin = split * cols_per_split;
  const int c_end = min(K, c_begin + cols_per_split);
  // the update spelled as two selects: all 4 RT of a tile stay compare + v_cndmask pairs beside packed distance arithmetic (as a
  // conditional store through the lambda's references the last one became a branch and the packing went odd: + 7 % VALU per tile)
  exact_search_stream<RT>(Bs, sbs, A + (int64_t)pair * J * 64, B + (int64_t)pair * K * 64, sa + (int64_t)pair * J, sb + (int64_t)pair * K,
                          row0, rowof, c_begin, c_end, [&](int rt, int r, float d, int col) __attribute__((always_inline)) {
                            const bool lt = d < best[rt][r];   // strict: ties stay with the lower column, NaN never wins
                            best[rt][r] = lt ? d : best[rt][r];
                            bidx[rt][r] = lt ? col : bidx[rt][r];
                          });
  // reduce over the 16 lanes that share a row; ties -> lower column
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float d = best[rt][r];
      int ix = bidx[rt][r];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const float d2 = __shfl_xor(d, o);
        const int i2 = __shfl_xor(ix, o);
        if (d2 < d || (d2 == d && i2 < ix)) { d = d2; ix = i2; }
      }
      const int row = rowof(row0 + rt * 16 + 4 * fq + r);
      if (fr == 0 && row >= 0 && ix != 0x7fffffff) {
        const unsigned long long key = ((unsigned long long)order_bits(d) << 32) | (unsigned int)ix;
        atomicMin(packed + (int64_t)pair * J + row, key);
      }
    }
  if (tstamp && threadIdx.x == 0) atomicMax(tstamp + 1, (unsigned long long)wall_clock64());
}

// A row whose distances are all NaN (non-finite descriptors) never updates its slot: index 0, like torch.min over an
// all-NaN row (the first NaN), never -1 - the consumers gather by this index.  The pair ends as identity + invalid
// flag in the Kabsch step (model.py:61-64).
__global__ void unpack_idx_kernel(const unsigned long long* __restrict__ packed, int64_t n, int32_t* __restrict__ idx) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
    idx[e] = packed_index(packed[e]);
}

}  // namespace

void launch_sqnorm(const float* x, int64_t rows, float* out, hipStream_t st) {
  hipLaunchKernelGGL(sqnorm_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, x, rows, out,
                     (unsigned long long*)nullptr);
}

size_t nn_match_scratch_bytes(int pairs, int J, int K) { return nn_match_scratch(pairs, J, K).bytes; }

// the exhaustive kernel over [pairs] x J x K with norms and the packed result slots supplied (slots preset to all ones)
static void launch_core(const float* a, const float* b, const float* sa, const float* sb, int pairs, int J, int K,
                        unsigned long long* packed, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1,
                        unsigned long long* tstamp, const int32_t* gate, int gate_min, const int32_t* rowlist = nullptr) {
  static const int force_rt = (int)tuning_int("DSIR_MATCH_RT", 0);           // tuning hooks
  static const int force_splits = (int)tuning_int("DSIR_MATCH_SPLITS", 0);
  const ExactPlan pl = nn_match_plan(pairs, J, K, rowlist ? gate_min : 0, force_rt, force_splits);   // a row list holds fewer than gate_min rows
  const dim3 grid((unsigned)pl.blocks(pairs));
  if (ev0) hipEventRecord(ev0, st);
#define DSIR_LAUNCH_MATCH(RTV)                                                                                                          \
  hipLaunchKernelGGL((nn_match_kernel<RTV>), grid, dim3(256), 0, st, a, b, sa, sb, J, K, pl.cols_per_split, pl.rb_count, pl.splits, packed, \
                     tstamp, gate, gate_min, rowlist)
  if (pl.rt == 4)      DSIR_LAUNCH_MATCH(4);
  else if (pl.rt == 2) DSIR_LAUNCH_MATCH(2);
  else                 DSIR_LAUNCH_MATCH(1);
#undef DSIR_LAUNCH_MATCH
  if (ev1) hipEventRecord(ev1, st);
}

void nn_match_scratch_layout(void* scratch, int pairs, int J, int K, float** sa, unsigned long long** packed) {
  const ExactScratch L = nn_match_scratch(pairs, J, K);
  *sa = at<float>(scratch, L.sa);
  *packed = at<unsigned long long>(scratch, L.tail);
}

void launch_nn_match_ws(const float* a, const float* b, int pairs, int J, int K, int32_t* idx, void* scratch,
                        hipStream_t st, hipEvent_t ev0, hipEvent_t ev1, bool ref_norms_cached, unsigned long long* tstamp,
                        bool src_norms_ready) {
  const ExactScratch L = nn_match_scratch(pairs, J, K);
  float *sa = at<float>(scratch, L.sa), *sb = at<float>(scratch, L.sb);
  unsigned long long* packed = at<unsigned long long>(scratch, L.tail);
  const int64_t ra = (int64_t)pairs * J, rb = (int64_t)pairs * K;
  if (!src_norms_ready) hipLaunchKernelGGL(sqnorm_kernel, dim3((unsigned)((ra + 15) / 16)), dim3(256), 0, st, a, ra, sa, packed);
  // the ref descriptors are loop invariant in dsir_register: their norms stay in the (persistent) scratch
  if (!ref_norms_cached) hipLaunchKernelGGL(sqnorm_kernel, dim3((unsigned)((rb + 15) / 16)), dim3(256), 0, st, b, rb, sb, nullptr);
  launch_core(a, b, sa, sb, pairs, J, K, packed, st, ev0, ev1, tstamp, nullptr, 0);
  hipLaunchKernelGGL(unpack_idx_kernel, dim3(256), dim3(256), 0, st, packed, ra, idx);
}

// Exhaustive search of what the screening (nn_screen.hip) could not decide: all rows of the pairs with
// gate[pair] >= gate_min, and the rows rowlist[pair][0 .. gate[pair]) of the other pairs (workgroups without work exit at
// once).  Results stay in `packed` (low word = index), whose slots the caller has preset to all ones.
void launch_nn_match_gated(const float* a, const float* b, const float* sa, const float* sb, int pairs, int J, int K,
                           unsigned long long* packed, const int32_t* gate, int gate_min, const int32_t* rowlist,
                           hipStream_t st) {
  launch_core(a, b, sa, sb, pairs, J, K, packed, st, nullptr, nullptr, nullptr, gate, gate_min, nullptr);
  launch_core(a, b, sa, sb, pairs, J, K, packed, st, nullptr, nullptr, nullptr, gate, gate_min, rowlist);
}

}  // namespace dsir
