// Spatial-consensus pose from correspondences: the fourth pose stage, beside ransac.hip, icp.hip and finetune.hip.  Neither the
// reference nor open3d has it (the idea is the second-order spatial compatibility of SC2-PCR, Chen et al., CVPR 2022), so parity is
// UNPINNED: the engine owns the rule, states it here once, and deepsir_amd/consensus.py restates it on the host for the tests.
// No sampling, no seed, no random number: a pose is a function of the inputs alone.
//
// THE RULE.  Front (step 1) and tail (step 7) are those of every pose-from-correspondences stage: the head of pose_corr.hip states
// them.  Per pair p:
//   1 gather: the shared front: clamp with bit 2 of invalid, park non-finite rows and rows >= count at s = 0, q = FLT_MAX.  A parked
//     row is compatible with nothing.
//   2 first-order compatibility, i != j, neither parked:   C[i][j] = 1  iff  | |s_i - s_j| - |q_i - q_j| | < compat_dist
//     in float64 on the fp32 coordinates, |d| = sqrt((dx dx + dy dy) + dz dz), every operation rounded once, no contraction (the
//     convention of fpfh.hip); compat_dist is the fp32 argument widened.  d -> -d changes no square: C is symmetric by construction,
//     its diagonal is 0.  C is a bit matrix: row i is W = ceil(M / 64) words of 64 bits, bit j % 64 of word j / 64 is C[i][j].
//   3 second-order score, integers:   S2[i][j] = C[i][j] popcount(row_i & row_j),   score[i] = sum_j S2[i][j]   (int32:
//     score < M^2 <= DSIR_CONSENSUS_MAX_M^2 < 2^31).
//   4 seeds: the `seeds` rows with the largest (score, lower index), in that order; fewer if fewer have score > 0.  Seed rank r.
//   5 members of seed i: i itself and the members - 1 rows j with the largest (S2[i][j], lower j) among those with S2[i][j] > 0,
//     taken in ascending index.  Fewer than 3 members: the seed is invalid.
//   6 fit: unweighted Kabsch of the members in member order - fit_rows64 of pose_corr.h, the fit of a RANSAC hypothesis; T rounded
//     to fp32 once.  A non-finite T is invalid.
//   7 the seed poses are scored, picked (largest inlier count under max_dist, ties to the lower seed rank), refitted refine_iters
//     times on all inliers and finished by the shared tail (launch_pose_tail), with H = seeds.
//   output: T_out, stats {fitness, inlier RMSE, winning seed rank or -1, valid seeds, inliers}.  No valid seed: T_out = T_init
//     (identity if NULL), stats {0, 0, -1, 0, 0} - not an error.
//
// KERNELS.
//   consensus_compat_kernel: a workgroup owns 64 rows, staged in LDS, and walks column blocks of 64.  A lane holds one column point
//     in registers, reads the row point from LDS (every lane the same address: a broadcast), and the wave ballot IS the 64-bit word;
//     lane 0 stores it with an ordinary store.  Every entry is computed: no mirrored store.
//   consensus_score_kernel (the hot path, M^2 W AND + popcount): a workgroup owns 256 rows i, one per lane, and one chunk of
//     CW = 8 words; the lane keeps its row's chunk in 16 registers.  Blocks of 64 rows j (their chunk: 4 KiB) go through LDS, the
//     next block's global loads issued before the current one is consumed; all lanes read the SAME j row (ds_read_b128 broadcasts).
//     C[i][j] gates the sum per lane; a wave whose 64 rows have no set bit in the block's word skips it (wave-uniform).  Integer sums,
//     one integer atomicAdd per row and chunk: exact, so order cannot matter.
//   seed selection: hipCUB segmented radix sort (descending) of score << 32 | (0xFFFFFFFF - i), as select.hip sorts.
//   consensus_members_kernel: one workgroup per (pair, seed rank).  The seed's S2 row goes into LDS as uint16 (S2 < M <=
//     DSIR_CONSENSUS_MAX_M < 2^16); the (members - 1)-th largest value is found by bisection over the integer range with exact
//     counts; rows above it are taken, ties at it in ascending index (ballot + prefix, no atomics); one lane fits in float64.
#include <hipcub/hipcub.hpp>

#include "kernels.h"
#include "device_utils.h"
#include "pose_corr.h"
#include "seg_sort.h"
#include "dsir.h"

namespace dsir {

namespace {

constexpr int CT = 64;    // rows per compat workgroup
constexpr int SI = 256;   // rows i per scoring workgroup (one per lane)
constexpr int CW = 8;     // words of a row per scoring workgroup
constexpr int SJ = 64;    // rows j per LDS block: one word of C

__device__ __forceinline__ double len64(float ax, float ay, float az, float bx, float by, float bz) {
  const double dx = (double)ax - (double)bx, dy = (double)ay - (double)by, dz = (double)az - (double)bz;
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

// bits [P][M][W].  grid (row tiles of CT, column slices, pairs); a slice is wps words
__global__ __launch_bounds__(256) void consensus_compat_kernel(const float* __restrict__ cs, const float* __restrict__ cq, int M, int W,
                                                               int wps, double compat, unsigned long long* __restrict__ bits) {
  __shared__ float rs[CT][3], rq[CT][3];
  __shared__ int rlive[CT];
  const int pair = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* S = cs + (int64_t)pair * M * 3;
  const float* Q = cq + (int64_t)pair * M * 3;
  const int i0 = blockIdx.x * CT;
  if (tid < CT) {
    const int i = i0 + tid;
    float s[3] = {0.f, 0.f, 0.f}, q[3] = {FLT_MAX, FLT_MAX, FLT_MAX};
    if (i < M)
      for (int k = 0; k < 3; ++k) { s[k] = S[(int64_t)i * 3 + k]; q[k] = Q[(int64_t)i * 3 + k]; }
    for (int k = 0; k < 3; ++k) { rs[tid][k] = s[k]; rq[tid][k] = q[k]; }
    rlive[tid] = (i < M && !parked(s, q)) ? 1 : 0;
  }
  __syncthreads();
  const int w_end = min(W, (int)(blockIdx.y + 1) * wps);
  for (int w = blockIdx.y * wps; w < w_end; ++w) {
    const int j = w * 64 + lane;
    float s[3] = {0.f, 0.f, 0.f}, q[3] = {FLT_MAX, FLT_MAX, FLT_MAX};
    if (j < M)
      for (int k = 0; k < 3; ++k) { s[k] = S[(int64_t)j * 3 + k]; q[k] = Q[(int64_t)j * 3 + k]; }
    const bool jlive = j < M && !parked(s, q);
    for (int r = wave * (CT / 4); r < (wave + 1) * (CT / 4); ++r) {
      const int i = i0 + r;
      if (i >= M) break;                                        // wave-uniform
      bool c = false;
      if (rlive[r] && jlive && i != j) {
        const double ls = len64(rs[r][0], rs[r][1], rs[r][2], s[0], s[1], s[2]);
        const double lq = len64(rq[r][0], rq[r][1], rq[r][2], q[0], q[1], q[2]);
        c = fabs(ls - lq) < compat;
      }
      const unsigned long long word = __ballot(c);
      if (lane == 0) bits[((int64_t)pair * M + i) * W + w] = word;
    }
  }
}

// score [P][M] (zeroed by the caller).  grid (row blocks of SI, chunks of CW words, pairs)
__global__ __launch_bounds__(SI) void consensus_score_kernel(const unsigned long long* __restrict__ bits, int M, int W,
                                                             int32_t* __restrict__ score) {
  __shared__ __attribute__((aligned(16))) unsigned long long sj[SJ][CW];
  const int pair = blockIdx.z, tid = threadIdx.x;
  const unsigned long long* B = bits + (int64_t)pair * M * W;
  const int i = blockIdx.x * SI + tid;
  const int w0 = blockIdx.y * CW;
  unsigned long long ri[CW];
#pragma unroll
  for (int k = 0; k < CW; ++k) ri[k] = (i < M && w0 + k < W) ? B[(int64_t)i * W + w0 + k] : 0ull;
  // staging: thread t brings words 2 (t & 3), 2 (t & 3) + 1 of row t >> 2 of the block
  const int lr = tid >> 2, lw = (tid & 3) * 2;
  unsigned long long n0 = 0ull, n1 = 0ull;
  if (lr < M) {
    if (w0 + lw < W) n0 = B[(int64_t)lr * W + w0 + lw];
    if (w0 + lw + 1 < W) n1 = B[(int64_t)lr * W + w0 + lw + 1];
  }
  int acc = 0;
  for (int jb = 0; jb < W; ++jb) {                              // block jb holds rows j = 64 jb .. 64 jb + 63: word jb of row i gates them
    sj[lr][lw] = n0; sj[lr][lw + 1] = n1;
    __syncthreads();
    const int nr = (jb + 1) * SJ + lr;                          // the next block's loads fly while this one is consumed
    n0 = 0ull; n1 = 0ull;
    if (jb + 1 < W && nr < M) {
      if (w0 + lw < W) n0 = B[(int64_t)nr * W + w0 + lw];
      if (w0 + lw + 1 < W) n1 = B[(int64_t)nr * W + w0 + lw + 1];
    }
    const unsigned long long cw = i < M ? B[(int64_t)i * W + jb] : 0ull;
    if (__ballot(cw != 0ull) != 0ull) {                         // wave-uniform skip
#pragma unroll 4
      for (int j = 0; j < SJ; ++j) {
        const uint4* row = reinterpret_cast<const uint4*>(&sj[j][0]);
        int p = 0;
#pragma unroll
        for (int k = 0; k < CW / 2; ++k) {
          const uint4 v = row[k];
          p += __popc(v.x & (uint32_t)ri[2 * k]) + __popc(v.y & (uint32_t)(ri[2 * k] >> 32));
          p += __popc(v.z & (uint32_t)ri[2 * k + 1]) + __popc(v.w & (uint32_t)(ri[2 * k + 1] >> 32));
        }
        acc += ((cw >> j) & 1ull) ? p : 0;
      }
    }
    __syncthreads();
  }
  if (i < M && acc) atomicAdd(score + (int64_t)pair * M + i, acc);
}

__global__ void consensus_key_kernel(const int32_t* __restrict__ score, int64_t total, int M, unsigned long long* __restrict__ key) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x)
    key[e] = ((unsigned long long)(uint32_t)score[e] << 32) | (0xFFFFFFFFu - (uint32_t)(e % M));
}

// seed [P][seeds]: row index of seed rank r, or -1
__global__ void consensus_seed_kernel(const unsigned long long* __restrict__ sorted, int pairs, int M, int seeds, int32_t* __restrict__ seed) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= pairs * seeds) return;
  const int pair = e / seeds, r = e % seeds;
  int v = -1;
  if (r < M) {
    const unsigned long long k = sorted[(int64_t)pair * M + r];
    if ((k >> 32) != 0ull) v = (int)(0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFull));
  }
  seed[e] = v;
}

// One workgroup per (seed rank, pair): the seed's S2 row, its members, their fit.  hyp_T [P][seeds][12], hyp_valid [P][seeds];
// members_out (optional) [P][seeds][members], -1 padded.  Dynamic LDS: W words of the seed's row, then M uint16 of S2.
__global__ __launch_bounds__(256) void consensus_members_kernel(const float* __restrict__ cs, const float* __restrict__ cq,
                                                                const unsigned long long* __restrict__ bits,
                                                                const int32_t* __restrict__ seed, int M, int W, int seeds, int members,
                                                                float* __restrict__ hyp_T, int32_t* __restrict__ hyp_valid,
                                                                int32_t* __restrict__ members_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
  __shared__ int wt[8];
  __shared__ int mem[DSIR_CONSENSUS_MAX_MEMBERS];
  unsigned long long* row = reinterpret_cast<unsigned long long*>(dyn);
  unsigned short* s2 = reinterpret_cast<unsigned short*>(dyn + (size_t)W * 8);
  const int r = blockIdx.x, pair = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t slot = (int64_t)pair * seeds + r;
  const int i = seed[slot];
  const unsigned long long* B = bits + (int64_t)pair * M * W;
  int n = 0;
  if (i >= 0) {                                                 // block-uniform
    for (int w = tid; w < W; w += 256) row[w] = B[(int64_t)i * W + w];
    __syncthreads();
    for (int j = tid; j < M; j += 256) {
      int v = 0;
      if ((row[j >> 6] >> (j & 63)) & 1ull)
        for (int w = 0; w < W; ++w) v += __popcll(row[w] & B[(int64_t)j * W + w]);
      s2[j] = (unsigned short)v;
    }
    __syncthreads();
    // the largest t >= 1 with #{S2 >= t} >= want; t = 1 if there is none (then every row with S2 > 0 is taken)
    const int want = members - 1;
    int lo = 1, hi = M;                                         // #{S2 >= lo} >= want or lo == 1;  #{S2 >= hi} = 0 < want
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      int c = 0;
      for (int j = tid; j < M; j += 256) c += s2[j] >= mid ? 1 : 0;
      for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
      __syncthreads();                                          // the previous round's reads of wt are done
      if (lane == 0) wt[wave] = c;
      __syncthreads();
      c = wt[0] + wt[1] + wt[2] + wt[3];
      if (c >= want) lo = mid; else hi = mid;                   // block-uniform
    }
    const int t = lo;
    int above = 0;
    for (int j = tid; j < M; j += 256) above += s2[j] > t ? 1 : 0;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o);
    if (lane == 0) wt[wave] = above;
    __syncthreads();
    above = wt[0] + wt[1] + wt[2] + wt[3];
    const int need = want - above;                              // ties at t to take, in ascending index (>= 0: #{S2 > t} < want)
    int tie_base = 0, out_base = 0;
    for (int j0 = 0; j0 < M; j0 += 256) {
      const int j = j0 + tid;
      const int v = j < M ? (int)s2[j] : 0;
      const bool tie = v == t && v > 0;
      const unsigned long long tb = __ballot(tie);
      __syncthreads();
      if (lane == 0) wt[wave] = __popcll(tb);
      __syncthreads();
      int trank = tie_base + __popcll(tb & ((1ull << lane) - 1ull));
      for (int ww = 0; ww < wave; ++ww) trank += wt[ww];
      tie_base += wt[0] + wt[1] + wt[2] + wt[3];
      const bool take = j < M && (j == i || v > t || (tie && trank < need));
      const unsigned long long kb = __ballot(take);
      if (lane == 0) wt[4 + wave] = __popcll(kb);
      __syncthreads();
      int pos = out_base + __popcll(kb & ((1ull << lane) - 1ull));
      for (int ww = 0; ww < wave; ++ww) pos += wt[4 + ww];
      if (take && pos < DSIR_CONSENSUS_MAX_MEMBERS) mem[pos] = j;
      out_base += wt[4] + wt[5] + wt[6] + wt[7];
    }
    __syncthreads();
    n = min(out_base, members);                                 // out_base <= members by construction
  }
  if (members_out)
    for (int k = tid; k < members; k += 256) members_out[slot * members + k] = k < n ? mem[k] : -1;
  if (tid == 0) {
    float T[12];
    for (int k = 0; k < 12; ++k) T[k] = 0.f;
    bool ok = n >= 3;
    if (ok) {
      const float* S = cs + (int64_t)pair * M * 3;
      const float* Q = cq + (int64_t)pair * M * 3;
      fit_rows64(n, [&](int k) { return S + (int64_t)mem[k] * 3; }, [&](int k) { return Q + (int64_t)mem[k] * 3; }, T);
      for (int k = 0; k < 12; ++k) ok = ok && isfinite(T[k]);
    }
    for (int k = 0; k < 12; ++k) hyp_T[slot * 12 + k] = T[k];
    hyp_valid[slot] = ok ? 1 : 0;
  }
}

}  // namespace

size_t consensus_scratch_bytes(int pairs, int M, int seeds, int refine_iters) {
  return ConsensusLayout(pairs, M, seeds, refine_iters, seg_sort_keys_desc_tmp_bytes((int64_t)pairs * M, pairs)).bytes;
}

int launch_consensus(const ConsensusArgs& a, void* scratch, hipStream_t st) {
  const CorrProblem& p = a.p;
  const int P = p.pairs, M = p.M, H = a.seeds, W = (M + 63) / 64;
  if (!pose_corr_shape_ok(P, M)) return 1;
  size_t tmp = seg_sort_keys_desc_tmp_bytes((int64_t)P * M, P);
  const ConsensusLayout lay(P, M, H, p.refine_iters, tmp);
  const PoseParts s(scratch, lay.pose);
  const CandSet hyp(scratch, lay.hyp, H);
  unsigned long long *bits = at<unsigned long long>(scratch, lay.bits), *k0 = at<unsigned long long>(scratch, lay.k0),
                     *k1 = at<unsigned long long>(scratch, lay.k1);
  int32_t *score = at<int32_t>(scratch, lay.score), *seed = at<int32_t>(scratch, lay.seed);
  int* seg = at<int>(scratch, lay.seg);
  const float cd = a.compat_dist > 0.f ? a.compat_dist : p.max_dist;

  launch_pose_front(p, s, st);
  {
    const int tiles = (M + CT - 1) / CT;
    int slices = (int)((512 + (int64_t)tiles * P - 1) / ((int64_t)tiles * P));
    slices = slices < 1 ? 1 : (slices > W ? W : slices);
    const int wps = (W + slices - 1) / slices;
    hipLaunchKernelGGL(consensus_compat_kernel, dim3(tiles, (W + wps - 1) / wps, P), dim3(256), 0, st, s.cs, s.cq, M, W, wps, (double)cd, bits);
  }
  hipMemsetAsync(score, 0, (size_t)P * M * 4, st);
  hipLaunchKernelGGL(consensus_score_kernel, dim3((M + SI - 1) / SI, (W + CW - 1) / CW, P), dim3(SI), 0, st, bits, M, W, score);
  const int64_t total = (int64_t)P * M;
  const int kg = (int)((total + 255) / 256 > 65535 ? 65535 : (total + 255) / 256);
  hipLaunchKernelGGL(consensus_key_kernel, dim3(kg), dim3(256), 0, st, score, total, M, k0);
  launch_seg_offsets(seg, P, M, st);
  if (hipcub::DeviceSegmentedRadixSort::SortKeysDescending(at<char>(scratch, lay.tmp), tmp, k0, k1, (int)total, P, seg, seg + 1, 0, 64, st) !=
      hipSuccess)
    return 2;
  hipLaunchKernelGGL(consensus_seed_kernel, dim3((P * H + 255) / 256), dim3(256), 0, st, k1, P, M, H, seed);
  const size_t lds = (size_t)W * 8 + (size_t)M * 2;
  hipLaunchKernelGGL(consensus_members_kernel, dim3(H, P), dim3(256), lds, st, s.cs, s.cq, bits, seed, M, W, H, a.members, hyp.T, hyp.valid,
                     a.diag_members);
  launch_pose_tail(p, s, hyp, st);
  if (a.diag_bits) hipMemcpyAsync(a.diag_bits, bits, (size_t)P * M * W * 8, hipMemcpyDeviceToDevice, st);
  if (a.diag_score) hipMemcpyAsync(a.diag_score, score, (size_t)P * M * 4, hipMemcpyDeviceToDevice, st);
  if (a.diag_seed) hipMemcpyAsync(a.diag_seed, seed, (size_t)P * H * 4, hipMemcpyDeviceToDevice, st);
  copy_candidates(hyp, P, a.diag_T, a.diag_valid, a.diag_count, st);
  return 0;
}

}  // namespace dsir
