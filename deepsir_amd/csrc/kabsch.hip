// Weighted Kabsch pose solve, entirely on device (reference network/model.py:22-66
// compute_rigid_transform_2 — which round-trips to the CPU for a float64 LAPACK
// SVD every iteration — plus the SE(3) bookkeeping of forward_align_4,
// model.py:586-595, common/math/se3_torch.py:28-77).
//
// One 1024-thread block per pair.  Three passes over the (L2-resident) points:
//   S = sum |w|;  c_s = sum s*wn, c_t = sum t*wn (wn = w/(S+1e-16));
//   H = sum (s-c_s) ((t-c_t)*wn)^T.
// Every product is rounded to fp32 exactly as the reference's element-wise ops
// produce it; the sums are accumulated in fp64 (wave shuffles + LDS), i.e. the
// exact value the reference's fp32 reductions approximate in some order.
// Thread 0 then runs a one-sided Jacobi SVD of H in fp64, R = V diag(1,1,d) U^T
// with d = sign(det(V U^T)), casts R to fp32 and forms t = -R c_s + c_t in fp32
// (model.py:53,57).  Non-finite H => identity + invalid flag (model.py:61-64).
// The same launch applies the transform to the src points, gathers the matched
// ref points and composes the cumulative transform.
//
// Each formula is written once: the per-point functions add_abs_weight /
// add_centroid_terms / add_covariance_terms hold the roundings of the three
// passes, PairView a pair's pointers, kabsch_solve the SVD and the bookkeeping,
// kabsch_frozen the step of a converged pair; block_sum and se3_row (p' = R p + t)
// live in device_utils.h, the Procrustes rotation in svd3.h.  The kernels differ
// only in where a thread's points come from: kabsch_kernel streams them from
// memory once per pass, kabsch_reg_kernel<TR> holds them in registers,
// kabsch_part_kernel<PHASE> streams one chunk of a large cloud (then
// kabsch_final_kernel, kabsch_apply_kernel).  A thread always adds its points
// i = first + tid, + 1024, .. in ascending order, so all three give the same bits.
#include <cstdlib>

#include "kernels.h"
#include "device_utils.h"
#include "svd3.h"

namespace dsir {

namespace {

// the passes' loops are unrolled x4: a thread's iterations are independent up to the fp64 adds (kept in order: same bits), and
// on large clouds - 64 points per thread and pass at 65536 - the index -> ref gather chains of consecutive iterations overlap
#define DSIR_KABSCH_UNROLL _Pragma("unroll 4")
constexpr int NTHR = 1024;
constexpr int NWAVE = NTHR / 64;

__device__ __forceinline__ void identity34(float (&T)[12]) {
  const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  for (int k = 0; k < 12; ++k) T[k] = I[k];
}

// a frozen pair (ICP converged; one thread): identity step, cumulative transform carried over
__device__ void kabsch_frozen(const KabschArgs& a, int pair) {
  float I[12];
  identity34(I);
  for (int k = 0; k < 12; ++k) a.T[(int64_t)pair * 12 + k] = I[k];
  if (a.T_cum) {
    float* out = a.T_cum + pair * a.T_stride;
    const float* P = a.T_prev ? a.T_prev + pair * a.T_stride : I;
    for (int k = 0; k < 12; ++k) out[k] = P[k];
  }
}

// a pair that per-pair counts leave without a source or a reference row (kernels.h): no correspondence, the frozen step
__device__ __forceinline__ bool pair_is_empty(const KabschArgs& a, int pair) {
  return (a.counts && a.counts[pair] <= 0) || (a.ref_counts && a.ref_counts[pair] <= 0);
}

// KabschArgs::zero_freeze: a pair whose S = sum |w| is exactly 0 takes the frozen step too.  Without the flag S = 0 runs on: wn = 0,
// H = 0 (finite, not the `bad` branch), svd3 gives U = V = I, so R = I and t = 0 - the identity in value, but composing it adds +0
// terms and turns a -0 of T_prev or of a point into +0 (icp_robust.h)
__device__ __forceinline__ bool all_weights_zero(const KabschArgs& a, double S) { return a.zero_freeze && S == 0.0; }

// thread 0 of a pair: H (fp32, as the reference forms it) -> SVD in fp64 -> R, t; the pair's transform, flag and cumulative
// transform to global memory, the transform to sT (12 floats) for the apply step
__device__ void kabsch_solve(const KabschArgs& a, int pair, const double (&v9)[9], const float (&cs)[3], const float (&ct)[3], float* sT) {
  bool finite = true;
  double H[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const float h = (float)v9[r * 3 + c];   // the reference's H is fp32, then .double()
      H[r][c] = (double)h;
      finite = finite && isfinite(h);
    }
  float T[12];
  identity34(T);
  int bad = 1;
  if (finite) {
    double U[3][3], S[3], V[3][3], Rd[3][3];
    svd3(H, U, S, V);
    procrustes_rotation(U, V, Rd);
    float R[3][3];
    bool ok = true;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        R[r][c] = (float)Rd[r][c];
        ok = ok && isfinite(R[r][c]);
      }
    if (ok) {
      bad = 0;
      for (int r = 0; r < 3; ++r) {
        T[r * 4 + 0] = R[r][0]; T[r * 4 + 1] = R[r][1]; T[r * 4 + 2] = R[r][2];
        float acc = __fmul_rn(-R[r][0], cs[0]);
        acc = fmaf(-R[r][1], cs[1], acc);
        acc = fmaf(-R[r][2], cs[2], acc);
        T[r * 4 + 3] = __fadd_rn(acc, ct[r]);
      }
    }
  }
  for (int k = 0; k < 12; ++k) { sT[k] = T[k]; a.T[(int64_t)pair * 12 + k] = T[k]; }
  if (a.invalid && bad) a.invalid[pair] |= 1;   // one thread per pair; bit 1 (clamped caller index, misc.hip) stays
  if (a.T_cum) {   // concatenate(R_t, T_prev): (R1 R2, R1 t2 + t1)   se3_torch.py:34-57
    float* out = a.T_cum + pair * a.T_stride;
    if (!a.T_prev) {
      for (int k = 0; k < 12; ++k) out[k] = T[k];
    } else {
      const float* P = a.T_prev + pair * a.T_stride;
      float C[12];
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c)
          C[r * 4 + c] = fmaf(T[r * 4 + 2], P[2 * 4 + c], fmaf(T[r * 4 + 1], P[1 * 4 + c], __fmul_rn(T[r * 4 + 0], P[c])));
        const float rt = fmaf(T[r * 4 + 2], P[2 * 4 + 3], fmaf(T[r * 4 + 1], P[1 * 4 + 3], __fmul_rn(T[r * 4 + 0], P[3])));
        C[r * 4 + 3] = __fadd_rn(rt, T[r * 4 + 3]);
      }
      for (int k = 0; k < 12; ++k) out[k] = C[k];
    }
  }
}

// one pair's inputs: the src points, the ref points they are matched to (through idx, or row by row) and the weights
struct PairView {
  const float* src; const float* ref; const int32_t* idx; const float* w;
  int ld, sigmoid;
  __device__ PairView(const KabschArgs& a, int pair)
      : src(a.src + pair * a.src_stride), ref(a.ref + pair * a.ref_stride), idx(a.idx ? a.idx + (int64_t)pair * a.m : nullptr),
        w(a.w + (int64_t)pair * a.m), ld(a.ref_ld ? a.ref_ld : 3), sigmoid(a.sigmoid) {}
  __device__ __forceinline__ float squash(float x) const { return sigmoid ? 1.f / (1.f + expf(-x)) : x; }
  __device__ __forceinline__ float weight(int i) const { return squash(w[i]); }
  __device__ __forceinline__ void source(int i, float (&s)[3]) const {
    s[0] = src[(int64_t)i * 3]; s[1] = src[(int64_t)i * 3 + 1]; s[2] = src[(int64_t)i * 3 + 2];
  }
  __device__ __forceinline__ void target(int i, float (&t)[3]) const {
    const int64_t j = idx ? idx[i] : i;
    t[0] = ref[j * ld]; t[1] = ref[j * ld + 1]; t[2] = ref[j * ld + 2];
  }
};

// ---- the three passes, one point at a time: THE statement of the fp32 roundings every kernel below shares
// pass 1: S = sum |w|
__device__ __forceinline__ void add_abs_weight(double (&v1)[1], float w) { v1[0] += (double)fabsf(w); }
__device__ __forceinline__ float weight_den(double S) { return (float)S + 1e-16f; }   // model.py:35 (fp32 sum + _EPS)
// pass 2: weighted centroids, wn = w / den
__device__ __forceinline__ void add_centroid_terms(double (&v6)[6], const float (&s)[3], const float (&t)[3], float wn) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    v6[c] += (double)__fmul_rn(s[c], wn);
    v6[3 + c] += (double)__fmul_rn(t[c], wn);
  }
}
__device__ __forceinline__ void centroids(const double (&v6)[6], float (&cs)[3], float (&ct)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) { cs[c] = (float)v6[c]; ct[c] = (float)v6[3 + c]; }
}
// pass 3: covariance H[a][b] = sum (s_a - cs_a) * ((t_b - ct_b) * wn)
__device__ __forceinline__ void add_covariance_terms(double (&v9)[9], const float (&s)[3], const float (&t)[3], float wn,
                                                     const float (&cs)[3], const float (&ct)[3]) {
  float sc[3], tw[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    sc[c] = __fsub_rn(s[c], cs[c]);
    tw[c] = __fmul_rn(__fsub_rn(t[c], ct[c]), wn);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) v9[r * 3 + c] += (double)__fmul_rn(sc[r], tw[c]);
}
// ---- the passes STREAMED: point i comes from memory.  DSIR_KABSCH_FOR_POINTS walks a thread's points i = first + tid, + 1024, .. < last
// in ascending order
#define DSIR_KABSCH_FOR_POINTS(i, first, last) DSIR_KABSCH_UNROLL for (int i = (first) + threadIdx.x; i < (last); i += NTHR)
__device__ __forceinline__ void stream_abs_weight(const PairView& p, int i, double (&v1)[1]) { add_abs_weight(v1, p.weight(i)); }
__device__ __forceinline__ void stream_centroid_terms(const PairView& p, int i, float den, double (&v6)[6]) {
  const float wn = p.weight(i) / den;
  float s[3], t[3];
  p.target(i, t);
  p.source(i, s);
  add_centroid_terms(v6, s, t, wn);
}
__device__ __forceinline__ void stream_covariance_terms(const PairView& p, int i, float den, const float (&cs)[3], const float (&ct)[3],
                                                        double (&v9)[9]) {
  const float wn = p.weight(i) / den;
  float s[3], t[3];
  p.target(i, t);
  p.source(i, s);
  add_covariance_terms(v9, s, t, wn, cs, ct);
}
// apply: p' = p R^T + t (se3_torch.py:60-77), and the matched ref point.  src_out may be the src array itself (ICP): a thread
// has read its point before it writes it
__device__ __forceinline__ void stream_apply(const PairView& p, float* so, float* mo, int i, const float* T) {
  if (mo) {
    float t[3];
    p.target(i, t);
    mo[(int64_t)i * 3] = t[0]; mo[(int64_t)i * 3 + 1] = t[1]; mo[(int64_t)i * 3 + 2] = t[2];
  }
  if (so) {
    float s[3];
    p.source(i, s);
#pragma unroll
    for (int r = 0; r < 3; ++r) so[(int64_t)i * 3 + r] = se3_row(T, r, s[0], s[1], s[2]);
  }
}

// one 1024-thread workgroup per pair, the points streamed once per pass
__global__ __launch_bounds__(NTHR) void kabsch_kernel(const KabschArgs a) {
  __shared__ double sh[NWAVE * 9 + 9];
  __shared__ float sT[12];
  const int pair = blockIdx.x;
  const int m = pair_rows(a.counts, pair, a.m);   // the pair's own points; a.m stays the stride of idx, w and matched_out (block-uniform)
  if ((a.skip && a.skip[pair]) || pair_is_empty(a, pair)) {   // block-uniform
    if (threadIdx.x == 0) kabsch_frozen(a, pair);
    return;
  }
  const PairView p(a, pair);
  double v1[1] = {0.0};
  DSIR_KABSCH_FOR_POINTS(i, 0, m) stream_abs_weight(p, i, v1);
  block_sum<NWAVE>(v1, sh);
  if (all_weights_zero(a, v1[0])) {   // block-uniform: block_sum leaves the block's sum with every thread
    if (threadIdx.x == 0) kabsch_frozen(a, pair);
    return;
  }
  const float den = weight_den(v1[0]);
  double v6[6] = {0, 0, 0, 0, 0, 0};
  DSIR_KABSCH_FOR_POINTS(i, 0, m) stream_centroid_terms(p, i, den, v6);
  block_sum<NWAVE>(v6, sh);
  float cs[3], ct[3];
  centroids(v6, cs, ct);
  double v9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  DSIR_KABSCH_FOR_POINTS(i, 0, m) stream_covariance_terms(p, i, den, cs, ct, v9);
  block_sum<NWAVE>(v9, sh);

  if (threadIdx.x == 0) kabsch_solve(a, pair, v9, cs, ct, sT);
  __syncthreads();
  if (a.src_out || a.matched_out) {
    float* so = a.src_out ? a.src_out + pair * a.src_out_stride : nullptr;
    float* mo = a.matched_out ? a.matched_out + (int64_t)pair * a.m * 3 : nullptr;
    for (int i = threadIdx.x; i < m; i += NTHR) stream_apply(p, so, mo, i, sT);
  }
}

// ---- clouds of up to TR x 1024 points: the same passes with the points HELD IN REGISTERS between them.  With one pair in
// flight (the reference's evaluation mode) the solve sits in the dependent chain of every iteration, and each pass of kabsch_kernel
// opens with its own weight -> index -> ref-point load chain (three round trips to L2 plus the apply step's fourth); here the chain
// is paid once.  A thread owns the same points i = tid, tid + 1024, .. and hands them to the same per-point functions in the same
// order: same bits as kabsch_kernel.
template <int TR>
__global__ __launch_bounds__(NTHR) void kabsch_reg_kernel(const KabschArgs a) {
  __shared__ double sh[NWAVE * 9 + 9];
  __shared__ float sT[12];
  const int pair = blockIdx.x;
  const int m = pair_rows(a.counts, pair, a.m);   // the pair's own points; a.m stays the stride of idx, w and matched_out (block-uniform)
  if ((a.skip && a.skip[pair]) || pair_is_empty(a, pair)) {   // block-uniform
    if (threadIdx.x == 0) kabsch_frozen(a, pair);
    return;
  }
  const PairView p(a, pair);
  float w[TR], s[TR][3], t[TR][3];
#pragma unroll
  for (int k = 0; k < TR; ++k) {
    const int i = threadIdx.x + k * NTHR;
    w[k] = 0.f;
    s[k][0] = s[k][1] = s[k][2] = t[k][0] = t[k][1] = t[k][2] = 0.f;
    if (i < m) {
      w[k] = p.w[i];
      p.target(i, t[k]);
      p.source(i, s[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < TR; ++k) w[k] = p.squash(w[k]);

  double v1[1] = {0.0};
#pragma unroll
  for (int k = 0; k < TR; ++k)
    if (threadIdx.x + k * NTHR < m) add_abs_weight(v1, w[k]);
  block_sum<NWAVE>(v1, sh);
  if (all_weights_zero(a, v1[0])) {   // block-uniform: block_sum leaves the block's sum with every thread
    if (threadIdx.x == 0) kabsch_frozen(a, pair);
    return;
  }
  const float den = weight_den(v1[0]);

  double v6[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < TR; ++k)
    if (threadIdx.x + k * NTHR < m) {
      w[k] = w[k] / den;          // wn, formed once: the quotient both streamed passes form
      add_centroid_terms(v6, s[k], t[k], w[k]);
    }
  block_sum<NWAVE>(v6, sh);
  float cs[3], ct[3];
  centroids(v6, cs, ct);

  double v9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < TR; ++k)
    if (threadIdx.x + k * NTHR < m) add_covariance_terms(v9, s[k], t[k], w[k], cs, ct);
  block_sum<NWAVE>(v9, sh);

  if (threadIdx.x == 0) kabsch_solve(a, pair, v9, cs, ct, sT);
  __syncthreads();
  if (a.src_out || a.matched_out) {
    float* so = a.src_out ? a.src_out + pair * a.src_out_stride : nullptr;
    float* mo = a.matched_out ? a.matched_out + (int64_t)pair * a.m * 3 : nullptr;
#pragma unroll
    for (int k = 0; k < TR; ++k)
      if (threadIdx.x + k * NTHR < m) {
        const int i = threadIdx.x + k * NTHR;
        if (mo) { mo[(int64_t)i * 3] = t[k][0]; mo[(int64_t)i * 3 + 1] = t[k][1]; mo[(int64_t)i * 3 + 2] = t[k][2]; }
        if (so) {
#pragma unroll
          for (int r = 0; r < 3; ++r) so[(int64_t)i * 3 + r] = se3_row(sT, r, s[k][0], s[k][1], s[k][2]);
        }
      }
  }
}

// ---- large clouds: the same three passes over CHUNKS of 4096 points, one workgroup per (chunk, pair) and pass, partial sums
// in fp64 in a.part [pairs][chunks][16] = {S, c_s, c_t, H}; every pass adds the chunks' partials in chunk order (every
// workgroup for itself: a few dozen doubles), so the result does not depend on the grid.  One workgroup per pair walks
// 65536 points in 64 dependent trips per pass (218 us per solve with 2 pairs in flight); in chunks: five short launches.
constexpr int CHUNK = 4096;

// the chunks' partials of one pass, added in chunk order
template <int NV>
__device__ __forceinline__ void sum_chunks(const double* part, int nch, int at, double (&v)[NV]) {
  for (int c = 0; c < nch; ++c)
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] += part[c * 16 + at + k];
}

template <int PHASE>
__global__ __launch_bounds__(NTHR) void kabsch_part_kernel(const KabschArgs a, int nch) {
  __shared__ double sh[NWAVE * 9 + 9];
  const int pair = blockIdx.y, ch = blockIdx.x;
  if (a.skip && a.skip[pair]) return;                 // block-uniform (frozen pair): kabsch_final_kernel writes the identity
  double* part = a.part + (int64_t)pair * nch * 16;
  const PairView p(a, pair);
  const int first = ch * CHUNK, last = min(a.m, first + CHUNK);
  float den = 0.f, cs[3] = {0.f, 0.f, 0.f}, ct[3] = {0.f, 0.f, 0.f};
  if (PHASE >= 1) {
    double S[1] = {0.0};
    sum_chunks(part, nch, 0, S);
    den = weight_den(S[0]);
  }
  if (PHASE >= 2) {
    double v[6] = {0, 0, 0, 0, 0, 0};
    sum_chunks(part, nch, 1, v);
    centroids(v, cs, ct);
  }
  if (PHASE == 0) {
    double v1[1] = {0.0};
    DSIR_KABSCH_FOR_POINTS(i, first, last) stream_abs_weight(p, i, v1);
    block_sum<NWAVE>(v1, sh);
    if (threadIdx.x == 0) part[ch * 16] = v1[0];
  } else if (PHASE == 1) {
    double v6[6] = {0, 0, 0, 0, 0, 0};
    DSIR_KABSCH_FOR_POINTS(i, first, last) stream_centroid_terms(p, i, den, v6);
    block_sum<NWAVE>(v6, sh);
    if (threadIdx.x < 6) part[ch * 16 + 1 + threadIdx.x] = v6[threadIdx.x];
  } else {
    double v9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    DSIR_KABSCH_FOR_POINTS(i, first, last) stream_covariance_terms(p, i, den, cs, ct, v9);
    block_sum<NWAVE>(v9, sh);
    if (threadIdx.x < 9) part[ch * 16 + 7 + threadIdx.x] = v9[threadIdx.x];
  }
}

// one thread per pair: the chunks' partials in order -> the solve of kabsch_kernel
__global__ __launch_bounds__(64) void kabsch_final_kernel(const KabschArgs a, int nch) {
  const int pair = blockIdx.x * 64 + threadIdx.x;
  if (pair >= a.pairs) return;
  if (a.skip && a.skip[pair]) { kabsch_frozen(a, pair); return; }
  const double* part = a.part + (int64_t)pair * nch * 16;
  double v6[6] = {0, 0, 0, 0, 0, 0}, v9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  sum_chunks(part, nch, 1, v6);
  sum_chunks(part, nch, 7, v9);
  float cs[3], ct[3], sT[12];
  centroids(v6, cs, ct);
  kabsch_solve(a, pair, v9, cs, ct, sT);
}

// the apply step of the chunked path, one thread per point
__global__ __launch_bounds__(256) void kabsch_apply_kernel(const KabschArgs a) {
  const int pair = blockIdx.y;
  if (a.skip && a.skip[pair]) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.m) return;
  stream_apply(PairView(a, pair), a.src_out ? a.src_out + pair * a.src_out_stride : nullptr,
               a.matched_out ? a.matched_out + (int64_t)pair * a.m * 3 : nullptr, i, a.T + (int64_t)pair * 12);
}

}  // namespace

// clouds of that many points and more take the chunked path (dsir_set_kabsch_chunked_min moves the threshold of a context)
static int chunked_min(int chunk_min) { return chunk_min > 0 ? chunk_min : kKabschChunkedMin; }

size_t kabsch_part_bytes(int pairs, int m, int chunk_min) {
  return m >= chunked_min(chunk_min) ? (size_t)pairs * ((m + CHUNK - 1) / CHUNK) * 16 * sizeof(double) : 0;
}

void launch_kabsch(const KabschArgs& a, hipStream_t st) {
  if (a.pairs <= 0) return;
  if (a.part && !a.counts && !a.ref_counts && a.m >= chunked_min(a.chunk_min)) {
    // the choice depends on the cloud size alone: a pair's pose does not depend on what else is in the batch
    const int nch = (a.m + CHUNK - 1) / CHUNK;
    const dim3 grid(nch, a.pairs);
    hipLaunchKernelGGL(kabsch_part_kernel<0>, grid, dim3(NTHR), 0, st, a, nch);
    hipLaunchKernelGGL(kabsch_part_kernel<1>, grid, dim3(NTHR), 0, st, a, nch);
    hipLaunchKernelGGL(kabsch_part_kernel<2>, grid, dim3(NTHR), 0, st, a, nch);
    hipLaunchKernelGGL(kabsch_final_kernel, dim3((a.pairs + 63) / 64), dim3(64), 0, st, a, nch);
    if (a.src_out || a.matched_out) hipLaunchKernelGGL(kabsch_apply_kernel, dim3((a.m + 255) / 256, a.pairs), dim3(256), 0, st, a);
    return;
  }
  // (the choice depends on the cloud size alone, and the two kernels give the same bits - which is why, with per-pair counts, the
  // capacity m may choose for every pair of the launch: a pair's bits are those of the kernel its own count would have chosen)
  static const bool no_reg = tuning_flag("DSIR_KABSCH_STREAM");      // A/B switch: the streaming kernel for every size
  if (a.m <= 5 * NTHR && !no_reg) hipLaunchKernelGGL(kabsch_reg_kernel<5>, dim3(a.pairs), dim3(NTHR), 0, st, a);
  else if (a.m <= 8 * NTHR && !no_reg) hipLaunchKernelGGL(kabsch_reg_kernel<8>, dim3(a.pairs), dim3(NTHR), 0, st, a);
  else hipLaunchKernelGGL(kabsch_kernel, dim3(a.pairs), dim3(NTHR), 0, st, a);
}

}  // namespace dsir
