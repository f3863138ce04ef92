// Training augmentation on the device (include/dsir_train.h, "training augmentation"): what sits between the voxel grid and the
// ground-truth matches in the reference's loaders (dataloader/data_base.py:221-296 apply_augment / apply_augment_V2).
//
// The reference draws from numpy's global RNG, an unseeded RandomState and python's random: nothing to pin, so the rule is owned
// here and written down once on the host in deepsir_amd/augment.py, which the tests compare against:
//     cloud key  k (host): splitmix64 chain over (seed, epoch, dataset index, side); never the position in a batch
//     draw       d = splitmix64(k ^ (stream << 40) ^ element),  u = (d >> 11) 2^-53
//     per point, fp32, every operation rounded on its own (no fused multiply-add), R, t, s, m rounded to fp32 once:
//         d = p - m (transform about the centroid only);  r_i = ((R_i0 d_0 + R_i1 d_1) + R_i2 d_2) + t_i
//         q_i = r_i + jitter_i (gate fired only);  out_i = s q_i (gate fired only)
//     jitter in float64, rounded once: uniform u * scale, or clip(sigma * Box-Muller(u1, u2), +-clip)
// The order of steps is the reference's (rotate -> resample -> jitter -> scale); the rotation is pointwise and runs after the gather.
//
// No atomics anywhere: the centroid is a two-stage sum in a fixed order (thread-strided partials, an LDS tree, the blocks' partials in
// block order), so two runs write the same bytes.  Every cloud is handled by its own blocks / lanes from its own key: a cloud's rows do
// not depend on what else is in the call.  The segmented sort is a library call (hipCUB).
#include <hipcub/hipcub.hpp>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsir_train.h"
#include "device_utils.h"

namespace dsir {
namespace {

constexpr int CB = 16;                 // centroid: blocks per cloud (stage 1)
constexpr int CT = 256;                // centroid: threads per block
constexpr uint64_t kPadKey = ~0ull;
constexpr uint64_t STREAM_PERM = 1ull << 40, STREAM_TOPUP = 2ull << 40, STREAM_JITTER = 3ull << 40;

// one cloud's parameter block: 24 eight-byte slots (deepsir_amd/augment.py::pack_params)
struct AugParams {
  double R[9], t[3], s, jscale, jclip;
  int64_t jmode, centered, normals;
  uint64_t key;
  int64_t rmode, scaled, pad[3];
};
static_assert(sizeof(AugParams) == 24 * 8, "AugParams is 24 slots");

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int grid1(int64_t total) { const int64_t g = (total + 255) / 256; return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g)); }
inline int done() { return (int)hipGetLastError(); }

// ---- centroids: stage 1, block (b, cloud) sums rows [b chunk, (b + 1) chunk) of the cloud's first n rows
__global__ __launch_bounds__(CT) void centroid_partial_kernel(const float* __restrict__ pts, const int32_t* __restrict__ counts, int cap,
                                                              int stride, double* __restrict__ partial) {
  __shared__ double red[3][CT];
  const int cloud = blockIdx.y, b = blockIdx.x;
  const int n = max(0, min(counts[cloud], cap));
  const int chunk = (n + CB - 1) / CB;
  const int lo = min(n, b * chunk), hi = min(n, lo + chunk);
  double s[3] = {0.0, 0.0, 0.0};
  for (int i = lo + (int)threadIdx.x; i < hi; i += CT) {
    const float* p = pts + ((int64_t)cloud * cap + i) * stride;
    s[0] += (double)p[0]; s[1] += (double)p[1]; s[2] += (double)p[2];
  }
  for (int k = 0; k < 3; ++k) red[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int o = CT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x < 3) partial[((int64_t)cloud * CB + b) * 3 + threadIdx.x] = red[threadIdx.x][0];
}

// stage 2: one thread per cloud adds the CB partials in block order
__global__ void centroid_final_kernel(const double* __restrict__ partial, const int32_t* __restrict__ counts, int clouds, int cap,
                                      double* __restrict__ centroids, int32_t* __restrict__ invalid) {
  const int cloud = blockIdx.x * blockDim.x + threadIdx.x;
  if (cloud >= clouds) return;
  const int n = max(0, min(counts[cloud], cap));
  int32_t bits = n == 0 ? 1 : 0;
  for (int k = 0; k < 3; ++k) {
    double s = 0.0;
    for (int b = 0; b < CB; ++b) s += partial[((int64_t)cloud * CB + b) * 3 + k];
    const double m = n > 0 ? s / (double)n : 0.0;
    if (!isfinite(m)) bits |= 2;
    centroids[cloud * 3 + k] = m;
  }
  invalid[cloud] = bits;
}

// ---- resampling with a key per cloud: dsir_resample's rule with the cloud's key in place of (seed, position in the call)
__global__ void aug_sort_key_kernel(const int32_t* __restrict__ counts, const AugParams* __restrict__ prm, int clouds, int cap,
                                    uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, int* __restrict__ seg) {
  const int64_t total = (int64_t)clouds * cap;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= total; e += (int64_t)gridDim.x * blockDim.x) {
    if (e <= clouds) seg[e] = (int)(e * cap);                                                  // total >= clouds: every offset is visited
    if (e == total) break;
    const int c = (int)(e / cap), i = (int)(e % cap);
    const int n = min(counts[c], cap);
    keys[e] = i < n ? (splitmix64(prm[c].key ^ STREAM_PERM ^ (uint64_t)i) >> 1) : kPadKey;   // padding sorts last
    vals[e] = (uint32_t)i;
  }
}

__global__ void aug_gather_kernel(const float* __restrict__ in, const int32_t* __restrict__ counts, const AugParams* __restrict__ prm,
                                  const uint32_t* __restrict__ perm, int cap, int stride, int k, float* __restrict__ out,
                                  int32_t* __restrict__ rows) {
  const int c = blockIdx.y;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  const int n = min(counts[c], cap);
  float* o = out + ((int64_t)c * k + j) * stride;
  if (n <= 0) {
    for (int ch = 0; ch < stride; ++ch) o[ch] = 0.f;
    if (rows) rows[(int64_t)c * k + j] = 0;
    return;
  }
  const int mode = (int)prm[c].rmode;
  int srow;
  if (mode == 1) srow = j % n;                                                   // FixedResampler: tile / prefix
  else if (mode == 2) srow = (int)perm[(int64_t)c * cap + j % n];                // the loader's permutation, then FixedResampler
  else if (j < n) srow = (int)perm[(int64_t)c * cap + j];                        // Resampler: random order, no repeats
  else srow = (int)(splitmix64(prm[c].key ^ STREAM_TOPUP ^ (uint64_t)j) % (uint64_t)n);   // top-up with replacement
  const float* s = in + ((int64_t)c * cap + srow) * stride;
  for (int ch = 0; ch < stride; ++ch) o[ch] = s[ch];
  if (rows) rows[(int64_t)c * k + j] = srow;
}

// ---- the per-point pass: one row per lane, a cloud's rows contiguous; in place is fine (a lane reads its row, then writes it)
__device__ __forceinline__ float jitter_draw(const AugParams& P, uint64_t e) {
  const uint64_t d0 = splitmix64(P.key ^ STREAM_JITTER ^ e);
  if (P.jmode == 1) return (float)((double)(d0 >> 11) * 0x1p-53 * P.jscale);
  const uint64_t d1 = splitmix64(P.key ^ STREAM_JITTER ^ (e + 1));
  const double u1 = ((double)(d0 >> 11) + 1.0) * 0x1p-53, u2 = (double)(d1 >> 11) * 0x1p-53;     // (0, 1], [0, 1)
  const double z = sqrt(-2.0 * log(u1)) * cos((2.0 * 3.14159265358979323846) * u2);
  return (float)fmin(fmax(P.jscale * z, -P.jclip), P.jclip);
}

__device__ __forceinline__ float rot_row(const float* R, float x, float y, float z) {
  return __fadd_rn(__fadd_rn(__fmul_rn(R[0], x), __fmul_rn(R[1], y)), __fmul_rn(R[2], z));
}

__global__ __launch_bounds__(256) void augment_kernel(const float* in, const int32_t* __restrict__ counts,
                                                      const AugParams* __restrict__ prm, const double* __restrict__ centroids, int k,
                                                      int stride, float* out) {
  const int c = blockIdx.y;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  const float* p = in + ((int64_t)c * k + j) * stride;
  float* o = out + ((int64_t)c * k + j) * stride;
  if (counts[c] <= 0) {                       // an empty cloud stays zeros, whatever its parameters
    for (int ch = 0; ch < stride; ++ch) o[ch] = 0.f;
    return;
  }
  const AugParams& P = prm[c];
  float R[9], t[3];
  for (int i = 0; i < 9; ++i) R[i] = (float)P.R[i];
  for (int i = 0; i < 3; ++i) t[i] = (float)P.t[i];
  float d[3] = {p[0], p[1], p[2]};
  if (P.centered)
    for (int i = 0; i < 3; ++i) d[i] = __fsub_rn(d[i], (float)centroids[c * 3 + i]);
  float q[3];
  for (int i = 0; i < 3; ++i) q[i] = __fadd_rn(rot_row(R + 3 * i, d[0], d[1], d[2]), t[i]);
  if (P.jmode != 0)
    for (int i = 0; i < 3; ++i) q[i] = __fadd_rn(q[i], jitter_draw(P, (uint64_t)j * 8 + (uint64_t)i * 2));
  if (P.scaled) {
    const float s = (float)P.s;
    for (int i = 0; i < 3; ++i) q[i] = __fmul_rn(s, q[i]);
  }
  float nv[3];
  const bool rot_n = P.normals != 0 && stride >= 6;
  if (rot_n) {
    const float v0 = p[3], v1 = p[4], v2 = p[5];
    for (int i = 0; i < 3; ++i) nv[i] = rot_row(R + 3 * i, v0, v1, v2);
  }
  if (in != out)
    for (int ch = 3; ch < stride; ++ch) o[ch] = p[ch];
  for (int i = 0; i < 3; ++i) o[i] = q[i];
  if (rot_n)
    for (int i = 0; i < 3; ++i) o[3 + i] = nv[i];
}

// ---- ground truth: T = A_ref M A_src^-1, A = [R | t - R m], float64, one thread per pair
__device__ void gt_affine(const AugParams& P, const double* cen, double* R, double* t) {
  for (int i = 0; i < 9; ++i) R[i] = P.R[i];
  for (int i = 0; i < 3; ++i) {
    double v = P.t[i];
    if (P.centered)                           // the centroid as the points saw it: rounded to fp32
      v -= (R[3 * i] * (double)(float)cen[0] + R[3 * i + 1] * (double)(float)cen[1]) + R[3 * i + 2] * (double)(float)cen[2];
    t[i] = v;
  }
}

__global__ void augment_gt_kernel(const double* __restrict__ M, const AugParams* __restrict__ ps, const AugParams* __restrict__ pr,
                                  const double* __restrict__ cs, const double* __restrict__ cr, int pairs, int reference_gt,
                                  float* __restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pairs) return;
  double Rs[9], ts[3], Rr[9], tr[3];
  gt_affine(ps[p], cs + p * 3, Rs, ts);
  gt_affine(pr[p], cr + p * 3, Rr, tr);
  const double* m = M + p * 12;
  double ti[3];                               // A_src^-1 = [Rs^T | -Rs^T ts]
  for (int i = 0; i < 3; ++i) ti[i] = -((Rs[i] * ts[0] + Rs[3 + i] * ts[1]) + Rs[6 + i] * ts[2]);
  double B[9], bt[3];                         // M A_src^-1
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) B[3 * i + j] = (m[4 * i] * Rs[3 * j] + m[4 * i + 1] * Rs[3 * j + 1]) + m[4 * i + 2] * Rs[3 * j + 2];
    bt[i] = ((m[4 * i] * ti[0] + m[4 * i + 1] * ti[1]) + m[4 * i + 2] * ti[2]) + m[4 * i + 3];
  }
  const double s = (ps[p].scaled && !reference_gt) ? ps[p].s : 1.0;
  float* o = out + p * 12;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o[4 * i + j] = (float)((Rr[3 * i] * B[j] + Rr[3 * i + 1] * B[3 + j]) + Rr[3 * i + 2] * B[6 + j]);
    o[4 * i + 3] = (float)(s * (((Rr[3 * i] * bt[0] + Rr[3 * i + 1] * bt[1]) + Rr[3 * i + 2] * bt[2]) + tr[i]));
  }
}

inline bool shape_ok(int clouds, int cap, int stride) {
  return clouds >= 1 && cap >= 1 && stride >= 3 && (int64_t)clouds * cap <= 0x7fffffffll && clouds <= 65535;
}

inline size_t seg_sort_bytes(int64_t total, int clouds) {
  size_t b = 0;
  hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                              (uint32_t*)nullptr, (int)total, clouds, (const int*)nullptr, (const int*)nullptr);
  return b;
}

}  // namespace
}  // namespace dsir

using namespace dsir;

extern "C" {

size_t dsir_t_cloud_centroids_scratch(int clouds) { return clouds < 1 ? 0 : align256((size_t)clouds * CB * 3 * sizeof(double)); }

int dsir_t_cloud_centroids(void* stream, const float* points, const int32_t* counts, int clouds, int cap, int stride, double* centroids,
                           int32_t* invalid, void* scratch) {
  if (!points || !counts || !centroids || !invalid || !scratch || !shape_ok(clouds, cap, stride)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  double* partial = reinterpret_cast<double*>(scratch);
  hipLaunchKernelGGL(centroid_partial_kernel, dim3(CB, clouds), dim3(CT), 0, st, points, counts, cap, stride, partial);
  hipLaunchKernelGGL(centroid_final_kernel, dim3((clouds + 63) / 64), dim3(64), 0, st, partial, counts, clouds, cap, centroids, invalid);
  return done();
}

size_t dsir_t_resample_keyed_scratch(int clouds, int cap) {
  if (!shape_ok(clouds, cap, 3)) return 0;
  const int64_t total = (int64_t)clouds * cap;
  return 2 * align256((size_t)total * 8) + 2 * align256((size_t)total * 4) + align256((size_t)(clouds + 1) * 4) +
         align256(seg_sort_bytes(total, clouds));
}

int dsir_t_resample_keyed(void* stream, const float* in, const int32_t* counts, int clouds, int cap, int stride, int k, const void* params,
                          int need_perm, float* out, int32_t* rows, void* scratch) {
  if (!in || !counts || !params || !out || !scratch || !shape_ok(clouds, cap, stride) || k < 1 || (int64_t)clouds * k > 0x7fffffffll)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = (int64_t)clouds * cap;
  const AugParams* prm = reinterpret_cast<const AugParams*>(params);
  char* p = reinterpret_cast<char*>(scratch);
  auto take = [&](size_t bytes) { char* r = p; p += align256(bytes); return r; };
  uint64_t* k0 = reinterpret_cast<uint64_t*>(take((size_t)total * 8));
  uint64_t* k1 = reinterpret_cast<uint64_t*>(take((size_t)total * 8));
  uint32_t* v0 = reinterpret_cast<uint32_t*>(take((size_t)total * 4));
  uint32_t* v1 = reinterpret_cast<uint32_t*>(take((size_t)total * 4));
  int* seg = reinterpret_cast<int*>(take((size_t)(clouds + 1) * 4));
  if (need_perm) {
    size_t tb = seg_sort_bytes(total, clouds);
    hipLaunchKernelGGL(aug_sort_key_kernel, dim3(grid1(total + 1)), dim3(256), 0, st, counts, prm, clouds, cap, k0, v0, seg);
    if (hipcub::DeviceSegmentedRadixSort::SortPairs(p, tb, k0, k1, v0, v1, (int)total, clouds, seg, seg + 1, 0, 64, st) != hipSuccess)
      return (int)hipErrorUnknown;
  }
  hipLaunchKernelGGL(aug_gather_kernel, dim3((k + 255) / 256, clouds), dim3(256), 0, st, in, counts, prm, (const uint32_t*)v1, cap, stride, k,
                     out, rows);
  return done();
}

int dsir_t_augment(void* stream, const float* in, const int32_t* counts, int clouds, int k, int stride, const void* params,
                   const double* centroids, float* out) {
  if (!in || !counts || !params || !centroids || !out || !shape_ok(clouds, k, stride)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(augment_kernel, dim3((k + 255) / 256, clouds), dim3(256), 0, (hipStream_t)stream, in, counts,
                     reinterpret_cast<const AugParams*>(params), centroids, k, stride, out);
  return done();
}

int dsir_t_augment_gt(void* stream, const double* M, const void* params_src, const void* params_ref, const double* centroids_src,
                      const double* centroids_ref, int pairs, int reference_gt, float* transform_gt) {
  if (!M || !params_src || !params_ref || !centroids_src || !centroids_ref || !transform_gt || pairs < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(augment_gt_kernel, dim3((pairs + 63) / 64), dim3(64), 0, (hipStream_t)stream, M, reinterpret_cast<const AugParams*>(params_src),
                     reinterpret_cast<const AugParams*>(params_ref), centroids_src, centroids_ref, pairs, reference_gt, transform_gt);
  return done();
}

}  // extern "C"
