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
// not depend on what else is in the call.  The resampling step (dsir_t_resample_keyed) is resample.hip's, shared with the engine.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsir_train.h"
#include "device_utils.h"
#include "augment_params.h"
#include "scratch.h"
#include "train_ops.h"

namespace dsir {
namespace {

constexpr int CB = 16;                 // centroid: blocks per cloud (stage 1)
constexpr int CT = 256;                // centroid: threads per block

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

}  // namespace
}  // namespace dsir

using namespace dsir;

extern "C" {

size_t dsir_t_cloud_centroids_scratch(int clouds) { return clouds < 1 ? 0 : align256((size_t)clouds * CB * 3 * sizeof(double)); }

int dsir_t_cloud_centroids(void* stream, const float* points, const int32_t* counts, int clouds, int cap, int stride, double* centroids,
                           int32_t* invalid, void* scratch) {
  if (!points || !counts || !centroids || !invalid || !scratch || !aug_shape_ok(clouds, cap, stride)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  double* partial = reinterpret_cast<double*>(scratch);
  hipLaunchKernelGGL(centroid_partial_kernel, dim3(CB, clouds), dim3(CT), 0, st, points, counts, cap, stride, partial);
  hipLaunchKernelGGL(centroid_final_kernel, dim3((clouds + 63) / 64), dim3(64), 0, st, partial, counts, clouds, cap, centroids, invalid);
  return done();
}

int dsir_t_augment(void* stream, const float* in, const int32_t* counts, int clouds, int k, int stride, const void* params,
                   const double* centroids, float* out) {
  if (!in || !counts || !params || !centroids || !out || !aug_shape_ok(clouds, k, stride)) return (int)hipErrorInvalidValue;
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
