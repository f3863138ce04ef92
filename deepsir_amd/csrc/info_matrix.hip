// Information matrix of a registered pair (dsir_information_matrix): open3d's get_information_matrix_from_point_clouds for P pairs at
// once.  open3d is not installable here: parity is unpinned, THE RULE IS OWNED HERE and restated in deepsir_amd/pose_graph.py
// (information_matrix_host).  The correspondence set is the one launch_icp_correspondences (icp.hip) writes for the same arguments
// - this file calls that search and does not restate it.  For every source row with idx >= 0, q = (x, y, z) the fp32 reference
// point it matched, taken to fp64:
//   G = [ 0  z -y 1 0 0 ;  -z 0 x 0 1 0 ;  y -x 0 0 0 1 ],   info = sum G^T G   (6 x 6, order [rotation; translation])
// which needs ten sums: n, Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz (a product of two fp32 values is exact in fp64):
//   info[0][0] = Syy + Szz   info[0][1] = -Sxy        info[0][2] = -Sxz        info[0][3] = 0    info[0][4] = -Sz  info[0][5] = Sy
//                            info[1][1] = Sxx + Szz   info[1][2] = -Syz        info[1][3] = Sz   info[1][4] = 0    info[1][5] = -Sx
//                                                     info[2][2] = Sxx + Syy   info[2][3] = -Sy  info[2][4] = Sx   info[2][5] = 0
//   info[3][3] = info[4][4] = info[5][5] = n, the rest of that block 0; the lower triangle mirrors the upper, bit for bit.
// Kernels, in the scheme of icp_plane_accum_kernel: info_accum_kernel, one workgroup per (chunk of kIcpPlaneChunk source points,
// pair), wave butterflies, then the waves in order, into the chunk's own slot; info_finish_kernel, one thread per sum, adds a pair's
// slots in chunk order and writes the 36 entries and the count.  No atomics: the partition depends on J alone, so a pair's bytes
// depend neither on the run nor on the other pairs of the call.  A pair without a correspondence gets the zero matrix and count 0.
// Clouds of unequal sizes (dsir_information_matrix_ex: per-pair counts, J and K the row capacities): the search is
// launch_icp_correspondences' with the same counts; the chunks are those of the pair's own Jp rows (last = min(Jp, first +
// kIcpPlaneChunk); chunks at or beyond icp_plane_chunks(Jp) leave without writing, and that many slots are added), so pair p gets,
// byte for byte, the matrix and count of the dense call on its first Jp and Kp rows alone.  Jp == 0 or Kp == 0: the zero matrix, count 0.
// No atomics, no scratch shared between pairs, the same bytes on every run - with counts as without.
#include "device_utils.h"
#include "engine_ctx.h"
#include "icp_grid.h"
#include "icp_layout.h"
#include "kernels.h"

namespace dsir {

namespace {

constexpr int PT = 256;
constexpr int kInfoSums = 10;     // n, Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz
constexpr int kInfoSlots = 16;    // doubles per (pair, chunk) partial

// the search's outputs and the partial sums, then the search's own scratch
struct InfoLayout {
  size_t idx, d2, part, corr, bytes;
  InfoLayout(int pairs, int J, size_t corr_bytes) {
    const size_t n = (size_t)pairs * (size_t)J;
    Carve c;
    idx = c.take(n * 4);
    d2 = c.take(n * 4);
    part = c.take((size_t)pairs * (size_t)icp_plane_chunks(J) * kInfoSlots * sizeof(double));
    corr = c.take(corr_bytes);
    bytes = c.p;
  }
};

__global__ __launch_bounds__(PT) void info_accum_kernel(const float* __restrict__ ref, int ref_stride, const int32_t* __restrict__ idx,
                                                        int J, int K, const int32_t* __restrict__ counts_src,
                                                        const int32_t* __restrict__ counts_ref, double* __restrict__ part) {
  __shared__ double sh[(PT / 64 + 1) * kInfoSums];
  const int pair = blockIdx.y, ch = blockIdx.x;
  const int Jp = pair_rows(counts_src, pair, J), Kp = pair_rows(counts_ref, pair, K);   // the pair's own rows; J, K: the capacities
  if (ch >= icp_plane_chunks(Jp)) return;                 // a chunk of padding rows only: no slot of the pair's sum (block-uniform)
  const float* S = ref + (int64_t)pair * K * ref_stride;
  const int first = ch * kIcpPlaneChunk, last = min(Jp, first + kIcpPlaneChunk);
  double v[kInfoSums];
#pragma unroll
  for (int k = 0; k < kInfoSums; ++k) v[k] = 0.0;
  for (int j = first + threadIdx.x; j < last; j += PT) {
    const int64_t i = idx[(int64_t)pair * J + j];
    if (i < 0 || i >= Kp) continue;                       // no correspondence (the search writes -1 .. Kp-1 only)
    const double x = (double)S[i * ref_stride], y = (double)S[i * ref_stride + 1], z = (double)S[i * ref_stride + 2];
    v[0] += 1.0; v[1] += x; v[2] += y; v[3] += z;
    v[4] += x * x; v[5] += y * y; v[6] += z * z; v[7] += x * y; v[8] += x * z; v[9] += y * z;
  }
  block_sum<PT / 64>(v, sh);
  if (threadIdx.x < kInfoSums)
    part[((int64_t)pair * gridDim.x + ch) * kInfoSlots + threadIdx.x] = sh[(PT / 64) * kInfoSums + threadIdx.x];
}

// nch: the slots a pair has (the capacity's chunks); the pair's sum adds the icp_plane_chunks(Jp) of them that its own rows fill
__global__ __launch_bounds__(64) void info_finish_kernel(const double* __restrict__ part, int nch, int J, const int32_t* __restrict__ counts_src,
                                                         double* __restrict__ info, int32_t* __restrict__ count) {
  __shared__ double t[kInfoSums];
  const int pair = blockIdx.x;
  if (threadIdx.x < kInfoSums) {
    double s = 0.0;
    const int used = icp_plane_chunks(pair_rows(counts_src, pair, J));
    for (int c = 0; c < used; ++c) s += part[((int64_t)pair * nch + c) * kInfoSlots + threadIdx.x];   // chunk order
    t[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x >= 36) return;
  const int r = threadIdx.x / 6, c = threadIdx.x % 6, a = min(r, c), b = max(r, c);   // entry (a, b) of the upper triangle
  const double n = t[0], sx = t[1], sy = t[2], sz = t[3], sxx = t[4], syy = t[5], szz = t[6], sxy = t[7], sxz = t[8], syz = t[9];
  double v = 0.0;
  if (a == 0 && b == 0) v = syy + szz;
  else if (a == 1 && b == 1) v = sxx + szz;
  else if (a == 2 && b == 2) v = sxx + syy;
  else if (a == 0 && b == 1) v = -sxy;
  else if (a == 0 && b == 2) v = -sxz;
  else if (a == 1 && b == 2) v = -syz;
  else if (a == 0 && b == 4) v = -sz;
  else if (a == 0 && b == 5) v = sy;
  else if (a == 1 && b == 3) v = sz;
  else if (a == 1 && b == 5) v = -sx;
  else if (a == 2 && b == 3) v = -sy;
  else if (a == 2 && b == 4) v = sx;
  else if (a >= 3 && a == b) v = n;
  info[(int64_t)pair * 36 + threadIdx.x] = v == 0.0 ? 0.0 : v;   // no negative zero: the zero matrix is all-zero bytes
  if (threadIdx.x == 0) count[pair] = (int32_t)n;
}

}  // namespace

}  // namespace dsir

using namespace dsir;

// both entries: the checks under the entry's own `name`, the search of launch_icp_correspondences, the sums
static int info_entry(dsir_ctx* c, const char* name, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                      float max_corr_dist, const float* T, int search, double* info_out, int32_t* count_out, const int32_t* counts_src,
                      const int32_t* counts_ref) {
  Call call(c); if (call.refused()) return 1;
  if (!points_src || !points_ref || !T || !info_out || !count_out || pairs < 1 || J < 1 || K < 1 || stride < 3 || !(max_corr_dist > 0.f) ||
      (search != 0 && search != 1))
    return fail(c, "%s: bad arguments", name);
  if (search == 1 && (!icp_grid_radius_ok(max_corr_dist) || !icp_grid_shape_ok(pairs, J, K)))
    return fail(c, "%s: bad arguments (the grid search needs a max_corr_dist whose fp32 square is finite, and "
                   "pairs x J and pairs x K below 2^31)", name);
  IcpArgs a{};
  a.src = points_src; a.ref = points_ref; a.pairs = pairs; a.J = J; a.K = K; a.stride = stride; a.max_corr_dist = max_corr_dist;
  a.counts_src = counts_src; a.counts_ref = counts_ref;
  a.T_init = T; a.search = search == 1 ? IcpSearch::Grid : IcpSearch::Brute;
  const InfoLayout l(pairs, J, icp_corr_scratch_bytes(a));
  void* scratch = c->ws.raw(l.bytes);
  if (c->ws.overflow) return fail(c, "workspace too small for %s (raise max_points / max_pairs)", name);
  int32_t* idx = at<int32_t>(scratch, l.idx);
  if (const int e = launch_icp_correspondences(a, idx, at<float>(scratch, l.d2), nullptr, at<char>(scratch, l.corr), c->stream))
    return fail(c, "%s: the index build failed (HIP error %d)", name, e);
  const int nch = icp_plane_chunks(J);
  double* part = at<double>(scratch, l.part);
  hipLaunchKernelGGL(info_accum_kernel, dim3(nch, pairs), dim3(PT), 0, c->stream, points_ref, stride, (const int32_t*)idx, J, K, counts_src, counts_ref, part);
  hipLaunchKernelGGL(info_finish_kernel, dim3(pairs), dim3(64), 0, c->stream, (const double*)part, nch, J, counts_src, info_out, count_out);
  return call.finish();
}

extern "C" int dsir_information_matrix_ex(dsir_ctx* c, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                                          float max_corr_dist, const float* T, int search, double* info_out, int32_t* count_out,
                                          const int32_t* counts_src, const int32_t* counts_ref) {
  return info_entry(c, "dsir_information_matrix_ex", points_src, points_ref, pairs, J, K, stride, max_corr_dist, T, search, info_out, count_out,
                    counts_src, counts_ref);
}

extern "C" int dsir_information_matrix(dsir_ctx* c, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                                       float max_corr_dist, const float* T, int search, double* info_out, int32_t* count_out) {
  return info_entry(c, "dsir_information_matrix", points_src, points_ref, pairs, J, K, stride, max_corr_dist, T, search, info_out, count_out,
                    nullptr, nullptr);
}
