// Pose-graph optimisation with a line process (dsir_pose_graph_optimize): open3d's global_optimization (Choi, Zhou, Koltun, "Robust
// reconstruction of indoor scenes") for G graphs at once, ONE WORKGROUP PER GRAPH.  open3d is not installable here: parity is
// unpinned, THE RULE IS OWNED HERE and restated in numpy by deepsir_amd/pose_graph.py (optimize_host).  No cross-workgroup hand-off,
// no spin-wait, no atomics; every loop is bounded by max_iter or by a size, so a bad input ends in a status code, never in a hang.
//
// Conventions.  Node pose X_i (3 x 4, fp64) maps fragment i's frame to the scene frame.  Edge (s, t, T, Lambda, uncertain) says
// p_t = T p_s, so a consistent graph has X_s = X_t T.  With A = T^-1 X_t^-1 and E = A X_s the residual is
//   e = [log(R_E) ; t_E]    (6: the axis-angle vector of E's rotation, then E's translation column; Lambda's order [rotation; translation])
//   log(R): w = (R - R^T)v / 2, s = |w|, c = (tr R - 1) / 2, angle = atan2(s, c); log = w angle / s for s >= 1e-12, else w
//           (exact at the identity; a rotation by exactly pi reads as 0: the rule does not resolve that axis)
// Objective  F = sum_e l_e e^T Lambda e + sum_uncertain mu (sqrt(l_e) - 1)^2,  l_e = 1 for certain edges and
// l_e = (mu / (mu + e^T Lambda e))^2 for uncertain ones, re-evaluated at every accepted step and held fixed inside an iteration.
// Update  X_i <- exp(d_i) X_i  with d = [w ; v]:  R <- Exp(w) R,  t <- Exp(w) t + v  (Exp: Rodrigues).
// First-order Jacobians: e(d_s, d_t) ~ e + Js (d_s - d_t),  Js = [ R_A 0 ; -R_A [t_s]x  R_A ]  (the rotation block takes log's
// Jacobian as the identity: exact where e_rot = 0).  With W = Js^T (l Lambda) Js and g = Js^T (l Lambda) e:
//   H_ss += W, H_tt += W, H_st -= W, H_ts -= W, b_s += g, b_t -= g,   edges IN ORDER (no scatter-add: same bytes every run).
// reference_node's rows and columns are left out (n = 6 (N - 1) unknowns) and its pose keeps its input bits.
// Levenberg-Marquardt in fp64, Nielsen's damping:  lambda = 1e-3, nu = 2;  an iteration = one solve:
//   (H + lambda diag H) d = -b  by the blocked Cholesky below;  stop (status 0) if |d| <= 1e-6 sqrt(sum_free(|t_i|^2 + 1))
//   trial poses, F' with the l of this iteration, pred = d^T (lambda diag(H) d - b), rho = (F - F') / pred
//   accepted iff F' < F and pred > 0:  poses <- trial, l re-evaluated, F'' = F at the new l (<= F');
//       lambda *= max(1/3, 1 - (2 rho - 1)^3), nu = 2;  stop (status 0) if F - F'' <= 1e-6 F
//   rejected:  lambda *= nu, nu *= 2;  stop with kPgLambda if lambda > 1e12
//   stop with kPgMaxIter after max_iter solves.
// A pivot that is not positive (kPgPivot) or not finite (kPgNonFinite), an input entry that is not finite or a mu that is not
// positive (kPgNonFinite), an edge whose s or t is outside [0, N) or s == t (kPgEdgeIndex): that graph returns its INPUT poses,
// line = 1 and its status; the other graphs of the call are unaffected bit for bit (nothing is shared between workgroups).
// stats [G][4] = {F at the input poses, F at the returned poses, solves made, status}.
//
// The factorisation (the hot path: n^3 / 3 fp64 per solve on one workgroup): right-looking blocked Cholesky, panel of 32 columns.
// H and the factor L (n x n, row-major, lower triangle) live in global scratch (4.6 MB each at N = 128); per panel the 32 x 32
// diagonal block is factored in LDS, the rows below solve against it from registers (one row per thread), and the trailing update
// L22 -= L21 L21^T runs over 32 x 128 tiles whose panel rows are staged transposed in LDS, 4 x 4 results per thread, fp64 FMAs.
// The trailing update is plain vector FMA; v_mfma_f64_16x16x4_f64 was not built (profiles/README.md, "Pose graph").
#include "device_utils.h"
#include "engine_ctx.h"
#include "pose_graph.h"

namespace dsir {

namespace {

constexpr int PT = 256;                  // threads of the workgroup
constexpr int NB = kPoseGraphPanel;      // 32
constexpr int TJ = 128;                  // columns of a trailing-update tile
constexpr int LDD = NB + 1, LDI = NB + 4, LDJ = TJ + 4;
constexpr double kLambda0 = 1e-3, kLambdaMax = 1e12, kStopRel = 1e-6;

struct PgArgs {
  const int64_t* desc; const double* X0; const int32_t* st; const double* eT; const double* info; const uint8_t* unc; const double* mu;
  int max_iter; char* scratch; size_t ework;
  double* X; double* line; double* stats;
};

__device__ __forceinline__ bool pg_finite(double v) { return v - v == 0.0; }

__device__ void pg_log3(const double* R, double* w) {
  const double wx = 0.5 * (R[7] - R[5]), wy = 0.5 * (R[2] - R[6]), wz = 0.5 * (R[3] - R[1]);
  const double s = sqrt((wx * wx + wy * wy) + wz * wz), c = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
  const double k = s >= 1e-12 ? atan2(s, c) / s : 1.0;
  w[0] = wx * k; w[1] = wy * k; w[2] = wz * k;
}

__device__ void pg_exp3(const double* w, double* R) {
  const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], t = sqrt(t2);
  const double a = t >= 1e-8 ? sin(t) / t : 1.0, b = t >= 1e-8 ? (1.0 - cos(t)) / t2 : 0.5;
  const double x = w[0], y = w[1], z = w[2];
  R[0] = 1.0 - b * (y * y + z * z); R[1] = b * x * y - a * z;          R[2] = b * x * z + a * y;
  R[3] = b * x * y + a * z;         R[4] = 1.0 - b * (x * x + z * z);  R[5] = b * y * z - a * x;
  R[6] = b * x * z - a * y;         R[7] = b * y * z + a * x;          R[8] = 1.0 - b * (x * x + y * y);
}

// one edge at the poses Xs, Xt (3 x 4): w[0..5] = e, w[6..14] = R_A, w[15..23] = M = -R_A [t_s]x
__device__ void pg_edge(const double* Xs, const double* Xt, const double* T, double* w) {
  double RA[9], u[3], RE[9];
  for (int r = 0; r < 3; ++r)                   // R_A = R_T^T R_t^T: (r, c) = sum_k R_T[k][r] R_t[c][k]
    for (int c = 0; c < 3; ++c) RA[r * 3 + c] = (T[r] * Xt[c * 4] + T[4 + r] * Xt[c * 4 + 1]) + T[8 + r] * Xt[c * 4 + 2];
  for (int r = 0; r < 3; ++r)                   // u = R_t^T t_t + t_T
    u[r] = ((Xt[r] * Xt[3] + Xt[4 + r] * Xt[7]) + Xt[8 + r] * Xt[11]) + T[r * 4 + 3];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) RE[r * 3 + c] = (RA[r * 3] * Xs[c] + RA[r * 3 + 1] * Xs[4 + c]) + RA[r * 3 + 2] * Xs[8 + c];
    const double tA = -((T[r] * u[0] + T[4 + r] * u[1]) + T[8 + r] * u[2]);
    w[3 + r] = ((RA[r * 3] * Xs[3] + RA[r * 3 + 1] * Xs[7]) + RA[r * 3 + 2] * Xs[11]) + tA;
  }
  pg_log3(RE, w);
  const double tx = Xs[3], ty = Xs[7], tz = Xs[11];
  for (int r = 0; r < 3; ++r) {
    const double a = RA[r * 3], b = RA[r * 3 + 1], c = RA[r * 3 + 2];
    w[6 + r * 3] = a; w[7 + r * 3] = b; w[8 + r * 3] = c;
    // -(row of R_A) [t]x,  [t]x = [0 -tz ty; tz 0 -tx; -ty tx 0]
    w[15 + r * 3] = -(b * tz - c * ty); w[16 + r * 3] = -(c * tx - a * tz); w[17 + r * 3] = -(a * ty - b * tx);
  }
}

// Js (r, c) from an edge's work row
__device__ __forceinline__ double pg_js(const double* w, int r, int c) {
  if (r < 3) return c < 3 ? w[6 + r * 3 + c] : 0.0;
  return c < 3 ? w[15 + (r - 3) * 3 + c] : w[6 + (r - 3) * 3 + (c - 3)];
}

// Cholesky of the lower triangle of L (n x n, row-major) in place.  false: *s_fail holds kPgPivot or kPgNonFinite.
__device__ bool pg_factor(double* __restrict__ L, int n, double* sD, double* sPi, double* sPj, int* s_fail) {
  const int tid = threadIdx.x;
  for (int k0 = 0; k0 < n; k0 += NB) {
    const int kb = min(NB, n - k0), k1 = k0 + kb;
    for (int t = tid; t < NB * NB; t += PT) {                 // the diagonal block, padded with the identity
      const int r = t / NB, c = t % NB;
      sD[r * LDD + c] = (r < kb && c < kb) ? (c <= r ? L[(size_t)(k0 + r) * n + k0 + c] : 0.0) : (r == c ? 1.0 : 0.0);
    }
    __syncthreads();
    for (int j = 0; j < kb; ++j) {
      if (tid == 0) {
        const double d = sD[j * LDD + j];
        if (!(d > 0.0) || !pg_finite(d)) *s_fail = (d <= 0.0) ? kPgPivot : kPgNonFinite;
        else sD[j * LDD + j] = sqrt(d);
      }
      __syncthreads();
      if (*s_fail) return false;                              // block-uniform
      if (tid > j && tid < kb) sD[tid * LDD + j] /= sD[j * LDD + j];
      __syncthreads();
      for (int t = tid; t < NB * NB; t += PT) {
        const int r = t / NB, c = t % NB;
        if (c > j && r >= c && r < kb) sD[r * LDD + c] = fma(-sD[r * LDD + j], sD[c * LDD + j], sD[r * LDD + c]);
      }
      __syncthreads();
    }
    for (int t = tid; t < NB * NB; t += PT) {
      const int r = t / NB, c = t % NB;
      if (r < kb && c <= r) L[(size_t)(k0 + r) * n + k0 + c] = sD[r * LDD + c];
    }
    if (k1 >= n) { __syncthreads(); break; }
    // the rows below: x L11^T = a, one row per thread from registers (the identity padding makes every column the same code)
    for (int i = k1 + tid; i < n; i += PT) {
      double x[NB];
      double* row = L + (size_t)i * n + k0;
#pragma unroll
      for (int c = 0; c < NB; ++c) x[c] = c < kb ? row[c] : 0.0;
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        double v = x[c];
#pragma unroll
        for (int k = 0; k < c; ++k) v = fma(-x[k], sD[c * LDD + k], v);
        x[c] = v / sD[c * LDD + c];
      }
#pragma unroll
      for (int c = 0; c < NB; ++c)
        if (c < kb) row[c] = x[c];
    }
    __syncthreads();
    // trailing update of the lower triangle: tiles of 32 rows x 128 columns, 4 x 4 results per thread
    const int ti = (tid & 7) * 4, tj = (tid >> 3) * 4;
    for (int i0 = k1; i0 < n; i0 += NB) {
      for (int t = tid; t < NB * NB; t += PT) {               // sPi[k][r] = L[i0 + r][k0 + k]
        const int r = t / NB, k = t % NB;
        sPi[k * LDI + r] = (i0 + r < n && k < kb) ? L[(size_t)(i0 + r) * n + k0 + k] : 0.0;
      }
      for (int j0 = k1; j0 < i0 + NB && j0 < n; j0 += TJ) {
        for (int t = tid; t < NB * TJ; t += PT) {             // sPj[k][c] = L[j0 + c][k0 + k]
          const int c = t / NB, k = t % NB;
          sPj[k * LDJ + c] = (j0 + c < n && k < kb) ? L[(size_t)(j0 + c) * n + k0 + k] : 0.0;
        }
        __syncthreads();
        if (j0 + tj <= i0 + ti + 3 && i0 + ti < n && j0 + tj < n) {   // some (i, j <= i) of the 4 x 4 block exists
          double acc[4][4];
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
#pragma unroll 4
          for (int k = 0; k < NB; ++k) {
            double pa[4], pb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { pa[a] = sPi[k * LDI + ti + a]; pb[a] = sPj[k * LDJ + tj + a]; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
              for (int b = 0; b < 4; ++b) acc[a][b] = fma(pa[a], pb[b], acc[a][b]);
          }
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              const int i = i0 + ti + a, j = j0 + tj + b;
              if (i < n && j <= i) L[(size_t)i * n + j] -= acc[a][b];
            }
        }
        __syncthreads();
      }
    }
  }
  return true;
}

// L L^T d = -b with the factor of pg_factor: blocks of 32, the triangular block by wave 0 through shuffles.  sY: n doubles of LDS.
__device__ void pg_solve(const double* __restrict__ L, int n, const double* __restrict__ b, double* __restrict__ d, double* sY, double* sD,
                         double* sR) {
  const int tid = threadIdx.x, lane = tid & 63;
  for (int t = tid; t < n; t += PT) sY[t] = -b[t];
  __syncthreads();
  for (int k0 = 0; k0 < n; k0 += NB) {                         // L y = -b
    const int kb = min(NB, n - k0), k1 = k0 + kb;
    for (int t = tid; t < NB * NB; t += PT) {
      const int r = t / NB, c = t % NB;
      sD[r * LDD + c] = (r < kb && c <= r) ? L[(size_t)(k0 + r) * n + k0 + c] : (r == c ? 1.0 : 0.0);
    }
    __syncthreads();
    if (tid < 64) {
      double y = lane < kb ? sY[k0 + lane] : 0.0;
      for (int j = 0; j < kb; ++j) {
        const double yj = __shfl(y, j) / sD[j * LDD + j];
        if (lane == j) y = yj;
        else if (lane > j && lane < kb) y = fma(-sD[lane * LDD + j], yj, y);
      }
      if (lane < kb) sY[k0 + lane] = y;
    }
    __syncthreads();
    for (int i = k1 + tid; i < n; i += PT) {
      const double* row = L + (size_t)i * n + k0;
      double v = sY[i];
      for (int c = 0; c < kb; ++c) v = fma(-row[c], sY[k0 + c], v);
      sY[i] = v;
    }
    __syncthreads();
  }
  const int nblk = (n + NB - 1) / NB;
  for (int blk = nblk - 1; blk >= 0; --blk) {                  // L^T d = y
    const int k0 = blk * NB, kb = min(NB, n - k0), k1 = k0 + kb;
    for (int t = tid; t < NB * NB; t += PT) {
      const int r = t / NB, c = t % NB;
      sD[r * LDD + c] = (r < kb && c <= r) ? L[(size_t)(k0 + r) * n + k0 + c] : (r == c ? 1.0 : 0.0);
    }
    {                                                          // column c of the block: sum over the rows below, 8 partials in row order
      const int c = tid % NB, g = tid / NB;
      double v = 0.0;
      if (c < kb)
        for (int i = k1 + g; i < n; i += PT / NB) v = fma(L[(size_t)i * n + k0 + c], sY[i], v);
      sR[g * NB + c] = v;
    }
    __syncthreads();
    if (tid < 64) {
      double y = 0.0;
      if (lane < kb) {
        double s = 0.0;
        for (int g = 0; g < PT / NB; ++g) s += sR[g * NB + lane];
        y = sY[k0 + lane] - s;
      }
      for (int j = kb - 1; j >= 0; --j) {
        const double xj = __shfl(y, j) / sD[j * LDD + j];
        if (lane == j) y = xj;
        else if (lane < j) y = fma(-sD[j * LDD + lane], xj, y);
      }
      if (lane < kb) sY[k0 + lane] = y;
    }
    __syncthreads();
  }
  for (int t = tid; t < n; t += PT) d[t] = sY[t];
  __syncthreads();
}

__global__ __launch_bounds__(PT) void pose_graph_kernel(PgArgs A) {
  __shared__ double sD[NB * LDD], sPi[NB * LDI], sPj[NB * LDJ], sY[6 * kPoseGraphMaxNodes], sR[(PT / NB) * NB];
  __shared__ double sJ[36], sLam[36], sW[36], sG[6], sE[6];
  __shared__ double s_F, s_lambda, s_nu, s_rho;
  __shared__ int s_fail, s_badval, s_badidx, s_stop, s_accept, s_iter, s_status;
  const int tid = threadIdx.x, g = blockIdx.x;
  const int64_t* dsc = A.desc + (int64_t)g * kPoseGraphDescWords;
  const int64_t nb = dsc[0], eb = dsc[2];
  const int N = (int)dsc[1], E = (int)dsc[3], ref = (int)dsc[4], n = (int)dsc[5];
  auto part = [&](int k) { return reinterpret_cast<double*>(A.scratch + dsc[k]); };   // the graph's parts: byte offsets 6 .. 12
  double *H = part(6), *L = part(7), *bv = part(8), *Dv = part(9), *dl = part(10), *Xc = part(11), *Xt = part(12);
  double* ew = reinterpret_cast<double*>(A.scratch + A.ework) + eb * kPoseGraphEdgeDoubles;
  const double* X0 = A.X0 + nb * 12;
  const int32_t* st = A.st + eb * 2;
  const double* eT = A.eT + eb * 12;
  const double* info = A.info + eb * 36;
  const uint8_t* unc = A.unc + eb;
  const double mu = A.mu[g];
  double* Xo = A.X + nb * 12;
  double* line = A.line + eb;
  double* stats = A.stats + (int64_t)g * 4;

  if (tid == 0) { s_fail = 0; s_badval = 0; s_badidx = 0; s_stop = 0; s_accept = 0; s_iter = 0; s_status = 0; s_F = 0.0; }
  __syncthreads();
  // ---- the inputs: finite entries, a positive mu, edge indices inside the graph
  for (int t = tid; t < N * 12; t += PT) { Xc[t] = X0[t]; if (!pg_finite(X0[t])) s_badval = 1; }
  for (int t = tid; t < E * 12; t += PT) if (!pg_finite(eT[t])) s_badval = 1;
  for (int t = tid; t < E * 36; t += PT) if (!pg_finite(info[t])) s_badval = 1;
  for (int t = tid; t < E; t += PT) {
    const int s = st[t * 2], q = st[t * 2 + 1];
    if (s < 0 || s >= N || q < 0 || q >= N || s == q) s_badidx = 1;
  }
  if (tid == 0 && E > 0 && !(mu > 0.0 && pg_finite(mu))) s_badval = 1;
  __syncthreads();
  const int bad = (s_badval ? kPgNonFinite : 0) | (s_badidx ? kPgEdgeIndex : 0);
  double F0 = 0.0;
  int status = bad;
  if (!bad && n > 0 && E > 0) {
    // ---- residuals and line weights at the input poses
    for (int e = tid; e < E; e += PT) {
      double* w = ew + (size_t)e * kPoseGraphEdgeDoubles;
      pg_edge(Xc + st[e * 2] * 12, Xc + st[e * 2 + 1] * 12, eT + (size_t)e * 12, w);
      const double* Lm = info + (size_t)e * 36;
      double chi = 0.0;
      for (int r = 0; r < 6; ++r) {
        double v = 0.0;
        for (int c = 0; c < 6; ++c) v += Lm[r * 6 + c] * w[c];
        chi += w[r] * v;
      }
      const double q = unc[e] ? mu / (mu + chi) : 1.0;
      w[24] = chi; w[25] = q * q;
      w[26] = q * q * chi + (unc[e] ? mu * ((q - 1.0) * (q - 1.0)) : 0.0);
    }
    __syncthreads();
    if (tid == 0) {
      double F = 0.0;
      for (int e = 0; e < E; ++e) F += ew[(size_t)e * kPoseGraphEdgeDoubles + 26];    // edge order
      s_F = F; s_lambda = kLambda0; s_nu = 2.0;
      if (!pg_finite(F)) s_fail = kPgNonFinite;
    }
    __syncthreads();
    F0 = s_F;
    bool assemble = true;
    // ---- Levenberg-Marquardt: at most max_iter solves
    for (int it = 0; !s_fail && !s_stop; ++it) {
      if (it >= A.max_iter) { if (tid == 0) s_status |= kPgMaxIter; break; }
      if (assemble) {
        for (int t = tid; t < n * n; t += PT) H[t] = 0.0;
        for (int t = tid; t < n; t += PT) bv[t] = 0.0;
        __syncthreads();
        for (int e = 0; e < E; ++e) {                          // edges in order: every entry of H has one fixed summation order
          const double* w = ew + (size_t)e * kPoseGraphEdgeDoubles;
          if (tid < 36) { sJ[tid] = pg_js(w, tid / 6, tid % 6); sLam[tid] = w[25] * info[(size_t)e * 36 + tid]; }
          else if (tid < 42) sE[tid - 36] = w[tid - 36];
          __syncthreads();
          if (tid < 42) {
            // (Js^T Lam)(a, c) = sum_r Js[r][a] Lam[r][c]
            const int a = tid < 36 ? tid / 6 : tid - 36;
            double jl[6];
            for (int c = 0; c < 6; ++c) {
              double v = 0.0;
              for (int r = 0; r < 6; ++r) v += sJ[r * 6 + a] * sLam[r * 6 + c];
              jl[c] = v;
            }
            double v = 0.0;
            if (tid < 36) { const int bcol = tid % 6; for (int c = 0; c < 6; ++c) v += jl[c] * sJ[c * 6 + bcol]; sW[tid] = v; }
            else { for (int c = 0; c < 6; ++c) v += jl[c] * sE[c]; sG[a] = v; }
          }
          __syncthreads();
          const int s = st[e * 2], q = st[e * 2 + 1];
          const int cs = s == ref ? -1 : (s < ref ? s : s - 1) * 6, cq = q == ref ? -1 : (q < ref ? q : q - 1) * 6;
          if (tid < 144) {
            const int blk = tid / 36, a = (tid % 36) / 6, bcol = tid % 6;
            const int rb = (blk == 0 || blk == 2) ? cs : cq, cb = (blk == 0 || blk == 3) ? cs : cq;
            if (rb >= 0 && cb >= 0) {
              double* h = H + (size_t)(rb + a) * n + cb + bcol;
              *h = blk < 2 ? *h + sW[tid % 36] : *h - sW[tid % 36];
            }
          } else if (tid < 150) {
            if (cs >= 0) bv[cs + tid - 144] += sG[tid - 144];
          } else if (tid < 156) {
            if (cq >= 0) bv[cq + tid - 150] -= sG[tid - 150];
          }
          __syncthreads();
        }
        for (int t = tid; t < n; t += PT) Dv[t] = H[(size_t)t * n + t];
        __syncthreads();
      }
      {
        const double lam = s_lambda;
        for (int t = tid; t < n * n; t += PT) {
          const int r = t / n, c = t % n;
          if (c <= r) L[t] = r == c ? H[t] + lam * Dv[r] : H[t];
        }
        __syncthreads();
      }
      if (!pg_factor(L, n, sD, sPi, sPj, &s_fail)) break;
      pg_solve(L, n, bv, dl, sY, sD, sR);
      if (tid == 0) {
        s_iter = it + 1;
        double d2 = 0.0, sc = 0.0;
        for (int k = 0; k < n; ++k) d2 += dl[k] * dl[k];
        for (int i = 0; i < N; ++i)
          if (i != ref) sc += ((Xc[i * 12 + 3] * Xc[i * 12 + 3] + Xc[i * 12 + 7] * Xc[i * 12 + 7]) + Xc[i * 12 + 11] * Xc[i * 12 + 11]) + 1.0;
        if (!pg_finite(d2)) s_fail = kPgNonFinite;
        else if (sqrt(d2) <= kStopRel * sqrt(sc)) s_stop = 1;
      }
      __syncthreads();
      if (s_fail || s_stop) break;
      for (int i = tid; i < N; i += PT) {                      // trial poses
        const double* x = Xc + i * 12;
        double* y = Xt + i * 12;
        if (i == ref) { for (int k = 0; k < 12; ++k) y[k] = x[k]; continue; }
        const double* d = dl + (i < ref ? i : i - 1) * 6;
        double R[9];
        pg_exp3(d, R);
        for (int r = 0; r < 3; ++r) {
          for (int c = 0; c < 3; ++c) y[r * 4 + c] = (R[r * 3] * x[c] + R[r * 3 + 1] * x[4 + c]) + R[r * 3 + 2] * x[8 + c];
          y[r * 4 + 3] = ((R[r * 3] * x[3] + R[r * 3 + 1] * x[7]) + R[r * 3 + 2] * x[11]) + d[3 + r];
        }
      }
      __syncthreads();
      for (int e = tid; e < E; e += PT) {                      // the edges at the trial poses, the line weights held
        double* w = ew + (size_t)e * kPoseGraphEdgeDoubles;
        pg_edge(Xt + st[e * 2] * 12, Xt + st[e * 2 + 1] * 12, eT + (size_t)e * 12, w);
        const double* Lm = info + (size_t)e * 36;
        double chi = 0.0;
        for (int r = 0; r < 6; ++r) {
          double v = 0.0;
          for (int c = 0; c < 6; ++c) v += Lm[r * 6 + c] * w[c];
          chi += w[r] * v;
        }
        const double l = w[25], q = sqrt(l);
        w[24] = chi;
        w[26] = l * chi + (unc[e] ? mu * ((q - 1.0) * (q - 1.0)) : 0.0);
      }
      __syncthreads();
      if (tid == 0) {
        double Fn = 0.0, pred = 0.0;
        for (int e = 0; e < E; ++e) Fn += ew[(size_t)e * kPoseGraphEdgeDoubles + 26];
        for (int k = 0; k < n; ++k) pred += dl[k] * (s_lambda * Dv[k] * dl[k] - bv[k]);
        s_accept = (Fn < s_F && pred > 0.0) ? 1 : 0;           // false for a NaN on either side
        s_rho = s_accept ? (s_F - Fn) / pred : 0.0;
      }
      __syncthreads();
      if (s_accept) {
        for (int t = tid; t < N * 12; t += PT) Xc[t] = Xt[t];
        for (int e = tid; e < E; e += PT) {                    // the line process at the accepted poses
          double* w = ew + (size_t)e * kPoseGraphEdgeDoubles;
          const double chi = w[24], q = unc[e] ? mu / (mu + chi) : 1.0;
          w[25] = q * q;
          w[26] = q * q * chi + (unc[e] ? mu * ((q - 1.0) * (q - 1.0)) : 0.0);
        }
        __syncthreads();
        if (tid == 0) {
          double Fa = 0.0;
          for (int e = 0; e < E; ++e) Fa += ew[(size_t)e * kPoseGraphEdgeDoubles + 26];
          const double r = 2.0 * s_rho - 1.0, f = 1.0 - r * r * r;
          s_lambda *= f > 1.0 / 3.0 ? f : 1.0 / 3.0;
          s_nu = 2.0;
          if (s_F - Fa <= kStopRel * s_F) s_stop = 1;
          s_F = Fa;
        }
        assemble = true;
      } else {
        if (tid == 0) {
          s_lambda *= s_nu; s_nu *= 2.0;
          if (!(s_lambda <= kLambdaMax)) { s_status |= kPgLambda; s_stop = 1; }
        }
        assemble = false;
      }
      __syncthreads();
    }
    __syncthreads();
    status = s_status | s_fail;
  }
  // ---- results: a failed graph returns its input poses and line = 1
  const bool failed = (status & (kPgPivot | kPgNonFinite | kPgEdgeIndex)) != 0;
  const bool ran = !bad && n > 0 && E > 0;
  for (int t = tid; t < N * 12; t += PT) Xo[t] = (failed || !ran) ? X0[t] : Xc[t];
  for (int e = tid; e < E; e += PT) line[e] = (failed || !ran) ? 1.0 : ew[(size_t)e * kPoseGraphEdgeDoubles + 25];
  if (tid == 0) {
    stats[0] = F0; stats[1] = (failed || !ran) ? F0 : s_F; stats[2] = ran ? (double)s_iter : 0.0; stats[3] = (double)status;
  }
}

}  // namespace

}  // namespace dsir

using namespace dsir;

extern "C" size_t dsir_pose_graph_scratch_bytes(int graphs, const int32_t* node_off, const int32_t* edge_off, const int32_t* reference_node) {
  if (pose_graph_batch_refusal(graphs, node_off, edge_off, reference_node, nullptr)) return 0;
  return PoseGraphLayout(graphs, node_off, edge_off).bytes;
}

extern "C" int dsir_pose_graph_optimize(dsir_ctx* c, int graphs, const int32_t* node_off, const int32_t* edge_off, const double* X0,
                                        const int32_t* edge_st, const double* edge_T, const double* edge_info,
                                        const uint8_t* edge_uncertain, const double* mu, const int32_t* reference_node, int max_iter,
                                        void* scratch, double* X, double* line, double* stats) {
  Call call(c); if (call.refused()) return 1;
  int which = -1;
  const int why = pose_graph_batch_refusal(graphs, node_off, edge_off, reference_node, &which);
  if (why == kPgTooManyNodes)
    return fail(c, "dsir_pose_graph_optimize: graph %d has %d nodes, more than DSIR_POSE_GRAPH_MAX_NODES = %d", which,
                node_off[which + 1] - node_off[which], kPoseGraphMaxNodes);
  if (why == kPgNoEdges) return fail(c, "dsir_pose_graph_optimize: graph %d has several nodes and no edge (disconnected)", which);
  if (why == kPgBadReference) return fail(c, "dsir_pose_graph_optimize: graph %d: reference_node %d is not one of its nodes", which, reference_node[which]);
  if (why) return fail(c, "dsir_pose_graph_optimize: bad arguments (graphs, offsets or an empty graph)");
  if (!X0 || !mu || !scratch || !X || !line || !stats || max_iter < 0 ||
      (edge_off[graphs] > 0 && (!edge_st || !edge_T || !edge_info || !edge_uncertain)))
    return fail(c, "dsir_pose_graph_optimize: bad arguments");
  const PoseGraphLayout l(graphs, node_off, edge_off);
  std::vector<int64_t> desc((size_t)graphs * kPoseGraphDescWords, 0);
  l.fill_desc(graphs, node_off, edge_off, reference_node, desc.data());
  HIP_OK(c, hipMemcpyAsync(at<char>(scratch, l.desc), desc.data(), desc.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  HIP_OK(c, hipStreamSynchronize(c->stream));                   // `desc` is this call's own storage
  PgArgs a{};
  a.desc = at<int64_t>(scratch, l.desc); a.X0 = X0; a.st = edge_st; a.eT = edge_T; a.info = edge_info; a.unc = edge_uncertain; a.mu = mu;
  a.max_iter = max_iter; a.scratch = static_cast<char*>(scratch); a.ework = l.ework; a.X = X; a.line = line; a.stats = stats;
  hipLaunchKernelGGL(pose_graph_kernel, dim3(graphs), dim3(PT), 0, c->stream, a);
  return call.finish();
}
