// Robust loss kernels of the ICP estimators (icp.hip): the weight a correspondence enters the update with, as a function of its
// squared residual q = r^2 and the kernel's scale k > 0 - open3d's `robust_kernel` of TransformationEstimationPointToPoint/Plane.
// Plain C++ for the host and the device alike, no HIP types, so that the arithmetic can be exercised from a host-only program:
// tools/icp_robust_check.cpp, built with the address and undefined-behaviour sanitizers and run on the CPU (its header gives the
// command).  open3d is not installable here: parity is unpinned, THE RULE IS OWNED HERE, stated once more at the head of icp.hip and
// restated in tests/icp_robust_host.py.
//
//   l2     (0)  1                                   the least-squares estimator; the loop does not call this header for it
//   huber  (1)  q <= k^2 ? 1 : k / sqrt(q)
//   cauchy (2)  1 / (1 + q / k^2)
//   gm     (3)  k / ((k + q) * (k + q))             open3d's GMLoss
//   tukey  (4)  q <= k^2 ? (1 - q / k^2)^2 : 0
// (open3d's L1Loss is left out on purpose: its weight 1 / |r| is unbounded at an exact partner.)
//
// Every value is fp64 and every operation below is ONE correctly rounded IEEE operation in the order written: k^2 = k * k first
// (exact when k came from an fp32 value), then the quotient, the sum or the difference, then the square.  No product feeds a sum, so
// there is nothing a compiler could contract into an FMA, and numpy's float64 expressions in the same order give the same bits.
// Properties (checked by tools/icp_robust_check.cpp): every weight is in [0, max(1, 1/k)] and does not increase with q; huber and
// tukey are continuous at q = k^2 (1 and 0 there); a q that is not a number gives a weight that is not > 0 under every kernel (NaN, or
// tukey's 0) - the plane sums take a weight that is not > 0 as "contributes nothing".
//
// Point-to-point: icp_stats_kernel rounds the weight ONCE to fp32 and hands it to the weighted Kabsch kernel as it is.  A pair whose
// weights are ALL zero (tukey with every residual beyond k): S = sum |w| = 0, the normalised weights are 0 / 1e-16 = 0, both
// centroids and H are 0, H is finite, so kabsch_solve does NOT take its `bad` branch: svd3 of the zero matrix returns U = V = I,
// the Procrustes rotation is I, t = -I 0 + 0 = 0.  That update is the identity in value, but composing it is not the identity in
// bits: R P + t and R p + t add +0 terms, which turn an entry -0 of T or of a moved point into +0.  So the weighted loop does not
// rely on it: KabschArgs::zero_freeze makes the Kabsch kernels test S == 0 after the first pass (block-uniform: every thread holds
// the block's sum) and take the frozen step of a converged pair - T carried over bit for bit, the points untouched.  The l2 loop
// leaves zero_freeze at 0 and is, byte for byte, what it was.
#pragma once
#include <math.h>

#ifndef DSIR_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSIR_HD __host__ __device__
#else
#define DSIR_HD
#endif
#endif

namespace dsir {

enum IcpKernel : int { kIcpL2 = 0, kIcpHuber = 1, kIcpCauchy = 2, kIcpGM = 3, kIcpTukey = 4 };
constexpr int kIcpKernels = 5;

// kernel in 0..4 and (for a kernel other than l2) a finite scale > 0: what the entries refuse before any launch
DSIR_HD inline bool icp_robust_args_ok(int kernel, float scale) {
  if (kernel < 0 || kernel >= kIcpKernels) return false;
  if (kernel == kIcpL2) return true;
  return scale > 0.f && scale <= 3.4028234663852886e38f;   // false for NaN, inf, 0 and negatives
}

// the weight of a correspondence with squared residual q under `kernel` with scale k (the rule: this file's header)
DSIR_HD inline double icp_robust_weight(int kernel, double q, double k) {
  switch (kernel) {
    case kIcpHuber: {
      const double kk = k * k;
      if (q <= kk) return 1.0;
      const double r = sqrt(q);
      return k / r;
    }
    case kIcpCauchy: {
      const double kk = k * k;
      const double u = q / kk;
      const double d = 1.0 + u;
      return 1.0 / d;
    }
    case kIcpGM: {
      const double s = k + q;
      const double ss = s * s;
      return k / ss;
    }
    case kIcpTukey: {
      const double kk = k * k;
      if (!(q <= kk)) return 0.0;
      const double u = q / kk;
      const double t = 1.0 - u;
      return t * t;
    }
    default: return 1.0;
  }
}

}  // namespace dsir
