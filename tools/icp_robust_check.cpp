// Stand-alone host check of deepsir_amd/csrc/icp_robust.h (the weights of the robust loss kernels of dsir_icp_refine_ex4 and the
// argument test of the entry) under AddressSanitizer + UndefinedBehaviorSanitizer: host code only, runs on the CPU, no GPU and no
// Python loader involved.
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Ideepsir_amd/csrc tools/icp_robust_check.cpp -o /tmp/icp_robust_check && /tmp/icp_robust_check
// (any host C++17 compiler with -fsanitize=address,undefined does as well.  The sanitizer run is this manual command;
// tests/test_icp_robust_host.py builds the file as plain host C++, without a sanitizer, and runs it.)
// Failures exit non-zero (no assert: the checks hold under NDEBUG too).
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include "icp_robust.h"
using namespace dsir;

static int checks = 0;
#define CHECK(x) do { ++checks; if (!(x)) { std::fprintf(stderr, "icp_robust_check: %s failed (line %d)\n", #x, __LINE__); std::exit(1); } } while (0)

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const float scales[] = {1e-6f, 0.03f, 0.08f, 1.0f, 250.0f};
  for (const float kf : scales) {
    const double k = (double)kf, kk = k * k;
    // q = 0: the weight of an exact partner
    CHECK(icp_robust_weight(kIcpL2, 0.0, k) == 1.0);
    CHECK(icp_robust_weight(kIcpHuber, 0.0, k) == 1.0);
    CHECK(icp_robust_weight(kIcpCauchy, 0.0, k) == 1.0);
    CHECK(icp_robust_weight(kIcpGM, 0.0, k) == k / (k * k));
    CHECK(icp_robust_weight(kIcpTukey, 0.0, k) == 1.0);
    // q = k^2 and the next doubles on either side of it
    const double below = std::nextafter(kk, 0.0), above = std::nextafter(kk, inf);
    CHECK(icp_robust_weight(kIcpHuber, below, k) == 1.0 && icp_robust_weight(kIcpHuber, kk, k) == 1.0);
    const double h_above = icp_robust_weight(kIcpHuber, above, k);
    CHECK(h_above <= 1.0 && h_above > 1.0 - 1e-15);                       // continuous at k: 1 on the inside, k / sqrt(q) -> 1 outside
    CHECK(icp_robust_weight(kIcpTukey, kk, k) == 0.0 && icp_robust_weight(kIcpTukey, above, k) == 0.0);
    const double t_below = icp_robust_weight(kIcpTukey, below, k);
    CHECK(t_below >= 0.0 && t_below < 1e-30);                             // continuous at k: (1 - q / k^2)^2 -> 0 on the inside
    CHECK(icp_robust_weight(kIcpCauchy, kk, k) == 0.5);
    CHECK(icp_robust_weight(kIcpGM, kk, k) == k / ((k + kk) * (k + kk)));
    // huge, denormal and non-finite q: finite weights in [0, max], never negative; NaN is never > 0
    const double odd[] = {DBL_MIN, 4.9406564584124654e-324, 1e-310, 1e300, DBL_MAX, inf};
    for (int kern = kIcpL2; kern <= kIcpTukey; ++kern) {
      const double top = icp_robust_weight(kern, 0.0, k);
      for (const double q : odd) {
        const double w = icp_robust_weight(kern, q, k);
        CHECK(w >= 0.0 && w <= top);
      }
      if (kern != kIcpL2) CHECK(!(icp_robust_weight(kern, nan, k) > 0.0));
      // the weight does not increase with q: a geometric sweep over 600 decades, and neighbouring doubles around k^2
      double prev = top;
      for (int e = -3000; e <= 3000; ++e) {
        const double q = std::pow(10.0, e / 10.0);
        const double w = icp_robust_weight(kern, q, k);
        CHECK(w <= prev && w >= 0.0);
        prev = w;
      }
      double q = kk;
      for (int s = 0; s < 64; ++s) q = std::nextafter(q, 0.0);
      prev = icp_robust_weight(kern, q, k);
      for (int s = 0; s < 128; ++s) {
        q = std::nextafter(q, inf);
        const double w = icp_robust_weight(kern, q, k);
        CHECK(w <= prev);
        prev = w;
      }
    }
    // far outside: huber decays like k / r, tukey is exactly 0, cauchy and gm tend to 0
    CHECK(std::fabs(icp_robust_weight(kIcpHuber, 4.0 * kk, k) - 0.5) < 1e-15);
    CHECK(icp_robust_weight(kIcpTukey, 4.0 * kk, k) == 0.0);
    CHECK(icp_robust_weight(kIcpCauchy, 1e300, k) < 1e-280 && icp_robust_weight(kIcpGM, 1e300, k) == 0.0);
  }
  // an unknown kernel number weighs like l2 (the entries refuse it before any launch)
  CHECK(icp_robust_weight(7, 3.0, 0.1) == 1.0 && icp_robust_weight(-1, 3.0, 0.1) == 1.0);

  // what the entries refuse
  const float finf = std::numeric_limits<float>::infinity(), fnan = std::numeric_limits<float>::quiet_NaN();
  CHECK(!icp_robust_args_ok(-1, 1.f) && !icp_robust_args_ok(5, 1.f) && !icp_robust_args_ok(kIcpKernels, 1.f));
  for (int kern = kIcpHuber; kern <= kIcpTukey; ++kern) {
    CHECK(icp_robust_args_ok(kern, 0.05f) && icp_robust_args_ok(kern, FLT_MAX) && icp_robust_args_ok(kern, FLT_MIN));
    CHECK(!icp_robust_args_ok(kern, 0.f) && !icp_robust_args_ok(kern, -0.f) && !icp_robust_args_ok(kern, -1.f));
    CHECK(!icp_robust_args_ok(kern, fnan) && !icp_robust_args_ok(kern, finf) && !icp_robust_args_ok(kern, -finf));
  }
  CHECK(icp_robust_args_ok(kIcpL2, 0.f) && icp_robust_args_ok(kIcpL2, fnan) && icp_robust_args_ok(kIcpL2, -finf));   // l2 ignores it
  std::printf("icp_robust: %d checks passed\n", checks);
  return 0;
}
