// What augment.hip and resample.hip share: a cloud's parameters (deepsir_amd/augment.py::pack_params), its draw streams, the shapes taken.
#pragma once
#include <stdint.h>

namespace dsir {

constexpr uint64_t STREAM_PERM = 1ull << 40, STREAM_TOPUP = 2ull << 40, STREAM_JITTER = 3ull << 40;
struct AugParams {   // one cloud's parameter block: 24 eight-byte slots
  double R[9], t[3], s, jscale, jclip;
  int64_t jmode, centered, normals;
  uint64_t key;
  int64_t rmode, scaled, pad[3];
};
static_assert(sizeof(AugParams) == 24 * 8, "AugParams is 24 slots");

inline bool aug_shape_ok(int clouds, int cap, int stride) {
  return clouds >= 1 && cap >= 1 && stride >= 3 && (int64_t)clouds * cap <= 0x7fffffffll && clouds <= 65535;
}

}  // namespace dsir
