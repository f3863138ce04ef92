// Stand-alone host check of deepsir_amd/csrc/fps.h (the candidate key of the farthest-point sampling, the row-to-lane map, the tiers
// and the scratch layout of dsir_farthest_point_sample) under AddressSanitizer + UndefinedBehaviorSanitizer: host code only, runs on
// the CPU, no GPU and no Python loader involved.
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Ideepsir_amd/csrc tools/fps_check.cpp -o /tmp/fps_check && /tmp/fps_check
// (any host C++17 compiler with -fsanitize=address,undefined does as well.  The sanitizer run is this manual command;
// tests/test_fps_host.py builds the file as plain host C++, without a sanitizer, and runs it.)  Failures exit non-zero (no assert: the
// checks hold under NDEBUG too).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "fps.h"
using namespace dsir;

static int checks = 0;
#define CHECK(x) do { ++checks; if (!(x)) { std::fprintf(stderr, "fps_check: %s failed (line %d)\n", #x, __LINE__); std::exit(1); } } while (0)

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main() {
  // ---- the key: packs and unpacks; orders by dist first, then by the LOWER index; 0 stays below every candidate
  const float dists[] = {0.f, 1e-45f, 1e-30f, 0.5f, 1.f, 1.0000001f, 3e38f, INFINITY};
  const uint32_t rows[] = {0u, 1u, 63u, 64u, 1023u, 1024u, 8191u, 8192u, 65534u, 65535u};
  for (float d : dists)
    for (uint32_t i : rows) {
      const unsigned long long k = fps_key(bits(d), i);
      CHECK(fps_key_index(k) == i && fps_key_dist_bits(k) == bits(d) && k != 0);
      for (float e : dists)
        for (uint32_t j : rows) {
          const unsigned long long q = fps_key(bits(e), j);
          const bool wins = d > e || (d == e && i < j);     // the rule: larger dist, ties to the lower index
          CHECK((k > q) == wins && (k == q) == (d == e && i == j));
        }
    }
  CHECK(bits(INFINITY) == kFpsInfBits && kFpsStartBits == kFpsInfBits + 1);
  CHECK(fps_key(kFpsStartBits, 65535u) > fps_key(kFpsInfBits, 0u));           // `start` beats every finite row in step 0
  CHECK(fps_key(kFpsInfBits, 5u) > fps_key(kFpsInfBits, 6u));                 // else the lowest finite row
  // ---- tiers: a function of the capacity alone, every row has a slot, refusals
  CHECK(fps_plan(0).threads == 0 && fps_plan(-1).threads == 0 && fps_plan(kFpsMaxRows + 1).threads == 0);
  const int caps[] = {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000, 8191, 8192, 8193, 20000, 65535, 65536};
  for (int cap : caps) {
    const FpsPlan p = fps_plan(cap);
    CHECK(p.threads == 256 || p.threads == 1024);
    CHECK((long long)p.threads * p.slots >= cap && p.threads % 64 == 0);
    CHECK(p.stream == (cap > kFpsRegisterRows) && (p.threads == 256) == (cap <= kFpsSmallRows));
    CHECK(p.slots == (cap <= kFpsSmallRows ? 4 : cap <= kFpsRegisterRows ? 8 : 64));
    // ---- the row-to-lane map: a bijection between rows [0, T R) and (lane, slot); the owner of row i is (i % T, i / T)
    std::vector<unsigned char> seen((size_t)p.threads * p.slots, 0);
    for (int s = 0; s < p.slots; ++s)
      for (int l = 0; l < p.threads; ++l) {
        const int i = fps_row(l, s, p.threads);
        CHECK(i >= 0 && i < p.threads * p.slots && !seen[i] && i % p.threads == l && i / p.threads == s);
        seen[i] = 1;
      }
    // live slots: exactly the slots that hold a row below n
    for (int n : {0, 1, cap / 2, cap - 1, cap}) {
      const int live = fps_live_slots(n, p.threads);
      CHECK(live >= 0 && live <= p.slots && (long long)live * p.threads >= n && (live == 0 || (long long)(live - 1) * p.threads < n));
      if (p.stream) {
        const int ld = fps_stream_slots(live);
        CHECK(ld >= live && ld % kFpsStreamGroup == 0 && ld < live + kFpsStreamGroup && ld <= p.slots);
        CHECK((long long)ld * p.threads <= fps_stream_rows(cap));             // every slot the loop loads lies inside the cloud's slice
      }
    }
    // ---- the scratch layout: nothing for the register tiers; the packed copy, one slice per cloud, for the streaming tier
    for (int clouds : {1, 3, 128}) {
      const FpsLayout l(clouds, cap);
      if (!p.stream) { CHECK(l.bytes == 0 && l.xyz4 == 0); continue; }
      const size_t rows_c = (size_t)fps_stream_rows(cap);
      CHECK(rows_c >= (size_t)cap && rows_c % ((size_t)kFpsStreamGroup * 1024) == 0 && rows_c <= (size_t)kFpsMaxRows);
      CHECK(l.xyz4 % 256 == 0 && l.xyz4 + (size_t)clouds * rows_c * 16 <= l.bytes && l.bytes % 256 == 0);
      if (clouds > 3) continue;
      // walk the memory the way the kernel indexes it: cloud c, lane t, slot r at byte (c rows_c + t + 1024 r) 16
      std::vector<unsigned char> buf(l.bytes);
      float* q = at<float>(buf.data(), l.xyz4);
      const int slots = fps_stream_slots(fps_live_slots(cap, p.threads));
      for (int c = 0; c < clouds; ++c)
        for (int r = 0; r < slots; ++r)
          for (int t = 0; t < p.threads; t += 1023) q[((size_t)c * rows_c + (size_t)fps_row(t, r, p.threads)) * 4 + 3] = 1.f;
    }
  }
  std::printf("fps: %d checks passed\n", checks);
  return 0;
}
