// Stand-alone host check of deepsir_amd/csrc/plane.h (the draw arithmetic of the plane segmentation, its pick key, the launch
// geometry, the limits and the scratch layout of dsir_segment_plane) under AddressSanitizer + UndefinedBehaviorSanitizer: host code
// only, runs on the CPU, no GPU and no Python loader involved.
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Ideepsir_amd/csrc tools/plane_check.cpp -o /tmp/plane_check && /tmp/plane_check
// (any host C++17 compiler with -fsanitize=address,undefined does as well.  The sanitizer run is this manual command;
// tests/test_plane_host.py builds the file as plain host C++, without a sanitizer, and runs it.)  Failures exit non-zero (no assert:
// the checks hold under NDEBUG too).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "plane.h"
using namespace dsir;

static int checks = 0;
#define CHECK(x) do { ++checks; if (!(x)) { std::fprintf(stderr, "plane_check: %s failed (line %d)\n", #x, __LINE__); std::exit(1); } } while (0)

int main() {
  // ---- splitmix64 against the published test vector (seed 0: the first three outputs of Vigna's splitmix64.c; the generator adds
  // the increment before mixing, so output i is mix(i * increment))
  const uint64_t inc = 0x9E3779B97F4A7C15ull;
  CHECK(plane_mix64(0) == 0xE220A8397B1DCDAFull);
  CHECK(plane_mix64(inc) == 0x6E789E6AA1B965F4ull);
  CHECK(plane_mix64(2 * inc) == 0x06C45D188009454Full);
  // ---- draws: hand values.  The cloud key folds the id at bit 40; the draw folds round, hypothesis and k at bits 32, 8 and 0.
  CHECK(plane_cloud_key(0, 0) == 0xE220A8397B1DCDAFull);
  CHECK(plane_cloud_key(5, 3) == plane_cloud_key(5 ^ (3ull << 40), 0));                 // cloud c of a batch is cloud 0 under seed ^ (c << 40)
  CHECK(plane_cloud_key(5, 3) != plane_cloud_key(5, 4));
  const uint64_t key = plane_cloud_key(12345, 7);
  for (uint32_t n : {1u, 2u, 3u, 100u, 5000u, 120000u, 0x7fffffffu}) {
    for (int j : {0, 1, 7})
      for (int h : {0, 1, 255, 256, 1023, (1 << 20) - 1})
        for (int k = 0; k < 3; ++k) {
          const uint64_t d = plane_mix64(key ^ ((uint64_t)j << 32) ^ ((uint64_t)h << 8) ^ (uint64_t)k);
          const uint32_t r = plane_draw(key, j, h, k, n);
          CHECK(r < n && r == (uint32_t)(((unsigned __int128)(d >> 32) * n) >> 32));
        }
  }
  CHECK(plane_draw(key, 0, 0, 0, 0) == 0);                                              // no live row: position 0, rejected by n_live < 3
  CHECK(plane_draw(0xE220A8397B1DCDAFull, 0, 0, 0, 1u << 31) == (uint32_t)((plane_mix64(0xE220A8397B1DCDAFull) >> 32) >> 1));
  // the fields do not overlap: the largest h stays below the round's bit
  CHECK(((uint64_t)(kPlaneMaxHyp - 1) << 8 | 2) < (1ull << 32) && kPlaneMaxPlanes - 1 < 256);
  // ---- the pick key: the larger count wins, ties to the LOWER h; never 0 for a scored hypothesis
  const uint32_t counts[] = {0u, 1u, 3u, 4999u, 0x7fffffffu}, hs[] = {0u, 1u, 511u, 512u, (1u << 20) - 1};
  for (uint32_t c : counts)
    for (uint32_t h : hs) {
      const unsigned long long k = plane_pick_key(c, h);
      CHECK(k != 0 && plane_key_count(k) == c && plane_key_h(k) == h);
      for (uint32_t c2 : counts)
        for (uint32_t h2 : hs) CHECK((k > plane_pick_key(c2, h2)) == (c > c2 || (c == c2 && h < h2)));
    }
  // ---- limits
  CHECK(plane_shape_ok(1, 1, 1) && plane_shape_ok(65535, 32768, 1 << 20));
  CHECK(!plane_shape_ok(0, 1, 1) && !plane_shape_ok(65536, 1, 1) && !plane_shape_ok(1, 0, 1) && !plane_shape_ok(65535, 32769, 1));
  CHECK(!plane_shape_ok(1, 1, 0) && !plane_shape_ok(1, 1, (1 << 20) + 1) && plane_shape_ok(1, 0x7fffffff, 1) && !plane_shape_ok(2, 0x40000000, 1));
  CHECK(kPlaneMaxPlanes == 8 && kPlaneMinInliers == 3 && kPlaneMaxRefits == 8 && kPlaneMaxClouds == 65535);
  // ---- geometry: every live position has a chunk, a slice and a refit slice; slices hold whole chunks
  const int caps[] = {1, 3, 255, 256, 257, 4095, 4096, 4097, 5000, 16384, 120000};
  for (int cap : caps)
    for (int clouds : {1, 8, 128})
      for (int H : {1, 64, 512, 513, 1024}) {
        const int hb = plane_hyp_blocks(H), cps = plane_chunks_per_slice(cap, hb, clouds), sl = plane_score_slices(cap, cps);
        CHECK(hb >= 1 && (long long)hb * kPlaneScoreCands >= H && (long long)(hb - 1) * kPlaneScoreCands < H);
        CHECK(cps >= 1 && sl >= 1 && (long long)sl * cps * kPlaneScoreLanes >= cap && (long long)(sl - 1) * cps * kPlaneScoreLanes < cap);
        CHECK(plane_row_blocks(cap) * kPlaneRowBlock >= cap && (plane_row_blocks(cap) - 1) * kPlaneRowBlock < cap);
        CHECK(plane_refit_slices(cap) * kPlaneRefitSlice >= cap && (plane_refit_slices(cap) - 1) * kPlaneRefitSlice < cap);
        // ---- the scratch layout: parts in order, aligned, disjoint, inside `bytes`; walk the ends of every part
        const PlaneLayout l(clouds, cap, H);
        const size_t C = (size_t)clouds;
        const struct { size_t off, len; } parts[] = {
            {l.pts4, C * cap * 16}, {l.live, C * cap * 4}, {l.blocks, C * l.row_blocks * 4}, {l.n_live, C * 4}, {l.done, C * 4},
            {l.hyp, C * H * 24}, {l.hyp_ok, C * H * 4}, {l.hyp_cnt, C * H * 4}, {l.info, C * 8}, {l.first_cnt, C * 4}, {l.cur, C * 24},
            {l.cur_cnt, C * 4}, {l.trial, C * 24}, {l.trial_cnt, C * 4}, {l.trial_ok, C * 4}, {l.kept, C * 4},
            {l.sum1, C * l.slices * 32}, {l.sum2, C * l.slices * 48}};
        CHECK(l.row_blocks == plane_row_blocks(cap) && l.slices == plane_refit_slices(cap) && l.bytes % 256 == 0);
        size_t end = 0;
        std::vector<unsigned char> buf(l.bytes);
        for (const auto& p : parts) {
          CHECK(p.off % 256 == 0 && p.off >= end && p.off + p.len <= l.bytes && p.len > 0);
          end = p.off + p.len;
          *at<unsigned char>(buf.data(), p.off) = 1;
          *at<unsigned char>(buf.data(), p.off + p.len - 1) = 1;
        }
      }
  std::printf("plane: %d checks passed\n", checks);
  return 0;
}
