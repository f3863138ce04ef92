// Stand-alone host check of deepsir_amd/csrc/scratch.h, csrc/op_layouts.h and csrc/fgr.h: the scratch layouts of select.hip,
// preprocess.hip, resample.hip, ransac.hip, consensus.hip, fgr.hip and match_targets.hip.  Every layout, at edge shapes: the parts start on 256 bytes, lie in
// declaration order, do not overlap and end inside `bytes`; and `bytes` equals the sum the operator's size function was written as
// before the layouts existed (spelled out below, term by term), with the library's temporary size an arbitrary number on both sides.
// Also csrc/search_plan.h's ExactScratch, the layout of the exact descriptor search (nn_match.hip, nn_topk.hip): its closed form and the
// byte counts of both size functions against recorded values.
// Host code only, runs on the CPU, no GPU and no Python loader.
//   hipcc -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ideepsir_amd/csrc \
//         tools/scratch_layout_check.cpp -o /tmp/scratch_layout_check && /tmp/scratch_layout_check
// (any host C++17 compiler does as well.  The sanitizer run is this manual command; tests/test_icp_search_host.py builds the file as
// plain host C++, without a sanitizer, and runs it.)  Failures exit non-zero (no assert: the checks hold under NDEBUG too).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fgr.h"
#include "op_layouts.h"
#include "search_plan.h"
using namespace dsir;

static long checks = 0;
#define CHECK(x) do { ++checks; if (!(x)) { std::fprintf(stderr, "scratch_layout_check: %s failed (line %d)\n", #x, __LINE__); std::exit(1); } } while (0)

static size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

// parts at[k] of need[k] bytes each, in declaration order, the first at `first`; the piece is `bytes` long
static void check_parts(const std::vector<size_t>& at, const std::vector<size_t>& need, size_t first, size_t bytes) {
  CHECK(at.size() == need.size() && at[0] == first);
  for (size_t k = 0; k < at.size(); ++k) {
    CHECK(at[k] % 256 == 0);
    const size_t end = at[k] + need[k];
    CHECK(end >= at[k]);                                               // no wrap
    CHECK(end <= (k + 1 < at.size() ? at[k + 1] : bytes));             // in order, no overlap, the last one inside the piece
  }
  CHECK(bytes % 256 == 0);
}

int main() {
  long shapes = 0;
  const size_t tmps[] = {0, 1, 255, 256, 257};
  const int counts[] = {1, 3, 1000}, lens[] = {1, 7, 256, 257}, Ms[] = {1, 63, 64, 65}, iters[] = {0, 2}, hyps[] = {1, 256}, partss[] = {4, 64};
  const int big_len = 715827882;                                       // 3 clouds of it: 2^31 - 2 elements
  const int64_t big = 0x7fffffffll;

  // ---- scratch.h
  {
    Carve c;
    CHECK(c.take(0) == 0 && c.p == 0 && c.take(1) == 0 && c.p == 256 && c.take(256) == 256 && c.take(257) == 512 && c.p == 1024);
    CHECK(align256(0) == 0 && align256(1) == 256 && align256(255) == 256 && align256(256) == 256 && align256(257) == 512);
    alignas(8) char buf[16] = {};
    const void* cbuf = buf;
    CHECK((char*)at<int32_t>((void*)buf, 8) == buf + 8 && (const char*)at<int64_t>(cbuf, 8) == buf + 8);
  }

  for (size_t tmp : tmps) {
    // ---- (clouds, per-cloud length): top-k, resample (both entries share the layout)
    std::vector<std::pair<int, int>> cl;
    for (int c : counts) for (int n : lens) cl.push_back({c, n});
    cl.push_back({3, big_len});
    for (auto [clouds, n] : cl) {
      const size_t total = (size_t)clouds * (size_t)n;
      ++shapes;
      const SegSortLayout t(clouds, n, 4, tmp);
      check_parts({t.k0, t.k1, t.v0, t.v1, t.seg, t.tmp}, {total * 4, total * 4, total * 4, total * 4, (size_t)(clouds + 1) * 4, tmp}, 0, t.bytes);
      CHECK(t.bytes == 4 * al(total * 4) + al((size_t)(clouds + 1) * 4) + al(tmp));
      const SegSortLayout r(clouds, n, 8, tmp);
      check_parts({r.k0, r.k1, r.v0, r.v1, r.seg, r.tmp}, {total * 8, total * 8, total * 4, total * 4, (size_t)(clouds + 1) * 4, tmp}, 0, r.bytes);
      CHECK(r.bytes == 2 * al(total * 8) + 2 * al(total * 4) + al((size_t)(clouds + 1) * 4) + al(tmp));
      // ---- voxel grid: `total` rows in all, the temporary the larger of the sort's and the scan's
      for (size_t scan : tmps) {
        const VoxelLayout v((int64_t)total, clouds, tmp, scan);
        const size_t C = (size_t)clouds, m = tmp > scan ? tmp : scan;
        check_parts({v.off, v.minb, v.k0, v.k1, v.v0, v.v1, v.head, v.ordinal, v.first, v.bad_row, v.tmp},
                    {(C + 1) * 8, C * 12, total * 8, total * 8, total * 4, total * 4, total * 4, total * 4, C * 4, 4, m}, 0, v.bytes);
        CHECK(v.tmp_bytes == m);
        CHECK(v.bytes == al((C + 1) * 8) + al(C * 3 * 4) + 2 * al(total * 8) + 2 * al(total * 4) + 2 * al(total * 4) + al(C * 4) + al(4) + al(m));
      }
      // ---- scatter plan and match keys: one flat count
      const ScatterPlanLayout s((int64_t)total, tmp);
      check_parts({s.k0, s.k1, s.v0, s.tmp}, {total * 4, total * 4, total * 4, tmp}, 0, s.bytes);
      CHECK(s.bytes == 3 * al(total * 4) + al(tmp));
      const BufferTmpLayout k(total * sizeof(int64_t), tmp);
      check_parts({k.buf, k.tmp}, {total * 8, tmp}, 0, k.bytes);
      CHECK(k.bytes == al(total * 8) + al(tmp));
      // ---- radius matches: rows x parts counts, the scan's temporary
      for (int parts : partss) {
        const BufferTmpLayout m(total * parts * sizeof(int32_t), tmp);
        check_parts({m.buf, m.tmp}, {total * parts * 4, tmp}, 0, m.bytes);
        CHECK(m.bytes == al(total * parts * 4) + al(tmp));
      }
    }
    {
      const ScatterPlanLayout s(big, tmp);
      const BufferTmpLayout k((size_t)big * 8, tmp);
      const VoxelLayout v(big, 3, tmp, 0);
      CHECK(s.bytes == 3 * al((size_t)big * 4) + al(tmp) && k.bytes == al((size_t)big * 8) + al(tmp) && v.tmp + al(tmp) == v.bytes);
    }

    // ---- the pose stages: (pairs, M, refine_iters) and the hypotheses / seeds
    std::vector<std::pair<int, int>> pm;
    for (int p : counts) for (int M : Ms) pm.push_back({p, M});
    pm.push_back({65535, 32767});                                      // 2^31 - 98303 correspondences
    for (auto [pairs, M] : pm) for (int R : iters) for (int H : hyps) {
      ++shapes;
      const size_t P = (size_t)pairs, W = (size_t)(M + 63) / 64;
      const PoseLayout po(pairs, M, R);
      const std::vector<size_t> pose_at = {po.cs, po.cq, po.w, po.Tcand, po.cnt, po.info};
      const std::vector<size_t> pose_need = {P * M * 12, P * M * 12, P * M * 4, P * (R + 1) * 48, P * (R + 1) * 4, P * 16};
      check_parts(pose_at, pose_need, 0, po.bytes);
      const size_t pose = 2 * al(P * M * 12) + al(P * M * 4) + al(P * (R + 1) * 48) + al(P * (R + 1) * 4) + al(P * 16);
      CHECK(po.bytes == pose);

      const RansacLayout ra(pairs, M, H, R);
      CHECK(ra.pose.cs == po.cs && ra.pose.info == po.info && ra.pose.bytes == po.bytes);
      check_parts({ra.hyp.T, ra.hyp.valid, ra.hyp.count}, {P * H * 48, P * H * 4, P * H * 4}, po.bytes, ra.bytes);
      CHECK(ra.bytes == pose + al(P * H * 48) + 2 * al(P * H * 4));

      const ConsensusLayout co(pairs, M, H, R, tmp);
      CHECK(co.pose.cs == po.cs && co.pose.info == po.info && co.pose.bytes == po.bytes);
      check_parts({co.bits, co.score, co.k0, co.k1, co.seg, co.tmp, co.seed, co.hyp.T, co.hyp.valid, co.hyp.count},
                  {P * M * W * 8, P * M * 4, P * M * 8, P * M * 8, (P + 1) * 4, tmp, P * H * 4, P * H * 48, P * H * 4, P * H * 4}, po.bytes, co.bytes);
      CHECK(co.bytes == pose + al(P * M * W * 8) + al(P * M * 4) + 2 * al(P * M * 8) + al((P + 1) * 4) + al(tmp) + al(P * H * 4) + al(P * H * 48) +
                            2 * al(P * H * 4));

      // FGR: H as max_tuples, a trial cap below and above 100 x M; one candidate pose per pair
      for (int tt = 0; tt < 2; ++tt) for (int trials : {300, 1 << 20}) {
        const FgrLayout fg(pairs, M, tt, H, trials, R, tmp);
        const size_t L = tt ? (size_t)3 * H : (size_t)M;
        const size_t cand = tt ? (size_t)((int64_t)100 * M < trials ? 100 * M : trials) : (size_t)M, NB = (cand + 255) / 256;
        CHECK(fg.pose.cs == po.cs && fg.pose.info == po.info && fg.pose.bytes == po.bytes);
        check_parts({fg.rows, fg.blk_cnt, fg.blk_pre, fg.tmp, fg.npts, fg.hyp.T, fg.hyp.valid, fg.hyp.count},
                    {P * L * 4, P * NB * 4, P * NB * 4, tmp, P * L * 48, P * 48, P * 4, P * 4}, po.bytes, fg.bytes);
        CHECK(fg.bytes == pose + al(P * L * 4) + 2 * al(P * NB * 4) + al(tmp) + al(P * L * 48) + al(P * 48) + 2 * al(P * 4));
      }
    }
  }

  // ---- the exact descriptor search (search_plan.h): sa | sb | pad to 4 floats | tail of 8-byte words - a closed form of its own, no
  // 256-byte parts.  {P, J, K} and the bytes nn_match_scratch_bytes / nn_topk_scratch_bytes (k = 1, 4, 8) gave when each spelled the
  // layout out itself.
  const struct { int P, J, K; size_t match, topk1, topk4, topk8; } ex[] = {
      {1, 5000, 5000, 80000ull, 600000ull, 1160000ull, 2280000ull},
      {2, 5000, 5000, 160000ull, 720000ull, 1360000ull, 2640000ull},
      {128, 5000, 5000, 10240000ull, 15360000ull, 25600000ull, 46080000ull},
      {256, 5000, 5000, 20480000ull, 30720000ull, 51200000ull, 92160000ull},
      {1, 1, 1, 24ull, 32ull, 48ull, 80ull},
      {1, 70, 63, 1104ull, 1664ull, 2784ull, 5024ull},
      {128, 129, 70, 233984ull, 366080ull, 630272ull, 1158656ull},
      {64, 385, 70, 313600ull, 510720ull, 904960ull, 1693440ull},
      {1, 5000, 511, 62048ull, 102048ull, 182048ull, 342048ull},
      {1, 5000, 512, 62048ull, 102048ull, 182048ull, 342048ull},
      {1, 5000, 513, 62064ull, 102064ull, 182064ull, 342064ull},
      {1, 5000, 1023, 64096ull, 184096ull, 344096ull, 664096ull},
      {1, 5000, 1024, 64096ull, 184096ull, 344096ull, 664096ull},
      {1, 5000, 1025, 64112ull, 184112ull, 344112ull, 664112ull},
      {128, 5000, 511, 7941632ull, 13061632ull, 23301632ull, 43781632ull},
      {128, 5000, 512, 7942144ull, 13062144ull, 23302144ull, 43782144ull},
      {128, 5000, 513, 7942656ull, 13062656ull, 23302656ull, 43782656ull},
      {128, 5000, 1023, 8203776ull, 13323776ull, 23563776ull, 44043776ull},
      {128, 5000, 1024, 8204288ull, 13324288ull, 23564288ull, 44044288ull},
      {128, 5000, 1025, 8204800ull, 13324800ull, 23564800ull, 44044800ull},
      {4096, 1 << 20, 1 << 20, 68719476736ull, 103079215104ull, 171798691840ull, 309237645312ull},
  };
  for (const auto& e : ex) {
    ++shapes;
    const size_t PJ = (size_t)e.P * e.J, PK = (size_t)e.P * e.K;
    for (size_t tail_bytes : {(size_t)0, (size_t)8, PJ * 8}) {
      const ExactScratch L(e.P, e.J, e.K, tail_bytes);
      CHECK(L.sa == 0 && L.sb == L.sa + PJ * 4 && L.tail >= L.sb + PK * 4 && L.tail < L.sb + PK * 4 + 16);   // ascending, the pad below 4 floats
      CHECK(L.tail % 8 == 0 && L.tail % 16 == 0);
      CHECK(L.bytes == ((PJ + PK + 3) & ~(size_t)3) * 4 + tail_bytes && L.bytes == L.tail + tail_bytes);
    }
    CHECK(nn_match_scratch(e.P, e.J, e.K).bytes == e.match);
    CHECK(nn_topk_scratch(e.P, e.J, e.K, 1).bytes == e.topk1 && nn_topk_scratch(e.P, e.J, e.K, 2).bytes == e.topk1);
    CHECK(nn_topk_scratch(e.P, e.J, e.K, 3).bytes == e.topk4 && nn_topk_scratch(e.P, e.J, e.K, 4).bytes == e.topk4);
    CHECK(nn_topk_scratch(e.P, e.J, e.K, 5).bytes == e.topk8 && nn_topk_scratch(e.P, e.J, e.K, 8).bytes == e.topk8);
    CHECK(nn_match_scratch(e.P, e.J, e.K).tail == nn_topk_scratch(e.P, e.J, e.K, 8).tail);
  }
  std::printf("scratch_layout: %ld checks passed, %ld shapes laid out\n", checks, shapes);
  return 0;
}
