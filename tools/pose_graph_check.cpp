// Host-only check of csrc/pose_graph.h: the scratch sizes, the parts' offsets and the refusal arithmetic of
// dsir_pose_graph_optimize for N in 1 .. 129 and ragged batches, under the address and undefined-behaviour sanitizers on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ideepsir_amd/csrc tools/pose_graph_check.cpp \
//       -o /tmp/pose_graph_check && /tmp/pose_graph_check
// Every part of a layout is written through, as the kernel would, into a buffer of exactly `bytes`: an overlap or an overrun is a
// sanitizer report or a failed check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pose_graph.h"

using namespace dsir;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static int check_batch(const std::vector<int>& Ns, const std::vector<int>& Es) {
  const int G = (int)Ns.size();
  std::vector<int32_t> no(G + 1, 0), eo(G + 1, 0), rf(G, 0);
  for (int g = 0; g < G; ++g) { no[g + 1] = no[g] + Ns[g]; eo[g + 1] = eo[g] + Es[g]; rf[g] = Ns[g] - 1; }
  int which = -2;
  CHECK(pose_graph_batch_refusal(G, no.data(), eo.data(), rf.data(), &which) == kPgOk && which == -1);
  const PoseGraphLayout l(G, no.data(), eo.data());
  std::vector<unsigned char> buf(l.bytes, 0);
  auto fill = [&](size_t off, size_t bytes, unsigned char tag) {           // every byte of a part must be unclaimed
    for (size_t k = 0; k < bytes; ++k) { if (buf.at(off + k) != 0) return false; buf[off + k] = tag; }
    return true;
  };
  CHECK(l.desc % 256 == 0 && l.ework % 256 == 0 && l.graphs % 256 == 0);
  CHECK(fill(l.desc, (size_t)G * kPoseGraphDescWords * 8, 1));
  CHECK(fill(l.ework, (size_t)eo[G] * kPoseGraphEdgeDoubles * 8, 2));
  std::vector<int64_t> desc((size_t)G * kPoseGraphDescWords, -1);
  l.fill_desc(G, no.data(), eo.data(), rf.data(), desc.data());            // the descriptors the launcher uploads and the kernel reads
  size_t off = l.graphs;
  for (int g = 0; g < G; ++g) {
    const int64_t* d = desc.data() + (size_t)g * kPoseGraphDescWords;
    const PoseGraphGraphLayout gl(Ns[g]);
    const size_t n = (size_t)pose_graph_unknowns(Ns[g]);
    CHECK(n == (size_t)6 * (Ns[g] - 1) && n <= 762);
    CHECK(d[0] == no[g] && d[1] == Ns[g] && d[2] == eo[g] && d[3] == Es[g] && d[4] == rf[g] && d[5] == (int64_t)n);
    const size_t sizes[7] = {n * n * 8, n * n * 8, n * 8, n * 8, n * 8, (size_t)Ns[g] * 96, (size_t)Ns[g] * 96};
    for (int k = 0; k < 7; ++k) {
      const size_t at_ = (size_t)d[6 + k];
      CHECK(at_ % 256 == 0 && at_ >= off && at_ + sizes[k] <= off + gl.bytes);
      CHECK(fill(at_, sizes[k], (unsigned char)(3 + k)));                  // every byte of a part unclaimed: no overlap, no overrun
    }
    off += gl.bytes;
  }
  CHECK(off == l.bytes);
  return 0;
}

int main() {
  for (int N = 1; N <= 129; ++N) {
    const int E = N == 1 ? 0 : 2 * N;
    CHECK(pose_graph_refusal(N, E, 0) == (N <= kPoseGraphMaxNodes ? kPgOk : kPgTooManyNodes));
    CHECK(pose_graph_refusal(N, E, N) == (N <= kPoseGraphMaxNodes ? kPgBadReference : kPgTooManyNodes));
    CHECK(pose_graph_refusal(N, E, -1) == (N <= kPoseGraphMaxNodes ? kPgBadReference : kPgTooManyNodes));
    if (N > 1 && N <= kPoseGraphMaxNodes) CHECK(pose_graph_refusal(N, 0, 0) == kPgNoEdges);
    if (N <= kPoseGraphMaxNodes && check_batch({N}, {E})) return 1;
  }
  CHECK(pose_graph_refusal(0, 0, 0) == kPgNoNodes && pose_graph_refusal(1, 0, 0) == kPgOk && pose_graph_refusal(2, -1, 0) == kPgBadOffsets);
  CHECK(PoseGraphGraphLayout(128).H == 0 && PoseGraphGraphLayout(128).L >= (size_t)762 * 762 * 8);
  if (check_batch({1, 128, 2, 7, 60, 1}, {0, 400, 1, 9, 400, 0})) return 1;     // ragged
  if (check_batch({128, 128, 128, 128, 128, 128, 128, 128}, {1000, 1, 5, 127, 400, 400, 400, 8128})) return 1;
  {  // refusals of a batch name the graph
    int32_t no[4] = {0, 7, 136, 140}, eo[4] = {0, 6, 200, 205}, rf[3] = {0, 0, 0};
    int which = -1;
    CHECK(pose_graph_batch_refusal(3, no, eo, rf, &which) == kPgTooManyNodes && which == 1);
    no[2] = 135; no[3] = 139; rf[2] = 4;
    CHECK(pose_graph_batch_refusal(3, no, eo, rf, &which) == kPgBadReference && which == 2);
    rf[2] = 3; eo[3] = 200;
    CHECK(pose_graph_batch_refusal(3, no, eo, rf, &which) == kPgNoEdges && which == 2);
    eo[3] = 199;
    CHECK(pose_graph_batch_refusal(3, no, eo, rf, &which) == kPgBadOffsets);
    no[0] = 1;
    CHECK(pose_graph_batch_refusal(3, no, eo, rf, &which) == kPgBadOffsets);
    CHECK(pose_graph_batch_refusal(0, no, eo, rf, &which) == kPgBadOffsets && pose_graph_batch_refusal(1, nullptr, eo, rf, &which) == kPgBadOffsets);
  }
  std::printf("pose_graph_check: ok\n");
  return 0;
}
