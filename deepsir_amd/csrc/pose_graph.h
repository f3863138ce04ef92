// Pose-graph optimisation (pose_graph.hip): the sizes, the refusals and the scratch layout of a batch of graphs - plain C++ that
// compiles for the host alone, so that the arithmetic can be exercised from a host-only program: tools/pose_graph_check.cpp, built with
// the address and undefined-behaviour sanitizers and run on the CPU (its header gives the command).  The rule itself is stated in the
// header of pose_graph.hip and restated in deepsir_amd/pose_graph.py.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "scratch.h"

namespace dsir {

constexpr int kPoseGraphMaxNodes = 128;     // DSIR_POSE_GRAPH_MAX_NODES: the dense system is 6 (N - 1) <= 762 square
constexpr int kPoseGraphDescWords = 16;     // int64 per graph: node begin, N, edge begin, E, reference node, unknowns n, then the byte
                                            // offsets of H, L, b, D, delta, Xc, Xt (PoseGraphGraphLayout) in the scratch [6 .. 12], 3 spare
constexpr int kPoseGraphEdgeDoubles = 32;   // per edge: e (6), R_A (9), M = -R_A [t_s]x (9), chi [24], l [25], the edge's cost term [26], 5 spare
constexpr int kPoseGraphPanel = 32;         // columns of the factorisation's panel

// status bits of stats[g][3]; 0 = stopped on the relative decrease of F or on the relative step
enum PoseGraphStatus : int {
  kPgMaxIter = 1,        // max_iter solves were made
  kPgLambda = 2,         // the damping passed kPoseGraphLambdaMax
  kPgPivot = 4,          // a pivot of the factorisation was not positive: input poses returned
  kPgNonFinite = 8,      // an input entry, or a pivot, is not finite: input poses returned
  kPgEdgeIndex = 16,     // an edge names a node outside the graph, or s == t: input poses returned
};

// reasons the host refuses a batch for; 0 = accepted
enum PoseGraphRefusal : int { kPgOk = 0, kPgBadOffsets = 1, kPgTooManyNodes = 2, kPgNoNodes = 3, kPgNoEdges = 4, kPgBadReference = 5 };

inline int pose_graph_unknowns(int N) { return N < 1 ? 0 : 6 * (N - 1); }

// what the sizes of graph g alone decide (connectivity needs the edge list: deepsir_amd/pose_graph.py checks it before packing)
inline int pose_graph_refusal(int64_t N, int64_t E, int64_t reference_node) {
  if (N < 1) return kPgNoNodes;
  if (N > kPoseGraphMaxNodes) return kPgTooManyNodes;
  if (E < 0) return kPgBadOffsets;
  if (E == 0 && N > 1) return kPgNoEdges;
  if (reference_node < 0 || reference_node >= N) return kPgBadReference;
  return kPgOk;
}

// first refused graph of a batch given its offsets (host arrays of G + 1) and reference nodes: *which gets its index
inline int pose_graph_batch_refusal(int G, const int32_t* node_off, const int32_t* edge_off, const int32_t* reference_node, int* which) {
  if (which) *which = -1;
  if (G < 1 || !node_off || !edge_off || !reference_node || node_off[0] != 0 || edge_off[0] != 0) return kPgBadOffsets;
  for (int g = 0; g < G; ++g) {
    if (which) *which = g;
    if (node_off[g + 1] < node_off[g] || edge_off[g + 1] < edge_off[g]) return kPgBadOffsets;
    const int r = pose_graph_refusal((int64_t)node_off[g + 1] - node_off[g], (int64_t)edge_off[g + 1] - edge_off[g], reference_node[g]);
    if (r) return r;
  }
  if (which) *which = -1;
  return kPgOk;
}

// One piece of scratch for the batch.  Shared parts: the graphs' descriptors and the edges' work rows, in the batch's own CSR order.
// Per graph (every part on 256 bytes): H and the factor L, n x n each, then the vectors of n and the trial
// poses.  A graph's parts depend on its own N alone; its offset on the graphs before it.
struct PoseGraphGraphLayout {
  size_t H, L, b, D, delta, Xc, Xt, bytes;
  explicit PoseGraphGraphLayout(int N) {
    const size_t n = (size_t)pose_graph_unknowns(N), nn = n * n;
    Carve c;
    H = c.take(nn * 8);                    // sum J^T (l Lambda) J, undamped, both triangles
    L = c.take(nn * 8);                    // H + lambda diag H, factored in place (lower triangle)
    b = c.take(n * 8);
    D = c.take(n * 8);                     // diag H
    delta = c.take(n * 8);
    Xc = c.take((size_t)(N < 0 ? 0 : N) * 96);    // current poses [N][3][4]
    Xt = c.take((size_t)(N < 0 ? 0 : N) * 96);    // trial poses
    bytes = c.p;
  }
};

struct PoseGraphLayout {
  size_t desc, ework, graphs, bytes;
  // node_off / edge_off: host arrays of G + 1, already accepted by pose_graph_batch_refusal
  PoseGraphLayout(int G, const int32_t* node_off, const int32_t* edge_off) {
    Carve c;
    desc = c.take((size_t)G * kPoseGraphDescWords * sizeof(int64_t));
    ework = c.take((size_t)edge_off[G] * kPoseGraphEdgeDoubles * sizeof(double));
    graphs = c.p;
    size_t p = c.p;
    for (int g = 0; g < G; ++g) p += PoseGraphGraphLayout(node_off[g + 1] - node_off[g]).bytes;
    bytes = p;
  }
  // the graphs' descriptors as the kernel reads them (kPoseGraphDescWords int64 each): the one place a graph's parts get their
  // byte offsets, used by the launcher and laid out on the CPU by tools/pose_graph_check.cpp
  void fill_desc(int G, const int32_t* node_off, const int32_t* edge_off, const int32_t* reference_node, int64_t* desc) const {
    size_t off = graphs;
    for (int g = 0; g < G; ++g) {
      int64_t* d = desc + (size_t)g * kPoseGraphDescWords;
      const int N = node_off[g + 1] - node_off[g];
      const PoseGraphGraphLayout gl(N);
      for (int k = 0; k < kPoseGraphDescWords; ++k) d[k] = 0;
      d[0] = node_off[g]; d[1] = N; d[2] = edge_off[g]; d[3] = edge_off[g + 1] - edge_off[g]; d[4] = reference_node[g];
      d[5] = pose_graph_unknowns(N);
      const size_t parts[7] = {gl.H, gl.L, gl.b, gl.D, gl.delta, gl.Xc, gl.Xt};
      for (int k = 0; k < 7; ++k) d[6 + k] = (int64_t)(off + parts[k]);
      off += gl.bytes;
    }
  }
};

}  // namespace dsir
