// The scratch of select.hip, preprocess.hip, resample.hip, ransac.hip, consensus.hip and match_targets.hip as offsets into one piece
// each (fgr.hip's, over the same head and candidate part, is in fgr.h): built from the operator's shape (and, where a library call needs temporary space, that size), read by the size function and
// the launcher alike.  Plain host C++ on the model of icp_layout.h: tools/scratch_layout_check.cpp lays every one out on the CPU.
#pragma once
#include "scratch.h"

namespace dsir {

// launch_topk (4-byte keys), launch_resample and dsir_t_resample_keyed (8-byte, 63-bit keys): (key, 4-byte value) ping and pong of a
// sort of `segments` segments of `len`, its offsets, its temporary
struct SegSortLayout {
  size_t k0, k1, v0, v1, seg, tmp, bytes;
  SegSortLayout(int segments, int len, size_t key_bytes, size_t sort_tmp) {
    const size_t total = (size_t)segments * (size_t)len;
    Carve c;
    k0 = c.take(total * key_bytes); k1 = c.take(total * key_bytes); v0 = c.take(total * 4); v1 = c.take(total * 4);
    seg = c.take((size_t)(segments + 1) * 4);
    tmp = c.take(sort_tmp);
    bytes = c.p;
  }
};

struct ScatterPlanLayout {   // launch_scatter_plan: the sorted values go straight to `order`
  size_t k0, k1, v0, tmp, bytes;
  ScatterPlanLayout(int64_t total, size_t sort_tmp) {
    Carve c;
    k0 = c.take((size_t)total * 4); k1 = c.take((size_t)total * 4); v0 = c.take((size_t)total * 4);
    tmp = c.take(sort_tmp);
    bytes = c.p;
  }
};

struct VoxelLayout {         // launch_voxel_downsample: the sort, then the scan, run in the same temporary
  size_t off, minb, k0, k1, v0, v1, head, ordinal, first, bad_row, tmp, tmp_bytes, bytes;
  VoxelLayout(int64_t total, int clouds, size_t sort_tmp, size_t scan_tmp) {
    const size_t n = (size_t)total, C = (size_t)clouds;
    Carve c;
    off = c.take((C + 1) * sizeof(int64_t));                             // offsets (device copy)
    minb = c.take(C * 3 * sizeof(float));                                // min bounds
    k0 = c.take(n * sizeof(uint64_t)); k1 = c.take(n * sizeof(uint64_t));   // keys in / out
    v0 = c.take(n * sizeof(uint32_t)); v1 = c.take(n * sizeof(uint32_t));   // vals in / out
    head = c.take(n * sizeof(int32_t)); ordinal = c.take(n * sizeof(int32_t));
    first = c.take(C * sizeof(int32_t));                                 // first ordinal
    bad_row = c.take(sizeof(int32_t));                                   // first row with an unrepresentable voxel index
    tmp_bytes = sort_tmp > scan_tmp ? sort_tmp : scan_tmp;
    tmp = c.take(tmp_bytes);
    bytes = c.p;
  }
};

// what every pose-from-correspondences stage keeps (pose_corr.hip): matched points cs / cq [P][M][3], refit weights w [P][M], round
// state Tcand [R + 1][P][12], cnt [R + 1][P], info [4][P].  It is the head of their scratch: RansacLayout, ConsensusLayout and
// FgrLayout (fgr.h) go on from `bytes` and end with a CandLayout.
struct PoseLayout {
  size_t cs, cq, w, Tcand, cnt, info, bytes;
  PoseLayout(int pairs, int M, int refine_iters) {
    const size_t P = (size_t)pairs, R1 = (size_t)(refine_iters + 1);
    Carve c;
    cs = c.take(P * M * 12); cq = c.take(P * M * 12); w = c.take(P * M * 4);
    Tcand = c.take(P * R1 * 48); cnt = c.take(P * R1 * 4); info = c.take(P * 16);
    bytes = c.p;
  }
};
// the gather, the scoring and the refit index [P][M] rows with 32-bit products
constexpr bool pose_corr_shape_ok(int pairs, int M) { return (int64_t)pairs * M <= 0x7fffffffll; }

// the candidate poses the middle of a stage hands to the tail: T [P][H][12], valid [P][H], count [P][H] - the last three parts of
// every stage's scratch
struct CandLayout {
  size_t T = 0, valid = 0, count = 0;
  void take(Carve& c, size_t P, size_t H) { T = c.take(P * H * 48); valid = c.take(P * H * 4); count = c.take(P * H * 4); }
};

struct RansacLayout {        // launch_ransac: P (M 28 + H 56) bytes plus a few hundred bytes per pair of round state
  PoseLayout pose;
  CandLayout hyp;
  size_t bytes;
  RansacLayout(int pairs, int M, int H, int refine_iters) : pose(pairs, M, refine_iters) {
    Carve c{pose.bytes};
    hyp.take(c, (size_t)pairs, (size_t)H);
    bytes = c.p;
  }
};

struct ConsensusLayout {     // launch_consensus: P M W 8 bytes of bit matrix, P (M 48 + seeds 56)-order scratch, the seed sort's own
  PoseLayout pose;
  size_t bits, score, k0, k1, seg, tmp, seed;
  CandLayout hyp;
  size_t bytes;
  ConsensusLayout(int pairs, int M, int seeds, int refine_iters, size_t sort_tmp) : pose(pairs, M, refine_iters) {
    const size_t P = (size_t)pairs, W = (size_t)(M + 63) / 64;
    Carve c{pose.bytes};
    bits = c.take(P * M * W * 8);                                        // C as a bit matrix [P][M][W]
    score = c.take(P * M * 4);
    k0 = c.take(P * M * 8); k1 = c.take(P * M * 8);                      // score << 32 | ~index, raw and sorted
    seg = c.take((P + 1) * 4);
    tmp = c.take(sort_tmp);
    seed = c.take(P * seeds * 4);
    hyp.take(c, P, (size_t)seeds);
    bytes = c.p;
  }
};

// dsir_t_radius_matches_count / _fill: buf = per-row match counts of every reference part (then their prefix) [rows][parts] int32, the
// scan's temporary; dsir_t_match_keys: buf = the unsorted int64 keys, the segmented sort's temporary
struct BufferTmpLayout {
  size_t buf, tmp, bytes;
  BufferTmpLayout(size_t buf_bytes, size_t tmp_bytes) {
    Carve c;
    buf = c.take(buf_bytes);
    tmp = c.take(tmp_bytes);
    bytes = c.p;
  }
};

}  // namespace dsir
