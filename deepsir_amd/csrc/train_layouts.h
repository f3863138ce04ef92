// The plans and scratch layouts of the training operators (train_gemm.hip, train_norm.hip, train_loss.hip): the row split of the
// weight-gradient GEMM, the row chunks of the GroupNorm reductions, and every operator's scratch as offsets into one piece, built from
// the operator's shape alone and read by its size function (include/dsir_train.h: dsir_t_*_scratch) and its launcher alike.
// Plain host C++ on the model of op_layouts.h, no device code: tools/train_layout_check.cpp lays every one out on the CPU.
// Every part starts on 256 bytes (Carve), so a byte count is at most the plain sum of its parts plus 255 bytes per part.
#pragma once
#include "scratch.h"

namespace dsir {

constexpr int TB = 64;        // GEMM tile: 64 rows x 64 columns
constexpr int TK = 16;        // K chunk

// ---- dsir_t_gemm_dw: the row split, one partial matrix [N][Kp] per split
struct DwPlan { int splits; int64_t rows_per_split; int Kp; };
inline DwPlan dw_plan(int64_t rows, int N, int K, bool bias) {
  DwPlan p;
  p.Kp = K + (bias ? 1 : 0);
  const int64_t tiles = (int64_t)((N + TB - 1) / TB) * ((p.Kp + TB - 1) / TB);
  int64_t sp = (rows + 127) / 128;                       // >= 128 rows per split (512 before: 32 barrier-separated K steps, 40 us, for 79 workgroups)
  const int64_t cap = tiles >= 2048 ? 1 : 2048 / tiles;   // ~ 2048 workgroups in all
  sp = sp > cap ? cap : sp;
  sp = sp > 1024 ? 1024 : sp;
  sp = sp < 1 ? 1 : sp;
  p.rows_per_split = (((rows + sp - 1) / sp) + TK - 1) / TK * TK;
  p.splits = (int)((rows + p.rows_per_split - 1) / p.rows_per_split);
  if (p.splits < 1) p.splits = 1;
  return p;
}

// dsir_t_gemm_dw plans with or without the bias column (db == NULL): one tile column fewer can mean a larger split cap, i.e. MORE
// partial matrices than the other plan - the piece is sized for the larger of the two
struct DwLayout {
  size_t partial, bytes;
  DwLayout(int64_t rows, int N, int K) {
    const DwPlan pb = dw_plan(rows, N, K, true), pn = dw_plan(rows, N, K, false);
    const size_t a = (size_t)pb.splits * N * pb.Kp, b = (size_t)pn.splits * N * pn.Kp;
    Carve c;
    partial = c.take((a > b ? a : b) * sizeof(float));
    bytes = c.p;
  }
};

// ---- GroupNorm / BatchNorm(train)
// row chunks of the GroupNorm reductions: 128 rows and up to 256 chunks per cloud (round 3; 1024 / 64 before: a per-point layer of
// 8 x 5000 rows ran as 40 workgroups whose threads walked 128 rows each, 60 us - the trace showed 24 - 80 workgroups per launch
// on most of the 148 layers of a step)
constexpr int GN_CHUNK_ROWS = 128, GN_MAX_CHUNKS = 256;
inline int gn_chunks(int M) { const int c = (M + GN_CHUNK_ROWS - 1) / GN_CHUNK_ROWS; return c < 1 ? 1 : (c > GN_MAX_CHUNKS ? GN_MAX_CHUNKS : c); }

struct GnFwdLayout {         // dsir_t_gn_fwd: partial [cloud][group][chunk][2] fp64 (sum, sum of squares)
  size_t partial, bytes;
  GnFwdLayout(int clouds, int M, int C, int groups) {
    (void)C;
    Carve c;
    partial = c.take((size_t)clouds * groups * gn_chunks(M) * 2 * sizeof(double));
    bytes = c.p;
  }
};

struct GnBwdLayout {         // dsir_t_gn_bwd: partial [cloud][chunk][C][2], then sums [cloud][C][2], both fp32
  size_t partial, sums, bytes;
  GnBwdLayout(int clouds, int M, int C) {
    Carve c;
    partial = c.take((size_t)clouds * gn_chunks(M) * C * 2 * sizeof(float));
    sums = c.take((size_t)clouds * C * 2 * sizeof(float));
    bytes = c.p;
  }
};

// dsir_t_gn_scratch(clouds, M, C) serves both calls and does not know `groups`: the forward at its largest (groups = C), or the backward
inline size_t gn_scratch_bytes(int clouds, int M, int C) {
  const size_t f = GnFwdLayout(clouds, M, C, C).bytes, b = GnBwdLayout(clouds, M, C).bytes;
  return f > b ? f : b;
}

// ---- dsir_t_det_des_loss: five [P][M][M] fp32 matrices, the per-row / per-column vectors, one CircleRow (train_loss.hip) per row.
// At most (5 P M M + 6 P M) floats + P M CircleRows + 255 bytes for each of the ten parts; the count before the layout was
// (5 P M M + 16 P M) floats + P M CircleRows + 256 bytes, so: no more than that plus 256 bytes per part.
constexpr size_t kCircleRowBytes = 32;
struct DetDesLayout {
  size_t dot, dist_pc, dist_feat, Wn, Wnt, lse_col, coef, rowsum, colsum, rows, bytes;
  DetDesLayout(int pairs, int M) {
    const size_t mm = (size_t)pairs * M * M, pm = (size_t)pairs * M;
    Carve c;
    dot = c.take(mm * sizeof(float)); dist_pc = c.take(mm * sizeof(float)); dist_feat = c.take(mm * sizeof(float));
    Wn = c.take(mm * sizeof(float)); Wnt = c.take(mm * sizeof(float));
    lse_col = c.take(pm * sizeof(float));
    coef = c.take(3 * pm * sizeof(float));               // {A, B, c} per row (t_circle_final_kernel)
    rowsum = c.take(pm * sizeof(float)); colsum = c.take(pm * sizeof(float));
    rows = c.take(pm * kCircleRowBytes);
    bytes = c.p;
  }
};

// ---- dsir_t_weighted_ce: per 256-row block {sum w nll, sum w, correct, valid} fp64
struct WceLayout {
  size_t partial, bytes;
  int blocks;
  explicit WceLayout(int64_t rows) {
    blocks = (int)((rows + 255) / 256);
    Carve c;
    partial = c.take((size_t)blocks * 4 * sizeof(double));
    bytes = c.p;
  }
};

}  // namespace dsir
