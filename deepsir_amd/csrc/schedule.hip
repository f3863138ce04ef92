// The launch schedules of libdsir.so: RandLA.forward, Network.aggregation and the KNN pyramid, layer by layer (Sched), and the
// deep-level walker's program bookkeeping.
#include <cstddef>
#include <cstring>
#include <vector>

#include "engine_ctx.h"

namespace dsir {

namespace {
void level_sizes(const dsir_cfg& cfg, int n, int* nl) {
  nl[0] = n;
  for (int l = 0; l < cfg.num_layers; ++l) nl[l + 1] = nl[l] / cfg.sub_sampling_ratio[l];
}
}  // namespace

void fill_pyramid_layout(const dsir_cfg& cfg, int clouds, int n, Pyramid& p) {
  p.clouds = clouds; p.n = n;
  level_sizes(cfg, n, p.nl);
  p.off[0] = 0; p.soff[0] = 0;
  for (int l = 0; l < cfg.num_layers; ++l) { p.off[l + 1] = p.off[l] + p.nl[l]; p.soff[l + 1] = p.soff[l] + p.nl[l + 1]; }
  p.S = p.off[cfg.num_layers]; p.S1 = p.soff[cfg.num_layers];
}

// The most contributions any (cloud, group) GroupNorm statistic receives when a cloud of n points goes through RandLA.forward: the
// maximum of the launchers' own counts (kernels.h) over every MLP2D of the schedule, under the default dispatch of launch_pw_gemm
// (Cin <= 64 and the relative-position layers: pw_stream.hip or - d / 2 = 8, 32 - lse_uv.hip; wider: pw_tile.hip, whose count also
// bounds the generic pw_gemm.hip kernel's 64-row blocks).  The exactness proof of the statistics' atomics (device_utils.h) needs
// this number <= kGnMaxContrib: dsir_create refuses a max_points beyond it.
// Under DSIR_FLAG_PPF the schedule gains the point-pair-feature layer (ppf.hip: one contribution per 64 points) and level 0's
// mlp1 / mlp_skip take 12 input channels, which no tuned family serves: the general kernel's 64-row blocks (pw_gemm.hip).  Both
// count n / 64 per statistic, half of lfa.mlp1's n / 32 at level 0 (16 n rows in units of 512), which stays the largest: the
// bound on max_points is the same with and without the flag, and it is re-derived here, not assumed.
int gn_max_contributions(const dsir_cfg& g, int n, int flags) {
  const bool ppf = (flags & DSIR_FLAG_PPF) != 0;
  int worst = 0;
  auto layer = [&](int M, int cin, int cout) {
    const int groups = cout >= 64 ? 8 : 4;
    const int c = cin <= 64 ? pw_stream_gn_contributions(M, cout) : pw_tile_gn_contributions(M, cout, groups);
    if (c > worst) worst = c;
  };
  int nl[DSIR_MAX_LEVELS + 1];
  level_sizes(g, n, nl);
  const int L = g.num_layers;
  if (ppf) { const int c = ppf_gn_contributions(nl[0]); if (c > worst) worst = c; }
  else layer(nl[0], 6 > g.feat_len ? 6 : g.feat_len, 8);
  int dim = ppf ? 12 : 8;
  for (int l = 0; l < L; ++l) {
    const int d = g.d_out[l], m = nl[l], mk = nl[l] * kKnn;
    if (ppf && l == 0) { const int c = pw_gemm_gn_contributions(m); if (c > worst) worst = c; }   // Cin = 12: the general kernel
    else { layer(m, dim, d / 2); layer(m, dim, 2 * d); }         // mlp1, mlp_skip
    if (d / 2 == 8 || d / 2 == 32) { const int c = lse_uv_gn_contributions(m, d / 2); if (c > worst) worst = c; }
    if (d / 2 == 8) { const int c = att_pool16_gn_contributions(m); if (c > worst) worst = c; }   // lfa.mlp2 from the first pooling (= its own launch's count)
    layer(mk, 10, d / 2);                                        // lfa.mlp1 (also when the tables are switched off)
    layer(mk, d / 2, d / 2);                                     // lfa.mlp2
    layer(m, d, d / 2); layer(m, d, d); layer(m, d, 2 * d);      // att_pooling_1.mlp, att_pooling_2.mlp, mlp2
    dim = 2 * d;
  }
  layer(nl[L], dim, dim);
  int dcur = dim;
  for (int j = 0; j < L; ++j) {
    const int lvl = L - 1 - j;
    const int cin = j < L - 1 ? dcur + 2 * g.d_out[L - j - 2] : 4 * g.d_out[0];
    dcur = j < L - 1 ? 2 * g.d_out[L - j - 2] : 2 * g.d_out[0];
    layer(nl[lvl], cin, dcur);
  }
  return worst;
}

namespace {

// A/B switch: DSIR_NO_LSE_UV = lfa.mlp1 of levels 0 / 1 written to memory as up to round 3 (pw_stream.hip, loader S_LSE) instead of
// the per-point tables of lse_uv.hip; the tables' consumers are att_pool.hip and pw_stream.hip (loader S_UV) only
bool lse_uv_enabled() {
  static const bool off = tuning_flag("DSIR_NO_LSE_UV") || tuning_flag("DSIR_NO_STREAM");   // the tables' GEMM consumer is pw_stream.hip alone
  return !off;
}

// ------------------------------------------------------------------ schedule helpers
// Upload a finished walker program and launch it (walk.hip).  Eager calls: in-stream copy from pinned staging; a registration under
// capture: collected on the host, uploaded once after the capture (dsir_register), the kernel node holds the final device address.
int walk_flush(dsir_ctx* c, WalkProgram& P, hipStream_t st) {
  if (P.nphases <= 0) return 0;
  if (c->call.walk_used >= dsir_ctx::kWalkSlots) return fail(c, "walker: more than %d programs in one call", dsir_ctx::kWalkSlots);
  const int slot = c->call.walk_used++;
  P.ctr = c->walk_ctr + (size_t)slot * dsir_ctx::kWalkClouds * kWalkCtrWords;
  P.trace = c->walk_trace ? c->walk_trace + (size_t)slot * kWalkMaxPhases * 4 : nullptr;
  const size_t bytes = offsetof(WalkProgram, job) + (size_t)P.nphases * sizeof(WalkJob);
  const WalkProgram* dev;
  if (c->capturing) {
    std::memcpy(c->cap_host.data() + (size_t)slot * sizeof(WalkProgram), &P, bytes);
    dev = c->cap_dev + slot;
  } else {
    WalkProgram* h = c->walk_host[c->walk_set] + slot;
    std::memcpy(reinterpret_cast<void*>(h), &P, bytes);
    HIP_OK(c, hipMemcpyAsync(c->walk_dev + slot, h, bytes, hipMemcpyHostToDevice, st));
    dev = c->walk_dev + slot;
  }
  // queues and counters of this program: part of the region a registration zeroes in its opening launch; otherwise here
  if (!c->call.stats_prezeroed) HIP_OK(c, hipMemsetAsync(P.ctr, 0, sizeof(unsigned) * P.clouds * kWalkCtrWords, st));
  launch_walk(P, dev, st);
  P.nphases = 0;
  return 0;
}

struct Sched {
  dsir_ctx* c;
  hipStream_t st;
  int clouds;
  // deep-level walker: while `rec` is set, layers whose kernel the walker holds become PHASES of one launch instead of launches
  WalkProgram* rec = nullptr;
  int rec_wpc = 1;
  int rec_error = 0;
  // launch what has been recorded; recording stops when the call has no program slot left (the rest of the pass: plain launches)
  void rec_flush() {
    if (!rec) return;
    if (rec->nphases > 0 && walk_flush(c, *rec, st)) rec_error = 1;
    if (c->call.walk_used >= dsir_ctx::kWalkSlots) rec = nullptr;
  }
  // false: not recorded (no room) - the caller launches the layer itself
  bool rec_push(const WalkJob& j) {
    if (!rec) return false;
    if (rec->nphases == kWalkMaxPhases) { rec_flush(); if (!rec) return false; }
    WalkJob& d = rec->job[rec->nphases];
    d = j;
    d.dep = rec->nphases > 0 ? rec->nphases - 1 : -1;     // the deep half of a pass is a chain: every phase reads the one before
    ++rec->nphases;
    return true;
  }
  // a launcher refused the layer: nothing more runs (as on an exhausted arena), the schedule's caller reports why
  void refuse(const char* why) {
    if (!c->ws.overflow) c->call.sched_error = why;
    c->ws.overflow = true;
  }
  // a point-wise GEMM launch: a phase when recording and plannable, else (after flushing what was recorded: order) its own launch
  void gemm(const GemmArgs& a) {
    if (rec) {
      WalkJob j;
      if (walk_plan_gemm(a, &j) && rec_push(j)) return;
      rec_flush();
    }
    if (!launch_pw_gemm(a, st)) refuse("point-wise GEMM: no kernel took the layer");
  }

  double* stats_slot(int groups) {
    double* p = c->stats + c->call.stats_top;
    c->call.stats_top += (size_t)clouds * groups * kGnWords;
    return p;
  }
  // the fp16 split of a weight matrix inside the context's blob (dsir_finalize_weights); off unless the split layers are on
  void split_of(GemmArgs& a) const {
    if (!c->agg_split || !c->dweights16 || a.W < c->dweights || a.W >= c->dweights + c->nweights) return;
    const size_t off = (size_t)(a.W - c->dweights);
    if (!c->split_ok(off)) return;          // outside the split's domain (split_f16.h): the layer's exact-fp32 kernel
    a.Wh = c->dweights16 + off;
    a.Wl = c->dweights16 + c->nweights + off;
  }
  // the lazy GroupNorm of a layer's output: statistics at st, M rows per cloud
  static GnRef gn_of(const double* st, const Mlp2dW& w, int M) {
    return GnRef{st, w.gamma, w.beta, w.groups, 1.0 / ((double)(w.cout / w.groups) * (double)M)};
  }
  static Seg seg_of(const Act& a, const int32_t* idx = nullptr, int64_t idx_cs = 0) {
    Seg s{};
    s.x = a.p; s.cloud_stride = (int64_t)a.rows * a.C; s.C = a.C; s.ld = a.C;
    s.idx = idx; s.idx_cloud_stride = idx_cs; s.gn = a.gn; s.act = a.act;
    s.uv = a.uv; s.uv_cloud_stride = (int64_t)(a.rows / kKnn) * 2 * a.C; s.dist = a.dist; s.dist_cloud_stride = a.rows; s.w8 = a.w8;
    return s;
  }
  // MLP2D: conv1x1 + GroupNorm (lazy) [+ LeakyReLU (lazy)]
  // out_buf / st_buf: caller-owned storage (persistent across launches) instead of the per-pass arenas
  Act mlp2d(const Mlp2dW& w, const Seg& s0, const Seg* s1, int M, bool act, float* out_buf = nullptr,
            double* st_buf = nullptr) {
    Act y;
    y.p = out_buf ? out_buf : c->ws.get<float>((size_t)clouds * M * w.cout);
    y.C = w.cout; y.rows = M; y.act = act ? 1 : 0;
    double* st_out = st_buf ? st_buf : stats_slot(w.groups);
    y.gn = gn_of(st_out, w, M);
    GemmArgs a;
    a.amode = A_SEGS; a.nseg = s1 ? 2 : 1; a.seg[0] = s0; if (s1) a.seg[1] = *s1;
    a.W = w.W; a.bias = w.b; a.Cin = w.cin; a.Cout = w.cout; a.M = M; a.clouds = clouds; a.epi = EPI_GN;
    a.Y = y.p; a.y_cloud_stride = (int64_t)M * w.cout; a.ldy = w.cout; a.stats_out = st_out; a.groups_out = w.groups;
    split_of(a);
    if (c->ws.overflow) return y;                 // an exhausted arena hands out its base: nothing may run on it
    if ((s0.uv && !s0.x) || (s1 && s1->uv && !s1->x)) {
      // table-only rows (lse_uv.hip) exist for ONE loader, pw_stream.hip's S_UV: the generic kernels would dereference the null row base
      rec_flush();
      if (launch_pw_stream(a, st) != Launch::done) refuse("MLP2D: no kernel took the table-only position encoding");
      return y;
    }
    gemm(a);
    return y;
  }
  // use_ppf: feat_grouping + mlp_pre + the mean over the neighbours (ppf.hip; RandLANet.py:324-332).  pts: the rows' xyz columns,
  // nrm: their "normals" (optionally gathered: the inlier model's matched ref points, model.py:574-577), nb: level-0 neighbour rows.
  // The result is a finished activation (normalised, activated, averaged): no lazy GroupNorm rides on it.
  Act ppf_pre(const Mlp2dW& w, const Seg& pts, const Seg& nrm, const int32_t* nb, int64_t nb_cs, int n, float* out_buf = nullptr) {
    Act y;
    y.p = out_buf ? out_buf : c->ws.get<float>((size_t)clouds * n * 12);
    y.C = 12; y.rows = n; y.act = 0;
    PpfArgs a;
    a.xyz = pts.x; a.xyz_cs = pts.cloud_stride; a.xyz_ld = pts.ld;
    a.nrm = nrm.x; a.nrm_cs = nrm.cloud_stride; a.nrm_ld = nrm.ld; a.nrm_idx = nrm.idx; a.nrm_idx_cs = nrm.idx_cloud_stride;
    a.neigh = nb; a.neigh_cs = nb_cs;
    a.W = w.W; a.b = w.b; a.gamma = w.gamma; a.beta = w.beta;
    a.stats = stats_slot(4);
    a.out = y.p; a.out_cs = (int64_t)n * 12; a.n = n; a.clouds = clouds;
    rec_flush();
    if (w.cin != 10 || w.cout != 12 || w.groups != 4) { refuse("mlp_pre: the point-pair-feature layer is 10 -> 12 channels in 4 groups"); return y; }
    if (!c->ws.overflow && !launch_ppf_pre(a, st)) refuse("mlp_pre: the point-pair-feature layer refused the launch");
    return y;
  }
  // mlp1 and mlp_skip of a block in ONE launch (same input; the weights one after the other, BlockW::pair_W): two outputs, two
  // sets of statistics - each element the chain the separate launch gives it.  False: not served (the caller launches them apart).
  bool mlp2d_pair(const BlockW& b, const Seg& s0, int M, Act& y1, Act& y2) {
    if (!b.pair_W) return false;
    const Mlp2dW &w1 = b.mlp1, &w2 = b.skip;
    GemmArgs a;
    a.amode = A_SEGS; a.nseg = 1; a.seg[0] = s0;
    a.W = b.pair_W; a.bias = b.pair_b; a.Cin = w1.cin; a.Cout = w1.cout + w2.cout; a.M = M; a.clouds = clouds; a.epi = EPI_GN;
    a.c_split = w1.cout;
    split_of(a);
    a.groups_out = w1.groups; a.groups_out2 = w2.groups;
    a.Y = reinterpret_cast<float*>(1); a.Y2 = a.Y; a.stats_out = reinterpret_cast<double*>(1); a.stats_out2 = a.stats_out;   // placeholders for the predicate
    a.ldy = w1.cout; a.ldy2 = w2.cout;
    if (!pw_gemm_serves_pair(a)) return false;
    y1.p = c->ws.get<float>((size_t)clouds * M * w1.cout); y1.C = w1.cout; y1.rows = M; y1.act = 1;
    y2.p = c->ws.get<float>((size_t)clouds * M * w2.cout); y2.C = w2.cout; y2.rows = M; y2.act = 0;
    double* st1 = stats_slot(w1.groups);
    double* st2 = stats_slot(w2.groups);
    y1.gn = gn_of(st1, w1, M);
    y2.gn = gn_of(st2, w2, M);
    a.Y = y1.p; a.y_cloud_stride = (int64_t)M * w1.cout; a.stats_out = st1;
    a.Y2 = y2.p; a.y2_cloud_stride = (int64_t)M * w2.cout; a.stats_out2 = st2;
    if (!c->ws.overflow) gemm(a);
    return true;
  }
  // lfa.mlp1 split by linearity (lse_uv.hip): per-point tables + dist + statistics, no output rows.  uv_buf / dist_buf: caller-owned
  // storage (persistent across launches) or nullptr
  Act lse_uv(const Mlp2dW& w, const float* w8, const float* xyz, int64_t xyz_cs, const int32_t* neigh, int64_t neigh_cs, int n,
             float* uv_buf, float* dist_buf, double* st_buf) {
    const int M = n * kKnn;
    Act y;
    y.p = nullptr; y.C = w.cout; y.rows = M; y.act = 1;
    float* uv = uv_buf ? uv_buf : c->ws.get<float>((size_t)clouds * n * 2 * w.cout);
    float* dist = dist_buf ? dist_buf : c->ws.get<float>((size_t)clouds * M);
    double* st_out = st_buf ? st_buf : stats_slot(w.groups);
    y.gn = gn_of(st_out, w, M);
    y.uv = uv; y.dist = dist; y.w8 = w8;
    LseUvArgs a;
    a.xyz = xyz; a.xyz_cs = xyz_cs; a.neigh = neigh; a.neigh_cs = neigh_cs; a.w8 = w8;
    a.uv = uv; a.uv_cs = (int64_t)n * 2 * w.cout; a.dist = dist; a.dist_cs = M;
    a.stats_out = st_out; a.groups = w.groups; a.n = n; a.clouds = clouds; a.KH = w.cout;
    rec_flush();
    if (!c->ws.overflow && !launch_lse_uv_stats(a, st)) refuse("lse_uv: layer outside the kernel's envelope");
    return y;
  }
  Act mlp2d_lse(const Mlp2dW& w, const float* xyz, int64_t xyz_cs, const int32_t* neigh, int64_t neigh_cs, int n,
                float* out_buf = nullptr, double* st_buf = nullptr) {
    const int M = n * kKnn;
    Act y;
    y.p = out_buf ? out_buf : c->ws.get<float>((size_t)clouds * M * w.cout);
    y.C = w.cout; y.rows = M; y.act = 1;
    double* st_out = st_buf ? st_buf : stats_slot(w.groups);
    y.gn = gn_of(st_out, w, M);
    GemmArgs a;
    a.amode = A_LSE; a.xyz = xyz; a.xyz_cloud_stride = xyz_cs; a.neigh = neigh; a.neigh_cloud_stride = neigh_cs;
    a.W = w.W; a.bias = w.b; a.Cin = 10; a.Cout = w.cout; a.M = M; a.clouds = clouds; a.epi = EPI_GN;
    a.Y = y.p; a.y_cloud_stride = (int64_t)M * w.cout; a.ldy = w.cout; a.stats_out = st_out; a.groups_out = w.groups;
    split_of(a);
    rec_flush();
    // an exhausted arena hands out its base: nothing may run on it
    if (!c->ws.overflow && !launch_pw_gemm(a, st)) refuse("lfa.mlp1: no kernel took the relative-position layer");
    return y;
  }
  // the operands of att_pool.hip's kernels: the score matrix as its fp16 split inside the context's blob
  AttPool16Args att_pool_args(const AttW& w, const Act& f, const Act& enc, const int32_t* neigh, int64_t neigh_cs, int n, const Act& y) const {
    AttPool16Args a;
    a.f = f.p; a.f_cs = (int64_t)f.rows * f.C; a.f_ld = f.C; a.f_gn = f.gn; a.f_act = f.act;
    a.enc = enc.p; a.enc_cs = (int64_t)enc.rows * enc.C; a.enc_gn = enc.gn; a.enc_act = enc.act;
    a.uv = enc.uv; a.uv_cs = (int64_t)n * 2 * enc.C; a.dist = enc.dist; a.dist_cs = (int64_t)n * kKnn; a.w8 = enc.w8;
    a.neigh = neigh; a.neigh_cs = neigh_cs;
    const size_t off = (size_t)(w.fc - c->dweights);
    a.Wh = c->dweights16 + off; a.Wl = c->dweights16 + c->nweights + off; a.ldw = w.d;
    a.Y = y.p; a.y_cs = (int64_t)n * w.d; a.n = n; a.clouds = clouds;
    return a;
  }
  // lfa.mlp2 as a second product of a block's FIRST pooling (att_pool.hip, the producing variant): what Sched::att is asked for and
  // what it answers.  buf / stats: caller-owned storage (the registration's cache) or nullptr: the pass's arenas.
  struct AttEnc2 {
    const Mlp2dW* w = nullptr;
    float* buf = nullptr;
    double* stats = nullptr;
    bool done = false;     // out is lfa.mlp2's activation, exactly mlp2d()'s: nothing more to launch
    Act out;
  };
  // Att_pooling up to (not including) its MLP2D: softmax_k(fc [gather(f); enc]) . [gather(f); enc].  One ladder by the level width d:
  //   16          att_pool.hip, four points per wave; with table-only enc and e2 set it also writes lfa.mlp2 (e2->done)
  //   64, 128     att_pool.hip, unsplit (a walker phase when recording)
  //   256         pw_tile.hip, EPI_ATT2: the score GEMM split by linearity, after its G GEMM (both walker phases when recording)
  //   otherwise, or when the width's own kernel refuses the layer: the general EPI_ATT kernel (pw_gemm.hip)
  // s2 / s2_mode: the cache of the enc half of the scores (kernels.h, GemmArgs::s2), kept by the widths of att_keeps_score_cache()
  Act att(const AttW& w, const Act& f, const Act& enc, const int32_t* neigh, int64_t neigh_cs, int n, float* s2 = nullptr,
          int s2_mode = 0, AttEnc2* e2 = nullptr) {
    Act y;
    y.p = c->ws.get<float>((size_t)clouds * n * w.d);
    y.C = w.d; y.rows = n;
    const bool halves = f.C * 2 == w.d && enc.C * 2 == w.d;
    const bool fc16 = c->dweights16 && w.fc >= c->dweights && w.fc < c->dweights + c->nweights;   // att_pool.hip reads fc as its fp16 split
    if (w.d == 16 && halves && fc16) {
      // att_pool.hip, level 0: four points per wave, fp16-split scores, softmax in registers
      AttPool16Args a = att_pool_args(w, f, enc, neigh, neigh_cs, n, y);
      rec_flush();
      if (e2 && e2->w && enc.uv && !enc.p && e2->w->cin == 8 && e2->w->cout == 8) {
        a.e2_W = e2->w->W; a.e2_b = e2->w->b; a.e2_groups = e2->w->groups;
        if (att_pool16_produces(a)) {
          const int M = n * kKnn;
          Act& o = e2->out;
          o.p = e2->buf ? e2->buf : c->ws.get<float>((size_t)clouds * M * 8);
          o.C = 8; o.rows = M; o.act = 1;
          double* st_out = e2->stats ? e2->stats : stats_slot(e2->w->groups);
          o.gn = gn_of(st_out, *e2->w, M);
          a.e2_Y = o.p; a.e2_cs = (int64_t)M * 8; a.e2_stats = st_out;
          if (c->ws.overflow) return y;
          if (launch_att_pool16(a, st)) { e2->done = true; return y; }
          refuse("attentive pooling: the producing variant refused a layer it had accepted");
          return y;
        }
        a.e2_W = a.e2_b = nullptr; a.e2_groups = 0;
      }
      if (!c->ws.overflow && launch_att_pool16(a, st)) return y;
    } else if ((w.d == 64 || w.d == 128) && halves && fc16 && (enc.p || w.d == 64)) {
      // att_pool.hip, levels 1 / 2 unsplit: the whole score contraction on the matrix pipe, nothing gathered in the epilogue
      const AttPool16Args a = att_pool_args(w, f, enc, neigh, neigh_cs, n, y);
      if (c->ws.overflow) return y;
      if (rec) {
        WalkJob j;
        if (walk_plan_att_full(a, w.d / 2, rec_wpc, &j) && rec_push(j)) return y;
        rec_flush();
      }
      if (launch_att_full(a, w.d / 2, st)) return y;
    } else if (att_keeps_score_cache(w.d) && w.fc_g && halves && enc.p) {
      // score GEMM split by linearity: fc [gather(f); enc] = gather(W1 f) + W2 enc  (kernels.h, EPI_ATT2).
      // G = W1 f runs on n rows instead of 16 n; the pooling launch contracts only the enc half.
      float* G = c->ws.get<float>((size_t)clouds * n * w.d);
      GemmArgs g;
      g.amode = A_SEGS; g.nseg = 1; g.seg[0] = seg_of(f);
      g.W = w.fc_g; g.ldw = w.d / 2; g.bias = nullptr; g.Cin = w.d / 2; g.Cout = w.d; g.M = n; g.clouds = clouds;   // G in the consumer's column order (up_fc_g)
      g.epi = EPI_LINEAR; g.Y = G; g.y_cloud_stride = (int64_t)n * w.d; g.ldy = w.d;
      if (c->ws.overflow) return y;
      split_of(g);
      gemm(g);
      GemmArgs a2;
      a2.amode = A_SEGS; a2.nseg = 1; a2.seg[0] = seg_of(enc);
      a2.W = w.fc + w.d / 2; a2.ldw = w.d; a2.bias = nullptr; a2.Cin = w.d / 2; a2.Cout = w.d; a2.M = n * kKnn;
      a2.clouds = clouds; a2.epi = EPI_ATT2; a2.Y = y.p; a2.y_cloud_stride = (int64_t)n * w.d; a2.ldy = w.d;
      a2.g = G; a2.g_cloud_stride = (int64_t)n * w.d; a2.fseg = seg_of(f, neigh, neigh_cs);
      a2.s2 = s2; a2.s2_mode = s2 ? s2_mode : 0; a2.s2_cloud_stride = (int64_t)n * kKnn * w.d;
      split_of(a2);
      if (rec) {
        WalkJob j;
        if (walk_plan_gemm(a2, &j) && rec_push(j)) return y;
      }
      rec_flush();
      if (launch_pw_tile(a2, st)) return y;
    }
    if (!enc.p) {     // table-only rows (lse_uv.hip) have no consumer but att_pool.hip
      refuse("attentive pooling: no kernel took the table-only position encoding");
      return y;
    }
    GemmArgs a;
    a.amode = A_SEGS; a.nseg = 2;
    a.seg[0] = seg_of(f, neigh, neigh_cs);
    a.seg[1] = seg_of(enc);
    a.W = w.fc; a.bias = nullptr; a.Cin = w.d; a.Cout = w.d; a.M = n * kKnn; a.clouds = clouds; a.epi = EPI_ATT;
    a.Y = y.p; a.y_cloud_stride = (int64_t)n * w.d; a.ldy = w.d;
    split_of(a);
    rec_flush();
    // an exhausted arena hands out its base: nothing may run on it
    if (!c->ws.overflow && !launch_pw_gemm(a, st)) refuse("attentive pooling: no kernel took the score layer");
    return y;
  }
  Act linear(const LinW& w, const Seg& s0, const Seg* s1, int M, int epi, float* out = nullptr,
             const float* residual = nullptr) {
    Act y;
    y.p = out ? out : c->ws.get<float>((size_t)clouds * M * w.cout);
    y.C = w.cout; y.rows = M;
    GemmArgs a;
    a.amode = A_SEGS; a.nseg = s1 ? 2 : 1; a.seg[0] = s0; if (s1) a.seg[1] = *s1;
    a.W = w.W; a.bias = w.b; a.Cin = w.cin; a.Cout = w.cout; a.M = M; a.clouds = clouds; a.epi = epi;
    a.Y = y.p; a.y_cloud_stride = (int64_t)M * w.cout; a.ldy = w.cout;
    a.residual = residual; a.res_cloud_stride = (int64_t)M * w.cout; a.ldres = w.cout;
    split_of(a);
    rec_flush();
    // an exhausted arena hands out its base: nothing may run on it
    if (!c->ws.overflow && !launch_pw_gemm(a, st)) refuse("linear layer: no kernel took the layer");
    return y;
  }
};

}  // namespace

// a call that may run RandLA passes: eager calls take the other pinned staging set (the previous call's copies may still be queued)
// after making sure that set's own last copy has run; a capture collects its programs on the host instead
int Call::begin_walker() {
  dsir_ctx* c = c_;
  if (c->capturing || !c->walk_dev) return 0;
  c->walk_set ^= 1;
  c->call.walk_begun = true;
  if (c->walk_ev_armed[c->walk_set]) { HIP_OK(c, hipEventSynchronize(c->walk_ev[c->walk_set])); c->walk_ev_armed[c->walk_set] = false; }
  return 0;
}
// the end of such a call, on every way out: the set's event after the last copy from it
hipError_t Call::end_walker(dsir_ctx* c) {
  if (!c->call.walk_begun || c->call.walk_used == 0) return hipSuccess;
  c->call.walk_begun = false;
  const hipError_t e = hipEventRecord(c->walk_ev[c->walk_set], c->stream);
  if (e == hipSuccess) c->walk_ev_armed[c->walk_set] = true;
  return e;
}

// persistent storage of the inlier model's position-encoding branch, alive across the iterations of a registration
int EncCache::plan(dsir_ctx* c, const Pyramid& ps, double* prezeroed) {
  const dsir_cfg& g = c->cfg;
  Arena& ws = c->ws;
  const int P = ps.clouds;
  for (int l = 0; l < g.num_layers; ++l) {
    const size_t rows = (size_t)P * ps.nl[l] * kKnn, ch = (size_t)g.d_out[l] / 2;
    if (c->net.inl.blk[l].lse_w8 && lse_uv_enabled()) {
      uv_buf[l] = ws.get<float>((size_t)P * ps.nl[l] * 2 * ch);
      dist_buf[l] = ws.get<float>(rows);
    } else {
      enc_buf[l] = ws.get<float>(rows * ch);
    }
    enc2_buf[l] = ws.get<float>(rows * ch);
    static const bool no_s2 = tuning_flag("DSIR_NO_S2");   // A/B switch: recompute the enc half of the scores every iteration
    if (att_keeps_score_cache(g.d_out[l]) && !no_s2) {
      s2_buf[l][0] = ws.get<float>(rows * (size_t)g.d_out[l]);
      s2_buf[l][1] = ws.get<float>(rows * (size_t)g.d_out[l]);
    }
  }
  double* cst = prezeroed;                       // zeroed by the opening launch
  if (!cst) {                                    // more iterations than the statistics arena holds side by side: own storage, own memset
    const size_t nstats = stats_words(g, P);
    cst = ws.get<double>(nstats);
    if (!ws.overflow) HIP_OK(c, hipMemsetAsync(cst, 0, nstats * sizeof(double), c->stream));
  }
  for (int l = 0; l < g.num_layers; ++l) {
    enc_stats[l] = cst + (size_t)(2 * l) * gn_layer_words(P);
    enc2_stats[l] = cst + (size_t)(2 * l + 1) * gn_layer_words(P);
  }
  return 0;
}

// use_ppf front end alone (dsir_ppf_pre): one layer's statistics, zeroed here
int run_ppf_pre(dsir_ctx* c, const RandlaW& w, const float* rows, int stride, const int32_t* neigh, int64_t neigh_cs, int clouds, int n,
                float* out) {
  const size_t stats_need = gn_layer_words(clouds, 4);
  if (stats_need > c->stats_cap) return fail(c, "stats arena too small (%zu > %zu)", stats_need, c->stats_cap);
  c->call.stats_top = 0;
  HIP_OK(c, hipMemsetAsync(c->stats, 0, stats_need * sizeof(double), c->stream));
  Sched s{c, c->stream, clouds};
  s.ppf_pre(w.pre, plain_seg(rows, (int64_t)n * stride, 3, stride), plain_seg(rows + 3, (int64_t)n * stride, 3, stride), neigh, neigh_cs, n, out);
  return 0;
}

// lfa.mlp2 of one level alone, by either of its producers (dsir_lfa_enc2_probe): lfa.mlp1's tables, then the row-streaming launch
// (fused = 0) or the first pooling's producing variant on zero features (fused = 1; the second product does not read them).
int run_lfa_enc2_probe(dsir_ctx* c, const RandlaW& w, int level, int fused, const Pyramid& py, float* rows_out, double* stats_out) {
  const BlockW& b = w.blk[level];
  if (!b.lse_w8 || !lse_uv_enabled()) return fail(c, "lfa_enc2_probe: level %d has no position-encoding tables", level);
  const int n = py.nl[level], M = n * kKnn, ch = b.lfa2.cout;
  hipStream_t st = c->stream;
  const size_t stats_need = 2 * gn_layer_words(py.clouds);
  if (stats_need > c->stats_cap) return fail(c, "stats arena too small (%zu > %zu)", stats_need, c->stats_cap);
  c->call.stats_top = 0;
  HIP_OK(c, hipMemsetAsync(c->stats, 0, stats_need * sizeof(double), st));
  Sched s{c, st, py.clouds};
  const int64_t xyz_cs = (int64_t)py.S * 3, neigh_cs = (int64_t)py.S * kKnn;
  const int32_t* nb_l = py.neigh + (int64_t)py.off[level] * kKnn;
  const Act enc = s.lse_uv(b.lfa1, b.lse_w8, py.xyz + (int64_t)py.off[level] * 3, xyz_cs, nb_l, neigh_cs, n, nullptr, nullptr, nullptr);
  Act enc2;
  if (fused) {
    Act f;
    f.C = b.d / 2; f.rows = n; f.act = 1;
    f.p = c->ws.get<float>((size_t)py.clouds * n * f.C);
    if (c->ws.overflow) return overflow_fail(c, "workspace exhausted in lfa_enc2_probe");
    HIP_OK(c, hipMemsetAsync(f.p, 0, sizeof(float) * py.clouds * n * f.C, st));
    Sched::AttEnc2 e2;
    e2.w = &b.lfa2;
    s.att(b.att1, f, enc, nb_l, neigh_cs, n, nullptr, 0, &e2);
    if (!c->ws.overflow && !e2.done) return fail(c, "lfa_enc2_probe: the first pooling of level %d does not produce lfa.mlp2", level);
    enc2 = e2.out;
  } else {
    enc2 = s.mlp2d(b.lfa2, Sched::seg_of(enc, nb_l, neigh_cs), nullptr, M, true);
  }
  if (c->ws.overflow) {
    if (c->call.sched_error) return fail(c, "lfa_enc2_probe: %s (level %d)", c->call.sched_error, level);
    return overflow_fail(c, "workspace exhausted in lfa_enc2_probe");
  }
  HIP_OK(c, hipMemcpyAsync(rows_out, enc2.p, sizeof(float) * py.clouds * M * ch, hipMemcpyDeviceToDevice, st));
  HIP_OK(c, hipMemcpyAsync(stats_out, enc2.gn.stats, sizeof(double) * py.clouds * b.lfa2.groups * kGnWords, hipMemcpyDeviceToDevice, st));
  return 0;
}

// RandLA.forward (RandLANet.py:311-372).  in0/in1: the (possibly concatenated / gathered) input features.
// cache: the position-encoding branch computed once per registration (EncCache, engine_ctx.h).
int randla_forward(dsir_ctx* c, const RandlaW& w, const Seg& in0, const Seg* in1, const Pyramid& py, float* feat_out,
                   float* logits_out, EncCache* cache) {
  const dsir_cfg& g = c->cfg;
  const int L = g.num_layers;
  hipStream_t st = c->stream;
  Sched s{c, st, py.clouds};
  const size_t stats_need = gn_pass_words(py.clouds);
  if (c->call.stats_prezeroed && c->call.stats_base + stats_need <= c->stats_cap) {
    c->call.stats_top = c->call.stats_base;               // zeroed by register_enqueue together with the other passes' regions
    c->call.stats_base += stats_need;
  } else {
    c->call.stats_top = 0;
    if (stats_need > c->stats_cap) return fail(c, "stats arena too small (%zu > %zu)", stats_need, c->stats_cap);
    HIP_OK(c, hipMemsetAsync(c->stats, 0, stats_need * sizeof(double), st));
  }

  const int64_t xyz_cs = (int64_t)py.S * 3, neigh_cs = (int64_t)py.S * kKnn, sub_cs = (int64_t)py.S1 * kKnn, interp_cs = py.S;
  // Deep-level walker (walk.hip): with a few clouds in flight the layers from level 1's pooling down to the decoder block of level 2
  // run as phases of ONE launch.  Which launches become phases is decided layer by layer (Sched::gemm / att: the same kernels, the
  // same bits); the position-encoding branch of the deep levels (lfa.mlp1, lfa.mlp2: row-streaming kernels the walker does not hold,
  // inputs the pyramid alone) is computed ahead of the chain so that it does not cut the chain in pieces.
  static const int walk_from = 2;                            // first level inside the walker
  const bool walk = c->walk_mode && c->walk_dev && py.clouds <= dsir_ctx::kWalkClouds && L > walk_from &&
                    c->call.walk_used < dsir_ctx::kWalkSlots;
  WalkProgram wprog;
  wprog.clouds = py.clouds;
  wprog.flags = c->walk_flags;
  wprog.wpc = c->walk_wpc > 0 ? c->walk_wpc : (py.clouds <= 8 ? 32 : 16);   // 256 workgroups: one per CU (the walker holds the widest bodies' registers)
  const bool reuse = cache && cache->valid;
  auto enc_of = [&](int l) {      // lfa.mlp1 of level l (RandLANet.py:176-177): per-point tables (levels 0 / 1) or the stored rows
    const BlockW& b = w.blk[l];
    const int n = py.nl[l];
    const float* xyz_l = py.xyz + (int64_t)py.off[l] * 3;
    const int32_t* nb_l = py.neigh + (int64_t)py.off[l] * kKnn;
    const bool uvl = b.lse_w8 && lse_uv_enabled();     // this level's lfa.mlp1 rows are rebuilt from per-point tables, never stored
    return reuse ? cache->enc[l]
           : uvl ? s.lse_uv(b.lfa1, b.lse_w8, xyz_l, xyz_cs, nb_l, neigh_cs, n, cache ? cache->uv_buf[l] : nullptr,
                            cache ? cache->dist_buf[l] : nullptr, cache ? cache->enc_stats[l] : nullptr)
                 : s.mlp2d_lse(b.lfa1, xyz_l, xyz_cs, nb_l, neigh_cs, n, cache ? cache->enc_buf[l] : nullptr,
                               cache ? cache->enc_stats[l] : nullptr);
  };
  auto enc2_of = [&](int l, const Act& enc) {   // lfa.mlp2 on top of it (RandLANet.py:186)
    const BlockW& b = w.blk[l];
    const int n = py.nl[l];
    const int32_t* nb_l = py.neigh + (int64_t)py.off[l] * kKnn;
    return reuse ? cache->enc2[l]
                 : s.mlp2d(b.lfa2, Sched::seg_of(enc, enc.uv ? nb_l : nullptr, enc.uv ? neigh_cs : 0), nullptr, n * kKnn, true,
                           cache ? cache->enc2_buf[l] : nullptr, cache ? cache->enc2_stats[l] : nullptr);
  };
  Act enc_pre[DSIR_MAX_LEVELS], enc2_pre[DSIR_MAX_LEVELS];
  if (w.ppf && !in1) return fail(c, "randla_forward: the point-pair-feature layer needs normals");
  Act x = w.ppf ? s.ppf_pre(w.pre, in0, *in1, py.neigh, neigh_cs, py.nl[0]) : s.mlp2d(w.pre, in0, in1, py.nl[0], true);
  std::vector<Act> skips;
  for (int l = 0; l < L; ++l) {
    const BlockW& b = w.blk[l];
    const int n = py.nl[l];
    const int32_t* nb_l = py.neigh + (int64_t)py.off[l] * kKnn;
    const Seg xin = Sched::seg_of(x);
    Act f, skipb;
    const bool ahead = walk && l >= walk_from;       // computed before the chain started (below)
    const bool paired = s.mlp2d_pair(b, xin, n, f, skipb);
    if (!paired) f = s.mlp2d(b.mlp1, xin, nullptr, n, true);
    const Act enc = ahead ? enc_pre[l] : enc_of(l);
    const int s2_mode = reuse ? 2 : 1;      // iteration 0 stores the pyramid-only half of the scores, later iterations load it
    // table-only rows, not from the cache: the first pooling rebuilds every row of lfa.mlp1 anyway and writes lfa.mlp2 of it as well
    // (level 0), into the storage enc2_of() would have used - the cache's when there is one, so later iterations read it as before
    // Only where that launch fills the chip: its grid is the virtual grid of the statistics (one wave per n / 32 rows of a cloud, fixed by
    // n), while the pooling alone spreads a small launch over 512 workgroups of one-unit waves - with a few clouds in flight (the
    // captured batch-1 registration) the two-launch schedule stands, unmeasured against the other there.
    static const bool no_att_enc2 = tuning_flag("DSIR_NO_ATT_ENC2");   // A/B switch: lfa.mlp2 as a launch of its own (pw_stream.hip)
    static const long long att_enc2_min = tuning_int("DSIR_ATT_ENC2_MIN_BLOCKS", 512);   // tuning hook: workgroups of the producing launch
    Sched::AttEnc2 e2;
    if (!no_att_enc2 && !reuse && !ahead && enc.uv && !enc.p && b.d == 16 &&
        (int64_t)((att_pool16_gn_contributions(n) + 3) / 4) * py.clouds >= att_enc2_min) {
      e2.w = &b.lfa2;
      e2.buf = cache ? cache->enc2_buf[l] : nullptr;
      e2.stats = cache ? cache->enc2_stats[l] : nullptr;
    }
    Act agg = s.att(b.att1, f, enc, nb_l, neigh_cs, n, cache ? cache->s2_buf[l][0] : nullptr, s2_mode, e2.w ? &e2 : nullptr);
    Act a1 = s.mlp2d(b.att1.mlp, Sched::seg_of(agg), nullptr, n, true);
    const Act enc2 = ahead ? enc2_pre[l] : (e2.done ? e2.out : enc2_of(l, enc));
    if (cache && !reuse) { cache->enc[l] = enc; cache->enc2[l] = enc2; }
    Act agg2 = s.att(b.att2, a1, enc2, nb_l, neigh_cs, n, cache ? cache->s2_buf[l][1] : nullptr, s2_mode);
    Act a2 = s.mlp2d(b.att2.mlp, Sched::seg_of(agg2), nullptr, n, true);
    Act mainb = s.mlp2d(b.mlp2, Sched::seg_of(a2), nullptr, n, false);
    if (!paired) skipb = s.mlp2d(b.skip, xin, nullptr, n, false);
    Act enc_out;
    enc_out.C = 2 * b.d; enc_out.rows = n;
    Act samp;
    samp.C = enc_out.C; samp.rows = py.nl[l + 1];
    samp.p = c->ws.get<float>((size_t)py.clouds * samp.rows * samp.C);
    if (l == 0) enc_out.p = c->ws.get<float>((size_t)py.clouds * n * enc_out.C);
    if (c->ws.overflow) {
      if (c->call.sched_error) return fail(c, "randla_forward: %s (level %d)", c->call.sched_error, l);
      return fail(c, "workspace exhausted in randla_forward (raise max_points / max_pairs)");
    }
    if (l == 0) {
      // the level-0 block output is also the decoder's last skip connection: materialise it
      launch_residual_combine(mainb.p, mainb.gn, skipb.p, skipb.gn, enc_out.C, n, py.clouds, enc_out.p, st);
      launch_gather_max(enc_out.p, (int64_t)n * enc_out.C, py.sub + (int64_t)py.soff[l] * kKnn, sub_cs, samp.C, samp.rows,
                        py.clouds, samp.p, st);
    } else {
      if (walk && l == walk_from - 1) {
        // the chain starts with this level's pooling: first the deep levels' position-encoding branch, as launches of their own
        for (int q = walk_from; q < L; ++q) { enc_pre[q] = enc_of(q); enc2_pre[q] = enc2_of(q, enc_pre[q]); }
        if (c->ws.overflow) return overflow_fail(c, "workspace exhausted in randla_forward (raise max_points / max_pairs)");
        s.rec = &wprog; s.rec_wpc = wprog.wpc;
      }
      // deeper levels: only the pooled ("randomly sampled") rows are ever read — combine inside the pooling kernel
      GmcArgs ga{mainb.p, mainb.gn, skipb.p, skipb.gn, n, py.sub + (int64_t)py.soff[l] * kKnn, sub_cs, samp.C, samp.rows, samp.p, 0};
      WalkJob wj;
      if (!(s.rec && walk_plan_gmc(ga, s.rec_wpc, &wj) && s.rec_push(wj))) {
        s.rec_flush();
        launch_gather_max_combine(mainb.p, mainb.gn, skipb.p, skipb.gn, n, py.sub + (int64_t)py.soff[l] * kKnn, sub_cs,
                                  samp.C, samp.rows, py.clouds, samp.p, st);
      }
    }
    if (l == 0) skips.push_back(enc_out);
    skips.push_back(samp);
    x = samp;
  }
  x = s.mlp2d(w.mid, Sched::seg_of(skips.back()), nullptr, py.nl[L], true);
  for (int j = 0; j < L; ++j) {
    const int lvl = L - 1 - j;
    const Act& sk = skips[skips.size() - 2 - j];
    const Seg s0 = Sched::seg_of(sk);
    const Seg s1 = Sched::seg_of(x, py.interp + py.off[lvl], interp_cs);
    if (s.rec && lvl < walk_from) { s.rec_flush(); s.rec = nullptr; }      // the chain ends with the decoder block of level walk_from
    x = s.mlp2d(w.dec[j], s0, &s1, py.nl[lvl], true);
  }
  if (s.rec) { s.rec_flush(); s.rec = nullptr; }
  if (s.rec_error) return 1;
  const int n0 = py.nl[0];
  bool fused = false;
  static const bool no_head = tuning_flag("DSIR_NO_HEAD");   // A/B switch
  if (logits_out && !no_head &&w.dec_out == 32 && g.out_feat_dim == 64 && w.fc[0].cout == 64 && w.fc[1].cout == 32) {
    // mlp_out + fc_label in one launch (head_mlp.hip); bit-identical to the four launches below
    HeadArgs h;
    h.in = Sched::seg_of(x);
    h.W1 = w.out_w; h.W2 = w.fc[0].W; h.b2 = w.fc[0].b; h.W3 = w.fc[1].W; h.b3 = w.fc[1].b; h.W4 = w.fc[2].W; h.b4 = w.fc[2].b;
    h.ncls = w.ncls; h.M = n0; h.clouds = py.clouds; h.feat_out = feat_out; h.logits_out = logits_out;
    if (c->ws.overflow) return overflow_fail(c, "workspace exhausted in randla_forward (raise max_points / max_pairs)");
    // default: the head's four layers as fp16-split products (fp32 accuracy); dsir_enable_agg_split(0) /
    // DSIR_AGG_F32: the exact-fp32 head, bit-identical to the four separate launches
    if (c->agg_split) {
      for (int k = 0; k < 4; ++k) { h.Wh[k] = w.head_wh[k]; h.Wl[k] = w.head_wl[k]; }
      fused = launch_head_mlp(h, true, st);
    }
    if (!fused) fused = launch_head_mlp(h, false, st);
  }
  LinW ow; ow.W = w.out_w; ow.b = nullptr; ow.cin = w.dec_out; ow.cout = g.out_feat_dim;
  Act feat;
  if (!fused) feat = s.linear(ow, Sched::seg_of(x), nullptr, n0, EPI_LINEAR, feat_out);
  if (logits_out && !fused) {
    Act h = s.linear(w.fc[0], Sched::seg_of(feat), nullptr, n0, EPI_ACT);
    h = s.linear(w.fc[1], Sched::seg_of(h), nullptr, n0, EPI_ACT);
    s.linear(w.fc[2], Sched::seg_of(h), nullptr, n0, EPI_LINEAR, logits_out);
  }
  if (c->ws.overflow) return overflow_fail(c, "workspace exhausted in randla_forward (raise max_points / max_pairs)");
  if (cache) cache->valid = true;
  return 0;
}

// mlp_feat (loop invariant part of Network.aggregation, model.py:218)
namespace {
// Does a launch of this size take the fused form by default?  A/B switch: DSIR_NO_FEAT_CHAIN = three point-wise launches throughout.
// The fused launch is taken from 64 workgroups of work up (feat_chain_blocks: 512 row tiles, 8192 points).  Timed at and above that
// size only: one captured pair of 5000 points (79 workgroups) registers in 2.919 ms against 2.954, 128 pairs in 0.40 of the three
// launches' time.  Smaller launches keep the three launches - untimed there, and the captured small registrations keep the launch
// census that tests/test_gpu_search_sites.py pins.  DSIR_FEAT_CHAIN_MIN_BLOCKS: tuning hook (0 = every size).
bool feat_chain_wanted(int clouds, int n) {
  static const bool off = tuning_flag("DSIR_NO_FEAT_CHAIN");
  static const long long min_blocks = tuning_int("DSIR_FEAT_CHAIN_MIN_BLOCKS", 64);
  return !off && feat_chain_blocks(clouds, n) >= min_blocks;
}
// the three layers in one launch (feat_chain.hip): clouds [0, split_cloud) into out0, the others into out1.  False: not launched -
// other layer shapes, or a configuration whose three launches run an arithmetic the kernel does not reproduce
bool mlp_feat_chain(dsir_ctx* c, const float* feat0, int clouds, int n, float* out0, float* out1, int split_cloud, int max_blocks) {
  const LinW* m = c->net.mlp_feat;
  if (m[0].cin != 64 || m[0].cout != 64 || m[1].cin != 64 || m[1].cout != 128 || m[2].cin != 128 || m[2].cout != 64) return false;
  FeatChainArgs a;
  a.X = feat0;
  a.W1 = m[0].W; a.b1 = m[0].b; a.W2 = m[1].W; a.b2 = m[1].b; a.W3 = m[2].W; a.b3 = m[2].b;
  GemmArgs last;                  // the last layer runs split exactly where Sched::linear would hand pw_tile.hip split weights
  last.W = m[2].W;
  Sched{c, c->stream, clouds}.split_of(last);
  a.W3h = last.Wh; a.W3l = last.Wl;
  a.out0 = out0; a.out1 = out1; a.split_cloud = split_cloud; a.n = n; a.clouds = clouds; a.max_blocks = max_blocks;
  return launch_feat_chain(a, c->stream);
}
bool takes_fused(FeatForm form, int clouds, int n) { return form == FeatForm::Fused || (form == FeatForm::Auto && feat_chain_wanted(clouds, n)); }
}  // namespace

float* run_mlp_feat(dsir_ctx* c, const float* feat0, int clouds, int n, float* out, FeatForm form, int max_blocks) {
  Sched s{c, c->stream, clouds};
  const NetW& w = c->net;
  if (takes_fused(form, clouds, n)) {
    float* y = out ? out : c->ws.get<float>((size_t)clouds * n * 64);
    if (c->ws.overflow) return y;                  // an exhausted arena hands out its base: nothing may run on it
    if (mlp_feat_chain(c, feat0, clouds, n, y, nullptr, clouds, max_blocks)) return y;
    if (form == FeatForm::Fused) return nullptr;
    out = y;
  }
  Act h = s.linear(w.mlp_feat[0], plain_seg(feat0, (int64_t)n * 64, 64, 64), nullptr, n, EPI_ACT);
  h = s.linear(w.mlp_feat[1], Sched::seg_of(h), nullptr, n, EPI_ACT);
  h = s.linear(w.mlp_feat[2], Sched::seg_of(h), nullptr, n, EPI_LINEAR, out);
  return h.p;
}
float* run_mlp_feat_pair(dsir_ctx* c, const float* feat0, int P, int n, float* out_a, FeatForm form, int max_blocks) {
  float* out_b = c->ws.get<float>((size_t)P * n * 64);
  if (c->ws.overflow) return out_b;
  if (takes_fused(form, 2 * P, n) && mlp_feat_chain(c, feat0, 2 * P, n, out_a, out_b, P, max_blocks)) return out_b;
  if (form == FeatForm::Fused) return nullptr;
  run_mlp_feat(c, feat0, P, n, out_a, FeatForm::Three);
  run_mlp_feat(c, feat0 + (size_t)P * n * 64, P, n, out_b, FeatForm::Three);
  return out_b;
}
// dsir_mlp_feat_probe: mlp_feat alone, by the three launches (fused = 0), the fused launch (1), or the fused launch on both halves
// of the clouds at once with two output bases (2: the second half through the arena, as a registration's ref side); max_blocks > 0
// caps the fused launch's grid
int run_mlp_feat_probe(dsir_ctx* c, const float* feat0, int clouds, int n, int fused, int max_blocks, float* out) {
  if (fused == 2) {
    const int P = clouds / 2;
    const float* half = run_mlp_feat_pair(c, feat0, P, n, out, FeatForm::Fused, max_blocks);
    if (c->ws.overflow) return overflow_fail(c, "workspace exhausted in mlp_feat_probe");
    if (!half) return fail(c, "mlp_feat_probe: the fused launch does not take this configuration");
    HIP_OK(c, hipMemcpyAsync(out + (size_t)P * n * 64, half, sizeof(float) * P * n * 64, hipMemcpyDeviceToDevice, c->stream));
    return 0;
  }
  const float* y = run_mlp_feat(c, feat0, clouds, n, out, fused ? FeatForm::Fused : FeatForm::Three, max_blocks);
  if (c->ws.overflow) {
    if (c->call.sched_error) return fail(c, "mlp_feat_probe: %s", c->call.sched_error);
    return overflow_fail(c, "workspace exhausted in mlp_feat_probe");
  }
  if (!y) return fail(c, "mlp_feat_probe: the fused launch does not take this configuration");
  return 0;
}
// normalize(mlp_proj(F + mlp_att([xyz; score])))   (model.py:223-234)
// ex: what the descriptor search wants written besides the descriptors (AggExtras); true: the epilogue wrote it
bool run_att_proj(dsir_ctx* c, const float* xyz, int64_t xyz_cs, const float* score, const float* F, int clouds, int n,
                  float* desc, const AggExtras* ex) {
  Sched s{c, c->stream, clouds};
  const NetW& w = c->net;
  static const bool no_agg = tuning_flag("DSIR_NO_AGG");   // A/B switch
  const LinW* m = w.mlp_att;
  if (!no_agg && m[0].cin == 4 && m[0].cout == 32 && m[1].cout == 64 && m[2].cout == 128 && m[3].cout == 256 &&
      m[4].cout == 64 && w.mlp_proj.cin == 64 && w.mlp_proj.cout == 64) {
    AggArgs a;
    a.xyz = xyz; a.xyz_cs = xyz_cs; a.score = score; a.F = F;
    a.W1 = m[0].W; a.b1 = m[0].b; a.W2 = m[1].W; a.b2 = m[1].b; a.W3 = m[2].W; a.b3 = m[2].b;
    a.W4 = m[3].W; a.b4 = m[3].b; a.W5 = m[4].W; a.b5 = m[4].b; a.W6 = w.mlp_proj.W; a.b6 = w.mlp_proj.b;
    a.desc = desc; a.n = n; a.clouds = clouds;
    // default: the chain's wide layers as fp16-split products on the fp16 matrix pipe (agg_chain.hip: fp32 accuracy, not the
    // fp32 kernel's bits); dsir_enable_agg_split(0) / DSIR_AGG_F32: the exact-fp32 chain, bit-identical to the unfused launches below
    static const bool no_fuse = tuning_flag("DSIR_NO_AGG_EXTRAS");   // A/B switch: the search prepares its operands itself
    if (c->agg_split) {
      for (int k = 0; k < 5; ++k) { a.Wh[k] = c->agg_wh[k]; a.Wl[k] = c->agg_wl[k]; }
      if (ex && !no_fuse) { a.sq = ex->sq; a.hi = ex->hi; a.lo = ex->lo; a.packed_init = ex->packed_init; }
      if (launch_agg_chain(a, true, c->stream)) return ex && !no_fuse;
      a.sq = nullptr; a.hi = a.lo = nullptr; a.packed_init = nullptr;
    }
    if (launch_agg_chain(a, false, c->stream)) return false;
  }
  const Seg sx = plain_seg(xyz, xyz_cs, 3, 3);
  const Seg ss = plain_seg(score, n, 1, 1);
  Act h = s.linear(w.mlp_att[0], sx, &ss, n, EPI_ACT);
  for (int k = 1; k < 4; ++k) h = s.linear(w.mlp_att[k], Sched::seg_of(h), nullptr, n, EPI_ACT);
  h = s.linear(w.mlp_att[4], Sched::seg_of(h), nullptr, n, EPI_LINEAR, nullptr, F);
  s.linear(w.mlp_proj, Sched::seg_of(h), nullptr, n, EPI_L2NORM, desc);
  return false;
}

int build_pyramid(dsir_ctx* c, const float* points, int stride, int clouds, int n, float* xyz, int32_t* neigh,
                  int32_t* sub, int32_t* interp) {
  const dsir_cfg& g = c->cfg;
  Pyramid p;
  fill_pyramid_layout(g, clouds, n, p);
  if (p.nl[g.num_layers - 1] < kKnn)
    return fail(c, "cloud too small: level %d has %d < %d points (need n >= %d)", g.num_layers - 1,
                p.nl[g.num_layers - 1], kKnn, kKnn * 64);
  hipStream_t st = c->stream;
  const int64_t xyz_cs = (int64_t)p.S * 3, neigh_cs = (int64_t)p.S * kKnn, sub_cs = (int64_t)p.S1 * kKnn;
  PyramidLevels lv{};
  lv.L = g.num_layers; lv.S = p.S; lv.S1 = p.S1;
  for (int l = 0; l <= g.num_layers; ++l) { lv.nl[l] = p.nl[l]; lv.off[l] = p.off[l]; lv.soff[l] = p.soff[l]; }
  // every level's points are a prefix of the level above, hence of the input cloud (data_base.py:166-172): one launch for all
  launch_copy_xyz_levels(points, (int64_t)n * stride, stride, lv, clouds, xyz, xyz_cs, st);
  static const bool no_grid = tuning_flag("DSIR_NO_GRID");   // A/B switch
  static const int grid_min = (int)tuning_int("DSIR_GRID_MIN", 1024);   // tuning hook
  static const bool no_nn1_grid = tuning_flag("DSIR_NO_NN1_GRID");   // A/B switch: brute-force interpolation search throughout
  static const long long nn1_grid_min = tuning_int("DSIR_NN1_GRID_MIN", 65536);   // tuning hook
  // interp_idx is read off the finished 16-NN lists by the launch that writes sub_idx (knn.hip, interp_lists_kernel: same bits), in
  // place of one search per level.  A/B switch: the searches (the kind-0 jobs, launch_nn1_grid, launch_nn1) and launch_copy_sub_levels
  static const bool nn1_search = tuning_flag("DSIR_NO_INTERP_LISTS");
  auto finish = [&]() {      // the last launch: every list exists
    if (nn1_search) launch_copy_sub_levels(neigh, neigh_cs, lv, clouds, sub, sub_cs, st);
    else launch_interp_lists(points, (int64_t)n * stride, stride, neigh, neigh_cs, lv, clouds, sub, sub_cs, interp, p.S, st);
  };
  // interpolation search of level l (support = level l + 1) through level l + 1's grid: when that level has one and the launch has
  // queries enough to fill the chip with one lane per query (same bits either way)
  auto nn1_by_grid = [&](int l) {
    return !no_grid && !no_nn1_grid && l + 1 < g.num_layers && p.nl[l + 1] >= grid_min && (int64_t)clouds * p.nl[l] >= nn1_grid_min;
  };
  // the grid scratch of every level stays until the pyramid is done: the level above's sorted points are the QUERIES of this level's
  // interpolation search (in cell order: a wave's lanes walk neighbouring cells)
  const size_t mark = c->ws.mark();
  const void* prev_scratch = nullptr;
  // Every level's searches read the input points alone (the levels are prefixes of the cloud), so the pyramid is THREE launches instead
  // of a chain of ten - the grids of the large levels, their searches, and everything else (the interpolation searches of all levels,
  // the 16-NN of the levels without a grid) - plus one per interpolation search that walks a grid (large launches).  With one pair in
  // flight (the reference's evaluation mode, test.py:56) the chain was 226 us of the registration's 3.05 ms, now 135; with eight, 373.
  // The same kernels' bodies on the same operands: same bits (tests/test_gpu_parity.py, two-process A/B).
  static const bool no_merge = tuning_flag("DSIR_NO_PYRAMID_MERGE");   // A/B switch
  if (!no_merge && g.num_layers <= KnnSmallJobs::kMax / 2) {
    int ngrid = 0, gn[4], grid_of[8];
    int32_t* gout[4];
    KnnSmallJobs jobs{};
    bool ok = true;
    for (int l = 0; l < g.num_layers && ok; ++l) {
      grid_of[l] = -1;
      if (p.nl[l] >= grid_min && !no_grid) {
        ok = knn16_grid_can_merge(p.nl[l]) && ngrid < 4;
        if (ok) { gn[ngrid] = p.nl[l]; gout[ngrid] = neigh + (int64_t)p.off[l] * kKnn; grid_of[l] = ngrid++; }
      } else {
        jobs.job[jobs.njobs++] = {knn16_takes_wave_kernel(p.nl[l], clouds) ? 1 : 2, p.nl[l], 0, neigh + (int64_t)p.off[l] * kKnn, neigh_cs, 0};
      }
      if (nn1_search && !nn1_by_grid(l)) jobs.job[jobs.njobs++] = {0, p.nl[l], p.nl[l + 1], interp + p.off[l], (int64_t)p.S, 0};
    }
    if (ok) {
      void* gscr[4];
      for (int k = 0; k < ngrid; ++k) gscr[k] = c->ws.raw(knn_grid_scratch_bytes(clouds, gn[k]));
      if (c->ws.overflow) return fail(c, "workspace exhausted in the KNN pyramid");
      if (ngrid) launch_knn16_grid_levels(points, (int64_t)n * stride, stride, ngrid, gn, clouds, gout, neigh_cs, gscr, st);
      launch_knn_small_levels(points, (int64_t)n * stride, stride, clouds, jobs, st);
      for (int l = 0; l + 1 < g.num_layers; ++l)
        if (nn1_search && nn1_by_grid(l))      // level l + 1 has a grid, hence the larger level l too: the search walks the one, its queries in the cell order of the other
          launch_nn1_grid(p.nl[l], p.nl[l + 1], clouds, interp + p.off[l], p.S, gscr[grid_of[l + 1]], gscr[grid_of[l]], st);
      c->ws.release(mark);
      finish();
      return 0;
    }
  }
  for (int l = 0; l < g.num_layers; ++l) {
    if (p.nl[l] >= grid_min && !no_grid) {
      // large levels: exact grid-pruned search (knn_grid.hip); same bits as the brute force
      void* scratch = c->ws.raw(knn_grid_scratch_bytes(clouds, p.nl[l]));
      if (c->ws.overflow) return fail(c, "workspace exhausted in the KNN pyramid");
      launch_knn16_grid(points, (int64_t)n * stride, stride, p.nl[l], clouds, neigh + (int64_t)p.off[l] * kKnn, neigh_cs,
                        scratch, st);
      // this level's points are the support of the level above's interpolation search: it walks the grid just built (the level above
      // is no smaller, so it took this branch too and prev_scratch is its grid)
      if (nn1_search && l > 0 && nn1_by_grid(l - 1))
        launch_nn1_grid(p.nl[l - 1], p.nl[l], clouds, interp + p.off[l - 1], p.S, scratch, prev_scratch, st);
      prev_scratch = scratch;
    } else {
      prev_scratch = nullptr;
      launch_knn16(points, (int64_t)n * stride, stride, p.nl[l], clouds, neigh + (int64_t)p.off[l] * kKnn, neigh_cs, st);
    }
    if (nn1_search && !nn1_by_grid(l)) launch_nn1(points, (int64_t)n * stride, stride, p.nl[l], p.nl[l + 1], clouds, interp + p.off[l], p.S, st);
  }
  c->ws.release(mark);   // stream-ordered: later users of this memory run after the query kernels
  // sub_idx of level l = the neighbour lists of its first n_{l+1} points: all levels in one launch
  finish();
  return 0;
}

}  // namespace dsir
