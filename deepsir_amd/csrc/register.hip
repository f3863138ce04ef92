// The registration loop (forward_align_4) behind dsir_register, eager or as a captured graph, and forward_pair.
#include <cstring>

#include "engine_ctx.h"

using namespace dsir;

extern "C" {

// Pyramids + forward_pair (model.py:609-648) of P pairs: everything both dsir_register and dsir_forward_pair need.
struct PairStage {
  Pyramid ps, pr;
  float *feat_s, *feat_r, *logit_s, *logit_r, *score_s, *score_r;
  int32_t *label_s, *label_r;     // only when want_label
  float *rxyz;                    // == pr.xyz
};
// pre: fills / copies the caller wants done before anything else; the stage adds its own (staging the input clouds, presetting the
// score reductions) and issues them all as ONE launch (launch_mem_ops)
static int forward_pair_stage(dsir_ctx* c, const dsir_pair_batch* in, bool want_score, bool want_label, PairStage& S,
                              int32_t* invalid = nullptr, MemOps pre = MemOps()) {
  const dsir_cfg& g = c->cfg;
  const int P = in->pairs, J = in->n_src, K = in->n_ref, cin = g.feat_len;
  if (P < 1 || P > g.max_pairs) return fail(c, "pairs=%d outside [1,%d]", P, g.max_pairs);
  if (J > g.max_points || K > g.max_points) return fail(c, "cloud larger than max_points=%d", g.max_points);
  if (!in->points_src || !in->points_ref) return fail(c, "null point clouds");
  const bool have_py = in->src_xyz && in->src_neigh && in->src_sub && in->src_interp && in->ref_xyz && in->ref_neigh &&
                       in->ref_sub && in->ref_interp;
  const bool any_py = in->src_xyz || in->src_neigh || in->src_sub || in->src_interp || in->ref_xyz || in->ref_neigh ||
                      in->ref_sub || in->ref_interp;
  if (any_py && !have_py) return fail(c, "either all eight pyramid tensors or none must be supplied");
  hipStream_t st = c->stream;
  Arena& ws = c->ws;

  // ---- pyramids of src and ref (engine-owned when built here)
  Pyramid& ps = S.ps; Pyramid& pr = S.pr;
  fill_pyramid_layout(g, P, J, ps);
  fill_pyramid_layout(g, P, K, pr);
  if (ps.nl[3] < kKnn || pr.nl[3] < kKnn) return fail(c, "cloud too small: need at least %d points", kKnn * 64);
  const bool joint = (J == K);   // src and ref share the feature extractor: run them as one batch of 2P clouds
  float* feat_all = ws.get<float>((size_t)P * (J + K) * 64);
  float* logit_all = ws.get<float>((size_t)P * (J + K) * g.num_classes);
  float* score_all = ws.get<float>((size_t)P * (J + K));
  int32_t* label_all = want_label ? ws.get<int32_t>((size_t)P * (J + K)) : nullptr;
  float* feat_s = feat_all; float* feat_r = feat_all + (size_t)P * J * 64;
  float* score_s = score_all; float* score_r = score_all + (size_t)P * J;
  float* logit_s = logit_all; float* logit_r = logit_all + (size_t)P * J * g.num_classes;
  int32_t* label_s = label_all; int32_t* label_r = label_all ? label_all + (size_t)P * J : nullptr;

  // pyramid storage: [src clouds | ref clouds] contiguous when joint
  float* pxyz = ws.get<float>((size_t)P * (ps.S + pr.S) * 3);
  int32_t* pneigh = ws.get<int32_t>((size_t)P * (ps.S + pr.S) * kKnn);
  int32_t* psub = ws.get<int32_t>((size_t)P * (ps.S1 + pr.S1) * kKnn);
  int32_t* pinterp = ws.get<int32_t>((size_t)P * (ps.S + pr.S));
  float* feats_in = ws.get<float>((size_t)P * (J + K) * cin);
  if (ws.overflow) return overflow_fail(c, "workspace exhausted (raise max_points / max_pairs)");
  float* rxyz = pxyz + (size_t)P * ps.S * 3;
  int32_t* rneigh = pneigh + (size_t)P * ps.S * kKnn;
  int32_t* rsub = psub + (size_t)P * ps.S1 * kKnn;
  int32_t* rinterp = pinterp + (size_t)P * ps.S;
  // the score stage's reduction targets (max feature, label weight, probability per cloud) live from here on: preset to -inf below
  float* score_red = want_score ? ws.get<float>((size_t)2 * P * 4) : nullptr;
  if (ws.overflow) return overflow_fail(c, "workspace exhausted (raise max_points / max_pairs)");
  pre.copy(feats_in, in->points_src, sizeof(float) * P * J * cin);
  pre.copy(feats_in + (size_t)P * J * cin, in->points_ref, sizeof(float) * P * K * cin);
  pre.fill(score_red, sizeof(float) * 2 * P * 4, 0xff800000u);
  if (have_py) {
    pre.copy(pxyz, in->src_xyz, sizeof(float) * P * ps.S * 3);
    pre.copy(rxyz, in->ref_xyz, sizeof(float) * P * pr.S * 3);
  }
  if (pre.overflow) return fail(c, "forward_pair: more than %d opening fills / copies", MemOps::kMax);
  launch_mem_ops(pre, st);
  if (have_py) {
    // caller-supplied indices: copied with every entry clamped into its level's range (a bad index can never fault a
    // gather), out-of-range entries reported through bit 1 of the pair's invalid flag
    auto copy_idx = [&](const Pyramid& py, const int32_t* nb, const int32_t* sb, const int32_t* ip, int32_t* nbo, int32_t* sbo,
                        int32_t* ipo) {
      PyramidIdxCopy a{};
      a.neigh = nb; a.sub = sb; a.interp = ip; a.neigh_out = nbo; a.sub_out = sbo; a.interp_out = ipo;
      a.S = py.S; a.S1 = py.S1; a.levels = g.num_layers;
      for (int l = 0; l <= g.num_layers; ++l) { a.nl[l] = py.nl[l]; a.off[l] = py.off[l]; a.soff[l] = py.soff[l]; }
      a.flag = invalid; a.flag_mod = P;
      launch_copy_pyramid_idx(a, P, st);
    };
    copy_idx(ps, in->src_neigh, in->src_sub, in->src_interp, pneigh, psub, pinterp);
    copy_idx(pr, in->ref_neigh, in->ref_sub, in->ref_interp, rneigh, rsub, rinterp);
  } else if (joint) {
    if (int r = build_pyramid(c, feats_in, cin, 2 * P, J, pxyz, pneigh, psub, pinterp)) return r;
  } else {
    if (int r = build_pyramid(c, feats_in, cin, P, J, pxyz, pneigh, psub, pinterp)) return r;
    if (int r = build_pyramid(c, feats_in + (size_t)P * J * cin, cin, P, K, rxyz, rneigh, rsub, rinterp)) return r;
  }
  ps.xyz = pxyz; ps.neigh = pneigh; ps.sub = psub; ps.interp = pinterp;
  pr.xyz = rxyz; pr.neigh = rneigh; pr.sub = rsub; pr.interp = rinterp;

  // ---- forward_pair (model.py:609-648): feature RandLA + score on src and ref
  const size_t mark0 = ws.mark();
  ScoreScratch sc;
  // the extractor's input rows; use_ppf: columns 0 - 2 the point, 3 - 5 its normal (RandLANet.py:326)
  const bool ppf = c->net.feat.ppf;
  auto extract = [&](const float* rows, int n, const Pyramid& py, float* feat, float* logit) {
    const Seg pts = plain_seg(rows, (int64_t)n * cin, ppf ? 3 : cin, cin), nrm = plain_seg(rows + 3, (int64_t)n * cin, 3, cin);
    return randla_forward(c, c->net.feat, pts, ppf ? &nrm : nullptr, py, feat, logit);
  };
  if (joint) {
    Pyramid pa = ps;
    pa.clouds = 2 * P;
    if (int r = extract(feats_in, J, pa, feat_all, logit_all)) return r;
    if (want_score) {
      sc.red = score_red; sc.prob = ws.get<float>((size_t)2 * P * J); sc.label = ws.get<int32_t>((size_t)2 * P * J);
      launch_score(feat_all, logit_all, g.num_classes, pxyz, (int64_t)ps.S * 3, pneigh, (int64_t)ps.S * kKnn, 2 * P, J, sc,
                   score_all, label_all, st, /*red_preset=*/true);
    }
  } else {
    if (int r = extract(feats_in, J, ps, feat_s, logit_s)) return r;
    ws.release(mark0);
    if (int r = extract(feats_in + (size_t)P * J * cin, K, pr, feat_r, logit_r)) return r;
    ws.release(mark0);
    if (want_score) {
      const int nmax = J > K ? J : K;
      sc.red = score_red; sc.prob = ws.get<float>((size_t)P * nmax); sc.label = ws.get<int32_t>((size_t)P * nmax);
      launch_score(feat_s, logit_s, g.num_classes, pxyz, (int64_t)ps.S * 3, pneigh, (int64_t)ps.S * kKnn, P, J, sc, score_s, label_s, st, true);
      sc.red = score_red + (size_t)P * 4;      // the ref clouds' own targets (the src launch is still reading the first set)
      launch_score(feat_r, logit_r, g.num_classes, rxyz, (int64_t)pr.S * 3, rneigh, (int64_t)pr.S * kKnn, P, K, sc, score_r, label_r, st, true);
    }
  }
  ws.release(mark0);
  S.feat_s = feat_s; S.feat_r = feat_r; S.logit_s = logit_s; S.logit_r = logit_r; S.score_s = score_s; S.score_r = score_r;
  S.label_s = label_s; S.label_r = label_r; S.rxyz = rxyz;
  return 0;
}

static int register_enqueue(dsir_ctx* c, Call& call, const dsir_pair_batch* in, int n_iter, const dsir_pair_result* out) {
  const dsir_cfg& g = c->cfg;
  const int P = in->pairs, J = in->n_src, K = in->n_ref;
  if (n_iter < 1) return fail(c, "n_iter must be >= 1");
  hipStream_t st = c->stream;
  Arena& ws = c->ws;
  PairStage S;
  // What opens a registration goes out as ONE launch (launch_mem_ops, issued by forward_pair_stage together with the staging of the
  // input clouds): the pairs' flags, and the GroupNorm statistics of ALL passes of this call (feature extractor on 2 P clouds, n_iter
  // inlier passes on P) plus those of the inlier model's cached position-encoding branch (EncCache) in one zeroed region - round 4
  // spent six memset / memcpy launches here
  MemOps pre;
  pre.fill(out->invalid, sizeof(int32_t) * P);
  if (int r = call.begin_walker()) return r;
  const size_t cache_stats = EncCache::stats_words(g, P);
  double* cache_stats_at = nullptr;
  {
    const size_t total = gn_register_words(P, n_iter);
    if (total + cache_stats <= c->stats_cap) {
      pre.fill(c->stats, (total + cache_stats) * sizeof(double));
      // ... and the tile queues / completion counters of the deep-level walker's programs (walk.hip), one per pass
      if (c->walk_mode && c->walk_ctr && P <= dsir_ctx::kWalkClouds)
        pre.fill(c->walk_ctr, sizeof(unsigned) * dsir_ctx::kWalkSlots * dsir_ctx::kWalkClouds * kWalkCtrWords);
      cache_stats_at = c->stats + total;
      c->call.stats_prezeroed = true;
    }
  }
  if (int r = forward_pair_stage(c, in, true, false, S, out->invalid, pre)) return r;
  const Pyramid& ps = S.ps; const Pyramid& pr = S.pr;
  float *feat_s = S.feat_s, *feat_r = S.feat_r, *score_s = S.score_s, *score_r = S.score_r, *rxyz = S.rxyz;
  const float* pxyz = ps.xyz;

  // ---- loop invariants of Network.aggregation: the whole ref side and mlp_feat(feat_src)
  float* desc_r = ws.get<float>((size_t)P * K * 64);
  float* desc_s = ws.get<float>((size_t)P * J * 64);
  float* F_s = ws.get<float>((size_t)P * J * 64);
  float* xyz_cur = ws.get<float>((size_t)P * J * 3);
  float* logits_it = ws.get<float>((size_t)P * J);
  int32_t* idx_it = ws.get<int32_t>((size_t)P * J);
  float* T_it = ws.get<float>((size_t)P * 12);
  // nearest ref descriptor: the mode (search_plan.h) and every operand of it.  The ref side is loop invariant.
  static const long long screen_min = tuning_int("DSIR_SCREEN_MIN_WORK", kScreenMinWork);   // A/B hook
  const SearchSwitches sw{c->screen_mode, c->prune_min_points, c->prune_min_rows, screen_min};
  DescSearch search{c, search_mode(sw, P, J, K, in->forced_idx != nullptr, nn_prune_supported(P, J, K)), P, J, K, /*timed=*/true, /*counted=*/true};
  search.alloc(/*with_match_scratch=*/true);
  // chunk partials of the pose solve on large clouds (kabsch.hip)
  const size_t kab_bytes = kabsch_part_bytes(P, J, c->kabsch_chunked_min);
  double* kab_part = kab_bytes ? ws.get<double>(kab_bytes / sizeof(double)) : nullptr;
  EncCache enc_cache;
  static const bool no_hoist = tuning_flag("DSIR_NO_HOIST");   // A/B switch
  const bool hoist = !no_hoist && n_iter > 1;
  if (hoist)
    if (int r = enc_cache.plan(c, ps, cache_stats_at)) return r;
  if (ws.overflow) return overflow_fail(c, "workspace exhausted (raise max_points / max_pairs)");
  const size_t mark1 = ws.mark();
  {
    // mlp_feat of both sides: F_s straight into the storage that outlives the iterations, F_r into the arena.  Clouds of one size
    // whose features lie one after the other (the extractor ran on 2 P clouds) are one launch where the fused form runs.
    float* F_r;
    if (J == K && feat_r == feat_s + (size_t)P * J * 64) {
      F_r = run_mlp_feat_pair(c, feat_s, P, J, F_s);
    } else {
      run_mlp_feat(c, feat_s, P, J, F_s);
      F_r = run_mlp_feat(c, feat_r, P, K);
    }
    launch_copy_xyz(pxyz, (int64_t)ps.S * 3, 3, J, P, xyz_cur, (int64_t)J * 3, st);      // xyz_cur = level-0 src coordinates
    const bool ref_prepared = run_att_proj(c, rxyz, (int64_t)pr.S * 3, score_r, F_r, P, K, desc_r, search.ref_extras());
    if (out->desc_ref) HIP_OK(c, hipMemcpyAsync(out->desc_ref, desc_r, sizeof(float) * P * K * 64, hipMemcpyDeviceToDevice, st));
    if (int r = search.prepare_ref(desc_r, ref_prepared, rxyz, (int64_t)pr.S * 3)) return r;
    ws.release(mark1);
  }

  for (int it = 0; it < n_iter; ++it) {
    int32_t* idx_out = out->idx ? out->idx + (size_t)it * P * J : idx_it;
    float* logit_out = out->logits ? out->logits + (size_t)it * P * J : logits_it;
    // aggregation of the (transformed) src cloud; its epilogue also leaves what this iteration's search needs of the descriptors
    // (screened search: the fp16 operand pair + norms; exhaustive search: norms + preset result slots)
    DescSearch::Iter si;
    si.it = it;
    si.src_prepared = run_att_proj(c, xyz_cur, (int64_t)J * 3, score_s, F_s, P, J, desc_s, search.src_extras());
    ws.release(mark1);
    if (out->desc_src)
      HIP_OK(c, hipMemcpyAsync(out->desc_src + (size_t)it * P * J * 64, desc_s, sizeof(float) * P * J * 64, hipMemcpyDeviceToDevice, st));
    if (in->forced_idx) { si.forced = in->forced_idx + (size_t)it * P * J; si.invalid = out->invalid; }
    if (int r = search.run(desc_s, desc_r, idx_out, si)) return r;
    // inlier RandLA on [xyz_src(t); xyz_ref[idx]] with the SRC pyramid (model.py:574-577)
    const Seg s0 = plain_seg(xyz_cur, (int64_t)J * 3, 3, 3);
    const Seg s1 = plain_seg(rxyz, (int64_t)pr.S * 3, 3, 3, idx_out, J);
    if (int r = randla_forward(c, c->net.inl, s0, &s1, ps, nullptr, logit_out, hoist ? &enc_cache : nullptr)) return r;
    ws.release(mark1);
    // weighted Kabsch + transform update (model.py:586-595)
    KabschArgs a{};
    a.src = xyz_cur; a.ref = rxyz; a.idx = idx_out; a.w = logit_out; a.src_stride = (int64_t)J * 3; a.ref_stride = (int64_t)pr.S * 3;
    a.sigmoid = 1; a.pairs = P; a.m = J; a.T = T_it; a.invalid = out->invalid;
    a.src_out = xyz_cur; a.src_out_stride = (int64_t)J * 3;
    a.T_cum = out->transforms + (size_t)it * 12; a.T_prev = it ? out->transforms + (size_t)(it - 1) * 12 : nullptr;
    a.T_stride = (int64_t)n_iter * 12;
    a.matched_out = (it == n_iter - 1) ? out->pt_ref_new : nullptr;
    a.part = kab_part; a.chunk_min = c->kabsch_chunked_min;
    launch_kabsch(a, st);
  }
  if (c->ws.overflow) return overflow_fail(c, "workspace exhausted (raise max_points / max_pairs in dsir_cfg)");   // before a capture ends
  return 0;
}

// Graph mode: capture one registration, instantiate it and keep it in c->graphs (the oldest evicted beyond kMaxGraphs).  Every exit
// leaves the context clean (Capture's destructor): the capture ended, the graph destroyed, the walker programs' block freed unless
// c->graphs holds it, capturing / cap_dev cleared.
static int capture_register(dsir_ctx* c, Call& call, const dsir_pair_batch* in, int n_iter, const dsir_pair_result* out,
                            const std::vector<unsigned char>& key, hipGraphExec_t* exec) {
  struct Capture {
    dsir_ctx* c;
    bool open = false;
    hipGraph_t graph = nullptr;
    void* walk_block = nullptr;
    ~Capture() {
      if (open) { hipGraph_t g = nullptr; hipStreamEndCapture(c->stream, &g); if (g) hipGraphDestroy(g); }
      if (graph) hipGraphDestroy(graph);
      if (walk_block) hipFree(walk_block);
      c->capturing = false;
      c->cap_dev = nullptr;
    }
  } cap{c};
  HIP_OK(c, hipStreamSynchronize(c->stream));
  // the walker programs of this registration get a device block of their own (the kernel nodes hold addresses inside it); they are
  // collected on the host while the launches are captured and uploaded once, below
  if (c->walk_mode && c->walk_dev) {
    HIP_OK(c, hipMalloc(&cap.walk_block, sizeof(WalkProgram) * dsir_ctx::kWalkSlots));
    c->cap_host.assign(sizeof(WalkProgram) * dsir_ctx::kWalkSlots, 0);
    c->cap_dev = reinterpret_cast<WalkProgram*>(cap.walk_block);
  }
  for (int64_t& v : c->graph_nodes) v = 0;     // a failed capture leaves no census
  HIP_OK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  cap.open = true;
  c->capturing = true;
  if (int r = register_enqueue(c, call, in, n_iter, out)) return r;
  c->capturing = false;
  cap.open = false;
  HIP_OK(c, hipStreamEndCapture(c->stream, &cap.graph));
  if (!cap.graph) return fail(c, "hipStreamEndCapture: no graph");
  if (cap.walk_block && c->call.walk_used > 0)
    HIP_OK(c, hipMemcpy(cap.walk_block, c->cap_host.data(), sizeof(WalkProgram) * (size_t)c->call.walk_used, hipMemcpyHostToDevice));
  {
    // what one registration costs in launches: the node census of the captured graph (dsir_graph_stats)
    size_t nn = 0;
    if (hipGraphGetNodes(cap.graph, nullptr, &nn) == hipSuccess && nn > 0) {
      std::vector<hipGraphNode_t> nodes(nn);
      if (hipGraphGetNodes(cap.graph, nodes.data(), &nn) == hipSuccess) {
        c->graph_nodes[0] = (int64_t)nn;
        for (size_t i = 0; i < nn; ++i) {
          hipGraphNodeType t;
          if (hipGraphNodeGetType(nodes[i], &t) != hipSuccess) continue;
          if (t == hipGraphNodeTypeKernel) ++c->graph_nodes[1];
          else if (t == hipGraphNodeTypeMemset) ++c->graph_nodes[2];
          else if (t == hipGraphNodeTypeMemcpy) ++c->graph_nodes[3];
        }
      }
    }
  }
  HIP_OK(c, hipGraphInstantiate(exec, cap.graph, nullptr, nullptr, 0));
  c->graphs.push_back({key, *exec, cap.walk_block});
  cap.walk_block = nullptr;                          // c->graphs owns it now
  if (c->graphs.size() > dsir_ctx::kMaxGraphs) {
    HIP_OK(c, hipStreamSynchronize(c->stream));     // the evicted graph may still be replaying
    hipGraphExecDestroy(c->graphs.front().exec);
    if (c->graphs.front().walk_block) hipFree(c->graphs.front().walk_block);
    c->graphs.erase(c->graphs.begin());
  }
  return 0;
}

int dsir_register(dsir_ctx* c, const dsir_pair_batch* in, int n_iter, const dsir_pair_result* out) {
  Call call(c, Call::kWeights); if (call.refused()) return 1;
  if (!in || !out || !out->transforms) return fail(c, "dsir_register: null argument");
  if (c->cfg.pipeline != DSIR_PIPELINE_ALIGN) return fail(c, "dsir_register needs an align-pipeline context");
  if (!c->use_graph || c->time_match) {
    if (int r = register_enqueue(c, call, in, n_iter, out)) return r;
    return call.finish();
  }
  // Graph mode: the whole launch sequence (~450 kernels) is captured once per distinct call
  // signature (sizes AND buffer addresses) and replayed with one hipGraphLaunch.
  std::vector<unsigned char> key(sizeof(*in) + sizeof(*out) + sizeof(int));
  std::memcpy(key.data(), in, sizeof(*in));
  std::memcpy(key.data() + sizeof(*in), out, sizeof(*out));
  std::memcpy(key.data() + sizeof(*in) + sizeof(*out), &n_iter, sizeof(int));
  hipGraphExec_t exec = nullptr;
  for (auto& g : c->graphs)
    if (g.key == key) { exec = g.exec; break; }
  if (!exec) {
    if (int r = capture_register(c, call, in, n_iter, out, key, &exec)) return r;
  }
  HIP_OK(c, hipGraphLaunch(exec, c->stream));
  return call.finish();
}

// One side of forward_pair's endpoints (model.py:637-666).
static int emit_cloud_out(dsir_ctx* c, const Pyramid& py, const float* feat0, const float* logits, const float* score,
                          const int32_t* label, int P, int n, int num_sub, const dsir_cloud_out* o) {
  const dsir_cfg& g = c->cfg;
  hipStream_t st = c->stream;
  Arena& ws = c->ws;
  const int M = num_sub > 0 ? num_sub : n;
  const int64_t xyz_cs = (int64_t)py.S * 3;
  if (o->logits) HIP_OK(c, hipMemcpyAsync(o->logits, logits, sizeof(float) * P * n * g.num_classes, hipMemcpyDeviceToDevice, st));
  if (g.pipeline == DSIR_PIPELINE_LABEL) {
    if (o->xyz) launch_copy_xyz(py.xyz, xyz_cs, 3, n, P, o->xyz, (int64_t)n * 3, st);
    if (o->feat) launch_l2norm64(feat0, (int64_t)P * n, o->feat, st);
    return 0;
  }
  const size_t mark = ws.mark();
  const int32_t* sel = nullptr;
  const float* xyz_m = py.xyz; int64_t xyz_m_cs = xyz_cs;
  const float* feat_m = feat0; const float* score_m = score;
  if (num_sub > 0) {
    int32_t* idx = ws.get<int32_t>((size_t)P * M);
    float* sc = ws.get<float>((size_t)P * M);
    float* xs = ws.get<float>((size_t)P * M * 3);
    float* fs = ws.get<float>((size_t)P * M * 64);
    void* scratch = ws.raw(topk_scratch_bytes(P, n));
    if (ws.overflow) return fail(c, "workspace exhausted in forward_pair");
    if (int r = launch_topk(score, P, n, M, idx, sc, scratch, st)) return fail(c, "top-k selection failed (%d)", r);
    launch_gather_rows(py.xyz, xyz_cs, 3, idx, 3, M, P, xs, st);
    launch_gather_rows(feat0, (int64_t)n * 64, 64, idx, 64, M, P, fs, st);
    sel = idx; xyz_m = xs; xyz_m_cs = (int64_t)M * 3; feat_m = fs; score_m = sc;
  }
  if (o->xyz) {
    if (sel) HIP_OK(c, hipMemcpyAsync(o->xyz, xyz_m, sizeof(float) * P * M * 3, hipMemcpyDeviceToDevice, st));
    else launch_copy_xyz(py.xyz, xyz_cs, 3, n, P, o->xyz, (int64_t)n * 3, st);
  }
  if (o->score) HIP_OK(c, hipMemcpyAsync(o->score, score_m, sizeof(float) * P * M, hipMemcpyDeviceToDevice, st));
  if (o->label) launch_gather_i32(label, n, sel, M, P, o->label, st);
  if (o->index && sel) HIP_OK(c, hipMemcpyAsync(o->index, sel, sizeof(int32_t) * P * M, hipMemcpyDeviceToDevice, st));
  if (o->feat) {
    if (g.pipeline == DSIR_PIPELINE_ALIGN) {
      HIP_OK(c, hipMemcpyAsync(o->feat, feat_m, sizeof(float) * P * M * 64, hipMemcpyDeviceToDevice, st));
    } else {
      // aggregation (already L2-normalised, model.py:232-233), then the second F.normalize of :650-651
      float* desc = ws.get<float>((size_t)P * M * 64);
      if (ws.overflow) return fail(c, "workspace exhausted in forward_pair");
      const size_t m2 = ws.mark();
      float* F = run_mlp_feat(c, feat_m, P, M);
      run_att_proj(c, xyz_m, xyz_m_cs, score_m, F, P, M, desc);
      ws.release(m2);
      launch_l2norm64(desc, (int64_t)P * M, o->feat, st);
    }
  }
  ws.release(mark);
  return 0;
}

int dsir_forward_pair(dsir_ctx* c, const dsir_pair_batch* in, int num_sub, const dsir_cloud_out* src, const dsir_cloud_out* ref) {
  Call call(c, Call::kWeights); if (call.refused()) return 1;
  if (!in || !src || !ref) return fail(c, "dsir_forward_pair: null argument");
  const dsir_cfg& g = c->cfg;
  if (num_sub > 0) {
    if (g.pipeline != DSIR_PIPELINE_FEAT) return fail(c, "num_sub > 0 is only meaningful for the feat pipeline");
    if (num_sub > in->n_src || num_sub > in->n_ref) return fail(c, "num_sub=%d exceeds the cloud size", num_sub);
  }
  const bool scored = g.pipeline != DSIR_PIPELINE_LABEL;
  PairStage S;
  if (int r = call.begin_walker()) return r;
  if (int r = forward_pair_stage(c, in, scored, scored, S)) return r;
  if (int r = emit_cloud_out(c, S.ps, S.feat_s, S.logit_s, S.score_s, S.label_s, in->pairs, in->n_src, num_sub, src)) return r;
  if (int r = emit_cloud_out(c, S.pr, S.feat_r, S.logit_r, S.score_r, S.label_r, in->pairs, in->n_ref, num_sub, ref)) return r;
  return call.finish();
}

}  // extern "C"
