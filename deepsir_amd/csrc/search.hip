// The descriptor search on the host side (DescSearch, engine_ctx.h): the one place that allocates the search's operands, prepares
// them and launches nn_match.hip / nn_screen.hip / nn_prune.hip.  A registration and the stand-alone entry points differ in
// arguments only; which mode a registration takes is search_plan.h's decision.
#include <vector>

#include "engine_ctx.h"

namespace dsir {

namespace {

dsir_ctx::MatchEvents* match_event_slot(dsir_ctx* c) {
  if (!c->time_match) return nullptr;
  if (c->match_events_used == c->match_events.size()) {
    dsir_ctx::MatchEvents e{};
    hipEventCreate(&e.op0); hipEventCreate(&e.op1); hipEventCreate(&e.k0); hipEventCreate(&e.k1);
    c->match_events.push_back(e);
  }
  return &c->match_events[c->match_events_used++];
}

unsigned long long* match_ts_slot(dsir_ctx* c) {
  if (!c->time_match || !c->match_ts || c->match_ts_used >= kMatchSlots) return nullptr;
  return c->match_ts + 2 * c->match_ts_used++;
}

}  // namespace

void DescSearch::alloc(bool with_match_scratch, bool with_stats, bool with_bad) {
  Arena& ws = c->ws;
  if (with_match_scratch) match_scratch = ws.raw(nn_match_scratch_bytes(P, J, K));
  if (search_screens(mode)) {
    const SearchOperandBytes b = search_operand_bytes(mode, P, J, K);
    ah = ws.raw(b.a_half); al = ws.raw(b.a_half);
    bh = ws.raw(b.b_half); bl = ws.raw(b.b_half);
    sa = reinterpret_cast<float*>(ws.raw(b.sa)); sb = reinterpret_cast<float*>(ws.raw(b.sb));
    scratch = ws.raw(nn_screen_scratch_bytes(P, J));
    ex_ref.sq = sb; ex_ref.hi = bh; ex_ref.lo = bl;
    ex_src.sq = sa; ex_src.hi = ah; ex_src.lo = al;
  } else if (mode == SearchMode::exhaustive && match_scratch) {
    // exhaustive search: the epilogue leaves the norms and the preset result slots
    nn_match_scratch_layout(match_scratch, P, J, K, &ex_src.sq, &ex_src.packed_init);
  }
  if (mode == SearchMode::pruned) prune_scratch = ws.raw(nn_prune_scratch_bytes(P, J, K));
  if (with_stats) stats = ws.get<unsigned long long>(2);
  if (with_bad) bad = ws.get<int32_t>(1);   // raised by the split when an element is outside the screening's domain
}

int DescSearch::split_pair(const float* a, const float* b) {
  hipStream_t st = c->stream;
  HIP_OK(c, hipMemsetAsync(bad, 0, 4, st));
  launch_split16_norm(a, (int64_t)P * J, ah, al, sa, st, bad);
  launch_split16_norm(b, (int64_t)P * K, bh, bl, sb, st, bad);
  return 0;
}

int DescSearch::prepare_ref(const float* desc_r, bool prepared, const float* rxyz, int64_t rxyz_cs) {
  hipStream_t st = c->stream;
  if (search_screens(mode) && !prepared) launch_split16_norm(desc_r, (int64_t)P * K, bh, bl, sb, st);
  if (mode == SearchMode::pruned && launch_prune_ref(rxyz, rxyz_cs, desc_r, bh, bl, sb, P, J, K, prune_scratch, st))
    return fail(c, "pruned search: sorting the ref side failed");
  return 0;
}

int DescSearch::run(const float* desc_s, const float* desc_r, int32_t* idx_out, const Iter& i) {
  hipStream_t st = c->stream;
  if (mode == SearchMode::forced) {
    // caller-supplied correspondences: clamped into [0, K), out-of-range entries reported through the pair's flag
    launch_copy_idx_clamped(i.forced, J, J, K, P, idx_out, J, i.invalid, P, st);
    return 0;
  }
  // HIP events on the engine's stream: op0..op1 around every kernel of the operation (split, screening, pick,
  // fallback / norms, search, unpack), k0..k1 around its dominant kernel alone
  dsir_ctx::MatchEvents* ev = timed ? match_event_slot(c) : nullptr;
  if (ev) hipEventRecord(ev->op0, st);
  if (search_screens(mode)) {
    if (!i.src_prepared) launch_split16_norm(desc_s, (int64_t)P * J, ah, al, sa, st);
    ScreenOrder ord;
    // an actual distance of every row - to its previous match, to the columns of its nearest tile - bounds its minimum from
    // above: skip the tiles that cannot beat it (iteration 0 has only the second kind)
    if (mode == SearchMode::pruned &&
        launch_prune_rows(desc_s, desc_r, ah, al, sa, sb, i.it == 0 ? nullptr : prev_idx, P, J, K, prune_scratch, st, &ord, c->screen_acc + 4))
      return fail(c, "pruned search: sorting the rows failed");
    launch_nn_screen(desc_s, desc_r, ah, al, bh, bl, sa, sb, P, J, K, idx_out, scratch, st, nullptr, nullptr, i.want_stats ? stats : nullptr,
                     /*keep_gate=*/i.it > 0, i.domain_gate ? bad : nullptr, counted ? c->screen_acc : nullptr, ev ? ev->k0 : nullptr,
                     ev ? ev->k1 : nullptr, ord);
  } else {
    if (counted) ++c->exhaustive_searches;
    launch_nn_match_ws(desc_s, desc_r, P, J, K, idx_out, match_scratch, st, ev ? ev->k0 : nullptr, ev ? ev->k1 : nullptr,
                       /*ref_norms_cached=*/i.it > 0, counted ? match_ts_slot(c) : nullptr, /*src_norms_ready=*/i.src_prepared);
  }
  if (ev) hipEventRecord(ev->op1, st);
  prev_idx = idx_out;
  return 0;
}

}  // namespace dsir

using namespace dsir;

// =================================================================== C ABI: the stand-alone searches, their timers and totals
extern "C" {

int dsir_nn_match(dsir_ctx* c, const float* a, const float* b, int pairs, int J, int K, int32_t* idx) {
  Call call(c); if (call.refused()) return 1;
  if (!a || !b || !idx || pairs < 1 || J < 1 || K < 1) return fail(c, "dsir_nn_match: bad arguments");
  DescSearch s{c, SearchMode::exhaustive, pairs, J, K, /*timed=*/true};
  s.alloc(/*with_match_scratch=*/true);
  if (c->ws.overflow) return fail(c, "workspace exhausted in nn_match");
  if (int r = s.run(a, b, idx, {})) return r;
  return call.finish();
}

int dsir_nn_match_screened(dsir_ctx* c, const float* a, const float* b, int pairs, int J, int K, int32_t* idx,
                           int64_t* stats) {
  Call call(c); if (call.refused()) return 1;
  if (!a || !b || !idx || pairs < 1 || J < 1 || K < 1) return fail(c, "dsir_nn_match_screened: bad arguments");
  DescSearch s{c, SearchMode::screened, pairs, J, K};
  s.alloc(/*with_match_scratch=*/false, /*with_stats=*/true, /*with_bad=*/true);
  if (c->ws.overflow) return fail(c, "workspace exhausted in nn_match_screened");
  if (int r = s.split_pair(a, b)) return r;
  DescSearch::Iter one;
  one.src_prepared = true; one.domain_gate = true; one.want_stats = stats != nullptr;
  if (int r = s.run(a, b, idx, one)) return r;
  if (stats) {
    HIP_OK(c, hipStreamSynchronize(c->stream));
    unsigned long long h[2];
    HIP_OK(c, hipMemcpy(h, s.stats, 16, hipMemcpyDeviceToHost));
    stats[0] = (int64_t)h[0]; stats[1] = (int64_t)h[1];
  }
  return call.finish();
}

int dsir_screen_bounds(dsir_ctx* c, const float* a, const float* b, int J, int K, float* lower, float* upper, float* exact,
                       float* zacc, int32_t* idx, float* thresh, int32_t* cand_count, int32_t* cand_code, float* cand_lower,
                       int32_t* out_of_domain) {
  Call call(c); if (call.refused()) return 1;
  if (!a || !b || !lower || !upper || !exact || !idx || !thresh || !cand_count || !cand_code || !cand_lower || J < 1 || K < 1 ||
      (int64_t)J * K > ((int64_t)1 << 26))
    return fail(c, "dsir_screen_bounds: bad arguments (J x K <= 2^26)");
  DescSearch s{c, SearchMode::screened, 1, J, K};
  s.alloc(/*with_match_scratch=*/false, /*with_stats=*/false, /*with_bad=*/true);
  if (c->ws.overflow) return fail(c, "workspace exhausted in dsir_screen_bounds");
  hipStream_t st = c->stream;
  if (int r = s.split_pair(a, b)) return r;
  launch_screen_bounds(a, b, s.ah, s.al, s.bh, s.bl, s.sa, s.sb, J, K, lower, upper, exact, zacc, st);
  // the product path on the same operands (no domain gate: the screening runs even outside its domain, so that the flag
  // and the bound can be looked at independently), then its candidate lists
  DescSearch::Iter one;
  one.src_prepared = true;
  if (int r = s.run(a, b, idx, one)) return r;
  launch_screen_export(s.scratch, J, thresh, cand_count, cand_code, cand_lower, st);
  if (out_of_domain) HIP_OK(c, hipMemcpyAsync(out_of_domain, s.bad, 4, hipMemcpyDeviceToDevice, st));
  return call.finish();
}
int dsir_screen_cap(void) { return nn_screen_cap(); }

int dsir_feature_correspondences(dsir_ctx* c, const float* desc_src, const float* desc_ref, int pairs, int J, int K, int mutual,
                                 int32_t* corr, int32_t* counts) {
  Call call(c); if (call.refused()) return 1;
  if (!desc_src || !desc_ref || !corr || !counts || pairs < 1 || J < 1 || K < 1)
    return fail(c, "dsir_feature_correspondences: bad arguments");
  if (J > c->cfg.max_points || K > c->cfg.max_points)
    return fail(c, "dsir_feature_correspondences: J=%d or K=%d beyond max_points=%d", J, K, c->cfg.max_points);
  int32_t* ab = c->ws.get<int32_t>((size_t)pairs * J);
  int32_t* ba = c->ws.get<int32_t>((size_t)pairs * K);
  DescSearch s_ab{c, SearchMode::exhaustive, pairs, J, K}, s_ba{c, SearchMode::exhaustive, pairs, K, J};
  s_ab.alloc(/*with_match_scratch=*/true);
  s_ba.alloc(/*with_match_scratch=*/true);
  if (c->ws.overflow) return fail(c, "workspace too small for dsir_feature_correspondences (raise max_points / max_pairs)");
  s_ab.run(desc_src, desc_ref, ab, {});
  if (mutual) s_ba.run(desc_ref, desc_src, ba, {});
  launch_corr_compact(ab, ba, pairs, J, K, mutual ? 1 : 0, corr, counts, c->stream);
  return call.finish();
}

static int match_ts_reset(dsir_ctx* c) {
  std::vector<unsigned long long> init(2 * kMatchSlots);
  for (size_t i = 0; i < kMatchSlots; ++i) { init[2 * i] = ~0ull; init[2 * i + 1] = 0ull; }
  HIP_OK(c, hipMemcpy(c->match_ts, init.data(), init.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
  c->match_ts_used = 0;
  return 0;
}
int dsir_enable_match_timer(dsir_ctx* c, int enable) {
  if (!c) return 1;
  HIP_OK(c, hipSetDevice(c->device));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  c->time_match = enable != 0;
  if (c->time_match) {
    if (!c->match_ts) HIP_OK(c, hipMalloc((void**)&c->match_ts, 2 * kMatchSlots * sizeof(unsigned long long)));
    if (int r = match_ts_reset(c)) return r;
  }
  return 0;
}
int dsir_match_timer_device(dsir_ctx* c, int reset, double* total_ms, int64_t* launches) {
  if (!c) return 1;
  HIP_OK(c, hipSetDevice(c->device));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  if (c->match_ts && c->match_ts_used) {
    std::vector<unsigned long long> h(2 * c->match_ts_used);
    HIP_OK(c, hipMemcpy(h.data(), c->match_ts, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess || khz <= 0) khz = 100000;
    for (size_t i = 0; i < c->match_ts_used; ++i)
      if (h[2 * i] != ~0ull && h[2 * i + 1] > h[2 * i]) {
        c->match_dev_ms += (double)(h[2 * i + 1] - h[2 * i]) / (double)khz;
        ++c->match_dev_launches;
      }
    if (int r = match_ts_reset(c)) return r;
  }
  if (total_ms) *total_ms = c->match_dev_ms;
  if (launches) *launches = c->match_dev_launches;
  if (reset) { c->match_dev_ms = 0.0; c->match_dev_launches = 0; }
  return 0;
}

int dsir_prune_stats(dsir_ctx* c, int reset, int64_t* out) {
  if (!c || !out) return 1;
  HIP_OK(c, hipSetDevice(c->device));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  unsigned long long h[2];
  HIP_OK(c, hipMemcpy(h, c->screen_acc + 4, sizeof h, hipMemcpyDeviceToHost));
  out[0] = (int64_t)h[0]; out[1] = (int64_t)h[1];
  if (reset) HIP_OK(c, hipMemset(c->screen_acc + 4, 0, sizeof h));
  return 0;
}

int dsir_screen_stats(dsir_ctx* c, int reset, int64_t* out) {
  if (!c || !out) return 1;
  HIP_OK(c, hipSetDevice(c->device));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  unsigned long long h[4];
  HIP_OK(c, hipMemcpy(h, c->screen_acc, sizeof h, hipMemcpyDeviceToHost));
  for (int i = 0; i < 4; ++i) out[i] = (int64_t)h[i];
  out[4] = c->exhaustive_searches;
  if (reset) {
    HIP_OK(c, hipMemset(c->screen_acc, 0, sizeof h));
    c->exhaustive_searches = 0;
  }
  return 0;
}

static int collect_match_events(dsir_ctx* c) {
  HIP_OK(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < c->match_events_used; ++i) {
    float ms = 0.f, kms = 0.f;
    const auto& e = c->match_events[i];
    if (hipEventElapsedTime(&ms, e.op0, e.op1) == hipSuccess && hipEventElapsedTime(&kms, e.k0, e.k1) == hipSuccess) {
      c->match_ms += ms; c->match_kernel_ms += kms; ++c->match_launches;
    }
  }
  c->match_events_used = 0;
  return 0;
}

int dsir_match_timer2(dsir_ctx* c, int reset, double* op_ms, double* kernel_ms, int64_t* launches) {
  if (!c) return 1;
  if (int r = collect_match_events(c)) return r;
  if (op_ms) *op_ms = c->match_ms;
  if (kernel_ms) *kernel_ms = c->match_kernel_ms;
  if (launches) *launches = c->match_launches;
  if (reset) { c->match_ms = 0.0; c->match_kernel_ms = 0.0; c->match_launches = 0; }
  return 0;
}
int dsir_match_timer(dsir_ctx* c, int reset, double* total_ms, int64_t* launches) { return dsir_match_timer2(c, reset, total_ms, nullptr, launches); }

}  // extern "C"

// =================================================================== top-k search (nn_topk.hip) and the correspondences built on it
namespace dsir {

int DescSearch::run_topk(const float* desc_s, const float* desc_r, int k, int32_t* idx_out, float* dist_out) {
  if (mode != SearchMode::exhaustive || !topk_scratch) return fail(c, "top-k search: exhaustive mode with alloc_topk() only");
  launch_nn_topk(desc_s, desc_r, P, J, K, k, idx_out, dist_out, topk_scratch, c->stream);
  return 0;
}

namespace {

inline size_t arena_pad(size_t b) { return (b + 255) & ~(size_t)255; }

// J, K and k of a top-k call against the context's limits
int topk_check_shape(dsir_ctx* c, const char* who, int pairs, int J, int K, int k) {
  if (pairs < 1 || J < 1 || K < 1) return fail(c, "%s: bad arguments", who);
  if (k < 1 || k > DSIR_TOPK_MAX) return fail(c, "%s: k=%d outside [1, %d]", who, k, DSIR_TOPK_MAX);
  if (J > c->cfg.max_points || K > c->cfg.max_points)
    return fail(c, "%s: J=%d or K=%d beyond max_points=%d", who, J, K, c->cfg.max_points);
  if ((int64_t)pairs * J * k > 0x7fffffffll || (int64_t)pairs * K * k > 0x7fffffffll)
    return fail(c, "%s: pairs x points x k beyond 2^31", who);
  return 0;
}

}  // namespace
}  // namespace dsir

extern "C" {

int dsir_nn_match_topk(dsir_ctx* c, const float* a, const float* b, int pairs, int J, int K, int k, int32_t* idx, float* dist) {
  Call call(c); if (call.refused()) return 1;
  if (!a || !b || !idx) return fail(c, "dsir_nn_match_topk: bad arguments");
  if (int r = topk_check_shape(c, "dsir_nn_match_topk", pairs, J, K, k)) return r;
  DescSearch s{c, SearchMode::exhaustive, pairs, J, K};
  // the whole scratch, checked before the first launch
  const size_t need = arena_pad(s.topk_bytes(k));
  if (need > c->ws.cap)
    return fail(c, "workspace too small for dsir_nn_match_topk: needs %zu bytes, the arena holds %zu (raise max_points / max_pairs, or pass "
                   "fewer pairs)", need, c->ws.cap);
  s.alloc_topk(k);
  if (c->ws.overflow) return fail(c, "workspace exhausted in dsir_nn_match_topk");
  if (int r = s.run_topk(a, b, k, idx, dist)) return r;
  return call.finish();
}

int dsir_nn_match_topk_splits(dsir_ctx* c, int pairs, int J, int K, int k) {
  if (!c || pairs < 1 || J < 1 || K < 1 || k < 1 || k > DSIR_TOPK_MAX) return -1;
  return nn_topk_splits(pairs, J, K, k);
}

int dsir_feature_correspondences_ex(dsir_ctx* c, const float* desc_src, const float* desc_ref, int pairs, int J, int K, int mutual,
                                    int k, float ratio, int32_t* corr, int32_t* counts, float* corr_dist) {
  Call call(c); if (call.refused()) return 1;
  if (!desc_src || !desc_ref || !corr || !counts) return fail(c, "dsir_feature_correspondences_ex: bad arguments");
  if (int r = topk_check_shape(c, "dsir_feature_correspondences_ex", pairs, J, K, k)) return r;
  if ((int64_t)J * k > c->cfg.max_points)
    return fail(c, "dsir_feature_correspondences_ex: J x k = %lld beyond max_points=%d (the pose stages take M <= max_points)",
                (long long)J * k, c->cfg.max_points);
  if (ratio != ratio || ratio - ratio != 0.f || ratio >= 1.f)
    return fail(c, "dsir_feature_correspondences_ex: ratio=%g must be finite and below 1 (<= 0: no test)", (double)ratio);
  if (ratio > 0.f && k > 1)
    return fail(c, "dsir_feature_correspondences_ex: the ratio test is defined on the 1-NN set (ratio=%g with k=%d)", (double)ratio, k);
  // today's rule on today's launches
  if (k == 1 && !(ratio > 0.f) && !corr_dist) return dsir_feature_correspondences(c, desc_src, desc_ref, pairs, J, K, mutual, corr, counts);
  const int ks = ratio > 0.f ? 2 : k;                 // ranks searched src -> ref: the ratio test reads rank 1
  const float r2 = ratio > 0.f ? ratio * ratio : 0.f;   // fp32, rounded once
  DescSearch s_ab{c, SearchMode::exhaustive, pairs, J, K}, s_ba{c, SearchMode::exhaustive, pairs, K, J};
  const size_t n_ab = (size_t)pairs * J * ks, n_ba = mutual ? (size_t)pairs * K * k : 0;
  const size_t need = 2 * arena_pad(n_ab * 4) + arena_pad(n_ba * 4) + arena_pad(s_ab.topk_bytes(ks)) + (mutual ? arena_pad(s_ba.topk_bytes(k)) : 0);
  if (need > c->ws.cap)
    return fail(c, "workspace too small for dsir_feature_correspondences_ex: needs %zu bytes, the arena holds %zu (raise max_points / "
                   "max_pairs, or pass fewer pairs)", need, c->ws.cap);
  int32_t* iab = c->ws.get<int32_t>(n_ab);
  float* dab = c->ws.get<float>(n_ab);
  int32_t* iba = mutual ? c->ws.get<int32_t>(n_ba) : nullptr;
  s_ab.alloc_topk(ks);
  if (mutual) s_ba.alloc_topk(k);
  if (c->ws.overflow) return fail(c, "workspace exhausted in dsir_feature_correspondences_ex");
  if (int r = s_ab.run_topk(desc_src, desc_ref, ks, iab, dab)) return r;
  if (mutual) if (int r = s_ba.run_topk(desc_ref, desc_src, k, iba, nullptr)) return r;
  launch_corr_topk_compact(iab, dab, ks, iba, k, pairs, J, K, mutual ? 1 : 0, k, r2, corr, counts, corr_dist, c->stream);
  return call.finish();
}

}  // extern "C"
