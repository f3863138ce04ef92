// The context of include/dsir.h: the tuning gate, fail(), create / destroy and the limits, stream and sync, weight names, the
// switches, graph on / off and its statistics, the walker's trace.  The other host-side files and what they share: engine_ctx.h.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "engine_ctx.h"

using namespace dsir;

// ------------------------------------------------------------------ the tuning gate
// The ONLY place of the library that reads the environment.  Every DSIR_* measurement / A-B switch goes through
// tuning_env(); unless the gate is open - DSIR_TUNING=1 in the environment, or dsir_set_tuning(1) before the first call
// that reads a switch (most are read once into function-static state) - the library ignores every DSIR_* variable, so a
// stray one in a user's environment cannot change kernel selection.
static int g_tuning = -1;     // -1: not decided yet, 0: closed, 1: open
const char* dsir::tuning_env(const char* name) {
  if (g_tuning < 0) {
    const char* e = getenv("DSIR_TUNING");
    g_tuning = (e && e[0] == '1' && e[1] == 0) ? 1 : 0;
  }
  return g_tuning == 1 ? getenv(name) : nullptr;
}

namespace {
thread_local std::string g_create_error;
}  // namespace

int dsir::fail(dsir_ctx* c, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else g_create_error = buf;
  return 1;
}

namespace {

// an A/B switch of the context: a captured registration has the choice baked in, so the graphs go
template <typename F> int set_switch(dsir_ctx* c, F set) {
  if (!c) return 1;
  set();
  c->drop_graphs();
  return 0;
}

}  // namespace

// =================================================================== C ABI
extern "C" {

int dsir_create(int device, const dsir_cfg* cfg, dsir_ctx** out) { return dsir_create_ex(device, cfg, 0, out); }

int dsir_create_ex(int device, const dsir_cfg* cfg, int flags, dsir_ctx** out) {
  if (!cfg || !out) return fail(nullptr, "dsir_create: null argument");
  if (flags & ~DSIR_FLAG_PPF) return fail(nullptr, "dsir_create_ex: unknown flags 0x%x", flags);
  const bool ppf = (flags & DSIR_FLAG_PPF) != 0;
  if (cfg->num_knn != kKnn) return fail(nullptr, "num_knn must be %d (got %d)", kKnn, cfg->num_knn);
  if (cfg->num_layers != 4) return fail(nullptr, "num_layers must be 4 (got %d)", cfg->num_layers);
  if (cfg->out_feat_dim != 64) return fail(nullptr, "out_feat_dim must be 64 (got %d)", cfg->out_feat_dim);
  if (cfg->num_classes < 1 || cfg->num_classes > 32) return fail(nullptr, "num_classes out of range");
  for (int l = 0; l < 4; ++l) {
    if (cfg->d_out[l] % 16 || cfg->d_out[l] < 16 || cfg->d_out[l] > 256) return fail(nullptr, "d_out[%d]=%d unsupported", l, cfg->d_out[l]);
    if (cfg->sub_sampling_ratio[l] < 1) return fail(nullptr, "bad sub_sampling_ratio");
  }
  if (cfg->feat_len < 3 || cfg->feat_len > 16) return fail(nullptr, "feat_len must be in [3,16]");
  // use_ppf: a point row is xyz + normal (+ more); the reference asserts it in RandLA.forward (RandLANet.py:325)
  if (ppf && cfg->feat_len < 6)
    return fail(nullptr, "use_ppf: feat_len=%d, but a point row needs xyz and a normal, at least 6 columns (reference RandLANet.py:325: \"feature dimension error\")", cfg->feat_len);
  if (cfg->max_points < kKnn * 64 || cfg->max_pairs < 1) return fail(nullptr, "max_points must be >= %d and max_pairs >= 1", kKnn * 64);
  // several kernels address a cloud's rows with 32-bit byte offsets from a per-cloud base (n * 16 * d * 4 < 2^32 at d = 64: knn_grid.hip,
  // att_pool.hip, lse_uv.hip check their own products); 2^20 points per cloud is far beyond what the 2.5 kB-per-point workspace admits
  if (cfg->max_points > (1 << 20)) return fail(nullptr, "max_points must be <= %d", 1 << 20);
  // the GroupNorm statistics' atomics are exact - order independent - for at most kGnMaxContrib contributions per statistic
  // (device_utils.h); the largest layer of a cloud of max_points points must stay within that
  if (const int gc = gn_max_contributions(*cfg, cfg->max_points, flags); gc > kGnMaxContrib)
    return fail(nullptr, "max_points=%d: %d workgroup contributions per GroupNorm statistic exceed the exactness bound %d of the statistics' atomics (max_points <= %d)",
                cfg->max_points, gc, kGnMaxContrib, dsir_max_points_limit_ex(cfg, flags));
  if (cfg->pipeline < DSIR_PIPELINE_ALIGN || cfg->pipeline > DSIR_PIPELINE_LABEL) return fail(nullptr, "unknown pipeline %d", cfg->pipeline);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, "no HIP device available");
  if (device < 0 || device >= ndev) return fail(nullptr, "device %d out of range (%d devices)", device, ndev);
  dsir_ctx* c = new dsir_ctx();
  c->device = device; c->cfg = *cfg; c->flags = flags;
  c->screen_mode = tuning_flag("DSIR_NO_SCREEN") ? 0 : 1;
  if (const char* e = tuning_env("DSIR_PRUNE_MIN_K")) c->prune_min_points = atoi(e) > 0 ? atoi(e) : 0;   // A/B hook; 0 = off
  if (const char* e = tuning_env("DSIR_PRUNE_MIN_ROWS")) c->prune_min_rows = atoll(e) > 0 ? atoll(e) : 0;   // tuning hook
  c->agg_split = tuning_flag("DSIR_AGG_F32") ? 0 : 1;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return fail(nullptr, "cannot initialise device %d", device);
  }
  c->own_stream = c->stream;
  expect_state_dict(c);
  // workspace: ~1.4k floats per point per cloud for one RandLA pass, 2P clouds, plus per-pair state
  const size_t clouds = (size_t)2 * cfg->max_pairs;
  const size_t per_cloud = (size_t)cfg->max_points * 2560 * sizeof(float) + ((size_t)1 << 22);
  c->ws.cap = clouds * per_cloud + ((size_t)64 << 20);
  if (cfg->pipeline == DSIR_PIPELINE_ALIGN) {
    // per pair: the inlier model's cached enc halves of the attention scores (EncCache::s2_buf), 2 x n_l x 16 x d_l floats for
    // the levels that keep them
    size_t s2 = 0;
    int nl = cfg->max_points;
    for (int l = 0; l < cfg->num_layers; ++l) {
      if (att_keeps_score_cache(cfg->d_out[l])) s2 += (size_t)2 * nl * kKnn * cfg->d_out[l] * sizeof(float) + 512;
      nl /= cfg->sub_sampling_ratio[l];
    }
    c->ws.cap += (size_t)cfg->max_pairs * s2;
  }
  if (hipMalloc((void**)&c->ws.base, c->ws.cap) != hipSuccess) {
    const size_t cap = c->ws.cap;
    hipStreamDestroy(c->stream);
    delete c;
    return fail(nullptr, "cannot allocate %zu MiB of workspace", cap >> 20);
  }
  c->stats_cap = gn_register_words(cfg->max_pairs, 10);   // one registration's passes side by side: (2 + n_iter) P clouds for n_iter <= 10
  if (hipMalloc((void**)&c->stats, c->stats_cap * sizeof(double)) != hipSuccess) {
    hipFree(c->ws.base); hipStreamDestroy(c->stream);
    delete c;
    return fail(nullptr, "cannot allocate the statistics arena");
  }
  {
    // deep-level walker: device programs + two pinned staging sets + the tile queues / completion counters of one call's programs
    const size_t pb = sizeof(WalkProgram) * dsir_ctx::kWalkSlots;
    const size_t cb = sizeof(unsigned) * dsir_ctx::kWalkSlots * dsir_ctx::kWalkClouds * kWalkCtrWords;
    bool ok = hipMalloc((void**)&c->walk_dev, pb) == hipSuccess && hipMalloc((void**)&c->walk_ctr, cb) == hipSuccess &&
              hipMemset(c->walk_ctr, 0, cb) == hipSuccess;
    for (int k = 0; k < 2 && ok; ++k)
      ok = hipHostMalloc((void**)&c->walk_host[k], pb, hipHostMallocDefault) == hipSuccess &&
           hipEventCreateWithFlags(&c->walk_ev[k], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
      for (int k = 0; k < 2; ++k) { if (c->walk_host[k]) hipHostFree(c->walk_host[k]); if (c->walk_ev[k]) hipEventDestroy(c->walk_ev[k]); }
      if (c->walk_dev) hipFree(c->walk_dev);
      if (c->walk_ctr) hipFree(c->walk_ctr);
      hipFree(c->stats); hipFree(c->ws.base); hipStreamDestroy(c->stream);
      delete c;
      return fail(nullptr, "cannot allocate the walker's program buffers");
    }
    c->walk_mode = tuning_flag("DSIR_WALK") ? 1 : 0;
    c->walk_wpc = (int)tuning_int("DSIR_WALK_WPC", 0);
    c->walk_flags = (int)tuning_int("DSIR_WALK_FLAGS", 0);
    if (tuning_flag("DSIR_WALK_TRACE")) {
      const size_t tb = sizeof(unsigned long long) * dsir_ctx::kWalkSlots * kWalkMaxPhases * 4;
      if (hipMalloc((void**)&c->walk_trace, tb) != hipSuccess) c->walk_trace = nullptr;
    }
  }
  if (hipMalloc((void**)&c->screen_acc, 6 * sizeof(unsigned long long)) != hipSuccess ||
      hipMemset(c->screen_acc, 0, 6 * sizeof(unsigned long long)) != hipSuccess) {
    hipFree(c->stats); hipFree(c->ws.base); hipStreamDestroy(c->stream);
    delete c;
    return fail(nullptr, "cannot allocate the screening counters");
  }
  *out = c;
  return 0;
}

void dsir_destroy(dsir_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  for (auto& e : c->match_events) { hipEventDestroy(e.op0); hipEventDestroy(e.op1); hipEventDestroy(e.k0); hipEventDestroy(e.k1); }
  c->drop_graphs();
  if (c->dweights) hipFree(c->dweights);
  if (c->dweights16) hipFree(c->dweights16);
  if (c->match_ts) hipFree(c->match_ts);
  if (c->screen_acc) hipFree(c->screen_acc);
  for (int k = 0; k < 2; ++k) { if (c->walk_host[k]) hipHostFree(c->walk_host[k]); if (c->walk_ev[k]) hipEventDestroy(c->walk_ev[k]); }
  if (c->walk_dev) hipFree(c->walk_dev);
  if (c->walk_ctr) hipFree(c->walk_ctr);
  if (c->walk_trace) hipFree(c->walk_trace);
  if (c->stats) hipFree(c->stats);
  if (c->ws.base) hipFree(c->ws.base);
  hipStreamDestroy(c->own_stream);     // a caller's stream (dsir_set_stream) is the caller's to destroy
  delete c;
}

int dsir_gn_contributions_ex(const dsir_cfg* cfg, int flags, int n_points) {
  if (!cfg || cfg->num_layers != 4 || n_points < 1 || (flags & ~DSIR_FLAG_PPF)) return -1;
  for (int l = 0; l < 4; ++l) if (cfg->sub_sampling_ratio[l] < 1) return -1;
  return gn_max_contributions(*cfg, n_points, flags);
}
int dsir_gn_contributions(const dsir_cfg* cfg, int n_points) { return dsir_gn_contributions_ex(cfg, 0, n_points); }
int dsir_gn_contribution_limit(void) { return kGnMaxContrib; }
int dsir_max_points_limit_ex(const dsir_cfg* cfg, int flags) {
  if (dsir_gn_contributions_ex(cfg, flags, 1024) < 0) return -1;
  int lo = 1024, hi = 1 << 20;                       // the count grows with n: bisect the largest n within the bound
  if (gn_max_contributions(*cfg, hi, flags) <= kGnMaxContrib) return hi;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (gn_max_contributions(*cfg, mid, flags) <= kGnMaxContrib) lo = mid; else hi = mid;
  }
  return lo;
}
int dsir_max_points_limit(const dsir_cfg* cfg) { return dsir_max_points_limit_ex(cfg, 0); }

void dsir_set_tuning(int on) { g_tuning = on ? 1 : 0; }
int dsir_tuning(void) { tuning_env("DSIR_TUNING"); return g_tuning == 1; }

const char* dsir_last_error(const dsir_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }
void* dsir_stream(dsir_ctx* c) { return c ? (void*)c->stream : nullptr; }
int dsir_set_stream(dsir_ctx* c, void* stream, int restore_own) {
  if (!c) return 1;
  HIP_OK(c, hipSetDevice(c->device));
  hipStream_t next = restore_own ? c->own_stream : (hipStream_t)stream;     // NULL is a valid caller stream: the legacy default stream
  if (next == c->stream) return 0;
  // Every call of a context re-uses its ONE workspace arena from the start: launches on the new stream must not overtake work
  // still running on the old one.  The new stream therefore waits (on the device, no host synchronisation) for everything
  // enqueued on the old stream so far.  Exception: a stream under capture cannot wait on outside work - whoever captures
  // synchronises before the capture begins (torch.cuda.graph does).
  hipStreamCaptureStatus cap_new = hipStreamCaptureStatusNone, cap_old = hipStreamCaptureStatusNone;
  hipStreamIsCapturing(next, &cap_new);
  hipStreamIsCapturing(c->stream, &cap_old);
  if (cap_new == hipStreamCaptureStatusNone && cap_old == hipStreamCaptureStatusNone) {
    hipEvent_t ev = nullptr;
    HIP_OK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, c->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(next, ev, 0);
    hipEventDestroy(ev);
    if (e != hipSuccess) return fail(c, "dsir_set_stream: ordering the new stream after the old one failed: %s", hipGetErrorString(e));
  }
  // a captured registration belongs to the old stream
  c->drop_graphs();
  c->stream = next;
  return 0;
}
int dsir_sync(dsir_ctx* c) {
  if (!c) return 1;
  HIP_OK(c, hipStreamSynchronize(c->stream));
  return 0;
}
int dsir_num_weights(const dsir_ctx* c) { return c ? (int)c->params.size() : 0; }
const char* dsir_weight_name(const dsir_ctx* c, int i, int64_t* numel) {
  if (!c || i < 0 || i >= (int)c->params.size()) return nullptr;
  if (numel) *numel = c->params[i].ignored ? 1 : c->params[i].numel();
  return c->params[i].name.c_str();
}

int dsir_graph_stats(dsir_ctx* c, int64_t* out) {
  if (!c || !out) return 1;
  for (int i = 0; i < 4; ++i) out[i] = c->graph_nodes[i];
  return 0;
}

int dsir_enable_graph(dsir_ctx* c, int enable) {
  if (!c) return 1;
  c->use_graph = enable != 0;
  if (!c->use_graph) c->drop_graphs();
  return 0;
}

void dsir_split_f16(const float* x, int64_t n, uint16_t* hi, uint16_t* lo) {
  if (x && hi && lo && n > 0) split_weights_f16(x, (size_t)n, hi, lo);
}

int dsir_enable_agg_split(dsir_ctx* c, int enable) { return set_switch(c, [&] { c->agg_split = enable != 0; }); }

int dsir_set_prune_thresholds(dsir_ctx* c, int min_points, int64_t min_rows) {
  return set_switch(c, [&] { c->prune_min_points = min_points > 0 ? min_points : 0; c->prune_min_rows = min_rows > 0 ? min_rows : 0; });
}

int dsir_set_kabsch_chunked_min(dsir_ctx* c, int min_points) { return set_switch(c, [&] { c->kabsch_chunked_min = min_points > 0 ? min_points : 0; }); }

int dsir_walk_trace(dsir_ctx* c, int reset, int64_t* out, int64_t* clock_khz) {
  if (!c) return 1;
  HIP_OK(c, hipSetDevice(c->device));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  const size_t n = (size_t)dsir_ctx::kWalkSlots * kWalkMaxPhases * 4;
  if (!c->walk_trace) return fail(c, "dsir_walk_trace: tracing is off (DSIR_TUNING=1 DSIR_WALK_TRACE=1 before dsir_create)");
  if (out) HIP_OK(c, hipMemcpy(out, c->walk_trace, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  if (reset) {
    std::vector<unsigned long long> init(n);
    for (size_t i = 0; i < n; ++i) init[i] = (i & 3) < 2 ? ~0ull : 0ull;      // two minima, two maxima
    HIP_OK(c, hipMemcpy(c->walk_trace, init.data(), n * sizeof(unsigned long long), hipMemcpyHostToDevice));
  }
  if (clock_khz) {
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess || khz <= 0) khz = 100000;
    *clock_khz = khz;
  }
  return 0;
}

int dsir_enable_walk(dsir_ctx* c, int enable) { return set_switch(c, [&] { c->walk_mode = enable != 0; }); }

int dsir_enable_screen(dsir_ctx* c, int enable) { return set_switch(c, [&] { c->screen_mode = enable != 0; }); }

}  // extern "C"
