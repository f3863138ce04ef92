// The C ABI of include/dsir.h and the registration loop (forward_align_4).  The context and what the host-side files share:
// engine_ctx.h; weights: weights.hip; layer schedules: schedule.hip; descriptor search: search.hip.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "engine_ctx.h"
#include "icp_grid.h"

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

// the workspace is sized from max_pairs and max_points: inside them no allocation of a call can overflow
int check_batch(dsir_ctx* c, const char* name, int clouds, int n) {
  if (clouds > 2 * c->cfg.max_pairs || n > c->cfg.max_points) return fail(c, "%s: batch exceeds max_pairs/max_points", name);
  return 0;
}

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
    // per pair: the inlier model's cached enc halves of the attention scores (EncCache::s2_buf), 2 x n_l x 16 x d_l floats
    size_t s2 = 0;
    int nl = cfg->max_points;
    for (int l = 0; l < cfg->num_layers; ++l) {
      if (cfg->d_out[l] >= 64) s2 += (size_t)2 * nl * kKnn * cfg->d_out[l] * sizeof(float) + 512;
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

int dsir_narrow_i64(dsir_ctx* c, const int64_t* src, int32_t* dst, int64_t n) {
  if (!c) return 1;
  HIP_OK(c, hipSetDevice(c->device));
  launch_narrow_i64(src, dst, n, c->stream);
  return post(c);
}

int dsir_knn_pyramid(dsir_ctx* c, const float* points, int stride, int clouds, int n, float* xyz, int32_t* neigh,
                     int32_t* sub, int32_t* interp) {
  if (!c) return 1;
  HIP_OK(c, hipSetDevice(c->device));
  if (clouds < 1 || stride < 3) return fail(c, "dsir_knn_pyramid: bad arguments");
  c->ws.top = 0; c->ws.overflow = false;
  if (int r = build_pyramid(c, points, stride, clouds, n, xyz, neigh, sub, interp)) return r;
  return post(c);
}

int dsir_randla_forward(dsir_ctx* c, int which, const float* features, int cin, int clouds, int n, const float* xyz,
                        const int32_t* neigh, const int32_t* sub, const int32_t* interp, float* feat, float* logits) {
  if (check_ready(c)) return 1;
  HIP_OK(c, hipSetDevice(c->device));
  if (which != 0 && c->cfg.pipeline != DSIR_PIPELINE_ALIGN) return fail(c, "randla_forward: this context has no inlier_model (pipeline != align)");
  const RandlaW& w = which == 0 ? c->net.feat : c->net.inl;
  if (w.ppf ? cin < 6 : cin != w.cin)
    return w.ppf ? fail(c, "randla_forward: use_ppf needs rows of xyz + normal, at least 6 columns, got %d (reference RandLANet.py:325)", cin)
                 : fail(c, "randla_forward: expected %d input channels, got %d", w.cin, cin);
  if (check_batch(c, "randla_forward", clouds, n)) return 1;
  Pyramid py;
  fill_pyramid_layout(c->cfg, clouds, n, py);
  if (py.nl[3] < kKnn) return fail(c, "cloud too small (n=%d)", n);
  py.xyz = xyz; py.neigh = neigh; py.sub = sub; py.interp = interp;
  // use_ppf: the row's first three columns are the point, the next three its normal (RandLANet.py:326)
  const Seg in0 = plain_seg(features, (int64_t)n * cin, w.ppf ? 3 : cin, cin);
  const Seg in1 = plain_seg(features + 3, (int64_t)n * cin, 3, cin);
  if (int r = walk_begin_call(c)) return r;
  if (int r = randla_forward(c, w, in0, w.ppf ? &in1 : nullptr, py, feat, logits)) return r;
  if (int r = walk_end_call(c)) return r;
  return post(c);
}

int dsir_ppf_pre(dsir_ctx* c, int which, const float* rows, int stride, const int32_t* neigh, int64_t neigh_cs, int clouds, int n,
                 float* out) {
  if (check_ready(c)) return 1;
  HIP_OK(c, hipSetDevice(c->device));
  if (!(c->flags & DSIR_FLAG_PPF)) return fail(c, "dsir_ppf_pre: the context was not created with DSIR_FLAG_PPF");
  if (which != 0 && c->cfg.pipeline != DSIR_PIPELINE_ALIGN) return fail(c, "dsir_ppf_pre: this context has no inlier_model (pipeline != align)");
  if (!rows || !neigh || !out || clouds < 1 || n < kKnn) return fail(c, "dsir_ppf_pre: bad arguments");
  if (stride < 6) return fail(c, "dsir_ppf_pre: rows of xyz + normal need at least 6 columns, got %d (reference RandLANet.py:325)", stride);
  if (check_batch(c, "dsir_ppf_pre", clouds, n)) return 1;
  if (int r = run_ppf_pre(c, which == 0 ? c->net.feat : c->net.inl, rows, stride, neigh, neigh_cs, clouds, n, out)) return r;
  return post(c);
}

int dsir_estimate_normals(dsir_ctx* c, const float* points, int stride, const int32_t* neigh, int64_t neigh_cs, int clouds, int n,
                          const float* viewpoint, float* normals, int32_t* flags) {
  if (!c) return 1;
  HIP_OK(c, hipSetDevice(c->device));
  if (!points || !neigh || !normals || clouds < 1 || clouds > 65535 || n < 1 || stride < 3) return fail(c, "dsir_estimate_normals: bad arguments");
  const float v[3] = {viewpoint ? viewpoint[0] : 0.f, viewpoint ? viewpoint[1] : 0.f, viewpoint ? viewpoint[2] : 0.f};
  launch_estimate_normals(points, (int64_t)n * stride, stride, neigh, neigh_cs, n, clouds, v[0], v[1], v[2], normals, flags, c->stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, "HIP launch error: %s", hipGetErrorString(e));
  return 0;
}

int dsir_estimate_normals_csr(dsir_ctx* c, const float* points, int stride, const int32_t* csr_offsets, const int32_t* csr_cols, int clouds,
                              int n, const float* viewpoint, float* normals, int32_t* flags) {
  if (!c) return 1;
  HIP_OK(c, hipSetDevice(c->device));
  if (!points || !csr_offsets || !csr_cols || !normals || clouds < 1 || clouds > 65535 || n < 1 || stride < 3)
    return fail(c, "dsir_estimate_normals_csr: bad arguments");
  const float v[3] = {viewpoint ? viewpoint[0] : 0.f, viewpoint ? viewpoint[1] : 0.f, viewpoint ? viewpoint[2] : 0.f};
  launch_estimate_normals_csr(points, (int64_t)n * stride, stride, csr_offsets, csr_cols, n, clouds, v[0], v[1], v[2], normals, flags, c->stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, "HIP launch error: %s", hipGetErrorString(e));
  return 0;
}

int dsir_fpfh(dsir_ctx* c, const float* points, int stride, const float* normals, const int32_t* neigh, int64_t neigh_cs,
              const int32_t* csr_offsets, const int32_t* csr_cols, int clouds, int n, float* desc, int out_ld, int32_t* flags) {
  if (!c) return 1;
  if (!points || !desc || clouds < 1 || clouds > 65535 || n < 1 || stride < 3 || out_ld < kFpfhDim) return fail(c, "dsir_fpfh: bad arguments");
  if (!normals && stride < 6) return fail(c, "dsir_fpfh: without normals the rows need xyz + normal, at least 6 columns, got %d", stride);
  const bool fixed = neigh != nullptr, csr = csr_offsets != nullptr || csr_cols != nullptr;
  if (fixed == csr) return fail(c, "dsir_fpfh: exactly one of neigh_idx and (csr_offsets, csr_cols) expected");
  if (csr && (!csr_offsets || !csr_cols)) return fail(c, "dsir_fpfh: a CSR list needs both csr_offsets and csr_cols");
  if ((int64_t)clouds * n > 0x7fffffffll / kFpfhRow) return fail(c, "dsir_fpfh: clouds x n = %lld rows beyond the int32 range of the SPFH table", (long long)clouds * n);
  HIP_OK(c, hipSetDevice(c->device));
  c->ws.top = 0; c->ws.overflow = false;
  FpfhArgs a;
  a.table = reinterpret_cast<int32_t*>(c->ws.raw(fpfh_scratch_bytes(clouds, n)));
  if (c->ws.overflow) return fail(c, "workspace too small for dsir_fpfh (clouds x n x 136 bytes: raise max_points / max_pairs)");
  a.pts = points; a.pts_cs = (int64_t)n * stride; a.pts_ld = stride;
  a.nrm = normals ? normals : points + 3; a.nrm_ld = normals ? 3 : stride; a.nrm_cs = (int64_t)n * a.nrm_ld;
  a.cols = fixed ? neigh : csr_cols; a.neigh_cs = neigh_cs; a.offsets = csr_offsets;
  a.desc = desc; a.out_ld = out_ld; a.flags = flags; a.n = n; a.clouds = clouds;
  if (!launch_fpfh(a, c->stream)) return fail(c, "dsir_fpfh: shape refused");
  return post(c);
}

int dsir_score(dsir_ctx* c, const float* feat, const float* logits, const float* xyz, int64_t xyz_cs,
               const int32_t* neigh, int64_t neigh_cs, int clouds, int n, float* score, int32_t* label) {
  if (check_ready(c)) return 1;
  HIP_OK(c, hipSetDevice(c->device));
  if (!feat || !logits || !xyz || !neigh || !score || clouds < 1 || n < 1) return fail(c, "dsir_score: bad arguments");
  if (check_batch(c, "dsir_score", clouds, n)) return 1;
  ScoreScratch s;
  s.red = c->ws.get<float>((size_t)clouds * 4);
  s.prob = c->ws.get<float>((size_t)clouds * n);
  s.label = c->ws.get<int32_t>((size_t)clouds * n);
  if (c->ws.overflow) return fail(c, "workspace exhausted in dsir_score");
  launch_score(feat, logits, c->cfg.num_classes, xyz, xyz_cs, neigh, neigh_cs, clouds, n, s, score, label, c->stream);
  return post(c);
}

int dsir_aggregate(dsir_ctx* c, const float* xyz, int64_t xyz_cs, const float* feat0, const float* score, int clouds,
                   int n, float* desc) {
  if (check_ready(c)) return 1;
  if (c->cfg.pipeline == DSIR_PIPELINE_LABEL) return fail(c, "dsir_aggregate: a label-pipeline context has no aggregation layers");
  HIP_OK(c, hipSetDevice(c->device));
  if (!xyz || !feat0 || !score || !desc || clouds < 1 || n < 1) return fail(c, "dsir_aggregate: bad arguments");
  if (check_batch(c, "dsir_aggregate", clouds, n)) return 1;
  float* F = run_mlp_feat(c, feat0, clouds, n);
  run_att_proj(c, xyz, xyz_cs, score, F, clouds, n, desc);
  return post(c);
}

int dsir_kabsch(dsir_ctx* c, const float* src, const float* tgt, const float* w, int pairs, int m, float* T,
                int32_t* invalid) {
  if (!c) return 1;
  if (!src || !tgt || !w || !T || pairs < 1 || m < 1) return fail(c, "dsir_kabsch: bad arguments");
  HIP_OK(c, hipSetDevice(c->device));
  if (invalid) HIP_OK(c, hipMemsetAsync(invalid, 0, sizeof(int32_t) * pairs, c->stream));
  KabschArgs a{};
  a.src = src; a.ref = tgt; a.idx = nullptr; a.w = w; a.src_stride = (int64_t)m * 3; a.ref_stride = (int64_t)m * 3;
  a.sigmoid = 0; a.pairs = pairs; a.m = m; a.T = T; a.invalid = invalid;
  a.chunk_min = c->kabsch_chunked_min;
  if (const size_t pb = kabsch_part_bytes(pairs, m, c->kabsch_chunked_min)) {      // large clouds: the chunked reduction of dsir_register (kabsch.hip)
    c->ws.top = 0; c->ws.overflow = false;
    a.part = c->ws.get<double>(pb / sizeof(double));
    if (c->ws.overflow) return fail(c, "dsir_kabsch: workspace exhausted");
  }
  launch_kabsch(a, c->stream);
  return post(c);
}

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
  if (ws.overflow) return fail(c, "workspace exhausted (raise max_points / max_pairs)");
  float* rxyz = pxyz + (size_t)P * ps.S * 3;
  int32_t* rneigh = pneigh + (size_t)P * ps.S * kKnn;
  int32_t* rsub = psub + (size_t)P * ps.S1 * kKnn;
  int32_t* rinterp = pinterp + (size_t)P * ps.S;
  // the score stage's reduction targets (max feature, label weight, probability per cloud) live from here on: preset to -inf below
  float* score_red = want_score ? ws.get<float>((size_t)2 * P * 4) : nullptr;
  if (ws.overflow) return fail(c, "workspace exhausted (raise max_points / max_pairs)");
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

static int register_enqueue(dsir_ctx* c, const dsir_pair_batch* in, int n_iter, const dsir_pair_result* out) {
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
  if (int r = walk_begin_call(c)) return r;
  struct StatsGuard { dsir_ctx* c; ~StatsGuard() { c->stats_prezeroed = false; c->stats_base = 0; } } stats_guard{c};
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
      c->stats_prezeroed = true;
      c->stats_base = 0;
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
  if (ws.overflow) return fail(c, "workspace exhausted (raise max_points / max_pairs)");
  const size_t mark1 = ws.mark();
  {
    run_mlp_feat(c, feat_s, P, J, F_s);       // straight into the storage that outlives the iterations
    launch_copy_xyz(pxyz, (int64_t)ps.S * 3, 3, J, P, xyz_cur, (int64_t)J * 3, st);      // xyz_cur = level-0 src coordinates
    float* F_r = run_mlp_feat(c, feat_r, P, K);
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
  if (c->ws.overflow) return overflow_fail(c, "workspace exhausted (raise max_points / max_pairs in dsir_cfg)");
  if (int r = walk_end_call(c)) return r;
  return 0;
}

// Graph mode: capture one registration, instantiate it and keep it in c->graphs (the oldest evicted beyond kMaxGraphs).  Every exit
// leaves the context clean (Capture's destructor): the capture ended, the graph destroyed, the walker programs' block freed unless
// c->graphs holds it, capturing / cap_dev cleared.
static int capture_register(dsir_ctx* c, const dsir_pair_batch* in, int n_iter, const dsir_pair_result* out,
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
  if (int r = register_enqueue(c, in, n_iter, out)) return r;
  c->capturing = false;
  cap.open = false;
  HIP_OK(c, hipStreamEndCapture(c->stream, &cap.graph));
  if (!cap.graph) return fail(c, "hipStreamEndCapture: no graph");
  if (cap.walk_block && c->walk_used > 0)
    HIP_OK(c, hipMemcpy(cap.walk_block, c->cap_host.data(), sizeof(WalkProgram) * (size_t)c->walk_used, hipMemcpyHostToDevice));
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
  if (check_ready(c)) return 1;
  if (!in || !out || !out->transforms) return fail(c, "dsir_register: null argument");
  if (c->cfg.pipeline != DSIR_PIPELINE_ALIGN) return fail(c, "dsir_register needs an align-pipeline context");
  HIP_OK(c, hipSetDevice(c->device));
  if (!c->use_graph || c->time_match) {
    if (int r = register_enqueue(c, in, n_iter, out)) return r;
    return post(c);
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
    if (int r = capture_register(c, in, n_iter, out, key, &exec)) return r;
  }
  HIP_OK(c, hipGraphLaunch(exec, c->stream));
  return post(c);
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
  if (check_ready(c)) return 1;
  if (!in || !src || !ref) return fail(c, "dsir_forward_pair: null argument");
  HIP_OK(c, hipSetDevice(c->device));
  const dsir_cfg& g = c->cfg;
  if (num_sub > 0) {
    if (g.pipeline != DSIR_PIPELINE_FEAT) return fail(c, "num_sub > 0 is only meaningful for the feat pipeline");
    if (num_sub > in->n_src || num_sub > in->n_ref) return fail(c, "num_sub=%d exceeds the cloud size", num_sub);
  }
  const bool scored = g.pipeline != DSIR_PIPELINE_LABEL;
  PairStage S;
  if (int r = walk_begin_call(c)) return r;
  if (int r = forward_pair_stage(c, in, scored, scored, S)) return r;
  if (int r = walk_end_call(c)) return r;
  if (int r = emit_cloud_out(c, S.ps, S.feat_s, S.logit_s, S.score_s, S.label_s, in->pairs, in->n_src, num_sub, src)) return r;
  if (int r = emit_cloud_out(c, S.pr, S.feat_r, S.logit_r, S.score_r, S.label_r, in->pairs, in->n_ref, num_sub, ref)) return r;
  return post(c);
}

// search 1 -> the grid without its query order under the measurement switch DSIR_ICP_GRID_NO_ORDER: same bytes, other speed
static IcpSearch icp_search_mode(int search) {
  if (search != 1) return IcpSearch::Brute;
  return tuning_flag("DSIR_ICP_GRID_NO_ORDER") ? IcpSearch::GridUnordered : IcpSearch::Grid;
}

struct IcpCorrOut { int32_t* idx; float* d2; double* stats; };

// What the four ICP entries share: the checks under the entry's own `name`, the workspace reset, the scratch, the normals
// (normals_ref [pairs][K][3], or columns 3..5 of the points_ref rows) and the launch; corr != nullptr: one search step, not the loop.
static int icp_entry(dsir_ctx* c, const char* name, IcpArgs a, const float* normals_ref, int search, const IcpCorrOut* corr) {
  if (!c) return 1;
  const bool outs = corr ? corr->idx && corr->d2 : a.T_out != nullptr;
  if (!a.src || !a.ref || !a.T_init || !outs || a.pairs < 1 || a.J < 1 || a.K < 1 || a.stride < 3 || a.max_iter < 0 ||
      !(a.max_corr_dist > 0.f) || (a.estimator != 0 && a.estimator != 1) || (search != 0 && search != 1))
    return fail(c, "%s: bad arguments", name);
  if (a.estimator == 1 && !normals_ref && a.stride < 6)
    return fail(c, "%s: bad arguments (the plane estimator without normals_ref reads the normals from columns 3..5 "
                   "of the points_ref rows: stride=%d, needs >= 6)", name, a.stride);
  if (search == 1 && (!icp_grid_radius_ok(a.max_corr_dist) || !icp_grid_shape_ok(a.pairs, a.J, a.K)))
    return fail(c, "%s: bad arguments (the grid search needs a max_corr_dist whose fp32 square is finite, and pairs x J "
                   "and pairs x K below 2^31)", name);
  a.search = icp_search_mode(search);
  a.normals = normals_ref ? normals_ref : a.ref + 3;
  a.normals_cs = normals_ref ? (int64_t)a.K * 3 : (int64_t)a.K * a.stride;
  a.normals_ld = normals_ref ? 3 : a.stride;
  HIP_OK(c, hipSetDevice(c->device));
  c->ws.top = 0; c->ws.overflow = false;
  void* scratch = c->ws.raw(corr ? icp_corr_scratch_bytes(a) : icp_scratch_bytes(a));
  if (c->ws.overflow) return fail(c, "workspace too small for %s (raise max_points / max_pairs)", name);
  if (const int e = corr ? launch_icp_correspondences(a, corr->idx, corr->d2, corr->stats, scratch, c->stream)
                         : launch_icp_refine(a, scratch, c->stream))
    return fail(c, "%s: the index build failed (HIP error %d)", name, e);
  return post(c);
}

static IcpArgs icp_args(const float* points_src, const float* points_ref, int pairs, int J, int K, int stride, float max_corr_dist,
                        int max_iter, float rel_fitness, float rel_rmse, const float* T_init, float* T_out, int estimator) {
  IcpArgs a{};
  a.src = points_src; a.ref = points_ref; a.pairs = pairs; a.J = J; a.K = K; a.stride = stride; a.max_corr_dist = max_corr_dist;
  a.max_iter = max_iter; a.rel_fitness = rel_fitness; a.rel_rmse = rel_rmse; a.T_init = T_init; a.T_out = T_out; a.estimator = estimator;
  return a;
}

int dsir_icp_refine(dsir_ctx* c, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                    float max_corr_dist, int max_iter, float rel_fitness, float rel_rmse, const float* T_init,
                    float* T_out, double* stats) {
  IcpArgs a = icp_args(points_src, points_ref, pairs, J, K, stride, max_corr_dist, max_iter, rel_fitness, rel_rmse, T_init, T_out, 0);
  a.stats_out = stats;                                            // [pairs][4]
  return icp_entry(c, "dsir_icp_refine", a, nullptr, 0, nullptr);
}

int dsir_icp_refine_ex(dsir_ctx* c, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                       float max_corr_dist, int max_iter, float rel_fitness, float rel_rmse, const float* T_init, float* T_out,
                       int estimator, const float* normals_ref, double* stats) {
  IcpArgs a = icp_args(points_src, points_ref, pairs, J, K, stride, max_corr_dist, max_iter, rel_fitness, rel_rmse, T_init, T_out, estimator);
  a.stats5_out = stats;                                           // [pairs][5]
  return icp_entry(c, "dsir_icp_refine_ex", a, normals_ref, 0, nullptr);
}

int dsir_icp_refine_ex2(dsir_ctx* c, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                        float max_corr_dist, int max_iter, float rel_fitness, float rel_rmse, const float* T_init, float* T_out,
                        int estimator, const float* normals_ref, int search, double* stats) {
  IcpArgs a = icp_args(points_src, points_ref, pairs, J, K, stride, max_corr_dist, max_iter, rel_fitness, rel_rmse, T_init, T_out, estimator);
  a.stats5_out = stats;
  return icp_entry(c, "dsir_icp_refine_ex2", a, normals_ref, search, nullptr);
}

int dsir_icp_correspondences(dsir_ctx* c, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                             float max_corr_dist, const float* T, int search, int32_t* idx_out, float* d2_out, double* stats_out) {
  const IcpArgs a = icp_args(points_src, points_ref, pairs, J, K, stride, max_corr_dist, 0, 0.f, 0.f, T, nullptr, 0);
  const IcpCorrOut out{idx_out, d2_out, stats_out};
  return icp_entry(c, "dsir_icp_correspondences", a, nullptr, search, &out);
}

int dsir_ransac_correspondence(dsir_ctx* c, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                               const int32_t* corr, const int32_t* counts, int M, float max_dist, int ransac_n, float edge_sim,
                               int hypotheses, int refine_iters, uint64_t seed, const float* T_init, float* T_out, double* stats,
                               int32_t* invalid, const dsir_ransac_diag* diag) {
  if (!c) return 1;
  if (!points_src || !points_ref || !corr || !T_out || !stats || !invalid || pairs < 1 || J < 1 || K < 1 || M < 1 || stride < 3 ||
      !(max_dist > 0.f) || !std::isfinite(max_dist) || !std::isfinite(edge_sim))
    return fail(c, "dsir_ransac_correspondence: bad arguments");
  if (ransac_n != 3 && ransac_n != 4) return fail(c, "dsir_ransac_correspondence: ransac_n must be 3 or 4 (got %d)", ransac_n);
  if (hypotheses < 1 || hypotheses > DSIR_RANSAC_MAX_HYPOTHESES)
    return fail(c, "dsir_ransac_correspondence: hypotheses=%d outside [1,%d]", hypotheses, DSIR_RANSAC_MAX_HYPOTHESES);
  if (refine_iters < 0 || refine_iters > DSIR_RANSAC_MAX_REFINE)
    return fail(c, "dsir_ransac_correspondence: refine_iters=%d outside [0,%d]", refine_iters, DSIR_RANSAC_MAX_REFINE);
  if (M > c->cfg.max_points || J > c->cfg.max_points || K > c->cfg.max_points)
    return fail(c, "dsir_ransac_correspondence: M=%d, J=%d or K=%d beyond max_points=%d", M, J, K, c->cfg.max_points);
  HIP_OK(c, hipSetDevice(c->device));
  c->ws.top = 0; c->ws.overflow = false;
  void* scratch = c->ws.raw(ransac_scratch_bytes(pairs, M, hypotheses, refine_iters));
  if (c->ws.overflow) return fail(c, "workspace too small for dsir_ransac_correspondence (pairs x (M x 28 + hypotheses x 56) bytes: raise max_points / max_pairs)");
  RansacArgs a{};
  a.src = points_src; a.ref = points_ref; a.pairs = pairs; a.J = J; a.K = K; a.stride = stride; a.corr = corr; a.counts = counts;
  a.M = M; a.max_dist = max_dist; a.n = ransac_n; a.edge_sim = edge_sim; a.hypotheses = hypotheses; a.refine_iters = refine_iters;
  a.seed = seed; a.T_init = T_init; a.T_out = T_out; a.stats = stats; a.invalid = invalid;
  if (diag) { a.diag_sample = diag->hyp_sample; a.diag_T = diag->hyp_T; a.diag_valid = diag->hyp_valid; a.diag_count = diag->hyp_count; }
  launch_ransac(a, scratch, c->stream);
  return post(c);
}

int dsir_consensus_correspondence(dsir_ctx* c, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                                  const int32_t* corr, const int32_t* counts, int M, float max_dist, float compat_dist, int seeds,
                                  int members, int refine_iters, const float* T_init, float* T_out, double* stats, int32_t* invalid,
                                  const dsir_consensus_diag* diag) {
  if (!c) return 1;
  if (!points_src || !points_ref || !corr || !T_out || !stats || !invalid || pairs < 1 || J < 1 || K < 1 || M < 1 || stride < 3 ||
      !(max_dist > 0.f) || !std::isfinite(max_dist) || !std::isfinite(compat_dist))
    return fail(c, "dsir_consensus_correspondence: bad arguments");
  if (seeds < 1 || seeds > DSIR_CONSENSUS_MAX_SEEDS)
    return fail(c, "dsir_consensus_correspondence: seeds=%d outside [1,%d]", seeds, DSIR_CONSENSUS_MAX_SEEDS);
  if (members < 3 || members > DSIR_CONSENSUS_MAX_MEMBERS)
    return fail(c, "dsir_consensus_correspondence: members=%d outside [3,%d]", members, DSIR_CONSENSUS_MAX_MEMBERS);
  if (refine_iters < 0 || refine_iters > DSIR_RANSAC_MAX_REFINE)
    return fail(c, "dsir_consensus_correspondence: refine_iters=%d outside [0,%d]", refine_iters, DSIR_RANSAC_MAX_REFINE);
  if (M > c->cfg.max_points || J > c->cfg.max_points || K > c->cfg.max_points)
    return fail(c, "dsir_consensus_correspondence: M=%d, J=%d or K=%d beyond max_points=%d", M, J, K, c->cfg.max_points);
  if (M > DSIR_CONSENSUS_MAX_M) return fail(c, "dsir_consensus_correspondence: M=%d beyond DSIR_CONSENSUS_MAX_M=%d", M, DSIR_CONSENSUS_MAX_M);
  if ((int64_t)pairs * M > 0x7fffffffll) return fail(c, "dsir_consensus_correspondence: pairs x M = %lld unsupported", (long long)pairs * M);
  HIP_OK(c, hipSetDevice(c->device));
  // the whole workspace, validated before the first launch
  const size_t need = consensus_scratch_bytes(pairs, M, seeds, refine_iters);
  if (need > c->ws.cap)
    return fail(c, "workspace too small for dsir_consensus_correspondence: needs %zu bytes (the bit matrix alone: pairs x M x ceil(M / 64) x 8 = "
                   "%zu), the arena holds %zu (raise max_points / max_pairs, or pass fewer pairs)", need,
                (size_t)pairs * M * ((size_t)(M + 63) / 64) * 8, c->ws.cap);
  c->ws.top = 0; c->ws.overflow = false;
  void* scratch = c->ws.raw(need);
  if (c->ws.overflow) return fail(c, "workspace too small for dsir_consensus_correspondence");
  ConsensusArgs a{};
  a.src = points_src; a.ref = points_ref; a.pairs = pairs; a.J = J; a.K = K; a.stride = stride; a.corr = corr; a.counts = counts;
  a.M = M; a.max_dist = max_dist; a.compat_dist = compat_dist; a.seeds = seeds; a.members = members; a.refine_iters = refine_iters;
  a.T_init = T_init; a.T_out = T_out; a.stats = stats; a.invalid = invalid;
  if (diag) {
    a.diag_bits = diag->bits; a.diag_score = diag->score; a.diag_seed = diag->seed; a.diag_members = diag->seed_members;
    a.diag_T = diag->seed_T; a.diag_valid = diag->seed_valid; a.diag_count = diag->seed_count;
  }
  if (int r = launch_consensus(a, scratch, c->stream)) return fail(c, "dsir_consensus_correspondence: launch failed (%d)", r);
  return post(c);
}

int dsir_pose_finetune(dsir_ctx* c, const float* xyz_src, const float* xyz_ref, const float* weights, int weights_are_logits,
                       int pairs, int m, const float* T_init, float quantization_size, int max_iter, float break_threshold_ratio,
                       int max_break_count, float* T_out, double* stats) {
  if (!c) return 1;
  if (!xyz_src || !xyz_ref || !T_init || !T_out || pairs < 1 || m < 1 || max_iter < 0 || max_break_count < 1 ||
      !(quantization_size > 0.f) || !(break_threshold_ratio >= 0.f))
    return fail(c, "dsir_pose_finetune: bad arguments");
  HIP_OK(c, hipSetDevice(c->device));
  launch_pose_finetune(xyz_src, xyz_ref, weights, weights_are_logits ? 1 : 0, pairs, m, T_init, quantization_size, max_iter,
                       break_threshold_ratio, max_break_count, T_out, stats, c->stream);
  return post(c);
}

// One body behind the three entries: the kernel always writes three columns (point distance, confidence, pose error); the
// two older entries run it with weight 0 and hand their callers the first two.
static int align_loss_body(dsir_ctx* c, const float* pt_src, const float* pt_ref, const int32_t* idx, const float* logits,
                           const float* labels, const float* transform_gt, int pairs, int J, int K, int n_iter, int loss_type,
                           float wt_ptDist_loss, float wt_inlier_loss, float loss_discount_factor, float wt_pose_loss, float* transforms,
                           double* losses, float* grad_logits, double* losses_per_pair, int cols) {
  if (!c) return 1;
  if (!pt_src || !pt_ref || !idx || !logits || !transform_gt || !grad_logits || pairs < 1 || J < 1 || K < 1 || n_iter < 1 ||
      n_iter > 8 || (loss_type != 0 && loss_type != 1))
    return fail(c, "dsir_align_loss_backward: bad arguments (n_iter in [1,8], loss_type 0 = mae / 1 = mse)");
  if (!(wt_pose_loss >= 0.f) || !std::isfinite(wt_pose_loss))
    return fail(c, "dsir_align_loss_backward3: wt_pose_loss must be finite and >= 0");
  HIP_OK(c, hipSetDevice(c->device));
  c->ws.top = 0; c->ws.overflow = false;
  // correspondences come from the caller: clamped into [0, K) before any gather
  int32_t* idx_ok = c->ws.get<int32_t>((size_t)n_iter * pairs * J);
  double* dloss = c->ws.get<double>((size_t)3 * n_iter);
  double* dpart = c->ws.get<double>((size_t)3 * n_iter * pairs);       // every pair's loss terms, added in pair order (align_loss.hip)
  if (c->ws.overflow) return fail(c, "workspace too small for dsir_align_loss_backward");
  launch_copy_idx_clamped(idx, (int64_t)pairs * J, pairs * J, K, n_iter, idx_ok, (int64_t)pairs * J, nullptr, 1, c->stream);
  if (launch_align_loss(pt_src, pt_ref, idx_ok, logits, labels, transform_gt, pairs, J, K, n_iter, loss_type, wt_ptDist_loss,
                        wt_inlier_loss, loss_discount_factor, wt_pose_loss, transforms, dloss, grad_logits, c->stream, dpart))
    return fail(c, "dsir_align_loss_backward: launch failed");
  if (losses || losses_per_pair) {
    HIP_OK(c, hipStreamSynchronize(c->stream));
    const size_t rows = (size_t)n_iter * pairs;
    std::vector<double> h(3 * rows);
    if (losses) {
      HIP_OK(c, hipMemcpy(h.data(), dloss, sizeof(double) * 3 * n_iter, hipMemcpyDeviceToHost));
      for (int i = 0; i < n_iter; ++i)
        for (int k = 0; k < cols; ++k) losses[(size_t)i * cols + k] = h[(size_t)i * 3 + k];
    }
    if (losses_per_pair) {
      // the kernel's per-pair partials carry the batch mean's 1 / pairs: a pair's own mean is pairs x its share
      HIP_OK(c, hipMemcpy(h.data(), dpart, sizeof(double) * 3 * rows, hipMemcpyDeviceToHost));
      for (size_t r = 0; r < rows; ++r)
        for (int k = 0; k < cols; ++k) losses_per_pair[r * cols + k] = h[r * 3 + k] * (double)pairs;
    }
  }
  return post(c);
}

int dsir_align_loss_backward3(dsir_ctx* c, const float* pt_src, const float* pt_ref, const int32_t* idx, const float* logits,
                              const float* labels, const float* transform_gt, int pairs, int J, int K, int n_iter, int loss_type,
                              float wt_ptDist_loss, float wt_inlier_loss, float loss_discount_factor, float wt_pose_loss,
                              float* transforms, double* losses, float* grad_logits, double* losses_per_pair) {
  return align_loss_body(c, pt_src, pt_ref, idx, logits, labels, transform_gt, pairs, J, K, n_iter, loss_type, wt_ptDist_loss,
                         wt_inlier_loss, loss_discount_factor, wt_pose_loss, transforms, losses, grad_logits, losses_per_pair, 3);
}

int dsir_align_loss_backward2(dsir_ctx* c, const float* pt_src, const float* pt_ref, const int32_t* idx, const float* logits,
                              const float* labels, const float* transform_gt, int pairs, int J, int K, int n_iter, int loss_type,
                              float wt_ptDist_loss, float wt_inlier_loss, float loss_discount_factor, float* transforms,
                              double* losses, float* grad_logits, double* losses_per_pair) {
  return align_loss_body(c, pt_src, pt_ref, idx, logits, labels, transform_gt, pairs, J, K, n_iter, loss_type, wt_ptDist_loss,
                         wt_inlier_loss, loss_discount_factor, 0.f, transforms, losses, grad_logits, losses_per_pair, 2);
}

int dsir_align_loss_backward(dsir_ctx* c, const float* pt_src, const float* pt_ref, const int32_t* idx, const float* logits,
                             const float* labels, const float* transform_gt, int pairs, int J, int K, int n_iter, int loss_type,
                             float wt_ptDist_loss, float wt_inlier_loss, float loss_discount_factor, float* transforms,
                             double* losses, float* grad_logits) {
  return align_loss_body(c, pt_src, pt_ref, idx, logits, labels, transform_gt, pairs, J, K, n_iter, loss_type, wt_ptDist_loss,
                         wt_inlier_loss, loss_discount_factor, 0.f, transforms, losses, grad_logits, nullptr, 2);
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

int dsir_voxel_downsample(dsir_ctx* c, const float* points, const int64_t* offsets, int clouds, int stride, float voxel_size,
                          const float* crop, int cap, float* out, int32_t* counts) {
  if (!c) return 1;
  if (!points || !offsets || !out || !counts || stride < 3 || stride > 16 || cap < 1 || !(voxel_size > 0.f))
    return fail(c, "dsir_voxel_downsample: bad arguments");
  if (clouds < 1 || clouds > 1000) return fail(c, "dsir_voxel_downsample: %d clouds in one call (1 to 1000 supported)", clouds);
  HIP_OK(c, hipSetDevice(c->device));
  const int64_t total = offsets[clouds];
  if (total <= 0 || total > 0x7fffffffll) return fail(c, "dsir_voxel_downsample: %lld points unsupported", (long long)total);
  c->ws.top = 0; c->ws.overflow = false;
  void* scratch = c->ws.raw(voxel_downsample_scratch_bytes(total, clouds));
  if (c->ws.overflow) return fail(c, "workspace too small for %lld raw points (raise max_points / max_pairs)", (long long)total);
  // the host offsets are consumed by an async copy: make the call self-contained
  HIP_OK(c, hipStreamSynchronize(c->stream));
  const int32_t* bad_dev = nullptr;
  if (int r = launch_voxel_downsample(points, offsets, clouds, stride, voxel_size, crop, cap, out, counts, scratch, c->stream,
                                      &bad_dev))
    return fail(c, "dsir_voxel_downsample: launch failed (%d)", r);
  HIP_OK(c, hipStreamSynchronize(c->stream));
  int32_t bad = kVoxelNoBadRow;
  HIP_OK(c, hipMemcpy(&bad, bad_dev, sizeof(bad), hipMemcpyDeviceToHost));
  if (bad != kVoxelNoBadRow) {                       // never dropped, never aliased into a neighbouring key field
    int cloud = 0;
    while (cloud + 1 < clouds && offsets[cloud + 1] <= bad) ++cloud;
    return fail(c, "dsir_voxel_downsample: cloud %d row %lld survives the crop with a voxel index outside [0, 2^18) or a "
                   "coordinate that is not finite (counts / out are unspecified)", cloud, (long long)(bad - offsets[cloud]));
  }
  return post(c);
}

int dsir_resample(dsir_ctx* c, const float* in, const int32_t* counts, int clouds, int cap, int stride, int k, int mode,
                  uint64_t seed, float* out) {
  if (!c) return 1;
  if (!in || !counts || !out || clouds < 1 || cap < 1 || stride < 1 || k < 1 || (mode != 0 && mode != 1))
    return fail(c, "dsir_resample: bad arguments");
  HIP_OK(c, hipSetDevice(c->device));
  c->ws.top = 0; c->ws.overflow = false;
  void* scratch = c->ws.raw(resample_scratch_bytes(clouds, cap));
  if (c->ws.overflow) return fail(c, "workspace too small for dsir_resample");
  if (int r = launch_resample(in, counts, clouds, cap, stride, k, mode, seed, out, scratch, c->stream))
    return fail(c, "dsir_resample: launch failed (%d)", r);
  return post(c);
}

int dsir_eval_metrics(dsir_ctx* c, const float* pred_T, int64_t pred_stride, const float* gt_T, const float* points_src,
                      const float* points_ref, int pairs, int n, int stride, float rte_thresh, float rre_thresh,
                      double* out) {
  if (!c) return 1;
  if (!pred_T || !gt_T || !points_src || !points_ref || !out || pairs < 1 || n < 1 || stride < 3 || pred_stride < 12)
    return fail(c, "dsir_eval_metrics: bad arguments");
  HIP_OK(c, hipSetDevice(c->device));
  launch_eval_metrics(pred_T, pred_stride, gt_T, points_src, points_ref, pairs, n, stride, rte_thresh, rre_thresh, out,
                      c->stream);
  return post(c);
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
