// The pose entries of include/dsir.h: weighted Kabsch, ICP, RANSAC, spatial consensus and FGR from correspondences, the pose
// fine-tune, the alignment loss with its backward, and the evaluation metrics.
#include <cmath>

#include "engine_ctx.h"
#include "fgr.h"
#include "icp_grid.h"
#include "icp_robust.h"
#include "pose_corr.h"

using namespace dsir;

extern "C" {

int dsir_kabsch(dsir_ctx* c, const float* src, const float* tgt, const float* w, int pairs, int m, float* T,
                int32_t* invalid) {
  Call call(c); if (call.refused()) return 1;
  if (!src || !tgt || !w || !T || pairs < 1 || m < 1) return fail(c, "dsir_kabsch: bad arguments");
  if (invalid) HIP_OK(c, hipMemsetAsync(invalid, 0, sizeof(int32_t) * pairs, c->stream));
  KabschArgs a{};
  a.src = src; a.ref = tgt; a.idx = nullptr; a.w = w; a.src_stride = (int64_t)m * 3; a.ref_stride = (int64_t)m * 3;
  a.sigmoid = 0; a.pairs = pairs; a.m = m; a.T = T; a.invalid = invalid;
  a.chunk_min = c->kabsch_chunked_min;
  if (const size_t pb = kabsch_part_bytes(pairs, m, c->kabsch_chunked_min)) {      // large clouds: the chunked reduction of dsir_register (kabsch.hip)
    a.part = c->ws.get<double>(pb / sizeof(double));
    if (c->ws.overflow) return fail(c, "dsir_kabsch: workspace exhausted");
  }
  launch_kabsch(a, c->stream);
  return call.finish();
}

// search 1 -> the grid without its query order under the measurement switch DSIR_ICP_GRID_NO_ORDER: same bytes, other speed
static IcpSearch icp_search_mode(int search) {
  if (search != 1) return IcpSearch::Brute;
  return tuning_flag("DSIR_ICP_GRID_NO_ORDER") ? IcpSearch::GridUnordered : IcpSearch::Grid;
}

struct IcpCorrOut { int32_t* idx; float* d2; double* stats; };

// What the ICP entries share (a.counts_src / a.counts_ref set by the _ex3 / _ex entries, nullptr by the others: clamped, not refused): the checks under the entry's own `name`, the workspace reset, the scratch, the normals
// (normals_ref [pairs][K][3], or columns 3..5 of the points_ref rows) and the launch; corr != nullptr: one search step, not the loop.
static int icp_entry(dsir_ctx* c, const char* name, IcpArgs a, const float* normals_ref, int search, const IcpCorrOut* corr) {
  Call call(c); if (call.refused()) return 1;
  const bool outs = corr ? corr->idx && corr->d2 : a.T_out != nullptr;
  if (!a.src || !a.ref || !a.T_init || !outs || a.pairs < 1 || a.J < 1 || a.K < 1 || a.stride < 3 || a.max_iter < 0 ||
      !(a.max_corr_dist > 0.f) || (a.estimator != 0 && a.estimator != 1) || (search != 0 && search != 1))
    return fail(c, "%s: bad arguments", name);
  if (a.estimator == 1 && !normals_ref && a.stride < 6)
    return fail(c, "%s: bad arguments (the plane estimator without normals_ref reads the normals from columns 3..5 "
                   "of the points_ref rows: stride=%d, needs >= 6)", name, a.stride);
  if (!icp_robust_args_ok(a.kernel, a.kernel_scale))
    return fail(c, "%s: bad arguments (kernel=%d must be 0 l2, 1 huber, 2 cauchy, 3 gm or 4 tukey, and with a kernel other than l2 "
                   "kernel_scale=%g must be finite and positive)", name, a.kernel, (double)a.kernel_scale);
  if (search == 1 && (!icp_grid_radius_ok(a.max_corr_dist) || !icp_grid_shape_ok(a.pairs, a.J, a.K)))
    return fail(c, "%s: bad arguments (the grid search needs a max_corr_dist whose fp32 square is finite, and pairs x J "
                   "and pairs x K below 2^31)", name);
  a.search = icp_search_mode(search);
  a.normals = normals_ref ? normals_ref : a.ref + 3;
  a.normals_cs = normals_ref ? (int64_t)a.K * 3 : (int64_t)a.K * a.stride;
  a.normals_ld = normals_ref ? 3 : a.stride;
  void* scratch = c->ws.raw(corr ? icp_corr_scratch_bytes(a) : icp_scratch_bytes(a));
  if (c->ws.overflow) return fail(c, "workspace too small for %s (raise max_points / max_pairs)", name);
  if (const int e = corr ? launch_icp_correspondences(a, corr->idx, corr->d2, corr->stats, scratch, c->stream)
                         : launch_icp_refine(a, scratch, c->stream))
    return fail(c, "%s: the index build failed (HIP error %d)", name, e);
  return call.finish();
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

int dsir_icp_refine_ex3(dsir_ctx* c, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                        float max_corr_dist, int max_iter, float rel_fitness, float rel_rmse, const float* T_init, float* T_out,
                        int estimator, const float* normals_ref, int search, double* stats, const int32_t* counts_src, const int32_t* counts_ref) {
  IcpArgs a = icp_args(points_src, points_ref, pairs, J, K, stride, max_corr_dist, max_iter, rel_fitness, rel_rmse, T_init, T_out, estimator);
  a.stats5_out = stats;
  a.counts_src = counts_src; a.counts_ref = counts_ref;
  return icp_entry(c, "dsir_icp_refine_ex3", a, normals_ref, search, nullptr);
}

int dsir_icp_refine_ex4(dsir_ctx* c, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                        float max_corr_dist, int max_iter, float rel_fitness, float rel_rmse, const float* T_init, float* T_out,
                        int estimator, const float* normals_ref, int search, double* stats, const int32_t* counts_src, const int32_t* counts_ref,
                        int kernel, float kernel_scale) {
  IcpArgs a = icp_args(points_src, points_ref, pairs, J, K, stride, max_corr_dist, max_iter, rel_fitness, rel_rmse, T_init, T_out, estimator);
  a.stats5_out = stats;
  a.counts_src = counts_src; a.counts_ref = counts_ref;
  a.kernel = kernel; a.kernel_scale = kernel == kIcpL2 ? 0.f : kernel_scale;   // l2: the scale is ignored
  return icp_entry(c, "dsir_icp_refine_ex4", a, normals_ref, search, nullptr);
}

int dsir_icp_correspondences(dsir_ctx* c, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                             float max_corr_dist, const float* T, int search, int32_t* idx_out, float* d2_out, double* stats_out) {
  const IcpArgs a = icp_args(points_src, points_ref, pairs, J, K, stride, max_corr_dist, 0, 0.f, 0.f, T, nullptr, 0);
  const IcpCorrOut out{idx_out, d2_out, stats_out};
  return icp_entry(c, "dsir_icp_correspondences", a, nullptr, search, &out);
}

int dsir_icp_correspondences_ex(dsir_ctx* c, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                                float max_corr_dist, const float* T, int search, int32_t* idx_out, float* d2_out, double* stats_out,
                                const int32_t* counts_src, const int32_t* counts_ref) {
  IcpArgs a = icp_args(points_src, points_ref, pairs, J, K, stride, max_corr_dist, 0, 0.f, 0.f, T, nullptr, 0);
  a.counts_src = counts_src; a.counts_ref = counts_ref;
  const IcpCorrOut out{idx_out, d2_out, stats_out};
  return icp_entry(c, "dsir_icp_correspondences_ex", a, nullptr, search, &out);
}

// What the three pose-from-correspondences entries share, under the entry's own `name`: the Call scope and the checks of the common
// arguments; after the entry's checks of its own parameters the whole scratch, validated before the first launch; the way out.
struct CorrEntry {
  Call call; dsir_ctx* c; const char* name; CorrProblem p; bool refused;
  CorrEntry(dsir_ctx* c_, const char* name_, const CorrProblem& p_)
      : call(c_), c(c_), name(name_), p(p_), refused(call.refused() || check()) {}
  int check() {
    if (!p.src || !p.ref || !p.corr || !p.T_out || !p.stats || !p.invalid || p.pairs < 1 || p.J < 1 || p.K < 1 || p.M < 1 || p.stride < 3 ||
        !(p.max_dist > 0.f) || !std::isfinite(p.max_dist))
      return fail(c, "%s: bad arguments", name);
    if (p.refine_iters < 0 || p.refine_iters > DSIR_RANSAC_MAX_REFINE)
      return fail(c, "%s: refine_iters=%d outside [0,%d]", name, p.refine_iters, DSIR_RANSAC_MAX_REFINE);
    if (p.M > c->cfg.max_points || p.J > c->cfg.max_points || p.K > c->cfg.max_points)
      return fail(c, "%s: M=%d, J=%d or K=%d beyond max_points=%d", name, p.M, p.J, p.K, c->cfg.max_points);
    if (!pose_corr_shape_ok(p.pairs, p.M)) return fail(c, "%s: pairs x M = %lld unsupported", name, (long long)p.pairs * p.M);
    return 0;
  }
  void* reserve(size_t need, const char* what) {   // the arena is empty here: `need` bytes fit iff they are no more than it holds
    if (need <= c->ws.cap) return c->ws.raw(need);
    fail(c, "workspace too small for %s: needs %zu bytes (%s), the arena holds %zu (raise max_points / max_pairs, or pass fewer pairs)",
         name, need, what, c->ws.cap);
    return nullptr;
  }
  int launched(int r) { return r ? fail(c, "%s: launch failed (%d)", name, r) : call.finish(); }
};

int dsir_ransac_correspondence(dsir_ctx* c, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                               const int32_t* corr, const int32_t* counts, int M, float max_dist, int ransac_n, float edge_sim,
                               int hypotheses, int refine_iters, uint64_t seed, const float* T_init, float* T_out, double* stats,
                               int32_t* invalid, const dsir_ransac_diag* diag) {
  CorrEntry e(c, "dsir_ransac_correspondence",
              {points_src, points_ref, pairs, J, K, stride, corr, counts, M, max_dist, refine_iters, T_init, T_out, stats, invalid});
  if (e.refused) return 1;
  if (!std::isfinite(edge_sim)) return fail(c, "%s: bad arguments (edge_sim must be finite)", e.name);
  if (ransac_n != 3 && ransac_n != 4) return fail(c, "%s: ransac_n must be 3 or 4 (got %d)", e.name, ransac_n);
  if (hypotheses < 1 || hypotheses > DSIR_RANSAC_MAX_HYPOTHESES)
    return fail(c, "%s: hypotheses=%d outside [1,%d]", e.name, hypotheses, DSIR_RANSAC_MAX_HYPOTHESES);
  void* scratch = e.reserve(ransac_scratch_bytes(pairs, M, hypotheses, refine_iters), "pairs x (M x 28 + hypotheses x 56)-order");
  if (!scratch) return 1;
  RansacArgs a{e.p, ransac_n, edge_sim, hypotheses, seed};
  if (diag) { a.diag_sample = diag->hyp_sample; a.diag_T = diag->hyp_T; a.diag_valid = diag->hyp_valid; a.diag_count = diag->hyp_count; }
  return e.launched(launch_ransac(a, scratch, c->stream));
}

int dsir_consensus_correspondence(dsir_ctx* c, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                                  const int32_t* corr, const int32_t* counts, int M, float max_dist, float compat_dist, int seeds,
                                  int members, int refine_iters, const float* T_init, float* T_out, double* stats, int32_t* invalid,
                                  const dsir_consensus_diag* diag) {
  CorrEntry e(c, "dsir_consensus_correspondence",
              {points_src, points_ref, pairs, J, K, stride, corr, counts, M, max_dist, refine_iters, T_init, T_out, stats, invalid});
  if (e.refused) return 1;
  if (!std::isfinite(compat_dist)) return fail(c, "%s: bad arguments (compat_dist must be finite)", e.name);
  if (seeds < 1 || seeds > DSIR_CONSENSUS_MAX_SEEDS) return fail(c, "%s: seeds=%d outside [1,%d]", e.name, seeds, DSIR_CONSENSUS_MAX_SEEDS);
  if (members < 3 || members > DSIR_CONSENSUS_MAX_MEMBERS)
    return fail(c, "%s: members=%d outside [3,%d]", e.name, members, DSIR_CONSENSUS_MAX_MEMBERS);
  if (M > DSIR_CONSENSUS_MAX_M) return fail(c, "%s: M=%d beyond DSIR_CONSENSUS_MAX_M=%d", e.name, M, DSIR_CONSENSUS_MAX_M);
  void* scratch = e.reserve(consensus_scratch_bytes(pairs, M, seeds, refine_iters), "the bit matrix alone: pairs x M x ceil(M / 64) x 8");
  if (!scratch) return 1;
  ConsensusArgs a{e.p, compat_dist, seeds, members};
  if (diag) {
    a.diag_bits = diag->bits; a.diag_score = diag->score; a.diag_seed = diag->seed; a.diag_members = diag->seed_members;
    a.diag_T = diag->seed_T; a.diag_valid = diag->seed_valid; a.diag_count = diag->seed_count;
  }
  return e.launched(launch_consensus(a, scratch, c->stream));
}

int dsir_fgr_correspondence(dsir_ctx* c, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                            const int32_t* corr, const int32_t* counts, int M, float max_dist, int tuple_test, float tuple_scale,
                            int max_tuples, int max_trials, int iterations, float division_factor, int refine_iters, uint64_t seed,
                            const float* T_init, float* T_out, double* stats, int32_t* invalid, const dsir_fgr_diag* diag) {
  CorrEntry e(c, "dsir_fgr_correspondence",
              {points_src, points_ref, pairs, J, K, stride, corr, counts, M, max_dist, refine_iters, T_init, T_out, stats, invalid});
  if (e.refused) return 1;
  if (!(tuple_scale > 0.f) || !(tuple_scale <= 1.f)) return fail(c, "%s: tuple_scale=%g outside (0,1]", e.name, (double)tuple_scale);
  if (max_tuples < 1 || max_tuples > DSIR_FGR_MAX_TUPLES) return fail(c, "%s: max_tuples=%d outside [1,%d]", e.name, max_tuples, DSIR_FGR_MAX_TUPLES);
  if (max_trials < 1 || max_trials > DSIR_FGR_MAX_TRIALS) return fail(c, "%s: max_trials=%d outside [1,%d]", e.name, max_trials, DSIR_FGR_MAX_TRIALS);
  if (iterations < 1 || iterations > DSIR_FGR_MAX_ITERS) return fail(c, "%s: iterations=%d outside [1,%d]", e.name, iterations, DSIR_FGR_MAX_ITERS);
  if (!std::isfinite(division_factor)) return fail(c, "%s: division_factor must be finite", e.name);
  if (!fgr_shape_ok(pairs, M, max_trials))
    return fail(c, "%s: pairs=%d with max_trials=%d and M=%d unsupported (pairs <= 65535, pairs x max_trials and pairs x M below 2^31)",
                e.name, pairs, max_trials, M);
  const int tt = tuple_test ? 1 : 0;
  void* scratch = e.reserve(fgr_scratch_bytes(pairs, M, tt, max_tuples, max_trials, refine_iters),
                            tt ? "pairs x (M x 28 + rows x 52)-order, rows = 3 x max_tuples" : "pairs x (M x 28 + rows x 52)-order, rows = M");
  if (!scratch) return 1;
  FgrArgs a{e.p, tt, tuple_scale * tuple_scale, max_tuples, max_trials, iterations, division_factor, seed};   // ts2: fp32, rounded once
  if (diag) {
    a.diag_rows = diag->rows; a.diag_n_rows = diag->n_rows; a.diag_trials = diag->trials; a.diag_norm = diag->norm;
    a.diag_iter_T = diag->iter_T; a.diag_iter_mu = diag->iter_mu; a.diag_iter_energy = diag->iter_energy; a.diag_iters_run = diag->iters_run;
  }
  return e.launched(launch_fgr(a, scratch, c->stream));
}

int dsir_pose_finetune(dsir_ctx* c, const float* xyz_src, const float* xyz_ref, const float* weights, int weights_are_logits,
                       int pairs, int m, const float* T_init, float quantization_size, int max_iter, float break_threshold_ratio,
                       int max_break_count, float* T_out, double* stats) {
  Call call(c); if (call.refused()) return 1;
  if (!xyz_src || !xyz_ref || !T_init || !T_out || pairs < 1 || m < 1 || max_iter < 0 || max_break_count < 1 ||
      !(quantization_size > 0.f) || !(break_threshold_ratio >= 0.f))
    return fail(c, "dsir_pose_finetune: bad arguments");
  launch_pose_finetune(xyz_src, xyz_ref, weights, weights_are_logits ? 1 : 0, pairs, m, T_init, quantization_size, max_iter,
                       break_threshold_ratio, max_break_count, T_out, stats, c->stream);
  return call.finish();
}

// One body behind the three entries: the kernel always writes three columns (point distance, confidence, pose error); the
// two older entries run it with weight 0 and hand their callers the first two.
static int align_loss_body(dsir_ctx* c, const float* pt_src, const float* pt_ref, const int32_t* idx, const float* logits,
                           const float* labels, const float* transform_gt, int pairs, int J, int K, int n_iter, int loss_type,
                           float wt_ptDist_loss, float wt_inlier_loss, float loss_discount_factor, float wt_pose_loss, float* transforms,
                           double* losses, float* grad_logits, double* losses_per_pair, int cols) {
  Call call(c); if (call.refused()) return 1;
  if (!pt_src || !pt_ref || !idx || !logits || !transform_gt || !grad_logits || pairs < 1 || J < 1 || K < 1 || n_iter < 1 ||
      n_iter > 8 || (loss_type != 0 && loss_type != 1))
    return fail(c, "dsir_align_loss_backward: bad arguments (n_iter in [1,8], loss_type 0 = mae / 1 = mse)");
  if (!(wt_pose_loss >= 0.f) || !std::isfinite(wt_pose_loss))
    return fail(c, "dsir_align_loss_backward3: wt_pose_loss must be finite and >= 0");
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
  return call.finish();
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

int dsir_eval_metrics(dsir_ctx* c, const float* pred_T, int64_t pred_stride, const float* gt_T, const float* points_src,
                      const float* points_ref, int pairs, int n, int stride, float rte_thresh, float rre_thresh,
                      double* out) {
  Call call(c); if (call.refused()) return 1;
  if (!pred_T || !gt_T || !points_src || !points_ref || !out || pairs < 1 || n < 1 || stride < 3 || pred_stride < 12)
    return fail(c, "dsir_eval_metrics: bad arguments");
  launch_eval_metrics(pred_T, pred_stride, gt_T, points_src, points_ref, pairs, n, stride, rte_thresh, rre_thresh, out,
                      c->stream);
  return call.finish();
}

}  // extern "C"
