// The pose entries of include/dsir.h: weighted Kabsch, ICP, RANSAC, spatial consensus and FGR from correspondences, the pose
// fine-tune, the alignment loss with its backward, and the evaluation metrics.
#include <cmath>

#include "engine_ctx.h"
#include "icp_grid.h"

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

// What the four ICP entries share: the checks under the entry's own `name`, the workspace reset, the scratch, the normals
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
  Call call(c); if (call.refused()) return 1;
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
  void* scratch = c->ws.raw(ransac_scratch_bytes(pairs, M, hypotheses, refine_iters));
  if (c->ws.overflow) return fail(c, "workspace too small for dsir_ransac_correspondence (pairs x (M x 28 + hypotheses x 56) bytes: raise max_points / max_pairs)");
  RansacArgs a{};
  a.src = points_src; a.ref = points_ref; a.pairs = pairs; a.J = J; a.K = K; a.stride = stride; a.corr = corr; a.counts = counts;
  a.M = M; a.max_dist = max_dist; a.n = ransac_n; a.edge_sim = edge_sim; a.hypotheses = hypotheses; a.refine_iters = refine_iters;
  a.seed = seed; a.T_init = T_init; a.T_out = T_out; a.stats = stats; a.invalid = invalid;
  if (diag) { a.diag_sample = diag->hyp_sample; a.diag_T = diag->hyp_T; a.diag_valid = diag->hyp_valid; a.diag_count = diag->hyp_count; }
  launch_ransac(a, scratch, c->stream);
  return call.finish();
}

int dsir_consensus_correspondence(dsir_ctx* c, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                                  const int32_t* corr, const int32_t* counts, int M, float max_dist, float compat_dist, int seeds,
                                  int members, int refine_iters, const float* T_init, float* T_out, double* stats, int32_t* invalid,
                                  const dsir_consensus_diag* diag) {
  Call call(c); if (call.refused()) return 1;
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
  // the whole workspace, validated before the first launch
  const size_t need = consensus_scratch_bytes(pairs, M, seeds, refine_iters);
  if (need > c->ws.cap)
    return fail(c, "workspace too small for dsir_consensus_correspondence: needs %zu bytes (the bit matrix alone: pairs x M x ceil(M / 64) x 8 = "
                   "%zu), the arena holds %zu (raise max_points / max_pairs, or pass fewer pairs)", need,
                (size_t)pairs * M * ((size_t)(M + 63) / 64) * 8, c->ws.cap);
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
  return call.finish();
}

int dsir_fgr_correspondence(dsir_ctx* c, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                            const int32_t* corr, const int32_t* counts, int M, float max_dist, int tuple_test, float tuple_scale,
                            int max_tuples, int max_trials, int iterations, float division_factor, int refine_iters, uint64_t seed,
                            const float* T_init, float* T_out, double* stats, int32_t* invalid, const dsir_fgr_diag* diag) {
  Call call(c); if (call.refused()) return 1;
  if (!points_src || !points_ref || !corr || !T_out || !stats || !invalid || pairs < 1 || J < 1 || K < 1 || M < 1 || stride < 3 ||
      !(max_dist > 0.f) || !std::isfinite(max_dist))
    return fail(c, "dsir_fgr_correspondence: bad arguments");
  if (!(tuple_scale > 0.f) || !(tuple_scale <= 1.f))
    return fail(c, "dsir_fgr_correspondence: tuple_scale=%g outside (0,1]", (double)tuple_scale);
  if (max_tuples < 1 || max_tuples > DSIR_FGR_MAX_TUPLES)
    return fail(c, "dsir_fgr_correspondence: max_tuples=%d outside [1,%d]", max_tuples, DSIR_FGR_MAX_TUPLES);
  if (max_trials < 1 || max_trials > DSIR_FGR_MAX_TRIALS)
    return fail(c, "dsir_fgr_correspondence: max_trials=%d outside [1,%d]", max_trials, DSIR_FGR_MAX_TRIALS);
  if (iterations < 1 || iterations > DSIR_FGR_MAX_ITERS)
    return fail(c, "dsir_fgr_correspondence: iterations=%d outside [1,%d]", iterations, DSIR_FGR_MAX_ITERS);
  if (!std::isfinite(division_factor)) return fail(c, "dsir_fgr_correspondence: division_factor must be finite");
  if (refine_iters < 0 || refine_iters > DSIR_RANSAC_MAX_REFINE)
    return fail(c, "dsir_fgr_correspondence: refine_iters=%d outside [0,%d]", refine_iters, DSIR_RANSAC_MAX_REFINE);
  if (M > c->cfg.max_points || J > c->cfg.max_points || K > c->cfg.max_points)
    return fail(c, "dsir_fgr_correspondence: M=%d, J=%d or K=%d beyond max_points=%d", M, J, K, c->cfg.max_points);
  if (pairs > 65535 || (int64_t)pairs * ((int64_t)max_trials + 256) > 0x7fffffffll || (int64_t)pairs * M > 0x7fffffffll)
    return fail(c, "dsir_fgr_correspondence: pairs=%d with max_trials=%d and M=%d unsupported (pairs <= 65535, pairs x max_trials and "
                   "pairs x M below 2^31)", pairs, max_trials, M);
  // the whole workspace, validated before the first launch
  const size_t need = fgr_scratch_bytes(pairs, M, tuple_test ? 1 : 0, max_tuples, max_trials, refine_iters);
  if (need > c->ws.cap)
    return fail(c, "workspace too small for dsir_fgr_correspondence: needs %zu bytes (pairs x (M x 28 + rows x 52)-order, rows = %s), "
                   "the arena holds %zu (raise max_points / max_pairs, or pass fewer pairs or a smaller max_tuples)", need,
                tuple_test ? "3 x max_tuples" : "M", c->ws.cap);
  void* scratch = c->ws.raw(need);
  if (c->ws.overflow) return fail(c, "workspace too small for dsir_fgr_correspondence");
  FgrArgs a{};
  a.src = points_src; a.ref = points_ref; a.pairs = pairs; a.J = J; a.K = K; a.stride = stride; a.corr = corr; a.counts = counts;
  a.M = M; a.max_dist = max_dist; a.tuple_test = tuple_test ? 1 : 0; a.ts2 = tuple_scale * tuple_scale;   // fp32, rounded once
  a.max_tuples = max_tuples; a.max_trials = max_trials; a.iterations = iterations; a.division_factor = division_factor;
  a.refine_iters = refine_iters; a.seed = seed; a.T_init = T_init; a.T_out = T_out; a.stats = stats; a.invalid = invalid;
  if (diag) {
    a.diag_rows = diag->rows; a.diag_n_rows = diag->n_rows; a.diag_trials = diag->trials; a.diag_norm = diag->norm;
    a.diag_iter_T = diag->iter_T; a.diag_iter_mu = diag->iter_mu; a.diag_iter_energy = diag->iter_energy; a.diag_iters_run = diag->iters_run;
  }
  if (int r = launch_fgr(a, scratch, c->stream)) return fail(c, "dsir_fgr_correspondence: launch failed (%d)", r);
  return call.finish();
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
