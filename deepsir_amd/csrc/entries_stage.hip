// The stage entries of include/dsir.h: index narrowing, the KNN pyramid, one RandLA pass and the use_ppf front end, normals,
// FPFH, ISS keypoints, farthest-point sampling, plane segmentation, score, aggregation, and the preprocessing (voxel down-sampling, resampling).
#include <cmath>

#include "engine_ctx.h"
#include "fps.h"
#include "plane.h"

using namespace dsir;

extern "C" {

int dsir_narrow_i64(dsir_ctx* c, const int64_t* src, int32_t* dst, int64_t n) {
  Call call(c); if (call.refused()) return 1;
  launch_narrow_i64(src, dst, n, c->stream);
  return call.finish();
}

int dsir_knn_pyramid(dsir_ctx* c, const float* points, int stride, int clouds, int n, float* xyz, int32_t* neigh,
                     int32_t* sub, int32_t* interp) {
  Call call(c); if (call.refused()) return 1;
  if (clouds < 1 || stride < 3) return fail(c, "dsir_knn_pyramid: bad arguments");
  if (int r = build_pyramid(c, points, stride, clouds, n, xyz, neigh, sub, interp)) return r;
  return call.finish();
}

int dsir_randla_forward(dsir_ctx* c, int which, const float* features, int cin, int clouds, int n, const float* xyz,
                        const int32_t* neigh, const int32_t* sub, const int32_t* interp, float* feat, float* logits) {
  Call call(c, Call::kWeights); if (call.refused()) return 1;
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
  if (int r = call.begin_walker()) return r;
  if (int r = randla_forward(c, w, in0, w.ppf ? &in1 : nullptr, py, feat, logits)) return r;
  return call.finish();
}

int dsir_lfa_enc2_probe(dsir_ctx* c, int which, int level, int fused, int clouds, int n, const float* xyz, const int32_t* neigh,
                        float* rows, double* stats) {
  Call call(c, Call::kWeights); if (call.refused()) return 1;
  if (which != 0 && c->cfg.pipeline != DSIR_PIPELINE_ALIGN) return fail(c, "dsir_lfa_enc2_probe: this context has no inlier_model (pipeline != align)");
  if (!xyz || !neigh || !rows || !stats || clouds < 1 || level < 0 || level >= c->cfg.num_layers) return fail(c, "dsir_lfa_enc2_probe: bad arguments");
  if (check_batch(c, "dsir_lfa_enc2_probe", clouds, n)) return 1;
  Pyramid py;
  fill_pyramid_layout(c->cfg, clouds, n, py);
  if (py.nl[c->cfg.num_layers - 1] < kKnn) return fail(c, "cloud too small (n=%d)", n);
  py.xyz = xyz; py.neigh = neigh;
  if (int r = run_lfa_enc2_probe(c, which == 0 ? c->net.feat : c->net.inl, level, fused, py, rows, stats)) return r;
  return call.finish();
}

int dsir_mlp_feat_probe(dsir_ctx* c, const float* feat0, int clouds, int n, int fused, int max_workgroups, float* out) {
  Call call(c, Call::kWeights); if (call.refused()) return 1;
  if (c->cfg.pipeline == DSIR_PIPELINE_LABEL) return fail(c, "dsir_mlp_feat_probe: a label-pipeline context has no aggregation layers");
  if (!feat0 || !out || clouds < 1 || n < 1 || fused < 0 || fused > 2 || (fused == 2 && (clouds & 1)) || max_workgroups < 0) return fail(c, "dsir_mlp_feat_probe: bad arguments");
  if (check_batch(c, "dsir_mlp_feat_probe", clouds, n)) return 1;
  if (int r = run_mlp_feat_probe(c, feat0, clouds, n, fused, max_workgroups, out)) return r;
  return call.finish();
}

int dsir_ppf_pre(dsir_ctx* c, int which, const float* rows, int stride, const int32_t* neigh, int64_t neigh_cs, int clouds, int n,
                 float* out) {
  Call call(c, Call::kWeights); if (call.refused()) return 1;
  if (!(c->flags & DSIR_FLAG_PPF)) return fail(c, "dsir_ppf_pre: the context was not created with DSIR_FLAG_PPF");
  if (which != 0 && c->cfg.pipeline != DSIR_PIPELINE_ALIGN) return fail(c, "dsir_ppf_pre: this context has no inlier_model (pipeline != align)");
  if (!rows || !neigh || !out || clouds < 1 || n < kKnn) return fail(c, "dsir_ppf_pre: bad arguments");
  if (stride < 6) return fail(c, "dsir_ppf_pre: rows of xyz + normal need at least 6 columns, got %d (reference RandLANet.py:325)", stride);
  if (check_batch(c, "dsir_ppf_pre", clouds, n)) return 1;
  if (int r = run_ppf_pre(c, which == 0 ? c->net.feat : c->net.inl, rows, stride, neigh, neigh_cs, clouds, n, out)) return r;
  return call.finish();
}

int dsir_estimate_normals(dsir_ctx* c, const float* points, int stride, const int32_t* neigh, int64_t neigh_cs, int clouds, int n,
                          const float* viewpoint, float* normals, int32_t* flags) {
  Call call(c); if (call.refused()) return 1;
  if (!points || !neigh || !normals || clouds < 1 || clouds > 65535 || n < 1 || stride < 3) return fail(c, "dsir_estimate_normals: bad arguments");
  const float v[3] = {viewpoint ? viewpoint[0] : 0.f, viewpoint ? viewpoint[1] : 0.f, viewpoint ? viewpoint[2] : 0.f};
  launch_estimate_normals(points, (int64_t)n * stride, stride, neigh, neigh_cs, n, clouds, v[0], v[1], v[2], normals, flags, c->stream);
  return call.finish();
}

int dsir_estimate_normals_csr(dsir_ctx* c, const float* points, int stride, const int32_t* csr_offsets, const int32_t* csr_cols, int clouds,
                              int n, const float* viewpoint, float* normals, int32_t* flags) {
  Call call(c); if (call.refused()) return 1;
  if (!points || !csr_offsets || !csr_cols || !normals || clouds < 1 || clouds > 65535 || n < 1 || stride < 3)
    return fail(c, "dsir_estimate_normals_csr: bad arguments");
  const float v[3] = {viewpoint ? viewpoint[0] : 0.f, viewpoint ? viewpoint[1] : 0.f, viewpoint ? viewpoint[2] : 0.f};
  launch_estimate_normals_csr(points, (int64_t)n * stride, stride, csr_offsets, csr_cols, n, clouds, v[0], v[1], v[2], normals, flags, c->stream);
  return call.finish();
}

int dsir_fpfh(dsir_ctx* c, const float* points, int stride, const float* normals, const int32_t* neigh, int64_t neigh_cs,
              const int32_t* csr_offsets, const int32_t* csr_cols, int clouds, int n, float* desc, int out_ld, int32_t* flags) {
  Call call(c); if (call.refused()) return 1;
  if (!points || !desc || clouds < 1 || clouds > 65535 || n < 1 || stride < 3 || out_ld < kFpfhDim) return fail(c, "dsir_fpfh: bad arguments");
  if (!normals && stride < 6) return fail(c, "dsir_fpfh: without normals the rows need xyz + normal, at least 6 columns, got %d", stride);
  const bool fixed = neigh != nullptr, csr = csr_offsets != nullptr || csr_cols != nullptr;
  if (fixed == csr) return fail(c, "dsir_fpfh: exactly one of neigh_idx and (csr_offsets, csr_cols) expected");
  if (csr && (!csr_offsets || !csr_cols)) return fail(c, "dsir_fpfh: a CSR list needs both csr_offsets and csr_cols");
  if ((int64_t)clouds * n > 0x7fffffffll / kFpfhRow) return fail(c, "dsir_fpfh: clouds x n = %lld rows beyond the int32 range of the SPFH table", (long long)clouds * n);
  FpfhArgs a;
  a.table = reinterpret_cast<int32_t*>(c->ws.raw(fpfh_scratch_bytes(clouds, n)));
  if (c->ws.overflow) return fail(c, "workspace too small for dsir_fpfh (clouds x n x 136 bytes: raise max_points / max_pairs)");
  a.pts = points; a.pts_cs = (int64_t)n * stride; a.pts_ld = stride;
  a.nrm = normals ? normals : points + 3; a.nrm_ld = normals ? 3 : stride; a.nrm_cs = (int64_t)n * a.nrm_ld;
  a.cols = fixed ? neigh : csr_cols; a.neigh_cs = neigh_cs; a.offsets = csr_offsets;
  a.desc = desc; a.out_ld = out_ld; a.flags = flags; a.n = n; a.clouds = clouds;
  if (!launch_fpfh(a, c->stream)) return fail(c, "dsir_fpfh: shape refused");
  return call.finish();
}

int dsir_iss_keypoints(dsir_ctx* c, const float* points, int stride, const int32_t* sal_offsets, const int32_t* sal_cols,
                       const int32_t* nms_offsets, const int32_t* nms_cols, int clouds, int n, double gamma_21, double gamma_32,
                       int min_neighbors, float* saliency, int32_t* mask, int32_t* index, int32_t* counts) {
  Call call(c); if (call.refused()) return 1;
  if (!points || !sal_offsets || !sal_cols || !nms_offsets || !nms_cols || !saliency || !mask || !index || !counts)
    return fail(c, "dsir_iss_keypoints: a null pointer among points, the two CSR lists and the four outputs");
  if (clouds < 1 || clouds > 65535 || n < 1 || stride < 3)
    return fail(c, "dsir_iss_keypoints: clouds in [1, 65535], n >= 1 and stride >= 3 expected, got clouds=%d n=%d stride=%d", clouds, n, stride);
  if (!(gamma_21 > 0.0) || !(gamma_32 > 0.0) || std::isinf(gamma_21) || std::isinf(gamma_32))
    return fail(c, "dsir_iss_keypoints: gamma_21 and gamma_32 must be finite and positive, got %g and %g", gamma_21, gamma_32);
  if (min_neighbors < 1) return fail(c, "dsir_iss_keypoints: min_neighbors >= 1 expected, got %d", min_neighbors);
  if ((int64_t)clouds * n > 0x7fffffffll - 1) return fail(c, "dsir_iss_keypoints: clouds x n = %lld rows beyond the int32 range of the offsets", (long long)clouds * n);
  IssArgs a;
  a.block_counts = reinterpret_cast<int32_t*>(c->ws.raw(iss_scratch_bytes(clouds, n)));
  if (c->ws.overflow) return fail(c, "workspace too small for dsir_iss_keypoints (raise max_points / max_pairs)");
  a.pts = points; a.pts_cs = (int64_t)n * stride; a.pts_ld = stride;
  a.sal_offsets = sal_offsets; a.sal_cols = sal_cols; a.nms_offsets = nms_offsets; a.nms_cols = nms_cols;
  a.gamma_21 = gamma_21; a.gamma_32 = gamma_32; a.min_neighbors = min_neighbors;
  a.saliency = saliency; a.mask = mask; a.index = index; a.counts = counts; a.n = n; a.clouds = clouds;
  if (!launch_iss_keypoints(a, c->stream)) return fail(c, "dsir_iss_keypoints: shape refused");
  return call.finish();
}

int dsir_farthest_point_sample(dsir_ctx* c, const float* points, int stride, const int32_t* counts, int clouds, int cap, int k, int start,
                               int32_t* index, int32_t* counts_out, float* min_d2) {
  Call call(c); if (call.refused()) return 1;
  if (!points || !index || !counts_out || !min_d2)
    return fail(c, "dsir_farthest_point_sample: a null pointer among points and the three outputs");
  if (clouds < 1 || clouds > 65535 || cap < 1 || stride < 3)
    return fail(c, "dsir_farthest_point_sample: clouds in [1, 65535], cap >= 1 and stride >= 3 expected, got clouds=%d cap=%d stride=%d", clouds, cap, stride);
  if (k < 1 || k > cap) return fail(c, "dsir_farthest_point_sample: k in [1, cap] expected, got k=%d cap=%d", k, cap);
  if (start < 0) return fail(c, "dsir_farthest_point_sample: start >= 0 expected, got %d", start);
  if (cap > kFpsMaxRows) return fail(c, "dsir_farthest_point_sample: cap=%d beyond the limit of %d rows per cloud (one workgroup per cloud)", cap, kFpsMaxRows);
  FpsArgs a;
  a.scratch = c->ws.raw(fps_scratch_bytes(clouds, cap));
  if (c->ws.overflow) return fail(c, "workspace too small for dsir_farthest_point_sample (raise max_points / max_pairs)");
  a.pts = points; a.pts_cs = (int64_t)cap * stride; a.pts_ld = stride; a.counts = counts;
  a.clouds = clouds; a.cap = cap; a.k = k; a.start = start;
  a.index = index; a.counts_out = counts_out; a.min_d2 = min_d2;
  if (!launch_fps(a, c->stream)) return fail(c, "dsir_farthest_point_sample: shape refused");
  return call.finish();
}

int dsir_segment_plane(dsir_ctx* c, const float* points, int stride, const int32_t* counts, const int32_t* cloud_ids, int clouds, int cap,
                       float distance_threshold, int hypotheses, int max_planes, int min_inliers, int refine_iters, float axis_x,
                       float axis_y, float axis_z, double cos_min, uint64_t seed, int32_t* labels, int32_t* num_planes, float* planes,
                       float* anchors, int32_t* plane_counts, int32_t* stats) {
  Call call(c); if (call.refused()) return 1;
  if (!points || !labels || !num_planes || !planes || !anchors || !plane_counts || !stats)
    return fail(c, "dsir_segment_plane: a null pointer among points and the six outputs");
  if (clouds < 1 || clouds > kPlaneMaxClouds) return fail(c, "dsir_segment_plane: clouds in [1, %d] expected, got %d", kPlaneMaxClouds, clouds);
  if (cap < 1 || (int64_t)clouds * cap >= ((int64_t)1 << 31))
    return fail(c, "dsir_segment_plane: cap >= 1 with clouds x cap < 2^31 expected, got clouds=%d cap=%d", clouds, cap);
  if (stride < 3) return fail(c, "dsir_segment_plane: stride >= 3 expected, got %d", stride);
  if (hypotheses < 1 || hypotheses > kPlaneMaxHyp) return fail(c, "dsir_segment_plane: hypotheses in [1, %d] expected, got %d", kPlaneMaxHyp, hypotheses);
  if (!(distance_threshold > 0.f) || !std::isfinite(distance_threshold))
    return fail(c, "dsir_segment_plane: distance_threshold finite and positive expected, got %g", (double)distance_threshold);
  if (max_planes < 1 || max_planes > kPlaneMaxPlanes) return fail(c, "dsir_segment_plane: max_planes in [1, %d] expected, got %d", kPlaneMaxPlanes, max_planes);
  if (min_inliers < kPlaneMinInliers) return fail(c, "dsir_segment_plane: min_inliers >= %d expected, got %d", kPlaneMinInliers, min_inliers);
  if (refine_iters < 0 || refine_iters > kPlaneMaxRefits) return fail(c, "dsir_segment_plane: refine_iters in [0, %d] expected, got %d", kPlaneMaxRefits, refine_iters);
  if (!std::isfinite(axis_x) || !std::isfinite(axis_y) || !std::isfinite(axis_z) || !std::isfinite(cos_min))
    return fail(c, "dsir_segment_plane: axis and cos_min must be finite");
  PlaneArgs a;
  a.scratch = c->ws.raw(plane_scratch_bytes(clouds, cap, hypotheses));
  if (c->ws.overflow) return fail(c, "workspace too small for dsir_segment_plane (raise max_points / max_pairs)");
  a.pts = points; a.pts_cs = (int64_t)cap * stride; a.pts_ld = stride; a.counts = counts; a.cloud_ids = cloud_ids;
  a.clouds = clouds; a.cap = cap; a.H = hypotheses; a.max_planes = max_planes; a.min_inliers = min_inliers; a.refine_iters = refine_iters;
  a.thr = distance_threshold; a.axis[0] = axis_x; a.axis[1] = axis_y; a.axis[2] = axis_z; a.cos_min = cos_min; a.seed = seed;
  a.labels = labels; a.num_planes = num_planes; a.planes = planes; a.anchors = anchors; a.plane_counts = plane_counts; a.stats = stats;
  if (!launch_segment_plane(a, c->stream)) return fail(c, "dsir_segment_plane: shape refused");
  return call.finish();
}

int dsir_score(dsir_ctx* c, const float* feat, const float* logits, const float* xyz, int64_t xyz_cs,
               const int32_t* neigh, int64_t neigh_cs, int clouds, int n, float* score, int32_t* label) {
  Call call(c, Call::kWeights); if (call.refused()) return 1;
  if (!feat || !logits || !xyz || !neigh || !score || clouds < 1 || n < 1) return fail(c, "dsir_score: bad arguments");
  if (check_batch(c, "dsir_score", clouds, n)) return 1;
  ScoreScratch s;
  s.red = c->ws.get<float>((size_t)clouds * 4);
  s.prob = c->ws.get<float>((size_t)clouds * n);
  s.label = c->ws.get<int32_t>((size_t)clouds * n);
  if (c->ws.overflow) return fail(c, "workspace exhausted in dsir_score");
  launch_score(feat, logits, c->cfg.num_classes, xyz, xyz_cs, neigh, neigh_cs, clouds, n, s, score, label, c->stream);
  return call.finish();
}

int dsir_aggregate(dsir_ctx* c, const float* xyz, int64_t xyz_cs, const float* feat0, const float* score, int clouds,
                   int n, float* desc) {
  Call call(c, Call::kWeights); if (call.refused()) return 1;
  if (c->cfg.pipeline == DSIR_PIPELINE_LABEL) return fail(c, "dsir_aggregate: a label-pipeline context has no aggregation layers");
  if (!xyz || !feat0 || !score || !desc || clouds < 1 || n < 1) return fail(c, "dsir_aggregate: bad arguments");
  if (check_batch(c, "dsir_aggregate", clouds, n)) return 1;
  float* F = run_mlp_feat(c, feat0, clouds, n);
  run_att_proj(c, xyz, xyz_cs, score, F, clouds, n, desc);
  return call.finish();
}

int dsir_voxel_downsample(dsir_ctx* c, const float* points, const int64_t* offsets, int clouds, int stride, float voxel_size,
                          const float* crop, int cap, float* out, int32_t* counts) {
  Call call(c); if (call.refused()) return 1;
  if (!points || !offsets || !out || !counts || stride < 3 || stride > 16 || cap < 1 || !(voxel_size > 0.f))
    return fail(c, "dsir_voxel_downsample: bad arguments");
  if (clouds < 1 || clouds > 1000) return fail(c, "dsir_voxel_downsample: %d clouds in one call (1 to 1000 supported)", clouds);
  const int64_t total = offsets[clouds];
  if (total <= 0 || total > 0x7fffffffll) return fail(c, "dsir_voxel_downsample: %lld points unsupported", (long long)total);
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
  return call.finish();
}

int dsir_resample(dsir_ctx* c, const float* in, const int32_t* counts, int clouds, int cap, int stride, int k, int mode,
                  uint64_t seed, float* out) {
  Call call(c); if (call.refused()) return 1;
  if (!in || !counts || !out || clouds < 1 || cap < 1 || stride < 1 || k < 1 || (mode != 0 && mode != 1))
    return fail(c, "dsir_resample: bad arguments");
  void* scratch = c->ws.raw(resample_scratch_bytes(clouds, cap));
  if (c->ws.overflow) return fail(c, "workspace too small for dsir_resample");
  if (int r = launch_resample(in, counts, clouds, cap, stride, k, mode, seed, out, scratch, c->stream))
    return fail(c, "dsir_resample: launch failed (%d)", r);
  return call.finish();
}

}  // extern "C"
