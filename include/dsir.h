/*
 * dsir.h — C ABI of the MI355X-native registration engine (libdsir.so).
 *
 * Drop-in boundary for the hot path of LeoQLi/DeepSIR.  Every
 * entry point names the reference interface it replaces (file:line into the
 * reference tree).  Plain pointers and sizes only; no torch types.
 *
 * Conventions
 *   - All tensor pointers are DEVICE pointers (HBM) unless a parameter says
 *     "host".  Calls are asynchronous on the context's HIP stream
 *     (dsir_stream) unless documented otherwise; dsir_sync waits for it.
 *   - Activations are POINT-MAJOR: a feature tensor is [clouds][points][C]
 *     fp32 (the reference is channel-major [B,C,N]; the Python wrapper
 *     transposes where it returns such tensors to the caller).
 *   - Indices are int32 on this side (the reference's int64 index tensors are
 *     narrowed with dsir_narrow_i64).
 *   - A "cloud batch" is a set of clouds with the same point count; src and
 *     ref clouds of P pairs are 2P clouds for the shared feature extractor.
 *   - Return value: 0 on success, non-zero on error; the message is then
 *     available from dsir_last_error.  A degenerate Kabsch covariance is NOT
 *     an error: identity is returned and the pair's invalid flag is set
 *     (reference network/model.py:61-64).
 *   - A context is not thread-safe: one context per (thread, device).
 */
#ifndef DSIR_H
#define DSIR_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSIR_MAX_LEVELS 4
#define DSIR_KNN 16

typedef struct dsir_ctx dsir_ctx;

/* The args fields the path reads: reference arguments.py:27-82,
 * network/model.py:122-126, network/RandLANet.py:240-247. */
typedef struct dsir_cfg {
  int32_t feat_len;                       /* 3 (xyz) or 4 (xyz+reflectance)   */
  int32_t num_knn;                        /* must be 16                        */
  int32_t num_layers;                     /* must be 4                         */
  int32_t sub_sampling_ratio[DSIR_MAX_LEVELS];
  int32_t d_out[DSIR_MAX_LEVELS];         /* 16,64,128,256                     */
  int32_t out_feat_dim;                   /* 64                                */
  int32_t num_classes;                    /* 19 (semantic head of feat_extractor) */
  int32_t max_points;                     /* workspace sizing: points per cloud (1024 .. dsir_max_points_limit(): 131072, the bound up
                                           * to which the GroupNorm statistics are provably order independent) */
  int32_t max_pairs;                      /* workspace sizing: pairs per call   */
  int32_t pipeline;                       /* args.pipeline (network/model.py:122,131): DSIR_PIPELINE_*; selects
                                           * which sub-networks exist, i.e. which state-dict keys are expected  */
} dsir_cfg;

#define DSIR_PIPELINE_ALIGN 0   /* feat_extractor + mlp_feat/att/proj + inlier_model (370 keys): the whole path  */
#define DSIR_PIPELINE_FEAT  1   /* feat_extractor + mlp_feat/att/proj: key-point descriptors (dsir_forward_pair)  */
#define DSIR_PIPELINE_LABEL 2   /* feat_extractor only: semantic head (dsir_forward_pair)                         */

/* ---- lifecycle ------------------------------------------------------------ */

/* Replaces Network.__init__ + .to(device) (network/model.py:119-195, test.py:609-611). */
int dsir_create(int device, const dsir_cfg* cfg, dsir_ctx** out);
/* The same with option flags (dsir_create is flags = 0; dsir_cfg itself does not grow).
 * DSIR_FLAG_PPF = args.use_ppf (network/RandLANet.py:251-254): both RandLA networks take the point-pair-feature input layer -
 * mlp_pre is conv 10 -> 12 on feat_grouping's code (:110-137) and level 0 takes 12 channels (the state dict's shapes follow:
 * mlp_pre.conv.weight [12,10,1,1], dilated_res_blocks.0.mlp1 / .mlp_skip 12 inputs).  cfg.feat_len is then the number of
 * columns of a point row: xyz, the normal, anything more is ignored; fewer than 6 is an error (the reference's assertion,
 * RandLANet.py:325 "feature dimension error").  Training: dsir_t_ppf_fwd / dsir_t_ppf_bwd (dsir_train.h) are the layer's taped
 * forward - the same bits as dsir_ppf_pre - and the backward of its four parameter tensors. */
#define DSIR_FLAG_PPF 1
int dsir_create_ex(int device, const dsir_cfg* cfg, int flags, dsir_ctx** out);
void dsir_destroy(dsir_ctx* ctx);
const char* dsir_last_error(const dsir_ctx* ctx);   /* ctx may be NULL: creation errors */
/* The HIP stream (hipStream_t) every call is ordered on. */
void* dsir_stream(dsir_ctx* ctx);
int dsir_sync(dsir_ctx* ctx);
/* Order every later call of this context on a CALLER-OWNED hipStream_t instead (restore_own != 0: back to the context's own
 * stream; a NULL hip_stream with restore_own == 0 is the legacy default stream, which is what torch's default stream is) - e.g.
 * the host framework's current stream, so that the engine's operators interleave with the caller's kernels without host
 * synchronisation and can be captured into the caller's hipGraph.  The context never destroys a caller's stream.  Work enqueued earlier stays
 * on the stream it was enqueued on, and the new stream WAITS for it on the device (an event recorded on the old stream): every
 * call of a context re-uses its one workspace arena, so launches on the new stream must not overtake the old stream's.  The
 * one exception is a stream under capture, which cannot wait on outside work: synchronise before the capture begins. */
int dsir_set_stream(dsir_ctx* ctx, void* hip_stream, int restore_own);
int dsir_num_weights(const dsir_ctx* ctx);
/* i-th expected state-dict key and its element count (for host-side validation). */
const char* dsir_weight_name(const dsir_ctx* ctx, int i, int64_t* numel);

/* Replaces Network.load_state_dict (test.py:614): called once per state-dict
 * key with a HOST fp32 pointer; the engine copies.  Unknown keys and shape
 * mismatches are errors (strict loading); '*.num_batches_tracked' is accepted
 * and ignored.  dsir_finalize_weights folds eval-mode BatchNorm1d into the
 * preceding Conv1d (RandLANet.py:34-55) and uploads everything; it fails if a
 * key is missing. */
int dsir_load_weight(dsir_ctx* ctx, const char* key, const float* host_data, const int64_t* shape, int ndim);
int dsir_finalize_weights(dsir_ctx* ctx);

/* ---- stage entry points (each mirrors one reference operator) ------------- */

/* torch int64 index tensor -> int32 (device to device). */
int dsir_narrow_i64(dsir_ctx* ctx, const int64_t* src, int32_t* dst, int64_t n);

/* Replaces DataBase.nn_search (dataloader/data_base.py:153-183) incl. the
 * third-party torch_points_kernels.knn: 4-level KNN pyramid of `clouds`
 * clouds of n points each.  points: [clouds][n][stride] fp32, xyz in the
 * first three columns.
 * Outputs (per cloud, levels concatenated; S = sum n_l, S1 = sum n_{l+1}):
 *   xyz_multi [clouds][S][3] f32, neigh_idx [clouds][S][16] i32,
 *   sub_idx [clouds][S1][16] i32, interp_idx [clouds][S] i32.
 * Tie rule: (fp32 squared distance, then lower index) — oracle/knn.py. */
int dsir_knn_pyramid(dsir_ctx* ctx, const float* points, int stride, int clouds, int n,
                     float* xyz_multi, int32_t* neigh_idx, int32_t* sub_idx, int32_t* interp_idx);

/* Replaces RandLA.forward (network/RandLANet.py:311-372).
 * which: 0 = feat_extractor (Cin = feat_len, num_classes logits),
 *        1 = inlier_model   (Cin = 6, 1 logit).
 * features [clouds][n][cin]; pyramids as produced by dsir_knn_pyramid.
 * Outputs: feat [clouds][n][64], logits [clouds][n][ncls] (either may be NULL). */
int dsir_randla_forward(dsir_ctx* ctx, int which, const float* features, int cin, int clouds, int n,
                        const float* xyz_multi, const int32_t* neigh_idx, const int32_t* sub_idx,
                        const int32_t* interp_idx, float* feat, float* logits);

/* Debug entry: lfa.mlp2 (RandLANet.py:186) of pyramid level `level` of network `which`, alone, by either of its two producers on
 * the per-point tables of lfa.mlp1: fused = 0 the row-streaming launch of its own, fused = 1 the producing variant of the block's
 * first attentive pooling (an error where that level's pooling has none).  Pyramids as produced by dsir_knn_pyramid.
 * Outputs: rows [clouds][16 n_level][d_out[level] / 2], the raw convolution outputs; stats [clouds][groups][4] doubles (groups = 8 from 64 channels up, else 4), the layer's
 * GroupNorm statistics as committed ({L1, L0} limbs of the sum, then of the sum of squares, per group).  The two producers must
 * agree in every bit of both. */
int dsir_lfa_enc2_probe(dsir_ctx* ctx, int which, int level, int fused, int clouds, int n, const float* xyz_multi,
                        const int32_t* neigh_idx, float* rows, double* stats);

/* Debug entry: mlp_feat of Network.aggregation (model.py:218) alone, feat0 [clouds][n][64] -> out [clouds][n][64], by either of
 * its forms: fused = 0 the three point-wise launches, fused = 1 the one launch of csrc/feat_chain.hip, fused = 2 that launch on
 * both halves of the clouds at once with two output bases, as a registration runs its src and ref sides (clouds even).  An
 * error where the fused launch does not take the configuration.  max_workgroups > 0 caps the fused launch's grid, so that a wave
 * walks several row tiles at sizes a test can afford (0: the launch's own grid).  The forms must agree in every bit. */
int dsir_mlp_feat_probe(dsir_ctx* ctx, const float* feat0, int clouds, int n, int fused, int max_workgroups, float* out);

/* Under DSIR_FLAG_PPF dsir_randla_forward takes rows of cin >= 6 columns (xyz, normal) for either network (the reference's
 * inlier model is handed [moved src xyz ; matched ref xyz] there, model.py:574-577: its "normals" are the matched points),
 * and dsir_forward_pair / dsir_register read points_src / points_ref as rows of feat_len columns with the normal in 3 .. 5.
 *
 * dsir_ppf_pre replaces the use_ppf front end of RandLA.forward alone (network/RandLANet.py:324-332: feat_grouping :110-137 with
 * matchnet.py:11-30 angle, mlp_pre, mean over the neighbours).  which as above; rows [clouds][n][stride] (stride >= 6: xyz,
 * normal); neigh_idx = the level-0 rows of the pyramid, neigh_cloud_stride ints between clouds -> out [clouds][n][12], the
 * input of dilated_res_blocks[0].  Needs a DSIR_FLAG_PPF context.  Same bytes on every run; clouds are independent, bit for bit. */
int dsir_ppf_pre(dsir_ctx* ctx, int which, const float* rows, int stride, const int32_t* neigh_idx, int64_t neigh_cloud_stride,
                 int clouds, int n, float* out);

/* Normals for the rows above where the data has none (the reference's 3DMatch / KITTI loaders; it would call open3d's
 * estimate_normals, which is unpinned here: the rule is this engine's own, stated in csrc/ppf.hip and restated in
 * deepsir_amd/ppf.py).  Per point: the 16 level-0 neighbours (self included), fp64 mean and covariance in list order, the
 * eigenvector of the smallest eigenvalue, normalised in fp64, oriented towards the viewpoint (n . (v - p) >= 0; exactly 0: largest
 * component positive, ties to the lower axis), rounded to fp32 once.  points [clouds][n][stride] (xyz first); neigh_idx /
 * neigh_cloud_stride as for dsir_ppf_pre; viewpoint = HOST float[3] or NULL (the origin) -> normals [clouds][n][3], flags
 * [clouds][n] i32 or NULL (1: degenerate - all neighbours coincide or a value is not finite - normal (0,0,0); not an error:
 * angle() of a zero vector is 0, matchnet.py:16).  Any context serves. */
int dsir_estimate_normals(dsir_ctx* ctx, const float* points, int stride, const int32_t* neigh_idx, int64_t neigh_cloud_stride,
                          int clouds, int n, const float* viewpoint, float* normals, int32_t* flags);
/* The same normals from a CSR neighbour list in place of the fixed 16 (open3d's estimate_normals over KDTreeSearchParamRadius /
 * Hybrid): csr_offsets [clouds * n + 1] / csr_cols with cloud-local columns, the form dsir_fpfh takes and dsir_t_nn_radius_fill
 * (include/dsir_train.h) writes; offsets must be non-decreasing and stay inside csr_cols, columns are clamped into the cloud.  The
 * arithmetic is dsir_estimate_normals' over the entries of the row in row order, the mean's divisor the row's length; a row of
 * fewer than 3 entries gets flag 1 and a zero normal like any degenerate neighbourhood.  On a CSR that lists the 16 level-0
 * neighbours in list order the two entries write the same bytes. */
int dsir_estimate_normals_csr(dsir_ctx* ctx, const float* points, int stride, const int32_t* csr_offsets, const int32_t* csr_cols,
                              int clouds, int n, const float* viewpoint, float* normals, int32_t* flags);

/* FPFH descriptors (the classical feature of open3d's compute_fpfh_feature -> registration_ransac_based_on_feature_matching
 * baseline, unpinned here: the rule is this engine's own, stated in csrc/fpfh.hip and restated in deepsir_amd/fpfh.py) from
 * points, normals and neighbour lists, all float64 on the fp32 inputs.  points [clouds][n][stride] (xyz first); normals
 * [clouds][n][3], or NULL: columns 3..5 of the rows, which needs stride >= 6.  Exactly one list form:
 *   neigh_idx / neigh_cloud_stride  the fixed 16 entries per point of dsir_estimate_normals (the pyramid's level-0 rows), or
 *   csr_offsets [clouds * n + 1] / csr_cols  a CSR list with cloud-local columns, the layout of dsir_t_radius_matches_fill for
 *                                            src == ref; offsets must be non-decreasing and stay inside csr_cols.
 * Neighbour indices are clamped into the cloud.  -> desc [clouds][n][out_ld] (out_ld >= 33: 33 values, then +0; out_ld = 64 feeds
 * dsir_feature_correspondences, whose squared distances the zero columns leave unchanged), flags [clouds][n] i32 or NULL (1: the
 * point has no valid pair, its row is all zeros; not an error).  Scratch: 34 ints per point from the context's workspace; a cloud
 * set that does not fit is refused before any launch.  Same bytes on every run; clouds are independent, bit for bit.  Any
 * context serves (no weights needed). */
int dsir_fpfh(dsir_ctx* ctx, const float* points, int stride, const float* normals, const int32_t* neigh_idx,
              int64_t neigh_cloud_stride, const int32_t* csr_offsets, const int32_t* csr_cols, int clouds, int n, float* desc,
              int out_ld, int32_t* flags);

/* ISS keypoints (intrinsic shape signatures; open3d's compute_iss_keypoints, unpinned here: the rule is this engine's own, stated in
 * csrc/iss.hip and restated in deepsir_amd/iss.py).  points [clouds][n][stride] (xyz first); two CSR lists with cloud-local columns,
 * self included, in the layout dsir_fpfh takes (offsets [clouds * n + 1], non-decreasing and inside cols; columns are clamped into
 * the cloud): the salient neighbourhoods (stage 1) and the non-maximum-suppression neighbourhoods (stage 2).  Stage 1: a row of
 * fewer than min_neighbors entries, a covariance that is not finite or all zero, or eigenvalues e1 >= e2 >= e3 of the fp64
 * covariance that fail e2 / e1 < gamma_21 or e3 / e2 < gamma_32 give saliency 0, else (float)e3.  Stage 2: a point is a keypoint iff
 * its saliency is > 0, its non-max row has at least min_neighbors entries, and no entry of that row has a larger saliency, or an
 * equal one and a lower index (exact duplicates yield one keypoint, where open3d keeps both).  -> saliency [clouds][n] f32, mask
 * [clouds][n] i32, index [clouds][n] i32 (the cloud's keypoints ascending, then -1), counts [clouds] i32.  Refused with a message,
 * launching nothing: a null pointer, clouds < 1, n < 1, stride < 3, a gamma that is not finite and positive, min_neighbors < 1.
 * No atomics: same bytes on every run; clouds are independent, bit for bit.  Any context serves (no weights needed). */
int dsir_iss_keypoints(dsir_ctx* ctx, const float* points, int stride, const int32_t* sal_offsets, const int32_t* sal_cols,
                       const int32_t* nms_offsets, const int32_t* nms_cols, int clouds, int n, double gamma_21, double gamma_32,
                       int min_neighbors, float* saliency, int32_t* mask, int32_t* index, int32_t* counts);

/* Farthest-point sampling of a batch of clouds: what dataloader/data_base.py:328 (farthest_point_sampler) does on the host and
 * network/tools.py:30 (farthest_point_sample) with a loop of torch ops, and open3d's farthest_point_down_sample (unpinned here: the
 * rule is this engine's own, stated in csrc/fps.hip and restated in deepsir_amd/fps.py).  points [clouds][cap][stride] (xyz first);
 * counts [clouds] on the device or NULL: cloud c has clamp(counts[c], 0, cap) rows (NULL: cap), rows at and past it are never read.
 * s_0 = start if that row exists and is finite, else the lowest finite row; then, k - 1 times, every remaining candidate's
 * dist = min(dist, d2 to the row chosen last) from +inf - fp32, d2 = (dx dx + dy dy) + dz dz - and the candidate of largest dist is
 * chosen, ties to the lower index.  A row with a non-finite coordinate is never chosen, a chosen row never again; a cloud that runs
 * out of candidates ends early.  -> index [clouds][k] i32 in selection order (-1 beyond the cloud's count), counts_out [clouds] i32,
 * min_d2 [clouds][k] f32: the dist of each chosen row when it was chosen (+inf for s_0, 0 beyond the count), non-increasing.
 * One workgroup per cloud, the k steps inside one launch.  Refused with a message, launching nothing: a null pointer (counts may be
 * NULL), clouds outside [1, 65535], cap < 1, stride < 3, k < 1 or k > cap, start < 0, cap > 65536, a workspace too small.
 * No atomics: same bytes on every run; clouds are independent, bit for bit.  Any context serves (no weights needed). */
int dsir_farthest_point_sample(dsir_ctx* ctx, const float* points, int stride, const int32_t* counts, int clouds, int cap, int k, int start,
                               int32_t* index, int32_t* counts_out, float* min_d2);

/* RANSAC plane segmentation of a batch of clouds, up to max_planes planes peeled per cloud in one call: what open3d's segment_plane
 * and PCL's SACSegmentation do in front of a lidar registration (unpinned here: the rule is this engine's own, stated in
 * csrc/plane.hip and restated in deepsir_amd/plane.py).  points [clouds][cap][stride] (xyz first); counts [clouds] on the device or
 * NULL: cloud c has clamp(counts[c], 0, cap) rows (NULL: cap), rows at and past it are never read; cloud_ids [clouds] on the device or
 * NULL: the id that enters cloud c's draws (NULL: c), so that cloud c of a batch is cloud 0 of a call with seed ^ (c << 40).
 * Per round j: `hypotheses` keyed draws of three live rows, an fp64 fit (normal, anchor) rounded to fp32 once, the fp32 residual
 * e = ((nx (x - ax)) + (ny (y - ay))) + (nz (z - az)) with |e| < distance_threshold counted over the live rows, the largest count
 * wins (ties to the lower hypothesis), refine_iters refits through the fp64 covariance of the inliers kept while the count does not
 * drop; the inliers get labels = j and leave.  A cloud is finished when no hypothesis is valid or the winner counts fewer than
 * min_inliers.  axis_x/y/z: a unit vector, all zero for none; with one a plane is accepted only if |n . axis| >= cos_min.
 * -> labels [clouds][cap] i32 (-1: no plane), num_planes [clouds] i32, planes [clouds][max_planes][4] f32 (nx, ny, nz, d with
 * n . p + d = 0; oriented n . axis >= 0, or d >= 0 without an axis), anchors [clouds][max_planes][3] f32, plane_counts
 * [clouds][max_planes] i32, stats [clouds][max_planes][4] i32 = {winning hypothesis, valid hypotheses, count before the refits,
 * refits kept}; rows at and behind num_planes are 0.  Refused with a message, launching nothing: a null pointer (counts and
 * cloud_ids may be NULL), clouds outside [1, 65535], cap < 1 or clouds x cap >= 2^31, stride < 3, hypotheses outside [1, 2^20],
 * distance_threshold not finite and positive, max_planes outside [1, 8], min_inliers < 3, refine_iters outside [0, 8], a non-finite
 * axis or cos_min, a workspace too small.  Integer atomics only: same bytes on every run; clouds are independent, bit for bit.
 * Any context serves (no weights needed). */
int dsir_segment_plane(dsir_ctx* ctx, const float* points, int stride, const int32_t* counts, const int32_t* cloud_ids, int clouds, int cap,
                       float distance_threshold, int hypotheses, int max_planes, int min_inliers, int refine_iters, float axis_x,
                       float axis_y, float axis_z, double cos_min, uint64_t seed, int32_t* labels, int32_t* num_planes, float* planes,
                       float* anchors, int32_t* plane_counts, int32_t* stats);

/* Replaces torch.max(logits,1) + Network.feat_score/score_fun with num_sub<=0
 * (network/model.py:638-644, :668-757).
 * feat [clouds][n][64], logits [clouds][n][ncls], xyz [clouds][n][3],
 * neigh_idx = level-0 rows of the pyramid with row stride `neigh_stride` ints
 * between clouds.  Outputs: score [clouds][n] f32, label [clouds][n] i32 (may be NULL). */
int dsir_score(dsir_ctx* ctx, const float* feat, const float* logits, const float* xyz, int64_t xyz_cloud_stride,
               const int32_t* neigh_idx, int64_t neigh_cloud_stride, int clouds, int n, float* score, int32_t* label);

/* Replaces one cloud's half of Network.aggregation (network/model.py:209-235):
 * desc = normalize(mlp_proj(mlp_feat(feat0) + mlp_att([xyz; score]))).
 * xyz [clouds][n][3], feat0 [clouds][n][64], score [clouds][n] -> desc [clouds][n][64]. */
int dsir_aggregate(dsir_ctx* ctx, const float* xyz, int64_t xyz_cloud_stride, const float* feat0, const float* score,
                   int clouds, int n, float* desc);

/* Replaces match_features_V2 + min(dim=2)[1] incl. the 6000-row chunking
 * (network/matchnet.py:96-144, network/model.py:558-569): for every src
 * descriptor the index of the nearest ref descriptor, distance evaluated as
 * fp32 ((-2 a.b) + |a|^2) + |b|^2, ties to the lower index.
 * desc_src [pairs][J][64], desc_ref [pairs][K][64] -> idx [pairs][J] i32. */
int dsir_nn_match(dsir_ctx* ctx, const float* desc_src, const float* desc_ref, int pairs, int J, int K, int32_t* idx);

/* The same arg-min as dsir_nn_match, bit for bit, the way dsir_register computes it: columns are first discarded by an
 * fp16-split MFMA screening with a rigorous error bound, the exact fp32 formula then decides among the survivors
 * (csrc/nn_screen.hip); rows the screening cannot decide are searched by the exhaustive fp32 kernel of dsir_nn_match.
 * Any finite input gives the exact result: components outside the screening's domain (|x| > 16) or not finite switch the whole
 * call to the exhaustive kernel.
 * stats (HOST, optional): [0] = candidate entries emitted by the screening, [1] = rows left to the exhaustive kernel. */
int dsir_nn_match_screened(dsir_ctx* ctx, const float* desc_src, const float* desc_ref, int pairs, int J, int K,
                           int32_t* idx, int64_t* stats);

/* Replaces compute_rigid_transform_2 (network/model.py:22-66): weighted
 * Kabsch with fp64 3x3 SVD on device.  src/tgt [pairs][m][3], w [pairs][m]
 * -> T [pairs][3][4] f32, invalid [pairs] i32 (1 = non-finite covariance,
 * identity returned). */
int dsir_kabsch(dsir_ctx* ctx, const float* src, const float* tgt, const float* w, int pairs, int m,
                float* T, int32_t* invalid);

/* ---- the whole path -------------------------------------------------------- */

typedef struct dsir_pair_batch {
  int32_t pairs;                 /* P */
  int32_t n_src, n_ref;          /* J, K points per cloud */
  const float* points_src;       /* [P][J][feat_len] */
  const float* points_ref;       /* [P][K][feat_len] */
  /* Optional caller-supplied pyramids (reference data dict keys
   * points_{src,ref}_{xyz,neigh_idx,sub_idx,interp_idx}, data_base.py:178-181),
   * already int32.  All NULL => built on device (dsir_knn_pyramid). */
  const float* src_xyz;   const int32_t* src_neigh;   const int32_t* src_sub;   const int32_t* src_interp;
  const float* ref_xyz;   const int32_t* ref_neigh;   const int32_t* ref_sub;   const int32_t* ref_interp;
  /* Optional teacher forcing (tests): correspondences per iteration [n_iter][P][J] i32.
   * Caller-supplied indices (these and the pyramids) are clamped into their valid range on device, so a bad index
   * can never fault a gather; the pair's invalid flag then carries bit 1 (value 2). */
  const int32_t* forced_idx;
} dsir_pair_batch;

typedef struct dsir_pair_result {
  float* transforms;     /* [P][n_iter][3][4] cumulative src->ref (model.py:595)        required */
  int32_t* idx;          /* [n_iter][P][J] arg-min correspondences (pred_pairs[...,1])   or NULL  */
  float* logits;         /* [n_iter][P][J] inlier logits (endpoints['perm_matrices'])    or NULL  */
  float* pt_ref_new;     /* [P][J][3] matched ref points of the last iteration           or NULL  */
  int32_t* invalid;      /* [P] OR over iterations: bit 0 = non-finite Kabsch covariance, identity returned
                          *     (endpoints['invalid_gradient'], model.py:61-64; also the outcome of a non-finite
                          *     input point: that pair alone, the other pairs of the batch are unaffected);
                          *     bit 1 = a caller-supplied index was out of range and clamped       or NULL  */
  /* test aids (parity of the arg-min on the engine's OWN descriptors, tests/test_gpu_large_configs.py): the aggregated,
   * L2-normalised descriptors Network.aggregation returns (model.py:552) as the search of each iteration saw them */
  float* desc_src;       /* [n_iter][P][J][64]                                                    or NULL  */
  float* desc_ref;       /* [P][K][64] (loop invariant)                                           or NULL  */
} dsir_pair_result;

/* Replaces Network.forward -> forward_align_4 (network/model.py:297-298,
 * :520-607) for P independent pairs in one call: KNN pyramids (if not
 * supplied), 2x feature RandLA + score, then n_iter x {aggregation, NN match,
 * inlier RandLA, weighted Kabsch, SE(3) update}. */
int dsir_register(dsir_ctx* ctx, const dsir_pair_batch* in, int n_iter, const dsir_pair_result* out);

/* ---- the `feat` / `label` pipelines of the same Network ---- */

typedef struct dsir_cloud_out {   /* one side (src or ref) of endpoints, point-major; M = num_sub > 0 ? num_sub : N */
  float* xyz;       /* [P][M][3]   endpoints['pt_*']                                                   or NULL */
  float* feat;      /* [P][M][64]  endpoints['feat_*'] (ALIGN ctx: raw feat0 of forward_pair's 8-tuple)  or NULL */
  float* logits;    /* [P][N][num_classes] endpoints['logits_*'] (always all N points)                 or NULL */
  float* score;     /* [P][M] endpoints['score_*'] (descending when num_sub > 0); not for LABEL        or NULL */
  int32_t* label;   /* [P][M] arg-max class of the (selected) points; not for LABEL                    or NULL */
  int32_t* index;   /* [P][M] selected point indices (only when num_sub > 0)                           or NULL */
} dsir_cloud_out;

/* Replaces Network.forward -> forward_pair (network/model.py:609-666) incl. feat_score's top-num_sub key-point
 * selection (:682-697, torch.topk; equal scores are taken in ascending index here) for P pairs:
 *   LABEL ctx: feat = normalize(feat_extractor features), logits.
 *   FEAT  ctx: score -> optional top-num_sub -> aggregation (:209-235) -> normalize (:650-651), logits, score.
 *   ALIGN ctx: forward_pair as forward_align_4 calls it (return_flag, :646-648): raw feat0, xyz, label, score;
 *              num_sub must be <= 0 (the inlier model needs the full pyramid, :575).
 * The KNN pyramids are built on device unless supplied in `in`. */
int dsir_forward_pair(dsir_ctx* ctx, const dsir_pair_batch* in, int num_sub, const dsir_cloud_out* src,
                      const dsir_cloud_out* ref);

/* ---- in front of the path: pre-processing ----------- */

/* Replaces the range/height crop of process_point_cloud (dataloader/data_base.py:299-312) and open3d's
 * voxel_down_sample as called at dataloader/threeDMatch_loader.py:168-175 / kitti_loader.py:335-338, for a
 * RAGGED batch: points [total][stride] (xyz first, every channel is voxel-averaged), offsets = HOST array
 * [clouds+1] of row offsets, crop = HOST [r_min, r_max, z_min, z_max] or NULL.
 * out [clouds][cap][stride] (voxels in ascending (ix,iy,iz) order; rows beyond cap are dropped),
 * counts [clouds] i32 on device = number of voxels of every cloud (may exceed cap: caller's overflow check).
 * 1 to 1000 clouds per call; a cloud may be empty, and a cloud the crop empties has count 0.  A voxel index has 18 bits
 * per axis: a point that survives the crop with an index outside [0, 2^18) on some axis (an extent of 2^18 voxels or
 * more, one stray far point) or with a coordinate that is not finite is neither dropped nor aliased - the call fails,
 * the error names the cloud and the cloud-local row, and counts / out are unspecified.  (With a crop such a coordinate
 * never survives: NaN and inf fail the crop's comparisons.)
 * The output order / arithmetic rule is this engine's own (open3d is unpinned): oracle/preprocess.py. */
int dsir_voxel_downsample(dsir_ctx* ctx, const float* points, const int64_t* offsets, int clouds, int stride,
                          float voxel_size, const float* crop, int cap, float* out, int32_t* counts);

/* Replaces Resampler._resample (mode 0: seeded random order, no repeats while points last, then draws with
 * replacement) and FixedResampler._resample (mode 1: tile / prefix) of dataloader/transformation.py:72-93.
 * in [clouds][cap][stride] with counts [clouds] (device, as written by dsir_voxel_downsample)
 * -> out [clouds][k][stride].  The random order makes the prefix sub-sampling of the pyramid a random sample. */
int dsir_resample(dsir_ctx* ctx, const float* in, const int32_t* counts, int clouds, int cap, int stride, int k,
                  int mode, uint64_t seed, float* out);

/* ---- after the path: evaluation metrics ------------- */

/* Replaces common/metrics_util.py:27-85 compute_metrics as called per iteration by test.py:308-355
 * evaluate_align.  pred_T: [pairs] transforms of 12 floats each, `pred_stride` floats apart (so one
 * iteration of a [P][n_iter][3][4] result can be addressed in place); gt_T [pairs][3][4];
 * points_src / points_ref [pairs][n][stride] (xyz first; the first min(n,2048) points are used).
 * out [pairs][8] float64: r_mse, r_mae, t_mse, t_mae, err_r_deg, err_t, succ (0/1), chamfer_dist. */
int dsir_eval_metrics(dsir_ctx* ctx, const float* pred_T, int64_t pred_stride, const float* gt_T,
                      const float* points_src, const float* points_ref, int pairs, int n, int stride,
                      float rte_thresh, float rre_thresh, double* out);

/* ---- after the path: pose refinement --------------- */

/* Replaces the `use_icp` branch of pose_optimization (test.py:241-258): open3d
 *   registration_icp(src, tgt, max_correspondence_distance, T_init, TransformationEstimationPointToPoint(),
 *                    ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration))
 * for P pairs at once, entirely on device.  points_src [P][J][stride], points_ref [P][K][stride] (xyz first);
 * T_init / T_out [P][3][4]; stats [P][4] float64 {fitness, inlier_rmse, converged (0/1), iterations} or NULL.
 * The branch is disabled in the reference and open3d is not pinned: the rule (open3d's RegistrationICP loop, exact
 * brute-force nearest neighbours in fp32 with ties to the lower index) is restated in oracle/icp.py.
 * max_iter == 0 returns the first search's {fitness, rmse} with T_out = T_init, converged = 0, iterations = 0; converged = 0
 * also when max_iter updates were made without meeting the criteria.  No correspondence: the update is the identity.
 * Pairs are independent: a pair's T_out and stats do not depend, bit for bit, on the other pairs of the call.
 * Non-finite coordinates (not an error): such a point is never part of a correspondence; a pair that holds one in
 * points_src, or in a reference point that an update gathers, takes identity updates from then on, so its T_out stays a
 * finite rotation and translation and its stats stay finite; the other pairs are not affected. */
int dsir_icp_refine(dsir_ctx* ctx, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                    float max_corr_dist, int max_iter, float rel_fitness, float rel_rmse, const float* T_init,
                    float* T_out, double* stats);

/* dsir_icp_refine with the transformation estimator chosen: estimator 0 = point-to-point (open3d's
 * TransformationEstimationPointToPoint: byte for byte what dsir_icp_refine writes), 1 = point-to-plane (open3d's
 * TransformationEstimationPointToPlane; open3d is not pinned, so parity is unpinned: the rule is this engine's own, stated in the
 * header of csrc/icp.hip and restated in tests/icp_plane_host.py).  Arguments as for dsir_icp_refine, plus
 *   normals_ref [P][K][3] (device) or NULL.  Estimator 1 with NULL reads the normals from columns 3..5 of the points_ref rows
 *               (the use_ppf row layout), which requires stride >= 6: NULL with stride < 6 is "bad arguments".  Estimator 0
 *               does not read them.
 *   stats       [P][5] float64 or NULL: the four values of dsir_icp_refine, then the number of identity updates taken for a
 *               singular system (always 0 with estimator 0).
 * The loop - first search, fitness, inlier RMSE from point distances, convergence test, max_iter - is dsir_icp_refine's; only
 * the update differs: with r = (s - t) . n and J = [s x n ; n] over the correspondences (s moved source point, t target point,
 * n target normal), A = sum J J^T and b = sum J r in fp64, A x = -b solved in fp64, update R = Rz(x2) Ry(x1) Rx(x0),
 * t = (x3, x4, x5), applied and composed onto T as the Kabsch step's transform is.  Corner cases of estimator 1 (none is an error):
 *   singular system   with fewer than 6 contributing correspondences, or a singular system, the update is the identity and
 *                     is counted in stats[4].  Singular = LDL^T without pivoting of A scaled to unit diagonal meets a pivot
 *                     below 1e-10 (csrc/icp_plane.h gives the reason for the value); a zero diagonal entry is singular.  A
 *                     planar target (all normals parallel) is the plain example: T_out = T_init.
 *   zero normal       (dsir_estimate_normals' degenerate output) the correspondence contributes nothing.
 *   non-finite        a non-finite normal or reference coordinate takes that correspondence out of the update (fitness and
 *                     RMSE are the search's, as ever).  A pair with a non-finite source point takes identity updates from
 *                     then on (counted in stats[4]), so its T_out stays a finite rigid transform; other pairs are untouched.
 * Same bytes on every run (fixed partition of the sums, no floating-point atomics); pairs are independent, bit for bit. */
int dsir_icp_refine_ex(dsir_ctx* ctx, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                       float max_corr_dist, int max_iter, float rel_fitness, float rel_rmse, const float* T_init,
                       float* T_out, int estimator, const float* normals_ref, double* stats);

/* dsir_icp_refine_ex with the nearest-neighbour search chosen: search 0 = exact brute force (byte for byte what
 * dsir_icp_refine_ex writes), 1 = a sparse cell index of the reference cloud, built once per call on the device and searched by
 * every iteration (csrc/icp_grid.hip).  The rule is the same - d2 = (dx dx + dy dy) + dz dz in fp32, the smallest d2 with ties to
 * the lower index, accepted iff d2 <= fl(r r) - and both searches return the same index and the same d2 bits, so T_out and stats
 * are byte for byte those of search 0: the choice changes time only (J x K distance evaluations per search against a few hundred
 * per query).  Arguments as for dsir_icp_refine_ex, `search` before `stats`.  No extent is refused: a pair whose reference box is
 * more than 2^20 cells of the radius wide gets coarser cells.  search 1 with a max_corr_dist whose fp32 square is not finite, or with
 * P x J or P x K of 2^31 and more, is "bad arguments".  The index, the query order and the sort's temporary storage come from the
 * context workspace: "workspace too small" says to raise max_points / max_pairs. */
int dsir_icp_refine_ex2(dsir_ctx* ctx, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                        float max_corr_dist, int max_iter, float rel_fitness, float rel_rmse, const float* T_init,
                        float* T_out, int estimator, const float* normals_ref, int search, double* stats);

/* One search step of the loop under pose T [P][3][4]: open3d's evaluate_registration(src, tgt, max_correspondence_distance, T).
 * idx_out [P][J] int32: the reference point of source point j moved by T, or -1 where none lies within max_corr_dist;
 * d2_out [P][J] fp32: its squared distance, 0 where idx is -1; stats_out [P][2] float64 {fitness = matched / J, inlier_rmse =
 * sqrt(sum d2 / matched), 0 without a match} or NULL.  search as for dsir_icp_refine_ex2: both values write the same bytes. */
int dsir_icp_correspondences(dsir_ctx* ctx, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                             float max_corr_dist, const float* T, int search, int32_t* idx_out, float* d2_out, double* stats_out);

/* ICP on batches of clouds of unequal sizes: dsir_icp_refine_ex2 and dsir_icp_correspondences (and, further down,
 * dsir_information_matrix) with per-pair row counts.  counts_src, counts_ref: [P] int32 on the device, or NULL.  J and K are then
 * the row CAPACITIES of the arrays (their strides: points_src [P][J][stride], points_ref [P][K][stride], with estimator 1
 * normals_ref [P][K][3], idx_out / d2_out [P][J]) and pair p has
 *     Jp = clamp(counts_src[p], 0, J) source rows  and  Kp = clamp(counts_ref[p], 0, K) reference rows:
 * a count outside the capacity is clamped, not refused.  One count NULL: that side is full (J or K) in every pair.  Both NULL:
 * exactly the bytes of the entry that is extended, from the same launches.
 * Padding is never read into a result: rows of points_src at or beyond Jp, rows of points_ref and normals_ref at or beyond Kp may
 * hold anything - NaN, inf, or finite points that would be perfectly good queries and neighbours - and nothing that is written
 * depends on them.  Entries [Jp, J) of idx_out and d2_out are written as -1 and 0.f.  fitness = matched / Jp.
 * The contract: pair p of a call with counts gets the T_out, the stats, the information matrix and count, and the first Jp
 * entries of idx_out and d2_out, that the dense entry writes for that pair ALONE with J = Jp and K = Kp on its first Jp and Kp
 * rows - byte for byte, for both estimators and both searches.  (The sums are partitioned by the pair's own Jp, the brute search's
 * arg-min does not depend on its slices, the cell index sorts padding behind the pair's own rows with stable sorts, and the two
 * single-workgroup Kabsch kernels give the same bits, so nothing depends on the capacity.)
 * Jp == 0 or Kp == 0 (not an error; the dense entries refuse J or K of 0, so there is no dense counterpart): the pair has no
 * correspondence and is treated as such a pair always is - every update is the identity, T_out = T_init bit for bit, fitness and
 * inlier_rmse are 0 (fitness is defined as 0 for Jp == 0), the convergence test freezes it at the first iteration, all stats are
 * finite (estimator 1 counts that identity update in stats[4]), the information matrix is zero with count 0.
 * The scratch is sized by the capacities: "workspace too small" compares P x J and P x K, as in the dense entries.  Same bytes on
 * every run, and a pair's bytes do not depend on the other pairs of the call, their counts included. */
int dsir_icp_refine_ex3(dsir_ctx* ctx, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                        float max_corr_dist, int max_iter, float rel_fitness, float rel_rmse, const float* T_init,
                        float* T_out, int estimator, const float* normals_ref, int search, double* stats,
                        const int32_t* counts_src, const int32_t* counts_ref);
int dsir_icp_correspondences_ex(dsir_ctx* ctx, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                                float max_corr_dist, const float* T, int search, int32_t* idx_out, float* d2_out, double* stats_out,
                                const int32_t* counts_src, const int32_t* counts_ref);

/* dsir_icp_refine_ex3 with a robust loss kernel of the estimator: open3d's `robust_kernel` argument of
 * TransformationEstimationPointToPoint / PointToPlane (open3d is not pinned: the rule is this engine's own, csrc/icp_robust.h and
 * the header of csrc/icp.hip, restated in tests/icp_robust_host.py).  Arguments as for dsir_icp_refine_ex3, then
 *   kernel        DSIR_ICP_L2 .. DSIR_ICP_TUKEY;  kernel_scale  k > 0, finite, in the cloud's length unit (not read under l2).
 * The weight of a correspondence, from its squared residual q and k, in fp64, every operation rounded once in the order written:
 *   l2 1;  huber q <= k^2 ? 1 : k / sqrt(q);  cauchy 1 / (1 + q / k^2);  gm k / ((k + q) * (k + q)) (open3d's GMLoss);
 *   tukey q <= k^2 ? (1 - q / k^2)^2 : 0.        (open3d's L1Loss is left out: its weight is unbounded at an exact partner.)
 * estimator 0: q = the fp32 squared distance of the correspondence; the weight, rounded once to fp32, is the correspondence's
 * weight in the weighted Kabsch update.  A pair whose weights are all 0 takes the identity update: T is carried over bit for bit.
 * estimator 1: q = r^2 of the fp64 plane residual; A = sum w J J^T, b = sum w J r; a correspondence of weight 0 is not a row, so
 * "fewer than 6 rows" and the singular-system rule (identity update, counted in stats[4]) apply to what is left.
 * The kernel acts on the update ALONE: the search, fitness, inlier_rmse (unweighted point distances), the convergence test,
 * max_iter, the stats columns - and dsir_information_matrix - do not see it.  kernel = DSIR_ICP_L2 writes, byte for byte, what
 * dsir_icp_refine_ex3 writes (the four older entries run the same path with it); huber with k >= max_corr_dist does too (every
 * weight is exactly 1; for estimator 1 given normals no longer than 1, so that |r| <= the point distance).  Same bytes on every run, for both values of `search`, and for a pair whatever else is in the batch,
 * the counts' padding included.  Refused before any launch, with the usual error code and message: a kernel outside 0..4, and
 * under a kernel other than l2 a scale that is 0, negative, NaN or infinite. */
#define DSIR_ICP_L2 0
#define DSIR_ICP_HUBER 1
#define DSIR_ICP_CAUCHY 2
#define DSIR_ICP_GM 3
#define DSIR_ICP_TUKEY 4
int dsir_icp_refine_ex4(dsir_ctx* ctx, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                        float max_corr_dist, int max_iter, float rel_fitness, float rel_rmse, const float* T_init,
                        float* T_out, int estimator, const float* normals_ref, int search, double* stats,
                        const int32_t* counts_src, const int32_t* counts_ref, int kernel, float kernel_scale);

/* NDT registration (the normal-distributions transform of PCL / Autoware / ndt_omp) for P pairs at once, entirely on device: the
 * correspondence-free refinement beside the ICP entries, for sparse scans on which a nearest neighbour is a point of the same
 * ring.  PCL is not pinned: the rule is this engine's own, stated in the header of csrc/ndt.hip and restated in numpy fp64 in
 * deepsir_amd/ndt.py.  The reference cloud becomes one Gaussian per occupied cell of edge `resolution`; every moved source point
 * is pulled towards the Gaussians of its own cell and, with neighbors = 7, of the six face-adjacent cells (neighbors = 1: the own
 * cell alone).  The step is iteratively reweighted Gauss-Newton on PCL's score (constants d1..d3 from outlier_ratio and
 * resolution), solved by the point-to-plane entry's 6 x 6 solve; no line search, monotone descent is not promised.
 *   points_src [P][J][stride], points_ref [P][K][stride] fp32 rows (xyz first); counts_src / counts_ref [P] int32 device arrays or
 *   NULL: the rows of each pair that hold points, clamped to [0, J] / [0, K], as for dsir_icp_refine_ex3 - rows beyond are never read;
 *   T_init / T_out [P][3][4];  resolution > 0 and finite, in the cloud's length unit;  max_iter >= 0;
 *   step_tol > 0 and finite: a pair is converged when the update's rotation vector is shorter than step_tol and its translation
 *   shorter than step_tol x resolution, or after an identity update;  outlier_ratio inside (0, 1) (PCL's default 0.55);
 *   stats [P][5] fp32 or NULL: mean likelihood score / Jp and matched fraction matched / Jp after the last move (0 for Jp == 0),
 *   converged, iterations run, identity updates.
 * The update is the identity (T and the moved points keep their bits; counted) when fewer than 6 visits contributed, the system is
 * singular (icp_plane.h), a moved source point is not finite, or Jp == 0 or Kp == 0.  A non-finite reference row is in no cell; a
 * cell of fewer than 6 points, or whose covariance has no positive finite largest eigenvalue, has no Gaussian.  max_iter = 0: T_out
 * is T_init bit for bit.  Same bytes on every run (no floating-point atomics, fixed partition of the sums), and pair p gets, byte
 * for byte, what the call on its first Jp and Kp rows alone writes, whatever else is in the batch.  Bad arguments - resolution or
 * step_tol not positive and finite, outlier_ratio outside (0, 1), neighbors not 1 or 7, shapes beyond the context's workspace -
 * return the usual error code and message before any launch.  Scratch comes from the context workspace (NdtLayout, csrc/ndt.h). */
int dsir_ndt_refine(dsir_ctx* ctx, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                    const int32_t* counts_src, const int32_t* counts_ref, const float* T_init, float resolution, int neighbors,
                    int max_iter, float step_tol, float outlier_ratio, float* T_out, float* stats);
/* The map dsir_ndt_refine builds of points_ref, for tests and for users who want it.  Device outputs:
 *   lattice_out [P][4] f64: origin (the per-axis minimum of the pair's finite rows; 0 without one) and cell edge
 *   h = max(resolution, longest extent / 2^20);   keys_out [P][K] u64: the pair's cell keys x | y << 21 | z << 42, ascending, ~0 for
 *   non-finite and padding rows (last);   index_out [P][K] i32: the original row of every sorted position (the sort is stable);
 *   records_out [P][K][10] f64: at the first sorted position of every valid cell (>= 6 points, positive finite largest eigenvalue)
 *   its mean (3), inverse regularised covariance B (6: 00 01 02 11 12 22; eigenvalues floored at 0.01 of the largest) and point
 *   count; zero everywhere else. */
int dsir_ndt_map(dsir_ctx* ctx, const float* points_ref, int pairs, int K, int stride, const int32_t* counts_ref, float resolution,
                 double* lattice_out, uint64_t* keys_out, int32_t* index_out, double* records_out);

/* Replaces the `use_tune` branch of pose_optimization (test.py:209-239): transformation_finetune (test.py:159-207) with
 * HighDimSmoothL1Loss (test.py:103-131) over the network's last correspondences, the pose re-parametrised as
 * network/DGR.py's Transformation (6-D rotation + translation, :60-132) and fitted by Adam (lr 0.1, ExponentialLR 0.999)
 * until the loss is below 1e-7, max_iter steps are done, or the relative loss change was below break_threshold_ratio
 * max_break_count times - for P pairs at once, each pair's whole optimisation inside one workgroup.
 * xyz_src / xyz_ref [P][m][3] MATCHED points (endpoints['pt_src'] and 'pt_ref_new' = dsir_pair_result.pt_ref_new);
 * weights [P][m] or NULL (unweighted mean); weights_are_logits != 0: sigmoid applied on the fly (perm_matrices[-1]);
 * T_init / T_out [P][3][4]; stats [P][3] float64 {iterations, loss, break_count} (opt_result) or NULL.
 * The branch is disabled in the reference (use_tune = False) and test.py / DGR.py cannot be imported offline (open3d):
 * the rule is restated with the same torch calls in oracle/finetune.py (parity unpinned).
 * stats.iterations is the reference's loop index of the last step: max_iter steps report max_iter - 1; stats.loss is the
 * loss before the last update.  Pairs are independent, bit for bit.
 * Weights that sum to zero (all zero, or logits so negative that the fp32 sigmoid is 0, e.g. -100) divide by zero as the
 * reference does: that pair's T_out and stats.loss are NaN, it runs all max_iter steps with break_count 0, and the other
 * pairs are not affected. */
int dsir_pose_finetune(dsir_ctx* ctx, const float* xyz_src, const float* xyz_ref, const float* weights, int weights_are_logits,
                       int pairs, int m, const float* T_init, float quantization_size, int max_iter, float break_threshold_ratio,
                       int max_break_count, float* T_out, double* stats);

/* Replaces open3d's registration_ransac_based_on_correspondence (network/DGR.py:26-36) as DGR.safeguard_registration uses it
 * (network/DGR.py:249-306: 80 000 iterations, threshold 2 x voxel size), and - after dsir_feature_correspondences - the
 * registration_ransac_based_on_feature_matching of network/DGR.py:7-24, for P pairs at once, entirely on device.
 * open3d cannot be imported here: parity at this boundary is UNPINNED.  The engine owns the rule; it is stated once in the header of
 * deepsir_amd/csrc/ransac.hip (and DESIGN.md section 8) and restated on the host in deepsir_amd/ransac.py, which the tests compare against.
 * points_src [P][J][stride], points_ref [P][K][stride] (xyz first); corr [P][M][2] (src index, ref index); counts [P] (device) live
 * rows per pair or NULL (all M).  Out-of-range indices of live rows are clamped and reported as bit 2 of invalid[p].
 * max_dist: inlier threshold; ransac_n in {3, 4}; edge_sim: open3d's edge-length similarity (<= 0: no check; DGR uses 0.9);
 * hypotheses in [1, DSIR_RANSAC_MAX_HYPOTHESES]; refine_iters in [0, DSIR_RANSAC_MAX_REFINE] refits on all inliers (default use: 2).
 * seed: hypothesis h of pair p draws from splitmix64(splitmix64(seed ^ (p << 40)) ^ (h << 8) ^ k) alone, so the same hypothesis is the
 * same sample for every P and H; pair p of a call is pair 0 of a call with seed ^ (p << 40).
 * T_init [P][3][4] or NULL (identity): returned for a pair without a valid hypothesis (stats {0, 0, -1, 0, 0}; not an error).
 * T_out [P][3][4]; stats [P][5] float64 {fitness = inliers / count, inlier RMSE, winning hypothesis or -1, valid hypotheses, inliers};
 * invalid [P].  Non-finite coordinates are never inliers and never sampled.  Pairs are independent, bit for bit; two runs write the
 * same bytes.  M, J, K <= max_points. */
#define DSIR_RANSAC_CHUNK 256               /* correspondences a scoring workgroup stages per step (tests place M around it) */
#define DSIR_RANSAC_MAX_HYPOTHESES (1 << 20)
#define DSIR_RANSAC_MAX_REFINE 8
/* test / measurement outputs of dsir_ransac_correspondence (all optional, device memory): the rows every hypothesis drew (-1 beyond
 * ransac_n), its fitted transform (zeros when the sample was rejected before the fit), its verdict and its inlier count */
typedef struct dsir_ransac_diag {
  int32_t* hyp_sample;   /* [P][H][4] */
  float* hyp_T;          /* [P][H][12] */
  int32_t* hyp_valid;    /* [P][H] */
  int32_t* hyp_count;    /* [P][H] */
} dsir_ransac_diag;
int dsir_ransac_correspondence(dsir_ctx* ctx, const float* points_src, const float* points_ref, int pairs, int J, int K,
                               int stride, const int32_t* corr, const int32_t* counts, int M, float max_dist, int ransac_n,
                               float edge_sim, int hypotheses, int refine_iters, uint64_t seed, const float* T_init, float* T_out,
                               double* stats, int32_t* invalid, const dsir_ransac_diag* diag /* NULL in production */);

/* Spatial-consensus pose from correspondences: the deterministic alternative to dsir_ransac_correspondence for correspondence sets
 * that are mostly wrong (hand-crafted descriptors: 90 % outliers and more), after the second-order spatial compatibility of SC2-PCR.
 * Neither the reference nor open3d has the stage: parity is UNPINNED, the engine owns the rule, stated once in the header of
 * deepsir_amd/csrc/consensus.hip (and DESIGN.md section 8) and restated on the host in deepsir_amd/consensus.py.
 * Same boundary as dsir_ransac_correspondence: points_src, points_ref, corr, counts, M, max_dist, T_init in; T_out, invalid and
 * stats [P][5] float64 {fitness, inlier RMSE, winning seed rank or -1, valid seeds, inliers} out; P pairs at once, no host round
 * trip, pairs independent bit for bit, two runs write the same bytes.  No seed and no random number anywhere.
 * compat_dist: two matches are compatible when the lengths |s_i - s_j| and |q_i - q_j| differ by less than it (<= 0: max_dist);
 * seeds in [1, DSIR_CONSENSUS_MAX_SEEDS] (default use: 64): candidate poses, from the rows of the largest second-order score;
 * members in [3, DSIR_CONSENSUS_MAX_MEMBERS] (default use: 32): rows each seed's pose is fitted to;
 * refine_iters in [0, DSIR_RANSAC_MAX_REFINE]: as for RANSAC.
 * M <= DSIR_CONSENSUS_MAX_M (the scores are int32: M^2 < 2^31; a row of second-order counts is held in LDS as uint16) and
 * M, J, K <= max_points.  The workspace holds the compatibility bit matrix, P x M x ceil(M / 64) x 8 bytes (M = 5000: 3.2 MB a pair),
 * plus P x (M x 48 + seeds x 56)-order scratch; a call that does not fit is refused, naming the needed and the available bytes. */
#define DSIR_CONSENSUS_MAX_SEEDS 256
#define DSIR_CONSENSUS_MAX_MEMBERS 128
#define DSIR_CONSENSUS_MAX_M 24576
/* test / measurement outputs of dsir_consensus_correspondence (all optional, device memory), W = ceil(M / 64) */
typedef struct dsir_consensus_diag {
  uint64_t* bits;        /* [P][M][W]: bit j % 64 of word j / 64 of row i is C[i][j] */
  int32_t* score;        /* [P][M] */
  int32_t* seed;         /* [P][seeds]: the row of seed rank r, or -1 */
  int32_t* seed_members; /* [P][seeds][members]: ascending rows, -1 padded */
  float* seed_T;         /* [P][seeds][12]: zeros for an invalid seed */
  int32_t* seed_valid;   /* [P][seeds] */
  int32_t* seed_count;   /* [P][seeds]: inliers of seed_T under max_dist */
} dsir_consensus_diag;
int dsir_consensus_correspondence(dsir_ctx* ctx, const float* points_src, const float* points_ref, int pairs, int J, int K,
                                  int stride, const int32_t* corr, const int32_t* counts, int M, float max_dist, float compat_dist,
                                  int seeds, int members, int refine_iters, const float* T_init, float* T_out, double* stats,
                                  int32_t* invalid, const dsir_consensus_diag* diag /* NULL in production */);

/* Fast global registration pose from correspondences (FGR: Zhou, Park, Koltun 2016; open3d's
 * registration_fgr_based_on_feature_matching): the third estimator behind the boundary of dsir_ransac_correspondence.  No hypotheses
 * and no quadratic memory: a tuple pre-filter, then `iterations` 6 x 6 Gauss-Newton steps under a graduated robust weight, O(rows x
 * iterations) per pair - for correspondence counts where consensus is refused for memory and RANSAC needs many hypotheses.
 * open3d cannot be imported here: parity is UNPINNED, the engine owns the rule, stated once in the header of
 * deepsir_amd/csrc/fgr.hip (and DESIGN.md section 8) and restated on the host in deepsir_amd/fgr.py.
 * Same boundary as dsir_ransac_correspondence: points_src, points_ref, corr, counts, M, max_dist, seed, T_init in; T_out, invalid and
 * stats [P][5] float64 {fitness, inlier RMSE, 0 or -1 (no pose), 1 or 0, inliers} out; P pairs at once, no host round trip, pairs
 * independent bit for bit, two runs write the same bytes; pair p of a call is pair 0 of a call with seed ^ (p << 40).
 * tuple_test != 0: min(100 x count, max_trials) keyed trials of three rows each; a trial whose three edges agree in length within
 * tuple_scale (in (0, 1], default use: 0.95) on both sides is accepted, and the rows of the first max_tuples accepted trials in trial
 * order (default use: 1000) are the optimisation's row list.  tuple_test == 0: every live finite row is listed (tuple_scale,
 * max_tuples, max_trials and seed are checked but unused).
 * iterations in [1, DSIR_FGR_MAX_ITERS] (default use: 64); division_factor (default use: 1.4; <= 1: the robust weight's mu stays 1);
 * refine_iters in [0, DSIR_RANSAC_MAX_REFINE]: as for RANSAC, on the optimised pose.
 * max_tuples in [1, DSIR_FGR_MAX_TUPLES] (a list of 3 x 65536 rows: 768 KiB of rows and 9 MiB of normalised points a pair),
 * max_trials in [1, DSIR_FGR_MAX_TRIALS] (pairs x max_trials stays below 2^31: the selection's positions are int32),
 * DSIR_FGR_MAX_ITERS bounds the per-iteration diagnostics.  M, J, K <= max_points.  The workspace holds P x (M x 28 + rows x 52)-order
 * scratch, rows = 3 x max_tuples (tuple_test == 0: M); a call that does not fit is refused, naming the needed and the available
 * bytes. */
#define DSIR_FGR_MAX_TUPLES 65536
#define DSIR_FGR_MAX_TRIALS (1 << 22)
#define DSIR_FGR_MAX_ITERS 1024
/* test / measurement outputs of dsir_fgr_correspondence (all optional, device memory), L = 3 x max_tuples (tuple_test == 0: M) */
typedef struct dsir_fgr_diag {
  int32_t* rows;         /* [P][L]: the row list, -1 padded */
  int32_t* n_rows;       /* [P]: rows in the list */
  int32_t* trials;       /* [P]: trials evaluated (tuple_test == 0: 0) */
  double* norm;          /* [P][8]: ms, mq, scale, 0 (zeros where the list has fewer than 3 rows) */
  double* iter_T;        /* [P][iterations][12]: T after the iteration, normalised frame; zeros for iterations that did not run */
  double* iter_mu;       /* [P][iterations]: the mu the iteration's weights used */
  double* iter_energy;   /* [P][iterations]: the energy at the iteration's start */
  int32_t* iters_run;    /* [P]: iterations completed; -(it + 1) when the solve refused at iteration it */
} dsir_fgr_diag;
int dsir_fgr_correspondence(dsir_ctx* ctx, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                            const int32_t* corr, const int32_t* counts, int M, float max_dist, int tuple_test, float tuple_scale,
                            int max_tuples, int max_trials, int iterations, float division_factor, int refine_iters, uint64_t seed,
                            const float* T_init, float* T_out, double* stats, int32_t* invalid,
                            const dsir_fgr_diag* diag /* NULL in production */);

/* The correspondence set open3d's registration_ransac_based_on_feature_matching (network/DGR.py:7-24; called at test.py:259-263)
 * draws from, made explicit (parity unpinned, as above): the exact descriptor arg-min of dsir_nn_match src -> ref, with mutual != 0
 * kept only where the ref -> src arg-min points back; survivors in ascending src index.  desc_src [P][J][64], desc_ref [P][K][64]
 * -> corr [P][J][2] (rows beyond counts[p] are -1), counts [P].  Same bytes on every run. */
int dsir_feature_correspondences(dsir_ctx* ctx, const float* desc_src, const float* desc_ref, int pairs, int J, int K, int mutual,
                                 int32_t* corr, int32_t* counts);

/* ---- the training slice (backward half) ------- */

/* Replaces ScanAlignmentLoss.forward with reduction='mean' (network/loss.py:705-851; defaults of arguments.py:51-61:
 * loss_type mae, wt_ptDist_loss 1, wt_inlier_loss 1, wt_pose_loss 0, loss_discount_factor 0.5; called at train.py:401;
 * wt_pose_loss > 0, the rotation + translation error term of loss.py:830-842: dsir_align_loss_backward3 below)
 * AND torch autograd's backward of it down to the inlier logits: through se3_torch.concatenate (model.py:595) and the
 * SVD of compute_rigid_transform_2 (model.py:22-66).  In forward_align_4 the matching runs under no_grad and the src
 * cloud is moved by R_t.detach(), so d total / d logits is the whole gradient the network receives from this loss: the
 * input of the inlier RandLA's backward pass (not built).
 * pt_src [P][J][3], pt_ref [P][K][3] (endpoints['pt_src'/'pt_ref']); idx [n_iter][P][J] i32 (pred_pairs[...,1]);
 * logits [n_iter][P][J] (perm_matrices); labels [n_iter][P][J] f32 0/1 = find_correct_correspondence(matches, pred_pairs)
 * (loss.py:723-749, host work in the reference too) or NULL = no confidence term; transform_gt [P][3][4].
 * loss_type 0 = mae, 1 = mse; wt_ptDist_loss only gates the point-distance term (> 0), as in the reference.
 * Outputs: transforms [P][n_iter][3][4] cumulative poses replayed from the logits (or NULL); losses = HOST float64
 * [n_iter][2] {mae_i | mse_i, outlier_i} (total = sum_i discount^(n_iter-1-i) (term_i + outlier_i)) or NULL;
 * grad_logits [n_iter][P][J] = d total / d logits.  n_iter <= 8.
 * dsir_align_loss_backward2: the same call with one more output, losses_per_pair = HOST float64 [P][n_iter][2] or NULL: every pair's own
 * terms as reduction='none' reports them (loss.py:779, :836: the mean over that pair's points / rows alone; validate_align, train.py:136). */
int dsir_align_loss_backward(dsir_ctx* ctx, const float* pt_src, const float* pt_ref, const int32_t* idx, const float* logits,
                             const float* labels, const float* transform_gt, int pairs, int J, int K, int n_iter, int loss_type,
                             float wt_ptDist_loss, float wt_inlier_loss, float loss_discount_factor, float* transforms,
                             double* losses, float* grad_logits);
int dsir_align_loss_backward2(dsir_ctx* ctx, const float* pt_src, const float* pt_ref, const int32_t* idx, const float* logits,
                              const float* labels, const float* transform_gt, int pairs, int J, int K, int n_iter, int loss_type,
                              float wt_ptDist_loss, float wt_inlier_loss, float loss_discount_factor, float* transforms,
                              double* losses, float* grad_logits, double* losses_per_pair);
/* dsir_align_loss_backward2 plus the pose-error term, float wt_pose_loss (finite, >= 0; 0 = the call above, same bits).  Per pair
 * and iteration, from the cumulative pose [Rc_i | tc_i] and the ground truth:
 *     s_i = (<R_gt, Rc_i>_F - 1) / 2,   err_r = acos(clamp(s_i, -1, 1)),   err_t = |t_gt - tc_i|_2
 *     poseError_i = (mean_pairs err_r + mean_pairs err_t) wt_pose_loss       (losses_per_pair: (err_r + err_t) wt_pose_loss)
 * losses = HOST float64 [n_iter][3], losses_per_pair = HOST float64 [P][n_iter][3]: {mae_i | mse_i, outlier_i, poseError_i}, the
 * third already multiplied by wt_pose_loss and, like the other two, not yet discounted; total adds discount^(n_iter-1-i) x it.
 * grad_logits carries the term's gradient through the same chain (concatenate, Kabsch / SVD adjoint, weight normalisation, sigmoid'):
 *     dL/dRc_i += c_i (-1 / (2 sqrt(1 - s_i^2))) R_gt,   dL/dtc_i += c_i (tc_i - t_gt) / |tc_i - t_gt|,   c_i = discount_i wt_pose_loss / P.
 * Corner rules:
 *   |tc_i - t_gt| == 0: zero translation gradient (torch.norm's own subgradient).
 *   1 - s_i^2 <= 0 (s_i in fp64 from the fp32 matrices): the value is acos of s_i clamped to [-1, 1]; the rotation gradient is ZERO.
 *     A deliberate departure: in fp32 the reference's clamp bounds -1 + 1e-16, 1 - 1e-16 round to -1, 1 and its autograd yields inf
 *     or NaN there, after which its loop skips the step (train.py:436-441); this entry returns a finite gradient instead.
 * A pair whose pose solve is degenerate gets no special treatment from this term, as it gets none from the point-distance term: the
 * kernel replays the chain as it is; the trainer's step is skipped on the engine's `invalid` flag, as before. */
int dsir_align_loss_backward3(dsir_ctx* ctx, const float* pt_src, const float* pt_ref, const int32_t* idx, const float* logits,
                              const float* labels, const float* transform_gt, int pairs, int J, int K, int n_iter, int loss_type,
                              float wt_ptDist_loss, float wt_inlier_loss, float loss_discount_factor, float wt_pose_loss,
                              float* transforms, double* losses, float* grad_logits, double* losses_per_pair);

/* Launch-bound small batches: capture the whole dsir_register launch sequence into a hipGraph once per
 * call signature (sizes and buffer addresses) and replay it; the context keeps the graphs of its 16 most recent signatures
 * (a server that coalesces 1 .. K single-pair requests per call replays K graphs in turn).  Off by default.
 * ROCm 7.x: the process must run with DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 (in the environment before the HIP runtime
 * initialises): the runtime's graph packet capture replays a captured registration wrongly from its third launch on once
 * the host has waited between launches (tools/graph_replay_check.py).  The Python host sets it on import. */
int dsir_enable_graph(dsir_ctx* ctx, int enable);
/* Launch census of the registration captured LAST by this context (dsir_enable_graph): out (HOST, 4 x i64) = graph nodes in all,
 * kernel nodes, memset nodes, memcpy nodes - what one dsir_register call of that signature costs in launches.  Zeros before the
 * first capture. */
int dsir_graph_stats(dsir_ctx* ctx, int64_t* out);
/* A/B switch (measurement / test): the deep pyramid levels of RandLA.forward (RandLANet.py:215-230, :339-359; levels 2 / 3, mlp_mid,
 * the first two decoder blocks) as ONE persistent launch whose phases are the former launches' tiles (csrc/walk.hip), for launches of
 * up to 16 clouds.  OFF by default: it removes 114 of a single-pair registration's 305 launches but is slower than they are (3.46 ms
 * against 3.09 ms per registration on MI355X: a dependent launch costs ~1.5 us, a phase hand-off ~2 us, and the tile bodies' own
 * latency chains - what the time is made of - are the same).  Same kernels' code on the same operands, statistics in exact atomics:
 * same bits either way (tests/test_gpu_walk.py). */
int dsir_enable_walk(dsir_ctx* ctx, int enable);
/* Measurement: with DSIR_TUNING=1 DSIR_WALK_TRACE=1 in the environment at dsir_create the walker stamps, per program of a call
 * (12 slots) and phase (32), the device clock of cloud 0's earliest tile picked up, earliest tile past its wait, latest tile body
 * end and latest publish: out (HOST, 12 x 32 x 4 i64), clock_khz the clock's rate.  reset: re-arm the stamps.  Synchronises. */
int dsir_walk_trace(dsir_ctx* ctx, int reset, int64_t* out, int64_t* clock_khz);

/* Test/measurement hooks. */
/* Wall-clock-free kernel timing of the dominant kernel (nn_match) accumulated
 * with HIP events on the engine stream since the last reset: total ms and
 * launch count. */
int dsir_match_timer(dsir_ctx* ctx, int reset, double* total_ms, int64_t* launches);
/* The same launches with the operation's dominant kernel (screen_kernel of csrc/nn_screen.hip, or nn_match_kernel when
 * the exhaustive path runs) bracketed on its own: op_ms = every kernel of the operation, kernel_ms = that kernel. */
int dsir_match_timer2(dsir_ctx* ctx, int reset, double* op_ms, double* kernel_ms, int64_t* launches);
/* A/B switch (measurement): 0 = dsir_register always takes the exhaustive exact-fp32 arg-min kernel, 1 (default) = the
 * fp16-screened path for large problems.  Both return the same bits.  Initialised from DSIR_NO_SCREEN (behind the tuning gate, below). */
int dsir_enable_screen(dsir_ctx* ctx, int enable);
/* A/B switch (measurement / test): 1 (default) = the five wide layers of the aggregation chain (mlp_att 32 -> 64 -> 128 -> 256 ->
 * 64, mlp_proj; network/model.py:223-233) run as fp16-split products on the fp16 matrix pipe (csrc/agg_chain.hip, csrc/split_f16.h: each fp32
 * operand = two fp16 numbers, three MFMAs per product, fp32 accumulation - descriptors within ~1e-7 of the fp32 kernel's for
 * weights the split carries); 0 = the exact-fp32 form of the same chain, bit-identical to the unfused layer-by-layer launches.
 * The split is as accurate as fp32 in one magnitude band only (csrc/split_f16.h): each part loses up to 2^-25 ABSOLUTE per
 * element, so a matrix of small entries is carried badly and one with an entry above 65504 not at all.  dsir_finalize_weights
 * therefore checks every matrix (all |w| <= 65504, and hi + lo within 2^-19 of the matrix in Frobenius norm); a layer whose matrix
 * fails runs in exact fp32 even with the switch on, and the aggregation chain and the head do so as a whole if any of their
 * matrices fails.  With that, state dicts rescaled by 2^-14 .. 2^+20 in ways that preserve the network's function keep
 * descriptors, features and logits within the tolerances at which they are compared with the fp64 oracle
 * (tests/test_gpu_split_magnitudes.py).  Inputs of dsir_aggregate for which the descriptor tolerance (rtol 1e-4, atol 2e-5)
 * is pinned: feat0 of 2^-12 .. 2^10 times unit normal, scores down to U(0, 2^-8), coordinates up to +-50.
 * Initialised from DSIR_AGG_F32 (set => 0).
 * What the switch covers: the aggregation chain, the per-point head (csrc/head_mlp.hip) and the LDS-tiled GEMMs (csrc/pw_tile.hip,
 * through GemmArgs::Wh staying unset).  What it does NOT cover: the attentive-pooling score contraction, which is an fp16-split
 * product unconditionally in csrc/att_pool.hip (levels 0 - 2, widths 16 / 64 / 128): those kernels have no exact-fp32 twin at run time,
 * their fp32 reference is the oracle (tests/test_gpu_parity.py).  Level 3 (width 256) pools in csrc/pw_tile.hip and follows the switch. */
int dsir_enable_agg_split(dsir_ctx* ctx, int enable);
/* The operand split those layers rest on, HOST buffers, no context, no GPU: hi[i] = fp16(x[i]) and lo[i] = fp16(x[i] - hi[i])
 * as IEEE binary16 bit patterns, both rounded to nearest even - what dsir_finalize_weights applies to every weight matrix (the
 * kernels apply the same rule to activations).  x = hi + lo + r with |r| <= max(2^-22 |x|, 2^-25) for |x| <= 65504: the second
 * term is an absolute floor (fp16 sub-normal spacing), so below |x| ~ 2^-3 the relative error of a split product grows like
 * 1 / |x|, and above 65504 hi is infinite.  See dsir_enable_agg_split for which matrices are contracted this way. */
void dsir_split_f16(const float* x, int64_t n, uint16_t* hi, uint16_t* lo);
/* Same launches, bracketed on the DEVICE's constant-rate clock inside the kernel (first wave start .. last wave end,
 * the quantity a kernel trace reports): unlike the HIP-event bracket it does not include time the launch spends
 * queued behind other streams' kernels when several engines share the GPU. */
int dsir_match_timer_device(dsir_ctx* ctx, int reset, double* total_ms, int64_t* launches);
int dsir_enable_match_timer(dsir_ctx* ctx, int enable);
/* Which arg-min path dsir_register took since the last reset, and how selective the screening was.  out (HOST, 5 x i64):
 * [0] searches through the screened path (csrc/nn_screen.hip), [1] src rows they searched, [2] of those the rows the
 * screening left undecided (searched by the exhaustive exact-fp32 kernel), [3] pairs searched exhaustively as a whole,
 * [4] searches that took the exhaustive kernel directly (small problems, forced runs excluded).  Synchronises.
 * Not counted while a hipGraph replays (dsir_enable_graph): [4] is a host-side counter. */
int dsir_screen_stats(dsir_ctx* ctx, int reset, int64_t* out);
/* The pruned search of long ref ranges (csrc/nn_prune.hip; clouds of 8192 points and more in launches of 65536 src rows and more,
 * every registration iteration): out (HOST, 2 x i64) = (row block, column tile) products the screening visited, and the number it
 * would have visited without pruning, since the last reset.  Synchronises. */
int dsir_prune_stats(dsir_ctx* ctx, int reset, int64_t* out);
/* A/B switch (measurement / test): the pruned search runs for ref clouds of min_points points and more (default 8192, initialised
 * from DSIR_PRUNE_MIN_K; 0 = never) in launches of min_rows src rows (pairs x points) and more (default 65536: below that the
 * launch does not fill the chip with work items and the preparation is pure cost).  Pruned and unpruned searches return the
 * same bits: only products that cannot hold a row's arg-min - nor tie with it - are skipped. */
int dsir_set_prune_thresholds(dsir_ctx* ctx, int min_points, int64_t min_rows);
/* A/B switch (test): clouds of `min_points` points and more solve their pose in chunks over several workgroups per pair
 * (csrc/kabsch.hip; default 16384, <= 0 restores it), in dsir_register and dsir_kabsch.  Same formulas either way; the fp64
 * partial sums are taken in another order. */
int dsir_set_kabsch_chunked_min(dsir_ctx* ctx, int min_points);

/* The tuning gate.  The library has a number of measurement / A-B switches named DSIR_* (kernel-family selection, tile
 * geometry, thresholds).  They are environment variables, read in ONE function (csrc/engine.hip,
 * tuning_env) and ONLY while the gate is open: DSIR_TUNING=1 in the environment, or dsir_set_tuning(1) called before the
 * first library call that reads a switch (most are read once per process).  With the gate closed - the default - every
 * DSIR_* variable is ignored, so a stray one in a user's environment cannot change what runs.  dsir_tuning() reports
 * the gate's state.  Every variant behind a switch is the HIP path; none is a fallback. */
void dsir_set_tuning(int on);
int dsir_tuning(void);

/* GroupNorm (RandLANet.py:90-107) statistics of a layer meet across workgroups in exact, order-independent atomics
 * (csrc/device_utils.h, gn_block_commit); the proof needs at most dsir_gn_contribution_limit() contributions per (cloud, group)
 * statistic.  dsir_gn_contributions: the most any statistic receives for a cloud of n_points points under this configuration (host
 * arithmetic over the launchers' grid rules; -1: bad arguments); dsir_max_points_limit: the largest max_points dsir_create accepts
 * for it.  No GPU needed. */
int dsir_gn_contributions(const dsir_cfg* cfg, int n_points);
int dsir_gn_contribution_limit(void);
int dsir_max_points_limit(const dsir_cfg* cfg);
/* The same under dsir_create_ex's flags.  DSIR_FLAG_PPF adds the point-pair-feature layer (one contribution per 64 points) and moves
 * level 0's mlp1 / mlp_skip to the general kernel (one per 64 rows); level 0's lfa.mlp1 (one per 32 points) remains the largest, so
 * the limit is the same number - computed, not assumed. */
int dsir_gn_contributions_ex(const dsir_cfg* cfg, int flags, int n_points);
int dsir_max_points_limit_ex(const dsir_cfg* cfg, int flags);

/* Diagnostics of the fp16 screening (csrc/nn_screen.hip) on ONE pair, all pointers DEVICE memory: for every (row, column)
 * the screening's lower bound L, its upper bound U = L + 2 d and the exact fp32 distance D of dsir_nn_match
 * (lower / upper / exact [J][K]; zacc [J][K], optional: the raw fp32 accumulator 2^22 (c + a.b) the six chained
 * v_mfma_f32_16x16x32_f16 leave, for measuring the matrix core's accumulation error against an fp64 sum of the same
 * fp16 products) - computed by the same MFMA chain on the same fp16 operands as the product kernel -,
 * plus what the product path did with the same inputs: idx [J] (its arg-min), thresh [J] (the row's final threshold),
 * cand_count [J] (entries emitted; > dsir_screen_cap() = the list overflowed), cand_code / cand_lower
 * [J][dsir_screen_cap()] (code >= 0: a column and the bits of its L; code < 0: a lane class), out_of_domain [1]
 * (non-zero: a component was outside the bound's domain |x| <= 16 - the product path would not screen such input).
 * The screened search is exact iff L <= D <= U for every entry; tests/test_gpu_screen_bound.py asserts it on
 * adversarial inputs.  J * K <= 2^26. */
int dsir_screen_bounds(dsir_ctx* ctx, const float* desc_src, const float* desc_ref, int J, int K, float* lower, float* upper,
                       float* exact, float* zacc, int32_t* idx, float* thresh, int32_t* cand_count, int32_t* cand_code, float* cand_lower,
                       int32_t* out_of_domain);
int dsir_screen_cap(void);

/* Top-k descriptor search (csrc/nn_topk.hip, whose header states the rule): a row's k smallest keys order_bits(d) << 32 | column in
 * ascending order, d dsir_nn_match's fp32 distance - rank 0 IS dsir_nn_match's result, ties go to the lower column, nothing depends
 * on the arrival order of workgroups.  A rank without an entry (k > K, non-finite distances) is index -1, distance +inf.  DEVICE
 * pointers; bad arguments (k outside [1, DSIR_TOPK_MAX], J or K beyond max_points, a workspace that does not fit) are errors and
 * leave the context usable. */
#define DSIR_TOPK_MAX 8
/* k nearest ref descriptors of every src descriptor: idx [P][J][k] i32, dist [P][J][k] f32 (dist may be NULL) */
int dsir_nn_match_topk(dsir_ctx* ctx, const float* desc_src, const float* desc_ref, int pairs, int J, int K, int k,
                       int32_t* idx, float* dist);
/* host only: the column splits the launcher takes for this shape (tests use it to place K across a split boundary); -1: bad arguments */
int dsir_nn_match_topk_splits(dsir_ctx* ctx, int pairs, int J, int K, int k);
/* dsir_feature_correspondences with k candidates per src row or a ratio test: corr [P][J*k][2], counts [P],
 * corr_dist [P][J*k] f32 or NULL.  k = 1, ratio = 0 gives dsir_feature_correspondences' bytes.
 * Candidates: (j, c) for every rank < k of row j that has an entry; under `mutual` kept iff j is among the k nearest of column c in
 * the ref -> src search; ascending j, then ascending rank; rows beyond counts[p] are -1 (corr_dist: +inf).
 * Ratio test (Lowe): with r2 = fp32(ratio * ratio), row j keeps its rank-0 match iff rank 1 is missing or
 * max(d0, 0) < r2 * max(d1, 0).  ratio <= 0: no test; ratio >= 1, a non-finite ratio, ratio > 0 with k > 1 (the test is defined on
 * the 1-NN set) and J * k > max_points (the pose stages take M <= max_points) are refused. */
int dsir_feature_correspondences_ex(dsir_ctx* ctx, const float* desc_src, const float* desc_ref, int pairs, int J, int K,
                                    int mutual, int k, float ratio, int32_t* corr, int32_t* counts, float* corr_dist);

/* ---- scene registration: edge information matrices and the pose graph ------- */

/* open3d's get_information_matrix_from_point_clouds(src, tgt, max_correspondence_distance, T) for P pairs at once (open3d is not
 * pinned: the rule is this engine's own, stated in the header of csrc/info_matrix.hip and restated in deepsir_amd/pose_graph.py).
 * Arguments as for dsir_icp_correspondences; the correspondence set is exactly the one that entry returns for the same arguments.
 * For every source row with idx >= 0, q = (x, y, z) the fp32 reference point it matched:
 *   G = [0 z -y 1 0 0; -z 0 x 0 1 0; y -x 0 0 0 1],  info = sum G^T G  in fp64 (ten sums; products of fp32 values are exact).
 * info_out [P][6][6] float64 row-major, open3d's order [rotation; translation], symmetric, both triangles written;
 * count_out [P] int32: the correspondences.  A pair without a correspondence gets the zero matrix and count 0; non-finite rows
 * are never correspondences.  Same bytes on every run (fixed partition of the sums, no floating-point atomics), for both values
 * of `search`, and for a pair whatever else is in the batch.  Scratch comes from the context workspace. */
int dsir_information_matrix(dsir_ctx* ctx, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                            float max_corr_dist, const float* T, int search, double* info_out, int32_t* count_out);
/* dsir_information_matrix with per-pair row counts: the rule, the Jp == 0 / Kp == 0 cases and the byte-for-byte contract are stated
 * at dsir_icp_refine_ex3.  The correspondence set is dsir_icp_correspondences_ex's for the same arguments. */
int dsir_information_matrix_ex(dsir_ctx* ctx, const float* points_src, const float* points_ref, int pairs, int J, int K, int stride,
                               float max_corr_dist, const float* T, int search, double* info_out, int32_t* count_out,
                               const int32_t* counts_src, const int32_t* counts_ref);

#define DSIR_POSE_GRAPH_MAX_NODES 128
#define DSIR_POSE_GRAPH_MAX_ITER 100        /* the default of the Python layer */
/* status bits of dsir_pose_graph_optimize's stats[g][3]; 0: stopped on the relative decrease of F or on the relative step */
#define DSIR_PG_MAX_ITER 1
#define DSIR_PG_LAMBDA 2
#define DSIR_PG_PIVOT 4
#define DSIR_PG_NON_FINITE 8
#define DSIR_PG_EDGE_INDEX 16

/* open3d's global_optimization (pose graph with a line process over uncertain edges; Choi et al., robust reconstruction) for G
 * graphs at once, one workgroup per graph (open3d is not pinned: the rule - residual, objective, Jacobians, damping, stops - is
 * this engine's own, stated in the header of csrc/pose_graph.hip and restated in deepsir_amd/pose_graph.py, optimize_host).
 * Node pose X_i maps fragment i's frame to the scene frame; edge (s, t, T, Lambda, uncertain) says p_t = T p_s, so a consistent
 * graph has X_s = X_t T; e = [log rot; trans] of T^-1 X_t^-1 X_s;  F = sum l e^T Lambda e + sum_uncertain mu (sqrt(l) - 1)^2 with
 * l = (mu / (mu + e^T Lambda e))^2 on uncertain edges, 1 on the others.  The default mu is the Python layer's
 * pose_graph.line_process_weight: preference x max_corr_dist^2 x mean over the uncertain edges of Lambda[3][3].
 * node_off, edge_off, reference_node: HOST arrays [G+1], [G+1], [G] (CSR over the batch; reference_node is graph-local and held
 * fixed: its pose is returned as its input bits).  Device arrays: X0 [sum N][3][4] f64, edge_st [sum E][2] int32 (graph-local s, t),
 * edge_T [sum E][3][4] f64, edge_info [sum E][6][6] f64, edge_uncertain [sum E] bytes, mu [G] f64; outputs X [sum N][3][4] f64,
 * line [sum E] f64 (the final l), stats [G][4] f64 {F at X0, F at X, solves made, status}.  scratch: device memory of
 * dsir_pose_graph_scratch_bytes(...) bytes (0 for a refused batch).
 * Refused on the host, before any launch: a graph of more than DSIR_POSE_GRAPH_MAX_NODES nodes or of none, E = 0 with N > 1, a
 * reference_node outside [0, N), offsets that do not ascend from 0.  (A graph whose edges do not connect it is refused by the Python
 * layer, which sees the edge list.)  N = 1 returns its input.  On the device, a pivot that is not positive, an entry that is not
 * finite (or mu <= 0) or an edge index outside the graph ends THAT graph with the bit set, X = X0 and line = 1; the other graphs
 * of the call are unaffected bit for bit.  Same bytes on every run: edges are assembled in order, nothing is scatter-added. */
size_t dsir_pose_graph_scratch_bytes(int graphs, const int32_t* node_off, const int32_t* edge_off, const int32_t* reference_node);
int dsir_pose_graph_optimize(dsir_ctx* ctx, int graphs, const int32_t* node_off, const int32_t* edge_off, const double* X0,
                             const int32_t* edge_st, const double* edge_T, const double* edge_info, const uint8_t* edge_uncertain,
                             const double* mu, const int32_t* reference_node, int max_iter, void* scratch, double* X, double* line,
                             double* stats);

#ifdef __cplusplus
}
#endif
#endif /* DSIR_H */
