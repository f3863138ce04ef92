/*
 * dsir_train.h — C ABI of the training operators (libdsir.so), SURVEY.md section 8(f) rank 4: the backward half.
 *
 * The reference trains with torch autograd (train.py:396-448): every operator below is the forward or the backward of
 * one ATen call that RandLA.forward (network/RandLANet.py:311-372) makes, so that the inlier model's training step
 * (forward with saved activations, backward from d loss / d logits - dsir_align_loss_backward - to every parameter,
 * Adam) runs on the device without autograd.  deepsir_amd/train.py strings them together in the reference's module
 * order; this header is what a non-Python host would bind.
 *
 * Conventions: device pointers, fp32, POINT-MAJOR rows ([rows][channels], leading dimension `ld` in floats), int32
 * indices; `stream` is a hipStream_t (NULL = default stream); calls are asynchronous; return 0 or a hipError_t.
 * Reductions are deterministic (fixed partition, fixed order) except the two scatter-adds, which use fp32 atomics
 * exactly like ATen's index/gather backward on a GPU.
 */
#ifndef DSIR_TRAIN_H
#define DSIR_TRAIN_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* nn.Conv2d 1x1 / nn.Conv1d / nn.Linear (RandLANet.py:77-88, :148, :270, :41): Y[r][n] = beta Y[r][n] + bias[n] +
 * sum_k X[r][k] W[n wn + k wk].  Forward: W = weight [Cout][Cin], wn = Cin, wk = 1.  Backward w.r.t. the input
 * (dX = dY W): X = dY, wn = 1, wk = Cin, N = Cin, K = Cout; beta = 1 accumulates into an existing gradient.
 * Exact-fp32 MFMA (v_mfma_f32_16x16x4_f32), k ascending. */
int dsir_t_gemm(void* stream, const float* X, int ldx, const float* W, int wn, int wk, const float* bias, float* Y, int ldy,
                int64_t rows, int K, int N, float beta);

/* Backward of the same call w.r.t. weight and bias: dW[n][k] += sum_r dY[r][n] X[r][k], db[n] += sum_r dY[r][n]
 * (db may be NULL).  scratch: dsir_t_gemm_dw_scratch(rows, N, K) bytes. */
size_t dsir_t_gemm_dw_scratch(int64_t rows, int N, int K);
int dsir_t_gemm_dw(void* stream, const float* dY, int ldy, const float* X, int ldx, int64_t rows, int N, int K, float* dW,
                   float* db, void* scratch);

/* nn.GroupNorm(groups, C) (+ LeakyReLU 0.2 when act) over one cloud's [M][C] block (RandLANet.py:90-107), also
 * nn.BatchNorm1d in training mode (clouds = 1, M = all rows, groups = C; RandLANet.py:44): biased variance, eps 1e-5.
 * stats [clouds][groups][2] = {mean, rstd} are kept for the backward.  scratch: dsir_t_gn_scratch(clouds, M, C) bytes
 * for either call (partial sums per row chunk, reduced in chunk order: csrc/train_layouts.h). */
size_t dsir_t_gn_scratch(int clouds, int M, int C);
int dsir_t_gn_fwd(void* stream, const float* Y, int clouds, int M, int C, int groups, const float* gamma, const float* beta,
                  int act, float* out, float* stats, void* scratch);
/* dY (may alias dOut) = d loss / d Y; dgamma / dbeta accumulate. */
int dsir_t_gn_bwd(void* stream, const float* dOut, const float* Y, const float* stats, int clouds, int M, int C, int groups,
                  const float* gamma, const float* beta, int act, float* dY, float* dgamma, float* dbeta, void* scratch);

/* The running statistics nn.BatchNorm1d keeps in training mode (momentum 0.1, unbiased variance); stats = dsir_t_gn_fwd's
 * with groups = C over M rows. */
int dsir_t_bn_running(void* stream, const float* stats, int C, int64_t M, float momentum, float* running_mean, float* running_var);

/* gather_neighbour_V2 / nearest_interpolation (network/tools.py:197-221, RandLANet.py:393-408):
 * Y[cloud][j][col_off + c] = X[cloud][idx[cloud][j]][c], j < m, c < C; X [clouds][n][C]; backward = scatter-add. */
int dsir_t_gather(void* stream, const float* X, int n, int C, const int32_t* idx, int m, int clouds, float* Y, int ldy, int col_off);
/* The backward of a gather is a sum over the SOURCES of every destination row.  It is taken in a fixed order - ascending source row -
 * through the inverse of the index (a "plan": one stable sort of (destination, source) pairs per index tensor, re-used by every
 * operator that shares the index), so a gradient has the same bits on every run (up to round 4: float atomics, 2e-6 of its scale
 * between runs).  dsir_t_scatter_plan: idx [clouds][m] into [clouds][n] -> order [clouds * m] i32 (sources grouped by destination),
 * offsets [clouds * n + 1] i32; scratch: dsir_t_scatter_plan_scratch(clouds * m) bytes.
 * dsir_t_scatter_add: dX[cloud][i][c] = sum over the sources j of row i of dY[cloud m + j][col_off + c]  (overwrites dX). */
size_t dsir_t_scatter_plan_scratch(int64_t total);
int dsir_t_scatter_plan(void* stream, const int32_t* idx, int m, int clouds, int n, int32_t* order, int32_t* offsets, void* scratch);
int dsir_t_scatter_add(void* stream, const float* dY, int ldy, int col_off, const int32_t* order, const int32_t* offsets, int clouds,
                       float* dX, int n, int C);

/* Building_block.relative_pos_encoding (RandLANet.py:197-212): out[cloud][i k + j][10] = {|pj - pi|, pj - pi, pi, pj};
 * xyz [clouds][n][3], idx [clouds][n][k].  No backward: the coordinates are data. */
int dsir_t_relpos(void* stream, const float* xyz, const int32_t* idx, int n, int k, int clouds, float* out);

/* The inlier model's input of one registration iteration (network/model.py:571-573; the src cloud moved by the previous
 * cumulative pose, :587 with R_t.detach()): out[pair][j] = {T x_src[j], x_ref[idx[pair][j]]}; xyz_src [P][J][3], xyz_ref
 * [P][K][3], T = NULL (iteration 0) or the pose of pair p at T + p t_stride ([3][4] row-major), out [P][J][6]. */
int dsir_t_inlier_input(void* stream, const float* xyz_src, const float* xyz_ref, const int32_t* idx, const float* T, int t_stride,
                        int pairs, int J, int K, float* out);

/* Att_pooling (RandLANet.py:148-155) after its fc: S [points][k][C] scores in, softmax over k written back in place (kept
 * for the backward), out[point][c] = sum_k cat[point][k][c] S[point][k][c].  Backward: dCat = direct part (the caller adds
 * dS W_fc with dsir_t_gemm beta = 1), dS = d loss / d scores. */
int dsir_t_attpool_fwd(void* stream, const float* cat, float* S, int64_t points, int k, int C, float* out);
int dsir_t_attpool_bwd(void* stream, const float* dOut, const float* cat, const float* A, int64_t points, int k, int C, float* dCat,
                       float* dS);

/* RandLA.random_sample (RandLANet.py:374-391): out[cloud][j][c] = max_t X[cloud][pool[cloud][j][t]][c]; arg = the row
 * that won (first of equals); backward adds dOut to that row, in ascending order of the outputs (no float atomics). */
int dsir_t_maxpool_fwd(void* stream, const float* X, int n, int C, const int32_t* pool, int m, int k, int clouds, float* out,
                       int32_t* arg);
/* backward: order / offsets = the plan of the pool index viewed as [clouds][m k] (dsir_t_scatter_plan); overwrites dX [clouds][n][C] */
int dsir_t_maxpool_bwd(void* stream, const float* dOut, const int32_t* arg, const int32_t* order, const int32_t* offsets, int m, int k, int C,
                       int clouds, float* dX, int n);

/* SemanticLoss.compute_loss (network/loss.py:930-960, :919-928): F.cross_entropy(weight = class weights, reduction 'mean')
 * over the points whose label is not 0 ("unlabeled"), class = label - 1; logits [rows][C] point-major, labels [rows] in 0..C.
 * out (device, 4 doubles) = {loss = sum w_y nll / sum w_y, sum w_y, correct arg-max predictions, valid rows};
 * dlogits [rows][C] = grad_scale * d loss / d logits (ignored rows 0).  scratch: dsir_t_weighted_ce_scratch(rows) bytes.
 * The reference passes the weights as a [1, C] tensor, which F.cross_entropy of the torch in this image rejects; the rule
 * here is the documented one for a [C] weight vector (oracle/train.py restates it; parity unpinned). */
size_t dsir_t_weighted_ce_scratch(int64_t rows);
int dsir_t_weighted_ce(void* stream, const float* logits, const int32_t* labels, const float* class_weights, int64_t rows, int C,
                       float grad_scale, float* dlogits, double* out, void* scratch);

/* F.normalize(x, p = 2, dim = channels) (model.py:232-233, :651-652) and its backward; norms [rows] = max(|x|, 1e-12). */
int dsir_t_l2norm_fwd(void* stream, const float* x, int64_t rows, int C, float* y, float* norms);
int dsir_t_l2norm_bwd(void* stream, const float* dy, const float* y, const float* norms, int64_t rows, int C, float* dx);

/* DetDesLoss.forward (network/loss.py:667-702) = CircleLoss.forward(feat_ref, feat_src, pt_ref, T_gt pt_src, score_ref, .)
 * (:500-571) with chamfer_loss_weight 0 (arguments.py:46), AND its backward w.r.t. both descriptor sets - what the `feat`
 * pipeline's loss.backward() hands the aggregation MLPs (the feature extractor is frozen there, model.py:136).
 * feat_* [P][M][C] point-major, pt_* [P][M][3], score_ref [P][M], transform_gt [P][3][4]; N1 = N2 = M as the reference's
 * element-wise sum of row and column terms requires.  out (device, 4 doubles) = {total, loss_feat, loss_det, accuracy}.
 * The reference's arithmetic is kept as it executes (see oracle/train.py::det_des_loss, pinned by its autograd). */
size_t dsir_t_det_des_loss_scratch(int pairs, int M);
int dsir_t_det_des_loss(void* stream, const float* feat_ref, const float* feat_src, const float* pt_ref, const float* pt_src,
                        const float* score_ref, const float* transform_gt, int pairs, int M, int C, float thres_radius, float det_loss_weight,
                        double* out, float* d_feat_ref, float* d_feat_src, void* scratch);

/* The point-pair-feature input layer of args.use_ppf in training mode (RandLANet.py:110-137 feat_grouping, :324-332: mlp_pre =
 * Conv2d 10 -> 12 + bias, GroupNorm(4, 12), LeakyReLU(0.2), then the mean over the 16 neighbours; network/matchnet.py:11-30 angle).
 * rows [clouds][n][stride >= 6]: columns 0 - 2 the point, 3 - 5 its normal (the inlier model: the matched reference point,
 * network/model.py:574-590); neigh [clouds][n][16] the level-0 neighbour lists; W [12][10], b, gamma, beta [12]: mlp_pre.conv.weight /
 * .bias, mlp_pre.norm.weight / .bias.  out [clouds][n][12]: the same bits as dsir_ppf_pre (include/dsir.h) on the same inputs - the
 * two launches are the same (csrc/ppf.hip states the arithmetic).  saved [clouds][32] is kept for the backward: the fp32 scale[12] /
 * shift[12] the layer applied and {mean, rstd} of the 4 groups; nothing of size n x 16 is stored.
 * scratch: dsir_t_ppf_fwd_scratch(clouds, n) bytes (0: the shape is refused - more than 4096 x 64 points per cloud). */
size_t dsir_t_ppf_fwd_scratch(int clouds, int n);
int dsir_t_ppf_fwd(void* stream, const float* rows, int stride, const int32_t* neigh, int clouds, int n, const float* W, const float* b,
                   const float* gamma, const float* beta, float* out, float* saved, void* scratch);
/* Its backward (what autograd does for the four parameters of RandLANet.py:251-254's mlp_pre; the rows are data in every pipeline -
 * the loader's points and normals, or [moved src ; matched ref] under R_t.detach() - so nothing flows to them).  The SAME rows, neigh
 * and parameters as the forward, its `saved`, dOut [clouds][n][12] = d loss / d out.  dW [12][10], db, dgamma, dbeta [12] ACCUMULATE.
 * Every row is rebuilt twice (pass A: d gamma, d beta and the group sums; pass B: dW, db) with the forward's bits; the sums take a
 * fixed partition (64 points per workgroup) and order, fp64 partials, no float atomics: the same bytes on every run.
 * scratch: dsir_t_ppf_bwd_scratch(clouds, n) bytes; after the call it begins with [clouds][24] doubles, every cloud's own
 * {d beta[12], d gamma[12]} - the same bytes for a cloud alone or inside a batch; the parameter gradients add them in cloud order. */
size_t dsir_t_ppf_bwd_scratch(int clouds, int n);
int dsir_t_ppf_bwd(void* stream, const float* rows, int stride, const int32_t* neigh, int clouds, int n, const float* W, const float* b,
                   const float* gamma, const float* beta, const float* saved, const float* dOut, float* dW, float* db, float* dgamma,
                   float* dbeta, void* scratch);

/* F.leaky_relu(a + b, 0.2) (RandLANet.py:230) and its backward (d a = d b = dOut * slope(out)). */
int dsir_t_add_leaky_fwd(void* stream, const float* a, const float* b, int64_t n, float* out);
int dsir_t_add_leaky_bwd(void* stream, const float* dOut, const float* out, int64_t n, float* d);

/* nn.Dropout (RandLANet.py:366) with the mask supplied: y = x * mask * scale (forward and backward alike). */
int dsir_t_mul_mask(void* stream, const float* x, const uint8_t* mask, float scale, int64_t n, float* y);
/* torch.topk(score, k) of feat_score (model.py:692): the k best key points per cloud, descending score, equal scores in
 * ascending index, NaNs first (csrc/select.hip, the operator dsir_forward_pair uses); idx [clouds][k], score_out [clouds][k]. */
size_t dsir_t_topk_scratch(int clouds, int n);
int dsir_t_topk(void* stream, const float* score, int clouds, int n, int k, int32_t* idx, float* score_out, void* scratch);

/* logit.sigmoid() (model.py:577): the correspondence weights of the weighted Kabsch step */
int dsir_t_sigmoid(void* stream, const float* x, int64_t n, float* y);
/* y += a x */
int dsir_t_axpy(void* stream, float a, const float* x, int64_t n, float* y);

/* "Check if any of the gradients is NaN" (train.py:437-441): flag[0] (device int32) = 1 if any of the n floats is NaN, else 0. */
int dsir_t_any_nan(void* stream, const float* x, int64_t n, int32_t* flag);

/* torch.optim.Adam.step (train.py:323, :446; betas 0.9 / 0.999, eps 1e-8, no weight decay, no amsgrad):
 * m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2; p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps). */
int dsir_t_adam(void* stream, float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps,
                int step);

/* ---- ground-truth matches and inlier targets of the `align` step (csrc/match_targets.hip) -------------------------------
 * The reference's loader builds data['matches'] with an open3d KD-tree radius search around every T_gt src_i
 * (dataloader/data_base.py:436-449, K = None: ALL reference points inside radius = voxel_size * positive_pair_radius_multiplier);
 * ScanAlignmentLoss.find_correct_correspondence (network/loss.py:723-749) asks on the host whether (j, idx[j]) is in that list:
 * the 0/1 targets of the confidence term.  open3d is not installable here: parity is unpinned, the engine owns the rule -
 *   moved point, fp32, no fused multiply-add:  c_r = ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3]
 *   squared distance as csrc/icp.hip forms it: d2 = (dx dx + dy dy) + dz dz, d = ref - c, every operation rounded
 *   match  <=>  d2 < r r, r r one fp32 product; strict, as nanoflann's radius result set compares (from memory: it cannot be
 *   checked here).
 * Every operator below decides through this one rule, so they agree bit for bit.  No atomics: two runs give the same bytes.
 * src [pairs][J][stride], ref [pairs][K][stride] (first three columns, stride >= 3), transform_gt [pairs][3][4]; pairs J K <= 2^31 - 1.
 *
 * The match list as CSR, in two passes (brute force, pairs J K distance tests each):
 *   _count: counts [pairs J] = matches of every source row, offsets [pairs J + 1] = their exclusive sum (offsets[pairs J] = total);
 *           scratch: dsir_t_radius_matches_scratch(pairs, J, K) bytes - it carries the per-slice counts over to _fill.
 *   the caller reads offsets[pairs J] from the device and sizes cols;
 *   _fill:  the SAME inputs, offsets and scratch -> cols [n_cols]: row (p, j)'s matching reference indices, ascending, at
 *           offsets[p J + j].  Nothing is written at or past n_cols. */
size_t dsir_t_radius_matches_scratch(int pairs, int J, int K);
int dsir_t_radius_matches_count(void* stream, const float* src, const float* ref, int stride, const float* transform_gt, int pairs, int J,
                                int K, float radius, int32_t* counts, int32_t* offsets, void* scratch);
int dsir_t_radius_matches_fill(void* stream, const float* src, const float* ref, int stride, const float* transform_gt, int pairs, int J,
                               int K, float radius, const int32_t* offsets, const void* scratch, int32_t* cols, int64_t n_cols);

/* Targets from geometry: labels[i][p][j] = rule(T_gt[p], src[p][j], ref[p][idx[i][p][j]]) ? 1 : 0; idx [n_iter][pairs][J] (clamped
 * into [0, K)), labels [n_iter][pairs][J] fp32 - what dsir_align_loss_backward2 takes as `labels`.  With the reference's K = None
 * list this IS "(j, idx[j]) is among the matches": no list is needed.
 * The loss entries themselves live in dsir.h; dsir_align_loss_backward3 there adds the pose-error term (wt_pose_loss > 0) with two
 * corner rules, stated in full next to it: |tc_i - t_gt| == 0 gives a zero translation gradient (torch.norm's subgradient), and
 * 1 - s_i^2 <= 0 gives acos of the clamped s_i as the value and a ZERO rotation gradient, where the reference's fp32 autograd
 * yields inf or NaN and its loop skips the step. */
int dsir_t_inlier_targets_radius(void* stream, const float* src, const float* ref, int stride, const int32_t* idx, const float* transform_gt,
                                 int n_iter, int pairs, int J, int K, float radius, float* labels);

/* Targets from a caller's list, the reference's semantics, hash included (loss.py:280-294, :723-749): matches [n_matches][2] =
 * (src, ref) of all pairs concatenated, pair_offsets [pairs + 1] (device) the rows of every pair; keys [n_matches] int64 =
 * src + ref * hash_seed, sorted within each pair (hipCUB segmented radix sort).  Duplicates, an empty list and a src index
 * >= hash_seed alias exactly as on the host.  scratch: dsir_t_match_keys_scratch(n_matches, pairs) bytes; n_matches = 0: no-op.
 * _targets_matches: labels[i][p][j] = (j + idx[i][p][j] * hash_seed is among pair p's keys) ? 1 : 0; idx is not clamped (it is
 * never used as an address); keys may be NULL when every pair's list is empty.  The reference passes hash_seed = J (:819). */
size_t dsir_t_match_keys_scratch(int64_t n_matches, int pairs);
int dsir_t_match_keys(void* stream, const int32_t* matches, const int32_t* pair_offsets, int64_t n_matches, int pairs, int64_t hash_seed,
                      int64_t* keys, void* scratch);
int dsir_t_inlier_targets_matches(void* stream, const int64_t* keys, const int32_t* pair_offsets, const int32_t* idx, int n_iter, int pairs,
                                  int J, int64_t hash_seed, float* labels);

/* ---- training augmentation (csrc/augment.hip) ------------------------------------------------------------------------------------
 * DataBase.apply_augment / apply_augment_V2 (dataloader/data_base.py:221-296) between the voxel grid and the ground-truth matches.
 * The reference's random sources cannot be pinned; the rule is this engine's and is written down in deepsir_amd/augment.py (the
 * host restatement the tests compare against): counter-keyed splitmix64 draws, fp32 point arithmetic in one order without fused
 * multiply-add, float64 for the centroid, the jitter and the pose.  No atomics: the same inputs give the same bytes, and a cloud's
 * rows depend on its own key alone, never on the other clouds of the call.
 * params [clouds][24] eight-byte slots per cloud: R[9], t[3], scale, jitter scale, jitter clip (doubles), jitter mode (0 none,
 * 1 uniform, 2 clipped normal), centered, normals (int64), key (uint64), resample mode (0 Resampler, 1 FixedResampler, 2 permute
 * then FixedResampler), scaled (int64), 3 unused.
 *
 * _cloud_centroids: float64 mean xyz of the first min(counts[c], cap) rows of points [clouds][cap][stride] (dsir_voxel_downsample's
 * output) -> centroids [clouds][3]; invalid [clouds] int32: bit 0 = no rows (centroid 0), bit 1 = non-finite centroid.  Two-stage
 * sum in a fixed order; scratch: dsir_t_cloud_centroids_scratch(clouds) bytes. */
size_t dsir_t_cloud_centroids_scratch(int clouds);
int dsir_t_cloud_centroids(void* stream, const float* points, const int32_t* counts, int clouds, int cap, int stride, double* centroids,
                           int32_t* invalid, void* scratch);
/* The rule of dsir_resample with a key per cloud (params[c].key, mode params[c].rmode) in place of (seed, position in the call):
 * cloud c's rows are the same whatever else the call holds.  in [clouds][cap][stride] -> out [clouds][k][stride]; rows (may be NULL) [clouds][k] =
 * the source row of every output row; an empty cloud gives zeros.  need_perm = 0 skips the sort when every cloud's mode is 1.
 * scratch: dsir_t_resample_keyed_scratch(clouds, cap) bytes. */
size_t dsir_t_resample_keyed_scratch(int clouds, int cap);
int dsir_t_resample_keyed(void* stream, const float* in, const int32_t* counts, int clouds, int cap, int stride, int k, const void* params,
                          int need_perm, float* out, int32_t* rows, void* scratch);
/* One pass over in [clouds][k][stride] (out may be in): row j of cloud c -> s ((R (p - m) + t) + jitter(key, j)), columns 3:6 rotated
 * by R when params[c].normals and stride >= 6, every other column copied.  A cloud with counts[c] <= 0 is written as zeros. */
int dsir_t_augment(void* stream, const float* in, const int32_t* counts, int clouds, int k, int stride, const void* params,
                   const double* centroids, float* out);
/* transform_gt [pairs][3][4] fp32 = A_ref M A_src^-1, A = [R | t - R m] (m: the fp32-rounded centroid where centered, else 0), M
 * [pairs][3][4] float64, composed in float64 and rounded once; the translation is multiplied by the pair's scale unless
 * reference_gt (the reference leaves it unscaled, data_base.py:250-256). */
int dsir_t_augment_gt(void* stream, const double* M, const void* params_src, const void* params_ref, const double* centroids_src,
                      const double* centroids_ref, int pairs, int reference_gt, float* transform_gt);

/* ---- half-space crop (csrc/crop.hip) ---------------------------------------------------------------------------------------------
 * Transforms.RandomCrop.crop (dataloader/transformation.py:121-145) as the Oxford loader applies it twice to one scan
 * (dataloader/oxford_loader.py:141-153, p_crop = 0.6): the rows of a cloud beyond a plane normal to a random
 * direction, placed at the (1 - p_keep) quantile of the rows' projections onto that direction.  The reference's RNG and np.percentile's interpolation
 * cannot be pinned; the rule is this engine's and is written down in deepsir_amd/crop.py (the host restatement the tests compare
 * against bit for bit):
 *   d_j = ((px - mx) ux + (py - my) uy) + (pz - mz) uz, fp32, every operation rounded, no fused multiply-add, m = the centroid of
 *   dsir_t_cloud_centroids rounded to fp32; with n = min(counts[c], cap) rows, v = (n - 1) * (((1 - p_keep) * 100) / 100) in float64
 *   and lo = floor(v): row j is kept iff d_j > d_(lo), the lo-th smallest projection (0-based; -0 equals +0).  p_keep == 0.5 keeps
 *   d_j > 0, p_keep >= 1 every row.  A row with a non-finite d_j is dropped, counts in n and sorts last.  In exact arithmetic this is
 *   dist > np.percentile(dist, q); numpy keeps one row fewer only where v is within rounding of an integer from below.
 * Per cloud, never an error - invalid [clouds] int32: bit 0 = no rows came in or none is kept (count 0), bit 1 = non-finite centroid,
 * or d_(lo) itself not finite (count 0).
 * in [clouds][cap][stride] + counts (device) -> out [clouds][out_cap][stride]: the kept rows in input order, every column copied;
 * out_counts [clouds] = kept rows, which may exceed out_cap - then the first out_cap are written and the check is the caller's, as
 * with dsir_voxel_downsample.  dirs [clouds][3] fp32 (device): the unit directions, per-cloud numbers the host draws like the
 * rotations; p_keep [clouds] float64 (HOST; each > 0 and finite, else an error before any launch); centroids [clouds][3] float64
 * (device) from dsir_t_cloud_centroids on the same input.
 * Radix select of one rank per cloud (four 8-bit digit histograms, integer LDS atomics), then a stable compaction by per-workgroup
 * counts prefixed in workgroup order: no sort, no floating-point atomics, no atomic that decides a position, no host round trip
 * between the launches.  Two runs write the same bytes and a cloud's output does not depend on the rest of the call.
 * scratch: dsir_t_halfspace_crop_scratch(clouds, cap) bytes (0: shape refused). */
size_t dsir_t_halfspace_crop_scratch(int clouds, int cap);
int dsir_t_halfspace_crop(void* stream, const float* in, const int32_t* counts, int clouds, int cap, int stride, const float* dirs,
                          const double* p_keep, const double* centroids, int out_cap, float* out, int32_t* out_counts, int32_t* invalid,
                          void* scratch);

/* ---- fragment overlap: radius-bounded nearest neighbour of one ragged cloud in another (csrc/overlap.hip) ------------------------
 * The core of the reference's offline dataloader/3DMatch_preprocess.py:82-89 (cv2.BFMatcher.match + distance < voxel size) for every
 * fragment pair of a scene; cv2 is not installable here: parity is unpinned, the engine owns the rule (deepsir_amd/overlap.py,
 * nn_within_host, restates it in numpy float32; the full statement and the lattice argument head csrc/overlap.hip) -
 *   d2 = (dx dx + dy dy) + dz dz, d = b - a, fp32, every operation rounded on its own (the rule of the match lists above);
 *   the neighbour of a is the b of smallest d2, ties to the lower original index of b; a match is d2 < r r, strict, r r one fp32
 *   product; a non-finite a matches nothing, a non-finite b is never a neighbour, an empty side gives count 0; with a pose per
 *   job the query is moved first by the match lists' expression ((T0 x + T1 y) + T2 z) + T3.
 * points [total][stride] (device) holds `fragments` ragged clouds, offsets [fragments + 1] (HOST, int64) their rows; jobs [n_jobs][2]
 * (HOST, int32) = (query fragment, target fragment); bounds [6] (HOST) = min xyz, max xyz over all finite points, which
 * dsir_t_finite_bounds computes on the device (bounds_dev [6] fp32; zeros when no point is finite).
 *
 * dsir_t_nn_within_check (host only, no device call): NULL when the call is acceptable, else the reason - radius <= 0 or not finite,
 * bounds not finite or inverted, an axis that needs more than 2^21 - 2 cells of edge radius (1 + 2^-10), offsets not ascending from 0,
 * more than 2^30 points or 2^20 fragments, a job index outside [0, fragments) (jobs may be NULL to check the index alone), a job
 * list of more than 2^31 - 1 query rows.  Both operators below run it first and return an error WITHOUT a launch when it objects.
 *
 * _index_build: the sparse cell index of every fragment on one lattice, once per call - per fragment its points sorted by a 64-bit
 *   cell key (hipCUB segmented radix sort), xyz + original index as float4, and the fragment's cell box.  index:
 *   dsir_t_nn_index_scratch(total, fragments) bytes (0: shape refused), linear in total, never in the box's cell count.
 * _within: per job, one lane per query point in the query fragment's cell order; 9 key-interval lookups in the target fragment.
 *   counts [n_jobs] (device, required) = matched queries per job (integer adds only); nn (device, may be NULL = count mode):
 *   the jobs' query rows concatenated in job order, nn[row] = original index in the target fragment or -1.  poses (device, may be
 *   NULL) [n_jobs][3][4].  job_scratch: dsir_t_nn_within_scratch(n_jobs) bytes.  The same index, offsets, bounds and radius as _build.
 * No floating-point atomics, no allocation, no host synchronisation between the launches; two runs write the same bytes, and a
 * job's result does not depend on the rest of the list. */
const char* dsir_t_nn_within_check(const int64_t* offsets, int fragments, const int32_t* jobs, int64_t n_jobs, float radius,
                                   const float* bounds);
int dsir_t_finite_bounds(void* stream, const float* points, int stride, int64_t n, float* bounds_dev);
size_t dsir_t_nn_index_scratch(int64_t total, int fragments);
int dsir_t_nn_index_build(void* stream, const float* points, int stride, const int64_t* offsets, int fragments, float radius,
                          const float* bounds, void* index);
size_t dsir_t_nn_within_scratch(int64_t n_jobs);
int dsir_t_nn_within(void* stream, const void* index, const int64_t* offsets, int fragments, const int32_t* jobs, int64_t n_jobs,
                     const float* poses, float radius, const float* bounds, int32_t* counts, int32_t* nn, void* job_scratch);

/* ---- neighbour lists: every neighbour within the radius, or the max_nn nearest, as a CSR (csrc/radius_nn.hip) -----------------------
 * The search over dsir_t_nn_index_build's index that returns ALL neighbours instead of the nearest: what FPFH (dsir_fpfh's csr form),
 * dsir_estimate_normals_csr and any later local-geometry stage read.  The same index, offsets, jobs, poses, radius and bounds as
 * dsir_t_nn_within.  The rule (stated in full at the head of csrc/radius_nn.hip; deepsir_amd/overlap.py::radius_neighbors_host restates it):
 *   the query a is moved first by ((T0 x + T1 y) + T2 z) + T3 when poses are given, read unmoved when poses == NULL;
 *   d2 = (dx dx + dy dy) + dz dz, d = b - a, fp32, every operation rounded on its own; b is a neighbour iff d2 < r r, strict, r r one
 *   fp32 product; a non-finite query has an empty row, a non-finite b is in no row, a query of the target fragment finds itself;
 *   max_nn = 0: the whole ball; max_nn > 0: the max_nn smallest under the order (d2, original index) - min(count, max_nn) entries, a tie
 *   at the boundary goes to the lower index; in both modes a row's columns ascend by original index within the target fragment.
 * rows = the jobs' query rows concatenated in job order (the numbering of dsir_t_nn_within's nn).  Two passes, as the match lists:
 *   _count: counts [rows] and row_offsets [rows + 1] = their exclusive sum, taken with a saturating add: every prefix above
 *           2^31 - 1 is -1, so row_offsets[rows] = the total, or -1 for ANY total that does not fit an int32 (split the job list,
 *           lower the radius or set max_nn; _fill writes nothing for a row whose offsets are -1);
 *           scratch: dsir_t_nn_radius_scratch(n_jobs, rows) bytes (0: refused), it carries the job table over to _fill;
 *   the caller reads row_offsets[rows] from the device and sizes cols (and d2);
 *   _fill:  the SAME arguments, row_offsets and scratch -> cols [n_cols] i32, and d2 [n_cols] fp32 aligned with it unless NULL.
 *           Nothing is written at or past n_cols.
 * For max_nn = 0 and one job (i, j) the CSR is byte for byte dsir_t_radius_matches_count / _fill on the same two clouds.
 * Refused before any launch: what dsir_t_nn_within_check refuses, max_nn < 0, and a job list of more than 2^26 - 1 query rows
 * (one 64-lane workgroup per row).  No atomics, no sort: two runs write the same
 * bytes, and a job's bytes do not depend on the rest of the list. */
size_t dsir_t_nn_radius_scratch(int64_t n_jobs, int64_t rows);
int dsir_t_nn_radius_count(void* stream, const void* index, const int64_t* offsets, int fragments, const int32_t* jobs, int64_t n_jobs,
                           const float* poses, float radius, const float* bounds, int max_nn, int32_t* counts, int32_t* row_offsets,
                           void* scratch);
int dsir_t_nn_radius_fill(void* stream, const void* index, const int64_t* offsets, int fragments, const int32_t* jobs, int64_t n_jobs,
                          const float* poses, float radius, const float* bounds, int max_nn, const int32_t* row_offsets, const void* scratch,
                          int32_t* cols, float* d2, int64_t n_cols);

#ifdef __cplusplus
}
#endif
#endif
