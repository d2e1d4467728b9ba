/* fpc.h — C ABI of libfpc_hip.so: the MI355X (gfx950) implementation of
 * FastPoseCNN's per-frame post-network hot path.
 *
 * This is the drop-in boundary.  Plain pointers and sizes only; no torch types.
 * Every pointer marked "device" must be device-accessible memory of the GPU
 * that is current on the calling thread; every function
 *   - allocates nothing and frees nothing (caller-owned buffers + workspace),
 *   - enqueues its kernels on `stream` (a hipStream_t, passed as void*; NULL is
 *     the default stream) and returns without synchronising,
 *   - returns FPC_OK or a negative FPC_E* code — it never exits the process
 *     (the reference's gpuAssert calls exit(), RV/src/cuda_common.h:17-26).
 *
 * Reference interfaces replaced (paths under /root/reference/source_code/FastPoseCNN,
 * RV = lib/ransac_voting_gpu_layer):
 *   fpc_generate_hypothesis      RV/src/ransac_voting.cpp:20-31  (+ kernel RV/src/ransac_voting_kernel.cu:11-86)
 *   fpc_voting_for_hypothesis    RV/src/ransac_voting.cpp:41-55  (+ kernel .cu:88-167)
 *   fpc_ransac_voting_v3         RV/ransac_voting_gpu.py:518-607 (ransac_voting_layer_v3 + b_inv :503-516)
 *   fpc_class_compress           lib/pose_regressor.py:445-457, lib/gpu_tensor_funcs.py:37-99
 *   fpc_cc_label                 lib/aggregation_layer.py:160-183 (cupyx / scipy ndimage.label)
 *   fpc_aggregate                lib/aggregation_layer.py:61-158
 *   fpc_pose_rt                  lib/gpu_tensor_funcs.py:204-253, 306-326
 *   fpc_pack_pose_records        (none: multi-GPU gather record)
 *   fpc_mask_iou                 lib/gpu_tensor_funcs.py:386-409 (batchwise_get_2d_iou), called by lib/matching.py:264-267
 *   fpc_net_*                    lib/pose_regressor.py:709-743 (+ segmentation_models_pytorch encoder/decoder/head)
 *   fpc_preprocess_u8            tools/dataset.py:249-262 (preprocessing_fn, transpose, / max|.|, img_as_float32)
 *   fpc_png_info / _decode / _decode_batch   tools/dataset.py:158-176 (skimage.io.imread / cv2.imread of *_color / *_mask / *_depth.png)
 *   fpc_png_pack_batch / _decode_device      the same files, inflated and un-filtered on the device (opt-in)
 *   fpc_gt_build / fpc_depth_decode   tools/dataset.py:183-228, 373-434 (class filter and instance_masks of a sample), data_manipulation.py:153-163
 *   fpc_pose_errors              lib/gpu_tensor_funcs.py:411-476, 486-547, 563-565 (degree error, 3-D IoU, offset error)
 *   fpc_pose_metrics_update      lib/metrics.py:11-260, lib/gpu_tensor_funcs.py:611-713, evaluate.py:238-292 (metric accumulators, APs)
 *   fpc_confusion_update         (none: the confusion matrix of the arg-max mask; the reference's mask metrics are Lightning's)
 *   fpc_post_network_backward    torch autograd over lib/aggregation_layer.py:119-156 + RV/ransac_voting_gpu.py:583-599
 *   fpc_vote_refine_backward     torch autograd over RV/ransac_voting_gpu.py:583-599
 *   fpc_class_compress_backward  torch autograd over lib/gpu_tensor_funcs.py:37-99
 *   fpc_mask_losses              lib/loss.py:26-98 (CE, CCE, Focal: forward sums and the combined logit gradient)
 *   fpc_match_assign             lib/matching.py:252-299 (the per-class arg-max and validity of batchwise_find_matches)
 *   fpc_matched_losses           lib/loss.py:272-541 (QLoss, XYLoss, ZLoss, ScalesLoss) + lib/pose_regressor.py:265-307 (task sums)
 *   fpc_matched_losses_backward  torch autograd over the same
 *   fpc_lookahead_radam_step     lib/pose_regressor.py:417-423 (catalyst Lookahead(RAdam)), F/train.py gradient_clip_val,
 *                                lib/pose_regressor.py:341-415 (inf / NaN guard)
 * The Python-side bindings a maintainer would add are shown in INTEGRATION.md.
 */
#ifndef FPC_H_
#define FPC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 11 also covers the Bottleneck encoders (fpc_net_create_encoder, fpc_net_force_pointwise, fpc_conv2d's 4000 + variant),
 * the FPN p2 fold (fpc_net_force_fold) and the three-product direct form (fpc_net_force_direct_h3, fpc_conv2d's 6000 + split and 7000 + parts, fpc_net_graph_recorded):
 * and the stem fused with its max-pool (fpc_net_force_stem_pool, fpc_stem_pool_tasks, fpc_conv2d's 3100):
 * and form -9's packed patch geometry (fpc_wino_pack_geometry, fpc_net_set_wino_pack, fpc_net_wino_blocks, fpc_conv2d's -10):
 * and the activation-range guard of the fp16-piece forms (fpc_act_range, fpc_net_survey_next, fpc_net_guard_ranges, fpc_net_guarded):
 * and the ground-truth batch builder (fpc_gt_build, fpc_depth_decode):
 * and the device PNG decode (fpc_inflate_host, fpc_png_pack_bytes, fpc_png_pack_batch, fpc_png_decode_device and its _workspace_bytes):
 * and the SE-ResNet encoders (fpc_net_create_encoder_se, fpc_se_pool_slabs, fpc_se_scratch_floats, fpc_se_gate, fpc_se_scale_add_relu, fpc_maxpool3x3s2_ceil_fwd):
 * and their gate in the training step (fpc_se_gate_train, fpc_se_bwd_scratch_floats, fpc_se_bwd):
 * and the MobileNetV2 encoder (fpc_net_create's "mobilenet_v2", fpc_dwconv3x3, fpc_conv1x1_f32, fpc_conv1x1_f32_form, fpc_stem3x3s2):
 * and its depthwise convolution and ReLU6 in the training step (fpc_dwconv3x3_dgrad, fpc_dwconv3x3_wgrad and its _workspace_bytes,
 *   fpc_batchnorm_act_fwd, fpc_batchnorm_act_bwd):
 * and the EfficientNet-B0 encoder (fpc_net_create's "efficientnet-b0", fpc_mbconv_dw, fpc_mbconv_gate and its _slabs / _scratch_floats,
 *   fpc_mbconv_pw, fpc_mbconv_pw_form, fpc_mbconv_stem):
 * and the gradients of its depthwise convolution for the training step (fpc_mbconv_dw_dgrad, fpc_mbconv_dw_wgrad and its _workspace_bytes):
 * and the DenseNet-121 / 169 / 201 encoders (fpc_net_create's "densenet121" / "densenet169" / "densenet201", fpc_dense_pw, fpc_dense_pw_form,
 *   fpc_dense_conv3x3, fpc_dense_conv3x3_pack, fpc_dense_conv3x3_form, fpc_dense_norm_pool, fpc_dense_place):
 * and the exit of the four-wave Winograd kernels (fpc_net_set_wino_fast_exit, fpc_wino_tile_patch, fpc_wino_tile_out, fpc_conv2d's -107 .. -113):
 * and the idle wave of the folded s2.0's second phase (fpc_net_set_fold_idle_row):
 * and the VGG encoders (fpc_net_create's "vgg11" .. "vgg19_bn", fpc_conv3x3_c3, fpc_maxpool2x2_fwd):
 * additions only, every earlier entry point keeps its behaviour. */
#define FPC_ABI_VERSION 11

#define FPC_OK 0
#define FPC_EINVAL (-1)      /* bad argument (shape, null pointer, ...) */
#define FPC_EWORKSPACE (-2)  /* workspace too small / misaligned */
#define FPC_ELAUNCH (-3)     /* HIP reported a launch error (hipGetLastError) */
#define FPC_EDEVICE (-4)     /* not running on a gfx950 device / no device */
#define FPC_EFORMAT (-5)     /* fpc_png_*: not a PNG this decoder reads (bad signature / CRC / zlib stream, Adam7, 1-4 bit samples) */

typedef void* fpc_stream_t;  /* hipStream_t */

int fpc_abi_version(void);
const char* fpc_error_string(int code);
/* Text of the last HIP error seen by this thread's failing call ("" if none). */
const char* fpc_last_hip_error(void);

/* ---- B1: the reference extension's two live entry points ------------------
 * direct f32 [tn,vn,2], coords f32 [tn,2] (x = column, y = row), idxs i32 [hn,vn,2]
 * -> hyp f32 [hn,vn,2].  hyp is fully written (zero where the pair is degenerate,
 * as the reference's zero-initialised result tensor).  All device, contiguous. */
int fpc_generate_hypothesis(const float* direct, const float* coords, const int32_t* idxs,
                            float* hyp, int tn, int vn, int hn, fpc_stream_t stream);

/* inliers u8 [hn,vn,tn] is caller-owned and only ever written with 1
 * (the caller pre-zeroes it, RV/ransac_voting_gpu.py:562). */
int fpc_voting_for_hypothesis(const float* direct, const float* coords, const float* hyp,
                              uint8_t* inliers, int tn, int vn, int hn, float inlier_thresh,
                              fpc_stream_t stream);

/* ---- B2: fused ransac_voting_layer_v3 for one keypoint channel ------------
 * mask    f32 [n,H,W] contiguous, foreground iff != 0
 * vertex  base pointer of the [n,H,W,(vn),2] view for the chosen keypoint, with
 *         ELEMENT strides vs_n, vs_h, vs_w, vs_c (the reference passes a permuted
 *         view of two planes, lib/hough_voting.py:51 — no copy is needed)
 * idxs    i32 [n,hn,2] injected pair indices, or NULL -> include/fpc_rng.h stream(seed)
 * keep    u8 [n,H,W] injected thinning selection (used only where fg > max_num), or NULL
 * out_xy  f32 [n,2]
 * optional diagnostics (NULL to skip): out_tn, out_win_idx, out_win_count, out_inl_count i32 [n];
 *         out_hyp f32 [n,hn,2]; out_counts i32 [n,hn] (the exact inlier count of every hypothesis — the path
 *         computes all of them; the diagnostics are copies).
 * n_dev   NULL, or DEVICE i32[1]: only the first min(n, *n_dev) instances are processed (output rows past it are
 *         left untouched).  Lets a caller size buffers by a capacity `n` and enqueue the vote behind
 *         fpc_cc_label without reading the instance count back to the host.
 * hn      1 .. 65536.
 * ws      device workspace of at least fpc_ransac_workspace_bytes(n,H,W,hn) bytes, 256-byte aligned.  Contents
 *         are scratch: nothing has to survive between calls and nothing has to be cleared before one (four stateless
 *         launches on `stream` — eight with the progressive count below —, no memset, no second stream: mask scan +
 *         compacted pixel list -> per-instance plan (hypotheses, work records) -> exact counts on the matrix cores ->
 *         winner + refinement; csrc/ransac.hip, csrc/vote_count.hip).
 * Results are those of the reference's exhaustive vote bit for bit (counts, winner, inlier set); the refinement solves
 * the 2x2 normal equations in fp64 like b_inv (RV/ransac_voting_gpu.py:503-516: inverse, pseudo-inverse when singular),
 * and also takes the pseudo-inverse when det <= 1e-12 trace^2 (conditioning beyond fp64's reach for f32 votes; torch
 * raises only on an exactly singular LU).  An instance above max_num without an injected `keep` / `idxs` draws its
 * pairs by rejection over the kept pixels (include/fpc_rng.h, FPC_SAMPLE_MAX_TRIES). */
size_t fpc_ransac_workspace_bytes(int n, int H, int W, int hn);
int fpc_ransac_voting_v3(const float* mask, const float* vertex,
                         int64_t vs_n, int64_t vs_h, int64_t vs_w, int64_t vs_c,
                         int n, const int32_t* n_dev, int H, int W, int hn,
                         const int32_t* idxs, const uint8_t* keep, uint64_t seed,
                         float inlier_thresh, int min_num, int max_num,
                         float* out_xy, int32_t* out_tn, int32_t* out_win_idx,
                         int32_t* out_win_count, int32_t* out_inl_count,
                         float* out_hyp, int32_t* out_counts, double* out_refine,
                         void* ws, size_t ws_bytes, fpc_stream_t stream);
/* The same with the foreground ALSO given as bit words (fpc_aggregate_bits' inst_bits: u64 [n][fpc_mask_bits_words(H,W)],
 * 8-byte aligned): when mask_bits is not NULL the f32 `mask` planes are not read (mask may then be NULL) — two thirds of
 * the mask scan's bytes at a typical foreground share.  The caller guarantees bit == (mask != 0); results are identical. */
int fpc_ransac_voting_v3_bits(const float* mask, const uint64_t* mask_bits, const float* vertex,
                              int64_t vs_n, int64_t vs_h, int64_t vs_w, int64_t vs_c,
                              int n, const int32_t* n_dev, int H, int W, int hn,
                              const int32_t* idxs, const uint8_t* keep, uint64_t seed,
                              float inlier_thresh, int min_num, int max_num,
                              float* out_xy, int32_t* out_tn, int32_t* out_win_idx,
                              int32_t* out_win_count, int32_t* out_inl_count,
                              float* out_hyp, int32_t* out_counts, double* out_refine,
                              void* ws, size_t ws_bytes, fpc_stream_t stream);

/* The same with the RT assembly of fpc_pose_rt appended (round 6: one launch less per frame — the post-network path at batch 1 is a
 * chain of launch latencies): when the six pose pointers are given (all or none), the workgroup of k_vote_final that writes an
 * instance's out_xy also writes R [n][9], T [n][3], RT [n][16] from (out_xy, pose_q [n][4] scalar-last, pose_z [n], pose_kinv [9]) —
 * the same function, the same bits as fpc_pose_rt on the same operands (F/lib/gpu_tensor_funcs.py:204-235 after
 * F/lib/hough_voting.py:33-63).  Rows at or beyond *n_dev are not written. */
int fpc_ransac_voting_v3_pose(const float* mask, const uint64_t* mask_bits, const float* vertex,
                              int64_t vs_n, int64_t vs_h, int64_t vs_w, int64_t vs_c,
                              int n, const int32_t* n_dev, int H, int W, int hn,
                              const int32_t* idxs, const uint8_t* keep, uint64_t seed,
                              float inlier_thresh, int min_num, int max_num,
                              float* out_xy, int32_t* out_tn, int32_t* out_win_idx,
                              int32_t* out_win_count, int32_t* out_inl_count,
                              float* out_hyp, int32_t* out_counts, double* out_refine,
                              const float* pose_q, const float* pose_z, const float* pose_kinv,
                              float* pose_R, float* pose_T, float* pose_RT,
                              void* ws, size_t ws_bytes, fpc_stream_t stream);

/* The progressive count (OFF by default).  Unless the caller asks for out_counts, only the WINNER of the vote is an output
 * (RV/ransac_voting_gpu.py:566-574: arg-max of the inlier counts, first maximum).  With fpc_vote_set_prune(1, ...) the count
 * runs in passes over disjoint sets of each instance's pixels; between two passes every hypothesis h with
 *     count_so_far(h) + valid pixels not yet counted  <  L      (or == L with an index above the leader's)
 * is dropped, L being the EXACT final count of the current leader (csrc/ransac.hip: k_vote_lead).  The winner, its count,
 * its inlier set and the refined centre are those of the exhaustive vote, bit for bit; out_win_idx / out_win_count /
 * out_inl_count stay available.  With out_counts the exhaustive count runs.  Measured on the 32-frame batch at hn = 1000:
 * 0.55 of the pairs, but 326 us against the exhaustive 283 us (three count launches and two k_vote_lead launches cost more
 * than the pairs they save: profiles/r05_vote_prune.md) - hence off unless asked for.
 * fpc_vote_set_prune: mode 0 = never (default), 1 = whenever out_counts is NULL and the sizes fit (n <= 1024 instances,
 * <= 8.4 M pixels).  npass = 0 keeps the schedule; else 2..4 passes, cum16[npass - 1] = increasing 16ths of an
 * instance's count units finished after each pass but the last (default 3 passes: 5, 10).  Process-wide.
 * fpc_vote_prune_info: copy of the last call's per-instance record out of its workspace -> out i32 [n,8] (device):
 * {-, count units, alive hypotheses entering the last pass, their 32-wide tiles, last leader, its final count L,
 * valid pixels that were still uncounted at the last decision, -}. */
int fpc_vote_set_prune(int mode, int npass, const int32_t* cum16);
int fpc_vote_prune_info(const void* ws, size_t ws_bytes, int n, int H, int W, int hn, int32_t* out, fpc_stream_t stream);

/* ---- class compression ------------------------------------------------------
 * mask_logits f32 [B,C,HW]; quat [B,4(C-1),HW]; scales [B,3(C-1),HW]; xy [B,2(C-1),HW];
 * z [B,(C-1),HW]; cat_mask_in i64 [B,HW] or NULL (NULL: arg-max of log-softmax, first
 * maximal index on ties; mask_logits may be NULL when cat_mask_in is given).
 * -> cat_mask i64 [B,HW], oq [B,4,HW], os [B,3,HW], oxy [B,2,HW], oz [B,HW]. */
int fpc_class_compress(const float* mask_logits, const float* quat, const float* scales,
                       const float* xy, const float* z, const int64_t* cat_mask_in,
                       int B, int C, int HW,
                       int64_t* cat_mask, float* oq, float* os, float* oxy, float* oz,
                       fpc_stream_t stream);
/* The same, also writing the foreground (cat_mask != 0) as bit words for fpc_cc_label_bits: fg_bits u64
 * [B][fpc_mask_bits_words-style stride = ceil(HW / 4096) * 64], bit j of word w = pixel 64 w + j; words past ceil(HW / 64)
 * are not written.  NULL fg_bits = fpc_class_compress. */
int fpc_class_compress_bits(const float* mask_logits, const float* quat, const float* scales,
                            const float* xy, const float* z, const int64_t* cat_mask_in,
                            int B, int C, int HW,
                            int64_t* cat_mask, float* oq, float* os, float* oxy, float* oz,
                            uint64_t* fg_bits, fpc_stream_t stream);


/* ---- connected components ---------------------------------------------------
 * cat_mask i64 [B,H,W]; foreground iff != 0; 4-connectivity inside an image, none
 * across images.  labels i32 [B,H,W]: 0 background, 1..N numbered in raster order of
 * each component's first pixel, continuing across the batch (scipy.ndimage.label order).
 * n_out: DEVICE i32[1] receiving N.  root_pix: DEVICE i32 [cap] (nullable) receiving the
 * linear index (over B*H*W) of each component's first pixel for labels 1..min(N,cap). */
size_t fpc_cc_workspace_bytes(int B, int H, int W);
int fpc_cc_label(const int64_t* cat_mask, int B, int H, int W,
                 int32_t* labels, int32_t* n_out, int32_t* root_pix, int cap,
                 void* ws, size_t ws_bytes, fpc_stream_t stream);
/* The same labelling from the foreground as BIT WORDS: fg_bits u64 [B][fpc_mask_bits_words(H, W)], bit j of word w = pixel
 * 64 w + j of the image, zero past H W (8-byte aligned).  No reference counterpart: the reference hands cupy an f32 copy of
 * the mask (F/lib/aggregation_layer.py:165); here the class compression (fpc_class_compress_bits, the network engine) writes
 * the words beside the i64 mask and the labelling never reads the mask itself — 1/64 of its bytes, two launches.  Available
 * when fpc_cc_bits_supported(B, H, W) (rows on word boundaries: W % 64 == 0, and an image whose words fit one workgroup's LDS:
 * up to ~630 000 pixels); fpc_cc_label takes the same path by itself on such shapes after converting the mask (fpc_fg_bits). */
int fpc_cc_bits_supported(int B, int H, int W);
int fpc_fg_bits(const int64_t* cat_mask, int B, int H, int W, uint64_t* fg_bits, fpc_stream_t stream);
int fpc_cc_label_bits(const uint64_t* fg_bits, int B, int H, int W, int32_t* labels, int32_t* n_out,
                      int32_t* root_pix, int cap, void* ws, size_t ws_bytes, fpc_stream_t stream);


/* ---- aggregation ------------------------------------------------------------
 * labels i32 [B,H,W] from fpc_cc_label, N instances (host value: the count read back by the caller,
 * or a capacity when n_dev — DEVICE i32[1], fpc_cc_label's n_out — is given: then only the first
 * min(N, *n_dev) instances are produced and the remaining rows are left untouched), categorical planes quat [B,4,HW], scales [B,3,HW], xy [B,2,HW], z [B,HW].
 * -> class_ids i64 [N], sample_ids i64 [N], inst_masks f32 [N,HW] (nullable),
 *    oq [N,4], os [N,3], oz [N], oxy f32 [N,2,HW] (nullable), out_stats f32 [N,2] (nullable: pixel count and the norm
 *    of the mean quaternion before normalisation — what fpc_post_network_backward's table is built from). */
size_t fpc_aggregate_workspace_bytes(int N);
int fpc_aggregate(const int32_t* labels, const int64_t* cat_mask,
                  const float* quat, const float* scales, const float* xy, const float* z,
                  int B, int H, int W, int N, const int32_t* n_dev,
                  int64_t* class_ids, int64_t* sample_ids, float* inst_masks,
                  float* oq, float* os, float* oz, float* oxy, float* out_stats,
                  void* ws, size_t ws_bytes, fpc_stream_t stream);
/* The same, and — when inst_bits is not NULL — every instance's foreground also as bit words u64
 * [N][fpc_mask_bits_words(H, W)] (bit j of word w = pixel 64 w + j, zero past H W; whole 4096-pixel chunks): 1/32 of
 * the f32 mask plane, which fpc_ransac_voting_v3_bits reads INSTEAD of it.  No reference counterpart: the reference's
 * voting re-reads the f32 masks its aggregation has just written (lib/hough_voting.py:41-63).
 * root_pix (nullable): fpc_cc_label's root_pix with at least N valid entries (its cap >= N).  With it the image of an
 * instance is known without the accumulation, and accumulation and planes run as ONE launch. */
size_t fpc_mask_bits_words(int H, int W);
int fpc_aggregate_bits(const int32_t* labels, const int64_t* cat_mask,
                       const float* quat, const float* scales, const float* xy, const float* z,
                       int B, int H, int W, int N, const int32_t* n_dev,
                       int64_t* class_ids, int64_t* sample_ids, float* inst_masks,
                       float* oq, float* os, float* oz, float* oxy, float* out_stats, uint64_t* inst_bits,
                       const int32_t* root_pix, void* ws, size_t ws_bytes, fpc_stream_t stream);

/* ---- pose assembly ----------------------------------------------------------
 * q f32 [n,4] scalar-last, xy [n,2], z [n], kinv f32 [9] row-major (device)
 * -> R [n,9], T [n,3], RT [n,16]. */
int fpc_pose_rt(const float* q, const float* xy, const float* z, const float* kinv, int n,
                float* R, float* T, float* RT, fpc_stream_t stream);

/* ---- multi-GPU pose records ---------------------------------------------------
 * No reference counterpart (its evaluate / inference scripts are single-GPU, evaluate.py:90,127): one rank's
 * per-instance results as fixed-width records for ONE all-gather (fastposecnn_amd/parallel.py).
 * out f32 [capacity+1][40]: row 0 = {n as int32 bits, 0...}; row 1+i = {sample_id + sample_offset, class_id (int32
 * bits), quaternion[4], scales[3], xy[2], z[1], R[9], T[3], RT[16]}; rows past n are zero.  n <= capacity. */
int fpc_pack_pose_records(const int64_t* sample_ids, const int64_t* class_ids, const float* q, const float* scales,
                          const float* xy, const float* z, const float* R, const float* T, const float* RT, int n,
                          int sample_offset, int capacity, float* out, fpc_stream_t stream);

/* ---- matching: 2D IoU of every (mask1, mask2) pair ----------------------------
 * lib/gpu_tensor_funcs.py:386-409 batchwise_get_2d_iou (the [n1,n2,H,W] logical_and / logical_or expansion
 * of lib/matching.py:264-267).  masks1 [n1,hw], masks2 [n2,hw]: contiguous, elem_size 4 (f32: non-zero
 * incl. NaN = set, -0.0 = clear) or 1 (u8 / bool).  iou f32 [n1,n2] = (float)|a & b| / (float)|a | b|
 * (NaN for two empty masks, as torch's 0/0); inter / uni i32 [n1,n2] optional (NULL).  n1 == 0 or n2 == 0: no-op. */
size_t fpc_mask_iou_workspace_bytes(int n1, int n2, int64_t hw);
int fpc_mask_iou(const void* masks1, int n1, const void* masks2, int n2, int64_t hw, int elem_size,
                 float* iou, int32_t* inter, int32_t* uni, void* ws, size_t ws_bytes, fpc_stream_t stream);

/* ---- input side: colour frame -> network tensor --------------------------------
 * tools/dataset.py:249-262 on the device.  img_hwc u8 [B,H,W,3] (device, 16-byte aligned; RGB as skimage.io.imread
 * returns it), mean3 / std3 HOST doubles (smp's preprocessing parameters of the encoder: imagenet 0.485 0.456 0.406 /
 * 0.229 0.224 0.225), input_range_01 != 0: smp's rule "x / 255 when x.max() > 1" applies.
 * -> out f32 [B,3,H,W] = float32( ((x [/ 255]) - mean) / std / max|.| ), all in IEEE double with one final rounding:
 * bit-identical to the reference's numpy chain.  For B > 1: H*W % 4 == 0 and (3*H*W) % 16 == 0. */
size_t fpc_preprocess_workspace_bytes(int B);
int fpc_preprocess_u8(const uint8_t* img_hwc, int B, int H, int W, const double* mean3, const double* std3,
                      int input_range_01, float* out_nchw, void* ws, size_t ws_bytes, fpc_stream_t stream);

/* ---- frame decoding, HOST side (tools/dataset.py:158-176: skimage.io.imread / cv2.imread of the NOCS *_color.png,
 * *_mask.png, *_depth.png) -------------------------------------------------------------------------------------------
 * PNG (ISO/IEC 15948) through zlib: colour types 0 / 2 / 3 / 4 / 6, 8 or 16 bits per sample, non-interlaced; anything
 * else (and any damaged file: signature, chunk CRC, zlib stream, filter type) is FPC_EFORMAT.  Host pointers, no stream.
 * fpc_png_info: out5 = {width, height, bit depth, colour type, channels of the mode-0 output}.
 * fpc_png_decode mode 0: the samples as stored, [H, W, C] u8 — or u16 in host byte order for 16-bit files; a palette is
 *   expanded to RGB8 — exactly what imread returns; mode 3: RGB8 whatever the file holds (grey replicated, alpha
 *   dropped, 16-bit samples by their high byte).  out_bytes is checked.
 * fpc_png_decode_batch: n files of ONE size H x W -> out u8 [n, H, W, 3] (mode 3), decoded by `threads` host threads
 *   (the calling thread included); out is typically FrameUploader's pinned staging slot. */
int fpc_png_info(const uint8_t* data, size_t nbytes, int32_t* out5);
int fpc_png_decode(const uint8_t* data, size_t nbytes, void* out, size_t out_bytes, int mode);
int fpc_png_decode_batch(const uint8_t* const* datas, const size_t* sizes, int n, uint8_t* out, int H, int W, int threads);

/* ---- frame decoding, DEVICE side (ABI 11 addition; opt-in, the host decoder above is untouched) --------------------
 * The host walks the container and copies the COMPRESSED bytes; the device inflates (csrc/inflate.hpp, RFC 1950/1951,
 * no zlib) and un-filters (csrc/png_device.hip: k_png_inflate, one wave per file; k_png_unfilter).
 *
 * fpc_inflate_host: the same inflate.hpp on the host.  `in` [zbytes]: a zlib stream; `out` [cap]: cap is the EXPECTED
 * size (a PNG's H (1 + W bpp)); *out_len (may be NULL) = bytes produced, also on failure.  Returns 0, FPC_EINVAL, or a
 * positive FPC_INF_* status, one per failure class.  Reads only [in, in + zbytes), writes only [out, out + cap); total
 * work is bounded by a constant times 8 zbytes + cap for any bytes.
 *
 * fpc_png_pack_batch: HOST.  n files of ONE size H x W (mode 0: also one bit depth and one mode-0 channel count), else
 * FPC_EINVAL with nothing written.  Signature, IHDR and every chunk CRC are checked as fpc_png_decode does (FPC_EFORMAT);
 * the IDAT payloads of file i are copied back to back to staging + desc[i][0] (a multiple of 16; the slice is zero-
 * padded to 16 bytes and, for a palette file, followed by 768 palette bytes).  staging: 16-byte aligned (pinned, for
 * an asynchronous copy), *used = bytes to copy to the device.  FPC_EWORKSPACE when staging_bytes does not hold the
 * payloads.  desc: int64 [n][FPC_PNG_DESC_WORDS] = {staging offset, compressed bytes, width, height, bit depth,
 * colour type, channels per pixel in the file, palette entries}.
 * fpc_png_pack_bytes(n, H, W): a staging size for n files, per file the raw scanlines at 8 bytes a pixel + 1/8 + 1024 +
 * the palette: no deflate stream that carries data can exceed it (stored blocks cost 5 bytes per 65535); a file padded
 * with empty blocks beyond it is refused by fpc_png_pack_batch with FPC_EWORKSPACE.
 *
 * fpc_png_decode_device: staging [staging_bytes] and desc as packed, DEVICE copies.  out: DEVICE, file i at
 * out + i * frame_bytes: mode 3 RGB8 [H][W][3] as fpc_png_decode mode 3; mode 0 the samples as stored (u16 LITTLE-
 * endian for 16-bit files, a palette expanded to RGB8).  status i32 [n] DEVICE: 0, an FPC_INF_* status, FPC_PNG_EDESC
 * (a descriptor that does not fit the call: size, max_bpp, staging_bytes, frame_bytes) or FPC_PNG_EFILTER (a filter
 * byte > 4); a file with a non-zero status leaves its frame of `out` unwritten (FPC_PNG_EFILTER: written, the row read
 * as filter 0) and never touches another file's bytes.  max_bpp: the largest bytes-per-pixel among the files (1 .. 8);
 * workspace >= fpc_png_decode_device_workspace_bytes(n, H, W, max_bpp), 16-byte aligned.  W * max_bpp <= 32768.
 * FPC_EINVAL before any launch: NULL or misaligned pointers (staging, out, workspace 16; desc 8; status 4), n < 1,
 * any total size from 2^31 bytes on.  Results are bit-identical run to run.  No synchronisation. */
#define FPC_PNG_DESC_WORDS 8
#define FPC_INF_ETRUNCATED 1
#define FPC_INF_EBLOCK_TYPE 2
#define FPC_INF_ESTORED_LEN 3
#define FPC_INF_EOVERSUBSCRIBED 4
#define FPC_INF_EINCOMPLETE 5
#define FPC_INF_EREPEAT_FIRST 6
#define FPC_INF_ELITLEN_SYMBOL 7
#define FPC_INF_EDIST_SYMBOL 8
#define FPC_INF_EDIST_TOO_FAR 9
#define FPC_INF_EOUT_OVERFLOW 10
#define FPC_INF_EOUT_SHORT 11
#define FPC_INF_EADLER 12
#define FPC_INF_EFDICT 13
#define FPC_INF_EMETHOD 14
#define FPC_INF_EFCHECK 15
#define FPC_INF_ELENGTHS_OVERRUN 16
#define FPC_INF_ENO_END_CODE 17
#define FPC_INF_EBAD_CODE 18
#define FPC_PNG_EDESC 20
#define FPC_PNG_EFILTER 21
int fpc_inflate_host(const uint8_t* in, size_t zbytes, uint8_t* out, size_t cap, size_t* out_len);
size_t fpc_png_pack_bytes(int n, int H, int W);
int fpc_png_pack_batch(const uint8_t* const* datas, const size_t* sizes, int n, int H, int W, int mode, uint8_t* staging,
                       size_t staging_bytes, int64_t* desc, size_t* used);
size_t fpc_png_decode_device_workspace_bytes(int n, int H, int W, int max_bpp);
int fpc_png_decode_device(const uint8_t* staging, size_t staging_bytes, const int64_t* desc, int n, int H, int W, int mode,
                          int max_bpp, void* out, size_t frame_bytes, int32_t* status, void* workspace, size_t workspace_bytes,
                          fpc_stream_t stream);

/* ---- ground-truth side: instance-id masks -> the batch's class mask and per-instance planes (ABI 11 addition) -------
 * tools/dataset.py: __getitem__'s class filter and generate_agg_data's instance_masks for B frames in one launch
 * (csrc/gt_build.hip).  ids: DEVICE bytes, the id of pixel p of frame b is ids[b * frame_stride + p * pix_stride]
 * (pix_stride 1: a grey mask; 4: the CAMERA set's RGBA mask files as decoded, the other channels are ignored).
 * row_of i16 [B][256]: the row of agg_data (0 .. n-1) of this id in this frame, or -1; class_of u8 [B][256]: its class
 * index, 0 = background / not wanted; first_row i32 [B+1]: the rows of frame b are first_row[b] .. first_row[b+1] - 1
 * (contiguous, ascending).  All three DEVICE.  The kernel applies the tables and nothing else (id 255 is background by
 * the caller's tables).
 * -> class_mask i64 [B,H,W] = class_of[b][id]; inst_masks [n,H,W] of f64 / f32 / u8 (mask_elem 8 / 4 / 1; 16-byte
 *    aligned): 1 where row_of[b][id] == r, else 0, every plane of a frame's rows written in full; pix_count i32 [n]: set
 *    pixels per row (zeroed on the stream by the entry).  Each output is optional (NULL).  Rows >= n are never touched;
 *    n == 0 still writes the class mask.  Bytes written: n H W mask_elem + 8 B H W.
 * FPC_EINVAL before any launch: NULL ids / tables, B < 1, H < 1, W < 1, n < 0, n > 32767, pix_stride outside 1 .. 4,
 * inst_masks given with another mask_elem or not 16-byte aligned, H W or the grid beyond 2^31. */
int fpc_gt_build(const uint8_t* ids, int64_t pix_stride, int64_t frame_stride, int B, int H, int W,
                 const int16_t* row_of, const uint8_t* class_of, const int32_t* first_row, int n,
                 int64_t* class_mask, void* inst_masks, int mask_elem, int32_t* pix_count, fpc_stream_t stream);
/* The batch's `depth` key: standardize_depth(...).astype('float32') of tools/dataset.py.  src_kind 0: u8 [B,H,W,channels]
 * (channels 3 or 4, R,G,B(,A)): G * 256 + R; src_kind 1: u16 [B,H,W].  -> depth_f32 [B,H,W].  All DEVICE. */
int fpc_depth_decode(const void* src, int src_kind, int channels, int B, int H, int W, float* depth_f32, fpc_stream_t stream);

/* ---- evaluation maths on matched pairs (lib/gpu_tensor_funcs.py:411-476, 486-547, 563-565) ----------------------
 * One launch for n (ground truth, prediction) pairs; every output is optional (NULL skips it and its inputs).
 * out_degree f64 [n]: get_raw_quat_distance (computed in f32) where symmetric_ids[i] == 0 or symmetric_ids is NULL,
 *   else get_symmetric_quat_distance over the nrot rotations rot f32 [nrot,4] (quat_symmetric_tf's table), in f64.
 *   Pair order is the input order (the Python wrapper applies the reference's non-symmetric-first concatenation).
 * out_iou3d f32 [n]: get_asymmetric_3d_iou(RT1, RT2, scales1, scales2), RT f32 [n,4,4], scales f32 [n,3].
 * out_offset f32 [n]: |T1 - T2| * 10, T f32 [n,3]. */
int fpc_pose_errors(const float* q0, const float* q1, const int64_t* symmetric_ids, const float* rot, int nrot,
                    const float* RT1, const float* RT2, const float* scales1, const float* scales2,
                    const float* T1, const float* T2, int n, double* out_degree, float* out_iou3d, float* out_offset,
                    fpc_stream_t stream);

/* ---- evaluation metrics accumulated on the device (lib/metrics.py:11-260, lib/gpu_tensor_funcs.py:611-713,
 * evaluate.py:238-292) ----------------------------------------------------------------------------------------------
 * fpc_pose_metrics_update folds the matched pairs (g, match_pred[g]), g = order[0..count), of ONE fpc_match_assign into a
 * persistent device state: one launch of one workgroup, nothing read back.  Per pair it takes fpc_pose_errors' three
 * errors (same device functions, csrc/pose_errors.hpp) from the ground truth's quaternion f32 [n1,4], RT f32 [n1,4,4],
 * scales f32 [n1,3], T f32 [n1,3], symmetric_ids i64 [n1], class_ids i64 [n1] and the predictions' f32 [n2,..] arrays.
 *
 * state i64 [fpc_pose_metrics_state_words(C, n_deg, n_iou, n_off, K)], zero-initialised by the caller; M = metric 0 degree,
 * 1 IoU, 2 offset; words marked f64 hold a double's bits:
 *   [0] updates with count > 0   [1] pairs left out of the per-class words (class id outside 1..C-1)
 *   [2] raw-log cursor (pairs offered so far)   [3] raw-log overflow (pairs offered beyond raw_capacity)
 *   [4],[5] DegreeErrorMeanAP correct, total (NaN pairs leave total)   [6],[7] Iou3dAP   [8],[9] OffsetAP (NaN pairs stay in total)
 *   [10] f64 DegreeError   [11] f64 Iou3dAccuracy   [12] f64 OffsetError: state = (state + this update's value) / 2
 *   [13..15] reserved (0)
 *   [16 + 6 c + 2 M], [.. + 1]          class c: non-NaN samples, NaN samples of metric M
 *   [16 + 6 C + c (n_deg + n_iou + n_off) + j]   class c: hits of threshold j (degree's, then IoU's, then offset's)
 *   [16 + 6 C + C (n_deg + n_iou + n_off) + c K + k]   class c: pairs with degree < thr_complex[k] and offset < thr_complex[K + k]
 * A hit is error < threshold (degree, offset) or error > threshold (IoU), strict, the error widened to f64; a NaN never hits.
 * thr_degree / thr_iou / thr_offset f64 [n_*], thr_complex f64 [2,K], thr_table f64 [3] (the thresholds of words 4-9), on
 * the device.  This update's values for words 10-12: the mean of the non-NaN degree errors, the mean of IoU * 100 (f32
 * product, NaN propagates), and from_RTs_get_T_offset_errors: ONE distance over all pairs between the camera origins
 * under inverse(RT), times 10.  Their sums run over the pairs in `order` order in f64, so two runs give the same bits.
 * count == 0 writes nothing at all (words 10-12 are not halved).  A class id outside 1..C-1 is never an index: the pair
 * still enters words 2-12 and the raw log, and is counted in word 1.
 * Raw log (raw_capacity > 0): raw_degree f64, raw_iou f32, raw_offset f32, raw_class i32, each [raw_capacity]; the pairs go
 * to cursor, cursor + 1, .. in `order` order while they fit.
 * Limits as fpc_match_assign: n1, n2 <= FPC_MATCH_MAX_INSTANCES; also 2 <= C <= 4096 and n_deg + n_iou + n_off + K <= 4096
 * (FPC_EINVAL before any launch). */
size_t fpc_pose_metrics_state_words(int num_classes, int n_deg, int n_iou, int n_off, int n_complex);
int fpc_pose_metrics_update(const int32_t* order, const int32_t* match_pred, const int32_t* count, int n1, int n2,
                            const float* gt_quaternion, const float* gt_RT, const float* gt_scales, const float* gt_T,
                            const int64_t* symmetric_ids, const int64_t* class_ids, const float* quaternion, const float* RT,
                            const float* scales, const float* T, const float* rot, int nrot, const double* thr_degree, int n_deg,
                            const double* thr_iou, int n_iou, const double* thr_offset, int n_off, const double* thr_complex,
                            int n_complex, const double* thr_table, int num_classes, int64_t* state, double* raw_degree,
                            float* raw_iou, float* raw_offset, int32_t* raw_class, int raw_capacity, fpc_stream_t stream);

/* Confusion matrix of two label planes: pred, gt i64 [n] (n = B * H * W), state i64 [C * C + 1], C <= 32.
 * state[gt * C + pred] += 1 for every pixel with both labels in [0, C); state[C * C] += the pixels left out (ignore
 * labels, negative values).  Integer atomics only; any n >= 0. */
int fpc_confusion_update(const int64_t* pred, const int64_t* gt, int64_t n, int num_classes, int64_t* state, fpc_stream_t stream);

/* ---- training: backward of the post-network path, optimiser step ----------------
 * fpc_post_network_backward: labels i32 [B,H,W] (fpc_cc_label), cat_xy f32 [B,2,H,W] (the categorical vote planes the
 * forward aggregated), table f64 [N,16] per instance: [0..3] dL/d(pixel quaternion), [4..6] dL/d(pixel scales),
 * [7] dL/d(pixel z) (the instance gradients chained through the mean / normalise / exp and divided by the pixel count),
 * [8..9] lam = (sum n n^T)^-1 dL/dxy, [10..11] the refined xy, [12..13] the winning hypothesis, [14] foreground count,
 * [15] != 0: the instance voted.  inlier_thresh / max_num / seed / keep: as in the forward fpc_ransac_voting_v3 call.
 * -> g_q [B,4,H,W], g_s [B,3,H,W], g_xy [B,2,H,W], g_z [B,H,W]: every element written.
 * fpc_vote_refine_backward: the vote term alone on the forward's mask [n,H,W] / vertex planes; table f64 [n,8]:
 * lam(2), refined xy(2), winner(2), foreground count, active.  -> g_vertex f32 [n,2,H,W].
 * fpc_ransac_voting_v3's out_refine f64 [n,8] = winner(2), a00, a01, a11, b0, b1, inliers supplies the normal equations.
 * fpc_class_compress_backward: go_* gradients of the four categorical outputs (NULL = zero) -> dense gradients of the four
 * logit tensors (layouts of fpc_class_compress). */
int fpc_post_network_backward(const int32_t* labels, const float* cat_xy, int B, int H, int W, int N,
                              const int32_t* n_dev, const double* table, float inlier_thresh, int max_num,
                              uint64_t seed, const uint8_t* keep, float* g_q, float* g_s, float* g_xy, float* g_z,
                              fpc_stream_t stream);
int fpc_vote_refine_backward(const float* mask, const float* vertex, int64_t vs_n, int64_t vs_h, int64_t vs_w,
                             int64_t vs_c, int n, int H, int W, const double* table, float inlier_thresh, int max_num,
                             uint64_t seed, const uint8_t* keep, float* g_vertex, fpc_stream_t stream);
int fpc_class_compress_backward(const int64_t* cat_mask, const float* quat, const float* xy, const float* go_q,
                                const float* go_s, const float* go_xy, const float* go_z, int B, int C, int HW,
                                float* g_q, float* g_s, float* g_xy, float* g_z, fpc_stream_t stream);
/* The three mask losses of lib/loss.py:26-98 (CE, CCE, Focal on log-softmax outputs) on logits f32 [B,C,HW] and target
 * i64 [B,HW], one pass.  grad == NULL: forward, sums6 f64 [6] (caller zeroes) += CE sum, CE count, CCE sum, CCE count,
 * Focal sum, Focal count (each loss = sum / count).  grad != NULL: backward, grad f32 [B,C,HW] = d/dlogits of
 * w3[0] * (CE sum) + w3[1] * (CCE sum) + w3[2] * (Focal sum), w3 DEVICE f32 [3] (upstream gradient / count). */
int fpc_mask_losses(const float* logits, const int64_t* target, int B, int C, int HW, int64_t ignore_ce,
                    int64_t ignore_cce, float alpha, float gamma, double* sums6, const float* w3, float* grad,
                    fpc_stream_t stream);
/* ---- training: instance matching and the matched losses, results left on the device (csrc/match_loss.hip) ----------
 * fpc_match_assign: the assignment half of matching.batchwise_find_matches.  iou f32 [n1,n2] row-major (fpc_mask_iou),
 * gt_cls i64 [n1], pred_cls i64 [n2].  For ground truth i the candidates are the predictions j with pred_cls[j] ==
 * gt_cls[i] in ascending j; the winner is torch.max's (the first index of the maximum; a NaN among the candidates makes
 * the maximum NaN) and i is matched iff the maximum is > 0.  match_pred i32 [n1]: the winner or -1.  order i32 [n1]:
 * order[0..count) = the matched ground-truth indices in the reference's output order (ascending class id, then ascending
 * i), the rest -1.  count i32 [1].  One launch of one workgroup.
 * n1 and n2 are limited to FPC_MATCH_MAX_INSTANCES each (FPC_EINVAL beyond it, before any launch; this holds for the two
 * entries below as well).  n1 == 0 is a no-op. */
#define FPC_MATCH_MAX_INSTANCES 1024
int fpc_match_assign(const float* iou, const int64_t* gt_cls, const int64_t* pred_cls, int n1, int n2, int32_t* match_pred,
                     int32_t* order, int32_t* count, fpc_stream_t stream);
/* The four matched losses of the criterion table over the pairs (i, match_pred[i]), i in order[0..count): ground truth
 * gt_quaternion [n1,4], gt_xy [n1,2], gt_z [n1,1], gt_scales [n1,3] and symmetric_ids i64 [n1]; predictions quaternion
 * [n2,4], xy [n2,2], z [n2,1], scales [n2,3]; all f32.  rot f32 [nrot,4]: quat_symmetric_tf's table, as fpc_pose_errors
 * takes it.  *_type: FPC_LOSS_* of XYLoss / ZLoss / ScalesLoss.  weights: HOST f64 [4], read during the call.
 * losses f64 [4] = QLoss, XYLoss, ZLoss, ScalesLoss:
 *   QLoss   per pair log(1 - dot^2 + eps) - log(eps): the f32 dot where symmetric_ids == 0, else the minimum over the nrot
 *           rotations of the ground truth (rotated and normalised in f64; the first minimum wins, a NaN among them makes
 *           the pair NaN); NaN pairs are dropped before the mean, no pair left gives NaN.
 *   XY / Scales   sum over the components of the mean over the pairs of L2 / L1 / SmoothL1(beta = 1); Z the same on
 *           log(gt), log(pred).  No NaN filter.
 *   count == 0: all four are NaN.
 * task_total f64 [4] = weights[k] * losses[k] (NaN where the loss is NaN); matched_total f64 [1] = the sum of the non-NaN
 * task totals (0 without any).  best_rot i32 [n1]: per ground truth the winning rotation of a symmetric pair, 0 for a
 * plain pair, -1 where the pair was dropped as NaN or the ground truth is unmatched (kept for the backward). */
#define FPC_LOSS_L2 0
#define FPC_LOSS_L1 1
#define FPC_LOSS_SMOOTH_L1 2
int fpc_matched_losses(const int32_t* order, const int32_t* match_pred, const int32_t* count, int n1, int n2,
                       const float* gt_quaternion, const float* gt_xy, const float* gt_z, const float* gt_scales,
                       const int64_t* symmetric_ids, const float* quaternion, const float* xy, const float* z,
                       const float* scales, const float* rot, int nrot, double eps, int xy_type, int z_type, int scales_type,
                       const double* weights, double* losses, double* task_total, double* matched_total, int32_t* best_rot,
                       fpc_stream_t stream);
/* d(sum_k g_losses[k] * losses[k]) / d(predictions): the forward's inputs, its outputs losses and best_rot, and g_losses
 * f64 [4] on the device.  Every element of g_quaternion [n2,4], g_xy [n2,2], g_z [n2,1], g_scales [n2,3] (f32) is written;
 * an unmatched prediction gets 0, a prediction matched by several ground truths the sum of their terms in `order` order
 * (no atomics: two runs are bit-identical).  A loss that was NaN in the forward and a QLoss pair that was dropped
 * contribute exactly 0 (their terms are skipped, not multiplied by 0).  Symmetric pairs: through best_rot only. */
int fpc_matched_losses_backward(const int32_t* order, const int32_t* match_pred, const int32_t* count, int n1, int n2,
                                const float* gt_quaternion, const float* gt_xy, const float* gt_z, const float* gt_scales,
                                const int64_t* symmetric_ids, const float* quaternion, const float* xy, const float* z,
                                const float* scales, const float* rot, int nrot, double eps, int xy_type, int z_type,
                                int scales_type, const double* weights, const double* losses, const int32_t* best_rot,
                                const double* g_losses, float* g_quaternion, float* g_xy, float* g_z, float* g_scales,
                                fpc_stream_t stream);
/* out2 f64 [2] (caller zeroes): [0] += sum g^2, [1] += 1 when a non-finite element was seen.  g 16-byte aligned. */
int fpc_grad_sumsq(const float* g, size_t n, double* out2, fpc_stream_t stream);
/* One Lookahead(RAdam) step on a flat f32 shard (p, g, m, v, slow: n elements each; step counts from 1).
 * ctl (device f32[2] or NULL): [0] multiplies every gradient (clip coefficient / world size); [1] != 0 (the inf / NaN guard):
 * the step runs with a ZERO gradient, as the reference's zero_grad() + optimizer.step() does. */
int fpc_lookahead_radam_step(float* p, const float* g, float* m, float* v, float* slow, size_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int64_t step, int la_k, float la_alpha,
                             const float* ctl, fpc_stream_t stream);

/* ---- backbone engine ----------------------------------------------------------
 * PoseRegressor.pure_model_forward + Model.class_compression for inference
 * (lib/pose_regressor.py:709-743, 445-457; encoder / FPN decoder / head graph of
 * segmentation_models_pytorch as built at :608-666): ResNet-18/34 encoder, four FPN decoders,
 * four 1x1 heads, x4 bilinear upsample, xyz -> xy/z split, class compression.  f32 throughout
 * (f32 matrix-core FMAs).  BatchNorm uses running statistics and Dropout2d is the identity
 * (eval mode).
 *
 * fpc_net_create     host-side plan for a fixed (encoder, classes, B, H, W); H, W multiples of 32;
 *                    2 <= classes <= 32 (background included: the bound of fpc_class_compress and
 *                    fpc_confusion), FPC_EINVAL outside — the same for every fpc_net_create_* below.
 *                    The heads have classes / 4G / 3G / 3G channels (G = classes - 1).  A plan with a
 *                    head wider than 32 channels (10 classes and more) always runs the merge + head in
 *                    two passes: FPC_MERGE_SPLIT=0 (the one-pass kernel, heads of at most 32 channels)
 *                    does not apply to it.  FPC_UP4_WIDE=0 (read at create) keeps plans of 9 to 32
 *                    classes on the one-pixel-per-thread x4 upsample + class compression kernel.
 * fpc_net_param_*    the parameter tensors the plan needs, by state-dict name (smp naming,
 *                    e.g. "encoder.layer1.0.conv1.weight", "mask_decoder.p4.skip_conv.bias",
 *                    "rotation_decoder.seg_blocks.0.block.1.block.1.weight", "scales_head.0.weight"),
 *                    each a contiguous f32 tensor in torch's own layout (OIHW weights).
 * fpc_net_load_params  repacks the weights into the workspace (OHWI, padded) and folds BatchNorm.
 *                    `params[i]` (device, 16-byte aligned) must stay valid and unchanged for as
 *                    long as the plan is used: GroupNorm / bias / head parameters are read in place.
 *                    ws: device, 256-byte aligned, >= fpc_net_workspace_bytes(); owned by the caller,
 *                    must outlive the plan's use; holds packed weights AND activations.
 * fpc_net_forward    x f32 [B,3,H,W] (NCHW) -> full-resolution logits (NCHW planes; pass all five
 *                    or all NULL to skip materialising them) and the categorical outputs:
 *                    logits_mask [B,C,H,W], logits_quat [B,4(C-1),H,W], logits_scales [B,3(C-1),H,W],
 *                    logits_xy [B,2(C-1),H,W], logits_z [B,(C-1),H,W];
 *                    cat_mask i64 [B,H,W], cq [B,4,H,W], cs [B,3,H,W], cxy [B,2,H,W], cz [B,H,W]. */
typedef struct fpc_net fpc_net_t;
int fpc_net_create(const char* encoder, int classes, int B, int H, int W, fpc_net_t** out);
/* The same plan for an encoder given by its descriptor: block 1 = BasicBlock, 4 = Bottleneck (torchvision's ResNet V1.5: the
 * stride on the 3x3; ResNet-50 / 101 / 152 = {3,4,6,3} / {3,4,23,3} / {3,8,36,3}); layers4 = blocks per stage, 1..64 each.
 * (1, {2,2,2,2}) and (1, {3,4,6,3}) give the parameter tables and workspaces of "resnet18" / "resnet34".  Same H / W / classes
 * rules as fpc_net_create. */
int fpc_net_create_encoder(int block, const int* layers4, int classes, int B, int H, int W, fpc_net_t** out);
/* ... with torchvision's `groups` and `width_per_group` (the ResNeXt encoders: Bottleneck, groups = 32, width 4 or 8): conv2 of
 * every block is then a GROUPED 3x3 of planes * width_per_group / 64 * groups channels (csrc/conv_grouped.hip; fpc_net_conv_plan
 * reports FPC_PLAN_GROUPED + form there), conv1 / conv3 are 1x1 sites of that width, the stage outputs stay 256 .. 2048.
 * (block, layers4, 1, 64) is fpc_net_create_encoder(block, layers4): the same parameter table, workspace and plans.
 * fpc_net_create answers "resnext50_32x4d", "resnext101_32x4d" and "resnext101_32x8d" with (4, {3,4,6,3} / {3,4,23,3}, 32, 4 / 8).
 * FPC_EINVAL: groups > 1 with block != 4, groups == 1 with another width than 64, channels per group (planes * width_per_group
 * / 64 at planes = 64 .. 512) outside {4, 8, 16, 32, 64}. */
int fpc_net_create_encoder_ex(int block, const int* layers4, int groups, int width_per_group, int classes, int B, int H, int W,
                              fpc_net_t** out);
/* The SE-ResNet encoders (smp's SENetEncoder over pretrainedmodels.senet, reached through smp.encoders.get_encoder at
 * F/lib/pose_regressor.py:608-613 with HPARAM.ENCODER = "se_resnet50" / "se_resnet101" / "se_resnet152"): SEResNetBottleneck x
 * layers4 — conv1 a 1x1 WITH the stride, conv2 a dense 3x3 / stride 1, conv3 a 1x1 x 4 with BatchNorm only, then the squeeze-and-
 * excitation gate sigmoid(fc2(relu(fc1(mean)))) (fc1: C -> C / reduction, fc2 back, both with bias; csrc/se.hip) and
 * relu(x * gate + residual).  The stem is layer0 (conv1, bn1, relu1, pool) and its pool MaxPool2d(3, 2, ceil_mode=True) without
 * padding.  Parameters by pretrainedmodels' names under "encoder." ("encoder.layer0.conv1.weight",
 * "encoder.layer2.0.se_module.fc1.bias"); fc1 / fc2 weights and biases are read in place.  fpc_net_create answers the three names
 * with {3,4,6,3} / {3,4,23,3} / {3,8,36,3} and reduction 16.  On such a plan fpc_net_force_stem_pool(net, 1) is refused (the fused
 * stem launch is a pad-1 pool) and the autotuner does not offer it.  FPC_EINVAL: a reduction < 1 or one that does not divide 256. */
int fpc_net_create_encoder_se(const int* layers4, int reduction, int classes, int B, int H, int W, fpc_net_t** out);
void fpc_net_destroy(fpc_net_t* net);
int fpc_net_param_count(const fpc_net_t* net);
const char* fpc_net_param_name(const fpc_net_t* net, int i);
int64_t fpc_net_param_numel(const fpc_net_t* net, int i);
size_t fpc_net_workspace_bytes(const fpc_net_t* net);
int fpc_net_load_params(fpc_net_t* net, const float* const* params, int count, void* ws, size_t ws_bytes,
                        fpc_stream_t stream);
int fpc_net_forward(fpc_net_t* net, const float* x, float* logits_mask, float* logits_quat,
                    float* logits_scales, float* logits_xy, float* logits_z, int64_t* cat_mask,
                    float* cq, float* cs, float* cxy, float* cz, fpc_stream_t stream);
/* The same, also writing the foreground of cat_mask as bit words (see fpc_class_compress_bits; the plan's W must be a
 * multiple of 64 when fg_bits is not NULL). */
int fpc_net_forward_bits(fpc_net_t* net, const float* x, float* logits_mask, float* logits_quat,
                         float* logits_scales, float* logits_xy, float* logits_z, int64_t* cat_mask,
                         float* cq, float* cs, float* cxy, float* cz, uint64_t* fg_bits, fpc_stream_t stream);

/* Autotuning: after fpc_net_autotune_next the NEXT fpc_net_forward times every candidate tiling
 * (block tile, split-K factor) of every convolution on the device, keeps the fastest, and is itself
 * a valid forward; it synchronises the stream, so it must not be captured into a graph.
 * fpc_net_conv_plan reports the tiling in use for convolution i: out5 = bm, bn, nsplit, Cout, K. */
int fpc_net_autotune_next(fpc_net_t* net, int mode /* 0: minimise each conv's latency; 1: latency x sqrt(share of
                                                      the chip its grid occupies) — for several frames in flight
                                                      (what FrameStreamer(tune_mode=1) and bench.py's stream use);
                                                      2: latency x share (the launch's CU-time) */);
/* Split-precision matrix products (library default 0; the Python front end turns it on unless
 * HPARAM.ENGINE_SPLIT_PRECISION is False).  1: autotuning may replace the f32 matrix instructions of a direct OR a
 * Winograd convolution by the exact three-way bf16 split of both operands (x = x1 + x2 + x3, each piece 8 significant
 * bits) and the six partial products with i + j <= 4 on v_mfma_f32_32x32x16_bf16, accumulated in f32: every kept product
 * is exact, the dropped ones are < 2^-23 of the term, so the result has f32-level accuracy (2.4e-7 of max|ref| against
 * float64, like another summation order) without being bit-identical to the f32 product chain.  Set before
 * fpc_net_autotune_next.  fpc_net_conv_plan reports -5 / -6 / -7 for a split-precision Winograd site (8 waves / 128 channels per
 * workgroup / four waves of 512 registers).
 * 2 (round 6): additionally the fp16 x 2 Winograd form (csrc/wino_h2.hip, reported as -8): two fp16 pieces per operand, all four
 * piece products in two matrix instructions per 8 channels.  Weights are scaled by a power of two on the device; a transformed ACTIVATION v is
 * represented to 3 * 2^-23 |v| while 2^-2 <= |v| < 2^16, to 2^-24 absolute below, loses precision above 2^16 and saturates beyond 1.3e5 — f32-level accuracy for
 * activations of ordinary scale (the tests hold it to the bars of every other form), NOT for tensors of tiny or huge values.  The
 * 3: additionally (and, where Cin is a multiple of 16, INSTEAD of -8) its three-product form (csrc/wino_h3.hip, reported as -9):
 * h1 g1 + h2 g1 + h1 g2 in three matrix instructions per 16 channels; the dropped h2 g2 is < 2^-20 of the term (2^-23 on average) — the size of the
 * two terms every two-piece form drops — and the same tests hold it to the same bars.  At this level the autotuner also times
 * s2.0 with the FPN p2 level folded in (ResNet-18/34 encoders): conv3x3(W, L c2 + b + up2(p3)) as conv3x3(W L, c2) + conv3x3(W,
 * up2(p3)) + a bias table by border class, in one launch that never writes p2; it is kept only when it beats the p2 lateral and
 * s2.0 together.  s2.0 then reports -9 and the p2 lateral site nsplit = 5000 (no launch).  Level 3 also offers, beside the bf16 x 3
 * tilings, the same k_conv_igemm tilings on two fp16 pieces per operand with three piece products (reported as 6000 + split-K
 * factor) at the direct sites of ResNet-18/34 plans that do not run on Winograd: the stride-2 3x3 and 1x1 convolutions and the
 * p5 / p4 / p3 laterals; and the pixel-resident lateral product on the same two pieces (reported as 7000 + parts).  The images
 * of this form are packed only at level 3 (by fpc_net_load_params, or when the level is raised on a loaded plan, on the stream of the
 * last load); their room is always reserved.  Weights: one power of two per convolution from max |w|, undone exactly before the epilogue; activations
 * as they come, with the range of the -8 / -9 forms (3 * 2^-23 relative while 2^-2 <= |x| < 2^16, 2^-24 absolute below, saturation beyond
 * 1.3e5 — finite).
 * The Python front end uses 3 unless HPARAM.ENGINE_SPLIT_F16_3P (then 2) or HPARAM.ENGINE_SPLIT_F16 (then 1) is False. */
int fpc_net_set_split_precision(fpc_net_t* net, int on);
/* HIP graph replay (default 0).  1: after autotuning, the frame-invariant launches of fpc_net_forward (everything
 * between the image conversion and the final upsample / class compression, ~57 kernels on the plan's workspace) are
 * captured once on the caller's stream and replayed with one hipGraphLaunch per frame. */
int fpc_net_set_graph(fpc_net_t* net, int on);
/* 1 while a recorded graph replays the frame (set_graph on and the frame was capturable), else 0. */
int fpc_net_graph_recorded(const fpc_net_t* net);
int fpc_net_conv_count(const fpc_net_t* net);
int fpc_net_conv_plan(const fpc_net_t* net, int i, int* out5);
/* Copies the convolution plans (tilings, split-K factors, kernel forms) of `src` into `dst`: same encoder, classes and frame
 * size, any batch sizes — a small batch then runs on the kernels a larger one was autotuned to (tests/test_gpu_net.py: the
 * headline configuration's plan set against float64 on two frames).  Plans whose split-K partials do not fit dst keep dst's own. */
int fpc_net_copy_plans(fpc_net_t* dst, const fpc_net_t* src);
/* Puts every 3x3 / stride-1 site on Winograd form `form` (1..9: fpc_conv2d's -form; 6 only where Cout % 128 == 0, 9 only where Cin % 16 == 0; other sites keep
 * their plan) — tests hold the whole network on ONE form (8: every eligible product on fp16 x 2 pieces) to the float64 bars.
 * Returns the number of sites changed or a negative code. */
int fpc_net_force_winograd(fpc_net_t* net, int form);
/* on = 1: every 1x1 site with Cin and Cout multiples of 64 on the 1x1 GEMM kernel (csrc/pointwise.hip, reported by
 * fpc_net_conv_plan as 4000 + variant); on = 0: those sites back on the implicit-GEMM kernel's heuristic tiling.  Returns the
 * number of sites changed or a negative code.  The autotuner offers the kernel itself in Bottleneck plans at split level >= 1. */
int fpc_net_force_pointwise(fpc_net_t* net, int on);
/* s2.0 with the FPN p2 level folded in (on = 1, ResNet-18/34 plans; see fpc_net_set_split_precision) or on plain form -9 (on = 0).
 * Returns 1 when the plan changed, 0 when it already was so, or a negative code.  Drops the recorded graph. */
int fpc_net_force_fold(fpc_net_t* net, int on);
/* on = 1 (split level 3 only): every site that has the three-product direct form's image on that form — a pixel-resident lateral
 * site on k_lateral1x1's two-piece build (7000 + parts), any other on its own implicit-GEMM tiling or the heuristic one (6000 +
 * split); on = 0: those sites back on the heuristic f32 tiling.  Returns the number of sites changed or a negative code.  Drops the
 * recorded graph. */
int fpc_net_force_direct_h3(fpc_net_t* net, int on);
/* on = 1 (split level 3 only; conv output rows even, columns a multiple of 64): the 7x7 stem and its 3x3 / 2 max-pool as ONE launch
 * on three fp16 piece products (csrc/stem.hip, k_stem_pool_h3; fpc_net_conv_plan reports 3100 at the stem site): the stem's own
 * output is never written, so fpc_net_tensor("stem") returns FPC_EINVAL while it is chosen ("pool" stays valid).  on = 0: back on
 * the weight-resident stem kernel (3000) followed by the max-pool launch.  At split level 3 the autotuner offers the fused launch
 * itself and keeps it where it beats stem + max-pool together.  Returns 1 when the plan changed, 0 when it was already so, or a
 * negative code.  Drops the recorded graph. */
int fpc_net_force_stem_pool(fpc_net_t* net, int on);
/* ---- The activation-range guard of the fp16-piece forms (opt-in; nothing here runs unless it is called).
 * The forms on two fp16 pieces per operand — Winograd -8 / -9 / -10, s2.0 with the p2 level folded in, the 6000 + split and 7000 +
 * parts plans, the fused stem 3100 — hold an activation to 3 * 2^-23 relative only while it lies in 2^-2 .. 2^16 (see
 * fpc_net_set_split_precision), and nothing in a forward looks at the activations.  The guard surveys them and moves the sites whose
 * input lies outside onto their range-free plans.
 *
 * fpc_act_range: one pass over n contiguous floats (x 4-byte aligned; any n >= 0), accumulated into the 4-word device record rec4:
 *   rec4[0]  the bits of max |x| over the FINITE elements, a non-negative float (atomicMax on the unsigned word; -0.0 counts as 0)
 *   rec4[1]  += the number of non-finite elements (inf, NaN)
 *   rec4[2]  += n, saturating at 2^32 - 1 (non-zero: the record was written at all)
 *   rec4[3]  reserved, not touched
 * The caller zeroes the record; several calls into one record give the maximum and the sums over all their tensors. */
int fpc_act_range(const float* x, long long n, unsigned* rec4, fpc_stream_t stream);
/* The NEXT fpc_net_forward, and only that one, runs fpc_act_range in front of every convolution site's launch, over every tensor the
 * site's CURRENT plan reads as its matrix operand, into records_dev + 4 * site (device memory, 4 * sites words, owned and zeroed by
 * the caller; sites must equal fpc_net_conv_count).  The four decoders of a grouped site accumulate into the index of decoder 0 (the
 * other decoders' indices stay zero); the folded s2.0 surveys what it reads, two operands of two scales: c2 into its own record and p3, at
 * p3's resolution (its nearest x2 upsample holds the same values), into the record of the p2 lateral site, which does not run while
 * it is folded away (either record outside the bounds demotes the fold); the fused stem surveys the image.  That forward
 * launches its kernels (no graph capture or replay, like a tuning pass; a recorded graph is kept), changes no plan, and its outputs
 * are those of an ordinary forward bit for bit.  The workspace does not grow.  The survey is disarmed when that forward call returns,
 * whatever it returns (a refused call included), and by records_dev = NULL (returns FPC_OK): the engine never keeps the pointer.
 * FPC_EINVAL: a plan without loaded parameters, records_dev not 4-byte aligned, sites != fpc_net_conv_count. */
int fpc_net_survey_next(fpc_net_t* net, unsigned* records_dev, int sites);
/* Host arithmetic only (no device call).  records_host: a survey's records copied to the host.  A site whose current plan is an
 * fp16-piece form is DEMOTED when its record shows a non-finite element (rec[1] > 0), max |x| >= hi, or 0 < max |x| < lo; not when
 * the record is all zeros (every form is exact on zeros) or was never written (rec[2] == 0).  It goes to its best range-free plan:
 * the best-scoring candidate of the autotuner that is not an fp16-piece form where the site was autotuned, else the plan of split
 * level 1 — a Winograd site -7 (else -5), a 6000 + split / 7000 + parts plan the same tiling / parts on three bf16 pieces, the
 * folded s2.0 the unfolded pair (the p2 lateral runs again on its own plan, s2.0 by the rule above), 3100 the stem kernel 3000 and
 * the max-pool launch.  Returns the number of sites demoted by this call (idempotent: the same records again give 0) or a negative
 * code (sites != fpc_net_conv_count, lo < 0, hi <= lo), and drops the recorded graph when it demoted any.  Demotions are sticky:
 * they outlast fpc_net_load_params, travel with fpc_net_copy_plans (with the fallback plans; dst keeps its own demotions too), and a later autotuning pass offers a
 * demoted site no fp16-piece form; an explicit fpc_net_force_* of the site wins and clears it.
 * The bounds the Python front end passes are lo = 2^-2 and hi = 2^14, the envelope above with the headroom of the Winograd forms:
 * the F(2x2, 3x3) input transform adds up to four values, so max |x| < 2^14 keeps every TRANSFORMED value below 2^16.  The direct and
 * lateral forms (6000 +, 7000 +, 3100) have no transform and could take 4 x more; they are held to the same two numbers so that
 * there is ONE rule.  The lower bound is on max |x|, not on the values that carry the sum: a tensor is demoted only when ALL of
 * it lies below 2^-2, where the pair's error is 2^-24 absolute instead of relative.  That is conservative by about the ratio of a
 * tensor's maximum to its RMS (a tensor with max 2^-3 and RMS 2^-6 is demoted although 2^-24 absolute is 2^-18 of its scale, and one
 * with max 1 and RMS 2^-8 is not): the record carries no second moment on purpose — one word, one atomic, exact to test — and the
 * guard sees only the frames that were surveyed. */
int fpc_net_guard_ranges(fpc_net_t* net, const unsigned* records_host, int sites, float lo, float hi);
/* 1 while site i stands demoted by fpc_net_guard_ranges, else 0. */
int fpc_net_guarded(const fpc_net_t* net, int i);
/* k_stem_pool_h3's task arithmetic for a stem output of Ho x Wo (host only, no device): out4 = bands of 10 pool rows, strips of 64
 * conv columns, conv outputs one frame's launch computes (the band overlap rows and the halo tiles included), conv outputs that
 * exist (Ho * Wo).  FPC_EINVAL for a shape the fused launch does not take. */
int fpc_stem_pool_tasks(int Ho, int Wo, int64_t* out4);
/* The XCD-banded workgroup order of the streaming and tile kernels (host only, no device): for workgroup `block` of a launch of
 * `grid` workgroups, out4[0] = the logical workgroup it works as (grid % 8 == 0: (block % 8) * (grid / 8) + block / 8, else block);
 * out4[1..3] = first, end, step of the items that slot `slot` (of `per_block` per workgroup and step) of that workgroup visits out of
 * `total`: first, first + step, ... below end.  FPC_EINVAL for grid < 1, block outside [0, grid), per_block < 1, slot outside
 * [0, per_block), total < 0 or total at or above the 32-bit walks' bound (2^32 - 2^20 - 8). */
int fpc_xcd_order(int grid, int block, int64_t total, int per_block, int slot, int64_t* out4);
/* Form -9's launch geometry (host arithmetic, no device) for a 3x3 / stride-1 site with output H x W, batch B, Cin input channels.
 * Where the tile columns of a frame do not fill whole 8-column patches, G frames are laid side by side on a canvas row and the
 * patches are cut out of the canvas (G = the smallest count in 1 .. min(B, 8) that minimises ceil(G tcw / 8) / G, tcw = ceil(W / 2);
 * eligible: tcw >= 8, not the folded s2.0, two frames of the input within 32-bit byte offsets).  out8 = G (1: one frame per patch
 * row), patches per full canvas row, patch rows, launched patches per (64-channel block, decoder), their tile slots (x 64), tiles
 * that exist, GroupNorm records per frame, GroupNorm records per frame and patch row. */
int fpc_wino_pack_geometry(int H, int W, int B, int Cin, int fold, int64_t* out8);
/* on = 1 (default): form-9 launches of the plan use that geometry where it needs fewer patches; on = 0: one frame per patch row.
 * The plans and fpc_net_conv_plan's reports do not change.  Drops the recorded graph. */
int fpc_net_set_wino_pack(fpc_net_t* net, int on);
/* The ORIENTATION of a form-9 site: a site whose output has ceil(W / 2) a multiple of 8 and ceil(H / 2) not (and >= 8) runs
 * TRANSPOSED: the patch's x axis walks the image's y, the frames pack along y, the weight image is packed from the transposed taps.
 * The rule depends on the shape alone.  on = 1 (default) / 0: every site in the stored orientation.  The switch repacks the affected
 * sites' images in place from the parameters and drops the recorded graph; plans, reports and the workspace do not change, and
 * fpc_net_set_wino_pack keeps governing the other sites only.  Results of a transposed site differ from the plain one's by rounding. */
int fpc_net_set_wino_orient(fpc_net_t* net, int on);
/* fpc_wino_pack_geometry under that rule (host only): out9[0] = 1 where the site runs transposed, then out9[1..8] = the out8 above of
 * the virtual image W x H (packed with or without the fold, whatever `pack`); else 0 and the plain site's out8 with packing as `pack`. */
int fpc_wino_orient_geometry(int H, int W, int B, int Cin, int fold, int pack, int64_t* out9);
/* The four-wave Winograd kernels decode their workgroup id by multiply-shift reciprocals of the launch's divisors, n / d =
 * (n * m) >> sh in 64 bits for 0 <= n < 2^31 (host only).  fpc_wino_recip: out2 = {m, sh} of the divisor d, 1 <= d <= 2^31.
 * fpc_wino_decode: what a launcher passes for a launch of `groups` groups and Cout output channels with tbx x tby patches per canvas
 * row on a (virtual) image W pixels wide, B frames, `pack` frames per canvas row (0: a plain launch): out14 = {m, sh} of Cout / 64,
 * groups, tbx, tby, tbx * tby, the patches per row of a ragged last canvas row (tbx where there is none), ceil(W / 2). */
int fpc_wino_recip(uint32_t d, int64_t* out2);
int fpc_wino_decode(int Cout, int groups, int tbx, int tby, int W, int B, int pack, int64_t* out14);
/* The TILE MAP of a packed form-9 launch (several frames per canvas row, or transposed).  Row-split: a lane's two tiles lie four tile
 * rows apart.  X-shared: they are the neighbours 2k, 2k + 1 of one tile row and share half their input columns (12 fragment reads
 * and 6 row transforms per K-step and wave instead of 16 and 8); taken iff the frame's tile-column count ceil(W / 2) of the launch's
 * (virtual) width is even — fpc_wino_xshare_rule(W) = 1 — since every seam of a packed patch is then even.  Outputs and GroupNorm
 * records are the same bit for bit.  fpc_net_set_wino_xshare: on = 1 (default) / 0 = every launch row-split; drops the recorded
 * graph.  fpc_conv2d's -12 / -13 are -10 / -11 on the row-split map.
 * fpc_wino_tile_*: the maps as the kernels compute them (host only; xshare 0 / 1).  _frag: out17 = {n, then per region column
 * x < n of (wave wi, lane) in a patch with its seam after pk_ks tile columns (>= 8: none) the byte offsets of the two fragment reads
 * in an input buffer}.  _slot: the staging plan's view of the buffer's 16-byte unit `slot` in a packed patch whose 18 x 18 region
 * starts at pixel (y_in0, x_in0) of the launch's (virtual; tr = 1: transposed) H x W image of Cs channels, read as its nearest-x2
 * upsample where up = 1, pk_two: the frame behind the seam exists: out6 = {region row, region column, channel half, behind the seam,
 * staged, byte offset of the source from the K-step's first channel of the patch's frame}.
 * _zrun: out3 = {byte offset in the output transform image of the run of (wave wi, tile half mt, accumulator register r, channel
 * tile nt, column cc), tile 8 ty + tx of its lanes 0-31, of its lanes 32-63}.  _zread: byte offset of the output stage's read of
 * thread t_e, tile pass tp, column cc, row i. */
int fpc_wino_xshare_rule(int W);
int fpc_net_set_wino_xshare(fpc_net_t* net, int on);
int fpc_wino_tile_frag(int xshare, int wi, int lane, int pk_ks, int64_t* out17);
int fpc_wino_tile_slot(int xshare, int tr, int slot, int y_in0, int x_in0, int H, int W, int Cs, int up, int pk_ks, int pk_two, int64_t* out6);
int fpc_wino_tile_zrun(int xshare, int wi, int mt, int r, int nt, int cc, int64_t* out3);
int fpc_wino_tile_zread(int xshare, int t_e, int tp, int cc, int i, int64_t* out1);
/* The EXIT of the four-wave Winograd kernels (forms -7, -8, -9 and what -10 .. -13 make of -9).  A thread addresses its 16 output
 * quads (and the residual's, the same) from ONE 64-bit element offset — its tile of pass 0, row 0, column 0; a seam patch has one
 * base per frame, of which a thread takes its side's — plus wave-uniform strides: quad (tp, rr, cc) lies (4 tp + rr) rows and cc
 * columns further.  A workgroup whose patch lies wholly inside its frame in both axes (a seam patch: inside both frames, the second
 * of which exists) takes the FAST exit, which tests no pixel; every other the general one.  Outputs and GroupNorm records are the
 * same bit for bit.  fpc_net_set_wino_fast_exit: on = 1 (default) / 0 = every workgroup takes the general exit; drops the recorded
 * graph.  fpc_conv2d's FPC_PLAN_WINO_GENERAL_EXIT + r (-107 .. -113) is request r = -7 .. -13 with every workgroup on the general exit.
 * fpc_wino_tile_patch (host only): patch `patch` (the workgroup id of a launch of one 64-channel block and one group) of a launch on a
 * (virtual) H x W image of B frames with tbx x tby patches per canvas row, `pack` frames per canvas row (packed = 0: the plain
 * decode, one frame per patch row; pack is then ignored): out8 = {frame b, first tile row ty0, first tile column tx0, seam after
 * that many tile columns (99: none), the frame behind the seam exists, patch row, patch column, takes the fast exit}.
 * fpc_wino_tile_out (host only): the element offsets of thread t_e's 16 quads, out16[4 tp + 2 rr + cc], as the kernels add them up,
 * for the patch (b, ty0, tx0, pk_ks) of 64-channel block nb on a (virtual; tr = 1: transposed) H x W image of Cout channels. */
int fpc_net_set_wino_fast_exit(fpc_net_t* net, int on);
/* The folded s2.0 (form 9 with the FPN p2 level folded in) reads p3 in its second phase as its nearest x2 upsample: a tile's input
 * rows are the low-resolution rows [a, b, b, c], whose transform B^T [a, b, b, c] = [a - b, 2b, 0, b - c] has an exact zero in row
 * 2, the row of one of the workgroup's four waves.  on = 1 (default): that wave only stages its share of the input in that phase;
 * on = 0: it runs the phase on its zeros as the other three do on their rows.  Outputs and GroupNorm records are the same bit for
 * bit for finite p3 (a non-finite value times the zero row made NaN with on = 0 and does not with on = 1); plans, images and the
 * workspace do not change; drops the recorded graph. */
int fpc_net_set_fold_idle_row(fpc_net_t* net, int on);
int fpc_wino_tile_patch(int packed, int H, int W, int B, int tbx, int tby, int pack, int patch, int64_t* out8);
int fpc_wino_tile_out(int tr, int H, int W, int Cout, int nb, int b, int ty0, int tx0, int pk_ks, int t_e, int64_t* out16);
/* Workgroups of all form-9 launches of the last forward that launched (or captured) its kernels: what the switch above changes. */
int64_t fpc_net_wino_blocks(const fpc_net_t* net);
/* FLOP of one forward over the batch under the current plans: out3 = {2 x MACs of the direct convolutions (what the
 * reference's cuDNN path executes), multiply-add FLOP the plans execute (Winograd sites: / 2.25), Winograd share}. */
int fpc_net_flops(const fpc_net_t* net, double* out3);
/* Intermediate activations (NHWC f32 inside the workspace) for tests: "stem", "pool", "c2".."c5",
 * "d<k>.p5".."d<k>.p2", "d<k>.seg<i>" (pre-GroupNorm conv outputs), "d<k>.low" (low-res logits).  "d<k>.p2" is FPC_EINVAL
 * while s2.0 runs with p2 folded in (fpc_net_set_split_precision): that tensor is never written. */
int fpc_net_tensor(const fpc_net_t* net, const char* name, const float** ptr, int* H, int* W, int* C);

/* Stand-alone convolution on the engine's implicit-GEMM kernel (tests / micro-benchmarks).
 * in: any element strides (sb, sh, sw, sc); w_oihw torch layout; out NHWC [B,Ho,Wo,Cout];
 * optional per-channel scale / shift, residual (as out), nearest-x2 `up` [B,Ho/2,Wo/2,Cout], ReLU,
 * GroupNorm partials gn_part [B][P32][Cout][2]; bm/bn/nsplit = 0 -> chosen by the planner.
 * `nsplit` also selects the engine's other kernels for tests: -1..-9 Winograd forms (-5 split precision; -10: form -9 with its
 * patches cut out of canvas rows of several frames, fpc_wino_pack_geometry, P32 = its records per frame; -11: form -9 in the
 * orientation fpc_wino_orient_geometry gives the shape, P32 = that geometry's records; a shape the rule leaves alone: -9), 100 + k split-K
 * summed by a second launch, 1000 + k split-precision (bf16 x 3) products, 2000 + parts the pixel-resident FPN lateral
 * product (1x1, Cin 64 / 128, bias + `up` epilogue), 3000 the weight-resident 7x7 / s2 stem (Cin = 4: NHWC4 image),
 * 3100 the same stem fused with its 3x3 / 2 / pad-1 max-pool on three fp16 piece products (`out` is then the POOLED tensor
 * [B][Ho / 2][Wo / 2][64]; relu must be on, Ho even, Wo a multiple of 64),
 * 4000 + variant the 1x1 GEMM (pad 0, stride 1 / 2, Cin and Cout multiples of 64, channel stride 1, no GroupNorm partials;
 * variant 0: 64-pixel tiles on 4 waves, 1: 128-pixel tiles on 8 waves; bf16 x 3 products), 6000 + k (1 <= k < 100) the
 * implicit GEMM with split-K factor k on two fp16 pieces per operand and three piece products (channel stride 1, Cin a multiple
 * of 32; 6100 + k: split-K summed by a second launch), 7000 + parts the pixel-resident FPN lateral product on the same two pieces.  5000 is never a request: fpc_net_conv_plan's "folded away". */
enum {      /* the bases of those codes, as fpc_net_conv_plan reports them and fpc_conv2d takes them (a Winograd form: -form) */
    FPC_PLAN_WINO_GENERAL_EXIT = -100,      /* + r, r = -7 .. -13: request r with every workgroup on the general exit (never reported) */
    FPC_PLAN_WINO_ORIENT_ROWSPLIT = -13, FPC_PLAN_WINO_PACKED_ROWSPLIT = -12,      /* -11 / -10 on the row-split tile map (fpc_wino_xshare_rule) */
    FPC_PLAN_WINO_ORIENT = -11, FPC_PLAN_WINO_PACKED = -10, FPC_PLAN_TWO_LAUNCH = 100, FPC_PLAN_BF3 = 1000, FPC_PLAN_LATERAL = 2000, FPC_PLAN_STEM = 3000,
    FPC_PLAN_STEM_POOL = 3100, FPC_PLAN_POINTWISE = 4000, FPC_PLAN_FOLDED = 5000, FPC_PLAN_H3 = 6000, FPC_PLAN_LATERAL_H3 = 7000,
    FPC_PLAN_GROUPED = 8000      /* + form: the grouped 3x3 kernel (fpc_conv2d_grouped; fpc_conv2d itself refuses the code) */
};
size_t fpc_conv2d_workspace_bytes(int B, int Ho, int Wo, int Cin, int Cout, int Kh, int Kw);
/* the exact need of one request (same bm / bn / nsplit as the fpc_conv2d call): <= the bound above, which reserves 32
 * split-K slices of the whole output; fpc_conv2d accepts either size */
size_t fpc_conv2d_workspace_bytes_for(int B, int Ho, int Wo, int Cin, int Cout, int Kh, int Kw, int bm, int bn, int nsplit);
int fpc_conv2d_plan(int B, int Ho, int Wo, int Cin, int Cout, int Kh, int Kw, int bm, int bn, int nsplit,
                    int* out4 /* bm, bn, nsplit, P32 */);
int fpc_conv2d(const float* in, int64_t sb, int64_t sh, int64_t sw, int64_t sc, const float* w_oihw,
               const float* scale, const float* shift, const float* res, const float* up, float* out,
               float* gn_part, int B, int Hi, int Wi, int Cin, int Cout, int Kh, int Kw, int stride, int pad,
               int relu, int bm, int bn, int nsplit, void* ws, size_t ws_bytes, fpc_stream_t stream);

/* Stand-alone GROUPED 3x3 convolution, pad 1, stride 1 or 2 (csrc/conv_grouped.hip, k_conv3x3_grouped: conv2 of the ResNeXt
 * blocks): C channels in and out in `groups` groups of C / groups channels each.  in: element strides (sb, sh, sw, sc) with sc = 1
 * (channels contiguous), sb / sh / sw multiples of 4, sw >= C; w_oihw torch's [C][C / groups][3][3]; out NHWC [B][Ho][Wo][C], Ho =
 * (Hi - 1) / stride + 1; optional per-channel scale / shift (folded BatchNorm) and ReLU.  form: 0 = plain f32 products (v_fma_f32,
 * fixed summation order: results are bit-identical run to run) — the only form built; fpc_net_conv_plan reports a site on it as
 * FPC_PLAN_GROUPED + form.  ws: fpc_conv2d_grouped_workspace_bytes(C, groups) bytes, 256-byte aligned (the weights are repacked
 * into it on every call).  FPC_EINVAL before any launch: groups not dividing C, C / groups outside {4, 8, 16, 32, 64}, C not a
 * multiple of 32, another stride or form, sc != 1, a pointer that is null or not 16-byte aligned.  The workspace size of a shape
 * the call refuses is 0. */
size_t fpc_conv2d_grouped_workspace_bytes(int C, int groups);
int fpc_conv2d_grouped(const float* in, int64_t sb, int64_t sh, int64_t sw, int64_t sc, const float* w_oihw, const float* scale,
                       const float* shift, float* out, int B, int Hi, int Wi, int C, int groups, int stride, int relu, int form,
                       void* ws, size_t ws_bytes, fpc_stream_t stream);

/* Data gradient of that GROUPED 3x3 convolution for the training step (csrc/conv_grouped_train.hip), pad 1, stride 1 or 2.
 * dy NHWC [B][Ho][Wo][C] contiguous, Ho = (Hi - 1) / stride + 1 (odd Hi / Wi included); w_oihw torch's [C][C / groups][3][3], the
 * FORWARD's weights; dx NHWC [B][Hi][Wi][C] contiguous, every element written.  Stride 1: k_conv3x3_grouped over dy on the weights
 * transposed inside each group and flipped; stride 2: k_conv3x3_grouped_dgrad_s2, each 2 x 2 block of dx from the 2 x 2 window of
 * dy it sees (9 tap products per channel pair).  Plain f32 products, fixed summation order: bit-identical run to run.  ws:
 * fpc_conv2d_grouped_dgrad_workspace_bytes(C, groups) bytes, 256-byte aligned: k_pack_grouped's image of the transposed weights,
 * rewritten on every call.  FPC_EINVAL before any launch: everything fpc_conv2d_grouped refuses (groups not dividing C, C / groups
 * outside {4, 8, 16, 32, 64}, C not a multiple of 32, another stride), a pointer that is null or not 16-byte aligned (ws: 256), a
 * workspace that is too small.  The workspace size of a shape the call refuses is 0. */
size_t fpc_conv2d_grouped_dgrad_workspace_bytes(int C, int groups);
int fpc_conv2d_grouped_dgrad(const float* dy, const float* w_oihw, float* dx, int B, int Hi, int Wi, int C, int groups, int stride,
                             void* ws, size_t ws_bytes, fpc_stream_t stream);
/* Weight gradient of that convolution (k_conv3x3_grouped_wgrad + k_wgrad_grouped_reduce): dw OIHW [C][C / groups][3][3], every
 * element written (not accumulated), dw[c][ci][ky][kx] = sum over b, oy, ox of dy[b][oy][ox][c] x[b][s oy + ky - 1][s ox + kx - 1]
 * [g (C / groups) + ci].  x: pixel (b, y, x) at x + b sb + y sh + x sw with its C channels contiguous (a channel slice of a wider
 * tensor is fine), sb / sh / sw multiples of 4, sw >= C; dy NHWC [B][Ho][Wo][C] contiguous.  The (frame, tile) list is cut into
 * slices, one partial per slice, summed in slice order: plain f32, no atomics, bit-identical run to run.  ws:
 * fpc_conv2d_grouped_wgrad_workspace_bytes(B, Ho, Wo, C, groups) bytes, 256-byte aligned: the partials [slice][C][C / groups][9]
 * (the call's slice count is that size over C * (C / groups) * 36, or its tile count — 8 x 16 output pixels at stride 1, 8 x 8 at
 * stride 2 — where that is less; with one slice the workspace is not touched).  FPC_EINVAL before any launch: as
 * fpc_conv2d_grouped_dgrad, and strides that are not multiples of 4 or sw < C.  The workspace size of a refused shape is 0. */
size_t fpc_conv2d_grouped_wgrad_workspace_bytes(int B, int Ho, int Wo, int C, int groups);
int fpc_conv2d_grouped_wgrad(const float* x, int64_t sb, int64_t sh, int64_t sw, const float* dy, float* dw, int B, int Hi, int Wi,
                             int C, int groups, int stride, void* ws, size_t ws_bytes, fpc_stream_t stream);

/* The training step's 7x7 / stride-2 / pad-3 stem (3 -> 64 channels) and the 3x3 / stride-2 / pad-1 max-pool behind it
 * (csrc/stem_train.hip, lib/train_conv.py: _StemConvFn, _MaxPoolFn).  Each entry replaces its part of conv1 / maxpool of the smp
 * ResNet encoder the reference builds at F/lib/pose_regressor.py:608, forward and backward under Lightning's training step
 * (cuDNN / aten there).  f32 throughout; no atomics and a fixed summation order: bit-identical run to run.  Every entry returns
 * FPC_EINVAL BEFORE any launch for a shape outside its class and for a pointer that is null or not 16-byte aligned.
 *
 * fpc_image_nhwc4 (k_nchw3_to_nhwc4): x NCHW contiguous [B][3][H][W] -> out [B][H][W][4], the fourth channel 0: the image the stem
 *   kernels read (fpc_conv2d's code 3000, fpc_stem_wgrad).  B, H, W >= 1, B H W < 2^31, H W < 2^30.  Replaces the layout
 *   change cuDNN makes inside conv1 (F/lib/pose_regressor.py:608).
 * fpc_stem_wgrad (k_stem_wgrad + k_stem_wgrad_reduce): dw OIHW [64][3][7][7], every element overwritten,
 *   dw[co][c][kh][kw] = sum over b, oy, ox of dy[b][oy][ox][co] img4[b][2 oy + kh - 3][2 ox + kw - 3][c], zero outside the image.
 *   img4 [B][Hi][Wi][4] (the fourth channel is ignored), dy NHWC [B][Hi / 2][Wi / 2][64] contiguous.  Shape class: Hi, Wi even and
 *   >= 8, B >= 1, B Hi Wi < 2^31.  Exact f32 products on the matrix cores.  The list of (frame, output row, 64-pixel segment)
 *   units is cut into fpc_stem_wgrad_slices(B, Hi, Wi) contiguous slices — a function of the shape alone —, one partial
 *   [64][224] per slice, added in slice order in double.  ws: fpc_stem_wgrad_workspace_bytes(B, Hi, Wi) = slices * 64 * 224 * 4
 *   bytes, 256-byte aligned (misaligned: FPC_EINVAL; too small: FPC_EWORKSPACE).  Slices and bytes of a refused shape are 0.
 *   Replaces the weight gradient of conv1 (cuDNN under autograd, F/lib/pose_regressor.py:608).
 * fpc_maxpool3x3s2_fwd (k_maxpool3x3s2): x NHWC [B][Hi][Wi][C] -> y [B][(Hi - 1) / 2 + 1][(Wi - 1) / 2 + 1][C].
 * fpc_maxpool3x3s2_bwd (k_maxpool3x3s2_bwd): dx [B][Hi][Wi][C] from x and dy (y's shape), every element written once: dy of each
 *   window goes to the window's FIRST maximum in row-major order over its in-bounds elements (torch's rule), contributions added
 *   in (window row, window column) order.  Shape class of both: Hi, Wi >= 1, C >= 4 and C % 4 == 0, B Hi Wi C < 2^32.  Inputs
 *   are finite: NaN is outside the contract.  Replace encoder.maxpool (F/lib/pose_regressor.py:608), aten forward / backward. */
int fpc_image_nhwc4(const float* x, float* out, int B, int H, int W, fpc_stream_t stream);
size_t fpc_stem_wgrad_workspace_bytes(int B, int Hi, int Wi);
int fpc_stem_wgrad_slices(int B, int Hi, int Wi);
int fpc_stem_wgrad(const float* img4, const float* dy, float* dw, int B, int Hi, int Wi, void* ws, size_t ws_bytes,
                   fpc_stream_t stream);
int fpc_maxpool3x3s2_fwd(const float* x, float* y, int B, int Hi, int Wi, int C, fpc_stream_t stream);
int fpc_maxpool3x3s2_bwd(const float* x, const float* dy, float* dx, int B, int Hi, int Wi, int C, fpc_stream_t stream);

/* ---- The squeeze-and-excitation gate of the SE-ResNet encoders, stand-alone (unit tests; the engine runs the same launches).
 * They replace pretrainedmodels.senet.SEModule.forward and the `se_module(out) + residual` / ReLU lines of
 * SEResNetBottleneck.forward (aten kernels in the reference, reached through smp.encoders.get_encoder, F/lib/pose_regressor.py:
 * 608-613), and layer0.pool = nn.MaxPool2d(3, stride=2, ceil_mode=True) of the same encoder.  NHWC f32, C a multiple of 64 (at
 * most 8192), every pointer 16-byte aligned; no float atomics and summation orders that depend on the shape alone: two calls agree
 * bit for bit.  FPC_EINVAL: C % 64 != 0, R < 1 or R not dividing C, a NULL or misaligned pointer, B < 1.
 *
 * fpc_se_pool_slabs: the slabs k_se_pool cuts one frame's H W pixels into — a function of (H, W, C) only; 0 for a refused shape.
 * fpc_se_scratch_floats: floats of `scratch` = B * slabs * C (the per-slab channel sums).
 * fpc_se_gate (k_se_pool + k_se_excite): gate[b][c] = 1 / (1 + exp(-(w2 relu(w1 m_b + b1) + b2)[c])) with m_b the mean of x[b] over
 *   its H W pixels (slab sums added in slab order, times 1 / (H W)), w1 [C / R][C], b1 [C / R], w2 [C][C / R], b2 [C]: the weights
 *   and biases of fc1 / fc2 in torch's layout.  A pre-activation of +-100 gives exactly 1 / 0.
 * fpc_se_scale_add_relu (k_se_scale_add_relu): y = max(x * gate[b][c] + res, 0) over [B][H][W][C]; y may be x.
 * fpc_maxpool3x3s2_ceil_fwd (k_maxpool3x3s2<0>): x [B][Hi][Wi][C] -> y [B][Hi / 2][Wi / 2][C], window (i, j) = rows 2 i .. 2 i + 2 and
 *   columns 2 j .. 2 j + 2 clipped to the map: F.max_pool2d(x, 3, 2, 0, ceil_mode=True) for every Hi, Wi >= 2 (odd ones included). */
int fpc_se_pool_slabs(int H, int W, int C);
size_t fpc_se_scratch_floats(int B, int H, int W, int C);
int fpc_se_gate(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* gate, float* scratch, int B,
                int H, int W, int C, int R, fpc_stream_t stream);
int fpc_se_scale_add_relu(const float* x, const float* gate, const float* res, float* y, int B, int H, int W, int C,
                          fpc_stream_t stream);
int fpc_maxpool3x3s2_ceil_fwd(const float* x, float* y, int B, int Hi, int Wi, int C, fpc_stream_t stream);

/* ---- The MobileNetV2 encoder's kernels (csrc/mobilenet.hip), stand-alone.  fpc_net_create("mobilenet_v2", ...) builds the plan that
 * runs them: torchvision's MobileNetV2 features as smp wraps it (F/lib/pose_regressor.py:608-613 through smp.encoders.get_encoder),
 * replacing cuDNN's depthwise and 1x1 convolutions and aten's BatchNorm / ReLU6 at inference.  Such a plan's encoder is the stem,
 * 17 depthwise, 16 expand, 17 project launches and the last 1x1; these ops have one form each: they are not convolution sites
 * (fpc_net_conv_count counts the decoders' alone), are not autotuned, and the activation-range survey and guard cover only the
 * decoder sites of such a plan — the three kernels take any finite f32.  fpc_net_force_stem_pool is refused on it,
 * fpc_net_force_fold(net, 1) too, fpc_net_force_direct_h3 changes 0 sites; the p2 lateral (24 channels) runs on the implicit GEMM's
 * Cin % 4 loader with the top-down addend in its epilogue.
 * All three: dense channel-last f32, every pointer non-NULL and 16-byte aligned (FPC_EINVAL otherwise), per-channel scale / shift =
 * the folded BatchNorm, act 0 = none, 1 = ReLU6 min(max(v, 0), 6); fixed summation order, no atomics: bit-identical run to run.
 * fpc_dwconv3x3 (csrc/depthwise.hip: k_dw_fwd): depthwise 3x3, pad 1, stride 1 or 2: in [B][Hi][Wi][C], w torch's [C][1][3][3] read in place,
 *   out [B][(Hi - 1) / stride + 1][(Wi - 1) / stride + 1][C].  Refused: B < 1, C < 4 or C % 4 != 0, any other stride or act.
 * fpc_conv1x1_f32 (k_conv1x1_f32): out[m][n] = act(scale[n] sum_k in[m][k] w[n][k] + shift[n]) (+ res[m][n]) over M pixel rows,
 *   w torch's [Cout][Cin][1][1], exact f32 products on v_mfma_f32_32x32x2_f32 with f32 accumulation.  Cin % 8 == 0, 8 .. 1024;
 *   Cout % 8 == 0, 8 .. 2048; res may be NULL and is added behind the affine, with no activation: res with act != 0 is refused.
 *   fpc_conv1x1_f32_form: the form a shape runs on (host arithmetic; FPC_EINVAL for a refused shape): 0 = 16 x 16 tiles on
 *   v_mfma_f32_16x16x4_f32 where M / 32 x Cout / 32 (rounded up) is below 1024, else 1 / 2 / 3 / 5 = that many 32-channel tiles per
 *   wave on 32 x 32 tiles.  The summation order depends on the form, i.e. on the shape alone.
 * fpc_stem3x3s2 (k_stem3x3s2): the dense 3x3 / stride 2 / pad 1 stem over fpc_image_nhwc4's image [B][Hi][Wi][4] with w [32][3][3][3]
 *   and ReLU6: out [B][(Hi - 1) / 2 + 1][(Wi - 1) / 2 + 1][32].  Cout must be 32. */
int fpc_dwconv3x3(const float* in, const float* w, const float* scale, const float* shift, float* out, int B, int Hi, int Wi, int C,
                  int stride, int act, fpc_stream_t stream);
int fpc_conv1x1_f32(const float* in, const float* w, const float* scale, const float* shift, const float* res, float* out, int64_t M,
                    int Cin, int Cout, int act, fpc_stream_t stream);
int fpc_conv1x1_f32_form(int64_t M, int Cin, int Cout);
int fpc_stem3x3s2(const float* in4, const float* w, const float* scale, const float* shift, float* out, int B, int Hi, int Wi, int Cout,
                  fpc_stream_t stream);

/* ---- The EfficientNet-B0 encoder's kernels (csrc/efficientnet.hip and the gated / swish instantiations of csrc/mobilenet.hip's stem
 * and 1x1 kernels), stand-alone.  fpc_net_create("efficientnet-b0", ...) builds the plan that runs them: efficientnet_pytorch's
 * EfficientNet as smp's EfficientNetEncoder wraps it (F/lib/pose_regressor.py:608-613 through smp.encoders.get_encoder), replacing
 * cuDNN's depthwise and 1x1 convolutions and aten's BatchNorm, swish, mean, sigmoid and multiply at inference.  Such a plan's encoder
 * is the stem and, for each of the 16 MBConv blocks, an expand 1x1 (not block 0), a depthwise, the gate (two launches) and a project
 * 1x1 that multiplies its input by the gate: 80 launches.  The ops follow the MobileNetV2 ops' rules: one form each, not convolution
 * sites (fpc_net_conv_count counts the decoders' alone), not autotuned, not surveyed or guarded; fpc_net_force_stem_pool and
 * fpc_net_force_fold(net, 1) are refused, fpc_net_force_direct_h3 changes 0 sites; the p2 / p3 / p4 laterals (24 / 40 / 112
 * channels) run on the implicit GEMM's Cin % 4 loader.  _conv_head and the top-level _bn1 are not parameters of the plan.
 * All: dense channel-last f32, every pointer non-NULL (but res and gate of fpc_mbconv_pw) and 16-byte aligned (FPC_EINVAL
 * otherwise), scale / shift = the folded BatchNorm (eps 1e-3 in this encoder), act 0 = none, 1 = ReLU6, 2 = swish v / (1 + exp(-v));
 * fixed summation orders, no atomics: bit-identical run to run.  The pads are efficientnet_pytorch's static "same" pads for the
 * declared 224 image: stride 1 (k - 1) / 2 on every side; stride 2 pads 0 before and 1 after for k = 3, 1 and 2 for k = 5.
 * fpc_mbconv_dw (csrc/depthwise.hip: k_dw_fwd; replaces _depthwise_conv + _bn1 + swish of MBConvBlock.forward): depthwise k x k, k 3 or 5, stride 1
 *   or 2: in [B][Hi][Wi][C], w torch's [C][1][k][k] read in place, out [B][Hi / stride][Wi / stride][C].  Refused: B < 1, C < 4 or
 *   C % 4 != 0, any other k, stride or act, an odd Hi or Wi at stride 2.
 * fpc_mbconv_gate (k_mb_pool + k_mb_excite; replaces adaptive_avg_pool2d, _se_reduce, swish, _se_expand and sigmoid):
 *   gate[b][c] = 1 / (1 + exp(-(w2 swish(w1 m_b + b1) + b2)[c])) with m_b the mean of x[b] [H][W][C] over its pixels (slab sums added
 *   in slab order, divided by H W), w1 [Cs][C], b1 [Cs], w2 [C][Cs], b2 [C]: torch's layouts.  C % 4 == 0, 4 .. 2048; Cs 1 .. 64;
 *   B <= 65535.  fpc_mbconv_gate_slabs: the slabs one frame is cut into, a function of (H, W, C) only, 0 for a refused shape;
 *   fpc_mbconv_gate_scratch_floats: floats of `scratch` = B * slabs * C.
 * fpc_mbconv_pw (k_conv1x1_f32's gated instantiations; replaces `x * gate`, _project_conv + _bn2 + the skip add, and _expand_conv +
 *   _bn0 + swish): out[m][n] = act(scale[n] sum_k (in[m][k] gate[m / HW][k]) w[n][k] + shift[n]) (+ res[m][n]) over B frames of HW
 *   rows each, the product in gate rounded to f32 before it enters the exact-f32 matrix instruction; gate [B][Cin] may be NULL (no
 *   multiply).  Cin % 8 == 0, 8 .. 2048; Cout % 8 == 0, 8 .. 2048; res with act != 0 is refused.  fpc_mbconv_pw_form: the form the
 *   shape runs on, as fpc_conv1x1_f32_form for M = B HW (0, 1, 2, 3 or 5; FPC_EINVAL for a refused shape).
 * fpc_mbconv_stem (k_stem3x3s2's instantiation; replaces _conv_stem + _bn0 + swish): the dense 3x3 / stride 2 stem with pads 0 before
 *   and 1 after over fpc_image_nhwc4's image [B][Hi][Wi][4], w [32][3][3][3], swish: out [B][Hi / 2][Wi / 2][32].  Cout must be 32,
 *   Hi and Wi even. */
int fpc_mbconv_dw(const float* in, const float* w, const float* scale, const float* shift, float* out, int B, int Hi, int Wi, int C,
                  int k, int stride, int act, fpc_stream_t stream);
int fpc_mbconv_gate_slabs(int H, int W, int C);
size_t fpc_mbconv_gate_scratch_floats(int B, int H, int W, int C);
int fpc_mbconv_gate(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* gate, float* scratch, int B,
                    int H, int W, int C, int Cs, fpc_stream_t stream);
int fpc_mbconv_pw(const float* in, const float* gate, const float* w, const float* scale, const float* shift, const float* res, float* out,
                  int B, int64_t HW, int Cin, int Cout, int act, fpc_stream_t stream);
int fpc_mbconv_pw_form(int B, int64_t HW, int Cin, int Cout);
int fpc_mbconv_stem(const float* in4, const float* w, const float* scale, const float* shift, float* out, int B, int Hi, int Wi, int Cout,
                    fpc_stream_t stream);

/* ---- The DenseNet encoders' kernels (csrc/densenet.hip), stand-alone.  fpc_net_create("densenet121" | "densenet169" | "densenet201", ...)
 * builds the plan that runs them: torchvision's DenseNet.features as smp's DenseNetEncoder wraps it (F/lib/pose_regressor.py:608-613
 * through smp.encoders.get_encoder), replacing cuDNN's 1x1 and 3x3 convolutions and aten's BatchNorm, ReLU, cat and avg_pool2d at
 * inference.  densenet161 (stem 96, growth 48) is not built: FPC_EINVAL.  Such a plan's encoder is the ResNet family's 7x7 stem
 * site (tuned, surveyed and guarded like theirs; fpc_net_force_stem_pool applies) and its max-pool, the place step, two launches per
 * dense layer (58 / 82 / 98 layers), two per transition and norm5.  A block's layers share one concatenation buffer
 * [B][h][w][C_end]: torch.cat is never executed, a layer reads the channel prefix in front of it and appends its 32 channels.  A
 * transition runs as conv(pool(relu(norm(x)))): the module's pool(conv(.)) is the same linear map, at four times the products; the
 * two orders differ by rounding only.  The dense ops are not convolution sites (fpc_net_conv_count counts the stem's and the
 * decoders' alone), are not autotuned, surveyed or guarded; fpc_net_force_fold(net, 1) is refused, fpc_net_force_direct_h3 changes
 * 0 sites; the laterals see 256 / 512 / 1024 .. channels, all on the fast loader.
 * All: channel-last f32, every pointer 16-byte aligned (FPC_EINVAL otherwise; NULL only where stated), exact f32 products on
 * v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32 with f32 accumulation, a summation order the shape and the form alone fix, no
 * atomics: bit-identical run to run.  `form` -1 runs the form the shape names (the _form function), 0 / 1 force one.
 * fpc_dense_pw (k_dense_pw32 / k_dense_pw16; replaces norm1 + relu1 + conv1 + norm2 + relu2 of _DenseLayer, and a _Transition's conv):
 *   out[m ldo + n] = act(s2[n] sum_{k < K} pre(in[m ldi + k]) w[n][k] + t2[n]) with pre(v) = max(s1[k] v + t1[k], 0) rounded to f32
 *   before the matrix instruction; s1 / t1 both NULL: pre is the identity; s2 / t2 both NULL: no affine.  w torch's [Cout][K][1][1]
 *   read in place.  Nothing at or behind channel K of an input row is read, only [0, Cout) of an output row is written.  K % 32 == 0,
 *   32 .. 2048; Cout % 32 == 0, 32 .. 1024; ldi >= K, ldi % 4 == 0; ldo >= Cout; 1 <= M < 2^31 - 64; act 0 or 1 (ReLU).
 *   fpc_dense_pw_form: 1 = 32 x 32 tiles, a wave each, where M / 32 (rounded up) x Cout / 32 reaches 1024, else 0 = 16 x 16 tiles, a
 *   workgroup each: its four waves take the K-steps of 32 in turn and are added through LDS as ((w0 + w1) + w2) + w3.
 * fpc_dense_conv3x3 (k_dense_conv3_tile / k_dense_conv3_split; replaces conv2 of _DenseLayer and the torch.cat behind it): 3x3, pad 1,
 *   stride 1, 128 -> 32 channels, no affine, no activation: out[((b H + h) W + w) ldo + c0 + n] = sum in[b][h + kh - 1][w + kw - 1][c]
 *   w[n][c][kh][kw] over in dense [B][H][W][128]; only channels [c0, c0 + 32) of a pixel are written.  c0 % 32 == 0, c0 + 32 <= ldo,
 *   B H W < 2^31 - 64.  wt is the image fpc_dense_conv3x3_pack makes of torch's w [32][128][3][3]: 9 x 32 x 128 floats, [tap][n][c].
 *   fpc_dense_conv3x3_form: 1 = one wave per 64 pixels where that gives 1024 waves (B H W > 65472), else 0 = a workgroup of nine waves
 *   per 16 pixels, a tap each, added through LDS in tap order.
 * fpc_dense_norm_pool (k_dense_norm_pool; replaces a _Transition's norm + relu + pool, and norm5): skip = act(s x + t) over dense
 *   [B][H][W][C] and, where pooled is not NULL (H and W even), pooled[b][h / 2][w / 2][c] = 0.25f ((skip00 + skip01) + (skip10 + skip11)).
 *   C % 4 == 0; B H W C / 4 < 2^32 - 2^20 - 8.
 * fpc_dense_place (k_dense_place; the pooled stem into block 1's buffer): out[m ld + c] = in[m C + c] for c < C, bit for bit; C % 4 == 0,
 *   ld >= C, ld % 4 == 0, M C / 4 < 2^32 - 2^20 - 8. */
int fpc_dense_pw(const float* in, const float* s1, const float* t1, const float* w, const float* s2, const float* t2, float* out, int64_t M,
                 int K, int Cout, int ldi, int ldo, int act, int form, fpc_stream_t stream);
int fpc_dense_pw_form(int64_t M, int K, int Cout);
int fpc_dense_conv3x3_pack(const float* w, float* wt, fpc_stream_t stream);
int fpc_dense_conv3x3(const float* in, const float* wt, float* out, int B, int H, int W, int c0, int ldo, int form, fpc_stream_t stream);
int fpc_dense_conv3x3_form(int B, int H, int W);
int fpc_dense_norm_pool(const float* x, const float* s, const float* t, float* skip, float* pooled, int B, int H, int W, int C, int act,
                        fpc_stream_t stream);
int fpc_dense_place(const float* in, float* out, int64_t M, int C, int ld, fpc_stream_t stream);

/* ---- The VGG encoders' kernels (csrc/vgg.hip), stand-alone.  fpc_net_create("vgg11" | "vgg13" | "vgg16" | "vgg19", each also with
 * "_bn", ...) builds the plan that runs them: torchvision's vgg.make_layers as smp's VGGEncoder wraps it (F/lib/pose_regressor.py:608-613
 * through smp.encoders.get_encoder).  features.0 runs on k_conv3x3_c3, every pool on k_maxpool2x2; every other convolution (3x3 /
 * stride 1 / pad 1, 64 .. 512 channels) is an ordinary convolution site: tuned, surveyed and range-guarded like a ResNet's, on a
 * Winograd form or the implicit GEMM, with ReLU and the bias — or the BatchNorm folded at load with the bias folded in behind it — in
 * its epilogue.  fpc_net_conv_count is the encoder's convolutions minus one plus the decoders' 44 (56 for vgg16).  c2 .. c5 are the
 * outputs of blocks 3, 4, 5 and of the last pool; fpc_net_tensor's "stem" and "pool" name the outputs of blocks 1 and 2 (smp's
 * feature levels 1 and 2), which outlive the forward.  fpc_net_force_fold(net, 1) and fpc_net_force_stem_pool are refused (c2 has 256
 * channels; there is no 7x7 stem).  SIZE: such a plan holds full-resolution 64-channel maps; fpc_net_create returns FPC_EINVAL unless
 * 16 B H W < 2^32 - 2^20 - 8 (features.0's walk; 873 frames of 640 x 480) and (H + 2) W 256 < 2^31 (the implicit GEMM's lane offsets
 * inside one frame): the smallest bounds of the kernels on the plan.  32 x 480 x 640 is built.
 * Both: channel-last f32, every pointer 16-byte aligned (FPC_EINVAL otherwise; NULL only where stated), no atomics, a summation
 * order the shape alone fixes: bit-identical run to run.
 * fpc_conv3x3_c3 (k_conv3x3_c3; replaces features.0 with its BatchNorm and ReLU): dense 3x3 / stride 1 / pad 1 over fpc_image_nhwc4's
 *   image in4 [B][H][W][4] — the fourth channel never enters a product, whatever it holds — with w torch's [64][3][3][3] read in
 *   place: out[b][h][w][n] = act(scale[n] sum + shift[n]), sum over (kh, kw, ci) in that order by fused multiply-adds from 0; scale
 *   NULL: sum + shift[n] (the bias alone).  act 0, or 1 = ReLU.  Nothing outside the image is read.  Cout must be 64; B, H, W >= 1;
 *   16 B H W < 2^32 - 2^20 - 8.
 * fpc_maxpool2x2_fwd (k_maxpool2x2; replaces MaxPool2d(2, 2)): x [B][H][W][C] -> y [B][H / 2][W / 2][C],
 *   y = max(max(x00, x01), max(x10, x11)).  H, W even and >= 2, C >= 4 and C % 4 == 0, B (H / 2) (W / 2) (C / 4) < 2^32 - 2^20 - 8.  Inputs
 *   are finite: NaN is outside the contract, as for fpc_maxpool3x3s2_fwd; of -0 and +0 either may be returned. */
int fpc_conv3x3_c3(const float* in4, const float* w, const float* scale, const float* shift, float* out, int B, int H, int W, int Cout,
                   int act, fpc_stream_t stream);
int fpc_maxpool2x2_fwd(const float* x, float* y, int B, int H, int W, int C, fpc_stream_t stream);

/* The training step's VGG pieces (csrc/vgg_train.hip, lib/train_conv.py: _VggConv0Fn, _MaxPool2x2Fn, behind FPC_TRAIN_NATIVE_VGG=1;
 * ABI 11, additive).  They replace the backward of features.0 (cuDNN's weight gradient and aten's bias reduction under autograd in
 * the reference) and of MaxPool2d(2, 2) (aten's index plane and scatter) inside smp's VGG encoder, reached from
 * F/lib/pose_regressor.py:608-613; the forwards in training are fpc_image_nhwc4 + fpc_conv3x3_c3 (scale NULL, shift = the bias,
 * act 0) and fpc_maxpool2x2_fwd above.  f32 throughout; no atomics and a fixed summation order: bit-identical run to run.  Every
 * entry returns FPC_EINVAL BEFORE any launch for a shape outside its class and for a pointer that is null (db excepted) or not
 * 16-byte aligned.
 *
 * fpc_conv3x3_c3_wgrad (k_c3_wgrad + k_c3_wgrad_reduce): dw OIHW [64][3][3][3] and db [64], every element of both overwritten,
 *   dw[co][ci][kh][kw] = sum over b, y, x of dy[b][y][x][co] img4[b][y + kh - 1][x + kw - 1][ci], zero outside the image;
 *   db[co] = sum over b, y, x of dy[b][y][x][co], from the same pass over dy; db NULL: not computed.  img4 [B][H][W][4]
 *   (fpc_image_nhwc4's; the fourth channel never enters a result, whatever it holds), dy NHWC [B][H][W][64] contiguous.  Shape class:
 *   fpc_conv3x3_c3's (B, H, W >= 1, 16 B H W < 2^32 - 2^20 - 8).  Exact f32 products on the matrix cores.  The list of (frame, row,
 *   64-pixel segment) units is cut into fpc_conv3x3_c3_wgrad_slices(B, H, W) contiguous slices — a function of the shape alone —,
 *   one partial [64][48] per slice, added in slice order in double.  ws: fpc_conv3x3_c3_wgrad_workspace_bytes(B, H, W) = slices *
 *   64 * 48 * 4 bytes, 16-byte aligned (too small: FPC_EINVAL).  Slices and bytes of a refused shape are 0.
 * fpc_maxpool2x2_bwd (k_maxpool2x2_bwd): dx [B][H][W][C] from x and dy [B][H / 2][W / 2][C], every element written once: dy of a
 *   window goes to the window's FIRST maximum in row-major order (torch's rule), 0 to its other three elements.  Shape class:
 *   fpc_maxpool2x2_fwd's.  Inputs are finite: NaN is outside the contract. */
size_t fpc_conv3x3_c3_wgrad_workspace_bytes(int B, int H, int W);
int fpc_conv3x3_c3_wgrad_slices(int B, int H, int W);
int fpc_conv3x3_c3_wgrad(const float* img4, const float* dy, float* dw, float* db, int B, int H, int W, void* ws, size_t ws_bytes,
                         fpc_stream_t stream);
int fpc_maxpool2x2_bwd(const float* x, const float* dy, float* dx, int B, int H, int W, int C, fpc_stream_t stream);

/* ---- The depthwise 3x3 convolution and the ReLU6 of the MobileNetV2 encoder in the training step (csrc/depthwise.hip,
 * csrc/batchnorm.hip; lib/train_conv.py: _DepthwiseConv2dFn and batchnorm_act(relu6=True) behind FPC_TRAIN_NATIVE_MBV2=1).  They
 * replace autograd through torch.nn.Conv2d(groups = C) and nn.ReLU6 inside smp's MobileNetV2 encoder (cuDNN's grouped kernels and
 * aten's hardtanh, forward and backward, in the reference; reached from F/lib/pose_regressor.py:608-613).  The FORWARD of the
 * convolution in training is fpc_dwconv3x3 above with act 0, scale 1 and shift 0 (v * 1 + 0 is exact).  Conventions of the entries
 * above: dense channel-last f32, w / dw torch's [C][1][3][3] read / written in place, pad 1, plain f32 FMAs in an order the shape
 * alone fixes, no atomics: bit-identical run to run.  FPC_EINVAL before any launch: a NULL or not 16-byte-aligned pointer, B < 1,
 * C < 4 or C % 4 != 0, a stride other than 1 or 2, Hi < 1 or Wi < 1, B Hi Wi C / 4 >= 2^32 - 2^20 - 8 (the 32-bit walk limit of
 * fpc_dwconv3x3).
 *
 * fpc_dwconv3x3_dgrad (k_dw_dgrad_s1 / _s2): dx [B][Hi][Wi][C] from dy [B][(Hi - 1) / stride + 1][(Wi - 1) / stride + 1][C],
 *   every element written exactly once: dx[h][w] = sum over kh, kw of dy[(h + 1 - kh) / stride][(w + 1 - kw) / stride] w[kh][kw] where
 *   the divisions are exact and the index is inside dy.  Stride 2 is evaluated per output parity (dx[2a] = dy[a] w[1],
 *   dx[2a + 1] = dy[a] w[2] + dy[a + 1] w[0] per axis): nine products per 2 x 2 block of dx and channel, no zero insertion.
 * fpc_dwconv3x3_wgrad (k_dw_wgrad + k_dw_wgrad_reduce): dw[c][kh][kw] = sum over b, ho, wo of
 *   dy[b][ho][wo][c] x[b][stride ho + kh - 1][stride wo + kw - 1][c], zero outside x; every element of dw is overwritten, a tap no
 *   pixel reaches (a 1 x 1 map: all but the centre) with an exact zero.  The list of the B Ho (frame, output row) pairs is cut into
 *       slices = max(1, min(max(1, 1024 / ceil(C / 32)), B Ho ceil(Wo / 8) / 32, B Ho))      (integer divisions)
 *   contiguous slices, slice i = rows [i B Ho / slices, (i + 1) B Ho / slices): a function of (B, Ho, Wo, C) alone.  One f32
 *   partial [C][9] per slice (inside a slice: 32 pixel slots over its (row, 8-column segment) units in turn, added in a fixed
 *   tree), the slices added in double in sixteen contiguous ranges, each ascending, the ranges ascending.
 *   ws: fpc_dwconv3x3_wgrad_workspace_bytes(B, Ho, Wo, C) = slices * C * 9 * 4 bytes (0 for a refused shape), 256-byte aligned;
 *   too small or misaligned: FPC_EWORKSPACE (a NULL ws: FPC_EINVAL). */
int fpc_dwconv3x3_dgrad(const float* dy, const float* w, float* dx, int B, int Hi, int Wi, int C, int stride, fpc_stream_t stream);
size_t fpc_dwconv3x3_wgrad_workspace_bytes(int B, int Ho, int Wo, int C);
int fpc_dwconv3x3_wgrad(const float* x, const float* dy, float* dw, int B, int Hi, int Wi, int C, int stride, void* ws,
                        size_t ws_bytes, fpc_stream_t stream);

/* ---- The gradients of the depthwise k x k convolution of the EfficientNet-B0 encoder, for the training step
 * (csrc/depthwise.hip; C entries only, their front end in lib/train_conv.py is DESIGN.md 6b item 8 d).  They replace
 * the backward of autograd through efficientnet_pytorch's Conv2dStaticSamePadding(groups = C) — nn.ZeroPad2d and cuDNN's grouped
 * kernels, forward and backward — inside smp's EfficientNetEncoder (reached from F/lib/pose_regressor.py:608-613).  The FORWARD of
 * the convolution in training is fpc_mbconv_dw above with act 0, scale 1 and shift 0 (v * 1 + 0 is exact).  Conventions of fpc_dwconv3x3_dgrad / _wgrad: dense channel-last f32, w / dw torch's
 * [C][1][k][k] read / written in place, plain f32 FMAs in an order the shape alone fixes, no atomics: bit-identical run to run.
 * The pads are fpc_mbconv_dw's: pad-before pb = (k - 1) / 2 at stride 1, 0 for k = 3 and 1 for k = 5 at stride 2; Ho = Hi / stride,
 * Wo = Wi / stride.  FPC_EINVAL before any launch: a NULL or not 16-byte-aligned pointer, B < 1, C < 4 or C % 4 != 0, k other than
 * 3 or 5, a stride other than 1 or 2, Hi < 1 or Wi < 1, an odd Hi or Wi at stride 2, B Hi Wi C / 4 >= 2^32 - 2^20 - 8 (the 32-bit
 * walk limit of fpc_mbconv_dw).  (k, stride) = (3, 1) is pad 1 on every side: both entries run fpc_dwconv3x3_dgrad / _wgrad's
 * kernels of stride 1 there.
 *
 * fpc_mbconv_dw_dgrad (k_dw_dgrad_s1 / _s2): dx [B][Hi][Wi][C] from dy [B][Ho][Wo][C], every element written exactly once:
 *   dx[h][w] = sum over kh, kw of dy[(h + pb - kh) / stride][(w + pb - kw) / stride] w[kh][kw] where the divisions are exact and
 *   the index is inside dy.  Stride 2 is evaluated per output parity, no zero insertion: k = 3 per axis dx[2a] = dy[a] w[0] +
 *   dy[a - 1] w[2], dx[2a + 1] = dy[a] w[1] (9 products per 2 x 2 block and channel); k = 5 dx[2a] = dy[a] w[1] + dy[a - 1] w[3],
 *   dx[2a + 1] = dy[a + 1] w[0] + dy[a] w[2] + dy[a - 1] w[4] (25 products).
 * fpc_mbconv_dw_wgrad (k_dw_wgrad + k_dw_wgrad_reduce): dw[c][kh][kw] = sum over b, ho, wo of
 *   dy[b][ho][wo][c] x[b][stride ho + kh - pb][stride wo + kw - pb][c], zero outside x; every element of dw is overwritten, a tap
 *   no pixel reaches with an exact zero.  The list of the B Ho (frame, output row) pairs is cut as fpc_dwconv3x3_wgrad's, its
 *   formula with `slots` in place of 32:
 *       slices = max(1, min(max(1, 1024 / ceil(C / 32)), B Ho ceil(Wo / 8) / slots, B Ho)),  slots = 32 (k = 3) or 8 (k = 5)
 *   a function of (B, Ho, Wo, C, k) alone, fpc_dwconv3x3_wgrad's count at k = 3.  One f32 partial [C][k k] per slice (inside a slice: `slots`
 *   pixel slots over its (row, 8-column segment) units in turn, added in a fixed tree; at k = 5 a thread holds one tap row of a
 *   channel quad), the slices added in double in sixteen contiguous ranges, each ascending, the ranges ascending.
 *   ws: fpc_mbconv_dw_wgrad_workspace_bytes(B, Ho, Wo, C, k) = slices * C * k * k * 4 bytes (0 for a refused shape), 256-byte
 *   aligned; too small or misaligned: FPC_EWORKSPACE (a NULL ws: FPC_EINVAL). */
int fpc_mbconv_dw_dgrad(const float* dy, const float* w, float* dx, int B, int Hi, int Wi, int C, int k, int stride, fpc_stream_t stream);
size_t fpc_mbconv_dw_wgrad_workspace_bytes(int B, int Ho, int Wo, int C, int k);
int fpc_mbconv_dw_wgrad(const float* x, const float* dy, float* dw, int B, int Hi, int Wi, int C, int k, int stride, void* ws,
                        size_t ws_bytes, fpc_stream_t stream);

/* ---- The same gate in the training step (csrc/se_train.hip; lib/train_conv.se_gate_add_relu behind FPC_TRAIN_NATIVE_SE=1).  They
 * replace autograd through pretrainedmodels.senet.SEModule and through the add / ReLU of SEResNetBottleneck.forward (aten forward
 * and backward kernels in the reference, reached from F/lib/pose_regressor.py:608-613).  Conventions, shape class and refusals of
 * the entries above: FPC_EINVAL, before any launch, for a NULL pointer (dres alone may be NULL), a pointer that is not 16-byte
 * aligned, C < 64 or C % 64 != 0 or C > 8192, R < 1 or R not dividing C, B < 1 or any other shape the entries above refuse.
 *
 * fpc_se_gate_train (k_se_pool + k_se_excite<SAVE>): fpc_se_gate, the same operations in the same order (the gate's bits are
 *   fpc_se_gate's), that also writes what the backward reads: mean [B][C] (the slab sums in slab order, times 1 / (H W)) and
 *   hidden [B][C / R] = relu(w1 mean + b1).  scratch: fpc_se_scratch_floats(B, H, W, C) floats.
 * fpc_se_bwd_scratch_floats: floats of fpc_se_bwd's scratch = B * (slabs * C + 2 C + C / R) with slabs = fpc_se_pool_slabs(H, W, C):
 *   the per-slab sums, dv, dm and dh; 0 for B < 1, a refused C or R.
 * fpc_se_bwd (k_se_bwd_reduce, k_se_excite_bwd, k_se_param_grad, k_se_bwd_apply): the whole backward of
 *   y = relu(x gate + res) with gate = sigmoid(w2 hidden + b2), hidden = relu(w1 mean + b1), mean = mean_hw(x), from the output
 *   gradient gy and the forward's y, gate, mean, hidden.  With d = gy where y > 0 and 0 elsewhere:
 *     dg[b][c] = sum_hw d x (per slab of pixels, the slabs in slab order), dv = dg gate (1 - gate),
 *     dh[b][j] = (hidden > 0) sum_c dv[c] w2[c][j] (c ascending per thread slice, the slices in order),
 *     dm[b][c] = sum_j dh[j] w1[j][c] (j ascending),
 *     dx = d gate + dm (1 / (H W)),  dres = d (skipped when dres is NULL),
 *     dw2[c][j] = sum_b dv[b][c] hidden[b][j], db2[c] = sum_b dv[b][c], dw1[j][c] = sum_b dh[b][j] mean[b][c],
 *     db1[j] = sum_b dh[b][j] (the batch in batch order).
 *   x, y, gy, dx, dres [B][H][W][C]; dw1 [C / R][C], db1 [C / R], dw2 [C][C / R], db2 [C]: every element of every output is
 *   written exactly once (nothing needs zeroing), gy is only read, dx and dres are distinct from every input and from one another. */
int fpc_se_gate_train(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* gate, float* mean,
                      float* hidden, float* scratch, int B, int H, int W, int C, int R, fpc_stream_t stream);
size_t fpc_se_bwd_scratch_floats(int B, int H, int W, int C, int R);
int fpc_se_bwd(const float* x, const float* y, const float* gy, const float* gate, const float* mean, const float* hidden,
               const float* w1, const float* w2, float* dx, float* dres, float* dw1, float* db1, float* dw2, float* db2, float* scratch,
               int B, int H, int W, int C, int R, fpc_stream_t stream);

/* Weight gradient of a convolution for the training step (BASELINE.json configs[4]; the reference leaves the
 * convolutions' backward to cuDNN through autograd, F/lib/pose_regressor.py:709-743 under Lightning's backward).
 * x: input [B,Hi,Wi,Cin] channel-last (channel stride 1; element strides sb, sh, sw multiples of 4; 16-byte aligned),
 * dy: output gradient NHWC contiguous [B,Ho,Wo,Cout]; dw: OIHW contiguous [Cout,Cin,Kh,Kw], overwritten.
 * Cin % 64 == 0 and Cout % 4 == 0 are required (FPC_EINVAL otherwise); any stride / padding.  Split over the pixels,
 * summed in a fixed order: deterministic.  The data gradient of a stride-1 convolution is fpc_conv2d on the flipped,
 * transposed weights (fastposecnn_amd/lib/train_conv.py). */
size_t fpc_conv2d_wgrad_workspace_bytes(int B, int Ho, int Wo, int Cin, int Cout, int Kh, int Kw);
int fpc_conv2d_wgrad(const float* x, int64_t sb, int64_t sh, int64_t sw, const float* dy, float* dw, int B, int Hi,
                     int Wi, int Cin, int Cout, int Kh, int Kw, int stride, int pad, void* ws, size_t ws_bytes,
                     fpc_stream_t stream);
/* The same sums with split-precision matrix products (see "split precision" above: three bf16 pieces per f32 operand,
 * the six leading piece products accumulated in f32), about twice the f32 matrix rate.  Same workspace and shape rules,
 * deterministic; differs from fpc_conv2d_wgrad in the last bits only (ABI 8). */
int fpc_conv2d_wgrad_split(const float* x, int64_t sb, int64_t sh, int64_t sw, const float* dy, float* dw, int B, int Hi,
                           int Wi, int Cin, int Cout, int Kh, int Kw, int stride, int pad, void* ws, size_t ws_bytes,
                           fpc_stream_t stream);

/* Bilinear upsampling with align_corners = True (the x2 steps of the FPN segmentation blocks and the x4 of the heads:
 * torch.nn.functional.interpolate / nn.UpsamplingBilinear2d in the reference's network, F/lib/pose_regressor.py:608-666),
 * forward and its exact adjoint, ATen's source-index arithmetic.  scale: 2 or 4.  The tensor that is READ is given by its
 * element strides (any layout); the one WRITTEN is contiguous [B,C,.,.], channel-last when *_nhwc != 0.  The backward runs
 * one axis at a time through `scratch` (fpc_upsample_bilinear_bwd_scratch_floats floats; 0 for a shape or scale the
 * backward refuses).  A refused call writes nothing, the scratch included.  Deterministic. */
int fpc_upsample_bilinear_fwd(const float* in, int64_t sb, int64_t sc, int64_t sh, int64_t sw, float* out, int B, int C, int h,
                              int w, int scale, int out_nhwc, fpc_stream_t stream);
size_t fpc_upsample_bilinear_bwd_scratch_floats(int B, int C, int h, int w, int scale);
int fpc_upsample_bilinear_bwd(const float* dout, int64_t sb, int64_t sc, int64_t sh, int64_t sw, float* din, float* scratch,
                              int B, int C, int h, int w, int scale, int din_nhwc, fpc_stream_t stream);
/* The kernel a call of the two above runs on (host arithmetic, the launchers switch on the same result; ABI 11, additive).
 * ptr_low4: the low four bits of the call's pointers, or-ed (in, out; dout, din, scratch); the strides, shape, scale and
 * dst_nhwc (out_nhwc / din_nhwc) as in the call.  backward == 0: 0 = one element per thread, 1 = channel-last on both
 * sides with four channels per thread, 2 = channel-last source -> NCHW through an LDS patch (C <= 32), 3 = NCHW
 * destination with four columns per thread.  backward != 0: the x pass in bits 0-3 and the y pass in bits 4-7, each
 * 0 = one element per thread, 1 = channel-last with four channels per thread, 2 = x-fastest (four rows per thread in
 * the x pass, four columns in the y pass).  FPC_EINVAL where the launcher refuses the shape (null pointers apart). */
int fpc_upsample_bilinear_form(int backward, unsigned ptr_low4, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int B, int C,
                               int h, int w, int scale, int dst_nhwc);

/* GroupNorm + ReLU on channel-last activations for the training step (the decoder blocks' GroupNorm(32, 128) -> ReLU,
 * segmentation_models_pytorch Conv3x3GNReLU, call sites F/lib/pose_regressor.py:608-666): x, y, dy, dx are [B, HW, C]
 * with C = 4 * groups (a group is one float4 of a pixel; groups divides 256 and is <= 64; FPC_EINVAL otherwise).
 * stats [B][groups][2] = mean, rstd (forward -> backward).  part: fpc_groupnorm4_relu_scratch_floats floats; after the
 * backward it holds [B][chunks][C][2] = per-chunk {sum dz, sum dz * xhat}, whose sums over the first two axes are
 * dbeta / dgamma.  Partial sums are combined in double in a fixed order: deterministic. */
size_t fpc_groupnorm4_relu_scratch_floats(int B, int HW, int C);
int fpc_groupnorm4_relu_fwd(const float* x, const float* gamma, const float* beta, float* y, float* stats, float* part, int B,
                            int HW, int C, int groups, float eps, fpc_stream_t stream);
int fpc_groupnorm4_relu_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* stats, float* dx,
                            float* part, int B, int HW, int C, int groups, fpc_stream_t stream);

/* Training-mode BatchNorm2d on channel-last activations, fused with the residual add and the ReLU behind it, forward and
 * backward, for the training step.  Replaces torch.nn.BatchNorm2d (and the add / ReLU after it) inside the smp / torchvision
 * ResNet encoder the reference builds at F/lib/pose_regressor.py:608, under Lightning's training step.  x, res, y, dy, dx,
 * dres are [P, C] f32 (P = B H W pixels, channel stride 1), gamma / beta / dgamma / dbeta [C], stats [C][2] = mean, rstd
 * (forward -> backward); all of them and `part` 16-byte aligned.  FPC_EINVAL for C % 4 != 0, P < 2, a null or misaligned
 * pointer, or a residual without relu (no block has it).  No allocation inside; three launches each way; per-chunk partial
 * sums (centred per chunk) are combined in double in a fixed order: bit-identical from run to run.
 *
 * fpc_batchnorm_scratch_floats: floats of `part`, for the forward and for the backward alike.
 * fpc_batchnorm_fwd: y = (x - mean) rstd gamma + beta over the batch statistics (biased variance, rstd = 1/sqrt(var + eps)),
 *   then y = relu(y) when relu, y = relu(y + res) when res is given too.  running_mean / running_var (both or neither) move
 *   by `momentum` towards the batch mean and the UNBIASED batch variance, as torch's module buffers do.
 * fpc_batchnorm_bwd: with g = dy [y > 0] (relu: the mask of the forward's saved output y; y may be null otherwise) or dy:
 *   dbeta = sum g, dgamma = sum g xhat, dx = gamma rstd (g - dbeta / P - xhat dgamma / P), dres = g.  dx and dres are each
 *   written only when not null (dres needs relu); neither: the elementwise pass is skipped. */
size_t fpc_batchnorm_scratch_floats(int P, int C);
int fpc_batchnorm_fwd(const float* x, const float* res, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, float* y, float* stats, float* part, int P, int C, float eps, float momentum, int relu,
                      fpc_stream_t stream);
int fpc_batchnorm_bwd(const float* x, const float* y, const float* dy, const float* gamma, const float* stats, float* dx,
                      float* dres, float* dgamma, float* dbeta, float* part, int P, int C, int relu, fpc_stream_t stream);
/* The two entries above with an activation code in place of `relu`: act 0 none, 1 ReLU, 2 ReLU6 (the activation behind every
 * BatchNorm but the last of a MobileNetV2 block: nn.ReLU6 in the reference's encoder, aten's hardtanh forward and backward).
 * act 2: y = min(max(z, 0), 6) forward, g = dy [0 < y < 6] on the saved output backward — torch's hardtanh rule on the
 * pre-activation.  Statistics, running buffers and the partial sums are those of the entries above, which are these with
 * act = (relu != 0).  FPC_EINVAL besides theirs: any other act, and a residual (res, dres) with act 2 — no block has it. */
int fpc_batchnorm_act_fwd(const float* x, const float* res, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, float* y, float* stats, float* part, int P, int C, float eps, float momentum, int act,
                          fpc_stream_t stream);
int fpc_batchnorm_act_bwd(const float* x, const float* y, const float* dy, const float* gamma, const float* stats, float* dx,
                          float* dres, float* dgamma, float* dbeta, float* part, int P, int C, int act, fpc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FPC_H_ */
