/*
 * mq_hip.h -- C ABI of libmq_hip.so, the MI355X (gfx950) implementation of the
 * per-frame 2D->3D pose hot path of sidd-bme/macaque-3d-pose-estimation.
 *
 * Conventions:
 *   - every function returns 0 on success, < 0 on error; mq_last_error() gives text;
 *   - the caller owns every data buffer (device pointers unless stated otherwise);
 *     contexts / models own their weights and workspaces;
 *   - work is stream ordered on the hipStream_t passed as `void* stream`
 *     (NULL = the null stream); nothing synchronises unless stated;
 *   - a context owns per-device scratch (decode, Viterbi, optim_points and affinity
 *     workspaces) and a model owns its activations and mq_topdown staging: calls that
 *     share one mq_ctx (or one mq_vitpose) must be issued on ONE stream (or be ordered
 *     by the caller); use one context per stream for concurrent work;
 *   - missing 2D / 3D data is NaN on the way in and out (Viterbi emits (-1,-1,0.001)
 *     for missing frames exactly like anipose).
 *
 * Camera parameter rows (`cams`, float64, 24 values per camera, device memory):
 *   fx, fy, skew, cx, cy, xi, d0, d1, d2, d3, R00..R22 (row-major, from rvec via
 *   Rodrigues), t0, t1, t2, model, d4.  `model` selects the camera class
 *   CameraGroup.from_dicts builds (cameras.py:1972-1982):
 *     0  OmnidirCamera (cameras.py:429-555): K / xi, d0..d3 = D (k1, k2, p1, p2), d4 = 0;
 *     1  Camera, pinhole (cameras.py:173-337): matrix, d0..d4 = distortions (k1, k2, p1, p2, k3),
 *        xi = skew = 0 (cv2.projectPoints / undistortPoints do not use the matrix's skew);
 *     2  FisheyeCamera (cameras.py:339-426): matrix, d0..d3 = distortions (k1..k4), xi = skew = d4 = 0.
 *   Every geometry entry point below (undistort, project, DLT, RANSAC, reprojection error,
 *   optim_points) runs the model of each row; any other model value gives NaN results.
 */
#ifndef MQ_HIP_H
#define MQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history:
 *   1 -- rounds 1-2.
 *   2 -- mq_viterbi_filter accepts n_back in [1, 3] only (was [1, 8]); the timing-ablation tuning keys and
 *        MQ_TUNE_ATTENTION_V2 (key 17, the first-generation attention kernel) were removed and now return -2;
 *        MQ_TUNE_OPTIM_PCG_ITERS defaults to 20 (was 40; optim_points results stay within their tolerance);
 *        mq_det_topk_boxes (config-5 capturable box selection) and mq_optim_prepare (host initialisation) added.
 *   3 -- camera rows carry a model (slot 22: 0 omnidir, 1 pinhole, 2 fisheye) and a fifth distortion
 *        coefficient (slot 23); rows written for ABI 1-2 (zeros there) keep the omnidir meaning.
 *        mq_camera_undistort / mq_camera_project added (mq_omnidir_* are the same functions).
 *   4 -- mq_alldata_json (host: step 1's alldata.json text from row arrays) added.
 *   5 -- mq_add_layernorm added; tuning key MQ_TUNE_OPTIM_STOP (21) added; optim_points defaults to 40 PCG iterations per LM step and
 *        the ftol test on two accepted steps in a row (it lands closer to the converged solution than
 *        scipy's own ftol stop on ViT-derived 2D).
 *   6 -- MQ_TUNE_OPTIM_STOP bit 4: the ftol test at ftol / 2; default 6 (two steps in a row at ftol / 2: at or
 *        below scipy's cost on every marker scene probed, where ftol alone stopped 1.5 % above it on one).
 *   7 -- mq_optim_points takes a solver (0: scipy's trust-region-reflective + lsmr, restated -- the default and
 *        the parity mode; 1: the Levenberg-Marquardt + PCG solver of ABI 1-6) and writes 8 stats per animal;
 *        tuning keys MQ_TUNE_OPTIM_TRF_CHUNK (22), MQ_TUNE_VIT_RESID_F32 (23), MQ_TUNE_ATTN_KRING (24) and
 *        MQ_TUNE_OPTIM_TRF_FB (25) added; tuning key MQ_TUNE_GEMM_BLASLT (26) and mq_gemm_plans added.
 *   8 -- the hipBLASLt route is gone: every GEMM of the library is a hand-written kernel.  MQ_TUNE_GEMM_BLASLT (26)
 *        now returns -2 like any unknown key, and mq_gemm_plans was removed.  MQ_TUNE_GEMM_W4 (27) and the host-only
 *        mq_trust_region_2d added. */
#define MQ_ABI_VERSION 8

typedef struct mq_ctx mq_ctx;
typedef struct mq_vitpose mq_vitpose;

int mq_abi_version(void);
const char* mq_last_error(void);

/* Process-wide knobs for A/B measurement.  The kernel-routing knobs select variants that compute the
 * same results (tested equal); the PCG cap changes only the inner-solve accuracy of optim_points,
 * whose results stay within that stage's tolerance.  No knob can select a variant that computes
 * something else.  Changing one makes the next mq_vitpose_forward re-capture its graph. */
#define MQ_TUNE_GEMM_FORCE_SMALL 2  /* 1: route every GEMM to the 128x128 / 64x64 kernel (default 0; the reference
                                       route of the bitwise implicit-convolution tests) */
#define MQ_TUNE_OPTIM_PCG_ITERS 4   /* cap on the conjugate-gradient iterations per Levenberg-Marquardt step (default 40;
                                       results stay within the optim_points tolerance) */
#define MQ_TUNE_GEMM_PINGPONG 12    /* 1 (default): 256x256 GEMMs with K % 64 == 0 on the ping-pong kernel (wave groups
                                       alternate LDS traffic and MFMA, gemm_pp.hip); 0: the interleaved-K-step kernel */
#define MQ_TUNE_OPTIM_PRECOND_LDS 18 /* 1 (default): optim_points' preconditioner on the series staged in LDS when it
                                        fits; 0: the global-memory substitution kernel (same preconditioner) */
#define MQ_TUNE_GEMM_TILE64 19      /* 1 (default): GEMMs whose 128x128 tiles cannot occupy every CU once take the
                                       64x64-tile kernel (same accumulation order, tested equal); 0: 128x128 */
#define MQ_TUNE_QKV_HEAD_MAJOR 20   /* 1 (default): the ViT qkv GEMM writes Q / K / V head-major (each head's rows
                                       contiguous) for the attention's loads; 0: row-major (same results) */
#define MQ_TUNE_OPTIM_STOP 21       /* optim_points' stop rule on an accepted LM step, bits: 0 = scipy's ftol test
                                       alone (dF < ftol F); 1 = and the step's actual / predicted reduction > 0.25
                                       (scipy trf's condition); 2 = the test passed on two accepted steps in a row;
                                       4 = the test at ftol / 2.  Default 6 (2 | 4).  Levenberg-Marquardt solver only */
#define MQ_TUNE_VIT_RESID_F32 23    /* 1: the ViT's proj / fc2 add their f32 accumulators to the residual stream in the
                                       GEMM epilogue (rounds 1-3); 0 (default): bf16 branch outputs added in the
                                       LayerNorm passes (round 4).  A precision A/B knob */
#define MQ_TUNE_ATTN_KRING 24       /* 1 (default): 192-token attention with the inline-asm K-fragment ring; 0: the
                                       compiler-scheduled loop (bit-identical; the fallback for a toolchain change) */
#define MQ_TUNE_OPTIM_TRF_CHUNK 22  /* lsmr iterations the trust-region solver launches between two reads of its done
                                       flags (default 16, 1..64; same results) */
#define MQ_TUNE_OPTIM_TRF_FB 25     /* most frames per workgroup of the trust-region solver's kernels (default 4, 1..4;
                                       same algorithm, the fixed reduction order follows the blocks) */
#define MQ_TUNE_GEMM_W4 27          /* 1: the ViT's bf16-output GEMMs (qkv, proj, fc1, fc2, deconv 1) on the one-wave-per-SIMD
                                       256x256 kernel (128 x 128 per wave, gemm_w4.hip); 0: the ping-pong kernel.  Same
                                       accumulation order, the same bits */
int mq_set_tuning(int key, int value);
/* Current value of a tuning knob (negative on an unknown key). */
int mq_get_tuning(int key);
/* Bind a context to HIP device `device`. */
int mq_create(int device, mq_ctx** out);
int mq_destroy(mq_ctx* ctx);

/* ======================================================================= pose
 * Replaces mmpose.apis.init_model + inference_topdown for the ViTPose top-down
 * model (reference: src/pipeline/step1_proc2d.py:100-101 init, :294-298 call,
 * model/pose/td-hm_ViTPose-huge_8xb64-210e_coco-256x192_sn_macaque.py:54-110).
 */

/* Create an (empty) ViTPose model: ViT-H = (1280, 32, 16, 5120, 17); ViT-B = (768, 12, 12, 3072, 17). */
int mq_vitpose_create(mq_ctx* ctx, int embed_dims, int num_layers, int num_heads, int ffn_dims, int n_joints,
                      mq_vitpose** out);
int mq_vitpose_destroy(mq_vitpose* model);

/* Load one float32 parameter by its mmpose state_dict name (e.g.
 * "backbone.layers.3.attn.qkv.weight", "head.deconv_layers.1.running_var").
 * `data` is device memory if on_device != 0, host memory otherwise.  Synchronous. */
int mq_vitpose_set_param(mq_vitpose* model, const char* name, const float* data, int64_t numel, int on_device);

/* Verify every parameter was loaded and fold the eval BatchNorms. */
int mq_vitpose_finalize(mq_vitpose* model);

/* Enable (1) / disable (0) hipGraph capture + replay of mq_vitpose_forward. */
int mq_vitpose_set_graph(mq_vitpose* model, int enable);

/* Live kernel timing for roofline reporting: while enabled, eager forwards (graph
 * replay is bypassed) record hipEvents around every FFN fc1 GEMM launch on the
 * launch stream.  _result synchronises on them and returns the average duration
 * (ms) per launch, the launch count, and the algorithmic FLOPs of one launch. */
int mq_vitpose_timing(mq_vitpose* model, int enable);
int mq_vitpose_timing_result(mq_vitpose* model, double* avg_ms, int* count, int64_t* flops_per_launch);

/* GetBBoxCenterScale(1.25) + TopdownAffine(UDP, 192x256) + PoseDataPreprocessor.
 *   frames   : uint8 BGR images, image i at frames + i * frame_stride, each height x width x 3
 *   boxes    : float32 (n, 4) xyxy;  box_frame : int32 (n,) image index of each box
 *   crops    : float32 (n, 3, 256, 192) normalised RGB (the model input)
 *   center, scale : float32 (n, 2)  (PoseDataSample input_center / input_scale)      */
int mq_crop_udp(mq_ctx* ctx, const uint8_t* frames, int64_t frame_stride, int height, int width,
                const float* boxes, const int32_t* box_frame, int n, float* crops, float* center, float* scale,
                void* stream);

/* Heatmaps of n crops: float32 (n, J, 64, 48).  With flip_test the model runs 2n
 * forwards and returns (H + flip_back(H_flip)) * 0.5 (test_cfg flip_mode 'heatmap'). */
int mq_vitpose_forward(mq_vitpose* model, const float* crops, int n, int flip_test, float* heatmaps, void* stream);

/* UDPHeatmap.decode (get_heatmap_maximum + refine_keypoints_dark_udp, blur 11) and
 * add_pred_to_datasample.  kp_img float64 (n, J, 2) image pixels; score float32 (n, J);
 * argmax int32 (n, J) flat heatmap index; kp_hm float32 (n, J, 2) heatmap-space (may be NULL). */
int mq_decode_udp(mq_ctx* ctx, const float* heatmaps, int n, int n_joints, int hm_h, int hm_w,
                  const float* center, const float* scale, double* kp_img, float* score, int32_t* argmax,
                  float* kp_hm, void* stream);

/* mq_decode_udp keeping up to n_cand (1..4) peaks per (instance, joint) instead of the first argmax only
 * (the reference's codec, td-hm_ViTPose-huge_8xb64-210e_coco-256x192_sn_macaque.py:4-14, keeps one; the
 * consumers of several are filter_pose.py:151-186 and cameras.py:639-724).
 *   kp_img float64 (n, J, n_cand, 2); score float32 (n, J, n_cand); peak int32 (n, J, n_cand) flat heatmap
 *   index; kp_hm float32 (n, J, n_cand, 2) (may be NULL).  Empty slots hold NaN, 0, -1, NaN.
 * The rule, on the raw averaged heatmap H of one (instance, joint):
 *   - pixel p is a peak iff H[p] > min_score and every in-map 8-neighbour q has H[p] > H[q], or
 *     H[p] == H[q] with flat index p < q (a plateau yields one peak, its lowest index);
 *   - slots are filled greedily: the highest remaining peak (lowest flat index on ties) whose Chebyshev
 *     distance to every peak already taken is > min_sep, until n_cand slots are full or no peak is left;
 *   - slot 0 is mq_decode_udp's result bit for bit in all four outputs (also for max <= 0: loc -1);
 *   - when the map's maximum is <= max(0, min_score) there are no peaks: slots 1.. stay empty;
 *   - slot k >= 1 gets the same DARK-UDP step on the same log-blurred map and the same image-space
 *     mapping; its score is H[peak].
 * NaN heatmaps: defined for slot 0 only (as mq_decode_udp).  min_sep 3 and min_score 0 are the defaults
 * of the Python layer. */
int mq_decode_udp_topk(mq_ctx* ctx, const float* heatmaps, int n, int n_joints, int hm_h, int hm_w,
                       const float* center, const float* scale, int n_cand, int min_sep, float min_score,
                       double* kp_img, float* score, int32_t* peak, float* kp_hm, void* stream);

/* crop -> forward(flip) -> decode in one call (inference_topdown batched over boxes of
 * many views).  heatmaps may be NULL. */
int mq_topdown(mq_vitpose* model, const uint8_t* frames, int64_t frame_stride, int height, int width,
               const float* boxes, const int32_t* box_frame, int n, int flip_test, double* kp_img, float* score,
               int32_t* argmax, float* heatmaps, void* stream);

/* bf16 MFMA GEMM building block used by the forward: C[M,N] = A[M,K] * W[N,K]^T + bias
 * (A, W bf16 K-contiguous; leading dims in elements).  epilogue: 0 C bf16, 1 C bf16 with
 * exact-erf GELU, 2 C f32 += (residual), 3 C f32 = . + aux[m % aux_rows][n] (pos_embed),
 * 4 C f32, 5 C f32 scattered to [m / aux_rows][n][m % aux_rows] (NCHW), 6 C bf16 = max(., 0) (ReLU).
 * bias/aux may be NULL. */
int mq_gemm_bf16(mq_ctx* ctx, const void* A, const void* W, void* C, const float* bias, const float* aux, int M,
                 int N, int K, int lda, int ldw, int ldc, int aux_rows, int epilogue, void* stream);

/* k x k / stride / pad convolution as an implicit GEMM (no im2col buffer): x bf16 NHWC (n_img, height, width,
 * ch), ch % 64 == 0; w bf16 (cout, k * k * ch) in the mq_id_im2col order ((ky * k + kx) * ch + c); out
 * (n_img * OH * OW, cout) with epilogue 0 (bf16), 4 (f32) or 6 (ReLU bf16) of mq_gemm_bf16, plus bias.  The
 * same bits as mq_id_im2col + mq_gemm_bf16: the ID classifier's 3x3 and strided 1x1 convolutions. */
int mq_id_conv_bf16(mq_ctx* ctx, const uint16_t* x, int n_img, int height, int width, int ch, int k, int stride,
                    int pad, const uint16_t* w, const float* bias, void* out, int cout, int epilogue, void* stream);

/* C f32 (M, ldc) = max(C + A W^T + bias, 0) and out bf16 (M, ldc) = the same values: a ResNet bottleneck's
 * conv3 + residual add + ReLU in one pass (mmpretrain Bottleneck.forward, the ID classifier
 * model/id/sn_resnet152_8xb32_in1k_pretrained_optimized_finetuned.py backbone), K % 64 == 0. */
int mq_gemm_resid_relu_bf16(mq_ctx* ctx, const void* A, const void* W, float* C, const float* bias, uint16_t* out,
                            int M, int N, int K, int lda, int ldw, int ldc, void* stream);

/* ======================================================================= detector
 * Building blocks of the step-1 detector, Swin-S Mask R-CNN bbox only
 * (model/detection/SWIN-Mask_R-CNN_bbox_only.py:29-226, inference_detector at step1_proc2d.py:226):
 * the GEMMs and LayerNorms of the backbone / FPN / heads go through mq_gemm_bf16 and mq_layernorm;
 * mqhip/detector.py sequences them.  Feature maps are NHWC f32, GEMM operands bf16 (uint16 storage).
 * Pointers are device pointers unless marked host. */

/* cv2.resize(INTER_LINEAR) of uint8 BGR frames (n_img, height, width, 3) to (new_h, new_w) with the
 * 11-bit coefficient tables xofs/xalpha (new_w, 2 per x) and yofs/yalpha (new_h) (device int32), then
 * BGR->RGB, (x - mean) / std, zero pad to (pad_h, pad_w), written as the 4x4 stride-4 patch-embed
 * im2col operand: patches bf16 (n_img * pad_h/4 * pad_w/4, 64), k = c * 16 + kh * 4 + kw, k >= 48 zero. */
int mq_det_resize_patch(mq_ctx* ctx, const uint8_t* frames, int64_t frame_stride, int n_img, int height, int width,
                        int new_h, int new_w, int pad_h, int pad_w, const int32_t* xofs, const int32_t* xalpha,
                        const int32_t* yofs, const int32_t* yalpha, uint16_t* patches, void* stream);

/* LayerNorm over rows of f32 x (rows, dim), dim % 4 == 0 and <= 3072: y bf16 (out_f32 = 0) or f32. */
int mq_layernorm(mq_ctx* ctx, const float* x, const float* gamma, const float* beta, void* y, int rows, int dim,
                 float eps, int out_f32, void* stream);

/* The pre-norm residual update fused in front of a LayerNorm (ABI 5): x (rows, dim) f32 += p1 (+= p2, in that
 * order; the bf16 branch outputs of the previous GEMMs, bias included; p2 may be null), x written back when
 * store_x, y = LayerNorm(x) in bf16.  dim as mq_layernorm.  Used by the ViT (inside mq_vitpose_forward) and
 * the Swin detector's blocks (x = x + attn(norm1 x); x = x + mlp(norm2 x): SWIN-Mask_R-CNN_bbox_only.py:29-61). */
int mq_add_layernorm(mq_ctx* ctx, float* x, const uint16_t* p1, const uint16_t* p2, int store_x, const float* gamma,
                     const float* beta, uint16_t* y, int rows, int dim, float eps, void* stream);

/* Swin (shifted) window attention, window 7, head_dim 32 (dim = 32 * heads): qkv bf16 (n_img * height *
 * width, 3 * dim) of the LayerNorm-ed tokens, qkv_bias f32 (3 * dim) (the q/k/v of the zero-padded
 * tokens), rel_table f32 (169, heads); out bf16 (n_img * height * width, dim).  shift 0 (W-MSA) or 3
 * (SW-MSA); the zero pad to a multiple of 7, the cyclic shift and its -100 mask, window partition
 * and reverse are done inside (ShiftWindowMSA + WindowMSA, mmdet swin.py). */
int mq_window_attention(mq_ctx* ctx, const uint16_t* qkv, const float* qkv_bias, const float* rel_table, uint16_t* out,
                        int n_img, int height, int width, int dim, int heads, int shift, void* stream);

/* PatchMerging gather: x f32 (n_img, height, width, dim) -> out f32 (n_img * ceil(h/2) * ceil(w/2), 4 dim)
 * in nn.Unfold(2, stride 2) order c * 4 + kh * 2 + kw (odd sizes zero padded at the bottom / right). */
int mq_patch_merge_gather(mq_ctx* ctx, const float* x, int n_img, int height, int width, int dim, float* out,
                          void* stream);

/* FPN top-down: lo (n_img, lo_h, lo_w, ch) += nearest-resized hi (n_img, hi_h, hi_w, ch). */
int mq_upsample_add(mq_ctx* ctx, float* lo, const float* hi, int n_img, int lo_h, int lo_w, int hi_h, int hi_w, int ch,
                    void* stream);

/* 3x3 / stride 1 / pad 1 im2col: x f32 NHWC -> out bf16 (n_img * h * w, 9 * ch), k = (ky * 3 + kx) * ch + c. */
int mq_im2col3x3(mq_ctx* ctx, const float* x, int n_img, int height, int width, int ch, uint16_t* out, void* stream);

/* 3x3 / stride 1 / pad 1 convolution as an implicit GEMM (no im2col buffer): x bf16 NHWC (n_img, h, w, ch),
 * ch % 64 == 0; w bf16 (cout, 9 * ch) with k = (ky * 3 + kx) * ch + c (the mq_im2col3x3 order); out
 * (n_img * h * w, ldc) with epilogue 0 (bf16), 4 (f32) or 6 (ReLU bf16) of mq_gemm_bf16, plus bias.
 * Same bits as mq_im2col3x3 + mq_gemm_bf16 on the bf16-rounded input.  Replaces the detector's FPN output
 * convolutions (neck, SWIN-Mask_R-CNN_bbox_only.py:80-89) and the RPN head convolution (rpn_head, :137). */
int mq_conv3x3_bf16(mq_ctx* ctx, const uint16_t* x, int n_img, int height, int width, int ch, const uint16_t* w,
                    const float* bias, void* out, int cout, int ldc, int epilogue, void* stream);

/* ConvTranspose2d(k4, s2, p1) + per-channel affine (eval BatchNorm) + ReLU as ONE implicit GEMM: the four
 * output parity classes are 2x2 convolutions over the input (sub-pixel decomposition), their taps gathered
 * per K-step and the result stored straight into out, bf16 NHWC (n_img, 2 h, 2 w, cout).  x bf16 NHWC
 * (n_img, h, w, ch), ch % 64 == 0, cout % 256 == 0; w_packed = mq_deconv_subpixel_pack of the torch weight
 * [ch][cout][4][4]; shift4 = the BatchNorm shift repeated for the 4 classes (4 * cout floats, may be null).
 * Replaces the head's second deconvolution + col2im (ViTPose HeatmapHead deconv_layers.3/.4/.5,
 * model/pose/td-hm_ViTPose-huge_8xb64-210e_coco-256x192_sn_macaque.py:85-108). */
int mq_deconv_subpixel_pack(mq_ctx* ctx, const float* w, const float* scale, uint16_t* w_packed, int ch, int cout,
                            void* stream);
int mq_deconv_subpixel_bf16(mq_ctx* ctx, const uint16_t* x, int n_img, int height, int width, int ch,
                            const uint16_t* w_packed, const float* shift4, uint16_t* out, int cout, int relu,
                            void* stream);

/* float32 -> bfloat16, round to nearest even (count elements). */
int mq_f32_to_bf16(mq_ctx* ctx, const float* src, uint16_t* dst, int64_t count, void* stream);

/* max_pool2d(kernel 1, stride 2) = every other pixel: x f32 NHWC -> out (n_img, ceil(h/2), ceil(w/2), ch). */
int mq_subsample2(mq_ctx* ctx, const float* x, int n_img, int height, int width, int ch, float* out, void* stream);

/* mmcv batched_nms + nms (offset 0): per image, candidates with valid != 0, visited in descending score
 * order (ties: lower index first), offset by level * (max coordinate + 1) when level != NULL; keep
 * int32 (n_img, max_keep) candidate indices in visiting order (-1 past n_keep). n_cand <= 8192. */
int mq_nms(mq_ctx* ctx, const float* boxes, const float* scores, const uint8_t* valid, const int8_t* level, int n_img,
           int n_cand, float iou_thr, int max_keep, int32_t* keep, int32_t* n_keep, void* stream);

/* RPNHead._predict_by_feat_single + _bbox_post_process for a batch: head f32 rows level-major over the
 * batch (level l, image i, position p at row n_img * sum_{l'<l} h_l' w_l' + i * h_l w_l + p), 15 columns
 * = the 3 anchor logits then 12 deltas (anchor-major); level_hw host
 * int32 (n_levels, 2), strides host int32, base_anchors host f32 (n_levels, 3, 4).  Sigmoid, top nms_pre
 * per level (stable descending), delta2bbox (stds 1, clip to img_h x img_w), w,h > 0, NMS per level,
 * first max_keep: proposals f32 (n_img, max_keep, 4), scores (n_img, max_keep) (may be NULL), counts. */
int mq_rpn_proposals(mq_ctx* ctx, const float* head, int n_img, int n_levels, const int32_t* level_hw,
                     const int32_t* strides, const float* base_anchors, int nms_pre, float img_h, float img_w,
                     float iou_thr, int max_keep, float* proposals, float* scores, int32_t* counts, void* stream);

/* SingleRoIExtractor + RoIAlign(7, sampling 0, aligned): P2..P5 f32 NHWC with 256 channels (level_hw /
 * strides host), rois f32 (n_img, max_rois, 4) with counts per image -> out bf16 (n_img * max_rois,
 * 256 * 49) in (c, 7, 7) order (rows past a count are zero). */
int mq_roi_align(mq_ctx* ctx, const float* p2, const float* p3, const float* p4, const float* p5,
                 const int32_t* level_hw, const int32_t* strides, const float* rois, const int32_t* counts, int n_img,
                 int max_rois, uint16_t* out, void* stream);

/* Shared2FCBBoxHead.predict_by_feat + multiclass_nms (1 class): head f32 (n_img * max_rois, 6) = 2 logits
 * (class, background) + 4 deltas; softmax, delta2bbox (stds 0.1 0.1 0.2 0.2), clip, * (inv_scale_w,
 * inv_scale_h), score > score_thr, NMS, first max_det: det_boxes (n_img, max_det, 4), det_scores, counts. */
int mq_rcnn_post(mq_ctx* ctx, const float* rois, const float* head, const int32_t* counts, int n_img, int max_rois,
                 float img_h, float img_w, float inv_scale_w, float inv_scale_h, float score_thr, float iou_thr,
                 int max_det, float* det_boxes, float* det_scores, int32_t* det_counts, void* stream);

/* Static top-k crop boxes per image from mq_rcnn_post's output, the capturable stand-in for the tracker's
 * box list in the config-5 per-frame graph: per image the first k detections (score order) with score >
 * score_thr whose int()-truncated box has positive extent (step1_proc2d.py:229-240, 255-268), expanded by
 * step 1's dynamic margin + aspect fix in float64 (step1:270-292; margins / aspect as there: 0.2, 0.5,
 * 0.75).  Out (n_img * k slots): boxes f32 (., 4) expanded xyxy, tight f32 (., 4) the truncated box,
 * img_of int32 (.) = image index, valid int32 (.) = 1 for a filled slot (0: placeholder box
 * (0, 0, 192, 256) so the crop stays in bounds). */
int mq_det_topk_boxes(mq_ctx* ctx, const float* det_boxes, const float* det_scores, const int32_t* det_counts,
                      int n_img, int max_det, int k, float score_thr, double min_margin, double max_margin,
                      double desired_ar, float* boxes, float* tight, int32_t* img_of, int32_t* valid, void* stream);

/* ======================================================================= ID classifier
 * Step-1 collar-ID classifier, ResNet-152 + GlobalAveragePooling + LinearClsHead (6 classes)
 * (model/id/sn_resnet152_8xb32_in1k_pretrained_optimized_finetuned.py:41-73), replacing
 * mmpretrain's ImageClassificationInferencer in classify_patches (step1_proc2d.py:140-163).  The
 * convolutions are mq_id_im2col + mq_gemm_bf16 (folded BN bias, MQ_EPI 6 = ReLU); mqhip/resnet_id.py
 * sequences them.  Maps are NHWC. */

/* classify_patches' crop + cv2.resize(patch, (out_size, out_size), INTER_LINEAR): boxes int32 (n, 5) =
 * (frame, x0, y0, x1, y1), the non-empty numpy slice frames[frame][y0:y1, x0:x1]; out u8 (n, out, out, 3). */
int mq_id_crop_resize(mq_ctx* ctx, const uint8_t* frames, int64_t frame_stride, int height, int width,
                      const int32_t* boxes, int n, int out_size, uint8_t* out, void* stream);

/* The inferencer's test pipeline on square u8 BGR images (n, in_size, in_size, 3): ResizeEdge(edge,
 * 'short', cv2 bilinear) + CenterCrop(crop) + to_rgb + (x - mean) / std -> bf16 NHWC (n, crop, crop, 3). */
int mq_id_preprocess(mq_ctx* ctx, const uint8_t* in, int n, int in_size, int edge, int crop, uint16_t* out,
                     void* stream);

/* im2col of a bf16 NHWC map (n, h, w, c) for a kh x kw / stride / zero-pad convolution:
 * out bf16 (n * oh * ow, kpad), k = (ky * kw + kx) * c + ch, zero for k >= kh * kw * c. */
int mq_id_im2col(mq_ctx* ctx, const uint16_t* x, int n, int h, int w, int c, int kh, int kw, int stride, int pad,
                 int kpad, uint16_t* out, void* stream);

/* MaxPool2d(3, 2, 1) on bf16 NHWC -> (n, (h - 1) / 2 + 1, (w - 1) / 2 + 1, c). */
int mq_id_maxpool(mq_ctx* ctx, const uint16_t* x, int n, int h, int w, int c, uint16_t* out, void* stream);

/* x = relu(x) in place (f32, count % 4 == 0) and y = bf16(x). */
int mq_id_relu_bf16(mq_ctx* ctx, float* x, uint16_t* y, int64_t count, void* stream);

/* GlobalAveragePooling + fc (ncls x c f32, bias) + softmax: x f32 (n, hw, c) -> logits, probs f32 (n, ncls). */
int mq_id_head(mq_ctx* ctx, const float* x, int n, int hw, int c, const float* fc_w, const float* fc_b, int ncls,
               float* logits, float* probs, void* stream);

/* ======================================================================= geometry
 * Replaces aniposelib CameraGroup (cameras.py:593-783), anipose filter_pose_viterbi
 * (filter_pose.py:48-186) and the mvpose DLT (multicam_toolbox.py:393-486).
 */

/* Camera.undistort_points (cameras.py:310-316, 376-382, 498-507; the row's model) for every camera:
 * pts/out float64 (C, N, 2) normalised image coordinates.  mq_omnidir_undistort is the ABI-2 name. */
int mq_camera_undistort(mq_ctx* ctx, const double* cams, int n_cams, const double* pts, int n, double* out,
                        void* stream);
int mq_omnidir_undistort(mq_ctx* ctx, const double* cams, int n_cams, const double* pts, int n, double* out,
                         void* stream);

/* Camera.project (cameras.py:318-323, 384-390, 509-516; the row's model) for every camera:
 * p3d (N, 3) -> out (C, N, 2) pixels.  mq_omnidir_project is the ABI-2 name. */
int mq_camera_project(mq_ctx* ctx, const double* cams, int n_cams, const double* p3d, int n, double* out,
                      void* stream);
int mq_omnidir_project(mq_ctx* ctx, const double* cams, int n_cams, const double* p3d, int n, double* out,
                       void* stream);

/* CameraGroup.triangulate: pts (C, N, 2) raw pixels (undistort != 0) or undistorted; out (N, 3). */
int mq_triangulate_dlt(mq_ctx* ctx, const double* cams, int n_cams, const double* pts, int n, int undistort,
                       double* out, void* stream);

/* CameraGroup.reprojection_error: p3d (N,3), p2d (C,N,2) -> out (C,N,2) or (N,) if mean. */
int mq_reproj_error(mq_ctx* ctx, const double* cams, int n_cams, const double* p3d, const double* p2d, int n,
                    int mean, double* out, void* stream);

/* CameraGroup.triangulate_ransac (triangulate_possible with n_possible = 1, cameras.py:724-743):
 * p3d (N,3), picked uint8 (C,N), p2d (C,N,2), err (N).  threshold 0.5 in the reference. */
int mq_triangulate_ransac(mq_ctx* ctx, const double* cams, int n_cams, const double* pts, int n, int min_cams,
                          double threshold, double* p3d, uint8_t* picked, double* p2d, double* err, void* stream);

/* CameraGroup.triangulate_possible (cameras.py:639-724): pts (C, N, P, 2) raw pixels, NaN = absent, P
 * candidates per camera and point.  Cameras with a non-NaN candidate take part in ascending order, each
 * with its candidates in ascending index and then "none"; combinations run in itertools.product order
 * (first camera slowest), skipped when len < min_cams and len != the number of cameras taking part; DLT
 * on undistorted points, mean reprojection error, strict err < best (best starts at 200), stop at the
 * first err < threshold.  p3d (N,3), picked uint8 (C,N,P), p2d (C,N,2), err (N).
 * n_cams <= 16, P <= 4 and (P + 1)^n_cams <= 65,536, else -2. */
int mq_triangulate_possible(mq_ctx* ctx, const double* cams, int n_cams, const double* pts, int n, int n_possible,
                            int min_cams, double threshold, double* p3d, uint8_t* picked, double* p2d, double* err,
                            void* stream);

/* multicam_toolbox.triangulatePoints: und (C,N,2) undistorted, use uint8 (N,C) -> out (N,3). */
int mq_triangulate_pinv(mq_ctx* ctx, const double* cams, int n_cams, const double* und, const uint8_t* use, int n,
                        double* out, void* stream);

/* step-2 cross-view geometry affinity (geometry_affinity2, step2_crossviewmatching.py:373-432),
 * batched over B frames:
 *   points     : float64 (B, M, J, 3) undistorted x, y and keypoint score per detection
 *   cam_of_det : int32 (B, M) camera index of each detection (its dimGroup slot), -1 = padding
 *   affinity   : float64 (B, M, M); padding rows / columns are 0
 * Rays through each keypoint at depth 0 and 1000 (deproject :327-355), mean line distance over the
 * keypoints both detections score above thr_kp (THR_KP = 0.1) when at least 3 qualify, z-score over
 * the frame's entries below 300, logistic(-5 z), 0 beyond 150. */
int mq_geometry_affinity(mq_ctx* ctx, const double* cams, int n_cams, const double* points, const int32_t* cam_of_det,
                         int B, int M, int J, double thr_kp, double* affinity, void* stream);

/* step-3 tracklet lift (step3_crossframematching.py calc_3dtrace :274-302, calc_p3d :1115-1130): one launch
 * lifts n_cells (tracklet, frame) cells.
 *   cams      : camera rows as for mq_omnidir_undistort (intrinsics) and mq_triangulate_pinv (R, t)
 *   row_start : int32 (C, F + 1) CSR offsets of each camera's rows per frame
 *   row_tid   : int32 (R) box id of each row
 *   row_kp    : float64 (R, J, 3) x, y, score per joint (NaN x, y where step 1 wrote NaN), J <= 32
 *   trk       : int32 (K, F, C) box id of tracklet k in camera c at frame f; negative = absent
 *   cells     : int32 (n_cells, 2) the (k, f) cells
 * Per cell and camera the last row of the frame carrying the box id; per joint the cameras whose x is not
 * NaN and whose score is not below thr_kp (0.3 in step 3; calc_3dpose :262-268) are undistorted and solved
 * by the pinv DLT when at least 2.
 *   p3d    : optional float64 (n_cells, J, 3) (NULL to skip)
 *   median : float64 (n_cells, 3) np.nanmedian over the joints;  mean: float64 (n_cells, 3) np.nanmean
 * A cell with fewer than 2 non-negative trk entries gives NaN in p3d and median. */
int mq_tracklet_traces(mq_ctx* ctx, const double* cams, int n_cams, const int32_t* row_start, const int32_t* row_tid,
                       const double* row_kp, int n_rows, int n_frames, int n_joints, const int32_t* trk, int n_trk,
                       const int32_t* cells, int n_cells, double thr_kp, double* p3d, double* median, double* mean,
                       void* stream);

/* step-3 ID votes (count_id_detections :839-870): votes int32 (n_cells, n_class) -- for every camera and every
 * row carrying the cell's box id with row_score > conf_thr (0.8), one vote for row_cls (n_class <= 16;
 * classes outside [0, n_class) are ignored).  row_cls int32 (R), row_score float64 (R); the rest as above. */
int mq_tracklet_id_votes(mq_ctx* ctx, int n_cams, const int32_t* row_start, const int32_t* row_tid,
                         const int32_t* row_cls, const double* row_score, int n_rows, int n_frames,
                         const int32_t* trk, int n_trk, const int32_t* cells, int n_cells, double conf_thr,
                         int n_class, int32_t* votes, void* stream);

/* step-2 matchSVT (step2_crossviewmatching.py:130-216) batched over B keyframes:
 *   S          : float64 (B, Nmax, Nmax) affinity W of each keyframe (first n_det[b] rows / columns used)
 *   n_det      : int32 (B) detections per keyframe (0 = empty keyframe), Nmax <= 64
 *   cam_of_det : int32 (B, Nmax) camera index of each detection (the dimGroup slot); detections of one
 *                camera form one zero block of X
 *   alpha, lambda, mu, tol, max_iter, pselect: matchSVT's keywords (step 2 calls alpha 0.5, lambda 50,
 *                mu 64, tol 5e-4, maxIter 500, pselect 1; dual_stochastic_SVT False -- not supported)
 *   match      : uint8 (B, Nmax, Nmax) = X > 0.5 after the final symmetrisation (0 outside n_det)
 *   x_out      : optional float64 (B, Nmax, Nmax) final X (NULL to skip)
 *   iters      : int32 (B) the last iteration index (the reference's info["iter"]; -1 for empty keyframes)
 * The SVD of the symmetric Y/mu + X is taken as its eigen-decomposition (parallel Jacobi in LDS,
 * warm-started across iterations); see association.hip. */
int mq_match_svt(mq_ctx* ctx, const double* S, const int32_t* n_det, const int32_t* cam_of_det, int B, int Nmax,
                 double alpha, double lambda, double mu, double tol, int max_iter, int pselect, uint8_t* match,
                 double* x_out, int32_t* iters, void* stream);

/* filter_pose_viterbi over every (animal, camera, joint) chain of kp (A,F,C,J,3)
 * [x, y, score] (step 4 layout of kp2d.pickle) -> out (A,F,C,J,3).  Scratch is
 * owned by the context.  score_threshold 0.3, n_back 3, offset_threshold 25 in step 4 (n_back 1..3). */
int mq_viterbi_filter(mq_ctx* ctx, const double* kp, int n_animals, int n_frames, int n_cams, int n_joints,
                      double score_threshold, int n_back, double offset_threshold, double* out, void* stream);

/* filter_pose_viterbi with n_possible candidates per (frame, joint) (filter_pose.py:26-46 remove_dups,
 * 48-120 viterbi_path, 151-186): kp (A,F,C,J,K,3) [x, y, score], K = n_possible in 1..4 -> out (A,F,C,J,3).
 * A candidate with score < score_threshold is NaN; candidate k of a frame is dropped when a lower-index
 * candidate of the frame lies within 5 px (remove_dups); a frame's particles are the surviving candidates
 * of frames i, i-1, ..., i-n_back+1 (ascending candidate index within a frame, scores times 2^-j), or
 * the single (-1, -1, 0.001) when none survives.  n_back 1..3.  K = 1 gives mq_viterbi_filter's bits. */
int mq_viterbi_filter_multi(mq_ctx* ctx, const double* kp, int n_animals, int n_frames, int n_cams, int n_joints,
                            int n_possible, double score_threshold, int n_back, double offset_threshold,
                            double* out, void* stream);

/* Global multi-head self-attention of the ViT encoder (mmpretrain MultiheadAttention, qkv_bias,
 * scale 1/sqrt(head_dim)) -- the building block inside mq_vitpose_forward.
 *   qkv  bf16 (n_img * tokens, 3 * dim) = [q | k | v] per token row; out bf16 (n_img * tokens, dim).
 *   tokens % 32 == 0 and <= 192; head_dim = dim / heads in {64, 80}. */
int mq_attention_bf16(mq_ctx* ctx, const uint16_t* qkv, uint16_t* out, int n_img, int tokens, int dim, int heads,
                      void* stream);

/* optim_points' parameter initialisation on the HOST (no HIP call; host pointers): per animal b of
 * p3ds (B, F, J, 3) float64 (NaN = missing) -> x0 (B, F*J*3 + n_strong + n_weak) = [p3d with every NaN gap
 * of a series linearly interpolated over frames (np.interp; an all-NaN series -> 0), median limb lengths
 * (strong then weak; 0 or > median + 5 MAD -> the median of all)], non-finite -> 0, and scale_smooth_full
 * (B) = scale_smooth / mean |diff(medfilt7(series))|: bit for bit the numpy arithmetic of cameras.py:
 * 1116-1150 / 1670-1697 (np.interp, medfilt_data's padding, np.median, np.linalg.norm and np.mean's
 * summation orders).  constraints: int32 (n_strong + n_weak, 2) joint pairs.  One host thread per animal. */
int mq_optim_prepare(const double* p3ds, int B, int F, int J, const int32_t* constraints, int n_strong, int n_weak,
                     double scale_smooth, double* x0, double* scale_smooth_full);

/* step 1's alldata.json text (step1_proc2d.py:345-375: json.dump of the per-frame row lists
 * [track id, x1, y1, x2, y2, [[x, y, score] x J], assigned id, id score]) from the rows as HOST arrays (no
 * HIP call): nrows int32 (n_frames) rows per frame; tid / assigned int64 (n); box float64 (n, 4); kp
 * float64 (n, J, 3); score float64 (n), n = sum(nrows).  Writes the text, byte for byte Python's
 * json.dumps of those lists (float repr, NaN, ", " separators), into out[cap] and its length into *len;
 * -2 if cap is too small.  Replaces the interpreter-bound json.dumps of step 1's writer. */
int mq_alldata_json(int n_frames, const int32_t* nrows, const int64_t* tid, const double* box, const double* kp,
                    int J, const int64_t* assigned, const double* score, char* out, int64_t cap, int64_t* len);

/* The 2-D trust-region subproblem of scipy's trf (scipy 1.15.3 optimize/_lsq/common.py solve_trust_region_2d, called
 * by trf_no_bounds for each trial step of optim_points' least_squares, cameras.py:1166-1180) on the HOST (no HIP
 * call): minimise 0.5 p^T B p + g^T p subject to |p| <= Delta, B = [B[0] B[1]; B[1] B[2]] (host arrays).  The
 * Newton point when B is positive definite and the point lies inside; else the best boundary point among the real
 * roots of scipy's quartic (found by bracketing and bisection instead of np.roots); when the quartic has no sign
 * change, its touching points, then the Cauchy point -Delta g / |g| (scipy raises there).  Writes p[2]. */
int mq_trust_region_2d(const double* B, const double* g, double Delta, double* p);

/* CameraGroup.optim_points (cameras.py:1116-1190) and optim_points_jointlenfix (:1192-1415) for
 * B animals at once.  Replaces scipy least_squares (cameras.py:1166-1180: trf, 2-point sparse Jacobian,
 * loss 'linear', ftol 1e-3; jointlenfix :1246-1260 adds max_nfev 15) on the analytic Jacobian, with
 *   solver 0: the same algorithm, restated (scipy 1.15.3 trf_no_bounds + lsmr: damped lsmr Gauss-Newton step,
 *             2-D subspace trust region, update_tr_radius, check_termination with ftol / xtol 1e-8 / gtol
 *             1e-8); the parity default (csrc/optim_trf.hip);
 *   solver 1: Levenberg-Marquardt + PCG inner solves with its own stop rule (MQ_TUNE_OPTIM_STOP): a
 *             "converged" mode that stops later than scipy (csrc/optim.hip).
 *   p2d  device (B, C, F, J, 2) float64, NaN = missing coordinate
 *   x    device (B, F*J*3 + n_strong + n_weak) in/out: [p3d, strong lengths, weak lengths]
 *        (the reference's _initialize_params_triangulation layout, :1670-1697)
 *   constraints host int32 (n_strong + n_weak, 2) joint pairs; scale_smooth_full host (B)
 *   reproj_loss 0 linear, 1 soft_l1 (reference default), 2 huber
 *   fix_lengths 1: lengths are constants (jointlenfix variant), only p3d is optimised
 *   max_iter solver 0: max_nfev (0 = scipy's default, 100 x parameters; the jointlenfix call passes 15);
 *            solver 1: Levenberg-Marquardt iterations
 *   stats host (B, 8): initial cost, final cost, iterations, status, then for solver 0 nfev, njev, lsmr
 *         iterations in total, the longest lsmr run.  status, solver 0: scipy's (0 max_nfev, 1 gtol, 2 ftol,
 *         3 xtol, 4 ftol + xtol); solver 1: 1 ftol, 2 max_iter, 3 damping overflow. */
int mq_optim_points(mq_ctx* ctx, const double* cams, int n_cams, const double* p2d, double* x, int n_animals,
                    int n_frames, int n_joints, const int32_t* constraints, int n_strong, int n_weak,
                    const double* scale_smooth_full, double scale_length, double scale_length_weak,
                    double reproj_error_threshold, int reproj_loss, int n_deriv_smooth, int fix_lengths,
                    int max_iter, double ftol, int solver, double* stats, void* stream);

/* CameraGroup.optim_points_possible (cameras.py:1417-1513; residuals _error_fun_triangulation_possible :1622-1667,
 * initialisation _initialize_params_triangulation_possible :1699-1712, pattern
 * _jac_sparsity_triangulation_possible :1795-1847) for B animals at once: optim_points' residuals on a soft 2D point
 * per (camera, frame, joint) cell -- the softmax (beta 5) over one variable per candidate -- plus one row
 * 10 (1 - std(softmax over all n_possible slots)) per cell with a finite candidate.  Replaces scipy least_squares
 * (:1473-1488: trf, 2-point sparse Jacobian, loss 'linear', ftol 1e-3) by the same algorithm on the analytic
 * Jacobian, as mq_optim_points solver 0 (csrc/optim_possible.hip).  Added within ABI 8.
 *   p2d  device (B, C, F, J, n_possible, 2) float64, NaN = absent candidate (any NaN pattern)
 *   x    device (B, F*J*3 + n_strong + n_weak) in/out: [p3d, strong lengths, weak lengths]; the alphas start
 *        at 0 and stay inside the library
 *   alphas_norm  device (B, C, F, J, n_possible) out: the softmax weights, NaN at NaN candidates
 *   cams device (n_cams, 24) float64 camera rows (layout at the top of this file)
 *   constraints host int32 (n_strong + n_weak, 2) joint pairs; scale_smooth_full host (B) float64
 *   reproj_loss 0 linear, 1 soft_l1 (reference default), 2 huber
 *   max_nfev 0 = scipy's default, 100 x parameters (3D points, lengths and one alpha per finite candidate)
 *   stats host (B, 8) float64 out: initial cost, final cost, iterations, scipy's status (0 max_nfev, 1 gtol, 2 ftol,
 *         3 xtol, 4 ftol + xtol), nfev, njev, lsmr iterations in total, the longest lsmr run
 *   stream the HIP stream (hipStream_t) the work is queued on; the call returns after it has finished
 *   solver must be 0; n_possible in [1, 4]; n_frames > n_deriv_smooth; 1 <= n_cams <= 16; n_joints <= 32;
 *   n_strong + n_weak <= 64; n_deriv_smooth in 1..3.  Errors (-2 and mq_last_error) are raised before anything
 *   is launched.
 * A workgroup per block of 4 frames of one animal; an animal's result depends, bit for bit, only on its own
 * problem (not on the batch or the device). */
int mq_optim_points_possible(mq_ctx* ctx, const double* cams, int n_cams, const double* p2d, double* x,
                             double* alphas_norm, int n_animals, int n_frames, int n_joints, int n_possible,
                             const int32_t* constraints, int n_strong, int n_weak, const double* scale_smooth_full,
                             double scale_length, double scale_length_weak, double reproj_error_threshold,
                             int reproj_loss, int n_deriv_smooth, int max_nfev, double ftol, int solver,
                             double* stats, void* stream);

/* ---- Camera-motion compensation for BoT-SORT (csrc/cmc.hip): boxmot 12.0.7 cmc/sift.py SIFT.apply restated
 * stage by stage, HIP from the uint8 frame to the 2x3 warp.  tests/cmc_ref.py is the numpy restatement the
 * kernels mirror; cv2 parity is unpinned.  All pointers are device pointers unless marked host. */
typedef struct mq_cmc mq_cmc;

/* cv2.cvtColor(BGR2GRAY) + cv2.resize(fx = fy = scale, INTER_LINEAR) in cv2's fixed-point arithmetic:
 * frames uint8 (n_img, height, width, 3) -> gray_out uint8 (n_img, rint(height scale), rint(width scale)). */
int mq_cmc_preprocess(mq_ctx* ctx, const uint8_t* frames, int64_t frame_stride, int n_img, int height, int width,
                      double scale, uint8_t* gray_out, void* stream);

/* cv2.SIFT_create(nOctaveLayers=3, contrastThreshold=0.02, edgeThreshold=20).detect (Lowe 2004; sigma 1.6,
 * assumed input blur 0.5): first_octave -1 (2x upsampled base, cv2's default) or 0; mask uint8 (n_img, height,
 * width) or null (a keypoint is dropped where mask[rint(y), rint(x)] == 0, cv2 runByPixelsMask).
 * kps_out float32 (n_img, max_kp, 7) [x, y, size, angle, octave, layer, response] sorted by (octave, layer, y, x,
 * angle), the first max_kp (<= 2048) of them; counts_out int32 (n_img).  dog_out (null, or float32 (n_img,
 * sum over octaves of 5 h_o w_o)) receives the difference-of-Gaussian pyramid, octave-major. */
int mq_sift_detect(mq_ctx* ctx, const uint8_t* gray, int n_img, int height, int width, int first_octave,
                   const uint8_t* mask, int max_kp, float* kps_out, int32_t* counts_out, float* dog_out,
                   void* stream);

/* cv2 SIFT compute (calcSIFTDescriptor, 4 x 4 x 8, clip 0.2, x 512, saturate to uint8) for the first counts[i]
 * keypoints of image i: desc_out uint8 (n_img, max_kp, 128). */
int mq_sift_describe(mq_ctx* ctx, const uint8_t* gray, int n_img, int height, int width, int first_octave,
                     const float* kps, const int32_t* counts, int max_kp, uint8_t* desc_out, void* stream);

/* cv2.BFMatcher(NORM_L2).knnMatch(query, train, k = 2) on the integer squared distance: query / train uint8
 * (n_img, max_kp, 128) with n_query / n_train int32 (n_img) rows in use; idx_out / dist_out int32 (n_img, max_kp,
 * 2), -1 where absent; on equal distance the lower train index comes first. */
int mq_desc_match_knn2(mq_ctx* ctx, const uint8_t* query, const int32_t* n_query, const uint8_t* train,
                       const int32_t* n_train, int n_img, int max_kp, int32_t* idx_out, int32_t* dist_out,
                       void* stream);

/* cv2.estimateAffinePartial2D(src, dst, method = RANSAC, threshold) with a deterministic hypothesis set (every
 * pair when there are <= 2000, else 2000 hashed pairs) and a closed-form least-squares refit over the inliers:
 * pts float64 (n_sets, max_pts, 4) [src x, src y, dst x, dst y], counts int32 (n_sets); warps_out float64
 * (n_sets, 6) row-major 2x3 (identity for <= 4 points), info_out int32 (n_sets, 2) [hypothesis, inliers],
 * mask_out uint8 (n_sets, max_pts). */
int mq_affine_partial_ransac(mq_ctx* ctx, const double* pts, const int32_t* counts, int n_sets, int max_pts,
                             double threshold, double* warps_out, int32_t* info_out, uint8_t* mask_out, void* stream);

/* boxmot SIFT(downscale = 1 / scale) for n_slots cameras: a slot holds one camera's previous keypoints and
 * descriptors on the device.  max_kp <= 2048. */
int mq_cmc_create(mq_ctx* ctx, int n_slots, int height, int width, double scale, int max_kp, mq_cmc** out);
int mq_cmc_destroy(mq_cmc* cmc);
/* forget the previous frame of a slot (-1: of every slot) */
int mq_cmc_reset(mq_cmc* cmc, int slot);
/* SIFT.apply for n_img frames at once (all cameras of a time step): frames uint8 BGR (n_img, height, width, 3);
 * slots host int32 (n_img), distinct; boxes host float64 (n_img, max_boxes, 4) x1 y1 x2 y2 with box_counts host
 * int32 (n_img) (max_boxes 0: none); warps_out host float64 (n_img, 6): previous-frame -> current-frame
 * coordinates at full resolution, the identity on a slot's first frame or with <= 4 good matches; stats_out host
 * int32 (n_img, 4) [keypoints, matches after ratio + gate, good matches, inliers] or null.  Synchronises the
 * stream. */
int mq_cmc_apply(mq_cmc* cmc, const uint8_t* frames, int64_t frame_stride, int n_img, const int32_t* slots,
                 const double* boxes, const int32_t* box_counts, int max_boxes, double* warps_out, int32_t* stats_out,
                 void* stream);

/* ---- Pose overlay (csrc/overlay.hip): the reference's last stage, src/pipeline/visualize_result.py (and
 * visualize_result_2.py), from kp3d to the drawn frame.  tests/overlay_ref.py is the numpy restatement; the
 * coverage rules are this project's own and exact (overlay.hip's head), cv2 parity of the edges is unpinned.
 *
 * The skeleton (host arrays): pairs int32 (n_pairs, 2) joint slots of each limb (draw_kps' kp_con, :73-93),
 * radius int32 (n_joints + 1) disc radius per slot (:102-105; mrksize, eyes mrksize + 1), joint_flags int32
 * (n_joints + 1): bit 0 draw the disc, bit 1 the joint is set to None before drawing (visualize_result_2.py's
 * clean_kp :39-41: no disc and no limb).  Slot n_joints is the neck.  n_joints >= 7, n_animals in [1, 8],
 * n_joints + 1 + n_pairs <= 64. */

/* Primitive tables of n_img output images (visualize_result.py proc :220-242, clean_kp :30-51, the geometry
 * of draw_kps :100-110 and ellipse_line :19-25):
 *   cam_of_img : int32 (n_img) camera row of each image (outside [0, n_cams): nothing is drawn)
 *   kp3d       : float64 (n_img, n_animals, n_joints, 3);  score: float64 (n_img, n_animals, n_joints)
 *   prim_i     : int32 (n_img, n_animals, n_joints + 1 + n_pairs, 8) per slot [valid, cx, cy, r, x0, y0, x1, y1]:
 *                disc slots first (centre from int(), radius), then limb slots (cx = cy = r = 0); x0..y1 is the
 *                inclusive bounding box; an invalid slot is all zero
 *   prim_d     : float64 (n_img, n_animals, n_pairs, 4) limb end points x1, y1, x2, y2 as projected (0 if invalid)
 * The neck is the mean of joints 5 and 6 in 3D and of their scores; a joint is dropped when no joint of the
 * animal has (X != 0) & (score > 0), when its projected x (or y) is NaN, or outside (-1000, 3000) on an axis. */
int mq_overlay_primitives(mq_ctx* ctx, const double* cams, int n_cams, const int32_t* cam_of_img, const double* kp3d,
                          const double* score, int n_img, int n_animals, int n_joints, const int32_t* pairs,
                          int n_pairs, const int32_t* radius, const int32_t* joint_flags, int mrksize,
                          int32_t* prim_i, double* prim_d, void* stream);

/* mq_overlay_primitives, then the fused copy + draw (copy.deepcopy(frame) :218, draw_kps per animal :239-242,
 * cv2.circle / cv2.ellipse thickness -1): out uint8 (n_img, height, width, 3) BGR, image b drawn over
 * frames + src_index[b] * frame_stride (bytes; frames holds n_src images, several outputs may share one; an
 * index outside [0, n_src) reads as black).  out must not overlap frames.  Colours (255,0,0), (0,255,0),
 * (0,0,255), (255,255,255) for animals 0..3, black from 4 (:191, :239-242); a pixel takes the highest animal
 * index covering it.  prim_i / prim_d as above (outputs, and the draw kernel's input). */
int mq_overlay_render(mq_ctx* ctx, const double* cams, int n_cams, const int32_t* cam_of_img, const double* kp3d,
                      const double* score, int n_img, int n_animals, int n_joints, const int32_t* pairs, int n_pairs,
                      const int32_t* radius, const int32_t* joint_flags, int mrksize, const uint8_t* frames,
                      int64_t frame_stride, int n_src, const int32_t* src_index, int height, int width,
                      int32_t* prim_i, double* prim_d, uint8_t* out, void* stream);

/* The labelled overlay: step 3's tracking video (step3_crossframematching.py visualize :1624-1670), where every
 * live tracklet is an "animal" whose colour is its voted collar ID (:1642-1646) and whose key is written at the
 * upper left of its skeleton (cv2.putText :1658-1670).  mq_overlay_primitives' arguments plus device tables:
 *   colour    : int32 (n_img, n_animals) or NULL.  0..3 picks mq_overlay_render's four colours, any other value
 *               (step 3's Cid = -1) is black; NULL keeps "colour = animal index"
 *   label_seg : int32 (n_img, n_animals, max_segs, 4) stroke segments x0, y0, x1, y1 relative to the label
 *               origin, each coordinate in [-8192, 8192] (a label with one outside is not drawn), 16-byte aligned;
 *               label_n int32 (n_img, n_animals) segments in use (clamped to [0, max_segs]); both may be NULL when
 *               max_segs is 0 (no labels);  max_segs in [0, 96];  label_t the stroke thickness in [1, 32]
 *   prim_i    : int32 (n_img, n_animals, n_joints + 2 + n_pairs, 8): mq_overlay_primitives' slots, then the
 *               label slot [valid, origin x, origin y, 0, x0, y0, x1, y1] (so n_joints + 2 + n_pairs <= 64)
 * The origin is (int)x_min, (int)y_min, the NaN-ignoring minima of the projected x and y over all
 * n_joints + 1 slots before any joint is dropped; no label when either minimum is missing or outside
 * [-1000, 3000], or label_n is 0.  The box is the segments' extent padded by ceil(label_t / 2).  Coverage of a
 * segment p0 -> p1 at pixel X, in integers (e = p1 - p0, w = X - p0): w.e <= 0: 4|w|^2 <= t^2; w.e >= |e|^2:
 * 4|X - p1|^2 <= t^2; else 4 (w x e)^2 <= t^2 |e|^2.  The rule and the stroke font that feeds it
 * (mqhip/overlay.py) are this project's own: cv2's Hershey glyphs and thick-line rasteriser are unpinned. */
int mq_overlay_primitives_labelled(mq_ctx* ctx, const double* cams, int n_cams, const int32_t* cam_of_img,
                                   const double* kp3d, const double* score, int n_img, int n_animals, int n_joints,
                                   const int32_t* pairs, int n_pairs, const int32_t* radius,
                                   const int32_t* joint_flags, int mrksize, const int32_t* colour,
                                   const int32_t* label_seg, const int32_t* label_n, int max_segs, int label_t,
                                   int32_t* prim_i, double* prim_d, void* stream);

/* mq_overlay_primitives_labelled, then the fused copy + draw of mq_overlay_render (visualize :1622, :1656,
 * :1667-1670).  A label belongs to its animal's layer: over that animal's skeleton, under every higher animal's
 * skeleton and label.  More than 8 tracklets: render in passes, a pass's output being the next pass's frames. */
int mq_overlay_render_labelled(mq_ctx* ctx, const double* cams, int n_cams, const int32_t* cam_of_img,
                               const double* kp3d, const double* score, int n_img, int n_animals, int n_joints,
                               const int32_t* pairs, int n_pairs, const int32_t* radius, const int32_t* joint_flags,
                               int mrksize, const uint8_t* frames, int64_t frame_stride, int n_src,
                               const int32_t* src_index, int height, int width, const int32_t* colour,
                               const int32_t* label_seg, const int32_t* label_n, int max_segs, int label_t,
                               int32_t* prim_i, double* prim_d, uint8_t* out, void* stream);

/* Bilinear resize of uint8 BGR images (csrc/resize.hip): cv2.resize(img, [800, 600]) of visualize :1685 and
 * visualize_result.py :164, :249, after cv2's 8-bit INTER_LINEAR fixed-point scheme.  src (n, H, W, 3) at
 * src_stride bytes per image, dst (n, h, w, 3) at dst_stride; they must not overlap.  Per axis, with
 * scale = (double)src / dst: f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s; s < 0: s = 0, f = 0;
 * s >= src - 1: s = src - 1, f = 0; taps s and min(s + 1, src - 1) with c1 = rint(f * 2048f),
 * c0 = rint((1f - f) * 2048f) in float32.  R = I[s] * a0 + I[s1] * a1 along x; out =
 * (((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2 along y, saturated to [0, 255].  This is the
 * project's restatement (tests/track_video_ref.py, equal bit for bit); parity with cv2 itself is unpinned. */
int mq_resize_bilinear(mq_ctx* ctx, const uint8_t* src, int64_t src_stride, int n, int height, int width,
                       uint8_t* dst, int64_t dst_stride, int out_height, int out_width, void* stream);

/* Bundle adjustment of the camera rig on marker traces (multicam_toolbox.py optimize_extrinsic :488-636 and
 * optimize_all_camera_params :638-824): a Schur-complement Levenberg-Marquardt with Marquardt scaling that
 * stands in for the reference's least_squares(method='trf', x_scale='jac') call (:611, :776).
 *   mode       : 0 -- 6 parameters per camera (rvec, tvec), residual (R X + t)[:2] / (R X + t)[2] - undistorted
 *                point (:566-589); 1 -- 16 per camera in the reference's order rvec, tvec, K00, K01, K02, K11,
 *                K12, xi, D[4] (:692-694), residual = omnidir projection - pixel (:724-751)
 *   cam_params : HOST float64 (n_cams, 6 or 16), in / out;  n_cams <= 16
 *   points3d   : device float64 (n_points, 3), in / out
 *   obs        : device float64 (n_cams, n_points, 2);  use : device uint8 (n_points, n_cams)
 *   fix_cam0   : freeze camera 0's six extrinsic parameters (:585-586, :746-747); a camera nobody observes keeps
 *                its parameters
 *   ftol       : stop when an accepted step with gain ratio > 1/4 lowers the cost by less than ftol * cost
 *                (the reference: 1e-5 :611, 1e-3 :639);  xtol: step norm below xtol * (xtol + |x|)
 *   max_iter   : trial steps (accepted or rejected); 0 only evaluates
 *   resid      : device float64 (n_points, n_cams, 2) or NULL: residuals at the returned parameters, 0 where unused
 *   info       : HOST, 8 doubles: initial cost, final cost (1/2 sum r^2), trial steps, stop reason (1 max_iter,
 *                2 ftol, 3 xtol, 4 damping exhausted), accepted steps, final lambda, linearisations, free camera
 *                unknowns
 * Every sum has a fixed order (no floating-point atomics): two calls give the same bits.  Synchronises stream. */
int mq_bundle_adjust(mq_ctx* ctx, int mode, int n_cams, int n_points, double* cam_params, double* points3d,
                     const double* obs, const uint8_t* use, int fix_cam0, double ftol, double xtol, int max_iter,
                     double* resid, double* info, void* stream);

/* Bundle adjustment of a camera group on 2D points (aniposelib cameras.py:894-980, CameraGroup.bundle_adjust with
 * its _error_fun_bundle, extra = None, loss = 'linear'): the solver of mq_bundle_adjust on the reference's
 * parametrisation.  Every camera and every point is an unknown (no camera is fixed: the damping carries the
 * 7-dimensional gauge); residual = projection - pixel on the reduced model Camera.set_params leaves
 * (:290-299, :392-403, :518-529).
 *   cam_fixed  : HOST float64 (n_cams, 11): the model (0 omnidir, 1 pinhole, 2 fisheye, the camera rows' ids),
 *                then what the solve does not move: cx, cy (pinhole, fisheye; the rest unused) or K00, K01, K02,
 *                K11, K12, xi, D[4] (omnidir)
 *   cam_params : HOST float64 (n_cams, 9), in / out: rvec, tvec, f, k1, k2.  pinhole: u = f x (1 + k1 r2 + k2 r2^2)
 *                + cx on x = Xc0 / Xc2; fisheye: u = f x theta_d / r + cx, theta_d = theta (1 + k1 theta^2 + k2
 *                theta^4), theta = atan r (theta_d / r = 1 at r <= 1e-8); omnidir: cv2.omnidir.projectPoints with
 *                the fixed K, xi, D -- f, k1, k2 do not enter (:509-516)
 *   free_mask  : HOST uint8 (n_cams * 9): the columns the solve may move.  Slot 8 is free only with extra_dist;
 *                slots 6-8 of an omnidir camera must be frozen (-2 otherwise); columns of a camera nobody observes
 *                are removed as well
 *   points3d, obs, use, ftol, xtol, max_iter, resid, info: as mq_bundle_adjust.  A point one camera sees is legal:
 *                its 3 x 3 block is rank 2 and moves through the damping alone; a block that cannot be inverted
 *                counts as a rejected step
 * Argument errors return -2.  The same bits on every call.  Synchronises stream. */
int mq_bundle_adjust_group(mq_ctx* ctx, int n_cams, int n_points, const double* cam_fixed, double* cam_params,
                           const uint8_t* free_mask, double* points3d, const double* obs, const uint8_t* use,
                           double ftol, double xtol, int max_iter, double* resid, double* info, void* stream);

/* ---- Camera calibration from detected points (csrc/calib.hip): the fits the reference takes from OpenCV in
 * calibrate_intrinsic (multicam_toolbox.py:74-116: cv2.calibrateCamera :96, cv2.omnidir.calibrate :100-111) and in
 * get_extrinsic_from_cagekeypoints (:213-242: cv2.solvePnP :234).  A problem is one camera: 10 intrinsic slots
 * and one pose (rvec, tvec) per view.  OpenCV is not a dependency; parity with it is not pinned.
 *   model       : 0 omnidir -- slots fx, fy, s, cx, cy, xi, k1, k2, p1, p2 (cv2.omnidir.projectPoints);
 *                 1 pinhole -- slots fx, fy, cx, cy, k1, k2, p1, p2, k3, unused (cv2.projectPoints)
 *   view_prefix : HOST int32 (n_prob + 1): problem p owns views view_prefix[p] .. view_prefix[p + 1]; a problem
 *                 may have no views
 *   pt_prefix   : HOST int32 (n_views + 1): view v owns points pt_prefix[v] .. pt_prefix[v + 1], at least 4
 *   obj, img    : device float64 (n_pts, 3) object points and (n_pts, 2) pixels
 *
 * mq_calib_init: closed-form starts.  Planar views (smallest eigenvalue of the object points' scatter matrix below
 * 1e-3 of the middle one): Hartley-normalised DLT homography; with use_intrinsics = 0 Zhang's two constraints per
 * view give fx, fy with the centre fixed at ((width - 1) / 2, (height - 1) / 2) and zero distortion (the omnidir
 * start: fx, fy doubled, xi = 1), and K^-1 H gives each pose.  With use_intrinsics != 0 the given slots are kept,
 * the pixels are normalised through them, and only poses are made; a non-planar view then takes a 3 x 4 DLT on
 * at least 6 points.
 *   intrinsics  : HOST float64 (n_prob, 10), in (use_intrinsics) / out;  poses : HOST float64 (n_views, 6), out
 * Returns -2 (nothing written) for an argument error, a non-planar view without intrinsics or with fewer than 6
 * points, a singular focal-length system, or a non-finite pose.
 *
 * mq_calibrate_views: Levenberg-Marquardt on the Schur complement of the 6 x 6 view blocks, Marquardt scaling,
 * the whole iteration in one launch with one workgroup per problem; mq_bundle_adjust's step rules.
 *   free_mask   : HOST uint8 (n_prob, 10): the intrinsic slots the solve may move; all zero is the pose-only
 *                 problem (solvePnP).  Slot 9 of a pinhole problem must be 0.
 *   ftol, xtol, max_iter : as mq_bundle_adjust (ftol = 0 disables the cost rule; max_iter = 0 only evaluates)
 *   intrinsics, poses : HOST, in / out;  resid : device float64 (n_pts, 2) or NULL, projection - pixel at the result
 *   info        : HOST float64 (n_prob, 8) in mq_bundle_adjust's layout; info[7] counts the problem's unknowns
 *                 (free slots + 6 per view).  A problem without views keeps its slots: cost 0, stop reason 4.
 * No floating-point atomics, no dependence between problems: the same bits on every call and in every batch.
 * Both synchronise stream. */
int mq_calib_init(mq_ctx* ctx, int model, int n_prob, const int* view_prefix, const int* pt_prefix,
                  const double* obj, const double* img, int width, int height, int use_intrinsics,
                  double* intrinsics, double* poses, void* stream);
int mq_calibrate_views(mq_ctx* ctx, int model, int n_prob, const int* view_prefix, const int* pt_prefix,
                       const double* obj, const double* img, const uint8_t* free_mask, double ftol, double xtol,
                       int max_iter, double* intrinsics, double* poses, double* resid, double* info, void* stream);

/* ---- Chessboard corners (csrc/chessboard.hip, csrc/chessboard_dev.hpp): the detection the reference takes from
 * OpenCV in analyze_chessboardvid (multicam_toolbox.py:22-72: cv2.findChessboardCorners :58, cv2.cornerSubPix :61),
 * as a detector of this project's own for the 9 x 6 pattern.  tests/chessboard_ref.py is the numpy restatement:
 * the response, the candidates and the grid are integer and equal it exactly; the refinement is float64 without FMA
 * contraction.  OpenCV is not a dependency; parity with it is not pinned.  All pointers are device pointers; every
 * call is stream-ordered with no host round trip (the context's workspace grows on the first call of a size).
 * n_img in [0, 65535] (0 returns at once), height and width in [1, 32767].
 *
 * mq_chess_response (replaces the feature stage inside :58): gray uint8 (n_img, height, width) -> resp_out int32
 * (n_img, height, width).  3 x 3 binomial blur ((1 2 1)^T (1 2 1), + 8 >> 4, replicated border), then ChESS
 * (Bennett & Lasenby) on the ring of 16 samples at radius 5: R = max(0, 5 SR - 5 DR - |5 S - 16 L|), 0 in the
 * 5-pixel border.
 *
 * mq_chess_candidates (:58): the pixels with R > 0 that equal the maximum of their 9 x 9 neighbourhood, the first
 * max_candidates (in [1, 1024]) of them under (R descending, y ascending, x ascending): pos_out int32 (n_img,
 * max_candidates, 2) [x, y], resp_out int32 (n_img, max_candidates), count_out int32 (n_img); rows past the count are
 * zero.  A radix select over the unique keys (R << 32 | ~(y width + x)) and a sort: the same result on every call.
 *
 * mq_chess_grid (:58): per image, seeds in candidate order (at most 54) over the candidates with 4 R >= the
 * strongest R; the nearest candidate and the nearest one more than 30 degrees off it span the first cell, and the
 * grid grows by local prediction (2 p - p_opposite, or p + the neighbouring row's step) accepting the nearest unused
 * candidate within 0.3 of the predicted step.  A seed is accepted with exactly 54 cells in a 9 x 6 block.  The order
 * is objp's (:34-35): 9 along the fast axis, not mirrored (cross(c[1] - c[0], c[9] - c[0]) > 0, y down), and of the
 * two orders 180 degrees apart the one whose first corner has the smaller (y, x).  found_out int32 (n_img);
 * corners_out float64 (n_img, 54, 2) = p / scale + (1 / scale - 1) / 2, NaN when not found; index_out (null, or
 * int32 (n_img, 54)) the candidate indices, -1 when not found.
 *
 * mq_corner_subpix (:61): cv2.cornerSubPix as documented -- window (2 win + 1)^2 with weights exp(-(i / win)^2)
 * exp(-(j / win)^2), a (2 win + 3)^2 bilinear patch with replicated border per iteration, central differences, the
 * 2 x 2 normal equations; stops on |det| <= eps_machine^2, a step <= eps, leaving the image, or max_iter iterations;
 * a corner that moved more than win in x or y returns to its start.  corners float64 (n_img, per_image, 2) in / out
 * (NaN stays NaN); found (null, or int32 (n_img)): the corners of an image with found == 0 are set to NaN.
 * win in [1, 16].  One wave per corner.
 *
 * mq_find_chessboard (:57-61): frames uint8 BGR (height, width, 3), frame i at frames + i * frame_stride ->
 * cvtColor(BGR2GRAY) -> detection on the copy reduced by scale (mq_cmc_preprocess's resize; scale = 1: the gray
 * image itself) -> refinement on the full-size gray image.  max_candidates in [54, 1024].  Arguments out of range
 * return -2 before anything is launched. */
int mq_chess_response(mq_ctx* ctx, const uint8_t* gray, int n_img, int height, int width, int32_t* resp_out,
                      void* stream);
int mq_chess_candidates(mq_ctx* ctx, const int32_t* resp, int n_img, int height, int width, int max_candidates,
                        int32_t* pos_out, int32_t* resp_out, int32_t* count_out, void* stream);
int mq_chess_grid(mq_ctx* ctx, const int32_t* pos, const int32_t* resp, const int32_t* count, int n_img,
                  int max_candidates, double scale, int32_t* found_out, double* corners_out, int32_t* index_out,
                  void* stream);
int mq_corner_subpix(mq_ctx* ctx, const uint8_t* gray, int n_img, int height, int width, double* corners,
                     int per_image, const int32_t* found, int win, int max_iter, double eps, void* stream);
int mq_find_chessboard(mq_ctx* ctx, const uint8_t* frames, int64_t frame_stride, int n_img, int height, int width,
                       double scale, int win, int max_iter, double eps, int max_candidates, int32_t* found_out,
                       double* corners_out, void* stream);

/* ---- ArUco markers (csrc/aruco.hip, csrc/aruco_dev.hpp): the detection the reference takes from OpenCV in
 * analyze_aruco_marker_vid and analyze_aruco_cube_vid (multicam_toolbox.py:244-391: cv2.resize :281, :354,
 * aruco.detectMarkers :283, :356), as a detector of this project's own for 4 x 4 codes in a one-cell border.  The
 * caller passes the dictionary; cv2's predefined ones are not included.  tests/aruco_ref.py is the numpy restatement:
 * the threshold, the labels and the components are integer and equal it exactly; the per-quad stage is float64 without
 * FMA contraction.  OpenCV is not a dependency; parity with cv2.aruco is not pinned.  All pointers are device
 * pointers; every call is stream-ordered with no host round trip (the context's workspace grows on the first call of a
 * size).  n_img in [0, 65535] (0 returns at once), height and width in [1, 32767].  Arguments out of range return -2
 * before anything is launched.
 *
 * mq_aruco_threshold (replaces the adaptive threshold inside :283): gray uint8 (n_img, height, width) -> dark_out
 * uint8, 1 where gray * 529 < boxsum - 7 * 529 over the 23 x 23 window with replicated border.
 *
 * mq_aruco_label (the contour stage inside :283): dark -> labels_out int32 (n_img, height, width): the smallest
 * linear index y * width + x of the pixel's 4-connected component of dark pixels, -1 where light.  A union-find with
 * atomicMin in three launches; no thread waits on another.  The answer is unique.
 *
 * mq_aruco_components (:283): per component area, bounding box and the extreme pixel in the eight directions x, x+y,
 * y, y-x, -x, -x-y, -y, x-y (the largest linear index among equal projections).  Candidates: area >= 100, both box
 * sides >= 12, the box clear of the image border.  count_out int32 (n_img): their number; cand_out int32 (n_img,
 * max_quads, 16): the first max_quads (in [1, 64]) in ascending label order: label, area, x0, y0, x1, y1, the eight
 * extremes as linear indices, two zeros; rows past the count are zero.
 *
 * mq_aruco_quads (:283), one wave per candidate: the corners are the extremes of the diagonal or of the axis
 * directions, whichever has the larger shoelace area (ties: diagonal); convex, sides >= 10 px, area / quad area in
 * [1/16, 5/4].  Per side 16 bilinear profiles across it find where the gray level rises through its mid-level; a
 * total-least-squares line per side; corners = intersections.  The square-to-quad homography samples 6 x 6 cells
 * (3 x 3 samples each); the 20 border cells must be dark but for border_errors (in [0, 20]); the inner 16 are the
 * code, row-major, white = 1.  dictionary: uint16 (n_codes in [1, 1024]) or null; the smallest Hamming distance over
 * the four turns of every code (ties: lowest id, lowest turn), accepted up to max_correction_bits (in [0, 16]).
 * ok_out / ids_out / rot_out int32 (n_img, max_quads); corners_out float64 (n_img, max_quads, 4, 2) in pixels of
 * gray, corner 0 the marker's top-left, clockwise (cv2's order), NaN where not ok.  A null dictionary accepts every
 * quad that passes the border test, with id -1 in the geometric order.
 *
 * mq_find_markers (:281-283, :354-356): frames uint8 BGR (height, width, 3), frame i at frames + i * frame_stride ->
 * mq_resize_bilinear to (det_width, det_height) (in [2, frame size]) -> mq_cmc_preprocess at scale 1 (gray) -> the
 * four stages -> count_out int32 (n_img), ids_out int32 (n_img, max_markers), corners_out float64 (n_img,
 * max_markers, 4, 2) in frame pixels p * ratio + (ratio - 1) / 2 with ratio = frame size / detection size per axis
 * (the reference's corner * rsize_ratio :289 without the half-pixel term), ordered by (id, label), NaN and -1 past
 * the count.  max_markers in [1, max_quads].  cand_count_out (null, or int32 (n_img)): the candidates before
 * max_quads cut them. */
int mq_aruco_threshold(mq_ctx* ctx, const uint8_t* gray, int n_img, int height, int width, uint8_t* dark_out,
                       void* stream);
int mq_aruco_label(mq_ctx* ctx, const uint8_t* dark, int n_img, int height, int width, int32_t* labels_out,
                   void* stream);
int mq_aruco_components(mq_ctx* ctx, const int32_t* labels, int n_img, int height, int width, int max_quads,
                        int32_t* count_out, int32_t* cand_out, void* stream);
int mq_aruco_quads(mq_ctx* ctx, const uint8_t* gray, int n_img, int height, int width, const int32_t* count,
                   const int32_t* cand, int max_quads, const uint16_t* dictionary, int n_codes,
                   int max_correction_bits, int border_errors, int32_t* ok_out, int32_t* ids_out, int32_t* rot_out,
                   double* corners_out, void* stream);
int mq_find_markers(mq_ctx* ctx, const uint8_t* frames, int64_t frame_stride, int n_img, int height, int width,
                    int det_width, int det_height, const uint16_t* dictionary, int n_codes, int max_correction_bits,
                    int border_errors, int max_quads, int max_markers, int32_t* count_out, int32_t* ids_out,
                    double* corners_out, int32_t* cand_count_out, void* stream);

/* ---- Motion-JPEG frames (csrc/jpeg.hip): a baseline JPEG encoder for the overlay frames, so that only the
 * compressed stream leaves the device.  tests/jpeg_ref.py is the numpy restatement, equal byte for byte: integer
 * arithmetic only, no atomics on global memory, the same bits on every call.
 *
 * The codec: 8-bit baseline sequential DCT, YCbCr 4:2:0 (JFIF colour; chroma (a + b + c + d + bias) >> 2 with
 * bias 1 / 2 in even / odd chroma columns, libjpeg's h2v2 rule), one interleaved scan, H and W padded to multiples of 16 by edge replication (SOF0 carries the true size), the matrix DCT
 * A = (T X + 1024) >> 11, B = A T^T with T = rint(8192 c_u / 2 cos((2x + 1) u pi / 16)), quantisation
 * q = sign(B) ((|B| + (Q << 14)) / (Q << 15)) with the Annex K tables under libjpeg's quality scaling, the four
 * Annex K Huffman tables, and a restart marker every restart_interval MCUs (the intervals are coded in parallel).
 * Header: SOI, APP0 (JFIF 1.01), DQT x 2, SOF0, DHT x 4, DRI, SOS: 629 bytes.
 *
 * mq_jpeg_max_bytes: the worst case of one frame's stream, header included (host only, no device call); 0 for
 * arguments outside the bounds below.  A block codes at most 20 + 63 * 26 = 1658 bits (DC: a code of at most 9
 * bits + 11 extra bits; 63 AC: a code of at most 16 bits + 10 extra bits each; a ZRL only replaces 16
 * coefficients by at most 11 bits).  An interval of RI MCUs is padded to a byte: at most ceil(RI * 6 * 1658 / 8)
 * bytes, twice that when every byte is stuffed, and one two-byte marker (RSTn, or EOI after the last) follows it:
 *   629 + ceil(n_mcu / RI) * (2 * ceil(RI * 6 * 1658 / 8) + 2),  n_mcu = ceil(H / 16) * ceil(W / 16). */
size_t mq_jpeg_max_bytes(int height, int width, int restart_interval);

/* Encode n frames: frames uint8 BGR (height, width, 3), frame i at frames + i * frame_stride (bytes, device);
 * frame i's complete JPEG is out[i * out_stride : + out_size[i]] (device; out_size int32 (n), device).  Nothing is
 * written past out_size[i] within a slot.  height, width in [1, 65535], quality in [1, 100], restart_interval in
 * [1, 32], n in [0, 65535]; out_stride < mq_jpeg_max_bytes (or a worst case beyond 2^31 - 1 bytes) returns -2.
 * Stream-ordered: no host round trip inside the call; the context's workspace grows on the first call of a size. */
int mq_jpeg_encode(mq_ctx* ctx, const uint8_t* frames, int64_t frame_stride, int n, int height, int width,
                   int quality, int restart_interval, uint8_t* out, int64_t out_stride, int32_t* out_size,
                   void* stream);

/* ---- Motion-JPEG decoding (csrc/jpeg_parse.cpp, csrc/jpeg_dec_dev.hpp, csrc/jpeg_dec.hip): the other half of the
 * codec, so that a frame store holds compressed frames and only those cross the disk and the bus.
 * tests/jpeg_dec_ref.py is the numpy restatement, equal byte for byte, and on every stream Pillow (libjpeg-turbo)
 * accepts both equal Image.open(...).convert('RGB') on every pixel.  Integer arithmetic only, no data-dependent
 * order: the same bits on every call.
 *
 * Accepted: SOF0, 8-bit samples; one interleaved scan over all components with Ss = 0, Se = 63, Ah = Al = 0;
 * 1 component (written B = G = R) or 3 components YCbCr with chroma sampled 1x1 and luma 1x1, 2x1 or 2x2; DQT with
 * Pq = 0, ids 0-3; DHT ids 0-1 per class (a DC symbol is at most 15); any DRI (0: no restart markers); APPn, COM
 * and unknown segments with a length are skipped; a stream without any DHT uses the four Annex K tables; height and
 * width in [1, 65535].  The first FF D9 after SOS ends the scan.
 *
 * mq_jpeg_parse (host only, no device call) fills *info and returns 0, or one of: */
#define MQ_JPEG_E_NOT_JPEG (-20)   /* null / empty / no SOI, or a byte that is no marker where one must stand */
#define MQ_JPEG_E_TRUNCATED (-21)  /* the header ends inside a segment, or a segment's length contradicts its content */
#define MQ_JPEG_E_SOF (-22)        /* SOF1..SOF15 (extended, progressive, lossless, arithmetic), two SOF0, SOS before SOF0 */
#define MQ_JPEG_E_PRECISION (-23)  /* samples of another precision than 8 bits */
#define MQ_JPEG_E_DQT (-24)        /* Pq = 1 (16-bit table) or a table id above 3 */
#define MQ_JPEG_E_COMPONENTS (-25) /* neither 1 nor 3 components, or an Adobe segment whose transform is not YCbCr */
#define MQ_JPEG_E_SAMPLING (-26)   /* sampling factors other than 4:4:4, 4:2:2 (2x1) and 4:2:0 (2x2) */
#define MQ_JPEG_E_SCANS (-27)      /* a scan over a subset of the components, Ss / Se / Ah / Al of another mode, or a
                                      segment between the scan and EOI (several scans) */
#define MQ_JPEG_E_TABLE (-28)      /* a component names a quantisation or Huffman table the stream never defined */
#define MQ_JPEG_E_HUFFMAN (-29)    /* a DHT that is no prefix code (more than 256 symbols, or the canonical code
                                      overflows its length), class / id above 1, a DC symbol above 15 */
#define MQ_JPEG_E_NO_EOI (-30)     /* no FF D9 after the scan */
#define MQ_JPEG_E_SIZE (-31)       /* height or width 0 */

typedef struct mq_jpeg_huff {
  uint8_t bits[16];   /* codes of length 1..16 */
  uint8_t vals[256];  /* symbols in code order, zero past the last */
} mq_jpeg_huff;

/* Everything of a header the kernels need: 1320 bytes, passed to them by value (nothing is uploaded). */
typedef struct mq_jpeg_info {
  int32_t height, width, n_comp;      /* n_comp 1 or 3 */
  int32_t h_luma, v_luma;             /* 1x1, 2x1 or 2x2 (1x1 for one component) */
  int32_t restart_interval;           /* MCUs; 0: the scan is one interval */
  int64_t scan_offset;                /* the first entropy-coded byte */
  uint8_t quant[3][64];               /* per component, natural order */
  uint8_t dc_sel[3], ac_sel[3];       /* per component: which of dc[] / ac[] */
  uint8_t reserved[2];
  mq_jpeg_huff dc[2], ac[2];
} mq_jpeg_info;

int mq_jpeg_parse(const uint8_t* bytes, int64_t size, mq_jpeg_info* info);

/* Decode n streams that share one header (info; their first info->scan_offset bytes are taken as read): stream i is
 * streams[i * stream_stride : + sizes[i]] -- mq_jpeg_encode's out / out_size layout, so encode -> decode chains on
 * the device -- and its frame, uint8 BGR (height, width, 3), is written at frames + i * frame_stride.  Every
 * pointer except info is a device pointer.  frame_stride < height * width * 3 returns -2, as do n outside
 * [0, 65535], an info that mq_jpeg_parse could not have filled, and a workspace beyond 2^40 bytes.  Stream-ordered:
 * no host round trip inside the call; the context's workspace grows on the first call of a size.
 *
 * Entropy decoding: bits MSB first; FF 00 unstuffs to FF (an FF before any other byte stays data); FF D0..D7 and
 * FF D9 end a restart interval wherever they stand; interval i must end in D0 + (i mod 8) and the last of
 * ceil(n_mcu / RI) (1 for RI 0) in D9; DC predictors start at 0 in every interval and are kept as int16 (wrapping);
 * EXTEND is Annex F's (v < 2^(n-1) ? v - 2^n + 1 : v); AC symbol 0xF0 is ZRL, every other symbol of size 0 is EOB.
 * One lane decodes one interval.  Dequantisation: coef[natural] = q[zigzag k] * Q[natural].
 * IDCT: libjpeg's jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2; FIX constants 2446 3196 4433 6270 7373 9633 12299
 * 15137 16069 16819 20995 25172), a column pass ((x + 1024) >> 11) and a row pass ((x + 131072) >> 18), + 128,
 * clamp to [0, 255].  The 32-bit arithmetic is unsigned and WRAPS (the shifts are arithmetic on the wrapped
 * value): defined for the huge coefficients a malformed stream can produce, and never reached by a valid one.
 * Chroma upsampling: libjpeg's "fancy" rules on the true chroma extent ceil(H / v) x ceil(W / h), edges repeating
 * the last true row / column.  h2v2: s = 3 cur + other (the row above for even output rows, below for odd ones),
 * even column (3 s + s_left + 8) >> 4, odd column (3 s + s_right + 7) >> 4.  h2v1: even (3 c + c_left + 1) >> 2, odd
 * (3 c + c_right + 2) >> 2.  A chroma plane at most 2 samples wide is replicated instead, in both modes.
 * Colour, cb and cr less 128: R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
 * B = Y + ((116130 cb + 32768) >> 16), clamped.
 *
 * status[i] (int32, device): 0 ok; 1 restart markers wrong in count or sequence, or no EOI (nothing of the frame
 * is decoded); 2 bits that match no Huffman code; 3 a run past coefficient 63; 4 an interval's bits exhausted
 * before its MCUs (also: no code matches and fewer than 16 bits are left).  An interval stops at its first fault;
 * the status is the largest code among the frame's intervals.  Every scan-byte read is bounded by the interval's
 * end and every coefficient index by 63.  A frame with a nonzero status leaves unspecified values inside its own
 * height * width * 3 bytes, writes nothing outside them, and does not affect the other frames of the call. */
int mq_jpeg_decode(mq_ctx* ctx, const uint8_t* streams, int64_t stream_stride, const int32_t* sizes, int n,
                   const mq_jpeg_info* info, uint8_t* frames, int64_t frame_stride, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MQ_HIP_H */
