/* mss_hip.h -- C ABI of libmss_hip.so, the MI355X (gfx950) kernels behind the dense-segmentation +
 * OOD-scoring hot path of gaozhitong/MultiShiftSeg.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); every call is asynchronous
 *     on that stream and performs no host synchronisation, allocation or free;
 *   - return value: 0 = launched, MSS_ERR_* (>= 1001) = rejected precondition, other = hipError_t.
 *     The reference only printf()s launch failures (ops/src/cuda/ms_deform_im2col_cuda.cuh:953-957);
 *     callers of this ABI must raise on non-zero.
 *   - activations inside the DeepLab path are NHWC fp32 with an explicit pixel stride (`ld*`,
 *     in floats) so that kernels read/write channel slices of concat buffers in place.
 *   - a process may drive several devices; what a launcher needs to know about a device (occupancy, CU count, a raised
 *     dynamic-LDS limit) is kept per device for indices 0..15. Every launcher that asks answers MSS_ERR_UNSUPPORTED when the
 *     current device has another index.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference root).
 */
#ifndef MSS_HIP_H
#define MSS_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSS_ABI_VERSION 26     /* 2: round-2 struct / workspace changes; 3: mss_msda_backward_binned_f32; 4: mss_add_layernorm_bwd_sum_f32, mss_stem_conv_pool_f32,
                                  mss_wino_input_transform_bnbwd_f32, mss_wino_input_transform_upcat_f32,
                                  mss_bn_fold_train_from_partials_f32; 5 (round 4): mss_adam_step_f32 takes double hyper-parameters, mss_env_reset,
                                  mss_wino_input_transform_aspp3_f32, mss_msda_prepare_backward_ld_f32, mss_rcl_pairs_device2_f32, mss_rcl_loss_device_f32, mss_m2f_fused_score_ws_f32, mss_oodm_compact_packed_f32,
                                  6 (late round 4, additive): mss_msda_forward_fused_ld_f32, mss_msda_prepare_ld_f32, mss_add_layernorm_q_f32, mss_add_layernorm_bwd_sum2_f32, mss_msda_forward_fused_save_f32, mss_msda_backward_binned_proj_f32, mss_gap_from_partials_f32;
                                  7 (round 5): MssConvArgs.w_split + mss_gemm_split_weights_bf16x3 (the split-bf16 GEMM route);
                                  8 (round 6): mss_msda_forward_window_f32 removed (the measured-slower LDS-window forward left the product); additive: the mss_oodm_*lanes* entry points,
                                  mss_gemm_split_last_mfma;
                                  9: mss_oodm_compact_f32, mss_oodm_compact_packed_f32, mss_add_layernorm_bwd_sum_f32 and mss_m2f_fused_score_f32 removed (uncalled);
                                  10 (additive): MssConvArgs.k_steps / w_img_stride appended, mss_chan_compact_index, mss_chan_compact_act_f32,
                                  mss_chan_compact_weights_f32 (Dropout2d-zeroed input channels skipped in the trunk's 1x1 products);
                                  11 (additive): mss_m2f_attn_mask_bits_f32, mss_m2f_masked_attention_f32, mss_m2f_attn_workspace_bytes
                                  (the masked cross-attention of the Mask2Former GMA transformer decoder);
                                  12: two entry points removed, one signature changed: mss_rcl_select_f32 is the 5-launch selection (scratch, scratch_zeroed) and
                                  its 9-launch form and second name are gone; the two-launch Feistel pairs entry point that mss_rcl_pairs_device2_f32 replaced
                                  in version 5 is gone;
                                  13 (additive): mss_m2f_match_workspace_bytes, mss_m2f_match_cost_f32, mss_m2f_match_assign_f32 (Hungarian matching);
                                  14 (additive): the six mss_m2f_loss_* entry points (SetCriterion: class and sampled-mask losses);
                                  15 (additive): the five mss_m2f_mix_* entry points (SetCriterion.loss_ood: the class mix, forward and backward);
                                  16 (additive): mss_m2f_masked_attention_lse_f32, mss_m2f_attn_bwd_workspace_bytes, mss_m2f_masked_attention_bwd_f32
                                  (the masked attention's training forward and backward);
                                  17 (additive): mss_adamw_clip_step_f32 and its five host-only queries mss_adamw_chunk_elems, mss_adamw_tensors_per_launch,
                                  mss_adamw_blocks_per_launch, mss_adamw_scratch_floats, mss_adamw_plan (multi-tensor AdamW with full-model gradient clipping);
                                  18: MssM2fMaps / MssM2fTargets / MssM2fSteps / MssM2fGrads replace the loose mask-map, target-pack and per-step pointer-table
                                  arguments of mss_m2f_match_cost_f32 and the mss_m2f_loss_* entry points (signatures changed, none added or removed);
                                  19: mss_wino_input_transform_aspp3_src2_f32 added (the ASPP transform on the two un-multiplied factors of the trunk output);
                                  mss_env_generation removed from the ABI (nothing outside the library called it; it is a hidden helper now);
                                  20: mss_wino_input_transform_aspp3_dropped_f32 added and MssConvArgs.k_base / k_imgs inserted in front of k_steps (the
                                  composed ASPP products without the Dropout2d-zeroed channels); mss_chan_compact_index also writes `col`,
                                  mss_conv2d_pack_weights_f32 / mss_conv2d_unpack_wgrad_f32 take the per-image column gather (signatures changed);
                                  mss_msda_prepare_backward_f32 removed: it was mss_msda_prepare_backward_ld_f32 with dense strides, which its callers now pass;
                                  21: no entry point or struct changes; mss_conv2d_wgrad_f32's per-image form (MssConvArgs.k_steps) takes an OPTIONAL scratch of
                                  MSS_WGRAD_PERIMG_TAIL_BYTES (the packed job plan's row-split last round);
                                  22: mss_m2f_targets_from_labels added (the Mask2Former target pack built from the label maps on the device); mss_peak_clock
                                  removed to make room (only a diagnostic tool called it);
                                  23 (additive): mss_wino_aspp3_supported, the host query of what the three single-read ASPP transforms refuse;
                                  24: no entry point or struct changes; mss_conv2d_forward_f32 takes the 7x7 / stride-2 / 4 -> 64 stem of the ResNet-50
                                  backbone (csrc/stem7.hip), which it answered MSS_ERR_UNSUPPORTED before; mss_conv2d_forward_route labels it 5;
                                  25: no entry point or struct changes; mss_conv2d_forward_f32 takes MssConvArgs.stride == -2, the data gradient of a
                                  stride-2 convolution (csrc/conv_dgrad_s2.hip; no caller passed a negative stride before);
                                  mss_conv2d_forward_route labels it 6;
                                  26 (additive): mss_conv2d_wgrad_plan, MssWgradPlan and the MSS_WG_* kernel names (what a weight-gradient call
                                  launches: kernel, splits, reducer), host-only;
                                  still 26 (no entry point or struct changes, and two tests pin the number): mss_conv2d_wgrad_f32 takes the 7x7 /
                                  stride-2 / 4 -> 64 stem of the ResNet-50 backbone (csrc/stem7_wgrad.hip), plain or with the max-pool and ReLU
                                  backward fused, which it answered MSS_ERR_UNSUPPORTED before; mss_conv2d_wgrad_plan names it MSS_WG_STEM7. A caller
                                  that needs to know asks the plan query for the stem form: MSS_OK with kernel 11;
                                  still 26 (the same two tests pin the number as well as the count of 142 entry points): mss_seg_hist added (the
                                  confusion matrix of the closed-set segmentation metrics, csrc/metric.hip); mss_peak_scatter_f32 removed to make
                                  room (only a layout experiment of a diagnostic tool called it). A library from before the swap lacks the new
                                  symbol and is refused at load by name, not by number */
int mss_abi_version(void);

/* The MSS_* environment switches (A/B experiments, test routes; none is needed in production) are read once per call site and
 * cached. A process that changes one after its first call into the library calls this to have them re-read. */
int mss_env_reset(void);        /* returns the new generation */

/* ---------------------------------------------------------------------------------------------
 * B1 -- MultiScaleDeformableAttention extension
 * replaces ms_deform_attn_forward / ms_deform_attn_backward
 *   lib/network/mask2former/modeling/pixel_decoder/ops/src/vision.cpp:18-21
 *   .../ops/src/ms_deform_attn.h:25-66, .../ops/src/cuda/ms_deform_attn_cuda.cu:25-157
 *   kernels: .../ops/src/cuda/ms_deform_im2col_cuda.cuh:242-304 (fwd), :306-925 (bwd variants)
 * value [N,S,M,D]; spatial_shapes int64 [L,2]=(H_l,W_l); level_start_index int64 [L];
 * sampling_loc [N,Lq,M,L,P,2] (x,y) in [0,1]; attn_weight [N,Lq,M,L,P]; out [N,Lq,M*D].
 * forward: `out` may be uninitialised. backward: the callee zero-fills grad_value, grad_loc,
 * grad_attn itself (the reference allocates them with at::zeros, ms_deform_attn_cuda.cu:126-128).
 * There is no im2col_step argument: the whole batch is one launch (the reference's chunk loop,
 * ms_deform_attn_cuda.cu:66-80, only bounds a temporary it needs and we do not). */
int mss_msda_forward_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                         const float* sampling_loc, const float* attn_weight, int N, int S, int M, int D, int L,
                         int Lq, int P, float* out, void* stream);
int mss_msda_forward_f64(const double* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                         const double* sampling_loc, const double* attn_weight, int N, int S, int M, int D, int L,
                         int Lq, int P, double* out, void* stream);
int mss_msda_backward_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                          const float* sampling_loc, const float* attn_weight, const float* grad_out, int N,
                          int S, int M, int D, int L, int Lq, int P, float* grad_value, float* grad_loc,
                          float* grad_attn, void* stream);
/* The same ms_deform_attn_backward (vision.cpp:18-21 -> ms_deform_attn_cuda.cu:88-157, kernel family
 * ms_deform_im2col_cuda.cuh:306-925) with grad_value on the BINNED owner-computes path (round 3): every sample is filed
 * once under the tile of its level that holds its top-left corner (counting sort on the device), a workgroup per tile sums
 * its records in 64-bit fixed-point LDS words and stores the tile -- no floating-point atomic, no re-scan, bit-reproducible.
 * `host_shapes`: HOST copy of spatial_shapes (tile geometry and launch grids depend on it); `workspace`: 256-byte aligned
 * device scratch of >= mss_msda_backward_workspace_bytes(...) bytes. fp32, D == 32, L <= 8, 16-byte aligned value / grad_out;
 * otherwise MSS_ERR_UNSUPPORTED (workspace_bytes query: 0) and the caller uses mss_msda_backward_f32. */
long long mss_msda_backward_workspace_bytes(const int64_t* host_shapes, int N, int M, int D, int L, int Lq, int P);
int mss_msda_backward_binned_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                 const int64_t* host_shapes, const float* sampling_loc, const float* attn_weight,
                                 const float* grad_out, int N, int S, int M, int D, int L, int Lq, int P, float* grad_value,
                                 float* grad_loc, float* grad_attn, void* workspace, long long workspace_bytes, void* stream);
int mss_msda_backward_f64(const double* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                          const double* sampling_loc, const double* attn_weight, const double* grad_out, int N,
                          int S, int M, int D, int L, int Lq, int P, double* grad_value, double* grad_loc,
                          double* grad_attn, void* stream);

/* forward straight from the module's raw projections -- offsets [N,Lq,M,L,P,2] (sampling_offsets Linear),
 * logits [N,Lq,M,L*P] (attention_weights Linear), reference_points [N,Lq,L,2] -- with the softmax and the location
 * arithmetic of ops/modules/ms_deform_attn.py:100-109 inside the sampling kernel: sampling_loc / attn_weight are never
 * materialised. fp32, D in {16, 32, 64}; MSS_ERR_UNSUPPORTED otherwise (run mss_msda_prepare_f32 + mss_msda_forward_f32).
 * Equal to that two-kernel route up to the summation order of the L*P exponentials; L*P <= 20. */
int mss_msda_forward_fused_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                               const float* offsets, const float* logits, const float* reference_points, int N, int S,
                               int M, int D, int L, int Lq, int P, float* out, void* stream);

/* Operand preparation of the MSDeformAttn module in one pass (ops/modules/ms_deform_attn.py:100-109, the
 * reference_points[..., 2] branch): attn = softmax over the L*P logits of each (query, head), sampling_loc =
 * reference_points[n,q,l] + offsets / (W_l, H_l). offsets [N,Lq,M,L,P,2], logits [N,Lq,M,L*P], reference_points
 * [N,Lq,L,2]; L*P <= 20 (MSS_ERR_UNSUPPORTED above). The backward returns the gradients w.r.t. offsets and logits. */
int mss_msda_prepare_f32(const float* offsets, const float* logits, const float* reference_points,
                         const int64_t* spatial_shapes, int N, int Lq, int M, int L, int P, float* sampling_loc,
                         float* attn_weight, void* stream);
/* Row strides: grad_offsets row (n, q) at + (n*Lq + q) * ld_offsets (>= M*2*L*P floats, equal: dense), grad_logits likewise with
 * ld_logits (>= M*L*P). Both gradients in ONE [N*Lq, M*3*L*P] buffer (offsets | logits) make the weight gradient and the data
 * gradient of `sampling_offsets` and `attention_weights` -- two Linears on the same query (ops/modules/ms_deform_attn.py:98-100)
 * -- one GEMM each. */
int mss_msda_prepare_backward_ld_f32(const float* attn_weight, const float* grad_attn, const float* grad_loc,
                                     const int64_t* spatial_shapes, int N, int Lq, int M, int L, int P, float* grad_offsets,
                                     long long ld_offsets, float* grad_logits, long long ld_logits, void* stream);
/* mss_msda_backward_binned_f32 with that module backward folded into its gather pass: d(offsets) / d(logits) leave instead of
 * grad_sampling_loc / grad_attn_weight (never materialised; no prepare-backward launch). Bit-identical to the two-call sequence. */
int mss_msda_backward_binned_proj_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                      const int64_t* host_shapes, const float* sampling_loc, const float* attn_weight,
                                      const float* grad_out, int N, int S, int M, int D, int L, int Lq, int P, float* grad_value,
                                      float* grad_offsets, long long ld_offsets, float* grad_logits, long long ld_logits,
                                      void* workspace, long long workspace_bytes, void* stream);
/* Forward side of the same idea (ops/modules/ms_deform_attn.py:98-101: `sampling_offsets(query)` and `attention_weights(query)`):
 * offsets row (n, q) at + (n*Lq + q) * ld_offsets, logits likewise with ld_logits (0 = dense), so that both may be column ranges of
 * the [N*Lq, M*3*L*P] output of ONE product query [Woff ; Watt]^T. Outputs of the prepare form stay dense. */
int mss_msda_forward_fused_ld_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                  const float* offsets, long long ld_offsets, const float* logits, long long ld_logits,
                                  const float* reference_points, int N, int S, int M, int D, int L, int Lq, int P, float* out,
                                  void* stream);
/* ... and with the sampling locations / attention weights the kernel formed written out (both or neither), for a backward that
 * reads what the forward used (mss_msda_backward_*_f32 take exactly these two tensors) instead of re-deriving them. */
int mss_msda_forward_fused_save_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                    const float* offsets, long long ld_offsets, const float* logits, long long ld_logits,
                                    const float* reference_points, int N, int S, int M, int D, int L, int Lq, int P, float* out,
                                    float* sampling_loc_out, float* attn_weight_out, void* stream);
int mss_msda_prepare_ld_f32(const float* offsets, long long ld_offsets, const float* logits, long long ld_logits,
                            const float* reference_points, const int64_t* spatial_shapes, int N, int Lq, int M, int L, int P,
                            float* sampling_loc, float* attn_weight, void* stream);

/* ---------------------------------------------------------------------------------------------
 * B2 -- DeepWV3Plus operator set (replaces the cuDNN/ATen ops under
 *        lib/network/deepv3/deepv3.py:258-285 and lib/network/deepv3/wider_resnet.py:169-182)      */

/* One bias-free 2-D convolution as an implicit GEMM on fp32 MFMA.
 * replaces nn.Conv2d forward at deepv3.py:62-72,79-81,235-250 and wider_resnet.py:104-137,303-305
 * Shapes: C % 16 == 0, ldx % 4 == 0, 1 <= R * S <= 9 -- and ONE more, the stem of the Mask2Former ResNet-50 backbone
 * (detectron2 BasicStem.conv1; csrc/stem7.hip, v_mfma_f32_16x16x4_f32, one filter tap per instruction):
 *   R == S == 7, stride == 2, pad == 3, dil == 1; C == 4 and ldx == 4 (the image as mss_nchw_to_nhwc_pad_f32 writes it with Cp = 4:
 *   three colour channels and one ZERO channel, which is the caller's contract); K == 64, Kpad >= 64, w [49][Kpad][4] from
 *   mss_conv2d_pack_weights_f32(K = 64, C = 3, R = S = 7, Cp = 4); batch <= 1; no prologue affine, res, stats, w_split or k_steps;
 *   OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1, ldy >= 64, ldy % 4 == 0, x and y 16-byte aligned. out_scale / out_shift and out_relu
 *   are honoured; columns of y from 64 on are not written. Every other combination with C % 16 != 0 or R * S > 9 is
 *   MSS_ERR_UNSUPPORTED as before.
 * stride == -2: the DATA GRADIENT of a stride-2 convolution (csrc/conv_dgrad_s2.hip; the backward of res3.0 / res4.0 / res5.0 of the
 * ResNet-50 backbone), gather form, no atomics, bit-reproducible:
 *   x = dz [N, H, W, C]: the strided convolution's output grid and its output channels; C % 16 == 0, ldx % 4 == 0.
 *   w = the data-gradient filter from mss_conv2d_pack_weights_f32(flip = 1), [R*S][Kpad][C].
 *   y = dx [N, OH, OW, K]: the strided convolution's input. OH and OW are the CALLER's, because the forward's floor loses one row or
 *       column: MSS_ERR_BAD_ARG unless H == (OH + 2 * pad - R) / 2 + 1 and W == (OW + 2 * pad - S) / 2 + 1.
 *   Shapes: R == S == 3 with pad == 1, R == S == 1 with pad == 0; dil == 1.
 *   Honoured: in_scale / in_shift with in_ss_stride == 0 and in_relu, applied to in-grid operand rows only; res / ldres, added or
 *       gating (res_mask); out_scale / out_shift; out_relu.
 *   MSS_ERR_UNSUPPORTED: stats, batch > 1, k_steps, a per-sample prologue (in_ss_stride != 0), any other R, S, pad or dil.
 *   w_split is ignored: the product runs on the native fp32 MFMA whatever the route.
 *   The output pixels are enumerated per parity class (oy & 1, ox & 1), so a tile's live filter taps are block-uniform and exactly the
 *   non-zero ones (3x3: 1 + 2 + 2 + 4 = 9 taps over the four classes; 1x1: one tap in class (0, 0)). A class without a live tap still
 *   writes epilogue(0) -- res, the gate, or zero: EVERY element of y in columns [0, K) is written on every call. */
typedef struct MssConvArgs {
  const float* x;          /* input  NHWC [N,H,W,>=C], pixel stride ldx                         */
  const float* w;          /* packed weights [R*S][Kpad][C] from mss_conv2d_pack_weights_f32     */
  float* y;                /* output NHWC [N,OH,OW,>=K], pixel stride ldy                        */
  const float* in_scale;   /* optional prologue  a = x*in_scale[c] + in_shift[c] (BatchNorm of   */
  const float* in_shift;   /*   the producer, folded); sample n uses row n*in_ss_stride          */
  const float* out_scale;  /* optional epilogue  y = acc*out_scale[k] + out_shift[k]             */
  const float* out_shift;
  const float* res;        /* optional residual  y += res[m*ldres + k]  (wider_resnet.py:181)    */
  int N, H, W, C, ldx;
  int OH, OW, K, Kpad, ldy;
  int R, S, stride, dil, pad;
  int in_ss_stride;        /* 0: one affine for all samples; C: one per sample (Dropout2d fold)  */
  int in_relu, out_relu;   /* ReLU after the prologue affine / at the very end of the epilogue   */
  int ldres;
  int M, mtiles, ntiles;   /* filled in by the launcher                                          */
  int batch;               /* > 1: that many independent GEMMs in one launch (1x1 only, no res);  */
  long long x_bs, w_bs, y_bs; /* element strides between their x / w / y (Winograd positions)    */
  float* stats;            /* optional: per-channel partial sums of the OUTPUT for the next layer's train-mode    */
                           /*   BatchNorm, [ceil(M/64)][2][K] floats (row group g: sum, sum of squares of rows      */
                           /*   64g..64g+63); reduce with mss_bn_stats_partials_f32. Not with batch > 1.            */
  int res_mask;            /* 1: `res` gates instead of adds -- y = res[m*ldres + k] > 0 ? y : 0 -- the ReLU backward of a  */
                           /*   producer whose stored OUTPUT is `res` (FFN of msdeformattn.py:122-131) fused in the dgrad   */
  const void* w_split;     /* optional: the SAME weights as `w`, split into three bf16 planes by mss_gemm_split_weights_bf16x3.     */
                           /*   Non-NULL selects the split-bf16 route (6 bf16 MFMAs with fp32 accumulation per product block,       */
                           /*   fp32 accuracy) for every shape the persistent GEMM kernel takes (1x1, > 64 output channels,         */
                           /*   >= 48 input channels); other shapes run the native fp32 kernels on `w` (which must always be set).   */
  int route;               /* 0: native fp32 MFMA. 1: mss_conv2d_wgrad_f32 evaluates the TN product the same split-bf16 way (both    */
                           /*   operands split in the loader) where K % 128 == 0 and C % 256 == 0; other shapes stay native.         */
  int k_base, k_imgs;      /* with k_steps (below). k_imgs > 0 (batch > 1, batch % k_imgs == 0): batch entry b holds the rows of      */
                           /*   image b % k_imgs alone (Winograd-domain entries ordered (position, image)) and runs k_base +           */
                           /*   k_steps[b % k_imgs] K-steps over its own weights (w_bs; w_img_stride 0); rows per entry need not be a  */
                           /*   multiple of 128. In mss_conv2d_wgrad_f32: entry b's dU' covers its first 16 * (k_base + k_steps)       */
                           /*   columns; c tiles behind them are not written. k_imgs == 0: the one-batch form described below.         */
  const int* k_steps;      /* optional (DEVICE, [N]): per-image reduction length of a 1x1 product over channel-compacted operands   */
  long long w_img_stride;  /*   (mss_chan_compact_*): image n runs k_steps[n] 16-deep K-steps (>= 3, 16 * k_steps[n] <= C) over the  */
                           /*   weights at w + n * w_img_stride floats. No prologue, no batch, OH * OW % 128 == 0, > 64 output       */
                           /*   channels, native route only; MSS_ERR_UNSUPPORTED otherwise (there is no other kernel for it).         */
} MssConvArgs;

int mss_conv2d_forward_f32(MssConvArgs* args, void* stream);
/* Per-sample channel compaction (csrc/chan_compact.hip) for a 1x1 product whose prologue is a Dropout2d-folded per-sample affine
 * (wider_resnet.py:161-162: Dropout2d between bn3 and conv3 of the two bottleneck blocks): the dropped channels of a sample are exact
 * zeros after the prologue, so sample n only multiplies its K_n kept channels. C % 16 == 0, 48 <= C (<= 2048 for the two row passes).
 *   index:   mask [N][C] (any value != 0: kept) -> idx [N][C] int32, of which the first K_n entries of row n are written: the kept
 *            channel numbers in ascending order; count [N] = K_n; k_steps [N] = max(3, ceil(K_n / 16)) (MssConvArgs.k_steps);
 *            place [N][C] int32, written whole: place[n][p] = the channel whose values go to column p of sample n's compacted rows,
 *            or -1. The kept channels occupy the first 8 * ceil(K_n / 8) columns in the order in which the GEMM kernel's chain of
 *            fused multiply-adds visits them in the DENSE product (per 8-deep chunk: k = 0, 4, 1, 5, 2, 6, 3, 7), so that the
 *            compacted product adds the same terms in the same order: bit-identical to the dense one for finite weights.
 *            One launch, no atomics, deterministic.
 *   act:     x rows [N * rows_per_image][ldx] -> out (pitch ldout >= C, out != x): out[row][p] = relu(x[row][c] * scale[n][c] +
 *            shift[n][c]) with c = place[n][p], 0 where place[n][p] < 0, for p < 16 * k_steps[n]; later columns are not written.
 *            The arithmetic is the prologue's of the persistent GEMM kernel, so the operand values are the ones the dense product sees.
 *   weights: packed w [Kpad][C] -> out [N][Kpad][C]: out[n][k][p] = w[k][place[n][p]], same zero fill, later columns not written.
 *            col [N][C] int32 (optional, NULL: not wanted), written whole: the inverse of place -- the column channel c of sample n
 *            went to, -1 for a dropped channel.
 * idx entries from K_n on are never written or read. All float pointers 16-byte aligned. */
/* 1 when a 1x1 product with these (dense) arguments -- per-sample prologue affine + ReLU as the Dropout2d fold builds it -- qualifies
 * for the compacted form and MSS_DROPOUT_COMPACT (default 1) is not 0: stride 1, no padding, OH * OW % 128 == 0, 64 < K, Kpad % 128
 * == 0, 48 <= C <= 2048, ldx == C, no batch, no epilogue affine, native route (w_split NULL), operands within 32-bit byte offsets. */
int mss_chan_compact_wanted(const MssConvArgs* args);
int mss_chan_compact_index(const float* mask, int N, int C, int* idx, int* place, int* count, int* k_steps, int* col, void* stream);
int mss_chan_compact_act_f32(const float* x, int ldx, float* out, int ldout, int N, int rows_per_image, int C, const int* place,
                             const int* k_steps, const float* scale, const float* shift, void* stream);
int mss_chan_compact_weights_f32(const float* w, float* out, int N, int Kpad, int C, const int* place, const int* k_steps,
                                 void* stream);
int mss_conv2d_kpad(int K);
/* 1 if mss_conv2d_forward_f32 runs these arguments on the persistent GEMM kernel (csrc/gemm.hip: 1x1, stride 1,
 * more than 64 output channels, or 33..64 of them over >= 16 384 rows), 2 for the few-rows kernel (1x1 over <= 8 pixels, nothing fused), 3 for the
 * split-bf16 form of the persistent GEMM kernel (args->w_split set and the shape eligible), 4 for its implicit-GEMM form, 5 for the 7x7 stem kernel
 * (csrc/stem7.hip; the shape listed above MssConvArgs), 6 for the stride-2 data-gradient kernel (csrc/conv_dgrad_s2.hip; stride == -2),
 * 0 for the native implicit-GEMM kernel. It is the launch's own decision (csrc/fwd_route.h). For arguments mss_conv2d_forward_f32
 * refuses (MSS_ERR_BAD_ARG, MSS_ERR_UNSUPPORTED) it still answers a code 0..6 -- the kernel whose checks refuse them, or the one that
 * would be asked once the general checks (pointers set and aligned, C % 16, ...) hold: callers label a call before its output
 * pointer is set. Nothing is launched or dereferenced. */
int mss_conv2d_forward_route(const MssConvArgs* args);
/* The split-bf16 form of packed weights for MssConvArgs.w_split: w [batch][Kpad][C] fp32 (batch stride w_bs floats; what
 * mss_conv2d_pack_weights_f32 with R = S = 1 or mss_wino_pack_weights_f32 produce, Kpad % 128 == 0, C % 16 == 0) -> `planes`,
 * mss_gemm_split_weights_bytes(batch, Kpad, C) = batch * Kpad * C * 6 bytes: every value as three round-to-nearest bf16 terms
 * hi + mid + lo (exact), stored per 128-row block and 16-deep K-step in the order the kernel stages them. A fp32 product is then
 * a_hi b_hi + a_hi b_mid + a_mid b_hi + a_hi b_lo + a_lo b_hi + a_mid b_mid on the bf16 matrix cores with fp32 accumulation
 * (the three dropped terms are below 2^-26 |a b|): same contraction as nn.Conv2d / F.linear in fp32
 * (deepv3.py:47-92,258-285, wider_resnet.py:169-182), at fp32 accuracy. mss_conv2d_forward_route answers 3 when a call runs it. */
long long mss_gemm_split_weights_bytes(int batch, int Kpad, int C);
int mss_gemm_split_weights_bf16x3(const float* w, void* planes, int batch, int Kpad, int C, long long w_bs, void* stream);
/* The same for an implicit-GEMM layer (3x3 with stride 2 or few input channels, 1x1 with stride 2: what conv_igemm_kernel takes, with
 * > 64 output channels and one prologue affine): w [taps][Kpad][C] from mss_conv2d_pack_weights_f32 (taps = R*S <= 9) -> planes of
 * mss_gemm_split_weights_bytes(taps, Kpad, C) bytes with the taps folded into ONE reduction of taps*C; mss_conv2d_forward_route answers 4. */
int mss_conv_split_weights_bf16x3(const float* w, void* planes, int taps, int Kpad, int C, void* stream);
/* Which matrix instruction the LAST split-bf16 GEMM launched by the calling thread used: 16 = v_mfma_f32_16x16x32_bf16 on concatenated
 * planes with the weights brought in by LDS-DMA (products without a prologue whose output start, pitch and batch stride sit on the
 * 16-byte grid), 32 = v_mfma_f32_32x32x16_bf16 (everything else), 0 = none yet. Observability for tests and profiling labels only. */
int mss_gemm_split_last_mfma(void);
/* w [K][C][R][S] (nn.Conv2d.weight) -> packed [R*S][Kpad][Cp] (zero padded).
 * flip=1 packs the data-gradient filter instead (K<->C swapped, taps rotated 180 degrees);
 * then Kpad/Cp refer to the swapped roles. */
/* col != NULL (flip 0): w is n_img tensors [n][K][C][R][S] whose channels from c0 on are per-image compacted COLUMNS (col [n_img][C - c0]
 * from mss_chan_compact_index: the column of image n that holds channel c0 + j, -1 none); `packed` gets, in original channel order, the
 * sum over the images in ascending n, exact zero for a channel no image holds (the weight gradients of the dropped-channel ASPP products). */
int mss_conv2d_pack_weights_f32(const float* w, float* packed, int K, int C, int R, int S, int Kpad, int Cp,
                                int flip, const int* col, int n_img, int c0, void* stream);
/* weight gradient: dwp[tap][k][c] = sum_m dy[m][k]*act(x[m@tap][c]); dwp [taps][Kpad][Cp] is fully overwritten.
 * Kpad and Cp may pad K and C up to the end of the last output tile of the kernel that runs: at least to the next multiple of 32
 * rows for K <= 32, of 64 for K <= 64, else of 128, and to the next multiple of 128 columns (so none where K or C is such a
 * multiple already; rounding up to a multiple of 4 always fits). Padding beyond that tile no kernel would write:
 * MSS_ERR_UNSUPPORTED (mss_conv2d_wgrad_plan answers the same without launching).
 * Deterministic (no atomics; pixel-range partials are summed in a fixed order: the reference pins
 * cudnn.deterministic, lib/utils/utils.py:10-13). ws: scratch of mss_conv2d_wgrad_workspace_bytes(args, Cp) bytes
 * (NULL allowed when that is 0). Replaces the autograd wgrad of nn.Conv2d for aspp/bot_aspp/bot_fine/ood_head
 * (exps/DeepLab.yaml:10-11, train_deeplab.py:113-132).
 * Per-image form (args->k_steps): mss_conv2d_wgrad_workspace_bytes is 0 and ws = NULL works -- the live tiles are packed densely and
 * every job is a whole tile. With ws_bytes >= MSS_WGRAD_PERIMG_TAIL_BYTES the last, partial round of one-wave jobs is cut by rows
 * as well: partial tiles go to ws and a second launch adds them in ascending order (still no atomics, one fixed order). Either
 * way, tiles behind an image's extent stay unwritten and the columns behind it inside a tile are exact zeros.
 * Shapes: C % 4 == 0, ldx % 4 == 0, lddy % 4 == 0, Cp % 4 == 0, 1 <= R * S <= 9 -- and ONE more, recognised in front of those checks:
 * the stem of the Mask2Former ResNet-50 backbone (csrc/stem7_wgrad.hip, v_mfma_f32_16x16x4_f32 with four output pixels as the K step;
 * MSS_WG_STEM7), exactly this argument set:
 *   R == S == 7, stride == 2, pad == 3, dil == 1; C == 4 and ldx == 4; K == 64, Kpad == 64 and Cp == 4; batch <= 1; no in_scale,
 *   in_shift, in_relu or k_steps. Every other combination with R * S > 9 is MSS_ERR_UNSUPPORTED as before. `route` is ignored: the
 *   product runs on the native fp32 MFMA.
 *   x = the image [N, H, W, 4] as mss_nchw_to_nhwc_pad_f32 writes it with Cp = 4 (three colour channels and one ZERO channel: the
 *       caller's contract, as the forward's). OH, OW: the stem's output grid; MSS_ERR_BAD_ARG unless OH == (H - 1) / 2 + 1 and
 *       OW == (W - 1) / 2 + 1. x, dy and res 16-byte aligned and lddy >= 64, else MSS_ERR_BAD_ARG.
 *   Plain form, res == NULL: dy = dz [N, OH, OW, 64] with pitch lddy: dwp[tap][k][c] = sum_m dz[m][k] * x[m @ tap][c], zero outside
 *       the image.
 *   Pool form, res != NULL (ldres >= 64, ldres % 4 == 0 and res_mask == 1, else MSS_ERR_BAD_ARG): res = the stored stem output
 *       a0 [N, OH, OW, 64] after norm and ReLU; dy = the gradient at the POOLED map [N, PH, PW, 64], PH = (OH - 1) / 2 + 1,
 *       PW = (OW - 1) / 2 + 1 (max-pool 3x3, stride 2, padding 1). The kernel forms dz[n, oy, ox, k] = [a0 > 0] * the sum, in
 *       ascending (py, px), of dy[n, py, px, k] over the up to four windows whose arg-max is (oy, ox). The arg-max is recomputed from
 *       a0 (no index tensor): the FIRST maximum in row-major order among the window's in-image positions, a NaN takes the window
 *       (F.max_pool2d's rule). A window whose maximum is not positive contributes nothing.
 *   dwp [49][64][4] is fully overwritten; column c == 3 holds the product with the pad channel (zero under the image contract).
 *   Deterministic and bit-reproducible as every form: no atomics, the pixel-range slabs are added in ascending order. Scratch:
 *   mss_conv2d_wgrad_workspace_bytes; MSS_ERR_BAD_ARG with less. mss_conv2d_wgrad_plan: positions = 49, ktiles = ctiles = 1, one
 *   workgroup per split (total = splits), rows_per_split = 64 x the 4 x 16-pixel tiles of a split. mss_conv2d_wgrad_route answers 0. */
#define MSS_WGRAD_PERIMG_TAIL_BYTES (1024ll * 128 * 128 * 4)     /* 1024 wave slots x one 128 x 128 fp32 tile: tail tiles x splits <= slots */
long long mss_conv2d_wgrad_workspace_bytes(const MssConvArgs* args, int Cp);
int mss_conv2d_wgrad_f32(MssConvArgs* args, const float* dy, int lddy, float* dwp, int Cp, float* ws,
                         long long ws_bytes, void* stream);
/* place != NULL (accumulate 0): grad is n_img tensors [n][K][C][R][S]; image n's holds packed's channels [0, c0) as they are, channel
 * c0 + place[n][p] in column c0 + p for p < 16 * k_steps[n] (place -1: zero) and zeros behind: weights in the per-image compacted column
 * order of mss_chan_compact_index (place [n_img][C - c0]). */
int mss_conv2d_unpack_wgrad_f32(const float* packed, float* grad, int K, int C, int R, int S, int Kpad,
                                int Cp, int accumulate, const int* place, const int* k_steps, int n_img, int c0, void* stream);
/* 1 when mss_conv2d_wgrad_f32 runs these arguments on the split-bf16 TN kernel (args->route == 1, K % 128 == 0, C % 256 == 0, enough
 * tiles to fill half the chip), else 0 (native fp32 MFMA kernels). Profiling label only. */
int mss_conv2d_wgrad_route(const MssConvArgs* args, int lddy);
/* What a mss_conv2d_wgrad_f32 call with these arguments launches (csrc/wgrad_route.h): the launch's own decision, read
 * through the same helper, so the two cannot disagree. Pure host arithmetic: no HIP call, and no pointer is dereferenced -- args->x,
 * in_scale, in_shift, k_steps, dy and dwp are compared with NULL and their alignment is read, as the launch does. ws_bytes: the
 * scratch the launch would be given; it decides one thing only, whether the split-bf16 kernel is skipped because the scratch is too
 * small for it (a scratch too small for the kernel that then runs is the launch's MSS_ERR_BAD_ARG, not this query's: out->ws_bytes
 * says what is needed). part: 0 = the product as given; for a MSS_WG_TWO_PART product 1 and 2 = its two parts (the first wide_K
 * output channels, then the rest); MSS_ERR_BAD_ARG for part 1 or 2 of any other product and for any other value.
 * Returns what mss_conv2d_wgrad_f32 returns from its argument checks; *out is written only on MSS_OK (0). A call without output
 * pixels (N * OH * OW <= 0) launches nothing: MSS_OK with every field 0 except kernel = -1. */
#define MSS_WG_CONV_32 0            /* conv_wgrad_kernel<32, 128, 16>: K <= 32                                             */
#define MSS_WG_CONV_64 1            /* conv_wgrad_kernel<64, 128, 16>: K <= 64                                             */
#define MSS_WG_CONV_128 2           /* conv_wgrad_kernel<128, 128, 16>                                                     */
#define MSS_WG_NARROW 3             /* gemm_tn_narrow_kernel                                                               */
#define MSS_WG_TN_LDS 4             /* gemm_tn_wgrad_kernel                                                                */
#define MSS_WG_TN_WIDE 5            /* gemm_tn2_wgrad_kernel                                                               */
#define MSS_WG_TN_DIRECT 6          /* gemm_tn_direct_kernel, whole tiles or row splits of every tile                      */
#define MSS_WG_TN_DIRECT_TAIL 7     /* gemm_tn_direct_kernel with the tail plan + tn_tail_reduce_kernel                    */
#define MSS_WG_TN_DIRECT_PERIMG 8   /* gemm_tn_direct_kernel, per-image form (MssConvArgs.k_steps)                         */
#define MSS_WG_TN_BF16X3 9          /* the split-bf16 TN kernel (args->route == 1)                                         */
#define MSS_WG_TWO_PART 10          /* K = 128 j + r: two launches, see `part`                                             */
#define MSS_WG_STEM7 11             /* stem7_wgrad_kernel: the 7x7 stem form (above mss_conv2d_wgrad_f32)                  */
typedef struct MssWgradPlan {
  int kernel;                /* MSS_WG_*                                                                                      */
  int ktiles, ctiles;        /* output tiles along K and C                                                                    */
  int positions;             /* independent products of the launch: filter taps, or the batch                                 */
  int splits;                /* row ranges; > 1: partial slabs in the scratch, added in ascending order by a reduce launch    */
  int rows_per_split;
  long long total;           /* jobs (workgroups or waves) of the launch                                                      */
  long long full;            /* MSS_WG_TN_DIRECT_TAIL: whole-tile jobs in front of the split ones; else -1                    */
  long long ws_bytes;        /* scratch the launch needs                                                                      */
  int wide_K;                /* MSS_WG_TWO_PART: output channels of the first part; else 0                                    */
  int reduce_group;          /* threads that share an output element in the reduce launch: 1 = wgrad_reduce_kernel, 2..32 =   */
                             /*   wgrad_reduce_par_kernel<G>; 0 = no such launch (one split, or a kernel with its own reducer) */
} MssWgradPlan;
int mss_conv2d_wgrad_plan(const MssConvArgs* args, const float* dy, int lddy, const float* dwp, int Cp, long long ws_bytes, int part,
                          MssWgradPlan* out);

/* Winograd F(m x m, 3x3) path, m = `tile` = 2 or 4, P = (m+2)^2 positions, for stride-1 3x3 convolutions with
 * many channels (csrc/winograd.hip): weights [K][C][3][3] -> U [P][Kpad][Cp]; x -> X' [P][T][C]
 * (T = mss_wino_num_tiles, BatchNorm/ReLU prologue and zero padding fused); then ONE mss_conv2d_forward_f32
 * call in batched 1x1 mode (batch = P, x_bs = T*C, w_bs = Kpad*Cp, y_bs = T*K) gives Y' [P][T][K];
 * Y' -> NHWC y (+ residual). Dilation is exact (per-residue sub-grids). MFMA work is 9*m^2/P = 2.25x (m = 2)
 * or 4x (m = 4) below the direct form; fp32 rounding error ~1e-6 (m = 2) / ~1e-5 (m = 4) relative per layer.
 * Tile geometry and layout (m = 2, 4 or 6; n = m + 2; d = dil), restated in float64 by tests/ref_winograd.py:
 *   Hs = ceil(H / d), tH = ceil(Hs / m), the same for W; T = N * d * d * tH * tW.
 *   Tile index t = (((img * d + a) * d + b) * tH + ty) * tW + tx for image img, residue sub-grid (a, b), tile (ty, tx) of it.
 *   Element (i, j), 0 <= i, j < n, of the input tile is image pixel ((m * ty + i - 1) * d + a, (m * tx + j - 1) * d + b), zero
 *   outside the image (after the prologue); element (u, v), 0 <= u, v < m, of the output tile is pixel ((m * ty + u) * d + a,
 *   (m * tx + v) * d + b), not written (dY': read as zero) outside it.
 *   X' is [n * n][T][C] and Y' / dY' are [n * n][T][K], Winograd position (xi, nu) = (row, column) of B^T d B at index xi * n + nu;
 *   U / dU are [n * n][Kpad][Cp] with (G g G^T)[xi][nu] of filter (k, c) at [xi * n + nu][k][c], zero for k >= K or c >= C. */
long long mss_wino_num_tiles(int N, int H, int W, int dil, int tile);
int mss_wino_pack_weights_f32(const float* w, float* u, int K, int C, int Kpad, int Cp, int tile, void* stream);
/* The same U straight into the split-bf16 planes MssConvArgs.w_split takes ((tile + 2)^2 batch entries of [Kpad][C]; bit-identical to
 * mss_gemm_split_weights_bf16x3 of the function above with Cp == C) without writing and re-reading U in fp32. Kpad % 128 == 0,
 * C % 16 == 0, both pointers 16-byte aligned; planes: mss_gemm_split_weights_bytes((tile + 2)^2, Kpad, C) bytes. */
int mss_wino_pack_split_bf16x3(const float* w, void* planes, int K, int C, int Kpad, int tile, void* stream);
int mss_wino_input_transform_f32(const float* x, int ldx, int N, int H, int W, int C, int dil, int tile,
                                 const float* scale, const float* shift, int relu, float* xt, void* stream);
/* The same X', but of dx = the train-mode BatchNorm+ReLU backward of the gradient dy w.r.t. the layer input x2, computed on the fly
 * (the arithmetic of mss_bn_relu_bwd_apply_f32): the data-gradient convolution behind a BatchNorm backward never materialises dx.
 * scale / shift: the forward's folded affine; mean / invstd: its saved batch statistics; accum: [2C] doubles of
 * mss_bn_relu_bwd_reduce_f32 over the same (dy, x2). MSS_ERR_UNSUPPORTED where the LDS-staged transform is not taken. */
int mss_wino_input_transform_bnbwd_f32(const float* dy, int lddy, const float* x2, int ldx2, int N, int H, int W, int C, int dil,
                                       int tile, const float* scale, const float* shift, const float* mean, const float* invstd,
                                       const double* accum, int relu, float* xt, void* stream);
/* The same X' for the decoder's first 3x3 layer, whose input is a concat (deepv3.py:269-275): channels [0, c_split) from `a`, the
 * rest = the align_corners=True bilinear upsample of `small` [N][IH][IW][C - c_split] to H x W, interpolated inside the transform
 * (the full-resolution upsampled map is never stored). MSS_ERR_UNSUPPORTED where the LDS-staged transform is not taken. */
int mss_wino_input_transform_upcat_f32(const float* a, int lda, int c_split, const float* small, int ld_small, int IH, int IW, int N,
                                       int H, int W, int C, int tile, float* xt, void* stream);
/* ASPP (deepv3.py:84-92: three 3x3 branches of rates d, 2d, 3d on the SAME 4096-channel map): X' for all three dilations from
 * ONE read of x. xt_m = exactly what mss_wino_input_transform_f32(x, ..., dil = (m+1)*d, tile = tiles[m], no prologue) writes.
 * tiles: a HOST pointer (the one exception to this header's "every pointer is a device pointer" rule; read before the launch, so
 * the call may be captured into a hipGraph) to 3 tile edges, each 4 or 6. MSS_ERR_UNSUPPORTED when a base residue sub-grid does not fit in LDS or a
 * tile edge is 2 (the caller then runs the three transforms separately). */
int mss_wino_input_transform_aspp3_f32(const float* x, int ldx, int N, int H, int W, int C, int d, const int* tiles, float* xt0,
                                       float* xt1, float* xt2, void* stream);
/* The same transform on a map that is never stored: w = [relu(x0 * scale0 + shift0) ; relu(x1 * scale1 + shift1)], C0 + C1 channels
 * (the two prologue factors of the trunk's last block, whose 1x1 output convolutions are folded into the ASPP weights). ss0 / ss1:
 * per-sample stride of that source's (scale, shift) vectors, 0 = shared by all samples. xt_m = exactly what
 * mss_affine_relu_nhwc_f32 into one (C0 + C1)-channel buffer followed by mss_wino_input_transform_aspp3_f32 writes; padding stays zero.
 * sums (optional, with gap): scratch [N][d*d][C0 + C1], the column sums of w over each base residue sub-grid, in a fixed order;
 * gap [N][C0 + C1] = their sum / (H*W) (float64 accumulation, fixed order): AdaptiveAvgPool2d(1) of w. xt0 = xt1 = xt2 = NULL:
 * sums only, the same code path and the same bits. MSS_ERR_UNSUPPORTED as for mss_wino_input_transform_aspp3_f32. */
int mss_wino_input_transform_aspp3_src2_f32(const float* x0, int ldx0, int C0, const float* scale0, const float* shift0, int ss0,
                                            const float* x1, int ldx1, int C1, const float* scale1, const float* shift1, int ss1,
                                            int N, int H, int W, int d, const int* tiles, float* xt0, float* xt1, float* xt2,
                                            float* sums, float* gap, void* stream);
/* The same without the second factor's Dropout2d-zeroed channels. x1c: v = relu(x1 * scale1 + shift1) channel-compacted per image by
 * mss_chan_compact_act_f32 (pitch ldx1 >= C1; place [N][C1], k_steps [N] of mss_chan_compact_index). Of image n's rows of every X'
 * (pitch C0 + C1) only the first C0 + 16 * k_steps[n] columns are written: u's C0 channels (C0 % 16 == 0), then v's kept channels in
 * `place` order -- each column bit for bit the dense X' column of its channel, exact zeros where place is -1. sums [N][d*d][C0 + C1]
 * and gap [N][C0 + C1] (both or neither) come out in ORIGINAL channel order with the dense call's bits. All three X' are required.
 * The batched products then take batch entries (position, image): MssConvArgs.k_steps / k_base = C0 / 16 / k_imgs = N. */
int mss_wino_input_transform_aspp3_dropped_f32(const float* x0, int ldx0, int C0, const float* scale0, const float* shift0, int ss0,
                                               const float* x1c, int ldx1, int C1, const int* place, const int* k_steps,
                                               int N, int H, int W, int d, const int* tiles, float* xt0, float* xt1, float* xt2,
                                               float* sums, float* gap, void* stream);
/* Host query, no launch: 1 where the three single-read transforms above take the shape, 0 where they answer MSS_ERR_UNSUPPORTED -- a
 * tile edge that is not 4 or 6, a base residue sub-grid over 80 KiB of LDS, 2^31 workgroups, and for the two-source forms (two_source
 * != 0, C = C0 + C1) C or d * d beyond 2^24. tiles: a HOST pointer to 3 tile edges. A caller asks it before it allocates X', so that
 * a refusal at the launch is an error and not a fallback (multishiftseg_amd/aspp_plan.py). */
int mss_wino_aspp3_supported(int N, int H, int W, int C, int d, const int* tiles, int two_source);
int mss_wino_output_transform_f32(const float* yt, int N, int H, int W, int K, int dil, int tile, const float* res,
                                  int ldres, float* y, int ldy, float* stats, void* stream);
/* stats (optional): [mss_wino_output_stats_parts(...)][2][K] partial sums / sums of squares of y, as MssConvArgs.stats */
int mss_wino_output_stats_parts(int N, int H, int W, int K, int dil, int tile);

/* weight gradient in the Winograd domain: dY' = A dY A^T per tile, then ONE mss_conv2d_wgrad_f32 call in
 * batched mode (batch = P, R = S = 1, x = X', x_bs = T*C, dy = dY', y_bs = T*K) accumulates
 * dU [P][Kpad][Cp], and dg = G^T dU G gives the [K][C][3][3] gradient. */
int mss_wino_grad_output_transform_f32(const float* dy, int lddy, int N, int H, int W, int K, int dil, int tile,
                                       float* dyt, void* stream);
int mss_wino_weight_grad_transform_f32(const float* du, float* dw, int K, int C, int Kpad, int Cp, int tile,
                                       void* stream);

/* image NCHW [N,C,H,W] -> NHWC [N,H,W,Cp] with channels C..Cp-1 zero (feeds mod1.conv1). */
int mss_nchw_to_nhwc_pad_f32(const float* x, float* y, int N, int C, int H, int W, int Cp, void* stream);
/* stem (mod1.conv1, 3 -> 64 channels, 3x3, padding 1; wider_resnet.py:303) as a dense GEMM: img [N,3,H,W] NCHW ->
 * out [N,H,W,32] NHWC with channel j = c*9 + r*3 + s holding img[n][c][y+r-1][x+s-1] (zero padding), 27..31 zero: the
 * column order of weight.reshape(64, 27). The 1x1 convolution of that tensor with the reshaped weight IS conv1. */
int mss_im2col3x3_c3_f32(const float* img, float* out, int N, int H, int W, void* stream);
/* The stem in ONE kernel (csrc/stem.hip): y [N][OH][OW][64] NHWC (pixel stride ldy >= 64) = MaxPool2d(3, stride 2, padding 1) of
 * conv3x3(img [N][3][H][W] NCHW, w [64][3][3][3], padding 1, no bias) -- mod1.conv1 + pool2 of the trunk (wider_resnet.py:343-345,
 * 353-355; no BatchNorm between them). OH = (H-1)/2 + 1, OW = (W-1)/2 + 1. The full-resolution 64-channel map is never stored. */
int mss_stem_conv_pool_f32(const float* img, const float* w, float* y, int ldy, int N, int H, int W, void* stream);

/* BatchNorm2d pieces (mynn.py:8-12 Norm2d = nn.BatchNorm2d, eps 1e-5, momentum 0.1).
 * stats: per-channel batch mean and biased variance of an NHWC tensor (M pixels). `accum` is a scratch of
 * mss_col_reduce_accum_doubles(M, C) doubles (contents irrelevant on entry): its first 2*C entries receive the
 * sums (sum | sum of squares), the rest holds the first stage's per-workgroup partials, which a second kernel adds
 * in a fixed order -- no atomics, bit-reproducible (the reference pins cudnn.deterministic, lib/utils/utils.py:10-13). */
long long mss_col_reduce_accum_doubles(long long M, int C);
/* accum[0:2C] = column sums of a partial-sum matrix [nparts][2][C] written by a producer (MssConvArgs.stats,
 * mss_wino_output_transform_f32): the statistics pass then never re-reads the activation. accum as above with
 * M = nparts. */
int mss_bn_stats_partials_f32(const float* partials, long long nparts, int C, double* accum, void* stream);
int mss_bn_stats_nhwc_f32(const float* x, long long M, int C, int ldx, double* accum, void* stream);
/* finalise: from accum -> (mean, var) -> scale = gamma*rsqrt(var+eps), shift = beta-mean*scale;
 * if running_mean != NULL also running = (1-mom)*running + mom*{mean, var*M/(M-1)}.
 * save_mean / save_invstd (optional) are kept for the backward. */
int mss_bn_finalize_train_f32(const double* accum, long long M, int C, const float* gamma, const float* beta,
                              float eps, float momentum, float* running_mean, float* running_var, float* scale,
                              float* shift, float* save_mean, float* save_invstd, void* stream);
/* mss_bn_stats_partials_f32 + mss_bn_finalize_train_f32 in two launches instead of three (bit-identical results): the train-mode fold
 * of a BatchNorm whose producer left partial sums. M = rows covered by the partial sums. */
int mss_bn_fold_train_from_partials_f32(const float* partials, long long nparts, int C, double* accum, long long M,
                                        const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                                        float* running_var, float* scale, float* shift, float* save_mean, float* save_invstd,
                                        void* stream);
/* eval mode: scale/shift from the running statistics. */
int mss_bn_fold_eval_f32(const float* gamma, const float* beta, const float* running_mean,
                         const float* running_var, float eps, int C, float* scale, float* shift, void* stream);
/* y = relu?(x*scale[c]+shift[c]) on NHWC rows (used where a fused prologue is not possible). */
int mss_affine_relu_nhwc_f32(const float* x, int ldx, float* y, int ldy, long long M, int C, const float* scale,
                             const float* shift, int relu, void* stream);
/* backward of y = relu(bn_train(x)): given dy and x (pre-BN), scale/save_mean/save_invstd/gamma,
 * per-channel sums into accum[0:2C] (scratch of mss_col_reduce_accum_doubles(M, C) doubles, as above):
 * sum(dz), sum(dz*xhat) where dz = dy * (y>0). */
int mss_bn_relu_bwd_reduce_f32(const float* dy, int lddy, const float* x, int ldx, long long M, int C,
                               const float* scale, const float* shift, const float* save_mean,
                               const float* save_invstd, int relu, double* accum, void* stream);
/* dx = gamma*invstd*(dz - sum_dz/M - xhat*sum_dzxhat/M) (train) or dz*scale (eval, accum==NULL);
 * optional dgamma/dbeta outputs (added to, may be NULL). */
int mss_bn_relu_bwd_apply_f32(const float* dy, int lddy, const float* x, int ldx, float* dx, int lddx,
                              long long M, int C, const float* gamma, const float* scale, const float* shift,
                              const float* save_mean, const float* save_invstd, int relu, const double* accum,
                              float* dgamma, float* dbeta, void* stream);

/* MaxPool2d(3, stride 2, padding 1) on NHWC (wider_resnet.py:353-355). */
int mss_maxpool3s2_nhwc_f32(const float* x, int ldx, float* y, int ldy, int N, int H, int W, int C, int OH,
                            int OW, void* stream);
/* AdaptiveAvgPool2d(1) (deepv3.py:77,87): y[n][c] = mean over HW. ws: scratch of mss_colsum_workspace_floats(N, HW, C)
 * floats (pixel-range partials, added in a fixed order: no atomics). */
long long mss_colsum_workspace_floats(int N, int HW, int C);
int mss_gap_nhwc_f32(const float* x, int ldx, float* y, int N, int HW, int C, float* ws, void* stream);
/* the same from the per-64-row column sums a producing conv / GEMM left in MssConvArgs.stats ([ceil(N*HW/64)][2][C]; HW % 64 == 0,
 * MSS_ERR_UNSUPPORTED otherwise): the map itself is not read again (r04). float64 accumulation in a fixed order. */
int mss_gap_from_partials_f32(const float* partials, int N, int HW, int C, float* y, void* stream);
/* broadcast y[n][p][c] = relu?(v[n][c]*scale[c]+shift[c]) over HW pixels: the "Upsample" of the
 * 1x1 image-pooling map (deepv3.py:86). */
int mss_broadcast_rows_nhwc_f32(const float* v, float* y, int ldy, int N, int HW, int C, const float* scale,
                                const float* shift, int relu, void* stream);
/* backward of the broadcast: dv[n][c] = sum_p dy[n][p][c] */
int mss_colsum_nhwc_f32(const float* dy, int lddy, float* dv, int N, int HW, int C, float* ws, void* stream);

/* F.interpolate(mode='bilinear', align_corners=True) (mynn.py:28-33) on NHWC, forward and its
 * transpose (gather form, deterministic). Optional prologue affine+relu on the input. */
int mss_upsample_ac_nhwc_f32(const float* x, int ldx, float* y, int ldy, int N, int IH, int IW, int OH, int OW,
                             int C, void* stream);
int mss_upsample_ac_nhwc_bwd_f32(const float* dy, int lddy, float* dx, int lddx, int N, int IH, int IW, int OH,
                                 int OW, int C, void* stream);

/* The OOD-score tail (deepv3.py:251-253,279-283):
 *   score[n,oy,ox] = bilinear_ac( -logsumexp_c dec2[n,:,:,c] )    dec2 NHWC [N,IH,IW,C] (ld)
 *   logit[n,c,oy,ox] = bilinear_ac( dec1[n,:,:,c] )               written NCHW
 *   label[n,oy,ox]  = argmax_c logit (first max wins, as torch.argmax; a NaN is maximal and the first NaN wins), optional (uint8)
 * Any of score/logit/label may be NULL. The logsumexp is max-shifted, computed once per source pixel, classes summed in ascending
 * order; the blend is l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11).
 * Class count: 1 <= C <= 100 (class indices above 99 mean "OOD" to RelContrastiveLoss and label_threshold, and label is uint8);
 * anything else -> MSS_ERR_UNSUPPORTED, checked first. Then: score without dec2, or logit / label without dec1 ->
 * MSS_ERR_BAD_ARG; N * OH * OW == 0 -> MSS_OK, nothing launched. C == 19 runs kernels specialised for the Cityscapes classes,
 * every other count a class-generic route that walks the classes in chunks of 24 (registers and LDS do not grow with C; at most
 * 64 KB of LDS per workgroup). Both routes pick one of three launch regimes:
 *   vector    OW % 4 == 0, up-sampling, and both heads in ONE pixel-contiguous buffer: ld1 == ld2, ld % 4 == 0, dec1 and dec2 each
 *             at a multiple of 4 floats from the lower of the two, each with 4 * ceil(C/4) readable floats inside the row (the
 *             columns past C are read and ignored), every operand 16-byte aligned, N * C * OH * OW * 4 < 2^32;
 *   tiled     up-sampling with any alignment and any OW;
 *   per-pixel everything else (down-sampling, identity, large ratios).
 * MSS_OOD_TAIL_GENERIC=1 (default 0; read through the cached switches, see mss_env_reset) sends C == 19 through the class-generic
 * route too: an A/B switch to measure and cross-check the two routes. */
int mss_ood_score_f32(const float* dec2, int ld2, const float* dec1, int ld1, int N, int IH, int IW, int C,
                      int OH, int OW, float* score, float* logit_nchw, uint8_t* label, void* stream);
/* backward: given dscore [N,OH,OW] and dlogit NCHW [N,C,OH,OW] (either may be NULL) produce
 * ddec2 = -softmax(dec2) * gathered dscore / ddec1[c] = gathered dlogit[c] (NHWC, assigned; either may be NULL). Gather form, no
 * atomics: every source pixel sums the output pixels whose taps contain it in a fixed order. Same class range, check order
 * (C, then ddec2 without dec2 -> MSS_ERR_BAD_ARG, then N * IH * IW == 0 -> MSS_OK) and switch as the forward.
 * Where both gradients go into ONE pixel-contiguous buffer (ldd1 == ldd2, the two heads not overlapping inside a row of ldd
 * floats) the tiled regime (up-sampling by at most ~x4, OW % 4 == 0, ldd % 4 == 0, ld2 % 4 == 0, heads at multiples of 4 floats
 * with 4 * ceil(C/4) floats each, 16-byte aligned operands) writes the WHOLE row: the columns outside the two heads, the padding
 * up to the channel quad and the head of an absent gradient as zeros, so the buffer needs no memset. The class-generic route's
 * per-pixel fallback does the same for such a buffer; the <19> fallback writes the C columns of each head only. */
int mss_ood_score_bwd_f32(const float* dec2, int ld2, const float* dscore, const float* dlogit_nchw, int N,
                          int IH, int IW, int C, int OH, int OW, float* ddec2, int ldd2, float* ddec1, int ldd1,
                          void* stream);

/* Mask2Former anomaly score (train_m2f.py:387-407):
 *   score[b,h,w] = 1 - max_{c<C} sum_q softmax(cls[b,q,:])[c] * sigmoid(mask[b,q,h,w])
 * cls [B,Q,C+1], mask [B,Q,H,W] (row stride Wm >= W so a padded mask can be cropped in place). */
int mss_m2f_score_f32(const float* cls, const float* mask, int B, int Q, int C, int H, int W, int Hm, int Wm,
                      float* score, void* stream);

/* Fused RelContrastiveLoss (lib/loss.py:34-156): value AND both gradients in a few streaming passes.
 * The host side (multishiftseg_amd/loss.py) owns the workspaces and the call order:
 *   pass1 -> select -> pass2 -> compact -> cin_bwd -> pairs x2 (device pairing: pairs_device2 once) -> finalize
 * Nothing here synchronises with the host; every normaliser is read from device counters. */
typedef struct MssRclArgs {
  const float* logit;      /* [B,C,H,W] NCHW                                          */
  const float* score;      /* [B,H,W]                                                 */
  int64_t* target;         /* [B,H,W] int64; mutated exactly like loss.py:110-111,115 */
  int B, C, H, W;
  float w_ce_orig, w_ce_aug, w_contras;   /* ce_weights[0], ce_weights[1], contras_weight */
  float m0, m1, m2;                        /* inoutaug_contras_margins_tri                 */
  int select;                              /* conduct_pixel_selection && 0 < ratio < 1     */
  float selection_ratio;
} MssRclArgs;
/* counters: double[16]; slots 0 sum_ce_orig, 1 n_in_orig, 2 n_in_aug, 3 n_ood, 4 sum_c_in,
 * 5 n_same_in, 6 sum_ce_aug_all, 7 sum_selected_ce, 8 n_selected, 9 sum_c_orig, 10 sum_c_aug,
 * 11 n_pairs, 12 labels in [C, 99) or < 0 (F.nll_loss raises on those, loss.py:59: here the loss turns NaN and
 * out[6] of finalize reports the count). pass1 zeroes them.
 * pass1 (loss.py:46-69,90-96): lse[B*H*W] (only the augmented half is guaranteed to be written), ce_aug[(B/2)*H*W]
 * (+inf where ignored), kind[B*H*W] (0 void / 1 in-distribution / 2 OOD, from the UNmutated targets); B must be even
 * ([orig...; aug...] pairs). dlogit (optional [B,C,H,W]): pass1 also writes the gradient of every pixel whose weight
 * does not depend on the selection: the original half always, the augmented half when a->select == 0. */
int mss_rcl_pass1_f32(const MssRclArgs* a, float* lse, float* ce_aug, uint8_t* kind, double* counters, float* dlogit,
                      void* stream);
/* exact k-th smallest of ce_aug, k = int(float32(ratio) * float32(n_in_aug)) as torch computes
 * it (loss.py:98-99); replaces torch.topk (loss.py:102). sel: uint32[8]
 * = {threshold key, n_less, k, n_equal_to_take, tie tickets, ...}. 5 launches (each digit's pick rides in front of the next byte's
 * histogram pass): what mss_rcl_loss_device_f32 runs. scratch: MSS_RCL_SELECT_SCRATCH_WORDS uint32 (four histograms + two state
 * buffers), cleared by the call unless scratch_zeroed != 0. */
#define MSS_RCL_SELECT_SCRATCH_WORDS (4 * 256 + 16)
int mss_rcl_select_f32(const float* ce_aug, long long n, const double* counters, float selection_ratio,
                       uint32_t* scratch, int scratch_zeroed, uint32_t* sel, void* stream);
/* the same selection (same histogram and pick code, bit-identical sel[0..3]) one radix pass at a time (shift = 24, 16, 8, 0): a
 * data-parallel caller all-reduces the 256-bin histogram between hist and pick -> exact GLOBAL k-th smallest. hist_ws: uint32[256],
 * zeroed by init and by every pick. */
int mss_rcl_select_init_f32(const double* counters, float selection_ratio, uint32_t* hist_ws, uint32_t* sel,
                            void* stream);
int mss_rcl_select_hist_f32(const float* ce_aug, long long n, const uint32_t* sel, int shift, uint32_t* hist_ws,
                            void* stream);
int mss_rcl_select_pick_f32(uint32_t* sel, uint32_t* hist_ws, int shift, void* stream);
/* pass2 (selection mode only; a no-op when a->select == 0): the AUGMENTED half of dlogit (NCHW, assigned; may be
 * NULL) = grad_scale * d loss / d logit for the selected pixels and 0 for the others, target mutation, counters[7..8].
 * The original half was written by pass1, unscaled: grad_scale must be 1 (MSS_ERR_BAD_ARG otherwise; scale the loss
 * gradient downstream). */
int mss_rcl_pass2_f32(const MssRclArgs* a, const float* lse, const float* ce_aug, const uint8_t* kind,
                      uint32_t* sel, double* counters, float grad_scale, float* dlogit, void* stream);
/* row-major ordered compaction of pixel indices into the three sets of loss.py:122-124
 * (in-dist original half, in-dist augmented half, OOD); sizes to n_out (uint32[3]);
 * block_counts: uint32[3 * mss_rcl_num_compact_blocks(B,H,W)]. */
int mss_rcl_num_compact_blocks(int B, int H, int W);
int mss_rcl_compact_f32(const uint8_t* kind, int B, int H, int W, int32_t* idx_orig, int32_t* idx_aug,
                        int32_t* idx_ood, uint32_t* block_counts, uint32_t* n_out, void* stream);
/* dscore of the consistency term (loss.py:141-145); ASSIGNS all of dscore, call before pairs. */
int mss_rcl_cin_bwd_f32(const MssRclArgs* a, const uint8_t* kind, const double* counters, float grad_w,
                        float* dscore, void* stream);
/* hinge over n pairs (loss.py:129-137): sum_i relu(score[idx_a[perm_a[i]]] + margin -
 * score[idx_o[perm_o[i]]]) -> counters[9 + slot]; dscore += -+ grad_w/n (atomics; may be NULL).
 * perm_*: int64 permutations as torch.randperm returns them (parity mode: the caller injects
 * the reference's own permutations). */
int mss_rcl_pairs_f32(const float* score, const int32_t* idx_a, const int64_t* perm_a, const int32_t* idx_o,
                      const int64_t* perm_o, long long n, float margin, double* counters, int slot, float grad_w,
                      float* dscore, void* stream);
/* Both hinge terms of the device-pairing mode in one launch: n = min(max_samples, n_out[0..2]) and the permutations are keyed
 * Feistel bijections evaluated on the fly (no host round trip, no materialised randperm). Pair i of set `orig` (slot 0, margin_orig,
 * element feistel(i, n_orig, seed_orig)) and of set `aug` (slot 1, margin_aug, seed_aug) meet OOD element feistel(i, n_ood, seed_ood);
 * no atomics on dscore: thread i is the only writer of the three elements pair i touches. */
int mss_rcl_pairs_device2_f32(const float* score, const int32_t* idx_orig, const int32_t* idx_aug, const int32_t* idx_ood,
                              const uint32_t* n_out, long long max_samples, uint32_t seed_orig, uint32_t seed_aug, uint32_t seed_ood,
                              float margin_orig, float margin_aug, double* counters, float grad_w, float* dscore, void* stream);
/* data-parallel pairing over the rank-major concatenation of all ranks' sets: this rank owns the
 * slice [a_off, a_off+a_cnt_local) of global set A (a_cnt_global elements); ood_all is the
 * all-gathered [W][cap] OOD score vector with exclusive global offsets ood_off[W+1]; gradients w.r.t.
 * OOD scores are accumulated into g_ood [W][cap] (the caller all-reduces it and scatters its row). */
int mss_rcl_pairs_global_f32(const float* score, const int32_t* idx_a, uint32_t a_off, uint32_t a_cnt_local,
                             uint32_t a_cnt_global, const float* ood_all, const uint32_t* ood_off, int W,
                             uint32_t cap, uint32_t n_pairs, uint32_t seed_a, uint32_t seed_o, float margin,
                             double* counters, int slot, float coef, float* dscore, float* g_ood, void* stream);
int mss_rcl_gather_f32(const float* src, const int32_t* idx, uint32_t n, float* dst, void* stream);
int mss_rcl_scatter_add_f32(const float* g, const int32_t* idx, uint32_t n, float* dst, void* stream);
/* The whole loss of the device-pairing mode in ONE call (pass 1, radix select, pass 2, compaction, the in-distribution hinge, both
 * paired hinges, finalize -- the launches of the entry points above, issued back to back): workspace of
 * mss_rcl_workspace_bytes(B, H, W) bytes (256-byte aligned, contents irrelevant), max_samples = int(B*H*W * sample_ratio),
 * seed = the caller's step counter (pair i of step s couples Feistel(i; s) elements), dlogit / dscore nullable, out float[8] as
 * mss_rcl_finalize_f32. No host synchronisation. */
long long mss_rcl_workspace_bytes(int B, int H, int W);
int mss_rcl_loss_device_f32(const MssRclArgs* a, void* workspace, long long workspace_bytes, long long max_samples, uint32_t seed,
                            float* dlogit, float* dscore, float* out, void* stream);
/* out: float[8] = {loss, ce_orig, ce_aug, c_orig, c_aug, c_in, -, -} (loss.py:73-88,147). */
int mss_rcl_finalize_f32(const MssRclArgs* a, const double* counters, const uint32_t* sel, float* out,
                         void* stream);

/* Adam with L2-coupled weight decay (torch.optim.Adam semantics, train_deeplab.py:134-149), one parameter tensor per
 * call, updated in place together with its two moment buffers. Hyper-parameters are doubles, as Python holds them: the
 * bias corrections 1 - beta^step, the step size lr / bias1 and sqrt(bias2) are formed in double on the host and only the
 * derived scalars are rounded to float (torch/optim/adam.py, single-tensor path); step counts from 1. */
int mss_adam_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, double lr,
                      double beta1, double beta2, double eps, double weight_decay, int step, void* stream);

/* ---- multi-tensor AdamW with full-model gradient clipping (csrc/m2f_optim.hip; Mask2Former stage 2, train_m2f.py:211-299) ----
 * One call updates a LIST of `count` float32 tensors: clip_grad_norm_(all grads, max_norm) followed by torch.optim.AdamW's
 * single-tensor arithmetic with per-tensor lr, weight_decay and step count (torch/nn/utils/clip_grad.py, torch/optim/adam.py).
 * param / grad / exp_avg / exp_avg_sq / numel / lr / weight_decay / step are HOST arrays of `count` entries (device pointers,
 * element counts, Python's doubles, step counts from 1); they are read during the call only. Pointers may be 4-byte aligned
 * (a tensor whose four pointers are all 16-byte aligned takes 16-byte accesses). grad is never written: the clipped gradient
 * exists in registers only (torch scales p.grad in place).
 * clip != 0: per-chunk sums of squares go to scratch[slot] (scratch_floats >= mss_adamw_scratch_floats(count, numel); every slot
 * is written before it is read, the buffer needs no initialisation), one workgroup folds them in a fixed order in double and
 * leaves norm_out[0] = total_norm and norm_out[1] = min((1 / (total_norm + 1e-6)) * max_norm, 1) (torch's reverse division: reciprocal, then product; a NaN stays NaN) on the device;
 * the host never reads them. clip == 0: no norm launches, coefficient 1, scratch and norm_out may be NULL.
 * Launches: with L = the launches the list needs (mss_adamw_plan), L + 1 + L with clipping and L without; *launches (host, may
 * be NULL) receives the number issued. Empty tensors (numel 0) are skipped; an empty list is MSS_OK and launches nothing. */
int mss_adamw_clip_step_f32(int count, float* const* param, const float* const* grad, float* const* exp_avg,
                            float* const* exp_avg_sq, const long long* numel, const double* lr, const double* weight_decay,
                            const int* step, double beta1, double beta2, double eps, int clip, double max_norm, float* scratch,
                            long long scratch_floats, float* norm_out, int* launches, void* stream);
/* Host-only queries of the compile-time launch geometry: elements per workgroup (chunk), tensors and workgroups one launch's
 * kernel-argument table holds, and the scratch floats (= chunks) of a list. */
int mss_adamw_chunk_elems(void);
int mss_adamw_tensors_per_launch(void);
int mss_adamw_blocks_per_launch(void);
long long mss_adamw_scratch_floats(int count, const long long* numel);
/* The launch plan the step uses for a list, entry by entry in issue order: workgroup `block` of launch `launch` handles chunk
 * `chunk` of list entry `tensor` and owns scratch slot `slot`. Returns the number of entries (-1: bad arguments, or more than
 * 2^31 - 1 chunks); writes the first `capacity` of them when all five arrays are given (pass NULLs to size them). */
long long mss_adamw_plan(int count, const long long* numel, long long capacity, int* launch, int* block, int* tensor,
                         long long* chunk, int* slot);

/* Mask2Former anomaly score fused with the mask upsample (csrc/m2f.hip): logit = pixel-major
 * low-resolution mask logits [B, hm, wm, ldq] (queries contiguous; produced by mss_conv2d_forward_f32 in batched 1x1
 * mode from mask_features and mask_embed = einsum("bqc,bchw->bqhw"), mask2former_transformer_decoder.py:544-548);
 * the kernel applies F.interpolate(size=(Hi,Wi), bilinear, align_corners=False) (maskformer_model.py:264-277), the
 * sigmoid, the class mix and 1 - max (train_m2f.py:387-407) and writes the crop [B,H,W]. Q % 4 == 0, C <= 20.
 * prob_ws: a scratch of B * Q * 32 floats: the class mix then runs on the matrix cores (v_mfma_f32_32x32x2_f32: [classes x Q] x
 * [Q x pixels] per 32-pixel strip, one interpolation + sigmoid per lane and MFMA) instead of 20 multiply-adds per (pixel, query)
 * on the vector ALUs; results agree with the all-VALU form to fp32 summation order. prob_ws NULL = the all-VALU form. */
int mss_m2f_fused_score_ws_f32(const float* cls, const float* logit, int B, int Q, int C, int hm, int wm, int ldq, int Hi,
                               int Wi, int H, int W, float* score, float* prob_ws, void* stream);

/* Masked attention of the Mask2Former GMA transformer decoder (mask2former_transformer_decoder.py:75-121, 438-542; csrc/m2f_attn.hip).
 *
 * mss_m2f_attn_mask_bits_f32: logit = pixel-major low-resolution mask logits [B, hm*wm, ldq] (queries contiguous, Q <= 128,
 * ldq >= Q). Resamples them to (h, w) as F.interpolate(mode="bilinear", align_corners=False) does and writes
 *   bits    [B][2][h*w][W] 32-bit words, W = ceil(Q / 32): bit q of row [b][0][key] set <=> logit < 0 (key masked for the
 *           foreground attention: sigmoid(x) < 0.5), of row [b][1][key] set <=> logit > 0 (masked for the background attention);
 *           a logit of exactly 0 is masked in neither;
 *   allowed [B][2][W] words: bit q set <=> query q has at least one un-masked key (cleared by this call before the launch). A
 *           query whose bit is clear ignores its mask in mss_m2f_masked_attention_f32: the reference's
 *           attn_mask[where(attn_mask.sum(-1) == HW)] = False (:476-477) without the host round trip.
 * The mask is shared by the 8 heads. The bits of a last word past Q are clear in `bits` and unspecified in `allowed` (no reader
 * looks at them).
 *
 * mss_m2f_masked_attention_f32: out[b, q, a, head, :] = softmax_key(scale * <q, k> + mask) v for 8 heads of 32 channels and A
 * attentions in one launch. q [B*Q, ldq], k [B*NK, ldk], v [B*NK, ldv], out [B*Q, ldo] row-major fp32; attention a, head hd use
 * columns a*256 + hd*32 .. +31 of each (ld* >= A*256, multiples of 4, 16-byte aligned bases). bits / allowed: as written above
 * with A attentions per image ([B][A][NK][W], [B][A][W]); NULL bits = no mask (the self-attention among the queries).
 * The key range is split into `chunks` pieces (rounded to 8 keys; 1 = one pass, no workspace); each piece leaves numerators,
 * maximum and denominator in `ws` (>= mss_m2f_attn_workspace_bytes(B, Q, A, chunks) bytes, contents irrelevant on entry) and a
 * second kernel merges the pieces in index order: no float atomics, bit-reproducible for a given chunk count. Q <= 128. */
int mss_m2f_attn_mask_bits_f32(const float* logit, int B, int Q, int ldq, int hm, int wm, int h, int w, uint32_t* bits,
                               uint32_t* allowed, void* stream);
long long mss_m2f_attn_workspace_bytes(int B, int Q, int A, int chunks);
int mss_m2f_masked_attention_f32(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const uint32_t* bits,
                                 const uint32_t* allowed, int B, int Q, int NK, int A, float scale, int chunks, float* ws,
                                 float* out, int ldo, void* stream);

/* The masked attention for training.
 *
 * mss_m2f_masked_attention_lse_f32: mss_m2f_masked_attention_f32 (the same kernels: `out` is bit-identical for the same arguments and
 * chunk count) that also writes lse [B][A][8][Q], per (image, attention, head, query) the log-sum-exp of the scaled, masked scores
 * in the LOG2 domain: lse = log2(sum over the allowed keys of 2^(scale * log2(e) * <q, k>)) = natural lse * log2(e).
 *
 * mss_m2f_masked_attention_bwd_f32: with P = 2^(scale * log2(e) * <q, k> - lse) (0 where masked) and D = <dout, out> per query and head,
 *   dv = P^T dout,  dS = P o (dout v^T - D),  dq = scale * dS k,  dk = scale * dS^T q.
 * q / k / v / bits / allowed / out / lse as given to / returned by the forward, dout [B*Q, lddo]; row strides >= A*256, multiples of 4,
 * 16-byte aligned bases. dq [B*Q, A*256], dk / dv [B*NK, A*256] dense; any of the three may be NULL (not computed). Every element of a
 * non-NULL output is assigned exactly once (nothing needs zeroing); a key no query may attend to gets exact zeros. `chunks` cuts the
 * key range of the dq sum as in the forward (it need not be the forward's count); ws >= mss_m2f_attn_bwd_workspace_bytes(B, Q, A,
 * chunks) bytes (host arithmetic; 0 = unsupported shape), always needed (it holds D), contents irrelevant on entry. No float atomics:
 * bit-reproducible for a given chunk count. Q <= 128, A <= 16. */
int mss_m2f_masked_attention_lse_f32(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const uint32_t* bits,
                                     const uint32_t* allowed, int B, int Q, int NK, int A, float scale, int chunks, float* ws,
                                     float* out, int ldo, float* lse, void* stream);
long long mss_m2f_attn_bwd_workspace_bytes(int B, int Q, int A, int chunks);
int mss_m2f_masked_attention_bwd_f32(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const uint32_t* bits,
                                     const uint32_t* allowed, const float* out, int ldo, const float* lse, const float* dout, int lddo,
                                     int B, int Q, int NK, int A, float scale, int chunks, float* ws, float* dq, float* dk, float* dv,
                                     void* stream);

/* Pixel-level OOD metrics on the device (csrc/metric.hip): exact AUROC / average precision / FPR at `recall_level`
 * over all pixels with label id_out (positives) and id_in (negatives). Replaces eval_ood_measure, get_measures and
 * fpr_and_fdr_at_recall (lib/utils/metric.py:170-180, 130-153, 87-127; callers test_deeplab.py:94-102,
 * train_deeplab.py:236-241), which run sklearn on host copies of every score map.
 *   compact:  one pass over a batch of n pixels: order-preserving u32 keys of the id_in pixels' scores packed
 *             at the front of a key segment, those of the id_out pixels at the back, counted on the device
 *             (mss_oodm_compact_lanes_f32 below). No host synchronisation per batch.
 *   sort:     ascending key sort (own 4-pass LSD radix sort, csrc/metric.hip; keys 4-byte aligned, n < 2^32), temp sized
 *             by mss_oodm_sort_temp_bytes
 *   measures: out[0..2] = {AUROC, AUPRC, FPR@recall_level} (device f64[3]); u2_part / ap_part: device scratch of
 *             mss_oodm_rank_blocks(P) elements each. P, N >= 1 (the host mirror returns None otherwise, as
 *             metric.py:176-180 does). */
/* Compaction on EIGHT counters (a single counter is one address 512 workgroups of a 1024 x 2048 map add to one after the other:
 * the kernel's 20 us). The 4096-pixel chunks are dealt round-robin onto 8 lanes; lane L owns keys[L * cap, (L + 1) * cap) with
 * cap = mss_oodm_compact_lanes_cap(n) (keys: 8 * cap slots), its id_in keys from the front of the segment, its id_out keys from the
 * back; lane_counts (device u64[8], zero on entry)[L] = #id_in | (#id_out << 32) of the lane. n < 2^32. */
long long mss_oodm_compact_lanes_cap(long long n);
/* ... and for up to MSS_OODM_BATCH maps in one launch (an evaluation sweep that holds its score maps: test_deeplab.py:84-102 appends
 * every batch and evaluates at the end): entry m as the arguments of mss_oodm_compact_lanes_f32; entries >= count are ignored. */
#define MSS_OODM_BATCH 16
typedef struct MssOodmBatch {
  const float* score[MSS_OODM_BATCH];
  const long long* label[MSS_OODM_BATCH];
  unsigned int* keys[MSS_OODM_BATCH];
  unsigned long long* lane_counts[MSS_OODM_BATCH];
  long long n[MSS_OODM_BATCH];
} MssOodmBatch;
int mss_oodm_compact_lanes_batch_f32(const MssOodmBatch* batch, int count, long long id_in, long long id_out, void* stream);
/* One map's eight lane segments (keys, cap, lane_counts as mss_oodm_compact_lanes_f32 left them) copied to neg_out[0 .. #id_in) and
 * pos_out[0 .. #id_out) of that map: the sweep's contiguous sort inputs, the caller advancing the two pointers by the map's totals. */
int mss_oodm_gather_lanes_u32(const unsigned int* keys, long long cap, const unsigned long long* lane_counts, unsigned int* neg_out,
                              unsigned int* pos_out, void* stream);
int mss_oodm_compact_lanes_f32(const float* score, const long long* label, long long n, long long id_in, long long id_out,
                               unsigned int* keys, unsigned long long* lane_counts, void* stream);
long long mss_oodm_sort_temp_bytes(long long n);
int mss_oodm_sort_u32(const unsigned int* keys_in, unsigned int* keys_out, long long n, void* temp, long long temp_bytes,
                      void* stream);
int mss_oodm_rank_blocks(long long P);
int mss_oodm_measures_f64(const unsigned int* pos_sorted, long long P, const unsigned int* neg_sorted, long long N,
                          double recall_level, unsigned long long* u2_part, double* ap_part, double* out, void* stream);

/* ---- closed-set segmentation metrics (csrc/metric.hip) ----
 * replaces hist_info (lib/utils/metric.py:10-18) on the device; compute_metric / compute_score / compute_score_per_class
 * (metric.py:21-64) are host arithmetic on the table this accumulates (multishiftseg_amd/metric.py).
 *   hist u64 [n_cl * n_cl + 1], ACCUMULATED into (the caller zeroes it once per sweep): hist[gt * n_cl + pred] += 1 for every pixel
 *   with 0 <= gt < n_cl (metric.py:12; 254 / 255 and negative labels drop out, the full 64-bit value is compared). The last slot
 *   counts labelled pixels whose map prediction lies outside 0 .. n_cl-1, where the reference raises or files the pixel in another
 *   row. `labeled` and `correct` of hist_info are the table's sum and trace.
 *   pred_kind 0: pred = float32 logits, B x n_cl planes of HW contiguous pixels, image b's plane c at pred + b * img_stride +
 *     c * chan_stride (elements; a channel slice of a wider tensor goes in as it is). The argmax over c is fused, with np.argmax's
 *     semantics: the first maximal index, -0.0 == 0.0, a NaN is maximal and the first NaN wins, all -inf gives 0. Any alignment.
 *   pred_kind 1 / 8: pred = a uint8 / int64 prediction map [B, HW] (what mss_ood_score_f32 writes as `label`); strides ignored.
 *   label [B, HW], label_bytes 1 (uint8) or 8 (int64).
 * Checked in this order, before any HIP call: a NULL pointer, another pred_kind or label_bytes, B < 0 or HW < 0 ->
 * MSS_ERR_BAD_ARG; n_cl outside 2..32 -> MSS_ERR_UNSUPPORTED; B == 0 or HW == 0 -> MSS_OK, nothing launched; B * HW >= 2^32 ->
 * MSS_ERR_UNSUPPORTED; for logits chan_stride < HW or img_stride < n_cl * chan_stride (overlapping planes; negative strides are
 * among them) -> MSS_ERR_BAD_ARG. One launch, integer atomics only: two runs give the same table. */
int mss_seg_hist(const void* pred, int pred_kind, long long img_stride, long long chan_stride, const void* label, int label_bytes,
                 int B, long long HW, int n_cl, unsigned long long* hist, void* stream);

/* ---- Mask2Former pixel decoder glue (csrc/norm.hip; msdeformattn.py:116-131,215-219,262-281,314-358) ----
 * y = LayerNorm(x + res) over the last dimension C (multiple of 256, <= 1024; res may be NULL): the post-norm residual
 * sites of MSDeformAttnTransformerEncoderLayer in one pass. stat (optional) [rows][2] = (mean, rstd) for the backward. */
int mss_add_layernorm_f32(const float* x, const float* res, long long rows, int C, const float* gamma, const float* beta,
                          float eps, float* y, float* stat, void* stream);
/* backward: dz [rows][C] (= gradient w.r.t. x and w.r.t. res), dgamma / dbeta [C] (optional). ws: scratch of
 * mss_add_layernorm_bwd_workspace_floats floats; per-workgroup partials added in a fixed order (no atomics). */
long long mss_add_layernorm_bwd_workspace_floats(long long rows, int C);
int mss_add_layernorm_bwd_f32(const float* gy, const float* x, const float* res, const float* stat, long long rows, int C,
                              const float* gamma, float* dz, float* dgamma, float* dbeta, float* ws, void* stream);
/* r04: the output of an encoder layer's second LayerNorm has two consumers in the next layer, the layer input `src` and the
 * query q = src + pos (msdeformattn.py:116-118 with_pos_embed). mss_add_layernorm_q_f32 also writes q = y + pos[row % pos_rows]
 * (pos: [pos_rows][C], one image's tokens when the batch shares them); mss_add_layernorm_bwd_sum2_f32 takes the two gradients
 * (gy2 may be NULL) and adds them while loading. Same bits as the separate elementwise passes they replace. It also writes
 * dzsum [C] = per-channel sums of dz: the bias gradient of the Linear whose output was `res` (msdeformattn.py:116-131:
 * output_proj / linear2) without another pass over [rows][C]. ws: 3/2 of mss_add_layernorm_bwd_workspace_floats. */
int mss_add_layernorm_q_f32(const float* x, const float* res, long long rows, int C, const float* gamma, const float* beta,
                            float eps, float* y, float* stat, const float* pos, long long pos_rows, float* q, void* stream);
int mss_add_layernorm_bwd_sum2_f32(const float* gy, const float* gy2, const float* x, const float* res, const float* stat, long long rows,
                                   int C, const float* gamma, float* dz, float* dgamma, float* dbeta, float* dzsum, float* ws,
                                   void* stream);
/* nn.GroupNorm(groups, C) on NHWC x [N][HW][C] (pixel stride ldx, sample stride x_sample_stride floats), optional ReLU,
 * output with its own pixel / sample strides (e.g. straight into the encoder's token buffer [N][sum HW][C]).
 * C/groups a multiple of 4, C <= 1024. ws: scratch of mss_groupnorm_workspace_floats floats. Deterministic. */
long long mss_groupnorm_workspace_floats(int N, int HW, int C, int groups);
int mss_groupnorm_nhwc_f32(const float* x, int ldx, long long x_sample_stride, int N, int HW, int C, int groups,
                           const float* gamma, const float* beta, float eps, int relu, float* y, int ldy,
                           long long y_sample_stride, float* ws, void* stream);
/* backward of mss_groupnorm_nhwc_f32 (the pixel decoder is trainable in Mask2Former's second stage): stat = the forward's
 * [N*groups][2] (mean, rstd), left by the forward at ws + mss_groupnorm_stat_offset(N, HW, C) floats; relu = the forward
 * fused a ReLU. dx contiguous NHWC (pixel stride lddx), dgamma / dbeta [C] optional. Deterministic (fixed-order sums). */
long long mss_groupnorm_stat_offset(int N, int HW, int C);
long long mss_groupnorm_bwd_workspace_floats(int N, int HW, int C, int groups);
int mss_groupnorm_nhwc_bwd_f32(const float* gy, int ldg, long long g_sample_stride, const float* x, int ldx,
                               long long x_sample_stride, int N, int HW, int C, int groups, const float* stat,
                               const float* gamma, const float* beta, int relu, float* dx, int lddx, float* dgamma,
                               float* dbeta, float* ws, void* stream);
/* transpose of the bilinear part of mss_upsample_bilinear_add_nhwc_f32: dtop (+)= B^T dy (the lateral gradient is dy). */
int mss_upsample_bilinear_bwd_nhwc_f32(const float* dy, int lddy, int N, int OH, int OW, float* dtop, int ldt,
                                       long long top_sample_stride, int IH, int IW, int C, int accumulate, void* stream);
/* NCHW gradient -> rows of an NHWC / token buffer (pixel stride ldd, sample stride d_sample_stride floats), optional +=. */
int mss_nchw_to_nhwc_strided_f32(const float* g, int N, int C, int HW, float* dst, int ldd, long long d_sample_stride,
                                 int accumulate, void* stream);
/* FPN top-down step (msdeformattn.py:344): y = lat + F.interpolate(top, size=(OH, OW), mode="bilinear",
 * align_corners=False); NHWC with pixel strides (top also with a sample stride: a level inside the token buffer).
 * lat == NULL: the interpolation alone, y = F.interpolate(top, ...), no lateral read and no add; ldl is ignored. Same source
 * coordinates and blend as the add form, whose result over an all-zero lat it equals. Mask2Former stage 1 takes the decoder's
 * pixel-major mask logits [n, hm, wm, ldq] to the padded image size with it (kernels.m2f_semantic_inference). */
int mss_upsample_bilinear_add_nhwc_f32(const float* top, int ldt, long long top_sample_stride, int N, int IH, int IW,
                                       const float* lat, int ldl, float* y, int ldy, int OH, int OW, int C, void* stream);
/* NHWC (pixel stride ldx, sample stride x_sample_stride floats) -> contiguous NCHW: the decoder returns NCHW maps like
 * the reference. */
int mss_nhwc_to_nchw_f32(const float* x, int ldx, long long x_sample_stride, int N, int HW, int C, float* y, void* stream);

/* ---- what the Mask2Former matcher and criterion share: the mask logits of S prediction steps and the target pack ----
 * Plain HOST structs that hold DEVICE pointers (as MssOodmBatch). One tensor per prediction step (the last output and the
 * aux_outputs are separate tensors), at most MSS_M2F_MAX_STEPS; entries >= S are ignored, an entry < S that is NULL is a bad argument. */
#define MSS_M2F_MAX_STEPS 16
typedef struct MssM2fSteps { const float* step[MSS_M2F_MAX_STEPS]; } MssM2fSteps;      /* tensors that are read, e.g. class logits [B,Q,C1] contiguous */
typedef struct MssM2fGrads { float* step[MSS_M2F_MAX_STEPS]; } MssM2fGrads;            /* tensors that are written, in the layout of what they are the gradient of */
/* Mask logits of B images, all steps of one shape and layout: element (b, q, y, x) of step s at step[s] + b*img_stride + q*query_stride
 * + (y*w + x)*pixel_stride floats. NCHW [B,Q,h,w]: (Q*h*w, h*w, 1); pixel-major [B,h,w,ldq]: (h*w*ldq, 1, ldq). */
typedef struct MssM2fMaps {
  const float* step[MSS_M2F_MAX_STEPS];
  long long img_stride, query_stride, pixel_stride;
  int S, B, Q, h, w;
} MssM2fMaps;
/* tmask uint8 [total_t,H,W] (0/1), tstart int32 [B+1]: image b owns targets tstart[b] .. tstart[b+1]-1; labels int32 [total_t] (NULL
 * where the call does not read them). Shared by all steps. tmask (and labels) may be NULL when total_t == 0. */
typedef struct MssM2fTargets {
  const uint8_t* tmask; const int* tstart; const int* labels;
  int total_t, H, W;
} MssM2fTargets;

/* ---- Hungarian matching of Mask2Former (csrc/m2f_match.hip) ----
 * replaces HungarianMatcher.memory_efficient_forward, lib/network/mask2former/modeling/matcher.py:95-156 (batch_dice_loss :15-30,
 * batch_sigmoid_ce_loss :38-62), called from criterion.py:444,463 once per prediction step. A problem is one (step s, image b):
 * all S*B problems of a train step go through one call = two launches, no float atomics, no host synchronisation.
 *   maps: the mask logits (S, B, Q come from it); cls: class logits [B,Q,C1] per step, C1 = classes + 1.
 *   targets: T_b <= Q <= 128, T_b <= Tmax <= 128; labels are read. points [S,B,P,2] = (x, y) in [0,1), shared by the masks of a problem
 *     (matcher.py:119-132); point_sample = F.grid_sample(2u-1, bilinear, align_corners=False, zeros): pixel coordinate u*n - 0.5.
 *   cost [S,B,Q,Tmax] fp32 = w_mask cost_mask + w_class cost_class + w_dice cost_dice (matcher.py:144-148), columns >= T_b
 *     written as 0. ws: mss_m2f_match_workspace_bytes bytes of float scratch = 4 * S*B * NC * (2*Q*TP + 2*Q + TP) with
 *     TP = Tmax rounded up to 16 and NC = min(16, ceil(P / 64)) point chunks, added in index order in float64 (bit-reproducible).
 *   match / status (both or neither; NULL = cost only): the assignment is solved in the same second launch. */
long long mss_m2f_match_workspace_bytes(int S, int B, int Q, int Tmax, int P);
int mss_m2f_match_cost_f32(const MssM2fMaps* maps, const MssM2fSteps* cls, const MssM2fTargets* targets, const float* points, int C1, int P,
                           int Tmax, float w_class, float w_mask, float w_dice, float* ws, float* cost, int* match, int* status, void* stream);
/* linear_sum_assignment (matcher.py:151) of cost [S,B,Q,Tmax] fp32, tcount int32 [B] targets per image: one wave per problem,
 * shortest augmenting paths (Crouse 2016, scipy's algorithm) in float64, every loop bounded by T_b or Q. match [S,B,Tmax] int32 =
 * the query of target m (-1 in the padding); status [S,B] int32: 0 solved, 1 infeasible / NaN / -inf cost / bad count (scipy's
 * ValueError; match is then all -1). Equal costs: the lowest column wins. */
int mss_m2f_match_assign_f32(const float* cost, const int* tcount, int S, int B, int Q, int Tmax, int* match, int* status,
                             void* stream);

/* ---- SetCriterion of Mask2Former: class and sampled-mask losses (csrc/m2f_loss.hip) ----
 * replaces loss_labels (lib/network/mask2former/modeling/criterion.py:189-205), loss_masks (:312-363), loss_masks_aug (:244-310),
 * get_clean_point_coords_with_randomness (:371-407) and detectron2's get_uncertain_point_coords_with_randomness for all S
 * prediction steps of a train step (criterion.py:455-467) in a fixed number of launches: no float atomics, no host synchronisation.
 * A row is one matched (step s, target g): r = s*total_t + g, g = tstart[b] + m; its source map is the mask logits of query
 * match[s,b,m] of image b in step s (maps and targets as above; labels are read by finalize only; match [S,B,Tmax]), its
 * target map tmask[g]. A row whose table entry is outside [0, Q) has no map: its points are written as 0 and its sums as NaN.
 *
 * select (criterion.py:335-341, :371-407): rows with g >= sel_start sample their K candidates cand[s, g - sel_start, :, :]
 *   (cand [S, total_t - sel_start, K, 2], (x, y) in [0,1)), keep the k with the largest key (mode 1 "uncertain": -|x|; mode 2
 *   "clean": -BCEWithLogits(x, t)) in ascending candidate index and append the first P - k points of rnd[r] (rnd [S*total_t, Pr, 2]);
 *   rows with g < sel_start ("random", :365-369) take the first P points of rnd[r]. Ties at the k-th largest key: the lowest
 *   candidate index wins; -0.0 == +0.0; a NaN key ranks below every number. The exact k-th largest comes from 4 x 8-bit radix
 *   passes over the row's keys in ws (mss_m2f_loss_workspace_bytes(S*total_t, K, P) bytes). points [S*total_t, P, 2] is written whole.
 * mask_forward (:343-358): rows [S*total_t, 4] double = sum_p BCEWithLogits(x,t), sum_p sigmoid(x) t, sum_p sigmoid(x), sum_p t
 *   at the row's P points, one fixed summation order.
 * finalize (:189-205, :301-306, :356-359): one workgroup per step. tclass [S,B,Q] int32 = labels[g] of the matched target, else
 *   C1 - 1; loss[s,0] = sum w[c] (logsumexp - x[c]) / sum w[c]; rows with g < split belong to group 0, the others to group 1;
 *   loss[s, 1 + 2 G] = scale_G sum_rows bce / P, loss[s, 2 + 2 G] = scale_G sum_rows (1 - (2 st + 1) / (sg + tt + 1)), in row order
 *   in float64; ncols = 3 (one group: split = total_t) or 5. wsum [S] double = sum w[c]. A table entry outside [0, Q) of a real
 *   target or a label outside [0, C1 - 1) sets bad[s] = 1 and every loss of the step to NaN.
 * mask_backward: gloss [S,ncols] = the upstream gradient of loss. Per point (sigmoid(x) - t) a / P - ((2 t D - N) / D^2) sigmoid(x)
 *   (1 - sigmoid(x)) d with a = gloss[s,1+2G] scale_G, d = gloss[s,2+2G] scale_G, N = 2 st + 1, D = sg + tt + 1, scattered through
 *   the four bilinear taps into an int64 fixed-point window in LDS (quantum 2^(e-60), 2^e >= P (|a|/P + 2|d|)), converted once:
 *   the map of a matched query is written whole by its row's workgroup, other maps are left as they are (the caller zeroes them).
 *   grads: one tensor per step in the layout of maps. ws: mss_m2f_loss_workspace_bytes(S*total_t, 0, P) bytes.
 *   Rows of a bad step write nothing.
 * label_backward: grads->step[s] [B,Q,C1] = w[c]/wsum (softmax - onehot) gloss[s,0], written whole (0 for a bad step). */
long long mss_m2f_loss_workspace_bytes(long long R, int K, int P);
int mss_m2f_loss_select_f32(const MssM2fMaps* maps, const MssM2fTargets* targets, const int* match, const float* cand, const float* rnd,
                            int Tmax, int K, int k, int P, int Pr, int mode, int sel_start, float* ws, float* points, void* stream);
int mss_m2f_loss_mask_forward_f32(const MssM2fMaps* maps, const MssM2fTargets* targets, const int* match, const float* points, int Tmax,
                                  int P, double* rows, void* stream);
/* finalize and label_backward read no mask logits: they take S, B and Q as they are; finalize reads tstart, labels and total_t of targets. */
int mss_m2f_loss_finalize_f32(const MssM2fSteps* cls, const MssM2fTargets* targets, const int* match, const float* weight,
                              const double* rows, int S, int B, int Q, int C1, int Tmax, int P, int split, double scale0, double scale1,
                              int ncols, int* tclass, int* bad, double* wsum, float* loss, void* stream);
int mss_m2f_loss_mask_backward_f32(const MssM2fMaps* maps, const MssM2fTargets* targets, const int* match, const int* bad,
                                   const float* points, const double* rows, const float* gloss, int Tmax, int P, int split, double scale0,
                                   double scale1, int ncols, float* ws, const MssM2fGrads* grads, void* stream);
int mss_m2f_loss_label_backward_f32(const MssM2fSteps* cls, const int* tclass, const int* bad, const float* weight, const double* wsum,
                                    const float* gloss, int S, int B, int Q, int C1, int ncols, const MssM2fGrads* grads, void* stream);

/* ---- SetCriterion.loss_ood, RCL branch: the class mix, forward and backward (csrc/m2f_mix.hip) ----
 * replaces, per prediction step, lib/network/mask2former/modeling/criterion.py:133-138 and :170-175 (softmax without the last
 * column, sigmoid, einsum("bqc,bqhw->bchw") at the low resolution h x w), :166-168 and :177-179 (F.interpolate to (H, W), bilinear,
 * align_corners=False, cropped to Ht x Wt), :181 (-max over the classes), and what autograd derives from them. fp32; Q <= 128,
 * 1 <= C <= 32. masks / strides as in mss_m2f_match_cost_f32: NCHW [B,Q,h,w] (pixel_stride 1, any Q) or pixel-major [B,h,w,ldq]
 * (query_stride 1, pixel_stride ldq, ldq % 4 == 0, Q <= ldq; the columns Q..ldq-1 are never read). No float atomics, no memset:
 * every output element is written once, every sum runs in one fixed order, two runs give the same bits.
 *
 * forward (:135-138): prob [B,Q,C] = softmax(cls [B,Q,C+1])[..., :C]; mix [B,C,h,w] = sum_q prob[b,q,c] sigmoid(masks[b,q,p]),
 *   the queries in index order.
 * upsample (:166-168, :177-181): neg_max == 0: out [B,Cl,Ht,Wt], Cl = min(C,19), = the first Cl channels interpolated;
 *   neg_max != 0: out [B,Ht,Wt] = -max over all C interpolated channels, which are never stored. The scale is h / H (w / W), not
 *   h / Ht; the coordinate is src_coord of csrc/mss_bilinear.h and the blend h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11) as ATen.
 * upsample_backward: dmix [B,C,h,w], written whole, from dlogits [B,Cl,Ht,Wt] and / or dscore [B,Ht,Wt] (either may be NULL; mix
 *   is needed with dscore). A low-resolution pixel sums over the output pixels of the crop whose taps contain it, rows then columns
 *   ascending. For dscore the C interpolated values of the output pixel are recomputed and -dscore goes to the largest; equal
 *   values: the lowest class index (torch.max leaves that unspecified).
 * backward: dmasks in the layout of masks (the pad columns of a pixel-major layout written as 0) = sigmoid'(x) sum_c prob dmix;
 *   dcls [B,Q,C+1] = the softmax backward with the dropped column of dP[b,q,c] = sum_p dmix[b,c,p] sigmoid(x[b,q,p]), summed per
 *   workgroup (mss_m2f_mix_backward_chunks(h*w) workgroups per image) into partial [B, chunks, Q, C] double and folded in index order
 *   (partial is scratch: the fold leaves each image's sums in the slot of its chunk 0).
 *   dmasks == NULL (frozen masks, Mask2Former stage 1): neither the sigmoid'(x) sum_c prob dmix work nor the store of a tensor of
 *   the size of masks; dcls is bit-identical to the full call's (the same partial sums, folded in the same order). */
int mss_m2f_mix_backward_chunks(long long hw);
int mss_m2f_mix_forward_f32(const float* cls, const float* masks, long long img_stride, long long query_stride, long long pixel_stride,
                            int B, int Q, int C, int h, int w, float* prob, float* mix, void* stream);
int mss_m2f_mix_upsample_f32(const float* mix, int B, int C, int h, int w, int H, int W, int Ht, int Wt, int neg_max, float* out,
                             void* stream);
int mss_m2f_mix_upsample_backward_f32(const float* dlogits, const float* dscore, const float* mix, int B, int C, int h, int w, int H,
                                      int W, int Ht, int Wt, float* dmix, void* stream);
int mss_m2f_mix_backward_f32(const float* dmix, const float* prob, const float* cls, const float* masks, long long img_stride,
                             long long query_stride, long long pixel_stride, int B, int Q, int C, int h, int w, double* partial,
                             float* dmasks, float* dcls, void* stream);

/* ---- Mask2Former targets from label maps (csrc/m2f_targets.hip) ----
 * replaces train_m2f.py:342-385 (prepare_input: target[b].cpu().numpy(), np.unique, one `sem_seg == class_id` map per class, the OOD
 * map) and lib/network/mask2former/maskformer_model.py:316-339 (prepare_targets: the zero padding to Hp x Wp) and leaves the pack
 * MssM2fTargets describes. sem [B,H,W] contiguous, sem_bytes per element: 8 (int64), 4 (int32) or 1 (uint8). A value v is a class
 * iff 0 <= v < label_threshold (1..128); a pixel is OOD iff v > label_threshold and v != ignore_label; v == label_threshold is
 * neither, and (unlike the reference, which would hand its criterion a negative label) neither is a negative v.
 *   phase 0 "count", two launches behind a memset of present: present uint64 [B][2] = the set of classes of image b (bit v of the
 *     128-bit set; integer atomicOr, exact); tstart int32 [B+1]; labels int32, room for B * label_threshold, the first tstart[B]
 *     valid: the classes of image b ascending (np.unique's order) from tstart[b]; rank int32 [B][label_threshold]: the row of
 *     class v inside image b, or -1. tmask, ood and total_t are not used.
 *   phase 1 "fill", one launch: EVERY byte of tmask uint8 [total_t,Hp,Wp] and of ood uint8 [B,Hp,Wp] is written: row
 *     tstart[b] + rank[b][v] of tmask is 1 where sem[b] == v, ood[b] is 1 where the pixel is OOD, both 0 elsewhere and in the padding
 *     (y >= H or x >= W). total_t = tstart[B] as the host read it; rows >= total_t are never written. total_t == 0 is valid: tmask
 *     may then be NULL and ood is still written. present and labels are not used. The stores are as wide (16 bytes at most) as Wp
 *     and the two base addresses are aligned to, single bytes where Wp is odd.
 * Integer arithmetic only, no float atomics, no scratch: two runs give the same bytes. */
int mss_m2f_targets_from_labels(const void* sem, int sem_bytes, int B, int H, int W, int Hp, int Wp, int label_threshold, int ignore_label,
                                int phase, unsigned long long* present, int* tstart, int* labels, int* rank, long long total_t,
                                unsigned char* tmask, unsigned char* ood, void* stream);

/* ---- on-device data path of the DeepLab trainer (csrc/data.hip) ----
 * One kernel for what DiverseCityscapes.__getitem__ + its transforms + the trainer's batch concat do per step
 * (lib/dataset/cityscapes.py:153-171, lib/utils/img_utils.py:110-153,246-259,398-435, train_deeplab.py:190-195):
 * img / gen [B,H,W,3] uint8 (original and generated image, pre-decoded, device), tgt / gen_tgt [B,H,W] uint8;
 * mix_p [B] double (device; NULL = no mixup): gen <- uint8(p*img + (1-p)*gen) in float64; crop [B][2] int (device): top,
 * left of the common h x w window; flip [B] int (device, NULL = none): horizontal flip of the window; mean3 / std3:
 * HOST double[3] (the Python floats of opt.data.mean / std; Normalize uses their float32 roundings, the pasted object the
 * doubles, as the reference does); obj_img [B][OHmax][OWmax][3] float32 (0..255, already rescaled), obj_mask
 * [B][OHmax][OWmax] uint8, obj_geom [B][6] int = (y1, x1, bh, bw, h0, w0): the mask's bounding box inside the object and
 * the paste corner in the window (bh = 0: nothing pasted; all three NULL: no anomaly mix). Outputs: out_img [2B,3,h,w]
 * float32 and out_tgt [2B,h,w] int64, originals first, then the augmented images. */
int mss_data_pair_f32(const uint8_t* img, const uint8_t* gen, const uint8_t* tgt, const uint8_t* gen_tgt, int B, int H, int W,
                      int h, int w, const double* mix_p, const int* crop, const int* flip, const double* mean3,
                      const double* std3, const float* obj_img, const uint8_t* obj_mask, const int* obj_geom, int OHmax,
                      int OWmax, float* out_img, int64_t* out_tgt, void* stream);

/* Calibration kernels (bench.py: achievable peaks of this device next to the datasheet ones).
 * mss_peak_mfma_f32: blocks x 4 waves x iters x 16 back-to-back v_mfma_f32_32x32x2_f32 (4096 FLOP
 * each), out >= blocks*256 floats. mss_peak_stream_f32: float4 copy of n floats (8*n bytes moved);
 * variant 0..3 = plain / 4 loads in flight / + nontemporal / + contiguous 16-KB chunks per workgroup; round 6: 4 = write-only (4*n bytes),
 * 5 = read-only (4*n bytes), 6 = first half of src read, all of dst written (6*n bytes: the 1 : 2 mix of the Winograd input transforms); n % 8 == 0. */
int mss_peak_mfma_f32(float* out, int blocks, int iters, void* stream);
/* The same for the bf16 matrix cores under load (the split-bf16 GEMM route's ceiling): register-only loops on pseudo-random operands,
 * blocks x 4 waves x iters x 1 572 864 FLOP; shape 0 = 48 x v_mfma_f32_32x32x16_bf16 per iteration, 1 = 96 x v_mfma_f32_16x16x32_bf16. */
int mss_peak_mfma_bf16(float* out, int blocks, int iters, int shape, void* stream);
int mss_peak_stream_f32(const float* src, float* dst, long long n, int variant, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSS_HIP_H */
