/* C ABI of libmss_ood.so: the pixel losses of SetCriterion.loss_ood, branches "margin" and "bce", on an MI355X (gfx950).
 *
 * Per prediction step the reference (lib/network/mask2former/modeling/criterion.py:128-161) takes the class mix
 * M = einsum("bqc,bqhw->bchw", softmax(pred_logits)[..., :-1], sigmoid(pred_masks)) at the LOW resolution h x w and computes
 *
 *     t = -max_c M                                                         [B, h, w]
 *     s = interpolate(t, (H, W), bilinear, align_corners=True)             [B, H, W]   the size of ood_mask, no crop
 *     margin: loss = 0.5 (mean_{ood == 0} s^2          + [n_ood > 0] mean_{ood == 1} max(margin - s, 0)^2)
 *     bce:    loss = 0.5 (mean_{ood == 0} softplus(s)  + [n_ood > 0] mean_{ood == 1} softplus(-s))
 *
 * with the two pixel sets counted over the whole batch; a mask byte other than 0 and 1 belongs to neither. The mix itself and its
 * backward are mss_m2f_mix_forward_f32 / mss_m2f_mix_backward_f32 of libmss_hip.so; this library holds what lies between them.
 * It is separate from libmss_hip.so (include/mss_hip.h, closed at 142 entry points) and libmss_aug.so (include/mss_aug_hip.h,
 * closed at 12), shares no symbol with either and needs none of theirs.
 *
 * Conventions (those of mss_hip.h):
 *   - every pointer is a device pointer;
 *   - a status-returning function returns int and ends in `void* stream` (a hipStream_t, NULL = the default stream):
 *     0 = launched, MSS_ERR_BAD_ARG / MSS_ERR_UNSUPPORTED = refused, anything else = a hipError_t;
 *   - the arguments are checked BEFORE any HIP call, in the order "the common checks" lists, so a refused call touches no device;
 *   - no float atomics, no memset, no device-to-host copy: two runs give the same bits; every output and workspace element is
 *     written before it is read.
 * Where classes tie for the maximum of M, the lowest class index counts and takes the gradient.
 */
#ifndef MSS_OOD_HIP_H
#define MSS_OOD_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSS_OOD_ABI_VERSION 1
#ifndef MSS_ERR_BAD_ARG
#define MSS_OK 0
#define MSS_ERR_BAD_ARG 1001
#define MSS_ERR_UNSUPPORTED 1002
#endif

/* the common checks, in this order:
 *   1. a NULL pointer that is not marked optional                                -> MSS_ERR_BAD_ARG
 *   2. B, C, h, w, H or W < 1                                                    -> MSS_ERR_BAD_ARG
 *   3. kind outside {MSS_OOD_MARGIN, MSS_OOD_BCE}, a margin that is not finite   -> MSS_ERR_BAD_ARG
 *   4. C > MSS_OOD_MAX_CLASSES, B h w or B H W > MSS_OOD_MAX_PIXELS              -> MSS_ERR_UNSUPPORTED (32-bit pixel indices) */
#define MSS_OOD_MAX_CLASSES 32
#define MSS_OOD_MAX_PIXELS 0x7fffffffll
#define MSS_OOD_MARGIN 0
#define MSS_OOD_BCE 1

int mss_ood_abi_version(void);

/* Workgroups of the forward reduction = rows of its `partial` workspace, for B H W = pixels; 0 for pixels < 1 or beyond the limit. */
int mss_ood_loss_partials(long long pixels);

/* t[b, p] = -max_c mix[b, c, p]. mix float32 [B, C, h, w], t float32 [B, h, w]. Checks: common 1, 2, 4. */
int mss_ood_negmax_f32(const float* mix, int B, int C, int h, int w, float* t, void* stream);

/* The loss of one step. t float32 [B, h, w]; ood uint8 [B, H, W]; margin is read for kind MSS_OOD_MARGIN only (and checked always).
 * partial: float64 [mss_ood_loss_partials(B H W), 4] workspace, written whole: per workgroup (S_id, S_ood, n_id, n_ood) over its fixed
 *          range of pixels, in one fixed order.
 * stats:   float64 [4] = the partials added in index order: the two sums of the per-pixel terms and the two pixel counts.
 * loss:    float32 [1] = (float)(0.5 * (S_id / n_id + (n_ood > 0 ? S_ood / n_ood : 0))) in double; n_id == 0 gives NaN, as the
 *          reference's mean over an empty tensor.
 * score:   optional float32 [B, H, W]: s, for tests and diagnosis.
 * Two launches. Checks: common 1-4. */
int mss_ood_pixel_loss_f32(const float* t, const uint8_t* ood, int B, int h, int w, int H, int W, int kind, float margin, double* partial,
                           double* stats, float* loss, float* score, void* stream);

/* d loss / d mix, written whole: for low-resolution pixel (b, p) the channel argmax_c mix[b, c, p] (the lowest index among equals)
 * gets -sum over the output pixels o that have p among their taps, rows then columns ascending, of wy wx g(o), every other channel 0;
 * g = gloss * 0.5 * l'(s) / n_set with s recomputed from t as the forward computes it, n_set from stats (1 / n = 0 for an empty set)
 * and l' = 2 s | -2 max(margin - s, 0) (margin), sigmoid(s) | sigmoid(s) - 1 (bce) for the sets ood == 0 | ood == 1.
 * mix float32 [B, C, h, w]; t, ood, stats as above (stats as the forward left it); gloss float32 [1], the upstream gradient of
 * loss; dmix float32 [B, C, h, w]. One launch. Checks: common 1-4. */
int mss_ood_pixel_loss_backward_f32(const float* mix, const float* t, const uint8_t* ood, const double* stats, const float* gloss, int B,
                                    int C, int h, int w, int H, int W, int kind, float margin, float* dmix, void* stream);

#ifdef __cplusplus
}
#endif
#endif
