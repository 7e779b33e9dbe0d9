/* C ABI of libmss_aug.so: the Mask2Former input pipeline on an MI355X (gfx950).
 *
 * The trainer's augmentation chain (train_m2f.py:48-61 over lib/utils/img_utils.py) and what surrounds it in
 * DiverseCityscapes.__getitem__ (lib/dataset/cityscapes.py:153-171), as HIP kernels over ONE sample's working set:
 *
 *     x   float32 [N, 3, H, W]   planar images in [0, 1]; N = 2: the image and the generated image, the reference's own stack
 *     m   uint8   [N, H, W]      their label maps (0..255; bytes until the last kernel widens them to int64)
 *
 * This library is separate from libmss_hip.so (include/mss_hip.h) and shares no symbol with it: the input pipeline has nothing in
 * common with the GEMM / convolution library, whose entry-point table is closed at 142 functions. A feature that needs an entry
 * point outside that library's subject puts it into a library of its own, as this one does.
 *
 * Conventions (those of mss_hip.h):
 *   - every pointer is a device pointer unless its comment says HOST;
 *   - a status-returning function returns int and ends in `void* stream` (a hipStream_t, NULL = the default stream):
 *     0 = launched, MSS_ERR_BAD_ARG / MSS_ERR_UNSUPPORTED = refused, anything else = a hipError_t;
 *   - the arguments are checked BEFORE any HIP call, in the order each comment lists, so a refused call touches no device;
 *   - the random decisions are the host's (multishiftseg_amd/m2f_datapath.py); no kernel draws anything;
 *   - no float atomics anywhere: two runs give the same bits.
 * The formulas are those of torchvision 0.16.2's tensor code paths (environment.yml:369), which the reference's transforms call.
 */
#ifndef MSS_AUG_HIP_H
#define MSS_AUG_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSS_AUG_ABI_VERSION 1
#ifndef MSS_ERR_BAD_ARG
#define MSS_OK 0
#define MSS_ERR_BAD_ARG 1001
#define MSS_ERR_UNSUPPORTED 1002
#endif

/* limits shared by every entry point below ("the common checks", in this order):
 *   1. a NULL pointer that is not marked optional           -> MSS_ERR_BAD_ARG
 *   2. N, H, W (or any other size) <= 0                     -> MSS_ERR_BAD_ARG
 *   3. N > MSS_AUG_MAX_IMAGES or H * W > MSS_AUG_MAX_PIXELS -> MSS_ERR_UNSUPPORTED (grid.z = 3 N, 32-bit pixel indices) */
#define MSS_AUG_MAX_IMAGES 64
#define MSS_AUG_MAX_PIXELS (1 << 28)

int mss_aug_abi_version(void);

/* ---- 1. load: PIL decode -> mixup -> ToTensor (cityscapes.py:157-164, img_utils.py:110-127) -------------------------------------
 * img, gen: uint8 [H, W, 3]; tgt, gen_tgt: uint8 [H, W]. x[0] = img / 255.0f; x[1] = mix / 255.0f with
 * mix = (uint8)(p * img + (1 - p) * gen) in float64, truncated (use_mix != 0), or gen itself (use_mix == 0); m[0] = tgt, m[1] = gen_tgt.
 * Checks: common (N = 2); then p outside [0, 1] with use_mix -> BAD_ARG. */
int mss_aug_load_f32(const uint8_t* img, const uint8_t* gen, const uint8_t* tgt, const uint8_t* gen_tgt, int H, int W, int use_mix,
                     double p, float* x, uint8_t* m, void* stream);

/* ---- 2. stats: what the contrast blend and autocontrast reduce over (torchvision F.adjust_contrast / F.autocontrast, called from
 * img_utils.py:135-139,199-203) ---------------------------------------------------------------------------------------------------
 * stats: float32 [N, 8] = {mean of gray, min r, max r, min g, max g, min b, max b, 0} per image, gray = 0.2989 r + 0.587 g + 0.114 b.
 * Two kernels: partials per workgroup (each thread sums its pixels in a fixed order, in double; a fixed tree inside the workgroup),
 * then one workgroup per image folds the partials in index order. ws: double [N * mss_aug_stats_ws_doubles(H, W)] scratch. */
long long mss_aug_stats_ws_doubles(int H, int W);
int mss_aug_stats_f32(const float* x, int N, int H, int W, double* ws, float* stats, void* stream);

/* ---- 3. point-wise run: ColorJitter's four ops and autocontrast (img_utils.py:135-139,199-203) -----------------------------------
 * Up to MSS_AUG_MAX_OPS ops applied in order to every pixel of x, in place, in ONE pass. blend(a, b, r) = clamp(r a + (1 - r) b, 0, 1).
 *   BRIGHTNESS  blend(x, 0, f)            CONTRAST   blend(x, stats[n][0], f)       SATURATION  blend(x, gray, f)
 *   HUE         rgb -> hsv, h = (h + f) mod 1, hsv -> rgb (torchvision's _rgb2hsv / _hsv2rgb)
 *   AUTOCONTRAST  lo = stats min, scale = 1 / (max - min); where scale is not finite lo = 0, scale = 1; clamp((x - lo) scale, 0, 1)
 * CONTRAST and AUTOCONTRAST read `stats` as mss_aug_stats_f32 wrote it: the caller cuts the run where an op needs statistics of
 * the current state (at most one stats-reading op per run, and only as its FIRST op, unless the caller knows better).
 * 16-byte accesses when H * W is a multiple of 4 (every plane is then 16-byte aligned), scalar accesses otherwise.
 * Checks: common; ops NULL -> BAD_ARG; ops->n outside 1..MSS_AUG_MAX_OPS -> BAD_ARG; an unknown kind -> BAD_ARG; a stats-reading
 * kind with stats NULL -> BAD_ARG. */
#define MSS_AUG_MAX_OPS 8
#define MSS_AUG_OP_BRIGHTNESS 1
#define MSS_AUG_OP_CONTRAST 2
#define MSS_AUG_OP_SATURATION 3
#define MSS_AUG_OP_HUE 4
#define MSS_AUG_OP_AUTOCONTRAST 5
typedef struct MssAugPointOps {
  int n;
  int kind[MSS_AUG_MAX_OPS];
  float factor[MSS_AUG_MAX_OPS];
} MssAugPointOps;
int mss_aug_pointwise_f32(float* x, int N, int H, int W, const MssAugPointOps* ops /* HOST */, const float* stats /* optional */,
                          void* stream);

/* ---- 4. filters: GaussianBlur((9, 9), sigma) and adjust_sharpness (img_utils.py:141-144,189-196) --------------------------------
 * blur: y = depth-wise correlation of x with k9^T k9 under reflect padding of 4 (edge pixel not repeated), evaluated separably
 * (rows, then columns) from an LDS tile with a 4-pixel halo. k9: HOST pointer to the nine normalised float32 weights, passed to the
 * kernel by value. y != x.
 * Checks: common; k9 NULL -> BAD_ARG; x == y -> BAD_ARG; H < 5 or W < 5 -> UNSUPPORTED (reflect padding of 4 needs 5 pixels);
 * H > 65535 * 16 -> UNSUPPORTED. */
int mss_aug_blur9_f32(const float* x, float* y, int N, int H, int W, const float* k9 /* HOST */, void* stream);
/* sharpness: y = blend(x, d, factor); d = x on the one-pixel border and the 3x3 correlation with [[1,1,1],[1,5,1],[1,1,1]] / 13 inside.
 * H <= 2 or W <= 2: y = x (torchvision returns the image unchanged). y != x.
 * Checks: common; x == y -> BAD_ARG; H > 65535 * 16 -> UNSUPPORTED. */
int mss_aug_sharpness_f32(const float* x, float* y, int N, int H, int W, float factor, void* stream);

/* ---- 5. equalize (img_utils.py:205-218 over torchvision F.equalize) -------------------------------------------------------------
 * In place: u = (uint8)(x * 255) by truncation; per image and channel the 256-bin histogram, step = (sum of the nonzero bins except
 * the last nonzero one) / 255; step == 0: lut = identity; else lut[0] = 0, lut[k] = clamp((cumsum[k-1] + step / 2) / step, 0, 255);
 * x = (float)lut[u] / 255.0f. All integer. Three kernels: quantise + histogram (integer LDS atomics flushed with integer global
 * atomics: exact), ONE workgroup that builds the 3 N look-up tables, apply. ws: int32 [N * 3 * 512] (histograms, then tables); the
 * call zeroes the histograms itself.
 * Checks: common; H * W >= 2^31 / 256 is already excluded by MSS_AUG_MAX_PIXELS (the cumulative counts stay below 2^31). */
int mss_aug_equalize_f32(float* x, int N, int H, int W, int* ws, void* stream);

/* ---- 6. warps: RandResize and RandRotate (img_utils.py:233-243,315-323) ---------------------------------------------------------
 * resize: y = bilinear, align_corners = False, no antialias, scale in / out in float32 (F.interpolate's source coordinate: the
 * src_coord of csrc/mss_bilinear.h); mo = nearest, src = min(floor(dst * (float)in / (float)out), in - 1).
 * Checks: common; OH, OW <= 0 -> BAD_ARG; OH * OW > MSS_AUG_MAX_PIXELS or OH > 65535 * 4 -> UNSUPPORTED. */
int mss_aug_resize_f32(const float* x, const uint8_t* m, int N, int H, int W, int OH, int OW, float* y, uint8_t* mo, void* stream);
/* rotate about the centre, same size: theta = [[c, s, 0], [-s, c, 0]] with c = cos(radians(-angle)), s = sin(radians(-angle)) rounded
 * to float32 by the caller; grid gx = (xg c + yg s) / (W / 2), gy = (-xg s + yg c) / (H / 2), xg = i - (W - 1) / 2, yg likewise;
 * grid_sample with align_corners = False and ZERO padding: ix = ((gx + 1) W - 1) / 2. Images bilinear, taps outside contribute 0;
 * label maps nearest (round half to even), outside -> label 0.
 * QUIRK kept on purpose: the reference passes no `fill`, so the corners that rotate in are black in the image and CLASS 0 (not an
 * ignore label) in the label map. This kernel reproduces that.
 * Checks: common; c or s outside [-1, 1] (NaN included) -> BAD_ARG; H > 65535 * 4 -> UNSUPPORTED. */
int mss_aug_rotate_f32(const float* x, const uint8_t* m, int N, int H, int W, float c, float s, float* y, uint8_t* mo, void* stream);

/* ---- 7. window and finish: the flips, RandCrop, Normalize, the COCO paste and the batch layout ----------------------------------
 * window (img_utils.py:246-259,326-337): y[n, c, i, j] = x[n, c, vi, hj] with (i', j') = (top + i, left + j), vi = vflip ? H-1-i' : i',
 * hj = hflip ? W-1-j' : j'; the label maps likewise. Exact copies: a flip alone is top = left = 0, h = H, w = W.
 * Checks: common; h, w <= 0 -> BAD_ARG; top < 0, left < 0, top + h > H or left + w > W -> BAD_ARG; h > 65535 -> UNSUPPORTED. */
int mss_aug_window_f32(const float* x, const uint8_t* m, int N, int H, int W, int hflip, int vflip, int top, int left, int h, int w,
                       float* y, uint8_t* mo, void* stream);
/* finish: window of the N = 2 stack, then Normalize (img_utils.py:147-152: sub float32(mean), div float32(std), separately rounded),
 * then the paste of cityscapes.py:168-169 / img_utils.py:398-435 into the ORIGINAL image and its label map in crop coordinates
 * (object pixels normalised in float64 as img_utils.normalize does, label = the mask's value; the arithmetic of csrc/data.hip), then
 * the trainer's batch layout (train_m2f.py:430-433): image 0 -> out_img[b], out_tgt[b]; image 1 -> out_img[B + b], out_tgt[B + b];
 * labels widened to int64. out_img: float32 [2B, 3, h, w]; out_tgt: int64 [2B, h, w].
 * mean3, std3: HOST pointers to three doubles. geom6: HOST pointer to {y1, x1, bh, bw, h0, w0} (datapath.draw_sample_params), NULL =
 * no paste; obj_img float32 [OH, OW, 3] in 0..255, obj_mask uint8 [OH, OW].
 * Checks: common (N = 2); mean3 / std3 NULL -> BAD_ARG; h, w <= 0, the window outside the image -> BAD_ARG; B <= 0 or b outside
 * 0..B-1 -> BAD_ARG; geom6 with obj_img / obj_mask NULL, OH / OW <= 0, a negative entry, or the object region outside the object
 * (y1 + bh > OH, x1 + bw > OW) -> BAD_ARG; h > 65535 -> UNSUPPORTED. */
int mss_aug_finish_f32(const float* x, const uint8_t* m, int H, int W, int hflip, int vflip, int top, int left, int h, int w,
                       const double* mean3 /* HOST */, const double* std3 /* HOST */, const float* obj_img, const uint8_t* obj_mask,
                       int OH, int OW, const int* geom6 /* HOST, optional */, int B, int b, float* out_img, long long* out_tgt,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
