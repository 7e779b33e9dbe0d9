/* C ABI of libmss_obj.so: the resident COCO-object bank of the anomaly mix, on an MI355X (gfx950).
 *
 * The reference picks a COCO object per sample, rescales it on the host with cv2.resize (lib/utils/img_utils.py:345-352:
 * INTER_LINEAR for the float32 image, INTER_NEAREST for the mask) and cuts it to the bounding box of its valid mask pixels
 * (extract_bboxes, :379-394; a pixel is valid when its mask byte is neither 0 nor 255, :400). Here the decoded objects live in two
 * flat device buffers, uploaded once,
 *
 *     bank_img   uint8 [bank_pixels, 3]     object k occupies the pixels [off_k, off_k + H_k W_k), row-major H_k x W_k
 *     bank_mask  uint8 [bank_pixels]        likewise
 *
 * and two kernels do the rest: the bounding box of every (object, scaled size) once, and per step ONE launch that writes the rescaled
 * and cut objects of a whole batch into the buffers the paste kernels read (mss_data_pair_f32, mss_aug_finish_f32).
 * The arithmetic is that of csrc/mss_cv_resize.h (coordinates, in double) and, for the image, one fixed sequence of float32
 * operations without fused multiply-adds: horizontal pass h = fl(fl(S0 a0) + fl(S1 a1)), then dst = fl(fl(h0 b0) + fl(h1 b1)),
 * a1 = f, a0 = 1.0f - f. DESIGN.md 3.33.
 *
 * It is separate from libmss_hip.so (include/mss_hip.h, closed at 142 entry points), libmss_aug.so (include/mss_aug_hip.h, closed
 * at 12) and libmss_ood.so (include/mss_ood_hip.h, closed at 5), shares no symbol with them and needs none of theirs.
 *
 * Conventions (those of mss_hip.h):
 *   - every pointer is a device pointer;
 *   - a status-returning function returns int and ends in `void* stream` (a hipStream_t, NULL = the default stream):
 *     0 = launched, MSS_ERR_BAD_ARG / MSS_ERR_UNSUPPORTED = refused, anything else = a hipError_t;
 *   - the scalar arguments are checked BEFORE any HIP call, in the order "the common checks" lists, so a refused call touches no
 *     device. The job tables live on the device and are checked there: a job that names pixels outside the bank, a window outside
 *     its rescaled object or outside its output slot, or a size < 1, reads and writes NOTHING (its box is four zeros);
 *   - no float atomics, no memset, no device-to-host copy, integer min / max reductions only: two runs give the same bits.
 */
#ifndef MSS_OBJ_HIP_H
#define MSS_OBJ_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSS_OBJ_ABI_VERSION 1
#ifndef MSS_ERR_BAD_ARG
#define MSS_OK 0
#define MSS_ERR_BAD_ARG 1001
#define MSS_ERR_UNSUPPORTED 1002
#endif

/* the common checks, in this order:
 *   1. a NULL pointer                                                                   -> MSS_ERR_BAD_ARG
 *   2. bank_pixels, n / B, OHmax or OWmax < 1                                           -> MSS_ERR_BAD_ARG
 *   3. bank_pixels > MSS_OBJ_MAX_PIXELS, n > MSS_OBJ_MAX_BBOX_JOBS, B > MSS_OBJ_MAX_BATCH,
 *      OHmax > MSS_OBJ_MAX_ROWS, B OHmax OWmax > MSS_OBJ_MAX_PIXELS                     -> MSS_ERR_UNSUPPORTED
 *      (32-bit pixel indices, the limits of the launch grid) */
#define MSS_OBJ_MAX_PIXELS 0x7fffffffll
#define MSS_OBJ_MAX_BBOX_JOBS 0x1000000
#define MSS_OBJ_MAX_BATCH 65535
#define MSS_OBJ_MAX_ROWS 0xffff0
#define MSS_OBJ_BBOX_JOB_INTS 5
#define MSS_OBJ_RESCALE_JOB_INTS 9

int mss_obj_abi_version(void);

/* Bounding boxes. jobs int32 [n, 5] = (off, H, W, sh, sw): the object at pixel offset off of the bank, H x W, nearest-resized to
 * sh x sw. boxes int32 [n, 4] = (y1, x1, y2, x2), written whole: the first and one past the last row and column of the resized mask
 * that hold a valid pixel (byte neither 0 nor 255), four zeros when there is none or when the job is refused on the device
 * (off < 0, H, W, sh or sw < 1, off + H W > bank_pixels, sh sw > MSS_OBJ_MAX_PIXELS). One workgroup per job. Checks: common 1-3. */
int mss_obj_bbox_u8(const uint8_t* bank_mask, long long bank_pixels, const int* jobs, int n, int* boxes, void* stream);

/* The rescaled and cut objects of a batch. jobs int32 [B, 9] = (off, H, W, sh, sw, y1, x1, bh, bw): the window
 * [y1, y1 + bh) x [x1, x1 + bw) of the object resized to sh x sw goes to the ORIGIN of slot b:
 *   out_img   float32 [B, OHmax, OWmax, 3]   out_img[b, r, c, :] = linear-resized image at (y1 + r, x1 + c), values 0..255
 *   out_mask  uint8   [B, OHmax, OWmax]      out_mask[b, r, c]   = nearest-resized mask at (y1 + r, x1 + c)
 * for r < bh, c < bw. Exactly these windows are written and nothing else; a job with bh == 0 or bw == 0 writes nothing, and so does
 * a job refused on the device (as for mss_obj_bbox_u8, or y1, x1, bh, bw < 0, y1 + bh > sh, x1 + bw > sw, bh > OHmax, bw > OWmax).
 * One launch: grid (tiles of OWmax, tiles of OHmax, B), a workgroup outside its sample's window leaves at once. Checks: common 1-3. */
int mss_obj_rescale_f32(const uint8_t* bank_img, const uint8_t* bank_mask, long long bank_pixels, const int* jobs, int B, int OHmax,
                        int OWmax, float* out_img, uint8_t* out_mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif
