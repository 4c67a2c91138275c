/*
 * isvins_equalize.h -- C ABI of the batched CLAHE: the first line of
 *   FeatureTracker::readImage             src/feature_tracker/feature_tracker_simple.cpp:86-92
 * that is, cv::createCLAHE(3.0, cv::Size(8, 8))->apply(_img, img) with EQUALIZE set (config/euroc_config.yaml:45, the reference's only
 * shipped configuration), for many sequences in one call (MI355X).  Everything behind that line -- the optical flow, the corner
 * detection, prev_img of the next frame -- reads the equalised image.  An equaliser is bound to a tracker handle
 * (include/isvins_tracker.h): isv_eq_track_batch is isv_trk_track_batch with every uploaded image equalised on the device before it
 * becomes level 0 of its slot's pyramid, so the steady state still uploads one raw image per frame and the feature detection
 * (isvins_detect.h), which reads level 0 of the resident pyramid, sees the equalised cur_img as in the reference (:104, :140).
 * isv_eq_apply_batch runs the same kernels on images that touch no slot and returns the equalised images.
 *
 * Not here: rejectWithF is isvins_reject.h; the host bookkeeping stays with the caller.
 *
 * The arithmetic is RESTATED from OpenCV 3.2.0 as published (imgproc: clahe.cpp, the 8-bit path; core: copy.cpp).  OpenCV is not
 * available to this project, so the restatement cannot be checked against it.  The CPU restatement tests/native/isv_eq_oracle.c pins
 * the GPU, not OpenCV; tests/test_eq_oracle.py pins the restatement against an independent numpy statement of the definitions below.
 * Everything is integer arithmetic or a short fixed sequence of IEEE float32 / double operations (contraction off): GPU and
 * restatement agree bit for bit.
 *
 *   tile grid   if W % tiles_x == 0 && H % tiles_y == 0 the tile is (tw, th) = (W / tiles_x, H / tiles_y) over the image.  Otherwise
 *               the image is extended on the right by tiles_x - W % tiles_x and at the bottom by tiles_y - H % tiles_y (K1: an axis
 *               that divides evenly is extended by a whole tiles_x / tiles_y then) with BORDER_REFLECT_101 (... 2 1 | 0 1 2 ... n-1 |
 *               n-2 n-3 ..., the general loop: an extension longer than the axis reflects again; an axis of length 1 repeats its
 *               pixel), and the tile is the extended size divided by the grid.  The extension only feeds the histograms.
 *               area = tw * th;  lutScale = (float)255 / area in float32;
 *               clip = clip_limit > 0 ? max((int)(clip_limit * area / 256), 1) : 0, the product and the quotient in double.
 *   per tile    the histogram of its tw x th pixels, 256 integer bins.  If clip > 0: every bin is capped at clip and the excess summed
 *               into `clipped`;  batch = clipped / 256, residual = clipped - 256 * batch;  every bin += batch;  if residual != 0:
 *               step = max(256 / residual, 1) and for (i = 0; i < 256 && residual > 0; i += step, residual--) bin[i]++  (E1).
 *               Then sum += bin[i], lut[i] = saturate_u8(cvRound((float)sum * lutScale)): int to float32 rounded to nearest, a
 *               float32 product, cvRound half to even.
 *   per pixel   (x, y) of the original image, v its value:  inv_tw = 1.0f / tw,  txf = x * inv_tw - 0.5f (E2),  tx1 = floor(txf),
 *               tx2 = tx1 + 1,  xa = txf - tx1,  xa1 = 1.0f - xa;  then tx1 = max(tx1, 0), tx2 = min(tx2, tiles_x - 1);  the same in y
 *               with th.  With L[ty][tx] the tile's lut:
 *               res = (L[ty1][tx1][v] * xa1 + L[ty1][tx2][v] * xa) * ya1 + (L[ty2][tx1][v] * xa1 + L[ty2][tx2][v] * xa) * ya,
 *               all float32 in this order;  dst = saturate_u8(cvRound(res)).
 *
 * Library quirk that is KEPT (marked K1 in the kernels and the restatement):
 *   K1  as soon as one axis does not divide, both are extended: the axis that divides gets a whole extra tiles_x / tiles_y.
 * Where published OpenCV versions differ (marked E1, E2 in the kernels and the restatement, for a reader with OpenCV at hand):
 *   E1  how the residual is spread: 3.2.0 steps through the bins as above, older releases increment the first `residual` bins.
 *   E2  x * inv_tw as above against x / tw.
 * Deviation (documented, not a quirk):
 *   E3  (int) of a double beyond int's range is undefined in C; a bin never exceeds area, so clip is taken from
 *       min(clip_limit * area / 256, area): the same lut for every value the cast is defined for.
 */
#ifndef ISVINS_EQUALIZE_H
#define ISVINS_EQUALIZE_H

#include <stddef.h>
#include <stdint.h>
#include "isvins_tracker.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISV_EQ_CLIP 3.0           /* cv::createCLAHE(3.0, cv::Size(8, 8)) (feature_tracker_simple.cpp:88) */
#define ISV_EQ_TILES 8
#define ISV_EQ_MAX_TILES 32       /* per axis */

typedef struct isv_eq_config {
    double  clip_limit;           /* finite, >= 0; 0: no clipping, as in OpenCV                                   */
    int32_t tiles_x, tiles_y;     /* the tile grid, 1 .. 32 each                                                  */
    int32_t max_items;            /* items per call, 1 .. 65535                                                   */
    int32_t _pad;
} isv_eq_config_t;

typedef struct isv_eq_image {
    int32_t width, height, stride;/* stride in bytes between rows, at least width                                 */
    int32_t _pad;
    const uint8_t *data;          /* [height][stride], 8-bit grey                                                 */
} isv_eq_image_t;

typedef struct isv_eq isv_eq_t;

/* An equaliser on a tracker handle: its slots, its stream, its device, its size limits.  ISV_ERR_INVALID_ARG for a null argument,
 * a clip_limit that is negative or not finite, a grid or max_items outside its range above.  (A tracker handle exists only with a
 * GPU.)  Destroy the equaliser before its tracker. */
int  isv_eq_create(isv_trk_t *trk, const isv_eq_config_t *cfg, isv_eq_t **out);
void isv_eq_destroy(isv_eq_t *h);
const char *isv_eq_last_error(const isv_eq_t *h);

/* isv_trk_track_batch on the equaliser's tracker, its contract word for word (items, results, the output arrays, the refusals, batch
 * independence, n at most the tracker's max_items), with one difference: every image the call uploads (cur, and prev where given)
 * is equalised on the device before it becomes level 0 of its slot buffer.  A slot remembers who wrote its resident image: an item
 * with prev == NULL is refused with ISV_TRK_INPUT on a slot whose resident image was not written by this equaliser, and
 * isv_trk_track_batch refuses an item with prev == NULL on a slot an equaliser wrote (the same class as "resident image has another
 * size").  Errors and times of the call are the equaliser's (isv_eq_last_error, isv_eq_last_ms). */
int  isv_eq_track_batch(isv_eq_t *h, int32_t n, const isv_trk_item_t *const *items, isv_trk_result_t *results, float *const *cur_pts,
                        uint8_t *const *flags, float *const *err, float *const *cur_un_pts);

/* items[0..n), n at most max_items: one packed upload, the CLAHE kernels, one download, synchronous on the tracker's stream; no slot
 * is read or written.  status [n]: isv_trk_status_t, ISV_TRK_INPUT for a size below 1, stride < width or null data (or a null
 * out[i]), ISV_TRK_CAPACITY for a size beyond the tracker's max_width / max_height.  out [n] pointers, caller-owned: out[i] is
 * [height][width], packed; a refused item's is left untouched.  The call returns ISV_OK whenever it ran. */
int  isv_eq_apply_batch(isv_eq_t *h, int32_t n, const isv_eq_image_t *const *items, int32_t *status, uint8_t *const *out);

/* milliseconds of the last successful call: the whole call (host clock), the CLAHE kernels, the pyramid kernels, k_trk_track, the
 * upload of the packed block (HIP events), the packing of that block on the host (host clock); the third and fourth are 0 after
 * isv_eq_apply_batch */
int  isv_eq_last_ms(isv_eq_t *h, double out_ms[6]);

#ifdef __cplusplus
}
#endif
#endif /* ISVINS_EQUALIZE_H */
