/*
 * isvins_tracker.h -- C ABI of the batched FEATURE TRACKING: the per-image, per-sequence part of
 *   FeatureTracker::readImage             src/feature_tracker/feature_tracker_simple.cpp:81-151
 * that is, cv::calcOpticalFlowPyrLK(prev_img, cur_img, prev_pts, cur_pts, status, err, cv::Size(21, 21), 3) (:114), inBorder of every
 * tracked point (:6-12, :116-118) and liftProjective of every tracked point (UndistortPixelMotion, :197-208), for many sequences in
 * one call (MI355X).  A sequence's tracker state, the image pyramid of its last `cur` image, stays on the device in a SLOT: the steady
 * state uploads one image and builds one pyramid per frame.
 *
 * Not here: setMask and goodFeaturesToTrack are isvins_detect.h and CLAHE is isvins_equalize.h, both on this handle's slots;
 * rejectWithF is isvins_reject.h, on this handle's device, stream and camera; the bookkeeping, that is the compaction
 * (reduceVector), track_cnt++, ids and the velocity map, stays with the caller of these stage calls -- or is isvins_frontend.h,
 * which runs all of readImage in one call with the state on the device.
 *
 * The arithmetic is RESTATED from OpenCV 3.2.0 as published (video: lkpyramid.cpp; imgproc: pyramids.cpp; core: copy.cpp) and from
 * PinholeCamera.cc:461-521, :657-673.  OpenCV is not available to this project, so the restatement cannot be checked against it.  The
 * CPU restatement tests/native/isv_trk_oracle.c pins the GPU, not OpenCV; tests/test_trk_oracle.py pins the restatement against
 * independent numpy statements of the definitions and against known translations of an analytic texture.  Everything is integer
 * arithmetic or a short fixed sequence of IEEE float32 / double operations (contraction off): GPU and restatement agree bit for bit.
 *
 *   pyramid     level 0 is the image; level l + 1 has size ((w + 1) / 2, (h + 1) / 2) and exists iff l < 3 and both of its dimensions
 *               exceed 21.  pyrDown on 8-bit: dst(x, y) = (sum_jk K[j] K[k] src(2 x + k - 2, 2 y + j - 2) + 128) >> 8 with
 *               K = [1 4 6 4 1], both passes in integers, BORDER_REFLECT_101 (... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...; an axis of length
 *               1 repeats its pixel).  A pixel read outside a level, at most 22 pixels outside, goes through BORDER_REFLECT_101 by the
 *               general loop (the padded pyramid of buildOpticalFlowPyramid), so that any size is safe.
 *   derivatives calcSharrDeriv in int16, with its own reflect-101 at the level's edges:
 *               t0 = 3 (s[y-1] + s[y+1]) + 10 s[y],  t1 = s[y+1] - s[y-1],  Ix = t0[x+1] - t0[x-1],  Iy = 3 (t1[x-1] + t1[x+1]) + 10 t1[x];
 *               outside the level both are 0 (BORDER_CONSTANT).
 *   per point   from the top level L down to 0, with status = 1 and err = 0 at the start:
 *               p = prev_pt * 2^-l;  q = p at the top level, else 2 q_out;  q_out = q before anything can fail;
 *               p -= (10, 10), ip = floor(p); the RANGE TEST: ip.x < -21 || ip.x >= W_l || ip.y < -21 || ip.y >= H_l fails the level.
 *               With a, b the fractions of p: iw00 = cvRound((1-a)(1-b) 16384), iw01 = cvRound(a (1-b) 16384),
 *               iw10 = cvRound((1-a) b 16384), iw11 = 16384 - iw00 - iw01 - iw10 (float32 products, left to right; half to even).
 *               Over the 21 x 21 window, DESCALE(v, n) = (v + (1 << (n-1))) >> n:  I = DESCALE(bilinear of the image, 9),
 *               dIx, dIy = DESCALE(bilinear of the derivative, 14);  S11 = sum dIx^2, S12 = sum dIx dIy, S22 = sum dIy^2 as exact
 *               64-bit integers;  A = (float)S * 2^-20;  D = A11 A22 - A12 A12;
 *               minEig = (A22 + A11 - sqrt((A11 - A22)^2 + 4 A12^2)) / 882 in float32 in this order;
 *               minEig < 1e-4 (as double) or D < FLT_EPSILON fails the level.  D = 1 / D, q -= (10, 10), prevDelta = 0.
 *               For j = 0 .. 29: iq = floor(q); the range test on iq (on failure: at level 0 status = 0; break); the weights from q;
 *               diff = DESCALE(bilinear of J, 9) - I;  T1 = sum diff dIx, T2 = sum diff dIy, exact integers;  b = (float)T * 2^-20;
 *               delta = ((A12 b2 - A22 b1) D, (A12 b1 - A11 b2) D);  q += delta;  q_out = q + (10, 10);
 *               break if (double)dx dx + (double)dy dy <= 0.01 * 0.01 (the double product);
 *               if j > 0 && |dx + prevDx| < 0.01 && |dy + prevDy| < 0.01 (float32 sums against the double 0.01): q_out -= 0.5 delta; break;
 *               prevDelta = delta.
 *               A failed level: at level 0 status = 0; then the next level.
 *               At level 0 with status still 1: the window of J again at q_out - (10, 10); if its range test fails status = 0,
 *               otherwise err = (float)(sum |diff|) / 14112.
 *   inBorder    x = cvRound(cur_pt.x), y = cvRound(cur_pt.y), half to even: 1 <= x < width - 1 && 1 <= y < height - 1.
 *   the lift    PinholeCamera::liftProjective as in isvins_keyframe.h: cur_un_pts = ((float)(b.x / b.z), (float)(b.y / b.z)), b.z = 1.
 *
 * Reference quirks that are KEPT (marked T1.. in the kernels and the restatement):
 *   T1  a level that fails above level 0 is no failure: the level is skipped, the guess is doubled and the point can end with status 1.
 *   T2  the err pass can clear status, although the reference never reads err.
 *   T3  two successive steps that cancel each other end the iteration half a step back.
 *   T4  the window may hang up to 21 pixels outside the image; there it reads reflected pixels but zero derivatives.
 * Deviations (documented, not quirks):
 *   D1  OpenCV's scalar path accumulates the five sums in float32 in raster order, its SIMD paths in other orders.  Here the sums are
 *       the exact integers, rounded to float32 once: the result does not depend on the shape of the reduction.  (sum |diff| is below
 *       2^24, so err is exact in every order.)
 *   D2  floor / cvRound of a float32 outside the range of int is undefined in C; here such a coordinate counts as out of range (it
 *       fails the range test and is not in the border).
 */
#ifndef ISVINS_TRACKER_H
#define ISVINS_TRACKER_H

#include <stddef.h>
#include <stdint.h>
#include "isvins_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISV_TRK_WIN 21            /* cv::Size(21, 21) (feature_tracker_simple.cpp:114) */
#define ISV_TRK_MAX_LEVEL 3       /* maxLevel: at most 4 pyramid levels                */
#define ISV_TRK_MAX_ITER 30       /* TermCriteria(COUNT + EPS, 30, 0.01), the default  */

typedef enum isv_trk_status {
    ISV_TRK_OK = 0,
    ISV_TRK_CAPACITY = 1,         /* width > max_width, height > max_height, n_points > max_points */
    ISV_TRK_INPUT = 2             /* sizes below 1, a negative count, stride < width, a slot outside [0, max_slots), a null array with a
                                     non-zero size, a non-finite point; prev == NULL on an empty slot or on a slot whose resident image
                                     has another size or was written by an equaliser (isvins_equalize.h); a slot that another item of
                                     the same call names as well */
} isv_trk_status_t;

#define ISV_TRK_FLAG_STATUS 1     /* bit 0 of flags: calcOpticalFlowPyrLK's status */
#define ISV_TRK_FLAG_BORDER 2     /* bit 1 of flags: inBorder(cur_pts[i])          */

typedef struct isv_trk_config {
    int32_t max_slots;            /* sequences with resident state, at most 65536                                 */
    int32_t max_items;            /* items per call, at most 65535                                                */
    int32_t max_width, max_height;/* at most 8192 each                                                            */
    int32_t max_points;           /* points per item, at most 65535                                               */
    int32_t win;                  /* ISV_TRK_WIN: nothing else is accepted                                        */
    int32_t max_level;            /* ISV_TRK_MAX_LEVEL: nothing else is accepted                                  */
    int32_t _pad;
    double  fx, fy, cx, cy;       /* the pinhole model's projection_parameters                                    */
    double  k1, k2, p1, p2;       /* its distortion_parameters                                                    */
} isv_trk_config_t;

typedef struct isv_trk_item {
    int32_t slot;                 /* the sequence's slot                                                          */
    int32_t width, height, stride;/* of cur and of prev alike; stride in bytes between rows, at least width       */
    int32_t n_points;
    int32_t _pad;
    const uint8_t *cur;           /* [height][stride], 8-bit grey: cur_img                                        */
    const uint8_t *prev;          /* [height][stride]: prev_img, or NULL: the slot's resident image is prev_img   */
    const float   *prev_pts;      /* [n_points][2]: pixel coordinates in prev_img                                 */
} isv_trk_item_t;

typedef struct isv_trk_result {
    int32_t status;               /* isv_trk_status_t                                                             */
    int32_t n_points;             /* the item's                                                                   */
    int32_t n_kept;               /* points with both flag bits set (0 for a refused item)                        */
    int32_t n_levels;             /* pyramid levels used, 1 .. 4 (0 for a refused item)                           */
} isv_trk_result_t;

typedef struct isv_trk isv_trk_t;

/* Fails with ISV_ERR_DEVICE without a GPU: there is no CPU path.  ISV_ERR_INVALID_ARG for a non-positive size or count, one beyond its
 * limit above, win != 21, max_level != 3, a non-positive focal length, non-finite intrinsics.  All slots start empty; their pyramids
 * (two per slot: the resident one and the one being built) are allocated here. */
int  isv_trk_create(const isv_trk_config_t *cfg, isv_trk_t **out);
void isv_trk_destroy(isv_trk_t *h);
const char *isv_trk_last_error(const isv_trk_t *h);

/* items[0..n): one packed upload (the images are the bulk), the pyramid kernels, k_trk_track, one download, synchronous on the
 * handle's own stream.  results [n].  The output arrays are [n] pointers each, caller-owned, [n_points] entries per item:
 *   cur_pts     [n_points][2]  cur_pts, also where status is 0 (the last estimate, as calcOpticalFlowPyrLK leaves it)
 *   flags       [n_points]     bit 0 status, bit 1 inBorder(cur_pts[i]); the reference keeps a point iff both are set
 *   err         [n_points]     err (0 where status is 0)
 *   cur_un_pts  [n_points][2]  the lifted cur_pts where bit 0 is set, 0 otherwise
 * After a successful item its slot holds cur's pyramid.  An item that cannot be tracked is refused by its status, never truncated: a
 * refused item changes nothing, neither its arrays nor its slot; the call returns ISV_OK whenever it ran.  An item's outputs do not
 * depend, bit for bit, on the batch it is in, nor on whether prev was uploaded or resident.  If the call itself fails on the device,
 * the slots of its items are empty afterwards. */
int  isv_trk_track_batch(isv_trk_t *h, int32_t n, const isv_trk_item_t *const *items, isv_trk_result_t *results, float *const *cur_pts,
                         uint8_t *const *flags, float *const *err, float *const *cur_un_pts);
/* milliseconds of the last successful call: the whole call (host clock), the pyramid kernels, k_trk_track, the upload of the packed
 * block (HIP events), the packing of that block on the host (host clock) */
int  isv_trk_last_ms(isv_trk_t *h, double out_ms[5]);
/* empties a slot: its next item has to bring prev.  ISV_ERR_INVALID_ARG for a slot outside [0, max_slots). */
int  isv_trk_slot_reset(isv_trk_t *h, int32_t slot);

#ifdef __cplusplus
}
#endif
#endif /* ISVINS_TRACKER_H */
