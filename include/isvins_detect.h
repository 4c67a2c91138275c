/*
 * isvins_detect.h -- C ABI of the batched FEATURE DETECTION: the part of
 *   FeatureTracker::readImage             src/feature_tracker/feature_tracker_simple.cpp:94-107, :126-143
 * that gives birth to tracks, that is FeatureTracker::setMask (:37-69) and
 *   cv::goodFeaturesToTrack(cur_img, n_pts, MAX_CNT - cur_pts.size(), 0.01, MIN_DIST, mask)     (:134)
 * and liftProjective of every new corner (UndistortPixelMotion, :197-208), for many sequences in one call (MI355X).  A detector is
 * bound to a tracker handle (include/isvins_tracker.h): the image it works on is level 0 of a slot's RESIDENT pyramid, which after a
 * successful tracking item is cur_img.  Detection moves no image: it uploads the surviving points and downloads the corners.
 * The first frame of a sequence (prev_img.empty()): seed the slot with a tracking item without points and prev == cur, then detect with n_points = 0.
 *
 * Not here: the fisheye mask and the host bookkeeping (ids, track_cnt++, velocities).  rejectWithF is isvins_reject.h, between the
 * tracking call and this one.  CLAHE is isvins_equalize.h: a
 * slot it wrote holds the equalised cur_img, which is what the reference detects on.
 *
 * The arithmetic is RESTATED from OpenCV 3.2.0 as published (imgproc: featureselect.cpp, corner.cpp, drawing.cpp, thresh.cpp).
 * OpenCV is not available to this project, so the restatement cannot be checked against it.  The CPU restatement
 * tests/native/isv_det_oracle.c pins the GPU, not OpenCV; tests/test_det_oracle.py pins the restatement against independent numpy
 * statements of the definitions below.  Everything is integer arithmetic or a short fixed sequence of IEEE float32 / double
 * operations (contraction off): GPU and restatement agree bit for bit.
 *
 *   setMask     the mask is 255 everywhere.  The points are ordered by track_cnt descending (G1).  In that order a point whose
 *               rounded pixel (cvRound of x and of y, half to even) still reads 255 is KEPT and a filled cv::circle of radius
 *               min_dist around that pixel is set to 0; otherwise the point is dropped.  kept_index lists the kept points' input
 *               indices in this order.
 *   the disc    cv::circle(thickness -1, LINE_8) is the midpoint raster, not a Euclidean test:
 *               err = 0, dx = r, dy = 0, plus = 1, minus = 2 r - 1;  while dx >= dy: fill rows cy - dy and cy + dy over
 *               [cx - dx, cx + dx] and rows cy - dx and cy + dx over [cx - dy, cx + dy], clipped to the image;  dy++, err += plus,
 *               plus += 2;  if err > 0: err -= minus, dx--, minus -= 2.
 *               Every filled interval is centred on cx, so the disc is a half-width per |row - cy|: the largest one any step gives.
 *   response    cornerMinEigenVal(image, eig, 3, 3).  Dx = sum_j [1 2 1][j] (s(x+1, y+j-1) - s(x-1, y+j-1)), Dy likewise with the
 *               axes exchanged: the 3 x 3 Sobel of the 8-bit image with BORDER_REFLECT_101, exact integers.  Sxx, Sxy, Syy: the
 *               unnormalised 3 x 3 box sums of Dx Dx, Dx Dy, Dy Dy; a position of the sum outside the image reflects its index first
 *               (BORDER_REFLECT_101 on the covariance images) and Sobel is taken there.  Exact integers, at most 9 * 1020^2 < 2^24.
 *               With k = (float)(1.0 / (3060.0 * 3060.0)) (3060 = 255 * 4 * 3):
 *               a = (float)Sxx * k * 0.5f,  b = (float)Sxy * k,  c = (float)Syy * k * 0.5f,
 *               eig = (a + c) - sqrt((a - c) * (a - c) + b * b), float32 in this order, the square root through double (G3).
 *   candidates  maxVal = the largest eig over all pixels whose mask is non-zero, border rows and columns included (0 if there is
 *               none);  t = (float)((double)maxVal * quality_level);  v = eig > t ? eig : 0 (THRESH_TOZERO).  A pixel with
 *               1 <= x < W - 1 and 1 <= y < H - 1 is a candidate iff v != 0, v is the maximum of v over its 3 x 3 neighbourhood, and
 *               its mask is non-zero.  A plateau makes every one of its pixels a candidate.
 *   selection   the candidates in descending v (G2); one is accepted iff no accepted corner has dx^2 + dy^2 < min_dist^2 (OpenCV's
 *               cell grid only accelerates this test); stop after max_new acceptances.  A corner is ((float)x, (float)y).
 *               max_new = 0: setMask only (readImage :132 does not call goodFeaturesToTrack then).
 *   the lift    PinholeCamera::liftProjective as in isvins_keyframe.h, with the tracker handle's camera.
 *
 * Deviations (documented, not quirks):
 *   G1  std::sort leaves the order of equal track_cnt open; here ties keep the input order.
 *   G2  3.2.0's comparator leaves equal v to std::sort; here, as in later OpenCV versions, the higher raster index goes first.
 *   G3  OpenCV scales inside a float32 Sobel kernel and accumulates the box sums in float32, in an order that differs between its
 *       scalar and SIMD paths.  Here the sums are the exact integers, scaled once: the result does not depend on the reduction's shape.
 *   G4  maxVal is the maximum in the total order of the float32 encodings (-0 below +0; the response never is -0 or a NaN).
 */
#ifndef ISVINS_DETECT_H
#define ISVINS_DETECT_H

#include <stddef.h>
#include <stdint.h>
#include "isvins_tracker.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISV_DET_BLOCK_SIZE 3      /* cornerMinEigenVal's blockSize: goodFeaturesToTrack's default   */
#define ISV_DET_APERTURE 3        /* its Sobel aperture                                             */
#define ISV_DET_USE_HARRIS 0      /* useHarrisDetector = false                                      */

typedef enum isv_det_status {
    ISV_DET_OK = 0,
    ISV_DET_CAPACITY = 1,         /* n_points > max_points, max_new > max_corners */
    ISV_DET_INPUT = 2             /* a slot outside the tracker's or empty; a negative count; a null array with a non-zero count (the
                                     output arrays included); a non-finite point; a point whose rounded pixel is outside the image (the
                                     reference's mask.at would be out of range; inBorder guarantees otherwise); a slot that another
                                     item of the same call names as well */
} isv_det_status_t;

typedef struct isv_det_config {
    int32_t max_items;            /* items per call, 1 .. 65535                                                   */
    int32_t max_points;           /* surviving points per item (setMask's input), 1 .. 65535                      */
    int32_t max_corners;          /* upper limit of an item's max_new, 1 .. 65535 (reference: MAX_CNT = 150)      */
    int32_t min_dist;             /* MIN_DIST, an integer as in the reference, 1 .. 255 (reference: 30)           */
    double  quality_level;        /* 0.01 in the reference; accepted in (0, 1]                                    */
} isv_det_config_t;

typedef struct isv_det_item {
    int32_t slot;                 /* a slot of the tracker handle; its resident image (level 0) is cur_img        */
    int32_t n_points;             /* cur_pts after the caller's reduceVector (and after rejectWithF: isvins_reject.h) */
    int32_t max_new;              /* MAX_CNT - n_points as the reference computes it; 0: setMask only; < 0 refused */
    int32_t _pad;
    const float   *cur_pts;       /* [n_points][2]                                                                */
    const int32_t *track_cnt;     /* [n_points]                                                                   */
} isv_det_item_t;

typedef struct isv_det_result {
    int32_t status;               /* isv_det_status_t                                                             */
    int32_t n_points;             /* the item's                                                                   */
    int32_t n_kept;               /* points setMask keeps (0 for a refused item, as everything below)             */
    int32_t n_new;                /* corners accepted, at most max_new                                            */
    int32_t n_candidates;         /* pixels that passed threshold, local maximum and mask (0 when max_new is 0)   */
    float   max_val;              /* minMaxLoc's maxVal under the mask (0 if the mask is empty or max_new is 0)   */
} isv_det_result_t;

typedef struct isv_det isv_det_t;

/* A detector on a tracker handle: its slots, its stream, its device, its camera.  ISV_ERR_INVALID_ARG for a null argument, a count
 * or min_dist outside its range above, a quality_level outside (0, 1].  (A tracker handle exists only with a GPU; ISV_ERR_DEVICE
 * when the detector's own events cannot be created.)  Destroy the detector before its tracker. */
int  isv_det_create(isv_trk_t *trk, const isv_det_config_t *cfg, isv_det_t **out);
void isv_det_destroy(isv_det_t *h);
const char *isv_det_last_error(const isv_det_t *h);

/* items[0..n): one packed upload (points only), k_det_mask, k_det_eig, k_det_cand, k_det_select, one download, synchronous on the
 * tracker's stream.  results [n].  The output arrays are [n] pointers each, caller-owned:
 *   kept_index  [n_points]     entries [0, n_kept) are written: input indices in setMask's output order
 *   new_pts     [max_new][2]   entries [0, n_new) are written, in acceptance order
 *   new_un_pts  [max_new][2]   liftProjective of new_pts
 * Every refusal is decided on the host before anything is launched: a refused item changes nothing, and the call returns ISV_OK
 * whenever it ran.  An item's outputs do not depend, bit for bit, on the batch it is in.  Detection never modifies a slot. */
int  isv_det_detect_batch(isv_det_t *h, int32_t n, const isv_det_item_t *const *items, isv_det_result_t *results, int32_t *const *kept_index,
                          float *const *new_pts, float *const *new_un_pts);
/* milliseconds of the last successful call: the whole call (host clock); k_det_eig; k_det_mask; k_det_cand + k_det_select; the
 * upload and the download together (HIP events) */
int  isv_det_last_ms(isv_det_t *h, double out_ms[5]);

#ifdef __cplusplus
}
#endif
#endif /* ISVINS_DETECT_H */
