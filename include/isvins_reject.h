/*
 * isvins_reject.h -- C ABI of the batched OUTLIER REJECTION: the epipolar gate of
 *   FeatureTracker::rejectWithF           src/feature_tracker/feature_tracker_simple.cpp:153-180
 * that is, the lift of prev_pts and cur_pts to a virtual pinhole of focal length FOCAL_LENGTH (:159-171) and
 * cv::findFundamentalMat(un_prev_pts, un_cur_pts, cv::FM_RANSAC, F_THRESHOLD, 0.99, status) (:174), for many sequences in one call
 * (MI355X).  It sits between the tracking call (isvins_tracker.h) and the detection call (isvins_detect.h) of every published frame
 * (:128).  A rejector is bound to a tracker handle for its device, its stream and its camera; it touches no slot and no image.
 *
 * Not here: reduceVector of prev_pts, cur_pts, ids and track_cnt by the status (:175-178) stays with the caller, as the rest of the
 * host bookkeeping does; the fisheye mask.
 *
 * The arithmetic is RESTATED from OpenCV 3.2.0 as published (calib3d: fundam.cpp, ptsetreg.cpp; core: rand.cpp, mathfuncs.cpp) and
 * from PinholeCamera.cc:461-521.  OpenCV is not available to this project, so the restatement cannot be checked against it.  The CPU
 * restatement tests/native/isv_rej_oracle.c pins the GPU, not OpenCV; tests/test_rej_oracle.py pins the restatement against numpy
 * statements of the definitions below and against the Python-integer reading of the RANSAC in tests/relpose_highprec.py.  The serial
 * pieces (the RNG, getSubset, run7Point, solveCubic, computeError, RANSACUpdateNumIters) are those of the relative-pose stage of the
 * initialisation (is-vins_amd/csrc/isv_init_common.h), with their reading; contraction is off on both sides, so the GPU and the
 * restatement can differ only where the device's and the host's pow / acos / cos / log round apart.
 *
 *   gate        n_points < 8: nothing runs, every point is kept (method ISV_REJ_NONE).
 *   the lift    b = PinholeCamera::liftProjective(pt) in doubles (b.z = 1), then, in doubles,
 *               x = focal_length * b.x / b.z + width / 2.0,  y = focal_length * b.y / b.z + height / 2.0,
 *               rounded to float32 (cv::Point2f, J1).  m1 is the prev side, m2 the cur side.
 *   the method  3.2.0's findFundamentalMat runs createRANSACPointSetRegistrator(cb, 7, f_threshold, 0.99) only when n_points >= 15;
 *               with 8 .. 14 points it runs createLMeDSPointSetRegistrator(cb, 7, 0.99), FM_RANSAC or not (J3).
 *   RANSAC      maxIters 1000, a fresh RNG((uint64)-1) (J6), 7 distinct draws per subset, up to three models per subset in root
 *               order.  A model's error per point is computeError's max of the two squared epipolar distances, stored as float32 and
 *               compared with (float)(f_threshold * f_threshold) (J2).  A model is kept when its inlier count is > max(best, 6); then
 *               niters = RANSACUpdateNumIters(0.99, (count - good) / count, 7, niters).  No refit.  status is the kept model's inlier
 *               mask; if no model is kept, every point is rejected (J5).
 *   LMedS       niters = max(RANSACUpdateNumIters(0.99, 0.45, 7, 1000), 3), fixed for the call; the same RNG, subsets and models; a
 *               subset without a model is skipped.  Per model: the count errors as float32, sorted as their 32-bit patterns read as
 *               signed integers (J4);  median = count odd ? e[count / 2] : (e[count / 2 - 1] + e[count / 2]) * 0.5 (a float32 sum,
 *               a double product);  the model is kept when median < minMedian, strictly, from DBL_MAX.  If a model was kept:
 *               sigma = max(2.5 * 1.4826 * (1 + 5. / (count - 7)) * sqrt(minMedian), 0.001) and status is the kept model's inlier mask
 *               at float32 error <= (float)(sigma * sigma); otherwise every point is rejected (J5).
 *
 * Library quirks that are KEPT (marked J1.. in the kernel and the restatement):
 *   J1  the estimator sees float32 points.
 *   J2  the float32 error against the float32 bound.
 *   J3  LMedS below 15 points, although FM_RANSAC was asked for.
 *   J4  the integer sort of the float32 errors: a NaN error with a clear sign bit sorts above +inf (and one with the sign bit set
 *       below everything; which of the two an invalid operation yields is the machine's).
 *   J5  nothing kept: every point is rejected.
 *   J6  the same RNG state on every call: the subsets depend on n_points alone.
 * Deviation (documented, not a quirk):
 *   the null space of the 7-point system comes from the two-sided Jacobi SVD of isv_init_common.h, not from OpenCV's one-sided SVD.
 *   OpenCV's "threshold <= 0 means 3" is refused at creation, not restated.
 */
#ifndef ISVINS_REJECT_H
#define ISVINS_REJECT_H

#include <stddef.h>
#include <stdint.h>
#include "isvins_tracker.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISV_REJ_MIN_POINTS 8      /* prev_pts.size() >= 8 (feature_tracker_simple.cpp:155)                       */
#define ISV_REJ_RANSAC_MIN 15     /* findFundamentalMat: RANSAC from 15 points on, LMedS below                    */
#define ISV_REJ_MAX_POINTS 4096   /* the LDS budget: one float4 per point, 64 KiB of the CU's 160                 */
#define ISV_REJ_FOCAL_LENGTH 460.0/* FOCAL_LENGTH (parameters.h)                                                  */
#define ISV_REJ_F_THRESHOLD 1.0   /* F_THRESHOLD (config/euroc_config.yaml)                                       */

#define ISV_REJ_NONE 0            /* method: fewer than 8 points, nothing ran                                     */
#define ISV_REJ_LMEDS 1
#define ISV_REJ_RANSAC 2

typedef struct isv_rej_config {
    int32_t max_items;            /* items per call, 1 .. 65535                                                   */
    int32_t max_points;           /* points per item, 1 .. min(ISV_REJ_MAX_POINTS, the tracker's max_points)      */
    double  focal_length;         /* FOCAL_LENGTH; finite, > 0                                                    */
    double  f_threshold;          /* F_THRESHOLD, in pixels of the virtual camera; finite, > 0                    */
} isv_rej_config_t;

typedef struct isv_rej_item {
    int32_t width, height;        /* COL, ROW, 1 .. 8192 each: only COL / 2.0 and ROW / 2.0 are read              */
    int32_t n_points;
    int32_t _pad;
    const float *prev_pts;        /* [n_points][2]: pixel coordinates, after the caller's reduceVector            */
    const float *cur_pts;         /* [n_points][2]                                                                */
} isv_rej_item_t;

typedef struct isv_rej_result {
    int32_t status;               /* isv_trk_status_t                                                             */
    int32_t n_points;             /* the item's                                                                   */
    int32_t n_kept;               /* entries of the status array that are 1 (0 for a refused item)                */
    int32_t method;               /* ISV_REJ_NONE / ISV_REJ_LMEDS / ISV_REJ_RANSAC                                */
    int32_t iters;                /* the RANSAC iterations run, or the LMedS niters; 0 for ISV_REJ_NONE           */
    int32_t best_inliers;         /* the kept model's inlier count; 0 when none was kept                          */
    double  min_median;           /* the LMedS minMedian; -1 when the method is not LMedS or nothing was kept     */
} isv_rej_result_t;

typedef struct isv_rej isv_rej_t;

/* A rejector on a tracker handle: its device, its stream, its camera (the intrinsics and the distortion of its configuration).
 * ISV_ERR_INVALID_ARG for a null argument, a max_items or max_points outside its range above, a focal_length or f_threshold that is
 * not finite or not positive.  (A tracker handle exists only with a GPU.)  Destroy the rejector before its tracker. */
int  isv_rej_create(isv_trk_t *trk, const isv_rej_config_t *cfg, isv_rej_t **out);
void isv_rej_destroy(isv_rej_t *h);
const char *isv_rej_last_error(const isv_rej_t *h);

/* items[0..n), n at most max_items (ISV_ERR_CAPACITY beyond, before anything is enqueued): one packed upload, k_rej_f, one download,
 * synchronous on the tracker's stream.  results [n].  status: [n] pointers, caller-owned, status[i] is [n_points] of 1 (kept) / 0.
 * An item is refused by its result's status, never truncated: ISV_TRK_CAPACITY for n_points > max_points; ISV_TRK_INPUT for a width
 * or height below 1 or above 8192, a negative count, a null array (prev_pts, cur_pts or status[i]) with n_points > 0, a non-finite
 * coordinate.  A refused item writes nothing into its array.  An item's outputs do not depend, bit for bit, on the batch it is in.
 * The call returns ISV_OK whenever it ran. */
int  isv_rej_reject_batch(isv_rej_t *h, int32_t n, const isv_rej_item_t *const *items, isv_rej_result_t *results, uint8_t *const *status);

/* milliseconds of the last successful call: the whole call (host clock), k_rej_f, the upload of the packed block (HIP events), the
 * packing of that block on the host (host clock) */
int  isv_rej_last_ms(isv_rej_t *h, double out_ms[4]);

#ifdef __cplusplus
}
#endif
#endif /* ISVINS_REJECT_H */
