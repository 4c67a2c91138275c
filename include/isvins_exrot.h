/*
 * isvins_exrot.h -- C ABI of the batched CAMERA-IMU ROTATION CALIBRATION (estimate_extrinsic: 2):
 *   InitialEXRotation::CalibrationExRotation, solveRelativeR, testTriangulation, decomposeE
 *                                          src/initial/initial_ex_rotation.cpp:1-141
 * as Estimator::processImage calls it on every frame from the second on until it succeeds (src/estimator.cpp:139-153), for many
 * sequences in one call (MI355X).  A calibrator is a handle of its own, with its own stream.  A sequence's calibration state lives in
 * a SLOT on the device: frame_count, ric and, per recorded frame i = 1 .. frame_count, the three matrices Rc[i], Rimu[i], Rc_g[i]
 * (27 doubles, row-major, in that order).  Nothing of it crosses to the host in the steady state.
 *
 * How a caller uses it: estimate_extrinsic = 2 with RIC = I means "calibrate, then go on as estimate_extrinsic = 1"
 * (estimator.cpp:150 sets ESTIMATE_EXTRINSIC = 1 at the moment of success).  So: one item per frame per sequence until a result says
 * `calibrated`; then create the solve handle with estimate_extrinsic = 1 and the result's ric.  The solve handle itself keeps refusing
 * the value 2.
 *
 * The arithmetic is RESTATED from OpenCV 3.2.0 as published (calib3d: fundam.cpp, ptsetreg.cpp, triangulate.cpp; core: rand.cpp,
 * matmul.cpp, matop.cpp) and from Eigen 3.3 (Quaternion.h, Inverse_impl.h, JacobiSVD.h).  Neither is available to this project, so the
 * restatement cannot be checked against them; the CPU restatement tests/native/isv_exr_oracle.c pins the GPU, tests/test_exr_oracle.py
 * pins the restatement against numpy statements, tests/exr_highprec.py against a 40-digit reading of the definitions.  The serial
 * pieces are shared text (is-vins_amd/csrc/isv_exrot.h, isv_init_common.h), contraction off on both sides: the GPU and the restatement
 * can differ only where the device's and the host's pow / acos / cos / log / atan2 round apart.
 *
 * One call of CalibrationExRotation, per item (quirks X1.. are KEPT and marked in the kernel and the restatement):
 *   X1  the correspondences are rounded to float32 (cv::Point2f) before anything reads them (:75-76).
 *   X2  cv::findFundamentalMat(ll, rr) is FM_RANSAC, 3.0, 0.99; in 3.2.0 that is RANSAC from 15 points on and LMedS for 9 .. 14.
 *       maxIters 1000, a fresh RNG((uint64)-1), float32 errors against (float)(3.0 * 3.0), no refit.  The points are normalised
 *       coordinates, so as a rule the first subset that yields a model keeps every point and niters falls to 0.  Reproduced.
 *   X3  decomposeE: R1 = U W Vt, R2 = U Wt Vt with W = [0 -1 0; 1 0 0; 0 0 1], t1 = u3, t2 = -u3, no sign fixes;
 *       if (det(R1) + 1.0 < 1e-9) E = -E and again (`negated`).
 *   X4  testTriangulation: P1 = [R | t] rounded to float32 (cv::Matx34f); cv::triangulatePoints builds its 6 x 4 system in doubles
 *       from the float32 values, the homogeneous point is stored as float32 (X Y Z W); with alpha = 1.0 / (double)W the depth in a
 *       camera P is (float)((P20 X + P21 Y + P22 Z + P23 W) * alpha), the sum in doubles from 0 in that order (the reading taken of
 *       pointcloud.col(i) / normal_factor as a scaled expression and of the float32 gemm with double accumulators: restated from the
 *       3.2.0 sources, not checked).  front counts the points with both depths > 0.  ratio = 1.0 * front / n;
 *       ratio1 = max over (R1,t1), (R1,t2); ratio2 = max over (R2,t1), (R2,t2); ratio1 > ratio2 ? R1 : R2 (a tie gives R2);
 *       Rc is the TRANSPOSE of the chosen matrix (:92-94).
 *   X5  fewer than 9 correspondences: Rc = I, and the frame still counts (:70, :97).
 *   X6  Rc_g = ric.inverse() * delta_q * ric with the ric from BEFORE this call; the 3 x 3 inverse by cofactors; delta_q is used as
 *       given, not normalised.  The Rc_g of earlier frames are not recomputed.
 *   X7  per frame i = 1 .. F: the matrix-to-quaternion conversion of Rc[i], Rc_g[i], Rimu[i];
 *       angle = 180 / M_PI * 2 * atan2(|d.vec|, |d.w|), d = r1 * r2.conjugate(); huber = angle > 5 ? 5 / angle : 1;
 *       rows 4(i-1) .. 4(i-1)+3 of A are huber * (L(Rc[i]) - R(Rimu[i])).
 *   X8  the right singular vector of A's smallest singular value, x = (x, y, z, w); ric = toRotationMatrix(x).inverse(), x not
 *       renormalised; calibrated = frame_count >= vo_size && singular[2] > 0.25.
 * Deviations (documented, not quirks):
 *   the SVDs: the 3 x 3 of decomposeE and the 7-point null space come from the two-sided Jacobi SVD of isv_init_common.h, not from
 *   cv::SVD; the triangulation's and A's right singular vectors from a Householder QR (column by column, no pivoting) and that Jacobi
 *   SVD of the 4 x 4 factor, where Eigen preconditions with a column-pivoted QR.  Singular values and the last right singular vector
 *   agree mathematically up to the vector's sign, which does not change the rotation.
 *   ISV_EXR_NO_MODEL: the estimator kept no model.  The reference would abort inside cv::SVD on the empty matrix.
 */
#ifndef ISVINS_EXROT_H
#define ISVINS_EXROT_H

#include <stddef.h>
#include <stdint.h>
#include "isvins_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISV_EXR_MIN_CORRES 9      /* corres.size() >= 9 (initial_ex_rotation.cpp:70)                              */
#define ISV_EXR_RANSAC_MIN 15     /* findFundamentalMat: RANSAC from 15 points on, LMedS below                    */
#define ISV_EXR_MAX_CORRES 4096   /* the LDS budget: one float4 per correspondence, 64 KiB of the CU's 160        */
#define ISV_EXR_MAX_FRAMES 1024
#define ISV_EXR_VO_SIZE 8         /* Vo_SIZE (initial_ex_rotation.h)                                              */

#define ISV_EXR_NONE 0            /* method: fewer than 9 correspondences, nothing ran                            */
#define ISV_EXR_LMEDS 1
#define ISV_EXR_RANSAC 2

typedef enum isv_exr_status {
    ISV_EXR_OK = 0,
    ISV_EXR_CAPACITY = 1,         /* n_corres > max_corres, or the slot already holds max_frames frames           */
    ISV_EXR_INPUT = 2,            /* a non-finite number, n_corres < 0, a null corres with n_corres > 0, a delta_q of zero norm, a slot
                                     outside [0, max_slots), a slot named by an earlier item of the same call      */
    ISV_EXR_NO_MODEL = 3          /* the estimator kept no model (deviation, above)                               */
} isv_exr_status_t;

typedef struct isv_exr_config {
    int32_t max_slots;            /* sequences resident at once, 1 .. 65535                                       */
    int32_t max_frames;           /* frames a slot records, 8 .. ISV_EXR_MAX_FRAMES                               */
    int32_t max_corres;           /* correspondences per item, 9 .. ISV_EXR_MAX_CORRES                            */
    int32_t vo_size;              /* Vo_SIZE, at least 2                                                          */
} isv_exr_config_t;

typedef struct isv_exr_item {
    int32_t slot;
    int32_t n_corres;
    const double *corres;         /* [n_corres][4] = first.x, first.y, second.x, second.y of
                                     getCorresponding(frame_count - 1, frame_count), in its order (z is not read) */
    double  delta_q[4];           /* w, x, y, z of pre_integrations[frame_count]->delta_q                         */
} isv_exr_item_t;

typedef struct isv_exr_result {
    int32_t status;               /* isv_exr_status_t                                                             */
    int32_t frame_count;          /* the slot's, after the call (unchanged by a refused item; -1: no such slot)   */
    int32_t method;               /* ISV_EXR_NONE / ISV_EXR_LMEDS / ISV_EXR_RANSAC                                */
    int32_t iters;                /* the RANSAC iterations run, or the LMedS niters; 0 for ISV_EXR_NONE           */
    int32_t best_inliers;         /* the kept model's inlier count (LMedS: at its own bound)                      */
    int32_t negated;              /* 1: the E = -E branch was taken                                               */
    int32_t front[4];             /* testTriangulation's front counts of (R1,t1), (R1,t2), (R2,t1), (R2,t2)       */
    int32_t choice;               /* 1: R1, 2: R2; 0 for ISV_EXR_NONE                                             */
    int32_t calibrated;           /* frame_count >= vo_size && singular[2] > 0.25                                 */
    double  Rc[9];                /* this frame's, row-major                                                      */
    double  angle_deg;            /* this frame's row: the angular distance of Rc and Rc_g in degrees             */
    double  huber;                /* and its weight                                                               */
    double  singular[4];          /* A's singular values, descending                                              */
    double  ric[9];               /* the slot's new ric, row-major                                                */
} isv_exr_result_t;

typedef struct isv_exr isv_exr_t;

/* A calibrator on the current device, every slot reset.  ISV_ERR_INVALID_ARG for a null argument or a value outside its range above
 * (before the device is touched); ISV_ERR_DEVICE without a GPU, or when the slots' store (max_slots * max_frames * 344 bytes) cannot be
 * allocated: there is no CPU path. */
int  isv_exr_create(const isv_exr_config_t *cfg, isv_exr_t **out);
void isv_exr_destroy(isv_exr_t *h);
const char *isv_exr_last_error(const isv_exr_t *h);

/* milliseconds of the last successful isv_exr_calibrate_batch that launched: the whole call (host clock), k_exr_calibrate (HIP events) */
int  isv_exr_last_ms(isv_exr_t *h, double out_ms[2]);

/* frame_count = 0, ric = I in each of slots[0..n).  ISV_ERR_INVALID_ARG, with nothing reset, for a slot outside [0, max_slots). */
int  isv_exr_reset(isv_exr_t *h, int32_t n, const int32_t *slots);

/* One CalibrationExRotation call per item: items[0..n), results [n].  One packed upload, k_exr_calibrate (one workgroup per good
 * item), one download of the result records, synchronous on the handle's stream.  An item is refused by its result's status, never
 * truncated; a refused item leaves its slot untouched, its result zero apart from status and frame_count, and does not stop the batch.
 * A call without a good item launches nothing.  A result, and the slot behind it, does not depend, bit for bit, on the batch it ran
 * in.  The call returns ISV_OK whenever it ran. */
int  isv_exr_calibrate_batch(isv_exr_t *h, int32_t n, const isv_exr_item_t *const *items, isv_exr_result_t *results);

/* A slot's state, for tests and for a caller that moves a sequence: frame_count, ric [9], history [frame_count][27] = Rc[i], Rimu[i],
 * Rc_g[i] of the frames i = 1 .. frame_count (each pointer may be NULL; history holds room for max_frames frames).  Synchronous. */
int  isv_exr_read_slot(isv_exr_t *h, int32_t slot, int32_t *frame_count, double *ric, double *history);

#ifdef __cplusplus
}
#endif
#endif /* ISVINS_EXROT_H */
