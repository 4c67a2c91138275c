/*
 * isv_relpose.h -- INTERNAL entry point of the relative-pose stage of the estimator's initialisation (relativePose), batched
 * over sequences on the MI355X.  Not part of the public ABI (include/).  It runs before the SfM stage of isv_sfm.h and fills
 * the `l`, relative_R and relative_T that stage takes; it reads the same isv_sfm_problem_t and ignores those three fields.
 * The library exports it as isv_internal_relpose_batch for its own tests and scripts/relpose_bench.py; its layout may change
 * with the window manager's wiring.  Stages, per problem:
 *   0 Estimator::checkIMUExcitation          src/estimator.cpp:213-238 (the same routine as isv_sfm.h's stage 0)
 *   1 Estimator::relativePose                src/estimator.cpp:431-456: for i = 0 .. n_window - 3 in order, the
 *     correspondences of window frames i and n_window - 1 (FeatureManager::getCorresponding, IDsfeatures order); a candidate
 *     passes when it has more than 20, their mean |a.xy - b.xy| * 460 > 30, and MotionEstimator::solveRelativeRT succeeds.
 *     The first that passes is l.
 *   2 MotionEstimator::solveRelativeRT       src/initial/solve_5pts.cpp:193-230: cv::findFundamentalMat(FM_RANSAC,
 *     0.3 / 460, 0.99), then the file's own recoverPose with K = I (its cheirality masks ANDed with the RANSAC mask);
 *     Rotation = R^T, Translation = -R^T t; success when recoverPose's count > 12.
 *
 * Restated from OpenCV 3.2.0's published sources (modules/calib3d/src/fundam.cpp, ptsetreg.cpp, triangulate.cpp and
 * modules/core/src/mathfuncs.cpp's solveCubic), not checked against them here: the CPU restatement
 * (tests/native/isv_relpose_oracle.c) pins the GPU, not the reference.  What the restatement takes from them:
 *   - RANSACPointSetRegistrator::run: maxIters 1000, a fresh RNG((uint64)-1) per call, getSubset's 7 distinct
 *     rng.uniform(0, count) draws (3.2's FMEstimatorCallback has no checkSubset, checkPartialSubsets is false: no collinearity
 *     redraws), every model of a subset tested in root order, a model kept when its inlier count > max(best, 6), then
 *     niters = RANSACUpdateNumIters(0.99, (count - good) / count, 7, niters) (log, pow, cvRound = round-half-even); a subset
 *     with no model still counts as an iteration; no 8-point refit after RANSAC;
 *   - run7Point: the 7 x 9 system, its last two right singular vectors f1, f2, the det cubic in lambda for
 *     lambda (f1 - f2) + f2, solveCubic's three branches (quadratic / linear when the leading coefficient is 0, three real
 *     roots by acos / cos, one by pow), F(3,3) = 1 unless |s| <= DBL_EPSILON;
 *   - computeError: the larger of the two squared epipolar distances, stored as float, inlier when <= (float)(thresh^2);
 *   - recoverPose: cvTriangulatePoints (a 6 x 4 system per point, three rows per view), the dist = 50 filters, the tie order
 *     good1 >= ..., then good2, good3, good4.
 *
 * Reference quirks reproduced (each marked R1..R5 in the kernel and in the restatement):
 *   R1 RANSAC and recoverPose see the points rounded to float32 (cv::Point2f); the parallax test uses the doubles.
 *   R2 the RANSAC error is stored as float32 and compared with (float)(thresh * thresh).
 *   R3 the "essential" matrix is the fundamental matrix of the normalised points, used as it is (its singular values are not
 *      equalised; decomposeEssentialMat reads only U and V, so this changes no result).
 *   R4 every RANSAC starts from the same RNG state, so every candidate i draws the same index sequence.
 *   R5 relativePose never tries i = n_window - 2.
 * Documented deviations: the 7-point null space, the 3 x 3 SVD of decomposeEssentialMat and the triangulation's SVD use
 * the Eigen-style two-sided Jacobi SVD of isv_init_common.h (the triangulation's 6 x 4 system through a Householder QR),
 * not OpenCV's one-sided one.  A RANSAC that keeps no model fails its candidate (the reference aborts in
 * decomposeEssentialMat on the empty matrix).
 *
 * Caps and input checks: those of isv_sfm.h (l is not read).  Conventions: as include/isvins_backend.h (row-major).
 */
#ifndef ISV_RELPOSE_H
#define ISV_RELPOSE_H

#include "isv_sfm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum isv_relpose_status {
    ISV_RELPOSE_OK = 0,
    ISV_RELPOSE_REFUSED_EXCITATION = 1,   /* checkIMUExcitation: spread of delta_v / sum_dt < 0.25 (checked first)        */
    ISV_RELPOSE_NO_RELATIVE_POSE = 2,     /* no candidate i passed                                                        */
    ISV_RELPOSE_REFUSED_CAPACITY = 3,     /* beyond an isv_sfm.h cap                                                       */
    ISV_RELPOSE_REFUSED_INPUT = 4         /* isv_sfm.h's input checks, l aside                                             */
} isv_relpose_status_t;

typedef struct isv_relpose_result {
    int32_t status;               /* isv_relpose_status_t                                                          */
    int32_t l;                    /* the chosen i (-1: none)                                                       */
    int32_t n_candidates;         /* candidates evaluated: i = 0 .. n_candidates - 1                               */
    int32_t _pad;
    double  excitation_var;       /* checkIMUExcitation's var                                                      */
    double  relative_R[9], relative_T[3];   /* solveRelativeRT's Rotation / Translation of l (zero unless OK)       */
    /* per candidate i (-1 when not evaluated: beyond n_candidates, or a test before it failed) */
    int32_t n_corres[ISV_ALIGN_MAX_WINDOW];        /* getCorresponding(i, n_window - 1).size()                      */
    int32_t ransac_iters[ISV_ALIGN_MAX_WINDOW];    /* RANSAC iterations run                                         */
    int32_t ransac_inliers[ISV_ALIGN_MAX_WINDOW];  /* the kept model's inliers (0: no model kept)                   */
    int32_t recover_inliers[ISV_ALIGN_MAX_WINDOW]; /* recoverPose's count                                           */
    int32_t solution[ISV_ALIGN_MAX_WINDOW];        /* recoverPose's choice: 1 [R1|t], 2 [R2|t], 3 [R1|-t], 4 [R2|-t] */
    double  parallax[ISV_ALIGN_MAX_WINDOW];        /* mean |a.xy - b.xy| (normalised units, -1: not evaluated)       */
} isv_relpose_result_t;

/* stages 0-2 for n independent problems: one upload, one launch (one 64-lane workgroup per problem), one download, on the
 * handle's device and stream.  masks: NULL, or n pointers (each NULL or [n_tracks]) that receive the chosen pair's final
 * inlier mask per track (1 / 0; -1 for a track that is not a correspondence of that pair, and everywhere when no pair was
 * chosen; not written for a CAPACITY or INPUT refusal).  Returns ISV_OK when the batch ran (a refusal is a per-problem status), ISV_ERR_INVALID_ARG for a null pointer or
 * n < 0, ISV_ERR_DEVICE on a HIP error.  A problem's result and mask are bitwise independent of the batch it is solved in.
 * Device buffers are kept on the handle and grow only. */
int isv_internal_relpose_batch(isv_backend_t *h, int32_t n, const isv_sfm_problem_t *const *problems, isv_relpose_result_t *results,
                               int32_t *const *masks);
/* times of the last isv_internal_relpose_batch on this handle: [0] the whole call, [1] the kernel alone (HIP events) */
int isv_internal_relpose_last_ms(isv_backend_t *h, double out_ms[2]);

#ifdef __cplusplus
}
#endif
#endif /* ISV_RELPOSE_H */
