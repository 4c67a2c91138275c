/*
 * isvins_loop.h -- C ABI of the batched loop-closure VERIFICATION: the geometric check of one loop candidate,
 *   KeyFrame::findConnection              src/pose_graph/keyframe.cpp:231-295                      (MI355X)
 *     searchByBRIEFDes / searchInAera / HammingDis        :77-126, :298-303     kernel k_loop_match
 *     PnPRANSAC (cv::solvePnPRansac), the relative pose, the yaw / distance gate, loop_weight      :155-228, :262-292
 *                                                                                kernel k_loop_pnp
 * for many (current keyframe, old keyframe) pairs in one call.  Its result is what isvins_posegraph.h consumes: the
 * has_loop / loop_index / loop_info / loop_weight members of isv_pg_keyframe_t (isv_loop_apply writes them).
 *
 * Not here: the DBoW query that proposes old_index (PoseGraph::detectLoop: include/isvins_bow.h, whose loop_index it is),
 * BRIEF extraction and FAST (include/isvins_keyframe.h), addKeyFrame's sequence shift and earliest_loop_index bookkeeping
 * (pose_graph.cpp:59-110).  The candidate and the descriptors are inputs.  point_2d_uv and point_id are only compacted by
 * findConnection and never read, so the pair does not carry them; point_2d_norm is carried (the reference's KeyFrame has
 * it) and, like them, never read.
 *
 * cv::solvePnPRansac is RESTATED from OpenCV 3.2.0 as published (calib3d: solvepnp.cpp, ptsetreg.cpp, epnp.cpp,
 * calibration.cpp); OpenCV is not available to this project, so the restatement cannot be checked against its source.  The CPU
 * restatement tests/native/isv_loop_oracle.c runs the same shared text (is-vins_amd/csrc/isv_loop_common.h) as the kernel and
 * pins the GPU, not the definition; an independent 40-digit reading of the definitions cited below (tests/loop_highprec.py) pins
 * both the restatement and the kernel.
 *   RANSACPointSetRegistrator::run   modelPoints 5, ransac_iterations at most, a fresh RNG((uint64)-1), getSubset's distinct
 *                                    draws, a model kept when its inlier count > max(best, 4), RANSACUpdateNumIters; the error of
 *                                    a point is the squared float32 distance of its float32 projection, compared in float32
 *   the minimal solver               EPnP on the five points: control points, barycentric coordinates, M^T M (12 x 12), its four
 *                                    smallest eigenvectors, L_6x10 / rho, three beta approximations with five Gauss-Newton
 *                                    iterations each, R and t by the 3 x 3 SVD; the N of lowest reprojection error
 *   the final solve                  solvePnP(SOLVEPNP_ITERATIVE, no guess) over the kept model's inliers: the non-planar DLT
 *                                    (12 x 12 L^T L), then CvLevMarq (20 iterations, FLT_EPSILON) -- the loop of the SfM stage
 *
 * Reference quirks that are KEPT (marked L1.. in the kernel and the restatement):
 *   L1  with more than 0.6 min_loop_num and at most min_loop_num matches the reference skips PnPRANSAC and then reads PnP_R_old /
 *       PnP_T_old uninitialised (:262-277).  Here: status ISV_LOOP_UNDEFINED_POSE, no loop.
 *   L2  of equal minimal Hamming distances the lowest old index wins (strict < from bestDist = 128, :84-95): a candidate counts
 *       below match_max_dist (128), the match is accepted below match_accept_dist (80).
 *   L3  loop_weight's residual is a normalised-plane residual divided by FOCAL_LENGTH once more; the point in the old camera is
 *       formed as p_ = R_pnp (p - T_w_c_old) (:216-220), not as R_pnp p + T_pnp.
 *   L4  the VIO-pose guess of :167-175 is computed and never read: OpenCV 3.2's RANSAC kernel is EPnP, which ignores the guess,
 *       and the final solvePnP is called without it.  (This is the restater's reading of 3.2.0.)  origin_vio_* enter only the
 *       relative pose.
 *   L5  every point passes through float32 (cv::Point3f / Point2f).
 *   L6  several window points may claim the same old corner; there is no uniqueness test.
 * Deviations (documented, not quirks): the SVDs / eigen-decompositions are this project's Jacobi routines and the small
 * least-squares solves Householder QR; Rodrigues(matrix) skips OpenCV's re-orthonormalisation (as in the SfM stage); a planar
 * inlier set (W[2] / W[1] < 1e-3 of the points' covariance, where OpenCV switches to a homography initialisation) is refused with
 * ISV_LOOP_PLANAR; the final solve is skipped when at most 0.6 min_loop_num inliers remain (findConnection returns false
 * whatever it yields); npoints == 4 (P3P) cannot occur behind the > min_loop_num gate.
 * Conventions: as include/isvins_backend.h (row-major matrices).
 */
#ifndef ISVINS_LOOP_H
#define ISVINS_LOOP_H

#include "isvins_posegraph.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum isv_loop_status {
    ISV_LOOP_OK = 0,              /* findConnection returns true                                                  */
    ISV_LOOP_FEW_MATCHES = 1,     /* at most 0.6 min_loop_num points matched                                      */
    ISV_LOOP_UNDEFINED_POSE = 2,  /* L1                                                                           */
    ISV_LOOP_PNP_FAILED = 3,      /* the RANSAC kept no model, or at most 0.6 min_loop_num points survive its mask */
    ISV_LOOP_GATE = 4,            /* the yaw or the distance test failed (:282)                                   */
    ISV_LOOP_PLANAR = 5,          /* deviation: planar inlier set                                                 */
    ISV_LOOP_CAPACITY = 6,        /* n_points > max_points or n_keypoints > max_keypoints                         */
    ISV_LOOP_INPUT = 7            /* non-finite values, negative counts, null arrays with a non-zero count        */
} isv_loop_status_t;

typedef struct isv_loop_config {
    int32_t max_pairs;             /* pairs per call                                                              */
    int32_t max_points;            /* window points per keyframe                                                  */
    int32_t max_keypoints;         /* the old keyframe's corners (at most 2^20)                                   */
    int32_t min_loop_num;          /* MIN_LOOP_NUM = 15 (at least 9)                                              */
    int32_t ransac_iterations;     /* 100 (keyframe.cpp:187)                                                      */
    int32_t match_max_dist;        /* 128 (:84)                                                                   */
    int32_t match_accept_dist;     /* 80 (:97)                                                                    */
    int32_t _pad;
    double  ric[9], tic[3];        /* RIC[0] / TIC[0]                                                             */
    double  focal_length;          /* FOCAL_LENGTH = 460                                                          */
    double  ransac_threshold;      /* 10.0 / 460.0 (:187)                                                         */
    double  ransac_confidence;     /* 0.99                                                                        */
    double  max_yaw_deg;           /* 30 (:282)                                                                   */
    double  max_distance;          /* 20 (:282)                                                                   */
} isv_loop_config_t;

/* one candidate pair: the current keyframe's window points and the old keyframe's corners.  A 256-bit descriptor is four
 * uint64_t words: bit 64 w + b of the descriptor is bit b of word w. */
typedef struct isv_loop_pair {
    int32_t n_points;              /* current keyframe: window points                                             */
    int32_t n_keypoints;           /* old keyframe: corners                                                       */
    int32_t old_index;             /* old keyframe's index                                                        */
    int32_t _pad;
    const uint64_t *window_brief;  /* [n_points][4]      window_brief_descriptors                                 */
    const float    *point_3d;      /* [n_points][3]      point_3d                                                 */
    const float    *point_2d_norm; /* [n_points][2]      point_2d_norm (never read; may be NULL)                  */
    const uint64_t *brief;         /* [n_keypoints][4]   old keyframe's brief_descriptors                         */
    const float    *keypoints_norm;/* [n_keypoints][2]   old keyframe's keypoints_norm                            */
    double origin_vio_T[3], origin_vio_R[9];   /* current keyframe's origin_vio_T / origin_vio_R                  */
} isv_loop_pair_t;

typedef struct isv_loop_result {
    int32_t status;                /* isv_loop_status_t                                                           */
    int32_t n_matched;             /* points matched by descriptor                                                */
    int32_t ransac_iters;          /* iterations the RANSAC ran (-1: it did not run)                              */
    int32_t ransac_inliers;        /* the kept model's inlier count (0: no model)                                 */
    int32_t pnp_iterations;        /* the final CvLevMarq's iterations (-1: it did not run)                       */
    int32_t n_final;               /* points left after the PnP mask (n_matched where the PnP did not run)        */
    int32_t has_loop, loop_index;
    double  loop_info[8];          /* relative t (3), relative q as w x y z (4), relative yaw in degrees (keyframe.h:110) */
    double  loop_weight;           /* :223-227                                                                    */
    double  PnP_T_old[3], PnP_R_old[9];
    double  res;                   /* the residual sum of :211-222                                                */
} isv_loop_result_t;

typedef struct isv_loop isv_loop_t;

/* Fails with ISV_ERR_DEVICE without a GPU: there is no CPU path. */
int  isv_loop_create(const isv_loop_config_t *cfg, isv_loop_t **out);
void isv_loop_destroy(isv_loop_t *h);
const char *isv_loop_last_error(const isv_loop_t *h);

/* findConnection of pairs[0..n): one packed upload, k_loop_match, k_loop_pnp, one download, synchronous on the handle's own
 * stream.  results [n].  match_index / match_dist / inlier: NULL, or [n] pointers each NULL or to [n_points] int32:
 *   match_index   the matched old corner, -1: none
 *   match_dist    the minimal Hamming distance found below match_max_dist, else match_max_dist
 *   inlier        1 / 0 for a point that reached the PnP, -1 otherwise
 * A pair that cannot be verified is refused by its status (ISV_LOOP_CAPACITY, ISV_LOOP_INPUT), never truncated, and its per-point
 * outputs are left untouched; the call returns ISV_OK whenever it ran.  A pair's result record and per-point outputs do not
 * depend, bit for bit, on the batch it is verified in. */
int  isv_loop_verify_batch(isv_loop_t *h, int32_t n, const isv_loop_pair_t *const *pairs, isv_loop_result_t *results,
                           int32_t *const *match_index, int32_t *const *match_dist, int32_t *const *inlier);
/* milliseconds of the last successful call: the whole call, k_loop_match, k_loop_pnp (HIP events) */
int  isv_loop_last_ms(isv_loop_t *h, double out_ms[3]);

/* Host only: what keyframe.cpp:285-289 and :224 write.  Status ISV_LOOP_OK: has_loop, loop_index, loop_info, loop_weight.
 * Any other status: loop_weight only (the reference writes it whenever PnPRANSAC ran; the result holds 0 where it did not, where
 * it kept no usable model and for ISV_LOOP_PLANAR). */
int  isv_loop_apply(const isv_loop_result_t *result, isv_pg_keyframe_t *cur);

#ifdef __cplusplus
}
#endif
#endif /* ISVINS_LOOP_H */
