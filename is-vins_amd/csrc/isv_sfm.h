/*
 * isv_sfm.h -- INTERNAL entry point of the structure-from-motion stage of the estimator's initialisation, batched over
 * sequences on the MI355X.  Not part of the public ABI (include/).  It sits between the relative-pose RANSAC of isv_relpose.h
 * (which finds the `l` and relative_R / relative_T this stage takes) and the visual-inertial alignment of isv_initial.h, whose per-frame inputs
 * (isv_align_frame_t::R, T, is_key_frame) it produces.  The library exports it as isv_internal_sfm_batch for its own tests
 * and scripts/init_bench.py only; its layout may change with the window manager's wiring.  Stages, per problem:
 *   0 Estimator::checkIMUExcitation       src/estimator.cpp:213-238
 *   1 GlobalSFM::construct, steps 1-5     src/initial/initial_sfm.cpp:117-220 (two-view set-up, PnP + triangulation sweeps)
 *   2 the full BA                         initial_sfm.cpp:222-279 (ReprojectionError3D, QuaternionParameterization, Ceres LM)
 *   3 GlobalSFM::solveFrameByPnP          initial_sfm.cpp:22-71 (cv::solvePnP, SOLVEPNP_ITERATIVE with a guess)
 *   4 the all-frame PnP                   src/estimator.cpp:281-347
 *
 * Restatements (tests/native/isv_sfm_oracle.c does the same operations in the same order on the CPU):
 *   - triangulatePoint: Eigen 3.3 JacobiSVD of the 4 x 4 design matrix (square: no QR preconditioner; scaled by its largest
 *     |entry|, two-sided 2 x 2 Jacobi sweeps, singular values sorted), V's last column divided by its fourth entry;
 *   - the BA: Ceres 2.0.0 TrustRegionMinimizer + LevenbergMarquardtStrategy with its defaults (50 iterations, radius 1e4,
 *     jacobi scaling, tolerances 1e-10 / 1e-8 / 1e-6, LM diagonal clamped to [1e-6, 1e32], 5 invalid steps) over
 *     DENSE_SCHUR: every triangulated point is eliminated (its 3 x 3 block plus the LM diagonal inverted by LLT, the
 *     full-rank branch of InvertPSDMatrix), the reduced camera system is factored by a dense unblocked Cholesky.  The
 *     Jacobian is the analytic derivative of ReprojectionError3D (AutoDiff's jet rounding is not restated) and the tangent
 *     Jacobian of QuaternionParameterization is -2 [R X]x;
 *   - cv::solvePnP(useExtrinsicGuess = true): OpenCV 3.2 cvFindExtrinsicCameraParams2's CvLevMarq (6 parameters, at most 20
 *     iterations, eps = FLT_EPSILON on the relative parameter change, lambdaLg10 from -3, +-1 on reject / accept, clamped to
 *     +-16, JtJ.diag() *= 1 + lambda), cvProjectPoints2 with K = I and no distortion (its terms that the zero distortion
 *     makes exact zeros are dropped) and cv::Rodrigues both ways.  Deviations: cv::solve(DECOMP_SVD) is restated with the
 *     same two-sided Jacobi SVD as the triangulation (back-substitution threshold 2 DBL_EPSILON sum(w)), and the SVD
 *     re-orthonormalisation of Rodrigues' matrix-to-vector path is dropped (its effect on a rotation matrix is at rounding
 *     level).  Written from the published OpenCV and Ceres sources, not checked against them: the CPU restatement pins the
 *     GPU, not the reference;
 *   - Eigen's vectorised reductions are restated as serial sums in storage order; the BA's cost, model cost and norms sum
 *     per point (observations in order), then over points in track order.
 *
 * Reference quirks reproduced (each marked S1..S8 in the kernel and in the restatement):
 *   S1 checkIMUExcitation's `Vector3d sum_g;` is never initialised; restated as zero.
 *   S2 both PnPs pass their points through cv::Point3f / cv::Point2f: 3-D and 2-D inputs are rounded to float32.
 *   S3 solveFrameByPnP fails below 10 points (15 is only a warning); the all-frame PnP fails below 6.
 *   S4 in the all-frame loop a non-keyframe first advances i when it lies after Headers[i] (`if (t > Headers[i]) i++`), and
 *      guesses from keyframe i: for a frame between two keyframes that is the NEXT keyframe's pose.
 *   S5 step 5 triangulates a track from its first and last observations; nothing checks cheirality, a point behind a
 *      camera enters the BA.  (triangulateTwoFrames keeps the last matching observation of a frame and solveFrameByPnP the
 *      first; with IDsfeatures' consecutive frames a track sees a frame at most once, so the two agree.)
 *   S6 the BA quaternion follows QuaternionParameterization::Plus and is never renormalised; QuaternionRotatePoint divides
 *      by its norm; the result's q.inverse() is conjugate / squaredNorm and T = -(q * t) is Eigen's _transformVector, which
 *      assumes a unit norm.
 *   S7 max_solver_time_in_seconds = 0.2 is a wall-clock stop and is NOT restated (nobody has measured whether the
 *      reference's BA reaches it on an 18-frame window).
 *   S8 SfM PnP points go in track order, the all-frame PnP's in ascending feature_id (std::map) order.
 *
 * Caps (more is refused with ISV_SFM_REFUSED_CAPACITY, never truncated): n_window <= ISV_ALIGN_MAX_WINDOW, n_frames <=
 * ISV_ALIGN_MAX_FRAMES, n_tracks <= ISV_SFM_MAX_TRACKS, n_obs <= ISV_SFM_MAX_OBS.  The kernel keeps the observations
 * (16 B each), the points (24 B each) and the packed reduced camera system in LDS: 64 + 24 + 49.7 KiB at the caps.
 * Conventions: as include/isvins_backend.h (row-major matrices, quaternions x y z w).
 */
#ifndef ISV_SFM_H
#define ISV_SFM_H

#include "isv_initial.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISV_SFM_MAX_TRACKS 1024   /* IDsfeatures entries per problem (the reference's NUM_OF_F is 1000)                */
#define ISV_SFM_MAX_OBS    4096   /* track observations per problem: the LDS budget (64 KiB of the kernel's 160)       */

typedef enum isv_sfm_status {
    ISV_SFM_OK = 0,
    ISV_SFM_REFUSED_EXCITATION = 1,      /* checkIMUExcitation: spread of delta_v / sum_dt < 0.25                            */
    ISV_SFM_REFUSED_SFM_PNP_POINTS = 2,  /* solveFrameByPnP: fewer than 10 points (fail_frame = window index)               */
    ISV_SFM_REFUSED_BA_NOT_CONVERGED = 3,/* the BA neither CONVERGENCE nor final_cost < 5e-3                                */
    ISV_SFM_REFUSED_ALL_PNP_POINTS = 4,  /* all-frame PnP: fewer than 6 points (fail_frame = all_image_frame index)         */
    ISV_SFM_REFUSED_CAPACITY = 5,        /* beyond a cap                                                                     */
    ISV_SFM_REFUSED_INPUT = 6            /* l < 0 or l >= n_window - 1, n_frames < 2, bad tracks or CSR, window indices not
                                            increasing, out of range or not ending at the last frame                        */
} isv_sfm_status_t;

typedef struct isv_sfm_track {   /* one IDsfeatures entry; observation k is in window frame start_frame + k       */
    int32_t id, start_frame, n_obs, obs_off;   /* obs rows [obs_off, obs_off + n_obs) of the problem's obs[]       */
} isv_sfm_track_t;

typedef struct isv_sfm_problem {
    int32_t n_window;             /* frame_count + 1                                                               */
    int32_t n_frames;             /* all_image_frame.size()                                                        */
    int32_t l;                    /* relativePose's frame (selectidx)                                              */
    int32_t n_tracks, n_obs, n_pts;
    double  relative_R[9], relative_T[3];
    double  RIC[9];
    const isv_sfm_track_t *tracks;     /* [n_tracks], IDsfeatures order                                            */
    const double  *obs;                /* [n_obs][2] normalised image points                                       */
    const int32_t *pt_off;             /* [n_frames + 1] CSR of all_image_frame's points                           */
    const int32_t *pt_id;              /* [n_pts] feature_id, strictly ascending within a frame                    */
    const double  *pt_uv;              /* [n_pts][2]                                                               */
    const double  *delta_v;            /* [n_frames][3] pre_integration->delta_v (frame 0's is not read)            */
    const double  *sum_dt;             /* [n_frames]                                                               */
    int32_t window_frame[ISV_ALIGN_MAX_WINDOW];   /* all_image_frame index of Headers[i], strictly increasing       */
    double  *position;                 /* OUT [n_tracks][3]: sfm_f[j].position after the BA (not written on refusal) */
    int32_t *state;                    /* OUT [n_tracks]: sfm_f[j].state                                            */
} isv_sfm_problem_t;

typedef struct isv_sfm_result {
    int32_t status;               /* isv_sfm_status_t                                                              */
    int32_t fail_frame;           /* the frame a stage refused at (-1: none)                                       */
    int32_t ba_iterations, ba_termination;   /* isv_termination_t                                                  */
    int32_t ba_residuals, ba_successful;
    int32_t n_triangulated, n_ba_cols;
    double  excitation_var;       /* checkIMUExcitation's var                                                      */
    double  ba_initial_cost, ba_final_cost;
    double  Q[ISV_ALIGN_MAX_WINDOW][4];      /* construct's q[i] (x y z w) and T[i]                                */
    double  T[ISV_ALIGN_MAX_WINDOW][3];
    int32_t sfm_pnp_iterations[ISV_ALIGN_MAX_WINDOW], sfm_pnp_points[ISV_ALIGN_MAX_WINDOW];
    /* per all_image_frame entry, as isv_align_frame_t has them */
    double  R[ISV_ALIGN_MAX_FRAMES][9];
    double  Tf[ISV_ALIGN_MAX_FRAMES][3];
    int32_t is_key_frame[ISV_ALIGN_MAX_FRAMES];
    int32_t pnp_iterations[ISV_ALIGN_MAX_FRAMES], pnp_points[ISV_ALIGN_MAX_FRAMES];
} isv_sfm_result_t;

/* stages 0-4 for n independent problems: one upload, one launch (one 64-lane workgroup per problem), one download, on the
 * handle's device and stream.  Returns ISV_OK when the batch ran (a refusal is a per-problem status), ISV_ERR_INVALID_ARG for
 * a null pointer or n < 0, ISV_ERR_DEVICE on a HIP error.  A problem's result, per-track outputs included, is bitwise
 * independent of the batch it is solved in.  Device buffers are kept on the handle and grow only. */
int isv_internal_sfm_batch(isv_backend_t *h, int32_t n, const isv_sfm_problem_t *const *problems, isv_sfm_result_t *results);
/* times of the last isv_internal_sfm_batch on this handle: [0] the whole call, [1] the kernel alone (HIP events) */
int isv_internal_sfm_last_ms(isv_backend_t *h, double out_ms[2]);

#ifdef __cplusplus
}
#endif
#endif /* ISV_SFM_H */
