/*
 * isv_initial.h -- INTERNAL entry point of the visual-inertial alignment stage of the estimator's initialisation, batched over
 * sequences on the MI355X.  Not part of the public ABI (include/): it is the building block of the window manager's
 * self-initialisation (initialStructure: relative-pose RANSAC, SfM, all-frame PnP, then this stage).  The SfM and the all-frame
 * PnP are isv_sfm.h, whose results fill this stage's R / T / is_key_frame; the relative-pose RANSAC before it is isv_relpose.h.
 * The window manager's wiring is not built yet.
 * The library exports it as isv_internal_visual_imu_align_batch for its own tests and scripts/init_bench.py only; its
 * layout may change with that work.  Stages:
 *   solveGyroscopeBias                    src/initial/initial_aligment.cpp:3-37
 *   IntegrationBase::repropagate          include/factor/integration_base.h:38-52 (deltas only, see below)
 *   TangentBasis / RefineGravity          src/initial/initial_aligment.cpp:40-126
 *   LinearAlignment / VisualIMUAlignment  src/initial/initial_aligment.cpp:128-208
 *   Estimator::visualInitialAlign         src/estimator.cpp:357-429 (the state rebuild; see "caller's share" below)
 *   Utility::g2R                          src/utility/utility.cpp:3-13
 * One problem = one sequence's all_image_frame after GlobalSFM::construct and the all-frame PnP of
 * Estimator::initialStructure (src/estimator.cpp:239-349): per frame the SfM rotation R (= R_pnp * RIC^T) and camera centre T
 * (up to scale) in the frame of the SfM's reference camera, the frame's pre-integration since the previous image, and its raw
 * IMU samples.  The relative-pose RANSAC, the SfM and the PnP that produce R / T are separate entry points (isv_relpose.h,
 * isv_sfm.h).
 *
 * The caller's share of visualInitialAlign (host or other kernels of this library):
 *   - the depth reset + f_manager.triangulate with tic = 0 and the `estimated_depth *= s` of good features (:378-411)
 *     (isv_backend_triangulate does the triangulation);
 *   - the window's own `pre_integrations[i]->repropagate(0, Bgs[i])` (:390-393) with the Bgs this call returns.
 *
 * Reference quirks reproduced (each marked in the kernel and in tests/native/isv_init_oracle.c):
 *   Q1 solveGyroscopeBias takes jacobian.block<3,3>(3,3) (d dtheta / d dtheta, "TODO verify") as the bias Jacobian, not
 *      block<3,3>(O_R, O_BG) -- the caller passes that block as `jac_rr`;
 *   Q2 RefineGravity zeroes A and b once, before its 4 passes: every pass adds to the previous pass's system, then scales the sum
 *      by 1000 (initial_aligment.cpp:53-56,111-113);
 *   Q3 Vs[kv] = R * x.segment<3>(kv * 3): kv counts keyframes, x is indexed by every frame of all_image_frame (estimator.cpp:398-406).
 * Eigen's LDLT is restated as its unblocked left-looking form with diagonal pivoting on the not yet updated diagonal
 * (Eigen 3.3 LDLT.h ldlt_inplace<Lower>::unblocked) and the solve's pseudo-inverse of D (|d| <= DBL_MIN -> 0).
 * Repropagation computes delta_p / delta_q / delta_v / sum_dt only: nothing downstream of the alignment reads the
 * repropagated jacobian or covariance of all_image_frame.
 * Conventions: as include/isvins_backend.h (row-major matrices, quaternions x y z w).
 */
#ifndef ISV_INITIAL_H
#define ISV_INITIAL_H

#include "../../include/isvins_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISV_ALIGN_MAX_FRAMES 40   /* all_image_frame capacity per problem; more is refused.  The kernel keeps RefineGravity's
                                     accumulated system and its factor in LDS: 2 x 123 x 124 / 2 doubles at 40 frames */
#define ISV_ALIGN_MAX_WINDOW 20   /* frame_count + 1 capacity                                                          */

typedef enum isv_align_stage {
    ISV_ALIGN_OK = 0,
    ISV_ALIGN_REFUSED_GRAVITY = 1,       /* LinearAlignment: fabs(|g| - |G|) > 1.0 (initial_aligment.cpp:189-192)           */
    ISV_ALIGN_REFUSED_SCALE = 2,         /* LinearAlignment: s < 0 before the refinement (:189-192)                       */
    ISV_ALIGN_REFUSED_REFINED_SCALE = 3, /* s < 0 after RefineGravity (:198-201)                                          */
    ISV_ALIGN_REFUSED_CAPACITY = 4,      /* n_frames > ISV_ALIGN_MAX_FRAMES or n_window > ISV_ALIGN_MAX_WINDOW: not truncated */
    ISV_ALIGN_REFUSED_INPUT = 5,         /* n_frames < 2, window indices not increasing / out of range, keyframe count != n_window,
                                            IMU rows out of range                                                         */
    ISV_ALIGN_REFUSED_ANTIPARALLEL = 6   /* g2R: g points along -z within 1e-12 (Eigen FromTwoVectors' SVD branch, not restated) */
} isv_align_stage_t;

/* one entry of all_image_frame (include/initial/initial_alignment.h ImageFrame), in time order */
typedef struct isv_align_frame {
    double  R[9];                 /* ImageFrame::R, row-major                                                        */
    double  T[3];                 /* ImageFrame::T                                                                   */
    double  delta_q[4];           /* pre_integration->delta_q (x y z w) as propagated, BEFORE the bias solve         */
    double  jac_rr[9];            /* pre_integration->jacobian.block<3,3>(3,3), row-major (quirk Q1)                 */
    double  linearized_acc[3];    /* pre_integration->linearized_acc / linearized_gyr: acc_0 / gyr_0 of repropagate */
    double  linearized_gyr[3];
    int32_t imu_begin, imu_count; /* rows [imu_begin, imu_begin + imu_count) of the problem's imu[]: its dt_buf / acc_buf / gyr_buf */
    int32_t is_key_frame, _pad;   /* ImageFrame::is_key_frame as initialStructure left it                            */
} isv_align_frame_t;              /* frame 0's pre-integration fields are not read (the loops start at next(begin)) */

typedef struct isv_align_problem {
    int32_t n_frames;             /* all_image_frame.size()                                                          */
    int32_t n_window;             /* frame_count + 1 (= ALL_BUF_SIZE when the window is full)                        */
    int32_t n_imu;                /* rows of imu[]                                                                   */
    int32_t _pad;
    const isv_align_frame_t *frames;   /* [n_frames]                                                                 */
    const double *imu;            /* [n_imu][7]: dt, acc xyz, gyr xyz                                                */
    int32_t window_frame[ISV_ALIGN_MAX_WINDOW];   /* index in frames[] of Headers[i], strictly increasing             */
    double  G[3];                 /* G (only |G| is read)                                                            */
    double  tic[3];               /* TIC[0]                                                                          */
    double  Bgs[ISV_ALIGN_MAX_WINDOW][3];         /* Bgs[0 .. n_window) on entry                                      */
} isv_align_problem_t;

typedef struct isv_align_result {
    int32_t status;               /* isv_align_stage_t                                                               */
    int32_t n_state;              /* LinearAlignment's 3 n_frames + 4                                                */
    double  delta_bg[3];          /* solveGyroscopeBias' increment                                                   */
    double  Bgs[ISV_ALIGN_MAX_WINDOW][3];
    double  g_linear[3], s_linear;     /* LinearAlignment's g and s = x(n-1)/100 before RefineGravity                 */
    double  g_c0[3];              /* RefineGravity's g, in the SfM frame                                             */
    double  g[3], s;              /* visualInitialAlign's output: g rotated by R0, s                                 */
    double  Ps[ISV_ALIGN_MAX_WINDOW][3], Rs[ISV_ALIGN_MAX_WINDOW][9], Vs[ISV_ALIGN_MAX_WINDOW][3];
    double  R0[9];                /* rot_diff                                                                        */
    double  x[3 * ISV_ALIGN_MAX_FRAMES + 3];      /* RefineGravity's solution (velocities of every frame, dg, s)     */
    /* every frame's pre-integration after repropagate(0, Bgs[0]) (frame 0: untouched, zeros) */
    double  rp_delta_p[ISV_ALIGN_MAX_FRAMES][3], rp_delta_q[ISV_ALIGN_MAX_FRAMES][4], rp_delta_v[ISV_ALIGN_MAX_FRAMES][3];
    double  rp_sum_dt[ISV_ALIGN_MAX_FRAMES];
} isv_align_result_t;

/* VisualIMUAlignment + the state rebuild of visualInitialAlign for n independent problems: one upload, one launch (one
 * workgroup per problem), one download, on the handle's device and stream.  Returns ISV_OK when the batch ran (a refusal is a
 * per-problem status, not an error), ISV_ERR_INVALID_ARG for a null pointer or n < 0, ISV_ERR_DEVICE on a HIP error.
 * Each problem's result is bitwise independent of the batch it is solved in.  Device buffers are kept on the handle and grow
 * only; the call is not thread-safe on one handle (like every isv_backend_* call). */
/* times of the last call on this handle: [0] the whole call (host packing, copies, kernel), [1] the kernel alone (HIP events) */
int  isv_internal_align_last_ms(isv_backend_t *h, double out_ms[2]);
int  isv_internal_visual_imu_align_batch(isv_backend_t *h, int32_t n, const isv_align_problem_t *const *problems, isv_align_result_t *results);

#ifdef __cplusplus
}
#endif
#endif /* ISV_INITIAL_H */
