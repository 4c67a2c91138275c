// isv_solver.hip -- on-device trust-region loop around k_build_solve: Ceres-Solver 2.0.0's
// TrustRegionMinimizer + DoglegStrategy(TRADITIONAL_DOGLEG) as problemSolve() configures them
// (reference src/estimator.cpp:1119-1128: DENSE_SCHUR, DOGLEG, max_num_iterations=NUM_ITERATIONS),
// then the pseudo-measurement update (:1133-1144) and double2vector (:518-594).
//
// No host round trip inside the solve: every kernel reads the per-window SolveState and skips
// windows that have terminated; the host enqueues a fixed schedule of max_iter iteration slots.
//   slot:  [linearize if need_linearize] -> k_sweep_mfma -> k_rank1_mfma -> k_build_solve_sb -> k_dogleg (incl. back-substitution)
//          -> candidate evaluation (cost + model cost change) -> k_step_control
#include <hip/hip_runtime.h>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include "isv_kernels.h"
#include "isv_device_math.h"
#include "isv_proj_factor.h"
#include "isv_prior_factor.h"
#include "isv_imu_factor.h"
#include "isv_batch_buffers.h"

extern size_t build_solve_lds_bytes(int N);
template <bool BIG, int NC, int MODE> __global__ void k_build_solve_sb(DevBatch d);
extern size_t build_solve_sb_bytes(int N, int prior_H_sz);
extern size_t build_solve_cs_doubles(int N);
template <bool EX, bool BIG, int NC, int NT> __global__ void k_lin_gram_chain(DevBatch d);
__global__ void k_front(DevBatch d);
template <bool BIG, int NC, bool EX> __global__ void k_pose_dogleg(DevBatch d);
extern size_t front_lds_bytes(int N, int slots);
template <bool BIG, int NC> __global__ void k_build_solve_st(DevBatch d);
extern size_t build_solve_st_bytes(int N, int prior_H_sz);
extern size_t build_solve_st_ws_doubles(int N);
__global__ void k_model_imu_prior(DevBatch d);
__global__ void k_backsub_split(DevBatch d);
__global__ void k_init_priors(DevBatch d, double *scratch, size_t per_window, double *kld_out);
__global__ void k_imu_raw(DevBatch d, const double *pose_src, const double *sb_src, int gate);
__global__ void k_imu_weight(DevBatch d, double *cost_out, int gate);
__global__ void k_sweep_mfma(DevBatch d);
template <int NT, int TPW, int R1_CHUNK, int MINW, bool EX> __global__ void k_rank1_mfma(DevBatch d);
__global__ void k_marg_clear(DevBatch d);
template <int MTF> __global__ void k_marg_fwd(DevBatch d);
template <int PART> __global__ void k_marg_bwd(DevBatch d);
template <int NC> __global__ void k_marg_jacobi(DevBatch d);
__global__ void k_build_solve(DevBatch d);

// ------------------------------------------------------------------------------------------
__global__ void k_init_state(DevBatch d) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= d.B) return;
    SolveState s;
    memset(&s, 0, sizeof(s));
    s.radius = 1e4; s.mu = 1e-8; s.need_linearize = 1; s.termination = ISV_TERM_RUNNING;
    if (ISV_SEQ_IDLE(d, w)) { s.termination = ISV_TERM_MAX_ITERATIONS; s.need_linearize = 0; }      // (a resident sequence without a frame this step: every solver kernel skips it)
    d.st[w] = s;
    for (int k = 0; k < ISV_MAX_TRACE; k++) {
        d.trace_cost[(size_t)w * ISV_MAX_TRACE + k] = 0; d.trace_radius[(size_t)w * ISV_MAX_TRACE + k] = 0;
        d.trace_step[(size_t)w * ISV_MAX_TRACE + k] = 0; d.trace_acc[(size_t)w * ISV_MAX_TRACE + k] = 0;
    }
}

#include "isv_dogleg.h"

// CONTROL: the candidate evaluation + TrustRegionMinimizer step control of this window follow in the same workgroup
// (one launch and one round of workgroups less per iteration than k_dogleg -> k_step_control<true>)
// EX: estimate_extrinsic = 1 (its own instantiation: the extra code costs the ordinary kernels registers otherwise)
template <bool CONTROL, bool EX>
__global__ __launch_bounds__(256, 4) void k_dogleg(DevBatch d) {
    __shared__ double red[256];
    __shared__ int s_accept;
    const int w = blockIdx.x, t = threadIdx.x;
#ifdef ISV_STAMP
    const unsigned long long tk0 = wall_clock64();
#endif
    dogleg_body<EX>(d, w, t, red);
#ifdef ISV_STAMP
    const unsigned long long tk1 = wall_clock64();
#endif
    if (CONTROL) {
        extern __shared__ __align__(16) double dync[];
        __syncthreads();                               // candidate states, per-factor costs and model pieces of this window are written
        step_control_body<true, EX>(d, w, t, dync, red, s_accept);
    }
#ifdef ISV_STAMP
    if (t == 0) { d.dbg[(size_t)w * 64 + 54] += (double)(tk1 - tk0); d.dbg[(size_t)w * 64 + 55] += (double)(wall_clock64() - tk1); }
#endif
}
template __global__ void k_dogleg<false, false>(DevBatch);
template __global__ void k_dogleg<true, false>(DevBatch);
template __global__ void k_dogleg<false, true>(DevBatch);
template __global__ void k_dogleg<true, true>(DevBatch);

// (round 4) the landmark back-substitution of a LONG window on many CUs (grid (B, groups of 128 landmarks)): what k_dogleg's
// first phase does with one workgroup -- per landmark the same function, so the same bits.  Launched between
// k_build_solve_sb and k_dogleg when the elimination is split (d.bs_split).
__global__ __launch_bounds__(128) void k_backsub_split(DevBatch d) {
    extern __shared__ __align__(16) double zsus[];
    const int w = blockIdx.x, t = threadIdx.x;
    const SolveState &st = d.st[w];
    if (st.termination != ISV_TERM_RUNNING || st.ls_fail || !st.fresh) return;
    const int n = d.np, l0 = d.lm_off[w], l1 = d.lm_off[w + 1];
    const int l = l0 + (int)blockIdx.y * 128 + t;
    if (l0 + (int)blockIdx.y * 128 >= l1) return;
    double *zs = zsus, *us = zsus + n;
    for (int i = t; i < n; i += 128) { zs[i] = d.zp[(size_t)w * n + i]; us[i] = d.up[(size_t)w * n + i]; }
    __syncthreads();
    if (l < l1) backsub_landmark<false>(d, l, d.f_off[w], zs, us, st.mu);
}


template <bool FUSED, bool EX>
__global__ __launch_bounds__(256) void k_step_control(DevBatch d) {
    extern __shared__ __align__(16) double cl[];
    __shared__ double red[256];
    __shared__ int s_accept;
    step_control_body<FUSED, EX>(d, blockIdx.x, threadIdx.x, cl, red, s_accept);
}

// ------------------------------------------------------------------------------------------
// after the solve: update() of every prior (estimator.cpp:1133-1144), then double2vector (:518-594)
// NT = 64: one wavefront per window, lane roles for the prior updates (lane 0 Linear9, lane 1 the SE3 prior, lanes 2-31 the
// relative poses, lanes 32-63 roll / pitch): the wavefront runs the four diverging so3_log / so3_exp chains one after another.
// NT = 256: a wavefront per role (0: Linear9 and the SE3 prior, 1: relative poses, 2: roll / pitch, 3: the extrinsic of part 2),
// so the chains run side by side; lane per frame for double2vector and lanes over the landmarks for the depths, over all NT.
// The arithmetic of every role and entry is the same: the two forms give the same bits.
// clear_marg: also clear the window's marginalisation record (k_marg_clear's job, which both marginalisation kernels wait for)
template <int NT>
__global__ __launch_bounds__(NT, NT > 64 ? 4 : 1) void k_finalize(DevBatch d, int do_update, int clear_marg) {
    // (NT = 256: at most 128 registers -- a batch of four windows per CU is then resident at once, not in two rounds)
    const int w = blockIdx.x, t = threadIdx.x, lane = t & 63;
    // the role of this lane and its index / stride inside the role
    constexpr bool WIDE = NT > 64;
    const int role = WIDE ? t >> 6 : (lane < 2 ? 0 : lane < 32 ? 1 : 2);
    const int rel0 = WIDE ? lane : lane - 2, rel_step = WIDE ? 64 : 30;
    const int rp0 = WIDE ? lane : lane - 32, rp_step = WIDE ? 64 : 32;
    const bool ex_lane = WIDE ? t == 192 : lane == 2;
    if (ISV_SEQ_IDLE(d, w)) return;
    const int N = d.N, v = d.Nvo - 1;
    const double *pose = d.pose + (size_t)w * N * 7, *sb = d.sb + (size_t)w * N * 9;
    double *Ps = d.Ps + (size_t)w * N * 3, *Rs = d.Rs + (size_t)w * N * 9, *Vs = d.Vs + (size_t)w * N * 3;
    double *Bas = d.Bas + (size_t)w * N * 3, *Bgs = d.Bgs + (size_t)w * N * 3;
    // ---- double2vector, part 1: the yaw re-anchoring rotation from the OLD Rs[0] / Ps[0] (every lane) ----
    double origin_R0[3], origin_P0[3], origin_R00[3], R00[9], rot_diff[9], Rs0[9];
    for (int k = 0; k < 9; k++) Rs0[k] = Rs[k];
    R2ypr(Rs0, origin_R0);
    for (int k = 0; k < 3; k++) origin_P0[k] = Ps[k];
    q_to_R(q_from_pose(pose), R00);
    R2ypr(R00, origin_R00);
    const double y_diff = origin_R0[0] - origin_R00[0];
    double ypr[3] = {y_diff, 0, 0};
    ypr2R(ypr, rot_diff);
    if (fabs(fabs(origin_R0[1]) - 90) < 1.0 || fabs(fabs(origin_R00[1]) - 90) < 1.0) m3_mul_nt(Rs0, R00, rot_diff);
    // ---- update() of the prior factors (pseudo-measurement shift), one lane each; they read the old Ps / Rs ----
    // (initFactorGraph creates its priors at the estimate and calls double2vector() only: do_update == 0)
    if (!do_update) {
    } else if (role == 0 && lane == 0) {
        // Linear9Factor::update  linear9_factor.h:60-68
        isv_linear9_t &f = d.lin9[w];
        for (int k = 0; k < 3; k++) {
            f.VB[k] += sb[9 * v + k] - Vs[3 * v + k];
            f.VB[3 + k] += sb[9 * v + 3 + k] - Bas[3 * v + k];
            f.VB[6 + k] += sb[9 * v + 6 + k] - Bgs[3 * v + k];
        }
    } else if (role == 0 && lane == 1) {
        // SE3PriorFactor::update  se3_prior_factor.h:73-81
        isv_se3_prior_t &f = d.se3[w];
        Quat R0 = q_from_R(Rs), R1 = q_normalized(q_from_pose(pose));
        double dR[3], E[9], Rn[9];
        so3_log(so3_mul(q_conj(R1), R0), dR);
        for (int k = 0; k < 3; k++) f.t[k] += pose[k] - Ps[k];
        q_to_R(so3_exp(dR), E); m3_mul(f.R, E, Rn);
        for (int k = 0; k < 9; k++) f.R[k] = Rn[k];
    } else if (role == 1) {
        // RelativePoseFactor::update (solver overload)  relative_pose_factor.h:103-117
        for (int i = rel0; i < d.Nvo - 1; i += rel_step) {
            isv_relpose_t &f = d.relpose[(size_t)w * (d.Nvo - 1) + i];
            const double *PSi = pose + 7 * i, *PSj = pose + 7 * (i + 1);
            const double *ti = Ps + 3 * i, *tj = Ps + 3 * (i + 1), *Ri = Rs + 9 * i, *Rj = Rs + 9 * (i + 1);
            Quat Qi = q_from_pose(PSi), Qj = q_from_pose(PSj);
            double d_tj[3], d_ti[3], A[9], Bm[9], Qm[9];
            for (int k = 0; k < 3; k++) { d_tj[k] = PSj[k] - tj[k]; d_ti[k] = PSi[k] - ti[k]; }
            q_to_R(q_inv(Qj), Qm); m3_mul(Qm, Rj, A); Quat d_Rj = q_from_R(A);
            q_to_R(q_inv(Qi), Qm); m3_mul(Qm, Ri, Bm); Quat d_Ri = q_from_R(Bm);
            double lgi[3], lgj[3], v1[3], v2[3], S[9], v3[3];
            so3_log(d_Ri, lgi); so3_log(d_Rj, lgj);
            m3tv(Ri, d_tj, v1); m3tv(Ri, d_ti, v2);
            skew3(f.delta_t, S); m3v(S, lgi, v3);
            for (int k = 0; k < 3; k++) f.delta_t[k] += v1[k] - v2[k] + v3[k];
            double Ji[9], ww[3], E[9], T[9];
            q_to_R(q_mul(q_inv(Qj), Qi), Ji);
            for (int k = 0; k < 9; k++) Ji[k] = -Ji[k];
            m3v(Ji, lgi, ww);
            q_to_R(so3_exp(ww), E); m3_mul(f.delta_R, E, T); for (int k = 0; k < 9; k++) f.delta_R[k] = T[k];
            q_to_R(so3_exp(lgj), E); m3_mul(f.delta_R, E, T); for (int k = 0; k < 9; k++) f.delta_R[k] = T[k];
        }
    } else if (role == 2) {
        // RollPitchFactor::update  rollpitch_factor.h:78-83
        for (int m = rp0; m < d.n_rp[w]; m += rp_step) {
            isv_rollpitch_t &f = d.rollpitch[(size_t)w * d.max_rp + m];
            const int idx = f.index;
            Quat R0 = q_from_R(Rs + 9 * idx), R1 = q_normalized(q_from_pose(pose + 7 * idx));
            double dR[3], E[9], T[9];
            so3_log(so3_mul(q_conj(R1), R0), dR);
            q_to_R(so3_exp(dR), E); m3_mul(f.R, E, T); for (int k = 0; k < 9; k++) f.R[k] = T[k];
        }
    }
    __syncthreads();                       // every update has read the old window states and written its prior
    // ---- double2vector, part 2 ----------------------------------------------------------------
    if (t == 0) {
        double tt[3];
        m3v(rot_diff, d.lin9[w].VB + 6, tt); for (int k = 0; k < 3; k++) d.lin9[w].VB[6 + k] = tt[k];     // :549 (gyro-bias slot)
    } else if (t == 1) {
        double Rn[9];
        m3_mul(rot_diff, d.se3[w].R, Rn); for (int k = 0; k < 9; k++) d.se3[w].R[k] = Rn[k];               // :550
    } else if (ex_lane) {
        // tic / ric <- para_Ex_Pose (:577-586); when the extrinsic is estimated the solved block is the pseudo-frame's
        // pose, which also becomes d.ex (MargForward linearises at it, and the caller reads para_Ex_Pose from it)
        double *exw = d.ex + (size_t)w * 7;
        if (d.est_ex) for (int k = 0; k < 7; k++) exw[k] = pose[7 * d.Nr + k];
        for (int k = 0; k < 3; k++) d.tic[(size_t)w * 3 + k] = exw[k];
        q_to_R(q_from_pose(exw), d.ric + (size_t)w * 9);
    }
    const double p0[3] = {pose[0], pose[1], pose[2]};
    for (int i = t; i < d.Nr; i += NT) {               // (the real frames: the pseudo-frame is not a body pose)
        double Ri[9], dd[3], tt[3], Ro[9];
        q_to_R(q_normalized(q_from_pose(pose + 7 * i)), Ri);
        m3_mul(rot_diff, Ri, Ro);
        for (int k = 0; k < 9; k++) Rs[9 * i + k] = Ro[k];
        for (int k = 0; k < 3; k++) dd[k] = pose[7 * i + k] - p0[k];
        m3v(rot_diff, dd, tt);
        for (int k = 0; k < 3; k++) Ps[3 * i + k] = tt[k] + origin_P0[k];
        m3v(rot_diff, sb + 9 * i, tt);
        for (int k = 0; k < 3; k++) { Vs[3 * i + k] = tt[k]; Bas[3 * i + k] = sb[9 * i + 3 + k]; Bgs[3 * i + k] = sb[9 * i + 6 + k]; }
    }
    for (int l = d.lm_off[w] + t; l < d.lm_off[w + 1]; l += NT) {        // FeatureManager::setDepth :145-163
        const double dep = 1.0 / d.lam[l];
        d.depth[l] = dep;
        d.solve_flag[l] = (dep < 0 || dep > 10) ? 2 : 1;
    }
    if (clear_marg) {                      // (as k_marg_clear: padding included, so that downloads are deterministic)
        double *z = reinterpret_cast<double *>(&d.marg[w]);
        for (int e = t; e < (int)(sizeof(isv_marg_result_t) / sizeof(double)); e += NT) z[e] = 0.0;
    }
}
template __global__ void k_finalize<64>(DevBatch, int, int);
template __global__ void k_finalize<256>(DevBatch, int, int);

// ------------------------------------------------------------------------------------------
// host side
#define HCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { err = std::string(#call) + ": " + hipGetErrorString(e_); return ISV_ERR_DEVICE; } } while (0)

template <typename T>
static int dal(T **p, size_t n, std::vector<void *> &allocs, std::string &err) {
    void *q = nullptr;
    HCHK(hipMalloc(&q, (n ? n : 1) * sizeof(T)));
    allocs.push_back(q);
    *p = (T *)q;
    return ISV_OK;
}
#define TRYA(x) do { int rc_ = (x); if (rc_ != ISV_OK) return rc_; } while (0)
// the dynamic-LDS attribute is per kernel and device and process-wide: raised to the largest size asked for and never lowered,
// so that handles of different shapes and the entry points sharing a kernel do not lower each other's value
hipError_t isv_raise_dynamic_lds(const void *fn, int device, size_t lds) {
    static std::mutex mtx;
    static std::map<std::pair<const void *, int>, size_t> raised;
    std::lock_guard<std::mutex> lk(mtx);
    size_t &cur = raised[{fn, device}];
    if (lds <= cur) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) cur = lds;
    return e;
}
// ---- the handle: environment, device, plan, allocations, kernel table ---------------------------------------------------------
// every environment hook of the solver, read at handle creation
static SolveEnv solve_env_read() {
    auto on = [](const char *name) { return getenv(name) != nullptr; };
    auto tri = [](const char *name) { const char *v = getenv(name); return v ? (atoi(v) != 0 ? 1 : 0) : -1; };
    SolveEnv e;
    e.one_stream = on("ISV_ONE_STREAM"); e.split_control = on("ISV_SPLIT_CONTROL"); e.generic_n = on("ISV_GENERIC_N");
    e.lg_batch_waves = on("ISV_LG_BATCH_WAVES"); e.debug_sw_global = on("ISV_DEBUG_SW_GLOBAL"); e.legacy_visual = on("ISV_LEGACY_VISUAL");
    e.no_split = on("ISV_NO_SPLIT"); e.no_update = on("ISV_DEBUG_NO_UPDATE"); e.no_pose_dogleg = on("ISV_NO_POSE_DOGLEG");
    e.marg_one_kernel = on("ISV_MARG_ONE_KERNEL"); e.marg_split = on("ISV_MARG_SPLIT"); e.tail_one_wave = on("ISV_TAIL_ONE_WAVE");
    e.r1_dense = on("ISV_R1_DENSE"); e.bsub_in_dogleg = on("ISV_BSUB_IN_DOGLEG"); e.debug_path = on("ISV_DEBUG_PATH");
    e.solve_st = tri("ISV_SOLVE_ST"); e.chain_split = tri("ISV_CHAIN_SPLIT");
    return e;
}

// the instantiation behind a role's enum: the only place that names them
template <int MODE> static const void *solve_sb_kernel(KernelInst i) {
    return i == SB_N11 ? (const void *)k_build_solve_sb<false, 11, MODE> : i == SB_RT ? (const void *)k_build_solve_sb<false, 0, MODE> : (const void *)k_build_solve_sb<true, 0, MODE>;
}
// the landmark elimination's kernels for NT 16-column tiles: TPW tiles per wavefront (the plan's thread count follows the same rule)
template <int NT> static const void *rank1_kernel(SolverRole r, bool ex) {
    constexpr int TPW = NT <= 5 ? 1 : NT <= 7 ? 2 : 3;
    if (r == KR_RANK1_SPLIT) return (const void *)k_rank1_split<NT, TPW>;
    if (r == KR_SCHUR_SPLIT) return (const void *)k_schur_split<NT, TPW>;
    return ex ? (const void *)k_rank1_mfma<NT, TPW, 64, 1, true> : (const void *)k_rank1_mfma<NT, TPW, 64, 1, false>;
}
const void *isv_solver_kernel(SolverRole r, KernelInst i, bool ex, int nt) {
    static const void *(*const rank1_for_nt[8])(SolverRole, bool) = {rank1_kernel<1>, rank1_kernel<2>, rank1_kernel<3>, rank1_kernel<4>,
                                                                     rank1_kernel<5>, rank1_kernel<6>, rank1_kernel<7>, rank1_kernel<8>};
    if (i == KI_NONE) return nullptr;
    switch (r) {
    case KR_SOLVE:
        if (i == KI_DENSE) return (const void *)k_build_solve;
        if (i == ST_N11) return (const void *)k_build_solve_st<false, 11>;
        if (i == ST_RT) return (const void *)k_build_solve_st<false, 0>;
        if (i == ST_N18) return (const void *)k_build_solve_st<true, 18>;
        if (i == ST_BIG) return (const void *)k_build_solve_st<true, 0>;
        return solve_sb_kernel<0>(i);
    case KR_CHAIN: return solve_sb_kernel<1>(i);
    case KR_POSE: return solve_sb_kernel<2>(i);
    case KR_LIN_GRAM_CHAIN:
        if (ex) return i == LGC_RT ? (const void *)k_lin_gram_chain<true, false, 0, 0> : (const void *)k_lin_gram_chain<true, true, 0, 0>;
        return i == LGC_N11 ? (const void *)k_lin_gram_chain<false, false, 11, 0> : i == LGC_RT ? (const void *)k_lin_gram_chain<false, false, 0, 0> : (const void *)k_lin_gram_chain<false, true, 0, 0>;
    case KR_LIN_GRAM_CHAIN_R1: return (const void *)k_lin_gram_chain<false, true, 0, 7>;
    case KR_POSE_DOGLEG: return ex ? (const void *)k_pose_dogleg<false, 0, true> : i == PD_N11 ? (const void *)k_pose_dogleg<false, 11, false> : (const void *)k_pose_dogleg<false, 0, false>;
    case KR_RANK1: case KR_RANK1_SPLIT: case KR_SCHUR_SPLIT: return rank1_for_nt[nt - 1](r, ex);     // (lds_T: wd_ld <= 128, so 1 <= nt <= 8)
    case KR_LIN_GRAM: return ex ? (const void *)k_lin_gram<true, LG_WAVES> : (const void *)k_lin_gram<false, LG_WAVES>;
    case KR_LIN_GRAM_SMALL: return ex ? (const void *)k_lin_gram<true, LG_WAVES_SMALL> : (const void *)k_lin_gram<false, LG_WAVES_SMALL>;
    case KR_DOGLEG: return ex ? (const void *)k_dogleg<false, true> : (const void *)k_dogleg<false, false>;
    case KR_DOGLEG_CONTROL: return ex ? (const void *)k_dogleg<true, true> : (const void *)k_dogleg<true, false>;
    case KR_STEP_CONTROL: return ex ? (const void *)k_step_control<true, true> : (const void *)k_step_control<true, false>;
    case KR_SWEEP: return (const void *)k_sweep_mfma;
    case KR_FRONT: return (const void *)k_front;
    default: return nullptr;
    }
}

int isv_solver_alloc(DevBatch &d, SolverHost &hc, size_t B, size_t L, size_t F, std::vector<void *> &allocs, std::string &err) {
    // 1. the environment, 2. the device: compute units, and the workgroups of k_dogleg<true, EX> per CU by registers alone (a small
    // dynamic LDS request; the LDS bound is applied per upload)
    hc.env = solve_env_read();
    int dev0 = 0, per_cu = 0;
    HCHK(hipGetDevice(&dev0));
    if (hipDeviceGetAttribute(&hc.dev.n_cus, hipDeviceAttributeMultiprocessorCount, dev0) != hipSuccess) { (void)hipGetLastError(); hc.dev.n_cus = 0; }
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, isv_solver_kernel(KR_DOGLEG_CONTROL, KI_PLAIN, d.est_ex != 0, 0), 256, 1024) != hipSuccess) { (void)hipGetLastError(); per_cu = 0; }
    hc.dev.dogleg_per_cu_regs = per_cu;
    // 3. the sizes that live beside their kernels, 4. the plan
    SolveShape shape;
    shape.N = d.N; shape.Nr = d.Nr; shape.est_ex = d.est_ex; shape.n_prior_slots = d.n_prior_slots; shape.prior_H_sz = d.prior_H_sz; shape.max_lm = d.max_lm; shape.max_batch = B;
    SolveSizes sz;
    sz.build_solve_sb_bytes = build_solve_sb_bytes(d.N, d.prior_H_sz); sz.build_solve_st_bytes = build_solve_st_bytes(d.N, d.prior_H_sz);
    sz.build_solve_lds_bytes = build_solve_lds_bytes(d.N); sz.front_lds_bytes = front_lds_bytes(d.N, d.n_prior_slots);
    sz.build_solve_st_ws_doubles = build_solve_st_ws_doubles(d.N); sz.build_solve_cs_doubles = build_solve_cs_doubles(d.N);
    hc.plan = plan_handle(shape, hc.env, hc.dev, sz);
    const HandlePlan &p = hc.plan;
    if (hc.env.debug_path) {
        char line[512];
        plan_format_lds(line, sizeof(line), p); fputs(line, stderr);
        plan_format_solve_st(line, sizeof(line), p); fputs(line, stderr);
        plan_format_handle(line, sizeof(line), p, hc.env); fputs(line, stderr);
    }
    // 5. what the plan names
    d.tvis_sz = p.tvis_sz; d.wd_ld = p.wd_ld; d.lds_T = p.lds_T ? 1 : 0; d.r1_dense = p.r1_dense ? 1 : 0; d.split_cap = p.split_cap;
    d.sw_global = 0; d.marg_scratch_sz = 26;
    d.sw_part = nullptr; d.st_ws = nullptr; d.cs_ws = nullptr; d.r1_part = nullptr;
    const size_t n = d.np, NI = B * (d.N - 1);
    TRYA(dal(&d.scale_p, B * n, allocs, err)); TRYA(dal(&d.diag_p, B * n, allocs, err)); TRYA(dal(&d.grad_p, B * n, allocs, err));
    TRYA(dal(&d.gn_p, B * n, allocs, err)); TRYA(dal(&d.delta_p, B * n, allocs, err)); TRYA(dal(&d.zp, B * n, allocs, err)); TRYA(dal(&d.up, B * n, allocs, err));
    TRYA(dal(&d.lmE, L, allocs, err)); TRYA(dal(&d.lmG, L, allocs, err)); TRYA(dal(&d.scale_l, L, allocs, err)); TRYA(dal(&d.diag_l, L, allocs, err));
    TRYA(dal(&d.grad_l, L, allocs, err)); TRYA(dal(&d.gn_l, L, allocs, err)); TRYA(dal(&d.delta_l, L, allocs, err)); TRYA(dal(&d.lm_aterm, L, allocs, err));
    TRYA(dal(&d.fcost_c, F, allocs, err)); TRYA(dal(&d.imu_cost_c, NI, allocs, err)); TRYA(dal(&d.prior_cost_c, B * (size_t)d.n_prior_slots, allocs, err)); TRYA(dal(&d.cost_c, B, allocs, err));
    TRYA(dal(&d.fmodel, F, allocs, err)); TRYA(dal(&d.imu_model, NI, allocs, err)); TRYA(dal(&d.prior_model, B * (size_t)d.n_prior_slots, allocs, err)); TRYA(dal(&d.model, B, allocs, err));
    // (the traces, d.marg, d.margin_old, d.header0: transfer buffers, placed by the caller -- isv_batch_buffers.h)
    TRYA(dal(&d.W, (F + L) * 6, allocs, err)); TRYA(dal(&d.lm_cg, L, allocs, err));
    TRYA(dal(&d.Tvis, B * (size_t)d.tvis_sz, allocs, err));
    TRYA(dal(&d.dbg, B * 64, allocs, err)); TRYA(dal(&d.act, ISV_MAX_TRACE, allocs, err));
    HCHK(hipMemset(d.dbg, 0, B * 64 * sizeof(double)));
    TRYA(dal(&d.Tglob, p.lds_T ? 1 : B * ((size_t)d.N * (d.N + 1) / 2 * 225), allocs, err));
    if (p.has_sw_part) TRYA(dal(&d.sw_part, B * p.n_pairs * 84, allocs, err));
    if (p.solve_st) TRYA(dal(&d.st_ws, B * sz.build_solve_st_ws_doubles, allocs, err));
    if (p.chain_split) {       // (entries above the diagonal of a diagonal block are never written: finite)
        TRYA(dal(&d.cs_ws, B * sz.build_solve_cs_doubles, allocs, err));
        HCHK(hipMemset(d.cs_ws, 0, B * sz.build_solve_cs_doubles * sizeof(double)));
    }
    if (p.r1_groups) TRYA(dal(&d.r1_part, B * p.r1_groups * (size_t)(p.nt * (p.nt + 1) / 2) * 256, allocs, err));
    TRYA(dal(&d.marg_scratch, L * 26, allocs, err));
    TRYA(dal(&d.marg_ws, B * ISV_MARG_WS, allocs, err));
    // 6. the kernel table, 7. the dynamic-LDS attributes
    for (int r = 0; r < KR_COUNT; r++) {
        hc.fn[r] = isv_solver_kernel((SolverRole)r, p.roles[r].inst, d.est_ex != 0, p.nt);
        HCHK(isv_raise_dynamic_lds(hc.fn[r], dev0, p.roles[r].lds));
    }
    return ISV_OK;
}

UploadPlan isv_solver_plan_upload(SolverHost &hc, const UploadShape &u) {
    hc.upload = u;
    return plan_upload(hc.plan, hc.dev, hc.env, u);
}

// launch role r with the arguments a: the runtime receives the same kernel handle as from hipLaunchKernelGGL of the
// instantiation, and a failed launch surfaces at the enqueue's closing hipGetLastError like theirs
template <typename... A> static void launch(const SolverHost &hc, SolverRole r, dim3 grid, size_t lds, hipStream_t s, A... a) {
    void *args[] = {&a...};
    (void)hipLaunchKernel(hc.fn[r], grid, dim3(hc.plan.roles[r].threads), args, lds, s);
}

// Enqueues the resident upload's solve by its plan (plan_upload, isv_solve_plan.h: every choice, grid and LDS size below is a field of it).
// prof_ev (optional): [max_iter][ISV_PROF_FAMILIES][2] events recorded around the three dominant
// kernel families on the solve stream, so bench.py can report per-kernel durations measured live.
int isv_solver_enqueue(DevBatch &d, const SolverHost &hc, hipStream_t st, hipStream_t st2, hipEvent_t *fj, int64_t *counts, hipEvent_t *prof_ev, std::string &err) {
    // st2 / fj[4]: side stream + fork/join events: the IMU and prior factor kernels are latency-bound and
    // independent of the reprojection pipeline, so they run beside it and are joined before their consumers
#define PROF(slot, fam, which) do { if (prof_ev) (void)hipEventRecord(prof_ev[((slot) * ISV_PROF_FAMILIES + (fam)) * 2 + (which)], st); } while (0)
    UploadShape shape = hc.upload;
    shape.init_mode = d.init_mode;
    const UploadPlan p = plan_upload(hc.plan, hc.dev, hc.env, shape);
    const RolePlan *K = hc.plan.roles;
    const unsigned B = (unsigned)p.B;
    d.ctl_stage_lm = p.ctl_stage_lm ? 1 : 0; d.dg_stage_ph = p.dg_stage_ph ? 1 : 0; d.sw_global = p.sw_global ? 1 : 0; d.bs_split = p.bsub_split ? 1 : 0;
    d.bsub_in_solve = p.bsub_in_solve ? 1 : 0;
    if (hc.env.debug_path) { char line[512]; plan_format_enqueue(line, sizeof(line), p); fputs(line, stderr); }
    if (hc.env.one_stream) st2 = st;            // diagnostics: serialise everything on one stream (per-kernel timelines)
    hipLaunchKernelGGL(k_init_state, dim3(p.grid_init_state), dim3(64), 0, st, d);
    for (int slot = 0; slot < d.max_iter; slot++) {
        // linearise where needed (k_*_linearize skip windows whose need_linearize == 0 via the tile/window flags)
        // Small-batch handles (chain_split: every workgroup of every kernel finds a CU of its own) run the whole iteration on ONE
        // stream: an event record costs the critical stream ~7 us and a wait that really blocks ~13 us on this GPU (measured, rocprofv3
        // kernel trace of one window), more than the kernels they would overlap.  Instead, independent work shares a LAUNCH:
        // k_front = {IMU factors | prior factors} of every window, k_lin_gram_chain = {k_lin_gram | chain half of the split solve}.
        // An upload k_lin_gram_chain does not take (windows beyond the fused kernel's limits: BASELINE config 5's 30 000 factors) runs
        // the chain half (~75 us at 20 frames) on the side stream beside the linearisation and the split elimination -- worth its fork /
        // join events there (on the solve stream behind them it made the one-launch solve's 142 us into 75 + 75)
        if (p.chain_split) {
            launch(hc, KR_FRONT, dim3(B, 2), K[KR_FRONT].lds, st, d);
            if (!p.lg_chain) {
                HCHK(hipEventRecord(fj[0], st)); HCHK(hipStreamWaitEvent(st2, fj[0], 0));
                launch(hc, KR_CHAIN, dim3(B), K[KR_CHAIN].lds, st2, d);
                HCHK(hipEventRecord(fj[1], st2));
            }
        } else {
            HCHK(hipEventRecord(fj[0], st)); HCHK(hipStreamWaitEvent(st2, fj[0], 0));
            if (p.has_imu) {
                hipLaunchKernelGGL(k_imu_raw, dim3(p.grid_imu_raw), dim3(256), 0, st2, d, d.pose, d.sb, 1);
                hipLaunchKernelGGL(k_imu_weight, dim3(p.grid_imu_weight), dim3(256), 0, st2, d, d.imu_cost, 1);
            }
            hipLaunchKernelGGL(k_prior_linearize<true>, dim3(B), dim3(64), p.lds_prior, st2, d, d.pose, d.sb, d.prior_cost, 1);
            HCHK(hipEventRecord(fj[1], st2));
        }
        PROF(slot, 0, 0);
        if (p.fused) {
            // linearisation fused with the Gram products: no Jacobian strip goes to HBM (isv_visual.hip)
            // (eight wavefronts per window while the batch leaves every window a CU of its own: 41 -> 27 us per launch for one window)
            launch(hc, p.visual_role, dim3(B, p.lg_chain ? 2 : 1), p.lds_visual, st, d);
            counts[ISV_CNT_LINEARIZE]++; counts[ISV_CNT_FUSED_VISUAL] = 1;
        } else if (p.has_tiles) { hipLaunchKernelGGL(k_proj_linearize<0>, dim3(p.grid_tiles), dim3(256), p.lds_proj, st, d, d.pose, d.lam, d.fcost, 1); counts[ISV_CNT_LINEARIZE]++; }
        PROF(slot, 0, 1);
        if (p.split) {
            // a SMALL batch with LONG windows: one window's elimination over many CUs (k_schur_split + k_schur_fold, isv_sweep.hip)
            const dim3 grid(B, p.grid_split_y);
            PROF(slot, 1, 0);
            if (p.fused) launch(hc, KR_RANK1_SPLIT, grid, K[KR_RANK1_SPLIT].lds, st, d, p.GrMax);          // the downdates alone: the lean kernel (two workgroups per CU)
            else launch(hc, KR_SCHUR_SPLIT, grid, K[KR_SCHUR_SPLIT].lds, st, d, p.Gs, p.GrMax);
            PROF(slot, 1, 1);
            PROF(slot, 2, 0);
            hipLaunchKernelGGL(k_schur_fold, dim3(B, p.grid_fold_y), dim3(256), 0, st, d, p.GrMax, hc.plan.nt, p.fused ? 0 : 1);
            PROF(slot, 2, 1);
            counts[ISV_CNT_ELIM]++; counts[ISV_CNT_SPLIT_GROUPS] = p.GrMax;
        } else if (p.lds_T) {
            // landmark elimination: Gram products of the pose Jacobians, then the rank-1 downdates (both FP64 MFMA)
            PROF(slot, 1, 0);
            if (!p.fused) launch(hc, KR_SWEEP, dim3(B), p.lds_sweep, st, d);
            counts[ISV_CNT_ELIM]++;
            PROF(slot, 1, 1);
            // one workgroup per window: nt(nt+1)/2 tile wavefronts, w vectors expanded to panel rows in LDS
            PROF(slot, 2, 0);
            if (!p.r1_in_lg) launch(hc, KR_RANK1, dim3(B), K[KR_RANK1].lds, st, d);
            PROF(slot, 2, 1);
        }
        if (!p.lg_chain) HCHK(hipStreamWaitEvent(st, fj[1], 0));
        if (!p.lds_T) hipLaunchKernelGGL(k_cost_reduce, dim3(B), dim3(256), 0, st, d, d.fcost, d.imu_cost, d.prior_cost, d.cost, 1);   // (k_build_solve_sb sums the cost itself)
        PROF(slot, 3, 0);
        // the whole reduced solve, or on chain-split handles its pose half (the chain half ran beside k_lin_gram), with the dogleg
        // and the step control when they fit one launch
        launch(hc, p.solve_role, dim3(B), p.lds_solve, st, d);
        if (p.pose_dogleg) counts[ISV_CNT_FUSED_CONTROL] = 1;
        if (p.solve_st) counts[ISV_CNT_SOLVE_ST] = 1;
        counts[ISV_CNT_SOLVE]++;
        PROF(slot, 3, 1);
        PROF(slot, 4, 0);
        if (p.bsub_split) hipLaunchKernelGGL(k_backsub_split, dim3(B, p.grid_backsub_y), dim3(128), p.lds_backsub, st, d);
        if (p.pose_dogleg) {
        } else if (p.fuse_control) {
            launch(hc, KR_DOGLEG_CONTROL, dim3(B), p.lds_dogleg, st, d);
            counts[ISV_CNT_FUSED_CONTROL] = 1;
        } else launch(hc, KR_DOGLEG, dim3(B), p.lds_dogleg, st, d);
        PROF(slot, 4, 1);
        if (!p.lds_T) {                    // (the LDS path evaluates these inside k_dogleg)
            HCHK(hipEventRecord(fj[2], st)); HCHK(hipStreamWaitEvent(st2, fj[2], 0));
            if (p.has_imu) hipLaunchKernelGGL(k_imu_linearize<false>, dim3(p.grid_imu_c), dim3(64), 0, st2, d, d.cpose, d.csb, d.imu_cost_c, 2);
            hipLaunchKernelGGL(k_prior_linearize<false>, dim3(B), dim3(64), p.lds_prior_c, st2, d, d.cpose, d.csb, d.prior_cost_c, 2);
            hipLaunchKernelGGL(k_model_imu_prior, dim3(p.grid_model), dim3(64), 0, st2, d);
            HCHK(hipEventRecord(fj[3], st2));
        }
        // candidate evaluation of the reprojection factors: inside the per-window control kernel, unless the windows are
        // so large that one workgroup per window would serialise it (config 5: 30 000 factors in one window)
        PROF(slot, 5, 0);
        if (p.fuse_control) {
        } else if (p.control_in_wg) launch(hc, KR_STEP_CONTROL, dim3(B), p.lds_step_control, st, d);
        else {
            if (p.has_tiles) hipLaunchKernelGGL(k_proj_linearize<1>, dim3(p.grid_tiles), dim3(256), p.lds_proj_c, st, d, d.cpose, d.clam, d.fcost_c, 2);
            if (!p.lds_T) HCHK(hipStreamWaitEvent(st, fj[3], 0));
            hipLaunchKernelGGL((k_step_control<false, false>), dim3(B), dim3(256), 0, st, d);
        }
        PROF(slot, 5, 1);
    }
    // The tail is bound by the window's latency (the GPU is almost idle: a wavefront per window and SIMD in the one-wavefront
    // forms), so k_finalize and MargBackward give a window four wavefronts and run its independent serial chains side by side;
    // the marginalisation record is cleared at the end of k_finalize (ISV_TAIL_ONE_WAVE: the one-wavefront forms and k_marg_clear).
    if (p.init_mode) hipLaunchKernelGGL(k_init_priors, dim3(B), dim3(64), 0, st, d, d.init_scratch, d.init_per_window, d.init_kld);      // Estimator::initFactorGraph: first priors from the solved estimate, then double2vector
    if (p.finalize_wide) hipLaunchKernelGGL(k_finalize<256>, dim3(B), dim3(256), 0, st, d, p.do_update, p.clear_marg);
    else hipLaunchKernelGGL(k_finalize<64>, dim3(B), dim3(64), 0, st, d, p.do_update, 0);
    if (p.init_mode) {
        HCHK(hipGetLastError());
        return ISV_OK;
    }
    if (!p.finalize_wide) hipLaunchKernelGGL(k_marg_clear, dim3(B), dim3(64), 0, st, d);
    // MargForward and MargBackward are independent: run them side by side.  The longer one (backward) goes on the main stream
    // so that it is dispatched FIRST: whichever kernel arrives second runs its last workgroups after the first one's when four
    // workgroups of each per CU do not fit together.  They do fit: LDS 4 x 24.4 KB (k_marg_bwd<3>) + 4 x 14.1 KB (k_marg_fwd<64>)
    // of 160 KB, registers 4 x 80 + 160 of a SIMD's 512 (k_marg_bwd<3> is held to 80 by its launch bounds).
    // Measured, 1024 windows of 11 frames / 300 landmarks, per launch (rocprofv3 kernel trace of the benchmark; the one-wavefront
    // tail first): k_finalize + k_marg_clear 37.5 + 4.7 -> k_finalize<256> 31.8 us; MargBackward 307 (k_marg_bwd<2>) -> 221 us
    // (k_marg_bwd<3>; per window, in-kernel stamps: build 30.5 -> 25.1, eigen-decomposition 179 -> 104, projections 31 -> 16,
    // KLD 26 -> 18); k_marg_fwd<64> beside it 148 -> 201 us and still ends 13 us before it; k_finalize's start to the later end
    // 357 -> 259 us; step 5.146 -> 5.046 ms.  One window 1.59 -> 1.54 ms, 128 windows 1.88 -> 1.85 ms: the four-wavefront launch
    // is the default for every batch size.  (The one-wavefront forms, B = 1 / 64 / 256 / 512: 1.95 / 2.27 / 2.47 / 3.16 ms with the
    // eigen-decomposition as a launch of its own against 1.98 / 2.35 / 2.55 / 3.25 with the one launch <2>.)
    HCHK(hipEventRecord(fj[0], st)); HCHK(hipStreamWaitEvent(st2, fj[0], 0));
    if (p.marg_bwd == MARG_BWD_FOUR_WAVES) hipLaunchKernelGGL(k_marg_bwd<3>, dim3(B), dim3(256), 0, st, d);
    else if (p.marg_bwd == MARG_BWD_ONE_LAUNCH) hipLaunchKernelGGL(k_marg_bwd<2>, dim3(B), dim3(64), 0, st, d);
    else {
        hipLaunchKernelGGL(k_marg_bwd<0>, dim3(B), dim3(64), 0, st, d);
        hipLaunchKernelGGL(k_marg_jacobi<21>, dim3(B), dim3(256), 0, st, d);
        hipLaunchKernelGGL(k_marg_bwd<1>, dim3(B), dim3(64), 0, st, d);
    }
    if (p.marg_fwd_wide) hipLaunchKernelGGL(k_marg_fwd<256>, dim3(B), dim3(256), 0, st2, d);
    else hipLaunchKernelGGL(k_marg_fwd<64>, dim3(B), dim3(64), 0, st2, d);
    HCHK(hipEventRecord(fj[1], st2));
    HCHK(hipStreamWaitEvent(st, fj[1], 0));
    HCHK(hipGetLastError());
    return ISV_OK;
}

// the result records of n solved windows, array by array: the summaries' (if asked for), the marginalisation records (if asked for);
// synchronises the handle's stream and unpacks them
int isv_solver_download(isv_backend *h, int n, isv_summary_t *summary, isv_marg_result_t *marg) {
    if (!summary && !marg) return ISV_OK;
    std::string &err = h->err;
    HCHK(copy_batch_buffers(h, BatchDims{(size_t)n, 0, 0, 0, 0}, (summary ? BUF_SUMMARY : 0u) | (marg ? BUF_MARG : 0u), 0, false));
    HCHK(hipStreamSynchronize(h->stream));
    for (int b = 0; b < n; b++) isv_solver_unpack_window(h->stage, b, summary ? &summary[b] : nullptr, marg ? &marg[b] : nullptr);
    return ISV_OK;
}

// window b's records out of the staging area (isv_batch_download's host threads call it per window; isv_solver_download for all)
void isv_solver_unpack_window(const SolverStage &g, int b, isv_summary_t *summary, isv_marg_result_t *marg) {
    if (marg) *marg = g.marg[b];
    if (summary) {
        isv_summary_t &s = *summary;
        memset(&s, 0, sizeof(s));
        s.status = ISV_OK; s.termination = g.st[b].termination; s.iterations = g.st[b].iteration; s.num_successful = g.st[b].num_successful;
        s.initial_cost = g.st[b].initial_cost; s.final_cost = g.st[b].x_cost;
        memcpy(s.trace_cost, &g.tc[(size_t)b * ISV_MAX_TRACE], sizeof(s.trace_cost));
        memcpy(s.trace_radius, &g.tr[(size_t)b * ISV_MAX_TRACE], sizeof(s.trace_radius));
        memcpy(s.trace_step_norm, &g.ts[(size_t)b * ISV_MAX_TRACE], sizeof(s.trace_step_norm));
        memcpy(s.trace_accepted, &g.ta[(size_t)b * ISV_MAX_TRACE], sizeof(s.trace_accepted));
        if (!(s.final_cost - s.final_cost == 0.0)) s.status = ISV_ERR_NONFINITE;
    }
}

// test hook: the step vectors of the last enqueue.  `count` is bounded by what the handle allocated (capB windows, capL landmarks):
// a wrong count from a test is an error, not a read past the buffer
int isv_solver_debug_read(DevBatch &d, hipStream_t st, int what, double *out, int64_t count, size_t capB, size_t capL, std::string &err) {
    const double *src = nullptr;
    const size_t per_p = capB * (size_t)d.np;
    size_t cap = 0;
    switch (what) {
    case 10: src = d.gn_p; cap = per_p; break;
    case 11: src = d.gn_l; cap = capL; break;
    case 12: src = d.grad_p; cap = per_p; break;
    case 13: src = d.grad_l; cap = capL; break;
    case 14: src = d.scale_p; cap = per_p; break;
    case 15: src = d.scale_l; cap = capL; break;
    case 16: src = d.diag_p; cap = per_p; break;
    case 17: src = d.delta_p; cap = per_p; break;
    case 18: src = d.delta_l; cap = capL; break;
    case 19: src = d.cost_c; cap = capB; break;
    case 20: src = d.model; cap = capB; break;
    case 21: src = d.dbg; cap = capB * 64; break;
    case 23: src = d.diag_l; cap = capL; break;
    default: return ISV_ERR_INVALID_ARG;
    }
    if (count < 0 || (size_t)count > cap) { err = "isv_debug_read: count exceeds the buffer"; return ISV_ERR_INVALID_ARG; }
    if (count == 0) return ISV_OK;
    HCHK(hipMemcpyAsync(out, src, sizeof(double) * count, hipMemcpyDeviceToHost, st));
    HCHK(hipStreamSynchronize(st));
    return ISV_OK;
}
