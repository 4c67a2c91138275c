// isv_solve_plan.h -- which kernels a handle and an upload run, as data.  plan_handle() decides once per handle (isv_solver_alloc
// allocates and fills the kernel table from it), plan_upload() once per uploaded batch (the two upload paths take lg_lcap and
// fused_visual from it, isv_solver_enqueue follows the rest).  Both are pure functions of plain integers: this header includes
// no HIP header, knows no DevBatch and no kernel, and compiles under a plain host compiler (tests/native/solve_plan_print.cpp
// runs the rules without a GPU).  The LDS size formulas the rules need live here, one definition each, for host and device.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define ISV_PLAN_HD __host__ __device__
#else
#define ISV_PLAN_HD
#endif

// ---- constants of the rules ---------------------------------------------------------------------------------------------
#define ISV_LDS_PER_CU ((size_t)160 * 1024)
#define ISV_CTL_STAGE_MAX_BYTES ((size_t)36 * 1024)      // the step control stages its landmarks only while four workgroups still share a CU
#define ISV_SPLIT_MAX_GROUPS 32       // workgroups one window's rank-1 downdates are split over (k_schur_split)
#ifndef ISV_SPLIT_MIN_PASSES
#define ISV_SPLIT_MIN_PASSES 4        // ... when it has at least this many 64-landmark passes (> 192 landmarks; measured on ONE 18-frame
                                      // window of 300 landmarks: 2.66 ms with 8, 2.52 ms with 4; 11 frames: 1.94 either way)
#endif
#define ISV_FUSED_MAX_FACTORS 8192   // longest window (reprojection factors) the one-workgroup-per-window k_lin_gram takes
#define ISV_SWEEP_WAVES 8
// wavefronts of k_lin_gram per window: LG_WAVES for batches (three workgroups per CU), LG_WAVES_SMALL while the batch leaves
// every window a CU of its own (each wavefront takes the pair groups of ISV_SWEEP_WAVES / LGW sweep wavefronts)
#define LG_WAVES 4
#define LG_WAVES_SMALL 8
#define ISV_WG_STATIC_LDS ((size_t)2304)      // k_dogleg's static reduction space, rounded up to the allocation granule

// ---- LDS sizes (bytes unless named otherwise) ---------------------------------------------------------------------------
static inline size_t plan_max(size_t a, size_t b) { return a > b ? a : b; }
static inline size_t plan_min(size_t a, size_t b) { return a < b ? a : b; }
// per-wave LDS of k_proj_linearize<MODE>: R,P per frame + extrinsic; MODE 0 adds a 64 x 15 transpose buffer, MODE 1 the poses at x and the tangent step
ISV_PLAN_HD inline size_t proj_lds_doubles_per_wave(int N, int mode) { return (size_t)N * 12 + 12 + (mode == 0 ? 64 * 15 : (size_t)N * 18); }
// (jac = false: the residual-only evaluation, see prior_linearize_body)
// + the window's prior factor records staged in LDS (round 3): SE3 49 + Linear9 91 + 49 per relative-pose / 14 per roll-pitch words
ISV_PLAN_HD static inline size_t prior_lds_bytes(int slots, bool jac = true) { return ((size_t)slots * (jac ? 82 + 90 : 10 + 10) + 140 + (size_t)(slots > 2 ? slots - 2 : 0) * 49) * sizeof(double); }
// bytes of the wave-private landmark lists of k_rank1_mfma's compacted downdates (isv_rank1.h): 64 per output-tile slot, and
// wavefronts x tiles per wavefront <= tiles + 3 slots for nt 16-column blocks
ISV_PLAN_HD inline size_t rank1_list_bytes(int nt) { return (size_t)(nt * (nt + 1) / 2 + 3) * 64; }
// k_rank1_mfma's panel (64 rows of wd_ld + 4) and its three per-landmark tables, without the lists
inline size_t rank1_panel_bytes(int wd_ld, int max_lm) { return (64 * (size_t)(wd_ld + 4) + (size_t)max_lm * 3 + 2) * sizeof(double); }
// k_sweep_mfma: the pair partials (unless they live in the global scratch) and the group starts
inline size_t sweep_lds_bytes(size_t n_pairs, bool partials_in_lds) { return ((partials_in_lds ? n_pairs * 84 : 0) + (n_pairs + 2) / 2 + 1) * sizeof(double); }
// k_lin_gram (isv_lin_gram.h): the factor staging row of a wavefront is lg_xld doubles per factor
ISV_PLAN_HD constexpr int lg_xld(bool ex) { return ex ? 39 : 27; }
inline size_t lin_gram_lds_bytes(int N /* real frames */, bool partials_in_lds, bool ex, int waves, int lcap) {
    const size_t NP = (size_t)N * (N - 1) / 2;
    return ((size_t)N * 12 + 12 + (size_t)waves * 16 * lg_xld(ex) + (partials_in_lds ? NP * 84 : 0) + (NP + 2) / 2 + 1 + (NP + 1) / 2 + 1 + 4 * (size_t)lcap) * sizeof(double);
}
// k_upload_build / k_seq_build: two ints per landmark slot and nine per frame pair
inline size_t upload_build_lds_bytes(int N, int lcap) { return ((size_t)2 * lcap + 9 * ((size_t)N * (N - 1) / 2 + 1)) * sizeof(int32_t); }
// dynamic LDS of k_dogleg (candidate-point IMU / prior evaluation on the LDS path + the two tangent vectors):
// + two 496-double staging rows for the IMU J^T J records of the model pieces and the tangent step (np)
// + the window's prior J^T J record (prior_H_sz) for the priors' model pieces while it is staged (stage_ph)
inline size_t dogleg_lds_bytes(int N, int n_prior_slots, int prior_H_sz, bool lds_T, bool stage_ph) {
    const size_t np = 15 * (size_t)N;
    return (lds_T ? ((size_t)(N - 1) * 48 + (size_t)n_prior_slots * 16 + 992 + np + (stage_ph ? (size_t)prior_H_sz : 0)) * sizeof(double) + prior_lds_bytes(n_prior_slots, false) : 0) + 2 * np * sizeof(double);
}
// the step control: candidate / current poses, the tangent step, and (stage_lm) the per-landmark data its factor loop gathers
// -- host point, candidate and current inverse depth, the landmark's step: 6 doubles each
inline size_t step_control_lds_bytes(int N, bool stage_lm, int lg_lcap) { return ((size_t)30 * N + 12 + (stage_lm ? 6 * (size_t)lg_lcap : 0)) * sizeof(double); }

// ---- inputs -------------------------------------------------------------------------------------------------------------
// the environment hooks the solver reads at handle creation (isv_solver.hip: solve_env_read)
struct SolveEnv {
    bool one_stream = false;          // ISV_ONE_STREAM: diagnostics, everything on one stream
    bool split_control = false;       // ISV_SPLIT_CONTROL: k_dogleg<false> + k_step_control
    bool generic_n = false;           // ISV_GENERIC_N: the run-time-N instantiations for every N
    bool lg_batch_waves = false;      // ISV_LG_BATCH_WAVES: never the eight-wavefront k_lin_gram
    bool debug_sw_global = false;     // ISV_DEBUG_SW_GLOBAL (test hook): give every LDS-path handle the global pair-partial scratch and use it for every launch
    bool legacy_visual = false;       // ISV_LEGACY_VISUAL: the unfused k_proj_linearize<0> + k_sweep_mfma pair
    bool no_split = false;            // ISV_NO_SPLIT: never spread one window's landmark elimination over several workgroups (k_schur_split)
    bool no_pose_dogleg = false;      // ISV_NO_POSE_DOGLEG (A/B and test hook): the pose half, the dogleg and the step control as separate launches (same bits)
    bool marg_one_kernel = false;     // ISV_MARG_ONE_KERNEL / ISV_MARG_SPLIT force MargBackward as one launch (k_marg_bwd<2>) or as build / k_marg_jacobi /
    bool marg_split = false;          // project, whatever the batch size (default: k_marg_bwd<3>, one launch of four wavefronts per window); all bitwise equal (tested)
    bool tail_one_wave = false;       // ISV_TAIL_ONE_WAVE (A/B and test hook): the one-wavefront tail -- k_finalize<64> + k_marg_clear, and MargBackward as
                                      // k_marg_bwd<2> (max_batch > 3 n_cus) or build / k_marg_jacobi / project -- in place of k_finalize<256> and k_marg_bwd<3> (same bits)
    bool r1_dense = false;            // ISV_R1_DENSE (A/B and test hook): k_rank1_mfma's dense MFMA loop, every landmark through every tile (same bits)
    bool bsub_in_dogleg = false;      // ISV_BSUB_IN_DOGLEG (A/B and test hook): the landmark back-substitution stays in k_dogleg, never inside k_build_solve_st (same bits)
    bool no_update = false;           // ISV_DEBUG_NO_UPDATE (sensitivity study, tests/test_sequence_long.py; the oracle has the same hook): skip the update() of
                                      // the prior factors' pseudo-measurements after the solve (src/estimator.cpp:1133-1144).  NOT the reference's behaviour.
    bool debug_path = false;          // ISV_DEBUG_PATH: stderr lines naming the handle's and every enqueue's kernel choices (tests assert them)
    int solve_st = -1;                // ISV_SOLVE_ST and ISV_CHAIN_SPLIT force their choice: -1 unset (the rule decides), 0 off, 1 on
    int chain_split = -1;
};
// what the handle was created with (N: device frames = Nr + est_ex; max_batch is the handle's capacity: kernel VARIANTS whose results
// differ in the last bits are chosen from it, never from the uploaded batch size, so a window gives the same bits alone and inside
// any batch of the same handle)
struct SolveShape { int N = 0, Nr = 0, est_ex = 0, n_prior_slots = 0, prior_H_sz = 0, max_lm = 0; size_t max_batch = 0; };
// the device: compute units, and workgroups of k_dogleg<true, EX> per CU by registers (the LDS bound is applied per upload)
struct SolveDevice { int n_cus = 0, dogleg_per_cu_regs = 0; };
// per-handle sizes whose formulas stay beside their kernels (isv_solver_alloc fills them; the plan takes them as given)
struct SolveSizes { size_t build_solve_sb_bytes = 0, build_solve_st_bytes = 0, build_solve_lds_bytes = 0, front_lds_bytes = 0, build_solve_st_ws_doubles = 0, build_solve_cs_doubles = 0; };
// one upload: windows, factors in all and in the longest window, landmarks of the longest window, factor tiles
// (est_ex repeats the handle's: the upload paths have it from the same configuration)
struct UploadShape { int B = 0; size_t Ftot = 0, Fmax = 0, Lmax = 0; int n_tiles = 0, est_ex = 0, init_mode = 0, resident = 0; };

// ---- the handle's plan --------------------------------------------------------------------------------------------------
// the roles of a handle's kernel table.  An absent role (inst == KI_NONE) is one the handle never launches.
enum SolverRole {
    KR_SOLVE,                 // the whole reduced solve: k_build_solve_sb MODE 0, k_build_solve_st, or the dense k_build_solve (!lds_T)
    KR_CHAIN, KR_POSE,        // chain_split handles: the chain half (k_build_solve_sb MODE 1) and the pose half (MODE 2)
    KR_LIN_GRAM_CHAIN,        // chain_split handles: k_lin_gram_chain ...
    KR_LIN_GRAM_CHAIN_R1,     // ... and its form with the rank-1 downdates in the same workgroup (NT = 7; N > 11, no extrinsic)
    KR_POSE_DOGLEG,           // chain_split handles of N <= 11: k_pose_dogleg
    KR_RANK1, KR_RANK1_SPLIT, KR_SCHUR_SPLIT,   // the landmark elimination for this nt (the split pair only with r1_part)
    KR_LIN_GRAM, KR_LIN_GRAM_SMALL,             // k_lin_gram with LG_WAVES / LG_WAVES_SMALL wavefronts
    KR_DOGLEG, KR_DOGLEG_CONTROL, KR_STEP_CONTROL,   // k_dogleg<false / true, EX>, k_step_control<true, EX>
    KR_SWEEP, KR_FRONT,       // k_sweep_mfma (lds_T), k_front (chain_split)
    KR_COUNT
};
// which instantiation fills a role.  EX (est_ex) and NT (wd_ld / 16) are the handle's; the window length is what varies:
// N11 = N compiled in as 11, N18 = as 18 (k_build_solve_st only), RT = run-time N up to 11 frames, BIG = run-time N beyond 11
enum KernelInst : uint8_t { KI_NONE, KI_PLAIN, KI_DENSE, SB_N11, SB_RT, SB_BIG, ST_N11, ST_RT, ST_N18, ST_BIG, LGC_N11, LGC_RT, LGC_BIG, LGC_R1, PD_N11, PD_RT };
struct RolePlan { KernelInst inst = KI_NONE; unsigned threads = 0; size_t lds = 0; };     // lds: what the role's dynamic-LDS attribute is raised to

struct HandlePlan {
    SolveShape shape;
    int wd_ld = 0, tvis_sz = 0, nt = 0;       // k_rank1_mfma's panel width (6N pose columns + the g_l column, rounded up to 16) and its 16-column tiles
    size_t n_pairs = 0;
    bool lds_T = false;                       // the LDS-resident path: the structure-aware solve, k_sweep_mfma's pair partials and k_rank1_mfma's panel fit a CU
    size_t lds_sb = 0, lds_st = 0, lds_sw = 0;
    size_t lds_r1_panel = 0, lds_r1 = 0;      // k_rank1_mfma without / with the compacted downdates' landmark lists (lds_T is decided WITHOUT them: the dense loop gives the same bits)
    bool r1_dense = false;                    // the dense rank-1 loop: ISV_R1_DENSE, or the lists do not fit beside the panel
    bool can_split = false;                   // a window of this handle can have ISV_SPLIT_MIN_PASSES passes (k_schur_split)
    bool sw_global_ok = false, has_sw_part = false;   // the pair partials may live in global memory; the scratch for them exists
    bool st_fits = false, solve_st = false;   // k_build_solve_st (four windows per CU): handles whose batches exceed k_build_solve_sb's resident windows
    bool chain_split = false;                 // the reduced solve as chain kernel + pose kernel: handles whose batches leave CUs idle (max_batch <= CUs)
    int split_cap = 1;                        // groups a window's rank-1 downdates may be split into (1: never split)
    size_t r1_groups = 0;                     // groups per window the partial-tile scratch r1_part is sized for (0: no scratch, no split)
    bool marg_one = false;                    // MargBackward's one-wavefront form is the one launch k_marg_bwd<2> (else build / k_marg_jacobi / project)
    RolePlan roles[KR_COUNT];
};

// the reduced-system kernels: N = 11 compiled in (unless ISV_GENERIC_N), else run-time N; BIG beyond 11 frames
static inline KernelInst plan_sb_inst(int N, bool generic_n) { return N == 11 && !generic_n ? SB_N11 : N <= 11 ? SB_RT : SB_BIG; }

inline HandlePlan plan_handle(const SolveShape &s, const SolveEnv &e, const SolveDevice &dev, const SolveSizes &z) {
    HandlePlan p;
    p.shape = s;
    const int N = s.N;
    const size_t B = s.max_batch, n_cus = (size_t)dev.n_cus;
    p.tvis_sz = 36 * (N * (N + 1) / 2) + 18 * N;
    p.wd_ld = 16 * ((6 * N + 16) / 16);
    p.nt = p.wd_ld / 16;
    p.n_pairs = (size_t)N * (N - 1) / 2;
    p.lds_r1_panel = rank1_panel_bytes(p.wd_ld, s.max_lm);
    const bool sw_long = p.n_pairs * 84 * sizeof(double) > 40 * 1024;      // partials too big to share a CU's LDS four ways
    p.lds_sw = sweep_lds_bytes(p.n_pairs, true);                          // (the LDS variant's size; the global one needs less)
    p.lds_sb = z.build_solve_sb_bytes; p.lds_st = z.build_solve_st_bytes;
    // two windows per CU up to N = 11, one beyond
    p.lds_T = N <= 20 && p.wd_ld <= 128 && s.prior_H_sz <= 1024 && p.lds_sb <= (N <= 11 ? 80u : 160u) * 1024 &&
              p.lds_r1_panel <= 160 * 1024 && p.lds_sw <= 160 * 1024;
    p.r1_dense = e.r1_dense || p.lds_r1_panel + rank1_list_bytes(p.nt) > ISV_LDS_PER_CU;
    p.lds_r1 = p.lds_r1_panel + (p.r1_dense ? 0 : rank1_list_bytes(p.nt));
    const size_t passes = ((size_t)s.max_lm + 63) / 64;
    p.can_split = p.lds_T && !s.est_ex && !e.no_split && passes >= ISV_SPLIT_MIN_PASSES && dev.n_cus > ISV_SPLIT_MIN_PASSES;
    p.sw_global_ok = sw_long || e.debug_sw_global;
    p.has_sw_part = p.lds_T && (p.sw_global_ok || p.can_split);
    // k_build_solve_st: a quarter (N <= 11) / half of a CU's LDS per window.  It wins when the batch fills the GPU more than twice
    // over with k_build_solve_sb's two (one) windows per CU; a window alone on a CU is faster with the 512-thread kernel
    p.st_fits = p.lds_T && p.lds_st <= (N <= 11 ? 40u : 80u) * 1024;
    p.solve_st = p.st_fits && (e.solve_st >= 0 ? e.solve_st != 0 : B > (N <= 11 ? 2u : 1u) * n_cus);
    // the split solve: handles that run k_build_solve_sb and whose batches leave CUs idle -- the chain kernel needs a CU of its own
    // beside k_lin_gram / k_rank1_mfma to take the speed/bias elimination off the critical path
    p.chain_split = p.lds_T && !p.solve_st && (e.chain_split >= 0 ? e.chain_split != 0 : B <= n_cus);
    // the split elimination, all or nothing: it pays while every group of every window of a FULL batch finds a CU of its own
    // (measured, round 5: with two groups' workgroups per CU -- 128 windows x 4 groups, 256 x 2 -- the partial tiles' traffic, 123 KB per
    // window and group against 20 KB of Tvis, and the fold launch cost what the shorter passes save: 1.89 -> 1.90 ms, 2.35 -> 2.45 ms)
    if (p.can_split && B * (plan_min(passes, ISV_SPLIT_MAX_GROUPS) + 1) <= n_cus) p.split_cap = ISV_SPLIT_MAX_GROUPS;
    if (p.can_split && p.split_cap >= 2) p.r1_groups = plan_min(passes, (size_t)p.split_cap);
    // (per handle: the two one-wavefront forms of MargBackward sum their convergence test in different orders)
    p.marg_one = e.marg_one_kernel || (!e.marg_split && B > 3 * n_cus);

    RolePlan *k = p.roles;
    const bool ex = s.est_ex != 0, gn = e.generic_n;
    k[KR_DOGLEG] = {KI_PLAIN, 256, 0}; k[KR_DOGLEG_CONTROL] = {KI_PLAIN, 256, 0}; k[KR_STEP_CONTROL] = {KI_PLAIN, 256, 0};
    if (!p.lds_T) { k[KR_SOLVE] = {KI_DENSE, 512, z.build_solve_lds_bytes}; return p; }
    k[KR_SWEEP] = {KI_PLAIN, 64 * ISV_SWEEP_WAVES, p.lds_sw};
    // the landmark elimination for nt 16-column tiles (lds_T: 1 <= nt <= 8): TPW tiles per wavefront, 64 * ceil(nt (nt + 1) / 2 / TPW) threads
    const int tpw = p.nt <= 5 ? 1 : p.nt <= 7 ? 2 : 3;
    const unsigned r1_threads = 64u * (unsigned)((p.nt * (p.nt + 1) / 2 + tpw - 1) / tpw);
    k[KR_RANK1] = {KI_PLAIN, r1_threads, p.lds_r1};
    if (p.r1_groups) {
        k[KR_RANK1_SPLIT] = {KI_PLAIN, r1_threads, p.lds_r1};
        k[KR_SCHUR_SPLIT] = {KI_PLAIN, r1_threads, plan_max(p.lds_r1, (2 * p.n_pairs + 2) * sizeof(int))};
    }
    // k_lin_gram: up to the whole CU (the launch sizes its LDS from the uploaded windows)
    k[KR_LIN_GRAM] = {KI_PLAIN, 64 * LG_WAVES, plan_min(lin_gram_lds_bytes(s.Nr, true, ex, LG_WAVES, s.max_lm), ISV_LDS_PER_CU)};
    k[KR_LIN_GRAM_SMALL] = {KI_PLAIN, 64 * LG_WAVES_SMALL, plan_min(lin_gram_lds_bytes(s.Nr, true, ex, LG_WAVES_SMALL, s.max_lm), ISV_LDS_PER_CU)};
    if (p.solve_st) {
        // (the reference's ALL_BUF_SIZE as a compile-time constant: 404 -> 357 us per launch, 1024 windows 10.27 -> 9.87 ms.  The same for
        //  k_build_solve_sb<true, 18> spills 62 registers and is SLOWER for the single window it serves: 2.54 against 2.48 ms; not instantiated)
        const KernelInst st = N == 11 && !gn ? ST_N11 : N <= 11 ? ST_RT : N == 18 && !gn ? ST_N18 : ST_BIG;
        k[KR_SOLVE] = {st, N <= 11 ? 256u : 512u, p.lds_st};      // (long windows: eight wavefronts, two windows per CU)
    } else if (!p.chain_split) k[KR_SOLVE] = {plan_sb_inst(N, gn), 512, p.lds_sb};
    else {
        k[KR_CHAIN] = {plan_sb_inst(N, gn), 512, p.lds_sb};
        k[KR_POSE] = {plan_sb_inst(N, gn), 512, p.lds_sb};
        k[KR_FRONT] = {KI_PLAIN, 512, z.front_lds_bytes};
        // k_lin_gram_chain: the larger of its two roles' needs
        const size_t lgc = plan_min(plan_max(plan_max(lin_gram_lds_bytes(s.Nr, true, ex, LG_WAVES_SMALL, s.max_lm), p.lds_sb), p.lds_r1), ISV_LDS_PER_CU);
        k[KR_LIN_GRAM_CHAIN] = {ex ? (N <= 11 ? LGC_RT : LGC_BIG) : N == 11 && !gn ? LGC_N11 : N <= 11 ? LGC_RT : LGC_BIG, 512, lgc};
        // the rank-1 downdates in the same workgroup (the shapes instantiated for it)
        if (!ex && !gn && N > 11 && p.nt == 7 && p.lds_r1 <= ISV_LDS_PER_CU) k[KR_LIN_GRAM_CHAIN_R1] = {LGC_R1, 512, lgc};
        // k_pose_dogleg: the pose half's LDS or the dogleg / step control's, whichever is larger (the latter is sized per upload: up to a CU).
        // 11 frames and fewer only (measured: 128 windows of 11 frames 1.92 -> 1.86 ms; the 18-frame form LOSES -- 117 us against 70 + 37
        // for the two launches, rocprofv3)
        if (N <= 11 && !e.no_pose_dogleg) k[KR_POSE_DOGLEG] = {!ex && N == 11 && !gn ? PD_N11 : PD_RT, 512, ISV_LDS_PER_CU - 4096};
    }
    return p;
}

// ---- an upload's plan ---------------------------------------------------------------------------------------------------
// why an upload does not take the fused k_lin_gram (FUSED_OK: it does)
enum FusedRefusal : uint8_t {
    FUSED_OK,
    FUSED_LEGACY,             // ISV_LEGACY_VISUAL
    FUSED_LONG_WINDOW,        // a window of more than ISV_FUSED_MAX_FACTORS factors (one workgroup per window would serialise it)
    FUSED_LDS,                // the longest window's landmarks do not fit k_lin_gram's LDS staging
    FUSED_NO_LDS_PATH,        // resident sequences: the handle is not on the LDS path
    FUSED_LONG_BATCH          // resident sequences: more than 4096 factors per window on average
};
enum MargBwdForm : uint8_t { MARG_BWD_FOUR_WAVES, MARG_BWD_ONE_LAUNCH, MARG_BWD_THREE_LAUNCHES };   // k_marg_bwd<3> | <2> | <0>, k_marg_jacobi, <1>

struct UploadPlan {
    int B = 0, lg_lcap = 0;                   // lg_lcap: landmarks per window k_lin_gram stages (the longest window, rounded up to 32)
    FusedRefusal fused_refusal = FUSED_OK;
    bool fused_visual = false;                // DevBatch::fused_visual: this upload is for k_lin_gram ...
    bool fused = false;                       // ... and the handle runs it (the LDS path)
    // the four flags the kernels read from DevBatch
    bool ctl_stage_lm = false;                // the step control stages its per-landmark gathers in LDS
    bool dg_stage_ph = false;                 // k_dogleg stages the priors' J^T J record in LDS: while that keeps the batch in one resident round
    bool sw_global = false;                   // the pair partials in the global scratch (more than one workgroup per CU: trade LDS for occupancy)
    bool bsub_split = false;                  // DevBatch::bs_split: k_backsub_split does the landmark back-substitution (long windows only)
    bool bsub_in_solve = false;               // DevBatch::bsub_in_solve: k_build_solve_st does it before its outputs (short windows); k_dogleg skips it
    bool lds_T = false, chain_split = false, solve_st = false, init_mode = false;
    bool control_in_wg = false;               // the candidate evaluation in the per-window control kernel (not for windows so long that it would serialise)
    bool fuse_control = false;                // dogleg + step control in one kernel: while the batch fits ONE resident round of it
    int lgw = LG_WAVES;                       // wavefronts of k_lin_gram: eight while every window finds a CU of its own
    bool lg_chain = false;                    // k_lin_gram_chain takes the chain half (else it runs on the side stream)
    bool split = false;                       // one window's elimination over many CUs (k_schur_split + k_schur_fold)
    int GrMax = 0, Gs = 0;                    // the split launch's downdate groups per window and (unfused uploads) its Gram-product groups
    bool r1_in_lg = false;                    // the rank-1 downdates inside k_lin_gram_chain
    bool pose_dogleg = false;                 // the pose half + dogleg + step control in one launch
    bool has_imu = false, has_tiles = false;
    // one iteration's launches: role (KR_COUNT: not launched), grid, dynamic LDS
    unsigned grid_init_state = 0, grid_imu_raw = 0, grid_imu_weight = 0, grid_imu_c = 0, grid_model = 0, grid_tiles = 0, grid_split_y = 0, grid_fold_y = 0, grid_backsub_y = 0;
    size_t lds_prior = 0, lds_prior_c = 0, lds_proj = 0, lds_proj_c = 0;
    SolverRole visual_role = KR_COUNT; size_t lds_visual = 0;          // k_lin_gram / k_lin_gram_chain
    size_t lds_sweep = 0;
    SolverRole solve_role = KR_SOLVE; size_t lds_solve = 0;            // KR_POSE_DOGLEG, KR_POSE or KR_SOLVE
    size_t lds_backsub = 0;
    SolverRole dogleg_role = KR_COUNT; size_t lds_dogleg = 0;          // KR_DOGLEG_CONTROL or KR_DOGLEG (none with pose_dogleg)
    size_t lds_step_control = 0;
    // the tail
    bool finalize_wide = true;                // k_finalize<256>, which also clears the marginalisation record (else k_finalize<64> + k_marg_clear)
    int do_update = 1, clear_marg = 1;        // k_finalize's arguments
    MargBwdForm marg_bwd = MARG_BWD_FOUR_WAVES;
    bool marg_fwd_wide = false;               // k_marg_fwd<256>: four wavefronts for the landmark phases while the batch leaves SIMDs idle
};

inline UploadPlan plan_upload(const HandlePlan &h, const SolveDevice &dev, const SolveEnv &e, const UploadShape &u) {
    UploadPlan p;
    const SolveShape &s = h.shape;
    const RolePlan *K = h.roles;
    const bool ex = s.est_ex != 0;
    const size_t B = (size_t)u.B, n_cus = (size_t)dev.n_cus, np = 15 * (size_t)s.N;
    p.B = u.B; p.lds_T = h.lds_T; p.chain_split = h.chain_split; p.solve_st = h.solve_st; p.init_mode = u.init_mode != 0;
    // k_lin_gram takes one window per workgroup and stages the window's inverse depths and host points in LDS (32 B per landmark):
    // the rule looks at the LONGEST window of the upload, so a window gives the same bits alone and inside any batch.  A batch with a
    // very long window takes the factor-parallel k_proj_linearize<0> + k_sweep_mfma pair, which spreads a window over the whole GPU.
    // A free extrinsic only exists in k_lin_gram<true>: whatever else holds, it is fused or refused.
    p.lg_lcap = (int)((u.Lmax + 31) / 32 * 32);
    const bool lg_fits = lin_gram_lds_bytes(s.Nr, true, ex, LG_WAVES, p.lg_lcap) <= ISV_LDS_PER_CU;
    if (u.resident && !h.lds_T) p.fused_refusal = FUSED_NO_LDS_PATH;
    else if (!lg_fits) p.fused_refusal = FUSED_LDS;
    else if (ex && !u.resident) p.fused_refusal = FUSED_OK;
    else if (e.legacy_visual) p.fused_refusal = FUSED_LEGACY;
    else if (u.Fmax > ISV_FUSED_MAX_FACTORS) p.fused_refusal = FUSED_LONG_WINDOW;
    else if (u.resident && u.Ftot > 4096 * B) p.fused_refusal = FUSED_LONG_BATCH;
    p.fused_visual = p.fused_refusal == FUSED_OK;
    p.fused = h.lds_T && p.fused_visual;
    // the staging flags first: the LDS sizes below are those of the FINAL flags.  dg_stage_ph drops when the staged form no longer
    // fits the batch in one resident round, and only then is the fused control's own resident round counted
    p.ctl_stage_lm = 6 * (size_t)p.lg_lcap * sizeof(double) <= ISV_CTL_STAGE_MAX_BYTES;
    const size_t lds_sc = step_control_lds_bytes(s.N, p.ctl_stage_lm, p.lg_lcap);
    p.dg_stage_ph = ISV_LDS_PER_CU / (plan_max(dogleg_lds_bytes(s.N, s.n_prior_slots, s.prior_H_sz, h.lds_T, true), lds_sc) + ISV_WG_STATIC_LDS) * n_cus >= B;
    const size_t lds_dg = dogleg_lds_bytes(s.N, s.n_prior_slots, s.prior_H_sz, h.lds_T, p.dg_stage_ph), lds_dgc = plan_max(lds_dg, lds_sc);
    // workgroups of k_dogleg<true> the GPU holds: by registers and by LDS (dynamic + static)
    const size_t res_dogleg_ctl = n_cus * plan_min((size_t)dev.dogleg_per_cu_regs, ISV_LDS_PER_CU / (lds_dgc + ISV_WG_STATIC_LDS));
    // (a free extrinsic is only evaluated by the per-window kernels: k_proj_linearize<1> reads the constant one)
    p.control_in_wg = h.lds_T && (u.Ftot <= 4096 * B || ex);
    p.fuse_control = p.control_in_wg && !e.split_control && B <= res_dogleg_ctl;
    p.sw_global = h.has_sw_part && h.sw_global_ok && (u.B > 256 || e.debug_sw_global);
    p.lgw = (p.fused && B <= n_cus && !e.lg_batch_waves && lin_gram_lds_bytes(s.Nr, !p.sw_global, ex, LG_WAVES_SMALL, p.lg_lcap) <= ISV_LDS_PER_CU) ? LG_WAVES_SMALL : LG_WAVES;
    p.lg_chain = h.chain_split && p.fused && p.lgw == LG_WAVES_SMALL;
    // WHETHER a window's downdates are split is decided by the HANDLE (split_cap, from its max_batch and max_landmarks); into how many
    // groups, by the window (schur_split_groups).  An upload without a window of ISV_SPLIT_MIN_PASSES passes skips the split launch
    const int Pmax = (p.lg_lcap + 63) / 64, PmaxH = (s.max_lm + 63) / 64;
    p.GrMax = PmaxH < h.split_cap ? PmaxH : h.split_cap;
    p.split = h.lds_T && h.r1_groups && !e.no_split && Pmax >= ISV_SPLIT_MIN_PASSES && h.split_cap >= 2;
    p.r1_in_lg = p.lg_chain && K[KR_LIN_GRAM_CHAIN_R1].inst != KI_NONE && !p.split;
    // k_backsub_split pays for LONG windows only: ~2.5 us for 300 landmarks inside k_dogleg against 6-8 us for the extra launch
    p.bsub_split = p.split && p.lg_lcap > 1024;
    // ... and a short window of a k_build_solve_st handle has it done by that kernel, before its outputs: its workgroups are out of step
    // by then, k_dogleg's all read their w vectors at once (fused uploads, constant extrinsic: backsub_landmark<false>).  Three frames at
    // least: z_p and u_p are staged over the dead pose blocks behind the chain recurrences' 45 N doubles, 60 N <= 18 N (N + 1)
    p.bsub_in_solve = h.solve_st && p.fused && s.N >= 3 && s.N <= 11 && !ex && !p.bsub_split && !e.bsub_in_dogleg;
    const size_t lds_pd = plan_max(K[KR_POSE].lds, lds_dgc);
    p.pose_dogleg = K[KR_POSE_DOGLEG].inst != KI_NONE && p.fuse_control && !p.bsub_split && lds_pd + ISV_WG_STATIC_LDS <= ISV_LDS_PER_CU;

    // the launches of an iteration
    const size_t NI = B * (size_t)(s.N - 1);
    p.has_imu = NI != 0; p.has_tiles = u.n_tiles > 0;
    p.grid_init_state = (unsigned)((u.B + 63) / 64);
    p.grid_imu_raw = (unsigned)(NI + 63) / 64; p.grid_imu_weight = (unsigned)(NI + 7) / 8; p.grid_imu_c = (unsigned)NI; p.grid_model = (unsigned)(u.B * s.N);
    p.grid_tiles = (unsigned)((u.n_tiles + 3) / 4);
    p.lds_prior = prior_lds_bytes(s.n_prior_slots); p.lds_prior_c = prior_lds_bytes(s.n_prior_slots, false);
    p.lds_proj = 4 * proj_lds_doubles_per_wave(s.N, 0) * sizeof(double); p.lds_proj_c = 4 * proj_lds_doubles_per_wave(s.N, 1) * sizeof(double);
    if (p.fused) {
        const size_t lds_lg = lin_gram_lds_bytes(s.Nr, !p.sw_global, ex, p.lgw, p.lg_lcap);
        p.visual_role = p.lg_chain ? (p.r1_in_lg ? KR_LIN_GRAM_CHAIN_R1 : KR_LIN_GRAM_CHAIN) : p.lgw == LG_WAVES_SMALL ? KR_LIN_GRAM_SMALL : KR_LIN_GRAM;
        p.lds_visual = !p.lg_chain ? lds_lg : plan_max(plan_max(lds_lg, K[KR_CHAIN].lds), p.r1_in_lg ? K[KR_RANK1].lds : 0);
    }
    if (p.split) {
        const int spare = p.fused ? 0 : dev.n_cus / u.B - p.GrMax;       // (fused uploads: the downdates alone, the lean kernel)
        p.Gs = p.fused ? 0 : spare > 16 ? 16 : spare < 1 ? 1 : spare;
        p.grid_split_y = (unsigned)(p.Gs + p.GrMax);
        p.grid_fold_y = (unsigned)(h.nt * (h.nt + 1) / 2);              // one accumulator-tile entry per thread
    }
    p.lds_sweep = sweep_lds_bytes(h.n_pairs, !p.sw_global);
    p.solve_role = p.pose_dogleg ? KR_POSE_DOGLEG : h.chain_split ? KR_POSE : KR_SOLVE;
    p.lds_solve = p.pose_dogleg ? lds_pd : K[p.solve_role].lds;
    p.grid_backsub_y = (unsigned)((p.lg_lcap + 127) / 128); p.lds_backsub = 2 * np * sizeof(double);
    p.dogleg_role = p.pose_dogleg ? KR_COUNT : p.fuse_control ? KR_DOGLEG_CONTROL : KR_DOGLEG;
    p.lds_dogleg = p.fuse_control ? lds_dgc : lds_dg;
    p.lds_step_control = lds_sc;
    // The tail is bound by the window's latency, so k_finalize and MargBackward give a window four wavefronts (ISV_TAIL_ONE_WAVE: the
    // one-wavefront forms).  Those, and what ISV_MARG_ONE_KERNEL / ISV_MARG_SPLIT force: a batch that leaves SIMDs idle takes the
    // four-wavefront eigen-decomposition as a launch of its own, beyond that the one launch <2>
    p.finalize_wide = !e.tail_one_wave;
    p.do_update = (u.init_mode || e.no_update) ? 0 : 1;      // (initFactorGraph creates its priors at the estimate and calls double2vector() only)
    p.clear_marg = (p.finalize_wide && !u.init_mode) ? 1 : 0;
    p.marg_bwd = (!e.tail_one_wave && !e.marg_one_kernel && !e.marg_split) ? MARG_BWD_FOUR_WAVES : h.marg_one ? MARG_BWD_ONE_LAUNCH : MARG_BWD_THREE_LAUNCHES;
    p.marg_fwd_wide = u.B <= 2 * dev.n_cus;
    return p;
}

// ---- the ISV_DEBUG_PATH lines ----------------------------------------------------------------------------------------------
inline int plan_format_lds(char *out, size_t n, const HandlePlan &p) {
    return snprintf(out, n, "isv: N=%d wd_ld=%d prior_H_sz=%d lds_sb=%zu lds_r1=%zu lds_sw=%zu -> lds_T=%d\n", p.shape.N, p.wd_ld, p.shape.prior_H_sz, p.lds_sb, p.lds_r1_panel, p.lds_sw, (int)p.lds_T);
}
inline int plan_format_solve_st(char *out, size_t n, const HandlePlan &p) {
    return snprintf(out, n, "isv: k_build_solve_st lds=%zu fits=%d -> solve_st=%d\n", p.lds_st, (int)p.st_fits, (int)p.solve_st);
}
inline int plan_format_handle(char *out, size_t n, const HandlePlan &p, const SolveEnv &e) {
    return snprintf(out, n, "isv: handle chain_split=%d generic_n=%d no_pose_dogleg=%d lg_batch_waves=%d split_control=%d legacy_visual=%d pose_dogleg_kernel=%d r1_in_lg_kernel=%d split_cap=%d\n",
                    (int)p.chain_split, (int)e.generic_n, (int)e.no_pose_dogleg, (int)e.lg_batch_waves, (int)e.split_control, (int)e.legacy_visual,
                    p.roles[KR_POSE_DOGLEG].inst != KI_NONE ? 1 : 0, p.roles[KR_LIN_GRAM_CHAIN_R1].inst != KI_NONE ? 1 : 0, p.split_cap);
}
inline int plan_format_enqueue(char *out, size_t n, const UploadPlan &p) {
    return snprintf(out, n, "isv: enqueue B=%d lg_lcap=%d fused=%d lgw=%d lg_chain=%d r1_in_lg=%d split=%d bsub_split=%d fuse_control=%d pose_dogleg=%d\n",
                    p.B, p.lg_lcap, (int)p.fused, p.lgw, (int)p.lg_chain, (int)p.r1_in_lg, (int)p.split, (int)p.bsub_split, (int)p.fuse_control, (int)p.pose_dogleg);
}
