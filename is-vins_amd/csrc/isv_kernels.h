// isv_kernels.h -- kernel and solver-stage declarations shared by the host translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "isv_device_types.h"

// per-wave LDS of k_proj_linearize<MODE>: R,P per frame + extrinsic; MODE 0 adds a 64 x 15 transpose buffer, MODE 1 the poses at x and the tangent step
__host__ __device__ inline size_t proj_lds_doubles_per_wave(int N, int mode) { return (size_t)N * 12 + 12 + (mode == 0 ? 64 * 15 : (size_t)N * 18); }

__global__ void k_vector2double(DevBatch d);
__global__ void k_imu_prep(DevBatch d, const int32_t *sel);     // sel: factor index per workgroup (null: identity; < 0: skip)
template <int MODE> __global__ void k_proj_linearize(DevBatch d, const double *pose_src, const double *lam_src, double *fcost_out, int gate);
template <bool JAC> __global__ void k_imu_linearize(DevBatch d, const double *pose_src, const double *sb_src, double *cost_out, int gate);
template <bool JAC> __global__ void k_prior_linearize(DevBatch d, const double *pose_src, const double *sb_src, double *cost_out, int gate);
__global__ void k_cost_reduce(DevBatch d, const double *fcost, const double *imu_cost, const double *prior_cost, double *out, int gate);

// solver stage (isv_solver.hip)
// one entry of a handle's kernel table: the instantiation, its threads per workgroup, and the dynamic LDS its attribute is
// raised to (0: not raised)
struct SolverKernel { const void *fn = nullptr; unsigned threads = 0; size_t lds = 0; };
// the roles of the table (SolverHost::kern).  isv_solver_alloc fills them ONCE per handle from its constants (N, est_ex,
// nt = wd_ld / 16, lds_T, solve_st, chain_split, ISV_GENERIC_N, ISV_NO_POSE_DOGLEG): the compile-time window lengths (N = 11,
// the st kernel's N = 18) are chosen there and nowhere else.  An empty role (fn == nullptr) is one the handle never launches.
enum SolverRole {
    KR_SOLVE,                 // the whole reduced solve: k_build_solve_sb MODE 0, k_build_solve_st, or the dense k_build_solve (!lds_T)
    KR_CHAIN, KR_POSE,        // chain_split handles: the chain half (k_build_solve_sb MODE 1) and the pose half (MODE 2)
    KR_LIN_GRAM_CHAIN,        // chain_split handles: k_lin_gram_chain ...
    KR_LIN_GRAM_CHAIN_R1,     // ... and its form with the rank-1 downdates in the same workgroup (NT = 7; N > 11, no extrinsic)
    KR_POSE_DOGLEG,           // chain_split handles of N <= 11: k_pose_dogleg
    KR_RANK1, KR_RANK1_SPLIT, KR_SCHUR_SPLIT,   // the landmark elimination for this nt (the split pair only with d.r1_part)
    KR_LIN_GRAM, KR_LIN_GRAM_SMALL,             // k_lin_gram with LG_WAVES / LG_WAVES_SMALL wavefronts
    KR_DOGLEG, KR_DOGLEG_CONTROL, KR_STEP_CONTROL,   // k_dogleg<false / true, EX>, k_step_control<true, EX>
    KR_SWEEP, KR_FRONT,       // k_sweep_mfma (lds_T), k_front (chain_split)
    KR_COUNT
};
// host-side launch parameters of a handle: device figures, environment hooks and the kernel table, set ONCE in isv_solver_alloc
// (isv_solver_enqueue then chooses among these per uploaded batch)
struct SolverHost {
    int n_cus = 0;                    // compute units of the handle's device
    size_t cap_batch = 0;             // the handle's max_batch: kernel VARIANTS whose results differ in the last bits (k_build_solve_st, the split
                                      // elimination, the one-launch MargBackward) are chosen from it, never from the uploaded batch size, so a
                                      // window gives the same bits alone and inside any batch of the same handle
    int dogleg_per_cu_regs = 0;       // workgroups of k_dogleg<true, EX> per CU by registers (the LDS bound is applied per enqueue)
    bool one_stream = false;          // ISV_ONE_STREAM: diagnostics, everything on one stream
    bool split_control = false;       // ISV_SPLIT_CONTROL: k_dogleg<false> + k_step_control
    bool generic_n = false;           // ISV_GENERIC_N: the run-time-N instantiations in the kernel table for every N
    bool lg_batch_waves = false;      // ISV_LG_BATCH_WAVES: never the eight-wavefront k_lin_gram
    bool debug_sw_global = false;     // ISV_DEBUG_SW_GLOBAL: pair partials in the global scratch for every launch
    bool legacy_visual = false;       // ISV_LEGACY_VISUAL: the unfused k_proj_linearize<0> + k_sweep_mfma pair
    bool sw_global_ok = false;        // the handle's windows are long enough (or ISV_DEBUG_SW_GLOBAL) for the pair partials in global memory
    bool solve_st = false;            // this handle runs k_build_solve_st (four windows per CU; chosen from the handle's max_batch, ISV_SOLVE_ST=0/1 forces)
    bool chain_split = false;         // this handle splits the reduced-system solve into the chain kernel (side stream) and the pose kernel (k_build_solve_sb MODE 1 / 2):
                                      // handles whose batches leave CUs idle (max_batch <= CUs); ISV_CHAIN_SPLIT=0/1 forces
    bool no_pose_dogleg = false;      // ISV_NO_POSE_DOGLEG (A/B and test hook): the pose half, the dogleg and the step control as separate launches (same bits)
    bool no_split = false;            // ISV_NO_SPLIT: never spread one window's landmark elimination over several workgroups (k_schur_split)
    bool marg_one_kernel = false;     // ISV_MARG_ONE_KERNEL / ISV_MARG_SPLIT force MargBackward as one launch (k_marg_bwd<2>) or as build / k_marg_jacobi /
    bool marg_split = false;          // project, whatever the batch size (default: k_marg_bwd<3>, one launch of four wavefronts per window); all bitwise equal (tested)
    bool tail_one_wave = false;       // ISV_TAIL_ONE_WAVE (A/B and test hook): the one-wavefront tail -- k_finalize<64> + k_marg_clear, and MargBackward as
                                      // k_marg_bwd<2> (max_batch > 3 n_cus) or build / k_marg_jacobi / project -- in place of k_finalize<256> and k_marg_bwd<3> (same bits)
    bool r1_dense = false;            // ISV_R1_DENSE (A/B and test hook): k_rank1_mfma's dense MFMA loop, every landmark through every tile (DevBatch::r1_dense; same bits)
    bool no_update = false;           // ISV_DEBUG_NO_UPDATE (sensitivity study, tests/test_sequence_long.py; the oracle has the same
                                      // hook): skip the update() of the prior factors' pseudo-measurements after the solve
                                      // (src/estimator.cpp:1133-1144).  NOT the reference's behaviour.
    bool debug_path = false;          // ISV_DEBUG_PATH (read at create): stderr lines naming the handle's and every enqueue's kernel choices (tests assert them)
    SolverKernel kern[KR_COUNT];      // the kernel of each role on this handle
};
int isv_solver_alloc(DevBatch &d, SolverHost &hc, size_t B, size_t L, size_t F, std::vector<void *> &allocs, std::string &err);
int isv_solver_enqueue(DevBatch &d, const SolverHost &hc, hipStream_t st, hipStream_t st2, hipEvent_t *fj, int64_t *counts, hipEvent_t *prof_ev, std::string &err);
// (jac = false: the residual-only evaluation, see prior_linearize_body)
// + the window's prior factor records staged in LDS (round 3): SE3 49 + Linear9 91 + 49 per relative-pose / 14 per roll-pitch words
__host__ __device__ static inline size_t prior_lds_bytes(int slots, bool jac = true) { return ((size_t)slots * (jac ? 82 + 90 : 10 + 10) + 140 + (size_t)(slots > 2 ? slots - 2 : 0) * 49) * sizeof(double); }
__global__ void k_triangulate(DevBatch d);
// wavefronts of k_lin_gram per window: LG_WAVES for batches (three workgroups per CU), LG_WAVES_SMALL while the batch leaves
// every window a CU of its own (each wavefront takes the pair groups of ISV_SWEEP_WAVES / LGW sweep wavefronts)
#define LG_WAVES 4
#define LG_WAVES_SMALL 8
template <bool EX, int LGW> __global__ void k_lin_gram(DevBatch d);     // EX: the extrinsic is estimated (J_ex, one more block row)
size_t lin_gram_lds_bytes(int N, bool partials_in_lds, bool ex, int waves, int lcap);
#define ISV_LDS_PER_CU ((size_t)160 * 1024)
// bytes of the wave-private landmark lists of k_rank1_mfma's compacted downdates (isv_rank1.h): 64 per output-tile slot, and
// wavefronts x tiles per wavefront <= tiles + 3 slots for nt 16-column blocks
__host__ __device__ inline size_t rank1_list_bytes(int nt) { return (size_t)(nt * (nt + 1) / 2 + 3) * 64; }
template <int NT, int TPW> __global__ void k_schur_split(DevBatch d, int Gs, int GrMax);
template <int NT, int TPW> __global__ void k_rank1_split(DevBatch d, int GrMax);
__global__ void k_schur_fold(DevBatch d, int GrMax, int NT, int from_partials);
__global__ void k_imu_raw(DevBatch d, const double *pose_src, const double *sb_src, int gate);
__global__ void k_imu_weight(DevBatch d, double *cost_out, int gate);
#define ISV_PROF_FAMILIES 6      // 0 = k_proj_linearize<0>, 1 = k_sweep_mfma, 2 = k_rank1_mfma, 3 = k_build_solve*, 4 = k_dogleg, 5 = k_step_control
// the launch counters of an optimize (isv_batch_last_counts): linearisations, reduced solves and landmark eliminations per slot,
// window-iterations (filled from d.act by isv_batch_last_counts), 1 when the fused k_lin_gram ran, 1 when the step control ran
// in the dogleg's workgroup, 1 when k_build_solve_st ran, the split elimination's groups per window (0: not split)
enum { ISV_CNT_LINEARIZE, ISV_CNT_SOLVE, ISV_CNT_ELIM, ISV_CNT_WINDOW_ITERS, ISV_CNT_FUSED_VISUAL, ISV_CNT_FUSED_CONTROL, ISV_CNT_SOLVE_ST, ISV_CNT_SPLIT_GROUPS };
// pinned staging for the result records (capacity max_batch): asynchronous device-to-host copies into pageable
// memory go through the runtime's own staging and may complete lazily, which stalled the NEXT upload by 13-30 ms for
// batches above ~1 MB of records
struct SolverStage { SolveState *st; double *tc, *tr, *ts; int32_t *ta; isv_marg_result_t *marg; };
// raise fn's dynamic-LDS attribute on `device` (the current one) to lds bytes unless it already allows that (isv_solver.hip)
hipError_t isv_raise_dynamic_lds(const void *fn, int device, size_t lds);
// isv_batch_upload's device half (isv_sequence.hip): raw CSR -> lm_* / f_* / pg_* arrays
size_t upload_build_lds_bytes(int N, int lcap);
int isv_upload_build_enqueue(DevBatch &d, const int32_t *optr, const double *obs_raw, int lcap, hipStream_t st);
int isv_solver_download(struct isv_backend *h, int n, isv_summary_t *summary, isv_marg_result_t *marg);
void isv_solver_unpack_window(const SolverStage &stage, int b, isv_summary_t *summary, isv_marg_result_t *marg);
int isv_solver_debug_read(DevBatch &d, hipStream_t st, int what, double *out, int64_t count, size_t capB, size_t capL, std::string &err);
