// isv_kernels.h -- kernel and solver-stage declarations shared by the host translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "isv_device_types.h"
#include "isv_solve_plan.h"      // the launch plans, the kernel roles and the LDS size formulas (HIP-free)

__global__ void k_vector2double(DevBatch d);
__global__ void k_imu_prep(DevBatch d, const int32_t *sel);     // sel: factor index per workgroup (null: identity; < 0: skip)
template <int MODE> __global__ void k_proj_linearize(DevBatch d, const double *pose_src, const double *lam_src, double *fcost_out, int gate);
template <bool JAC> __global__ void k_imu_linearize(DevBatch d, const double *pose_src, const double *sb_src, double *cost_out, int gate);
template <bool JAC> __global__ void k_prior_linearize(DevBatch d, const double *pose_src, const double *sb_src, double *cost_out, int gate);
__global__ void k_cost_reduce(DevBatch d, const double *fcost, const double *imu_cost, const double *prior_cost, double *out, int gate);

// solver stage (isv_solver.hip)
// What a handle and an upload launch is DATA: isv_solve_plan.h's plan_handle() and plan_upload() decide, from the handle's shape, the
// environment hooks, two device figures and the sizes of the upload.  isv_solver_alloc asks for the handle's plan once, allocates what
// it names and maps its kernel enums to the instantiations (the compile-time window lengths -- N = 11, the st kernel's N = 18 -- are
// named there and nowhere else); isv_solver_enqueue asks for the upload's plan and follows it.  A role without a pointer is one the
// handle never launches.
struct SolverHost {
    SolveEnv env;                     // the environment hooks, read once at creation
    SolveDevice dev;                  // compute units; workgroups of k_dogleg<true, EX> per CU by registers
    HandlePlan plan;                  // what this handle runs: sizes, per-handle choices, the instantiation / threads / LDS of every role
    UploadShape upload;               // the sizes of the resident upload (written by the two upload paths: isv_solver_plan_upload)
    const void *fn[KR_COUNT] = {};    // the kernel of each role on this handle
};
// the instantiation behind a role's enum for est_ex = ex and nt 16-column tiles (null: KI_NONE): the only place that names them
const void *isv_solver_kernel(SolverRole r, KernelInst i, bool ex, int nt);
// the plan of an upload of these sizes on this handle; remembers the sizes for the enqueues that follow
UploadPlan isv_solver_plan_upload(SolverHost &hc, const UploadShape &u);
int isv_solver_alloc(DevBatch &d, SolverHost &hc, size_t B, size_t L, size_t F, std::vector<void *> &allocs, std::string &err);
int isv_solver_enqueue(DevBatch &d, const SolverHost &hc, hipStream_t st, hipStream_t st2, hipEvent_t *fj, int64_t *counts, hipEvent_t *prof_ev, std::string &err);
__global__ void k_triangulate(DevBatch d);
template <bool EX, int LGW> __global__ void k_lin_gram(DevBatch d);     // EX: the extrinsic is estimated (J_ex, one more block row)
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
int isv_upload_build_enqueue(DevBatch &d, const int32_t *optr, const double *obs_raw, int lcap, hipStream_t st);
int isv_solver_download(struct isv_backend *h, int n, isv_summary_t *summary, isv_marg_result_t *marg);
void isv_solver_unpack_window(const SolverStage &stage, int b, isv_summary_t *summary, isv_marg_result_t *marg);
int isv_solver_debug_read(DevBatch &d, hipStream_t st, int what, double *out, int64_t count, size_t capB, size_t capL, std::string &err);
