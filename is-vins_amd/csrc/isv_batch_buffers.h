// isv_batch_buffers.h -- the ONE declaration of the handle's transfer buffers: every array that a batch hands over between the
// pinned staging area (isv_backend::Host, SolverStage) and the device (DevBatch, d_optr / d_obs_raw), with its element type (the
// pointers'), its element count and the roles it plays.  Handle creation, the upload's and download's copy plans, the pristine
// copies and the upload check all walk this table; a new batch array is one line here (plus its use).
#pragma once
#include "isv_backend_impl.h"

// the counts a buffer's size is a function of: the handle's capacity at creation, the uploaded batch afterwards
struct BatchDims { size_t B, L, F, O, T; };      // windows, landmarks, factors, observations (factors + landmarks), tiles

enum : unsigned {
    BUF_UP1 = 1,            // upload block, first part: what phase 1 of the two-part upload packs
    BUF_UP2 = 2,            // upload block, second part (phase 2)
    BUF_BACK = 4,           // of the first part, the contiguous run that isv_batch_download's first copy brings back
    BUF_RAW = 8,            // of the upload block, the raw CSR that only k_upload_build reads: a host-packed upload leaves it
    BUF_DERIVED = 16,       // built by k_upload_build; sent by the host-packed upload (ISV_HOST_PACK), compared by ISV_DEBUG_UPLOAD_CHECK
    BUF_STATE = 32,         // output block: the solved state that isv_batch_download unpacks
    BUF_SUMMARY = 64,       // output block: the records of isv_summary_t
    BUF_MARG = 128,         // output block: the marginalisation records
    BUF_UPLOAD = BUF_UP1 | BUF_UP2, BUF_OUT = BUF_STATE | BUF_SUMMARY | BUF_MARG,
};
// a buffer with a pristine twin (isv_backend::pristine[]: what was uploaded, which isv_batch_optimize starts from) names it in its role
enum { TW_Ps, TW_Rs, TW_Vs, TW_Bas, TW_Bgs, TW_depth, TW_tic, TW_ric, TW_se3, TW_lin9, TW_relpose, TW_rollpitch, TW_COUNT };      // (k_restore's job slots)
#define BUF_TWIN(k) ((unsigned)((k) + 1) << 16)
static inline int buf_twin(unsigned role) { return (int)(role >> 16) - 1; }
static_assert(TW_COUNT == sizeof(isv_backend::pristine) / sizeof(void *), "one pristine copy per twin");
static_assert(sizeof(isv_se3_prior_t) % 8 == 0 && sizeof(isv_linear9_t) % 8 == 0 && sizeof(isv_relpose_t) % 8 == 0 && sizeof(isv_rollpitch_t) % 8 == 0, "k_restore copies 8-byte words");

// visit(role, name, pinned pointer, device pointer, element count) for every transfer buffer, the pointers by reference.
// The upload block and the output block are laid out in THIS order (256-byte sections, BlockLayout): the two-part upload cuts
// where BUF_UP2 starts, the first download copy spans the BUF_BACK run.
template <typename Visit>
static inline void for_each_batch_buffer(isv_backend *h, const BatchDims &q, Visit visit) {
    const isv_config_t &c = h->cfg;
    auto &s = h->h; DevBatch &d = h->d; SolverStage &g = h->stage;
    const size_t N = d.N, NI = q.B * (N - 1), NP = (size_t)c.n_frames * (c.n_frames - 1) / 2, SW = ISV_SWEEP_WAVES + 1;
#define BUF(role, name, cnt) visit((unsigned)(role), #name, s.name, d.name, (size_t)(cnt))
    BUF(BUF_UP1, lm_off, q.B + 1); BUF(BUF_UP1, f_off, q.B + 1);
    BUF(BUF_UP1 | BUF_BACK | BUF_TWIN(TW_Ps), Ps, q.B * N * 3); BUF(BUF_UP1 | BUF_BACK | BUF_TWIN(TW_Rs), Rs, q.B * N * 9);
    BUF(BUF_UP1 | BUF_BACK | BUF_TWIN(TW_Vs), Vs, q.B * N * 3); BUF(BUF_UP1 | BUF_BACK | BUF_TWIN(TW_Bas), Bas, q.B * N * 3);
    BUF(BUF_UP1 | BUF_BACK | BUF_TWIN(TW_Bgs), Bgs, q.B * N * 3);
    BUF(BUF_UP1 | BUF_BACK | BUF_TWIN(TW_tic), tic, q.B * 3); BUF(BUF_UP1 | BUF_BACK | BUF_TWIN(TW_ric), ric, q.B * 9);
    BUF(BUF_UP1 | BUF_BACK | BUF_TWIN(TW_se3), se3, q.B); BUF(BUF_UP1 | BUF_BACK | BUF_TWIN(TW_lin9), lin9, q.B);
    BUF(BUF_UP1 | BUF_BACK | BUF_TWIN(TW_relpose), relpose, q.B * (c.n_vo - 1));
    BUF(BUF_UP1 | BUF_BACK | BUF_TWIN(TW_rollpitch), rollpitch, q.B * (size_t)c.max_rollpitch);
    BUF(BUF_UP1 | BUF_BACK | BUF_TWIN(TW_depth), depth, q.L);
    BUF(BUF_UP1, n_rp, q.B); BUF(BUF_UP1, margin_old, q.B); BUF(BUF_UP1, header0, q.B);
    BUF(BUF_UP1, imu_skip, NI); BUF(BUF_UP1, imu_in, NI * ISV_IMU_IN); BUF(BUF_UP1, imu_cov, NI * 225);
    // (the tiles of k_proj_linearize: the linearise API reads them whatever the solver runs; built on the host, a counting loop)
    BUF(BUF_UP2, tile_win, q.T); BUF(BUF_UP2, tile_f0, q.T); BUF(BUF_UP2, tile_n, q.T);
    BUF(BUF_UP2, lm_host, q.L);
    visit(BUF_UP2 | BUF_RAW, "lm_optr", s.lm_optr, h->d_optr, q.L + q.B); visit(BUF_UP2 | BUF_RAW, "obs_raw", s.obs_raw, h->d_obs_raw, q.O * 3);
    BUF(BUF_DERIVED, lm_k, q.L); BUF(BUF_DERIVED, lm_f0, q.L); BUF(BUF_DERIVED, lm_meta, q.L); BUF(BUF_DERIVED, lm_pts_i, q.L * 3);
    BUF(BUF_DERIVED, f_rec, q.F); BUF(BUF_DERIVED, f_pts_j, q.F * 2); BUF(BUF_DERIVED, f_pts_z, q.F);
    BUF(BUF_DERIVED, pg_perm, q.F); BUF(BUF_DERIVED, pg_off, q.B * (NP + 1)); BUF(BUF_DERIVED, pg_sched, q.B * NP);
    BUF(BUF_DERIVED, pg_sched_off, q.B * SW); BUF(BUF_DERIVED, pg_wstart, q.B * SW);
    BUF(BUF_DERIVED, pg_rec, q.F * 2); BUF(BUF_DERIVED, pg_pts, q.F * 2);
    BUF(BUF_STATE, pose, q.B * N * 7); BUF(BUF_STATE, sb, q.B * N * 9); BUF(BUF_STATE, ex, q.B * 7); BUF(BUF_STATE, lam, q.L); BUF(BUF_STATE, solve_flag, q.L);
    BUF(BUF_STATE | BUF_SUMMARY, st, q.B);          // (SolverStage::st is the same record: create_impl)
#undef BUF
    const size_t nt = q.B * ISV_MAX_TRACE;
    visit(BUF_SUMMARY, "trace_cost", g.tc, d.trace_cost, nt); visit(BUF_SUMMARY, "trace_radius", g.tr, d.trace_radius, nt);
    visit(BUF_SUMMARY, "trace_step", g.ts, d.trace_step, nt); visit(BUF_SUMMARY, "trace_acc", g.ta, d.trace_acc, nt);
    visit(BUF_MARG, "marg", g.marg, d.marg, q.B);
}

// the buffers of `roles` that the batch q fills, array by array on the handle's stream (to_device: pinned -> device, else back)
static inline hipError_t copy_batch_buffers(isv_backend *h, const BatchDims &q, unsigned roles, unsigned except, bool to_device) {
    hipError_t e = hipSuccess;
    for_each_batch_buffer(h, q, [&](unsigned role, const char *, auto *&hp, auto *&dp, size_t cnt) {
        if (!(role & roles) || (role & except) || cnt == 0 || e != hipSuccess) return;
        e = to_device ? hipMemcpyAsync(dp, hp, sizeof(*hp) * cnt, hipMemcpyHostToDevice, h->stream) : hipMemcpyAsync(hp, dp, sizeof(*hp) * cnt, hipMemcpyDeviceToHost, h->stream);
    });
    return e;
}
