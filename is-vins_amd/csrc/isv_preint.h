/*
 * isv_preint.h -- the IMU pre-integration recurrence, stated once: IntegrationBase's constructor, propagate -> midPointIntegration
 * (include/factor/integration_base.h:13-158) and processIMU's propagation of the newest frame (src/estimator.cpp:109-122), as plain
 * C that compiles as HIP device code (PRE_HD) or as host C.  The kernel k_pre_integrate (isv_preint.hip) and its CPU restatement
 * tests/native/isv_pre_oracle.c both run this text; every includer has FP contraction off.  The authority for the operation order is
 * the window manager's host code, PreIntegration::push_back and isv_estimator_process_imu in isv_estimator.cpp, which keeps its own
 * copy: every product and sum below is formed as it is there, so the three give the same bits.
 *
 * The step is split the way the kernel runs it: pre_small is the serial part on the 22 small numbers of the state and leaves the
 * 3 x 3 blocks F and V are made of; pre_F / pre_V give one entry of F (15 x 15) / V (15 x 18); pre_entry_fj gives one entry of
 * F jacobian and of F covariance; pre_entry_cov one entry of (F covariance) F^T + V noise V^T.  pre_step is the whole step, serially.
 * Below, for HIP only, the handle.
 */
#ifndef ISV_PREINT_H
#define ISV_PREINT_H
#ifdef __clang__
#pragma clang fp contract(off)
#endif
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "../../include/isvins_preint.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PRE_HD static __device__ __forceinline__
#else
#define PRE_HD static inline
#endif

#define PRE_FINITE(v) ((v) - (v) == 0)  /* neither an infinity nor a NaN */
#define PRE_SAMPLE 7                    /* doubles per buffered sample: dt, acc, gyr */

/* F's and V's non-zero 3 x 3 blocks: bit cb of byte rb is set where block (rb, cb) is one.  F: row 0 has columns 0 3 6 9 12, row 3 has
 * 3 12, row 6 has 3 6 9 12, row 9 has 9, row 12 has 12; V: row 0 has 0 3 6 9, row 3 has 3 9, row 6 has 0 3 6 9, row 9 has 12, row 12
 * has 15.  The other blocks are exact zeros, which add nothing to a dense sum; the sums run over the set blocks in ascending order. */
#define PRE_F_BLOCKS(rb) ((int)((0x10081E121FULL >> (8 * (rb))) & 0xFF))
#define PRE_V_BLOCKS(rb) ((int)((0x20100F0A0FULL >> (8 * (rb))) & 0xFF))

typedef struct PreState {         /* an IntegrationBase without its two matrices */
    double dp[3], dq[4], dv[3];   /* delta_p, delta_q (x y z w), delta_v */
    double ba[3], bg[3];          /* linearized_ba, linearized_bg */
    double sum_dt;
    double acc_0[3], gyr_0[3];
} PreState;

typedef struct PreBlocks {        /* what one step's F and V are made of */
    double Rd[9], Rr[9], ImW[9], RdA0[9], RrA1[9], RrA1W[9], dt;
} PreBlocks;

typedef struct PreSlotHead {      /* a slot beside its isv_imu_t record and its buffer */
    double acc_0[3], gyr_0[3], lin_acc[3], lin_gyr[3];
    int32_t constructed, n_buffered;
} PreSlotHead;

/* ---------------- 3-vectors, 3 x 3 matrices (row-major), quaternions (w x y z), as isv_estimator.cpp has them ---------------- */
PRE_HD void pre_cross(const double *a, const double *b, double *c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
PRE_HD void pre_hat(const double *v, double *M) {
    M[0] = 0; M[1] = -v[2]; M[2] = v[1]; M[3] = v[2]; M[4] = 0; M[5] = -v[0]; M[6] = -v[1]; M[7] = v[0]; M[8] = 0;
}
PRE_HD void pre_mm(const double *A, const double *B, double *C) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) C[r * 3 + c] = A[r * 3] * B[c] + A[r * 3 + 1] * B[3 + c] + A[r * 3 + 2] * B[6 + c];
}
PRE_HD void pre_mv(const double *A, const double *x, double *y) {
    for (int r = 0; r < 3; r++) y[r] = A[r * 3] * x[0] + A[r * 3 + 1] * x[1] + A[r * 3 + 2] * x[2];
}
PRE_HD void pre_qmul(const double *a, const double *b, double *q) {
    q[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    q[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    q[2] = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
    q[3] = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
}
/* Eigen's q * v for a quaternion that need not be unit: v + 2w (u x v) + 2 u x (u x v) */
PRE_HD void pre_qrot(const double *q, const double *v, double *o) {
    double uv[3], c[3];
    pre_cross(q + 1, v, uv);
    for (int k = 0; k < 3; k++) uv[k] = uv[k] + uv[k];
    pre_cross(q + 1, uv, c);
    for (int k = 0; k < 3; k++) o[k] = (v[k] + uv[k] * q[0]) + c[k];
}
/* Eigen's toRotationMatrix(), applied as is to a quaternion that need not be unit */
PRE_HD void pre_qmat(const double *q, double *R) {
    const double tx = 2 * q[1], ty = 2 * q[2], tz = 2 * q[3];
    const double twx = tx * q[0], twy = ty * q[0], twz = tz * q[0], txx = tx * q[1], txy = ty * q[1], txz = tz * q[1];
    const double tyy = ty * q[2], tyz = tz * q[2], tzz = tz * q[3];
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

/* ---------------- pre_reset: IntegrationBase::IntegrationBase (integration_base.h:13-28) ---------------- */
PRE_HD void pre_reset_small(PreState *s, const double *acc_0, const double *gyr_0, const double *ba, const double *bg) {
    for (int k = 0; k < 3; k++) {
        s->dp[k] = 0.0; s->dv[k] = 0.0; s->dq[k] = 0.0;
        s->ba[k] = ba[k]; s->bg[k] = bg[k];
        s->acc_0[k] = acc_0[k]; s->gyr_0[k] = gyr_0[k];
    }
    s->dq[3] = 1.0;
    s->sum_dt = 0.0;
}
/* entry e of the constructor's jacobian (the identity); its covariance is zero */
PRE_HD double pre_reset_J(int e) { return e % 16 == 0 ? 1.0 : 0.0; }

PRE_HD void pre_reset(PreState *s, double *J, double *C, const double *acc_0, const double *gyr_0, const double *ba, const double *bg) {
    pre_reset_small(s, acc_0, gyr_0, ba, bg);
    for (int e = 0; e < 225; e++) { J[e] = pre_reset_J(e); C[e] = 0.0; }
}

/* the four squared noise densities, per 3-column block of V: ACC_N^2, GYR_N^2, ACC_N^2, GYR_N^2, ACC_W^2, GYR_W^2 */
static inline void pre_noise(const isv_pre_config_t *c, double *nd) {
    const double n2[4] = {c->acc_n * c->acc_n, c->gyr_n * c->gyr_n, c->acc_w * c->acc_w, c->gyr_w * c->gyr_w};
    nd[0] = n2[0]; nd[1] = n2[1]; nd[2] = n2[0]; nd[3] = n2[1]; nd[4] = n2[2]; nd[5] = n2[3];
}

/* ---------------- pre_step: propagate -> midPointIntegration (integration_base.h:54-158) ---------------- */
/* the small part: the deltas, sum_dt, acc_0 / gyr_0 advance to the new sample; B is left for F and V */
PRE_HD void pre_small(PreState *s, double dt, const double *acc_1, const double *gyr_1, PreBlocks *B) {
    const double dq[4] = {s->dq[3], s->dq[0], s->dq[1], s->dq[2]};
    double a0[3], a1[3], w[3], un_acc_0[3], un_acc_1[3], rq[4], rp[3], rv[3], Wx[9], A[9];
    for (int k = 0; k < 3; k++) {
        a0[k] = s->acc_0[k] - s->ba[k]; a1[k] = acc_1[k] - s->ba[k];
        w[k] = (s->gyr_0[k] + gyr_1[k]) * 0.5 - s->bg[k];
    }
    pre_qrot(dq, a0, un_acc_0);
    const double half[4] = {1, w[0] * dt / 2, w[1] * dt / 2, w[2] * dt / 2};
    pre_qmul(dq, half, rq);
    pre_qrot(rq, a1, un_acc_1);
    for (int k = 0; k < 3; k++) {
        const double un_acc = (un_acc_0[k] + un_acc_1[k]) * 0.5;
        rp[k] = s->dp[k] + s->dv[k] * dt + 0.5 * un_acc * dt * dt;
        rv[k] = s->dv[k] + un_acc * dt;
    }
    pre_qmat(dq, B->Rd); pre_qmat(rq, B->Rr);
    pre_hat(w, Wx);
    for (int k = 0; k < 9; k++) B->ImW[k] = -Wx[k] * dt;
    B->ImW[0] += 1; B->ImW[4] += 1; B->ImW[8] += 1;
    pre_hat(a0, A); pre_mm(B->Rd, A, B->RdA0);
    pre_hat(a1, A); pre_mm(B->Rr, A, B->RrA1);
    pre_mm(B->RrA1, B->ImW, B->RrA1W);
    B->dt = dt;
    const double nq = sqrt(rq[0] * rq[0] + rq[1] * rq[1] + rq[2] * rq[2] + rq[3] * rq[3]);   /* delta_q.normalize() */
    s->dq[0] = rq[1] / nq; s->dq[1] = rq[2] / nq; s->dq[2] = rq[3] / nq; s->dq[3] = rq[0] / nq;
    for (int k = 0; k < 3; k++) { s->dp[k] = rp[k]; s->dv[k] = rv[k]; s->acc_0[k] = acc_1[k]; s->gyr_0[k] = gyr_1[k]; }
    s->sum_dt += dt;
}

/* F[i][k] */
PRE_HD double pre_F(const PreBlocks *B, int i, int k) {
    const int a = i % 3, b = k % 3, e = a * 3 + b;
    const double I = a == b ? 1.0 : 0.0, dt = B->dt;
    switch ((i / 3) * 5 + k / 3) {
    case 0: return I;
    case 1: return -0.25 * B->RdA0[e] * dt * dt + -0.25 * B->RrA1W[e] * dt * dt;
    case 2: return I * dt;
    case 3: return -0.25 * (B->Rd[e] + B->Rr[e]) * dt * dt;
    case 4: return -0.25 * B->RrA1[e] * dt * dt * -dt;
    case 6: return B->ImW[e];
    case 9: return -1.0 * I * dt;
    case 11: return -0.5 * B->RdA0[e] * dt + -0.5 * B->RrA1W[e] * dt;
    case 12: return I;
    case 13: return -0.5 * (B->Rd[e] + B->Rr[e]) * dt;
    case 14: return -0.5 * B->RrA1[e] * dt * -dt;
    case 18: return I;
    case 24: return I;
    default: return 0.0;
    }
}

/* V[i][k] */
PRE_HD double pre_V(const PreBlocks *B, int i, int k) {
    const int a = i % 3, b = k % 3, e = a * 3 + b;
    const double I = a == b ? 1.0 : 0.0, dt = B->dt;
    switch ((i / 3) * 6 + k / 3) {
    case 0: return 0.25 * B->Rd[e] * dt * dt;
    case 1: case 3: return 0.25 * -B->RrA1[e] * dt * dt * 0.5 * dt;
    case 2: return 0.25 * B->Rr[e] * dt * dt;
    case 7: case 9: return 0.5 * I * dt;
    case 12: return 0.5 * B->Rd[e] * dt;
    case 13: case 15: return 0.5 * -B->RrA1[e] * dt * 0.5 * dt;
    case 14: return 0.5 * B->Rr[e] * dt;
    case 22: return I * dt;
    case 29: return I * dt;
    default: return 0.0;
    }
}

/* entry (i, j) of F J and of F C: the sums over F's non-zero blocks, ascending */
PRE_HD void pre_entry_fj(const double *F, const double *J, const double *C, int i, int j, double *fj, double *fc) {
    const int blocks = PRE_F_BLOCKS(i / 3);
    double a = 0.0, b = 0.0;
    for (int cb = 0; cb < 5; cb++)
        if ((blocks >> cb) & 1)
            for (int k = 3 * cb; k < 3 * cb + 3; k++) {
                const double f = F[i * 15 + k];
                a += f * J[k * 15 + j]; b += f * C[k * 15 + j];
            }
    *fj = a; *fc = b;
}

/* entry (i, j) of the new covariance: FC = F C dense against F^T, then V noise V^T over V's non-zero blocks, V[i][k] nd[k / 3] first */
PRE_HD double pre_entry_cov(const double *F, const double *V, const double *FC, const double *nd, int i, int j) {
    const int blocks = PRE_V_BLOCKS(i / 3);
    double cn = 0.0, q = 0.0;
    for (int k = 0; k < 15; k++) cn += FC[i * 15 + k] * F[j * 15 + k];
    for (int cb = 0; cb < 6; cb++)
        if ((blocks >> cb) & 1)
            for (int k = 3 * cb; k < 3 * cb + 3; k++) {
                const double vn = V[i * 18 + k] * nd[cb];
                q += vn * V[j * 18 + k];
            }
    return cn + q;
}

/* the whole step, serially */
PRE_HD void pre_step(PreState *s, double *J, double *C, const double *nd, double dt, const double *acc_1, const double *gyr_1) {
    PreBlocks B;
    double F[225], V[270], FC[225], Jn[225], Cn[225];
    pre_small(s, dt, acc_1, gyr_1, &B);
    for (int e = 0; e < 225; e++) F[e] = pre_F(&B, e / 15, e % 15);
    for (int e = 0; e < 270; e++) V[e] = pre_V(&B, e / 18, e % 18);
    for (int e = 0; e < 225; e++) pre_entry_fj(F, J, C, e / 15, e % 15, &Jn[e], &FC[e]);
    for (int e = 0; e < 225; e++) Cn[e] = pre_entry_cov(F, V, FC, nd, e / 15, e % 15);
    memcpy(J, Jn, sizeof(Jn)); memcpy(C, Cn, sizeof(Cn));
}

/* ---------------- nav_step: processIMU's Rs / Ps / Vs (estimator.cpp:109-122), acc_0 / gyr_0 as they stand before the step ------- */
PRE_HD void nav_step(double *R, double *P, double *V, const double *Ba, const double *Bg, const double *G, const double *acc_0,
                     const double *gyr_0, double dt, const double *acc, const double *gyr) {
    double d[3], r[3], un_acc_0[3], un_acc_1[3], q[4], D[9], Rn[9];
    for (int k = 0; k < 3; k++) d[k] = acc_0[k] - Ba[k];
    pre_mv(R, d, r);
    for (int k = 0; k < 3; k++) un_acc_0[k] = r[k] - G[k];
    q[0] = 1.0;
    for (int k = 0; k < 3; k++) {
        const double un_gyr = (gyr_0[k] + gyr[k]) * 0.5 - Bg[k];
        q[1 + k] = un_gyr * dt / 2;
    }
    pre_qmat(q, D);
    pre_mm(R, D, Rn);
    for (int k = 0; k < 9; k++) R[k] = Rn[k];
    for (int k = 0; k < 3; k++) d[k] = acc[k] - Ba[k];
    pre_mv(R, d, r);
    for (int k = 0; k < 3; k++) un_acc_1[k] = r[k] - G[k];
    for (int k = 0; k < 3; k++) {
        const double un_acc = (un_acc_0[k] + un_acc_1[k]) * 0.5;
        P[k] = P[k] + dt * V[k] + 0.5 * dt * dt * un_acc;
        V[k] = V[k] + dt * un_acc;
    }
}

/* ---------------- host: the refusals ---------------- */
static int pre_finite_n(const double *v, int n) {
    for (int k = 0; k < n; k++)
        if (!PRE_FINITE(v[k])) return 0;
    return 1;
}

static int pre_check_config(const isv_pre_config_t *c) {
    const double noise[4] = {c->acc_n, c->gyr_n, c->acc_w, c->gyr_w};
    for (int k = 0; k < 4; k++)
        if (!PRE_FINITE(noise[k]) || noise[k] < 0.0) return 0;
    return c->max_slots >= 1 && c->max_slots <= ISV_PRE_MAX_SLOTS && c->max_samples >= 1 && c->max_samples <= ISV_PRE_MAX_SAMPLES &&
           c->max_items >= 1 && c->max_items <= ISV_PRE_MAX_ITEMS && pre_finite_n(c->gravity, 3);
}

#define PRE_NAMED_EARLIER 1       /* named[slot]: an earlier item of the call has it as its `slot` (a refused one too) */
#define PRE_NAMED_ANY 2           /* some item of the call has it as its `slot` */

/* the per-item refusals of isv_pre_run_batch, in their order.  n_buf [max_slots]: the slots' buffered samples before the call, -1 for
 * a slot that is not constructed; named [max_slots]: the bits above. */
static int pre_check_item(const isv_pre_config_t *cfg, const isv_pre_item_t *it, const int32_t *n_buf, const uint8_t *named) {
    const int S = cfg->max_slots;
    if (it->op != ISV_PRE_PUSH && it->op != ISV_PRE_REPROPAGATE && it->op != ISV_PRE_MERGE) return ISV_PRE_INPUT;
    if (it->slot < 0 || it->slot >= S) return ISV_PRE_INPUT;
    if (named[it->slot] & PRE_NAMED_EARLIER) return ISV_PRE_INPUT;
    if (it->op == ISV_PRE_PUSH) {
        if (it->n_samples < 0) return ISV_PRE_INPUT;
        if (it->n_samples > cfg->max_samples) return ISV_PRE_CAPACITY;
        if (it->n_samples > 0 && (!it->dt || !it->acc || !it->gyr)) return ISV_PRE_INPUT;
    }
    if (it->op == ISV_PRE_MERGE && (it->src_slot < 0 || it->src_slot >= S || it->src_slot == it->slot || (named[it->src_slot] & PRE_NAMED_ANY)))
        return ISV_PRE_INPUT;
    if (it->want_record && !it->record) return ISV_PRE_INPUT;
    if (it->op == ISV_PRE_PUSH) {
        if (!pre_finite_n(it->dt, it->n_samples) || !pre_finite_n(it->acc, 3 * it->n_samples) || !pre_finite_n(it->gyr, 3 * it->n_samples)) return ISV_PRE_INPUT;
        if (it->reset && (!pre_finite_n(it->acc_0, 3) || !pre_finite_n(it->gyr_0, 3))) return ISV_PRE_INPUT;
        if (it->nav && !pre_finite_n(it->nav->R, 21)) return ISV_PRE_INPUT;
    }
    if ((it->op == ISV_PRE_REPROPAGATE || (it->op == ISV_PRE_PUSH && it->reset)) && (!pre_finite_n(it->ba, 3) || !pre_finite_n(it->bg, 3))) return ISV_PRE_INPUT;
    const int fresh = it->op == ISV_PRE_PUSH && it->reset;
    if (!fresh && n_buf[it->slot] < 0) return ISV_PRE_UNSET;
    if (it->op == ISV_PRE_MERGE && n_buf[it->src_slot] < 0) return ISV_PRE_UNSET;
    if (it->op == ISV_PRE_PUSH && (fresh ? 0 : n_buf[it->slot]) + it->n_samples > cfg->max_samples) return ISV_PRE_CAPACITY;
    if (it->op == ISV_PRE_MERGE && n_buf[it->slot] + n_buf[it->src_slot] > cfg->max_samples) return ISV_PRE_CAPACITY;
    return ISV_PRE_OK;
}

/* a call's `named` bits: mark_all before the checks, mark_earlier after each item's check, clear at the end */
static void pre_named_all(const isv_pre_config_t *cfg, int n, const isv_pre_item_t *const *items, uint8_t *named, int set) {
    for (int i = 0; i < n; i++)
        if (items[i]->slot >= 0 && items[i]->slot < cfg->max_slots) named[items[i]->slot] = set ? PRE_NAMED_ANY : 0;
}

/* the slot's count a result reports */
static int pre_count_of(const isv_pre_config_t *cfg, int slot, const int32_t *n_buf) {
    return slot >= 0 && slot < cfg->max_slots ? n_buf[slot] : -1;
}

/* what a good item leaves in the mirror of the counts (src's count is the one before the call: a source is no item's target) */
static int pre_count_after(const isv_pre_item_t *it, const int32_t *n_buf) {
    if (it->op == ISV_PRE_PUSH) return (it->reset ? 0 : n_buf[it->slot]) + it->n_samples;
    if (it->op == ISV_PRE_MERGE) return n_buf[it->slot] + n_buf[it->src_slot];
    return n_buf[it->slot];
}

#ifdef __HIPCC__
#include <vector>
#include "isv_stage_launch.h"

struct PreHdr {                   // per-item record of a call
    int64_t s_off;                // PUSH: the item's first sample, into the call's samples (PRE_SAMPLE doubles each)
    int32_t op, slot, src, reset, n, nav, rec;   // n: the samples to run; nav: 1 with a nav state; rec: the row of the call's records, or -1
    int32_t pad;
    double acc_0[3], gyr_0[3], ba[3], bg[3];
    isv_pre_nav_t navs;
};

struct isv_pre : StageHandle {
    isv_pre_config_t cfg;
    isv_imu_t *d_rec = nullptr;       // [max_slots]: the records, one array indexed by slot
    PreSlotHead *d_head = nullptr;    // [max_slots]
    double *d_buf = nullptr;          // [max_slots][max_samples][PRE_SAMPLE]
    std::vector<int32_t> n_buf;       // [max_slots]: the slots' counts, mirrored (-1: not constructed); the checks need them before the launch
    std::vector<uint8_t> named;       // [max_slots]: scratch of a call's checks, all zero between calls
    std::vector<char> up;
};
#endif
#endif /* ISV_PREINT_H */
