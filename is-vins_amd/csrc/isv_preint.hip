// isv_preint.hip -- batched IMU pre-integration: IntegrationBase's constructor, push_back / propagate / midPointIntegration,
// repropagate (include/factor/integration_base.h:13-158), processIMU's propagation of the newest frame (src/estimator.cpp:109-122)
// and slideWindow's MARGIN_SECOND_NEW merge (:1660-1675), one operation per item on a slot of the device, many items in one launch
// (include/isvins_preint.h has the contract; the recurrence is isv_preint.h, shared with the CPU restatement
// tests/native/isv_pre_oracle.c).
//
// k_pre_integrate: one 64-lane wavefront (one workgroup) per item.  The chain over an item's samples is serial; the parallelism is
// inside one 15 x 15 step.  Per item, 11.6 KB of LDS: F (225), V (270), the jacobian twice (2 x 225: the step reads one and writes
// the other), the covariance C (225), F C (225) and the step's 3 x 3 blocks (55 doubles).  Per sample:
//   1  every lane runs the small part (pre_small, and nav_step beside it) on the same numbers in its own registers: the deltas, the
//      nav state and acc_0 / gyr_0 are wave-uniform and never leave the registers between samples; lane 0 stores the step's blocks;
//   2  a lane per entry of F and V (pre_F, pre_V);
//   3  a lane per entry of J and C, four passes of 64 over the 225: F J into the other jacobian and F C (pre_entry_fj), each lane
//      summing its entry's terms in the shared text's order;
//   4  the same lanes form their entries of (F C) F^T + V noise V^T (pre_entry_cov) into C, which part 3 was the last to read;
//   5  lanes 0..6 append the sample to the slot's buffer (PUSH, MERGE).
// Between the parts the wavefront orders its LDS traffic with ISV_WSYNC: there is no workgroup barrier.  PUSH reads its samples from
// the call's upload block, REPROPAGATE and MERGE from the slots' buffers in device memory.  At the end the lanes store the record, lane
// 0 the slot's head and the result, and an item that asked for it copies its record into the call's record rows.
// No atomics, plain stores.  Every index is bounded: a slot by the host's check against max_slots; a sample by the count the host
// checked on its mirror against max_samples, which the kernel checks again on the slot's own count before it writes; a matrix entry
// by e < 225 / e < 270.  The good items of a call have distinct slots and no MERGE source is another item's slot, so no two
// wavefronts touch the same slot's memory unless both only read it.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <vector>
#include "isv_device_math.h"
#include "isv_stage_launch.h"
#include "isv_preint.h"

namespace {

constexpr int kLanes = 64;

struct PreParams {
    int32_t max_samples, pad;
    double nd[6], G[3];
};

struct PreLds {
    double F[225], V[270], J[225], J2[225], C[225], FC[225];
    PreBlocks B;
};

}  // namespace

__global__ void __launch_bounds__(kLanes) k_pre_integrate(const PreHdr *__restrict__ hdrs, const double *__restrict__ samples, isv_pre_result_t *__restrict__ results,
                                                          isv_imu_t *__restrict__ out_rec, isv_imu_t *__restrict__ recs, PreSlotHead *__restrict__ heads,
                                                          double *__restrict__ bufs, const PreParams P) {
    __shared__ PreLds L;
    const PreHdr *H = hdrs + blockIdx.x;
    const int t = threadIdx.x, op = H->op, n = H->n;
    const bool fresh = op == ISV_PRE_PUSH && H->reset;
    isv_imu_t *rec = recs + H->slot;
    PreSlotHead *head = heads + H->slot;
    const int n0 = fresh || op == ISV_PRE_REPROPAGATE ? 0 : head->n_buffered;   // the samples this item's own come behind
    if (n0 < 0 || n0 + n > P.max_samples) {        // (the host's mirror refuses this first)
        if (t == 0) { memset(&results[blockIdx.x], 0, sizeof(isv_pre_result_t)); results[blockIdx.x].status = ISV_PRE_CAPACITY; results[blockIdx.x].n_buffered = head->n_buffered; }
        return;
    }
    double *own = bufs + (size_t)H->slot * P.max_samples * PRE_SAMPLE;
    const double *src = op == ISV_PRE_PUSH ? samples + H->s_off * PRE_SAMPLE
                                           : bufs + (size_t)(op == ISV_PRE_MERGE ? H->src : H->slot) * P.max_samples * PRE_SAMPLE;

    // ---- the state: the constructor's, repropagate's, or the slot's ----
    PreState s;
    double lin_acc[3], lin_gyr[3];
    if (fresh) {
        pre_reset_small(&s, H->acc_0, H->gyr_0, H->ba, H->bg);
        for (int k = 0; k < 3; k++) { lin_acc[k] = H->acc_0[k]; lin_gyr[k] = H->gyr_0[k]; }
    } else {
        for (int k = 0; k < 3; k++) { lin_acc[k] = head->lin_acc[k]; lin_gyr[k] = head->lin_gyr[k]; }
        if (op == ISV_PRE_REPROPAGATE)
            pre_reset_small(&s, lin_acc, lin_gyr, H->ba, H->bg);
        else {
            for (int k = 0; k < 3; k++) {
                s.dp[k] = rec->delta_p[k]; s.dv[k] = rec->delta_v[k]; s.ba[k] = rec->linearized_ba[k]; s.bg[k] = rec->linearized_bg[k];
                s.acc_0[k] = head->acc_0[k]; s.gyr_0[k] = head->gyr_0[k];
            }
            for (int k = 0; k < 4; k++) s.dq[k] = rec->delta_q[k];
            s.sum_dt = rec->sum_dt;
        }
    }
    const bool zeroed = fresh || op == ISV_PRE_REPROPAGATE;
    for (int e = t; e < 225; e += kLanes) {
        L.J[e] = zeroed ? pre_reset_J(e) : rec->jacobian[e];
        L.C[e] = zeroed ? 0.0 : rec->covariance[e];
    }
    double R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Pn[3] = {0, 0, 0}, Vn[3] = {0, 0, 0}, Ba[3] = {0, 0, 0}, Bg[3] = {0, 0, 0};
    const bool nav = H->nav != 0;
    if (nav) {
        for (int k = 0; k < 9; k++) R[k] = H->navs.R[k];
        for (int k = 0; k < 3; k++) { Pn[k] = H->navs.P[k]; Vn[k] = H->navs.V[k]; Ba[k] = H->navs.Ba[k]; Bg[k] = H->navs.Bg[k]; }
    }
    ISV_WSYNC();

    // ---- the chain ----
    double *Jo = L.J, *Jn = L.J2;                  // the jacobian the step reads, and the one it writes
    for (int i = 0; i < n; i++) {
        const double *sm = src + (size_t)i * PRE_SAMPLE;
        const double dt = sm[0], acc[3] = {sm[1], sm[2], sm[3]}, gyr[3] = {sm[4], sm[5], sm[6]};
        // 1: the small part, every lane the same
        if (nav) nav_step(R, Pn, Vn, Ba, Bg, P.G, s.acc_0, s.gyr_0, dt, acc, gyr);
        PreBlocks B;
        pre_small(&s, dt, acc, gyr, &B);
        if (t == 0) L.B = B;
        ISV_WSYNC();
        // 2: F and V, a lane per entry
        for (int e = t; e < 225; e += kLanes) L.F[e] = pre_F(&L.B, e / 15, e % 15);
        for (int e = t; e < 270; e += kLanes) L.V[e] = pre_V(&L.B, e / 18, e % 18);
        ISV_WSYNC();
        // 3: F J and F C
#pragma unroll 1
        for (int e = t; e < 225; e += kLanes) pre_entry_fj(L.F, Jo, L.C, e / 15, e % 15, &Jn[e], &L.FC[e]);
        ISV_WSYNC();
        // 4: (F C) F^T + V noise V^T
#pragma unroll 1
        for (int e = t; e < 225; e += kLanes) L.C[e] = pre_entry_cov(L.F, L.V, L.FC, P.nd, e / 15, e % 15);
        { double *x = Jo; Jo = Jn; Jn = x; }
        // 5: the slot's buffer
        if (op != ISV_PRE_REPROPAGATE && t < PRE_SAMPLE) own[(size_t)(n0 + i) * PRE_SAMPLE + t] = sm[t];
        ISV_WSYNC();
    }

    // ---- the record, the head, the result ----
    isv_imu_t *copy = H->rec >= 0 ? out_rec + H->rec : nullptr;
    for (int e = t; e < 225; e += kLanes) {
        const double j = Jo[e], c = L.C[e];
        rec->jacobian[e] = j; rec->covariance[e] = c;
        if (copy) { copy->jacobian[e] = j; copy->covariance[e] = c; }
    }
    if (t == 0) {
        const int nb = op == ISV_PRE_REPROPAGATE ? head->n_buffered : n0 + n;
        auto put = [&](isv_imu_t *r) {
            for (int k = 0; k < 3; k++) { r->delta_p[k] = s.dp[k]; r->delta_v[k] = s.dv[k]; r->linearized_ba[k] = s.ba[k]; r->linearized_bg[k] = s.bg[k]; }
            for (int k = 0; k < 4; k++) r->delta_q[k] = s.dq[k];
            r->sum_dt = s.sum_dt;
        };
        put(rec);
        if (copy) put(copy);
        for (int k = 0; k < 3; k++) { head->acc_0[k] = s.acc_0[k]; head->gyr_0[k] = s.gyr_0[k]; head->lin_acc[k] = lin_acc[k]; head->lin_gyr[k] = lin_gyr[k]; }
        head->constructed = 1; head->n_buffered = nb;
        isv_pre_result_t *res = results + blockIdx.x;
        res->status = ISV_PRE_OK; res->n_buffered = nb;
        res->sum_dt = s.sum_dt;
        for (int k = 0; k < 3; k++) { res->delta_p[k] = s.dp[k]; res->delta_v[k] = s.dv[k]; res->P[k] = Pn[k]; res->V[k] = Vn[k]; }
        for (int k = 0; k < 4; k++) res->delta_q[k] = s.dq[k];
        for (int k = 0; k < 9; k++) res->R[k] = R[k];
    }
}

extern "C" const char *isv_pre_last_error(const isv_pre_t *h) { return h ? h->err.c_str() : "null handle"; }

extern "C" void isv_pre_destroy(isv_pre_t *h) {
    if (!h) return;
    h->close();
    for (void *p : {(void *)h->d_rec, (void *)h->d_head, (void *)h->d_buf})
        if (p) (void)hipFree(p);
    delete h;
}

extern "C" int isv_pre_create(const isv_pre_config_t *c, isv_pre_t **out) {
    if (!c || !out) return ISV_ERR_INVALID_ARG;
    *out = nullptr;
    if (!pre_check_config(c)) return ISV_ERR_INVALID_ARG;
    isv_pre *h = new isv_pre();
    h->cfg = *c;
    const size_t S = (size_t)c->max_slots;
    hipError_t e = h->open();
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_rec, S * sizeof(isv_imu_t));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_head, S * sizeof(PreSlotHead));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_buf, S * c->max_samples * PRE_SAMPLE * sizeof(double));
    // no slot is constructed: zero records and heads (constructed = 0); the buffers are written before they are read
    if (e == hipSuccess) e = hipMemsetAsync(h->d_rec, 0, S * sizeof(isv_imu_t), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_head, 0, S * sizeof(PreSlotHead), h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (stage_open_failed("isv_pre_create", e)) {
        isv_pre_destroy(h);
        return ISV_ERR_DEVICE;
    }
    h->n_buf.assign(S, -1);
    h->named.assign(S, 0);
    *out = h;
    return ISV_OK;
}

extern "C" int isv_pre_last_ms(isv_pre_t *h, double out_ms[3]) {
    if (!h || !out_ms) return ISV_ERR_INVALID_ARG;
    out_ms[0] = h->slot.call_ms; out_ms[1] = h->slot.kernel_ms; out_ms[2] = h->slot.upload_ms;
    return ISV_OK;
}

extern "C" int isv_pre_run_batch(isv_pre_t *h, int32_t n, const isv_pre_item_t *const *items, isv_pre_result_t *results) {
    StageCall call{h ? h->ctx() : StageCtx{}, "isv_pre_run_batch"};
    if (const int rc = call.enter(n, items, results); rc != ISV_OK || n == 0) return rc;
    if (n > h->cfg.max_items) return call.fail(ISV_ERR_INVALID_ARG, "more items than max_items");
    // every refusal, on the host (pre_check_item: the restatement runs the same text)
    std::vector<PreHdr> hd;
    std::vector<int> who;                          // hd[k] is items[who[k]]
    size_t n_sm = 0;
    int n_rec = 0;
    pre_named_all(&h->cfg, n, items, h->named.data(), 1);
    for (int i = 0; i < n; i++) {
        const isv_pre_item_t *it = items[i];
        const int s = pre_check_item(&h->cfg, it, h->n_buf.data(), h->named.data());
        if (it->slot >= 0 && it->slot < h->cfg.max_slots) h->named[it->slot] |= PRE_NAMED_EARLIER;
        memset(&results[i], 0, sizeof(results[i]));
        results[i].status = s;
        if (s != ISV_PRE_OK) continue;
        PreHdr H;
        memset(&H, 0, sizeof(H));
        H.op = it->op; H.slot = it->slot; H.src = it->op == ISV_PRE_MERGE ? it->src_slot : -1; H.reset = it->op == ISV_PRE_PUSH && it->reset;
        H.n = it->op == ISV_PRE_PUSH ? it->n_samples : h->n_buf[it->op == ISV_PRE_MERGE ? it->src_slot : it->slot];
        H.rec = it->want_record ? n_rec++ : -1;
        if (it->op == ISV_PRE_PUSH) {
            H.s_off = (int64_t)n_sm; n_sm += it->n_samples;
            if (it->nav) { H.nav = 1; H.navs = *it->nav; }
        }
        for (int k = 0; k < 3; k++) { H.acc_0[k] = it->acc_0[k]; H.gyr_0[k] = it->gyr_0[k]; H.ba[k] = it->ba[k]; H.bg[k] = it->bg[k]; }
        hd.push_back(H); who.push_back(i);
    }
    pre_named_all(&h->cfg, n, items, h->named.data(), 0);
    auto counts = [&] {                            // every result reports its slot's count after the call
        for (int i = 0; i < n; i++)
            if (results[i].status != ISV_PRE_OK) results[i].n_buffered = pre_count_of(&h->cfg, items[i]->slot, h->n_buf.data());
    };
    const int m = (int)hd.size();
    if (m == 0) { counts(); return ISV_OK; }
    // one upload block: [headers | samples [PRE_SAMPLE] doubles each]; then, device only: the results, the records asked for
    BlockLayout L;
    const size_t o_hd = L.add(sizeof(PreHdr) * m), o_sm = L.add(sizeof(double) * PRE_SAMPLE * (n_sm + 1));
    const size_t up_end = L.end;
    const size_t o_res = L.add(sizeof(isv_pre_result_t) * m), o_rec = L.add(sizeof(isv_imu_t) * (n_rec + 1));
    std::vector<char> &up = h->up;
    up.resize(up_end);
    memcpy(up.data() + o_hd, hd.data(), sizeof(PreHdr) * m);
    for (int k = 0; k < m; k++) {
        const isv_pre_item_t *it = items[who[k]];
        if (it->op != ISV_PRE_PUSH) continue;
        double *sm = (double *)(up.data() + o_sm) + hd[k].s_off * PRE_SAMPLE;
        for (int i = 0; i < it->n_samples; i++, sm += PRE_SAMPLE) {
            sm[0] = it->dt[i];
            for (int c = 0; c < 3; c++) { sm[1 + c] = it->acc[3 * i + c]; sm[4 + c] = it->gyr[3 * i + c]; }
        }
    }
    std::vector<isv_pre_result_t> rm(m);
    std::vector<isv_imu_t> recs(n_rec);
    PreParams P;
    memset(&P, 0, sizeof(P));
    P.max_samples = h->cfg.max_samples;
    pre_noise(&h->cfg, P.nd);
    for (int k = 0; k < 3; k++) P.G[k] = h->cfg.gravity[k];
    return call.run(
        up, {{o_res, o_res + sizeof(isv_pre_result_t) * m, 0}}, L.end,
        [&](char *d, auto &&) {
            hipLaunchKernelGGL(k_pre_integrate, dim3(m), dim3(kLanes), 0, h->stream, (const PreHdr *)(d + o_hd), (const double *)(d + o_sm), (isv_pre_result_t *)(d + o_res),
                               (isv_imu_t *)(d + o_rec), h->d_rec, h->d_head, h->d_buf, P);
        },
        {{rm.data(), o_res, sizeof(isv_pre_result_t) * m}, {n_rec ? recs.data() : nullptr, o_rec, sizeof(isv_imu_t) * n_rec}},
        [&] {
            for (int k = 0; k < m; k++) {
                const isv_pre_item_t *it = items[who[k]];
                results[who[k]] = rm[k];
                if (rm[k].status != ISV_PRE_OK) continue;
                h->n_buf[it->slot] = rm[k].n_buffered;
                if (hd[k].rec >= 0) *it->record = recs[hd[k].rec];
            }
            counts();
            return hipSuccess;
        });
}
