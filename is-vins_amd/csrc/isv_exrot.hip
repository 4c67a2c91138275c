// isv_exrot.hip -- batched camera-IMU rotation calibration: InitialEXRotation::CalibrationExRotation with solveRelativeR,
// testTriangulation and decomposeE (src/initial/initial_ex_rotation.cpp), one call per item, for many sequences in one launch; one
// 64-lane workgroup per item (include/isvins_exrot.h has the contract, the reference lines, the restated OpenCV / Eigen arithmetic
// and the quirks X1..X8; the serial pieces are isv_init_common.h and isv_exrot.h, shared with the CPU restatement
// tests/native/isv_exr_oracle.c).  A calibrator is a handle of its own; a sequence's state lives in a slot on the device.
//
// k_exr_calibrate, by phase:
//   1  a lane per correspondence rounds it to float32 (X1) into LDS as one float4 (x0 y0 x1 y1), 16 bytes per correspondence of the
//      call's largest item (dynamic LDS);
//   2  the estimator, rej_estimate of isv_reject.h, the one k_rej_f runs (X2); no model kept: ISV_EXR_NO_MODEL, nothing written;
//   3  lane 0 decomposes E, twice if the negation is taken (X3), and rounds the four cameras to float32 (X4);
//   4  the four triangulation tests, lanes striding over the correspondences: 4 n small QR + Jacobi solves, the hot part.  The four
//      counts are ballot popcounts summed in chunk order (integers: any order gives the same sums);
//   5  lane 0 appends this frame's Rc, Rimu, Rc_g (X5, X6) to the slot's history; a lane per recorded frame forms its quaternions,
//      angle, weight and 4 x 4 block into the slot's scratch A (X7); the Householder QR of A runs column by column, lanes 0..3 each
//      computing the reflector (the same serial sums, redundantly) and lane c > k updating column c, then lane k column k behind a
//      barrier, because the reflector is read from column k (exr_qr_begin / exr_qr_apply: every sum in the serial row order);
//      lane 0 runs the 4 x 4 Jacobi, the inverse and the success rule (X8);
//   6  lane 0 stores the result, ric and frame_count.
// No atomics, plain stores; contraction is off for the whole translation unit.  Every index is bounded: a correspondence by the
// item's count, which the host holds to max_corres <= ISV_EXR_MAX_CORRES; a slot by the host's check against max_slots; a frame by
// frame_count + 1 <= max_frames, which the host checks on its mirror of the counts and the kernel checks again before it writes; a
// subset entry by rp_uniform's modulus, a hypothesis by the chunk length <= 64.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <vector>
#include "isv_stage_launch.h"
#include "isv_reject.h"
#include "isv_exrot.h"

namespace {

constexpr int kLanes = kRejLanes;

struct ExrParams { int32_t max_frames, vo_size; };

enum { SH_NEG = 0, SH_END };

}  // namespace

__global__ void __launch_bounds__(kLanes) k_exr_calibrate(const ExrHdr *__restrict__ hdrs, const double *__restrict__ pts, isv_exr_result_t *__restrict__ results,
                                                          ExrSlotHdr *__restrict__ heads, double *__restrict__ hist, double *__restrict__ scratch, const ExrParams P) {
    extern __shared__ float4 Lp[];             // correspondence (x0 y0 x1 y1) = (ll, rr), float32 (X1)
    __shared__ RejEstLds E;
    __shared__ double LR[18], Lt[3], LP[48];   // R1, R2; t; the four cameras [R1 | t], [R1 | -t], [R2 | t], [R2 | -t] (X4: float32 values)
    __shared__ int sh[SH_END];

    const ExrHdr H = hdrs[blockIdx.x];
    isv_exr_result_t *res = results + blockIdx.x;
    const int t = threadIdx.x, n = H.n;
    ExrSlotHdr *head = heads + H.slot;
    const int F = head->frame_count + 1;
    if (F > P.max_frames) {                    // (the host's mirror refuses this first)
        if (t == 0) exr_refuse(res, ISV_EXR_CAPACITY, F - 1);
        return;
    }
    double *hs = hist + (size_t)H.slot * P.max_frames * EXR_HIST;
    double *A = scratch + (size_t)H.slot * P.max_frames * 16;

    int method = ISV_EXR_NONE, best = 0, choice = 0, front[4] = {0, 0, 0, 0};
    if (n >= ISV_EXR_MIN_CORRES) {
        // ---- 1: the correspondences, a lane each ----
        const double *p = pts + 4 * H.pt_off;
        for (int j = t; j < n; j += kLanes) Lp[j] = make_float4((float)p[4 * j], (float)p[4 * j + 1], (float)p[4 * j + 2], (float)p[4 * j + 3]);
        __syncthreads();
        // ---- 2: findFundamentalMat ----
        rej_estimate(Lp, n, EXR_F_THRESH, E);  // X2
        if (!E.kept) {                         // the reference would abort
            if (t == 0) exr_refuse(res, ISV_EXR_NO_MODEL, F - 1);
            return;
        }
        const bool lmeds = n < ISV_EXR_RANSAC_MIN;
        method = lmeds ? ISV_EXR_LMEDS : ISV_EXR_RANSAC;
        best = E.max_good;
        if (lmeds) {                           // the kept model's inliers at its own bound
            const float4 v = t < n ? Lp[t] : make_float4(0.f, 0.f, 0.f, 0.f);
            best = __popcll(__ballot(t < n && (float)rp_fm_error(E.best, v.x, v.y, v.z, v.w) <= E.bound));
        }
        // ---- 3: decomposeE ----
        if (t == 0) {
            sh[SH_NEG] = exr_decompose_signed(E.best, LR, LR + 9, Lt);   // X3
            for (int s = 0; s < 4; s++) exr_camera(s < 2 ? LR : LR + 9, Lt, (s & 1) ? -1.0 : 1.0, 0, LP + 12 * s);
        }
        __syncthreads();
        // ---- 4: the four triangulation tests ----
        for (int b = 0; b < n; b += kLanes) {
            const int j = b + t;
            int bits = 0;
            if (j < n) {
                const float4 v = Lp[j];
                for (int s = 0; s < 4; s++) bits |= exr_front(LP + 12 * s, v.x, v.y, v.z, v.w, 0) << s;
            }
            for (int s = 0; s < 4; s++) front[s] += __popcll(__ballot((bits >> s) & 1));
        }
        choice = exr_choose(front, n);
    }
    // ---- 5: this frame's rows, every frame's block, the QR ----
    if (t == 0) {
        double *row = hs + (size_t)(F - 1) * EXR_HIST;
        if (choice) {
            const double *R = choice == 1 ? LR : LR + 9;
            for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) row[a * 3 + b] = R[b * 3 + a];   // the transpose (:92-94)
        } else
            for (int k = 0; k < 9; k++) row[k] = k % 4 == 0 ? 1.0 : 0.0;                             // X5
        double ric0[9], dq[4] = {H.dq[0], H.dq[1], H.dq[2], H.dq[3]};
        for (int k = 0; k < 9; k++) ric0[k] = head->ric[k];
        exr_imu_rows(ric0, dq, row + 9, row + 18);                                                  // X6
    }
    __syncthreads();
    for (int i = t; i < F; i += kLanes) {
        double ang, hub;
        exr_row(hs + (size_t)i * EXR_HIST, hs + (size_t)i * EXR_HIST + 9, hs + (size_t)i * EXR_HIST + 18, &ang, &hub, A + 16 * (size_t)i);   // X7
        if (i == F - 1) { res->angle_deg = ang; res->huber = hub; }
    }
    __syncthreads();
    const int rows = 4 * F;
    for (int k = 0; k < 4; k++) {              // X8
        double alpha = 0, vv = 0;
        const int ok = t < 4 ? exr_qr_begin(rows, A, k, &alpha, &vv) : 0;
        if (ok && t > k) exr_qr_apply(rows, A, k, t, alpha, vv);
        __syncthreads();
        if (ok && t == k) exr_qr_apply(rows, A, k, k, alpha, vv);
        __syncthreads();
    }
    // ---- 6: the solve, the success rule, the stores ----
    if (t == 0) {
        double sing[4], ric[9];
        exr_solve_ric(A, sing, ric);
        res->status = ISV_EXR_OK; res->frame_count = F; res->method = method;
        res->iters = method == ISV_EXR_NONE ? 0 : E.iters;
        res->best_inliers = best; res->negated = method == ISV_EXR_NONE ? 0 : sh[SH_NEG];
        for (int s = 0; s < 4; s++) res->front[s] = front[s];
        res->choice = choice;
        res->calibrated = exr_calibrated(F, P.vo_size, sing);
        const double *row = hs + (size_t)(F - 1) * EXR_HIST;
        for (int k = 0; k < 9; k++) { res->Rc[k] = row[k]; res->ric[k] = ric[k]; head->ric[k] = ric[k]; }
        for (int k = 0; k < 4; k++) res->singular[k] = sing[k];
        head->frame_count = F;
    }
}

// frame_count = 0, ric = I in n slots: list[i], or slot i itself without a list
__global__ void __launch_bounds__(kLanes) k_exr_reset(ExrSlotHdr *__restrict__ heads, const int32_t *__restrict__ list, int n) {
    const int i = blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    ExrSlotHdr *h = heads + (list ? list[i] : i);
    h->frame_count = 0; h->pad = 0;
    for (int k = 0; k < 9; k++) h->ric[k] = k % 4 == 0 ? 1.0 : 0.0;
}

extern "C" const char *isv_exr_last_error(const isv_exr_t *h) { return h ? h->err.c_str() : "null handle"; }

extern "C" void isv_exr_destroy(isv_exr_t *h) {
    if (!h) return;
    h->close();
    for (void *p : {(void *)h->d_head, (void *)h->d_hist, (void *)h->d_A, (void *)h->d_list})
        if (p) (void)hipFree(p);
    delete h;
}

extern "C" int isv_exr_create(const isv_exr_config_t *c, isv_exr_t **out) {
    if (!c || !out) return ISV_ERR_INVALID_ARG;
    *out = nullptr;
    if (!exr_check_config(c)) return ISV_ERR_INVALID_ARG;
    isv_exr *h = new isv_exr();
    h->cfg = *c;
    const size_t S = (size_t)c->max_slots, FR = (size_t)c->max_frames;
    hipError_t e = h->open();
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_head, S * sizeof(ExrSlotHdr));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_hist, S * FR * EXR_HIST * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_A, S * FR * 16 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_list, S * sizeof(int32_t));
    // the correspondences of the largest item beside the kernel's own 18 KB: beyond the 64 KB a kernel may use unasked
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_exr_calibrate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(float4) * ISV_EXR_MAX_CORRES);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_exr_reset, dim3((c->max_slots + kLanes - 1) / kLanes), dim3(kLanes), 0, h->stream, h->d_head, (const int32_t *)nullptr, c->max_slots);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (stage_open_failed("isv_exr_create", e)) {
        isv_exr_destroy(h);
        return ISV_ERR_DEVICE;
    }
    h->fc.assign(S, 0);
    h->named.assign(S, 0);
    *out = h;
    return ISV_OK;
}

extern "C" int isv_exr_last_ms(isv_exr_t *h, double out_ms[2]) {
    if (!h || !out_ms) return ISV_ERR_INVALID_ARG;
    out_ms[0] = h->slot.call_ms; out_ms[1] = h->slot.kernel_ms;
    return ISV_OK;
}

extern "C" int isv_exr_reset(isv_exr_t *h, int32_t n, const int32_t *slots) {
    if (!h) return ISV_ERR_INVALID_ARG;
    if (n < 0 || (n > 0 && !slots)) { h->err = "isv_exr_reset: bad arguments"; return ISV_ERR_INVALID_ARG; }
    std::vector<int32_t> list;                 // each slot once: the list fits d_list
    for (int i = 0; i < n; i++) {
        if (slots[i] < 0 || slots[i] >= h->cfg.max_slots) {
            for (int32_t s : list) h->named[s] = 0;
            h->err = "isv_exr_reset: no such slot";
            return ISV_ERR_INVALID_ARG;
        }
        if (!h->named[slots[i]]) { h->named[slots[i]] = 1; list.push_back(slots[i]); }
    }
    for (int32_t s : list) h->named[s] = 0;
    if (list.empty()) return ISV_OK;
    const int m = (int)list.size();
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(h->d_list, list.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_exr_reset, dim3((m + kLanes - 1) / kLanes), dim3(kLanes), 0, h->stream, h->d_head, (const int32_t *)h->d_list, m);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int32_t s : list) h->fc[s] = 0;
    return ISV_OK;
}

extern "C" int isv_exr_read_slot(isv_exr_t *h, int32_t slot, int32_t *frame_count, double *ric, double *history) {
    if (!h) return ISV_ERR_INVALID_ARG;
    if (slot < 0 || slot >= h->cfg.max_slots) { h->err = "isv_exr_read_slot: no such slot"; return ISV_ERR_INVALID_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    ExrSlotHdr head;
    HIPCHK(h, hipMemcpyAsync(&head, h->d_head + slot, sizeof(head), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (head.frame_count < 0 || head.frame_count > h->cfg.max_frames) { h->err = "isv_exr_read_slot: the slot's count is out of range"; return ISV_ERR_DEVICE; }
    if (frame_count) *frame_count = head.frame_count;
    if (ric) memcpy(ric, head.ric, sizeof(head.ric));
    if (history && head.frame_count > 0) {
        HIPCHK(h, hipMemcpyAsync(history, h->d_hist + (size_t)slot * h->cfg.max_frames * EXR_HIST, sizeof(double) * EXR_HIST * head.frame_count, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return ISV_OK;
}

extern "C" int isv_exr_calibrate_batch(isv_exr_t *h, int32_t n, const isv_exr_item_t *const *items, isv_exr_result_t *results) {
    StageCall call{h ? h->ctx() : StageCtx{}, "isv_exr_calibrate_batch"};
    if (const int rc = call.enter(n, items, results); rc != ISV_OK || n == 0) return rc;
    // every refusal, on the host (exr_check_item: the restatement runs the same text)
    std::vector<ExrHdr> hd;
    std::vector<int> who;                          // hd[k] is items[who[k]]
    size_t n_pt = 0;
    int max_n = 1;
    for (int i = 0; i < n; i++) {
        const isv_exr_item_t *it = items[i];
        const int s = exr_check_item(&h->cfg, it, h->fc.data(), h->named.data());
        const bool in_range = it->slot >= 0 && it->slot < h->cfg.max_slots;
        if (in_range) h->named[it->slot] = 1;
        if (s != ISV_EXR_OK) {
            exr_refuse(&results[i], s, in_range ? h->fc[it->slot] : -1);
            continue;
        }
        ExrHdr H;
        memset(&H, 0, sizeof(H));
        H.pt_off = (int64_t)n_pt; H.slot = it->slot; H.n = it->n_corres;
        for (int k = 0; k < 4; k++) H.dq[k] = it->delta_q[k];
        n_pt += it->n_corres;
        if (it->n_corres > max_n) max_n = it->n_corres;
        hd.push_back(H); who.push_back(i);
    }
    for (int i = 0; i < n; i++)
        if (items[i]->slot >= 0 && items[i]->slot < h->cfg.max_slots) h->named[items[i]->slot] = 0;
    const int m = (int)hd.size();
    if (m == 0) return ISV_OK;
    // one upload block: [headers | correspondences [n][4] doubles per item]; then, device only: the results
    BlockLayout L;
    const size_t o_hd = L.add(sizeof(ExrHdr) * m), o_pt = L.add(32 * (n_pt + 1));
    const size_t up_end = L.end;
    const size_t o_res = L.add(sizeof(isv_exr_result_t) * m);
    std::vector<char> &up = h->up;
    up.resize(up_end);
    memcpy(up.data() + o_hd, hd.data(), sizeof(ExrHdr) * m);
    for (int k = 0; k < m; k++) {
        const isv_exr_item_t *it = items[who[k]];
        if (it->n_corres > 0) memcpy(up.data() + o_pt + 32 * (size_t)hd[k].pt_off, it->corres, 32 * (size_t)it->n_corres);
    }
    std::vector<isv_exr_result_t> rm(m);
    const ExrParams P{h->cfg.max_frames, h->cfg.vo_size};
    return call.run(
        up, {{o_res, o_res + sizeof(isv_exr_result_t) * m, 0}}, L.end,
        [&](char *d, auto &&) {
            hipLaunchKernelGGL(k_exr_calibrate, dim3(m), dim3(kLanes), sizeof(float4) * (size_t)max_n, h->stream, (const ExrHdr *)(d + o_hd), (const double *)(d + o_pt),
                               (isv_exr_result_t *)(d + o_res), h->d_head, h->d_hist, h->d_A, P);
        },
        {{rm.data(), o_res, sizeof(isv_exr_result_t) * m}},
        [&] {
            for (int k = 0; k < m; k++) {
                results[who[k]] = rm[k];
                if (rm[k].status == ISV_EXR_OK) h->fc[hd[k].slot] = rm[k].frame_count;
            }
            for (int i = 0; i < n; i++)            // a refused item reports its slot's count after the call
                if (results[i].status != ISV_EXR_OK && results[i].frame_count >= 0) results[i].frame_count = h->fc[items[i]->slot];
            return hipSuccess;
        });
}
