// isv_reject.hip -- batched outlier rejection: FeatureTracker::rejectWithF, the lift of prev_pts / cur_pts to the virtual pinhole and
// cv::findFundamentalMat's status, for many sequences in one call; one 64-lane workgroup per item (include/isvins_reject.h has the
// contract, the reference lines, the restated OpenCV arithmetic and the quirks J1..J6; the serial pieces are isv_init_common.h and
// isv_reject.h, shared with the CPU restatement tests/native/isv_rej_oracle.c).  A rejector is bound to a tracker handle for its
// device, stream and camera.
//
// k_rej_f: a lane per point lifts both sides into LDS as one float4 (x0 y0 x1 y1) in point order (J1).  The estimator is rej_estimate
// (isv_reject.h), which the rotation calibration's kernel calls too (isv_exrot.hip).  From 15 points on the RANSAC
// runs as k_relpose's does (isv_relpose.hip), speculatively in chunks of up to 64 hypotheses: the subsets do not depend on the
// models, so lane 0 draws the next chunk's subsets from the serial RNG stream (J6), each lane solves one 7-point system and counts
// the inliers of its <= 3 models over the LDS points, and lane 0 then replays the serial loop over the chunk in iteration order, with
// the keep rule and the niters update, and stops where the serial loop stops; the last chunk is cut to niters - iter.  With 8 .. 14
// points (J3) the same chunks run to the fixed LMedS niters with no early stop: each lane takes the median of each of its models'
// errors, lane 0 replays the strict `<` in order.  The mask runs a lane per point; n_kept is a ballot popcount.  The points live in
// dynamic LDS, 16 bytes per point of the call's largest item.  No atomics; contraction is off for the whole translation unit.
// Every index is bounded: a point index by the item's count, which the host holds to max_points <= ISV_REJ_MAX_POINTS, a subset entry
// by rp_uniform's modulus, a hypothesis by the chunk length <= 64.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <chrono>
#include <vector>
#include "isv_stage_launch.h"
#include "isv_reject.h"

namespace {

constexpr int kLanes = kRejLanes;

struct RejParams {
    PinholeCam cam;
    double focal, thresh;
};

}  // namespace

__global__ void __launch_bounds__(kLanes) k_rej_f(const RejHdr *__restrict__ hdrs, const float *__restrict__ pts, isv_rej_result_t *__restrict__ results,
                                                  uint8_t *__restrict__ status, const RejParams P) {
    extern __shared__ float4 Lp[];             // correspondence (x0 y0 x1 y1) = (m1, m2), float32 (J1)
    __shared__ RejEstLds E;                    // the estimator's chunk, the kept model and its float32 inlier bound

    const RejHdr H = hdrs[blockIdx.x];
    isv_rej_result_t *res = results + blockIdx.x;
    const int t = threadIdx.x, count = H.n;
    uint8_t *st = status + H.pt_off;
    if (count < ISV_REJ_MIN_POINTS) {          // nothing runs, every point is kept
        for (int j = t; j < count; j += kLanes) st[j] = 1;
        if (t == 0) *res = isv_rej_result_t{ISV_TRK_OK, count, count, ISV_REJ_NONE, 0, 0, -1.0};
        return;
    }
    // ---- the lift, a lane per point, both sides ----
    const float *pp = pts + 4 * H.pt_off, *pc = pp + 2 * (size_t)count;
    for (int j = t; j < count; j += kLanes) {
        float4 v;
        rej_lift(&P.cam, P.focal, H.half_w, H.half_h, pp[2 * j], pp[2 * j + 1], &v.x, &v.y);
        rej_lift(&P.cam, P.focal, H.half_w, H.half_h, pc[2 * j], pc[2 * j + 1], &v.z, &v.w);
        Lp[j] = v;
    }
    __syncthreads();

    rej_estimate(Lp, count, P.thresh, E);      // J2, J3, J6
    const bool lmeds = count < ISV_REJ_RANSAC_MIN;
    // ---- the kept model's mask, a lane per point; nothing kept: every point is rejected (J5) ----
    const bool any = E.kept != 0;
    const float bound = E.bound;
    int n_kept = 0;
    for (int b = 0; b < count; b += kLanes) {
        const int j = b + t;
        bool in = false;
        if (j < count) {
            if (any) {
                const float4 v = Lp[j];
                in = (float)rp_fm_error(E.best, v.x, v.y, v.z, v.w) <= bound;
            }
            st[j] = in ? 1 : 0;
        }
        n_kept += __popcll(__ballot(in));
    }
    if (t == 0)
        *res = isv_rej_result_t{ISV_TRK_OK, count, n_kept, lmeds ? ISV_REJ_LMEDS : ISV_REJ_RANSAC, E.iters,
                                any ? (lmeds ? n_kept : E.max_good) : 0, lmeds && any ? E.min_median : -1.0};
}

extern "C" const char *isv_rej_last_error(const isv_rej_t *h) { return h ? h->err.c_str() : "null handle"; }

extern "C" void isv_rej_destroy(isv_rej_t *h) {
    if (!h) return;
    (void)hipSetDevice(h->trk->device);
    stage_slot_free(h->slot);
    delete h;
}

extern "C" int isv_rej_create(isv_trk_t *trk, const isv_rej_config_t *c, isv_rej_t **out) {
    if (!c || !out) return ISV_ERR_INVALID_ARG;
    *out = nullptr;
    if (!trk) return ISV_ERR_INVALID_ARG;
    if (!rej_check_config(c) || c->max_points > trk->cfg.max_points) return ISV_ERR_INVALID_ARG;
    isv_rej *h = new isv_rej();
    h->cfg = *c;
    h->trk = trk;
    hipError_t e = hipSetDevice(trk->device);
    // the points of the largest item beside the kernel's own 18 KB: beyond the 64 KB a kernel may use unasked
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_rej_f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(float4) * ISV_REJ_MAX_POINTS);
    if (stage_open_failed("isv_rej_create", e)) {
        isv_rej_destroy(h);
        return ISV_ERR_DEVICE;
    }
    *out = h;
    return ISV_OK;
}

extern "C" int isv_rej_last_ms(isv_rej_t *h, double out_ms[4]) {
    if (!h || !out_ms) return ISV_ERR_INVALID_ARG;
    const StageSlot &s = h->slot;
    out_ms[0] = s.call_ms; out_ms[1] = s.kernel_ms; out_ms[2] = s.upload_ms; out_ms[3] = h->pack_ms;
    return ISV_OK;
}

void rej_enqueue(isv_rej *h, const RejHdr *d_hdrs, int m, int max_n, const float *d_pts, isv_rej_result_t *d_results, uint8_t *d_status) {
    RejParams P;
    memset(&P, 0, sizeof(P));
    P.cam = h->trk->cam; P.focal = h->cfg.focal_length; P.thresh = h->cfg.f_threshold;
    hipLaunchKernelGGL(k_rej_f, dim3(m), dim3(kLanes), sizeof(float4) * (size_t)max_n, h->trk->stream, d_hdrs, d_pts, d_results, d_status, P);
}

extern "C" int isv_rej_reject_batch(isv_rej_t *h, int32_t n, const isv_rej_item_t *const *items, isv_rej_result_t *results, uint8_t *const *status) {
    StageCall call{h ? h->ctx() : StageCtx{}, "isv_rej_reject_batch"};
    if (const int rc = call.enter(n, items, results); rc != ISV_OK || n == 0) return rc;
    if (n > h->cfg.max_items) return call.fail(ISV_ERR_CAPACITY, "more items than max_items");
    if (!status) return call.fail(ISV_ERR_INVALID_ARG, "null output array");
    // every refusal, on the host (rej_check_item: the restatement runs the same text)
    std::vector<RejHdr> hd;
    std::vector<int> who;                          // hd[k] is items[who[k]]
    size_t n_pt = 0;
    int max_n = 1;
    for (int i = 0; i < n; i++) {
        const isv_rej_item_t *it = items[i];
        const int s = rej_check_item(&h->cfg, it, status[i]);
        if (s != ISV_TRK_OK) {
            results[i] = isv_rej_result_t{s, it->n_points, 0, ISV_REJ_NONE, 0, 0, -1.0};
            continue;
        }
        RejHdr H;
        memset(&H, 0, sizeof(H));
        H.pt_off = (int64_t)n_pt; H.n = it->n_points;
        H.half_w = it->width / 2.0; H.half_h = it->height / 2.0;
        n_pt += it->n_points;
        if (it->n_points > max_n) max_n = it->n_points;
        hd.push_back(H); who.push_back(i);
    }
    const int m = (int)hd.size();
    if (m == 0) return ISV_OK;
    // one upload block: [headers | points: per item prev [n][2], then cur [n][2]]; then, device only: results, status bytes
    BlockLayout L;
    const size_t o_hd = L.add(sizeof(RejHdr) * m), o_pt = L.add(16 * (n_pt + 1));
    const size_t up_end = L.end;
    const size_t o_res = L.add(sizeof(isv_rej_result_t) * m), o_st = L.add(n_pt + 1);
    const auto t_pack = std::chrono::steady_clock::now();
    std::vector<char> &up = h->up;
    up.resize(up_end);
    memcpy(up.data() + o_hd, hd.data(), sizeof(RejHdr) * m);
    for (int k = 0; k < m; k++) {
        const isv_rej_item_t *it = items[who[k]];
        if (it->n_points == 0) continue;
        char *dst = up.data() + o_pt + 16 * (size_t)hd[k].pt_off;
        memcpy(dst, it->prev_pts, 8 * (size_t)it->n_points);
        memcpy(dst + 8 * (size_t)it->n_points, it->cur_pts, 8 * (size_t)it->n_points);
    }
    const double pack_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_pack).count();
    std::vector<isv_rej_result_t> rm(m);
    std::vector<uint8_t> sm(n_pt + 1);
    const int rc = call.run(
        up, {}, L.end,
        [&](char *d, auto &&) {
            rej_enqueue(h, (const RejHdr *)(d + o_hd), m, max_n, (const float *)(d + o_pt), (isv_rej_result_t *)(d + o_res), (uint8_t *)(d + o_st));
        },
        {{rm.data(), o_res, sizeof(isv_rej_result_t) * m}, {n_pt ? sm.data() : nullptr, o_st, n_pt}},
        [&] {
            for (int k = 0; k < m; k++) {
                results[who[k]] = rm[k];
                if (hd[k].n) memcpy(status[who[k]], sm.data() + hd[k].pt_off, (size_t)hd[k].n);
            }
            return hipSuccess;
        });
    if (rc != ISV_OK) return rc;
    h->pack_ms = pack_ms;
    return ISV_OK;
}
