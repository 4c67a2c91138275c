// isv_frontend.hip -- the whole-frame feature tracker: FeatureTracker::readImage and the message of System::PubImageData for many
// sequences in one call, with a sequence's whole state in its slot on the device (include/isvins_frontend.h has the contract, the
// reference lines and the quirks F1..F3; the host half is isv_fe_host.h; the restatement is tests/fe_oracle.py).
//
// The stages' kernels run unchanged (trk_enqueue_*, rej_enqueue, det_enqueue) on records that live in the call's block.  The host
// writes what it knows of a record (the buffers, the shapes, every offset: item k's points are at k * max_points of every per-point
// section, its corners at k * max_cnt) and leaves the counts 0; four glue kernels, one 64-lane workgroup per item, write the counts:
//   k_fe_begin         TrkItem.np and the flow's input points, from the slot's state.
//   k_fe_after_flow    the ordered compaction by both flag bits (a ballot per chunk of 64, a running base: the order is the list's),
//                      track_cnt++, the rejector's packed prev | cur points and its RejHdr (n = 0 when rejectWithF does not run).
//   k_fe_after_reject  setMask's order: a survivor's place is the number of survivors with a larger track_cnt, or an equal one and a
//                      smaller index (the stable descending sort, without sorting); its DetPoint, rounded by det_round_coord, with
//                      its index in the compacted list; DetItem.np and max_new.  The compaction by the rejector's status is folded
//                      into this: nothing is moved, the detector's kept list indexes the list of k_fe_after_flow.
//   k_fe_finish        the gather by the kept list, addPoints, the lift (isv_pinhole.h), the velocities (F1, F2), updateID (an
//                      ordered count of the ids that are -1), the message rows (an ordered count of track_cnt > 1), the result
//                      record and the slot's new state.
// Plain stores, no atomics; a kernel boundary lies between every writer and its readers in other workgroups.  DESIGN section 21 has
// the memory-safety argument: every index is bounded by a count that a kernel clamps to max_points where it reads it.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <vector>
#include "isv_stage_launch.h"
#include "isv_tracker.h"
#include "isv_equalize.h"
#include "isv_reject.h"
#include "isv_detect.h"
#include "isv_pinhole.h"
#include "isv_fe_host.h"

namespace {

constexpr int kLanes = 64;

struct FeSlotHdr { int32_t n, n_id; double prev_time; };      // a slot's scalars on the device
struct FeItem {                   // one item that passed every check
    int32_t slot, first, pub, W, H, pad;
    double cur_time;
};
struct FeCount { int32_t n1, n2; };                           // after the flow, after rejectWithF

struct FeState {                  // the slots' feature state, [max_slots] and [max_slots][max_points]
    FeSlotHdr *hdr;
    float *pts, *un;              // prev_pts, the previous un-distorted points
    int32_t *ids, *cnt;
    uint8_t *map;                 // F1: the point was in prev_un_pts_map under its own id
};

struct FeOut {                    // the call's outputs in its block, [m][max_points] rows each
    isv_fe_result_t *res;
    int32_t *m_id; double *m_pt; float *m_uv, *m_vel;
    float *l_cp, *l_un; int32_t *l_id, *l_cnt; float *l_vel;
};

__device__ __forceinline__ int fe_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int fe_before(unsigned long long ballot, int lane) { return __popcll(ballot & ((1ull << lane) - 1ull)); }

}  // namespace

struct isv_fe {
    isv_fe_config_t cfg;
    isv_trk *trk = nullptr;
    isv_eq *eq = nullptr;
    isv_rej *rej = nullptr;
    isv_det *det = nullptr;
    std::string err;
    StageSlot slot;               // the call's device block (grow-only), events and times
    StageCtx ctx() { return StageCtx{trk->device, trk->stream, &slot, &err}; }   // (the device and the stream are the tracker's)
    FeState S{};
    std::vector<uint8_t> seq;     // [max_slots]: the slot holds a sequence
    std::vector<int64_t> seen;    // [max_slots]: the tracker's generation count of the slot when the front end last wrote (or took) its image
    std::vector<char> up;
    FeSlotView view(int slot_i) const {
        const TrkSlot &sl = trk->slots[slot_i];
        return FeSlotView{sl.valid, sl.W, sl.H, sl.tag == (eq ? eq->id : 0), seq[slot_i], seen[slot_i] == trk->gen[slot_i]};
    }
};

__global__ void __launch_bounds__(kLanes) k_fe_begin(const FeItem *__restrict__ items, TrkItem *__restrict__ ti, const FeState S, float *__restrict__ fp, int P) {
    const int k = blockIdx.x, t = threadIdx.x;
    const FeItem I = items[k];
    const int n = I.first ? 0 : fe_min(S.hdr[I.slot].n, P);
    const float2 *src = (const float2 *)S.pts + (size_t)I.slot * P;
    float2 *dst = (float2 *)fp + (size_t)k * P;
    for (int j = t; j < n; j += kLanes) dst[j] = src[j];
    if (t == 0) ti[k].np = n;
}

__global__ void __launch_bounds__(kLanes) k_fe_after_flow(const FeItem *__restrict__ items, const TrkItem *__restrict__ ti, const FeState S, const float *__restrict__ fp,
                                                         const float *__restrict__ cp, const uint8_t *__restrict__ fl, RejHdr *__restrict__ rh, float *__restrict__ rp,
                                                         int32_t *__restrict__ a_ids, int32_t *__restrict__ a_cnt, float *__restrict__ a_pun, uint8_t *__restrict__ a_map,
                                                         FeCount *__restrict__ cnts, int P) {
    const int k = blockIdx.x, t = threadIdx.x;
    const FeItem I = items[k];
    const int n = fe_min(ti[k].np, P);
    const size_t o = (size_t)k * P, so = (size_t)I.slot * P;
    int n1 = 0;
    for (int b = 0; b < n; b += kLanes) {
        const int j = b + t;
        n1 += __popcll(__ballot(j < n && fl[o + j] == (ISV_TRK_FLAG_STATUS | ISV_TRK_FLAG_BORDER)));
    }
    // the rejector's layout: prev [n1][2], then cur [n1][2] (isv_reject.h)
    float2 *a_prev = (float2 *)(rp + 4 * o), *a_cur = a_prev + n1;
    int base = 0;
    for (int b = 0; b < n; b += kLanes) {
        const int j = b + t;
        const bool keep = j < n && fl[o + j] == (ISV_TRK_FLAG_STATUS | ISV_TRK_FLAG_BORDER);
        const unsigned long long ballot = __ballot(keep);
        if (keep) {
            const size_t d = o + base + fe_before(ballot, t);
            a_prev[d - o] = ((const float2 *)fp)[o + j];
            a_cur[d - o] = ((const float2 *)cp)[o + j];
            a_ids[d] = S.ids[so + j];
            a_cnt[d] = S.cnt[so + j] + 1;                     // :124-125
            ((float2 *)a_pun)[d] = ((const float2 *)S.un)[so + j];
            a_map[d] = S.map[so + j];
        }
        base += __popcll(ballot);
    }
    if (t == 0) {
        RejHdr H;
        H.pt_off = (int64_t)o; H.n = (I.pub && !I.first) ? n1 : 0; H.pad = 0;
        H.half_w = I.W / 2.0; H.half_h = I.H / 2.0;
        rh[k] = H;
        cnts[k].n1 = n1;
    }
}

__global__ void __launch_bounds__(kLanes) k_fe_after_reject(const FeItem *__restrict__ items, FeCount *__restrict__ cnts, const uint8_t *__restrict__ rs,
                                                           const float *__restrict__ rp, const int32_t *__restrict__ a_cnt, DetItem *__restrict__ di,
                                                           DetPoint *__restrict__ dp, int max_cnt, int P) {
    const int k = blockIdx.x, t = threadIdx.x;
    const FeItem I = items[k];
    const int n1 = fe_min(cnts[k].n1, P);
    if (!I.pub && !I.first) {                     // no rejectWithF, no setMask, no detection: the DetItem stays empty
        if (t == 0) cnts[k].n2 = n1;
        return;
    }
    const size_t o = (size_t)k * P;
    const uint8_t *st = rs + o;                   // (a first frame has n1 = 0: nothing is read)
    const float2 *a_cur = (const float2 *)(rp + 4 * o) + n1;
    int n2 = 0;
    for (int b = 0; b < n1; b += kLanes) {
        const int j = b + t;
        n2 += __popcll(__ballot(j < n1 && st[j] != 0));
    }
    for (int i = t; i < n1; i += kLanes) {
        if (!st[i]) continue;
        const int c = a_cnt[o + i];
        int rank = 0;                             // setMask's place (G1): larger counts first, the list's order among equals
        for (int j = 0; j < n1; j++) {
            if (!st[j]) continue;
            const int cj = a_cnt[o + j];
            rank += (cj > c || (cj == c && j < i)) ? 1 : 0;
        }
        const float2 q = a_cur[i];
        int rx = 0, ry = 0;
        (void)det_round_coord(q.x, &rx); (void)det_round_coord(q.y, &ry);
        // inBorder held for q (both flag bits): 1 <= rx < W - 1, 1 <= ry < H - 1.  The clamp never acts; it is the bound k_det_mask relies on
        rx = rx < 0 ? 0 : (rx > I.W - 1 ? I.W - 1 : rx); ry = ry < 0 ? 0 : (ry > I.H - 1 ? I.H - 1 : ry);
        dp[o + rank] = DetPoint{rx, ry, i, 0};
    }
    if (t == 0) {
        di[k].np = n2;
        di[k].max_new = max_cnt - n2 > 0 ? max_cnt - n2 : 0;  // :130 (F3)
        cnts[k].n2 = n2;
    }
}

__global__ void __launch_bounds__(kLanes) k_fe_finish(const FeItem *__restrict__ items, const FeCount *__restrict__ cnts, const DetCount *__restrict__ dc,
                                                     const int32_t *__restrict__ kept, const float *__restrict__ new_pts, const isv_rej_result_t *__restrict__ rr,
                                                     const float *__restrict__ rp, const int32_t *__restrict__ a_ids, const int32_t *__restrict__ a_cnt,
                                                     const float *__restrict__ a_pun, const uint8_t *__restrict__ a_map, const FeState S, const PinholeCam cam,
                                                     const FeOut O, int max_cnt, int P) {
    const int k = blockIdx.x, t = threadIdx.x;
    const FeItem I = items[k];
    const size_t o = (size_t)k * P, so = (size_t)I.slot * P, co = (size_t)k * max_cnt;
    const int n1 = fe_min(cnts[k].n1, P);
    const bool det = I.pub || I.first;
    // n_kept <= n2 <= n1 and n_new <= max(max_cnt - n2, 0): n_kept + n_new <= max(max_cnt, n1) <= max_points.  The clamps never act.
    const int nk = det ? fe_min(dc[k].n_kept, n1) : n1;
    const int nn = det ? fe_min(fe_min(dc[k].n_new, max_cnt), P - nk) : 0;
    const int total = nk + nn;
    const float2 *a_cur = (const float2 *)(rp + 4 * o) + n1;
    const FeSlotHdr hdr = I.first ? FeSlotHdr{0, 0, 0.0} : S.hdr[I.slot];
    const bool map_nonempty = hdr.n > 0;          // F1: the previous frame ended with a point
    const double dt = I.cur_time - hdr.prev_time; // :215
    int next_id = hdr.n_id, n_msg = 0;
    for (int b = 0; b < total; b += kLanes) {
        const int r = b + t;
        const bool valid = r < total;
        float x = 0.f, y = 0.f, ux = 0.f, uy = 0.f, vx = 0.f, vy = 0.f;
        int id = 0, c = 0;
        if (valid) {
            float2 pun = make_float2(0.f, 0.f);
            int im = 0;
            if (r < nk) {
                int src = det ? kept[o + r] : r;
                src = src < 0 ? 0 : (src >= n1 ? n1 - 1 : src);           // (an index of k_fe_after_reject's: below n1)
                const float2 q = a_cur[src];
                x = q.x; y = q.y; id = a_ids[o + src]; c = a_cnt[o + src]; pun = ((const float2 *)a_pun)[o + src]; im = a_map[o + src];
            } else {                              // addPoints (:71-79)
                x = new_pts[2 * (co + r - nk)]; y = new_pts[2 * (co + r - nk) + 1]; id = -1; c = 1;
            }
            pinhole_lift(cam, x, y, &ux, &uy);    // :204-207
            if (map_nonempty && id != -1 && im) { // :219-227; everything else is (0, 0), F2 included
                vx = (float)((double)(ux - pun.x) / dt);
                vy = (float)((double)(uy - pun.y) / dt);
            }
        }
        const bool newborn = valid && id == -1;
        const unsigned long long nb = __ballot(newborn);
        const int id_out = newborn ? next_id + fe_before(nb, t) : id;     // updateID (:182-188), in list order
        next_id += __popcll(nb);
        const bool in_msg = valid && I.pub && c > 1;                      // System.cpp:116
        const unsigned long long mb = __ballot(in_msg);
        if (valid) {
            ((float2 *)S.pts)[so + r] = make_float2(x, y);
            ((float2 *)S.un)[so + r] = make_float2(ux, uy);
            S.ids[so + r] = id_out; S.cnt[so + r] = c;
            S.map[so + r] = newborn ? 0 : 1;      // F1: the map holds the point under the id it had in UndistortPixelMotion
            ((float2 *)O.l_cp)[o + r] = make_float2(x, y);
            ((float2 *)O.l_un)[o + r] = make_float2(ux, uy);
            O.l_id[o + r] = id_out; O.l_cnt[o + r] = c;
            ((float2 *)O.l_vel)[o + r] = make_float2(vx, vy);
        }
        if (in_msg) {
            const size_t d = o + n_msg + fe_before(mb, t);
            O.m_id[d] = id_out;                   // p_id * NUM_OF_CAM + i with one camera
            O.m_pt[3 * d] = (double)ux; O.m_pt[3 * d + 1] = (double)uy; O.m_pt[3 * d + 2] = 1.0;
            ((float2 *)O.m_uv)[d] = make_float2(x, y);
            ((float2 *)O.m_vel)[d] = make_float2(vx, vy);
        }
        n_msg += __popcll(mb);
    }
    __syncthreads();                              // every lane has read the slot's header
    if (t == 0) {
        S.hdr[I.slot] = FeSlotHdr{total, next_id, I.cur_time};
        const bool rejected = I.pub && !I.first;
        O.res[k] = isv_fe_result_t{ISV_TRK_OK, n1, fe_min(cnts[k].n2, n1), nk, nn, total, n_msg, rejected ? rr[k].method : ISV_REJ_NONE, rejected ? rr[k].iters : 0, 0};
    }
}

extern "C" const char *isv_fe_last_error(const isv_fe_t *h) { return h ? h->err.c_str() : "null handle"; }

extern "C" void isv_fe_destroy(isv_fe_t *h) {
    if (!h) return;
    (void)hipSetDevice(h->trk->device);
    stage_slot_free(h->slot);
    for (void *p : {(void *)h->S.hdr, (void *)h->S.pts, (void *)h->S.un, (void *)h->S.ids, (void *)h->S.cnt, (void *)h->S.map})
        if (p) (void)hipFree(p);
    delete h;
}

extern "C" int isv_fe_create(isv_trk_t *trk, struct isv_eq *eq, struct isv_rej *rej, struct isv_det *det, const isv_fe_config_t *c, isv_fe_t **out) {
    if (!c || !out) return ISV_ERR_INVALID_ARG;
    *out = nullptr;
    if (!trk || !rej || !det) return ISV_ERR_INVALID_ARG;
    if (c->max_items < 1 || c->max_items > 65535 || c->max_cnt < 1 || c->max_points < c->max_cnt || c->max_points > 65535) return ISV_ERR_INVALID_ARG;
    if (rej->trk != trk || det->trk != trk || (eq && eq->trk != trk)) return ISV_ERR_INVALID_ARG;
    if (c->max_items > trk->cfg.max_items || c->max_items > rej->cfg.max_items || c->max_items > det->cfg.max_items || (eq && c->max_items > eq->cfg.max_items))
        return ISV_ERR_INVALID_ARG;
    if (c->max_points > trk->cfg.max_points || c->max_points > rej->cfg.max_points || c->max_points > det->cfg.max_points || c->max_cnt > det->cfg.max_corners)
        return ISV_ERR_INVALID_ARG;
    isv_fe *h = new isv_fe();
    h->cfg = *c;
    h->trk = trk; h->eq = eq; h->rej = rej; h->det = det;
    h->seq.assign(trk->cfg.max_slots, 0);
    h->seen.assign(trk->cfg.max_slots, -1);
    const size_t ns = (size_t)trk->cfg.max_slots, np = ns * (size_t)c->max_points;
    hipError_t e = hipSetDevice(trk->device);
    if (e == hipSuccess) e = hipMalloc(&h->S.hdr, sizeof(FeSlotHdr) * ns);
    if (e == hipSuccess) e = hipMalloc(&h->S.pts, 8 * np);
    if (e == hipSuccess) e = hipMalloc(&h->S.un, 8 * np);
    if (e == hipSuccess) e = hipMalloc(&h->S.ids, 4 * np);
    if (e == hipSuccess) e = hipMalloc(&h->S.cnt, 4 * np);
    if (e == hipSuccess) e = hipMalloc(&h->S.map, np);
    if (e == hipSuccess) e = hipMemsetAsync(h->S.hdr, 0, sizeof(FeSlotHdr) * ns, trk->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(trk->stream);
    if (stage_open_failed("isv_fe_create", e)) {
        isv_fe_destroy(h);
        return ISV_ERR_DEVICE;
    }
    *out = h;
    return ISV_OK;
}

extern "C" int isv_fe_last_ms(isv_fe_t *h, double out_ms[6]) {
    if (!h || !out_ms) return ISV_ERR_INVALID_ARG;
    const StageSlot &s = h->slot;      // the marks: after the pyramids, after k_fe_after_flow, after k_fe_after_reject
    out_ms[0] = s.call_ms; out_ms[1] = s.part_ms[0]; out_ms[2] = s.part_ms[1]; out_ms[3] = s.part_ms[2]; out_ms[4] = s.part_ms[3]; out_ms[5] = s.upload_ms;
    return ISV_OK;
}

extern "C" int isv_fe_gate_init(isv_fe_gate_t *gate, int32_t freq) { return fe_gate_init(gate, freq); }
extern "C" int isv_fe_gate_step(isv_fe_gate_t *gate, double stamp, isv_fe_gate_out_t *out) { return fe_gate_step(gate, stamp, out); }

extern "C" int isv_fe_slot_reset(isv_fe_t *h, int32_t slot) {
    if (!h || slot < 0 || slot >= h->trk->cfg.max_slots) return ISV_ERR_INVALID_ARG;
    h->seq[slot] = 0;
    return ISV_OK;
}

extern "C" int isv_fe_slot_get(isv_fe_t *h, int32_t slot, isv_fe_state_t *state, float *prev_pts, int32_t *ids, int32_t *track_cnt, float *prev_un_pts, uint8_t *in_map) {
    if (!h || !state || slot < 0 || slot >= h->trk->cfg.max_slots) return ISV_ERR_INVALID_ARG;
    memset(state, 0, sizeof(*state));
    if (!h->seq[slot]) return ISV_OK;
    hipStream_t stream = h->trk->stream;
    const size_t P = (size_t)h->cfg.max_points, so = (size_t)slot * P;
    FeSlotHdr hdr;
    HIPCHK(h, hipSetDevice(h->trk->device));
    HIPCHK(h, hipMemcpyAsync(&hdr, h->S.hdr + slot, sizeof(hdr), hipMemcpyDeviceToHost, stream));
    HIPCHK(h, hipStreamSynchronize(stream));
    const size_t n = (size_t)(hdr.n < 0 ? 0 : (hdr.n > (int)P ? (int)P : hdr.n));
    if (n && prev_pts) HIPCHK(h, hipMemcpyAsync(prev_pts, h->S.pts + 2 * so, 8 * n, hipMemcpyDeviceToHost, stream));
    if (n && prev_un_pts) HIPCHK(h, hipMemcpyAsync(prev_un_pts, h->S.un + 2 * so, 8 * n, hipMemcpyDeviceToHost, stream));
    if (n && ids) HIPCHK(h, hipMemcpyAsync(ids, h->S.ids + so, 4 * n, hipMemcpyDeviceToHost, stream));
    if (n && track_cnt) HIPCHK(h, hipMemcpyAsync(track_cnt, h->S.cnt + so, 4 * n, hipMemcpyDeviceToHost, stream));
    if (n && in_map) HIPCHK(h, hipMemcpyAsync(in_map, h->S.map + so, n, hipMemcpyDeviceToHost, stream));
    HIPCHK(h, hipStreamSynchronize(stream));
    state->has_sequence = 1; state->n_points = (int32_t)n; state->n_id = hdr.n_id; state->prev_time = hdr.prev_time;
    return ISV_OK;
}

extern "C" int isv_fe_slot_set(isv_fe_t *h, int32_t slot, const isv_fe_state_t *state, const float *prev_pts, const int32_t *ids, const int32_t *track_cnt,
                               const float *prev_un_pts, const uint8_t *in_map) {
    if (!h || !state || slot < 0 || slot >= h->trk->cfg.max_slots) return ISV_ERR_INVALID_ARG;
    if (!state->has_sequence) return isv_fe_slot_reset(h, slot);
    if (const int rc = fe_check_state(h->cfg.max_points, h->view(slot), state, prev_pts, ids, track_cnt, prev_un_pts, in_map); rc != ISV_OK) {
        h->err = "isv_fe_slot_set: the state was refused";
        return rc;
    }
    hipStream_t stream = h->trk->stream;
    const size_t P = (size_t)h->cfg.max_points, so = (size_t)slot * P, n = (size_t)state->n_points;
    const FeSlotHdr hdr{state->n_points, state->n_id, state->prev_time};
    h->seq[slot] = 0;                              // (a failed copy leaves the slot without a sequence)
    HIPCHK(h, hipSetDevice(h->trk->device));
    HIPCHK(h, hipMemcpyAsync(h->S.hdr + slot, &hdr, sizeof(hdr), hipMemcpyHostToDevice, stream));
    if (n) {
        HIPCHK(h, hipMemcpyAsync(h->S.pts + 2 * so, prev_pts, 8 * n, hipMemcpyHostToDevice, stream));
        HIPCHK(h, hipMemcpyAsync(h->S.un + 2 * so, prev_un_pts, 8 * n, hipMemcpyHostToDevice, stream));
        HIPCHK(h, hipMemcpyAsync(h->S.ids + so, ids, 4 * n, hipMemcpyHostToDevice, stream));
        HIPCHK(h, hipMemcpyAsync(h->S.cnt + so, track_cnt, 4 * n, hipMemcpyHostToDevice, stream));
        HIPCHK(h, hipMemcpyAsync(h->S.map + so, in_map, n, hipMemcpyHostToDevice, stream));
    }
    HIPCHK(h, hipStreamSynchronize(stream));
    h->seq[slot] = 1;
    h->seen[slot] = h->trk->gen[slot];
    return ISV_OK;
}

extern "C" int isv_fe_read_image_batch(isv_fe_t *h, int32_t n, const isv_fe_item_t *const *items, isv_fe_result_t *results, int32_t *const *feature_id,
                                       double *const *point, float *const *uv, float *const *velocity, float *const *cur_pts, float *const *cur_un_pts,
                                       int32_t *const *ids, int32_t *const *track_cnt, float *const *pts_velocity) {
    StageCall call{h ? h->ctx() : StageCtx{}, "isv_fe_read_image_batch"};
    if (const int rc = call.enter(n, items, results); rc != ISV_OK || n == 0) return rc;
    if (n > h->cfg.max_items) return call.fail(ISV_ERR_CAPACITY, "more items than max_items");
    if (!feature_id || !point || !uv || !velocity) return call.fail(ISV_ERR_INVALID_ARG, "null output arrays");
    isv_trk *trk = h->trk;
    isv_eq *eq = h->eq;
    const isv_trk_config_t &tc = trk->cfg;
    const int P = h->cfg.max_points, C = h->cfg.max_cnt;
    const int32_t tag = eq ? eq->id : 0;
    // every refusal, on the host (isv_fe_host.h)
    std::vector<int32_t> status(n), slot_of(n);
    for (int i = 0; i < n; i++) {
        const isv_fe_item_t *it = items[i];
        int s = fe_check_item(tc.max_slots, tc.max_width, tc.max_height, it, feature_id[i] && point[i] && uv[i] && velocity[i]);
        if (s == ISV_TRK_OK) s = fe_check_slot(it, h->view(it->slot));
        status[i] = s; slot_of[i] = it->slot;
    }
    fe_refuse_duplicates(n, slot_of.data(), status.data());
    std::vector<FeItem> fi;
    std::vector<TrkItem> ti;
    std::vector<TrkJob> jobs;
    std::vector<DetItem> di;
    std::vector<int> who;
    size_t n_img = 0, mask_bytes = 0, plane_bytes = 0, maxPix = 0;
    int maxLev = 1, maxLW[kTrkLevels] = {}, maxLH[kTrkLevels] = {}, detW = 0, detH = 0, any_new = 0, any_flow = 0;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    for (int i = 0; i < n; i++) {
        if (status[i] != ISV_TRK_OK) continue;
        const isv_fe_item_t *it = items[i];
        const TrkSlot &sl = trk->slots[it->slot];
        const int par = sl.valid ? sl.par : 0, k = (int)fi.size();
        const size_t px = (size_t)it->width * it->height;
        FeItem F;
        memset(&F, 0, sizeof(F));
        F.slot = it->slot; F.first = !h->seq[it->slot]; F.pub = it->pub_this_frame != 0; F.W = it->width; F.H = it->height; F.cur_time = it->cur_time;
        TrkItem T;
        memset(&T, 0, sizeof(T));
        T.s = trk_make_shape(it->width, it->height);
        T.prev_off = trk->store_off(it->slot, par); T.cur_off = trk->store_off(it->slot, par ^ 1);
        T.np = 0; T.pt_off = k * P;              // np: k_fe_begin
        jobs.push_back(TrkJob{n_img, T.cur_off, T.s});
        n_img += (px + 15) & ~(size_t)15;
        DetItem D;
        memset(&D, 0, sizeof(D));
        D.img_off = T.cur_off; D.W = it->width; D.H = it->height; D.pt_off = k * P; D.out_off = k * C;     // np, max_new: k_fe_after_reject
        D.mask_off = mask_bytes; mask_bytes += al(px);
        if (F.pub || F.first) {
            D.eig_off = plane_bytes; plane_bytes += al(4 * px);
            D.key_off = plane_bytes; plane_bytes += al(8 * px);
            any_new = 1;
            if (it->width > detW) detW = it->width;
            if (it->height > detH) detH = it->height;
            if (px > maxPix) maxPix = px;
        }
        if (!F.first) any_flow = 1;
        if (T.s.nlev > maxLev) maxLev = T.s.nlev;
        for (int l = 0; l < T.s.nlev; l++) {
            if (T.s.lw[l] > maxLW[l]) maxLW[l] = T.s.lw[l];
            if (T.s.lh[l] > maxLH[l]) maxLH[l] = T.s.lh[l];
        }
        fi.push_back(F); ti.push_back(T); di.push_back(D); who.push_back(i);
    }
    const int m = (int)fi.size();
    auto refuse = [&](int i) {
        results[i] = isv_fe_result_t{};
        results[i].status = status[i];
    };
    if (m == 0) {
        for (int i = 0; i < n; i++) refuse(i);
        return ISV_OK;
    }
    const size_t mp = (size_t)m * P, mc = (size_t)m * C;
    if (mp > INT32_MAX / 4) return call.fail(ISV_ERR_CAPACITY, "batch too large");
    // one block: [the records | the disc table | the images], uploaded; [the detector's counts], zeroed; then, device only, every
    // stage's per-point sections at k * max_points, the outputs, the mask planes (set to 255), the response planes and key lists
    BlockLayout L;
    const size_t o_fi = L.add(sizeof(FeItem) * m), o_ti = L.add(sizeof(TrkItem) * m), o_job = L.add(sizeof(TrkJob) * m), o_di = L.add(sizeof(DetItem) * m),
                 o_hw = L.add(kDetMaxR + 1), o_img = L.add(n_img + 16);
    const size_t up_end = L.end;
    const size_t o_dc = L.add(sizeof(DetCount) * m);
    const size_t clear_end = L.end;
    const size_t o_fp = L.add(8 * mp), o_cp = L.add(8 * mp), o_un = L.add(8 * mp), o_er = L.add(4 * mp), o_fl = L.add(mp);
    const size_t o_rh = L.add(sizeof(RejHdr) * m), o_rp = L.add(16 * mp), o_rr = L.add(sizeof(isv_rej_result_t) * m), o_rs = L.add(mp);
    const size_t o_aid = L.add(4 * mp), o_acn = L.add(4 * mp), o_apu = L.add(8 * mp), o_ama = L.add(mp), o_fc = L.add(sizeof(FeCount) * m);
    const size_t o_dp = L.add(sizeof(DetPoint) * mp), o_kept = L.add(4 * mp), o_np = L.add(8 * mc), o_nu = L.add(8 * mc);
    const size_t o_res = L.add(sizeof(isv_fe_result_t) * m), o_mid = L.add(4 * mp), o_mpt = L.add(24 * mp), o_muv = L.add(8 * mp), o_mve = L.add(8 * mp);
    const size_t o_lcp = L.add(8 * mp), o_lun = L.add(8 * mp), o_lid = L.add(4 * mp), o_lcn = L.add(4 * mp), o_lve = L.add(8 * mp);
    const size_t o_lut = eq ? L.add(eq->lut_bytes() * m) : 0;
    const size_t o_mask = L.add(mask_bytes), o_plane = L.add(plane_bytes + 256);
    for (int k = 0; k < m; k++) {
        di[k].mask_off += o_mask;
        if (fi[k].pub || fi[k].first) { di[k].eig_off += o_plane; di[k].key_off += o_plane; }
    }
    std::vector<char> &up = h->up;
    up.resize(up_end);
    memcpy(up.data() + o_fi, fi.data(), sizeof(FeItem) * m);
    memcpy(up.data() + o_ti, ti.data(), sizeof(TrkItem) * m);
    memcpy(up.data() + o_job, jobs.data(), sizeof(TrkJob) * m);
    memcpy(up.data() + o_di, di.data(), sizeof(DetItem) * m);
    memcpy(up.data() + o_hw, h->det->hw, kDetMaxR + 1);
    for (int k = 0; k < m; k++) {
        const isv_fe_item_t *it = items[who[k]];
        char *dst = up.data() + o_img + jobs[k].src_off;
        if (it->stride == it->width) memcpy(dst, it->cur, (size_t)it->width * it->height);
        else for (int y = 0; y < it->height; y++) memcpy(dst + (size_t)y * it->width, it->cur + (size_t)y * it->stride, it->width);
    }
    hipStream_t stream = trk->stream;
    const bool lists = cur_pts || cur_un_pts || ids || track_cnt || pts_velocity;
    std::vector<isv_fe_result_t> res(m);
    // the downloads' host image: the message, then the lists
    const size_t b_mid = 0, b_mpt = b_mid + 4 * mp, b_muv = b_mpt + 24 * mp, b_mve = b_muv + 8 * mp, b_lcp = b_mve + 8 * mp, b_lun = b_lcp + 8 * mp, b_lid = b_lun + 8 * mp,
                 b_lcn = b_lid + 4 * mp, b_lve = b_lcn + 4 * mp, b_end = b_lve + 8 * mp;
    std::vector<char> dl(b_end);
    auto to = [&](size_t b, bool wanted) { return wanted ? (void *)(dl.data() + b) : nullptr; };
    const int rc = call.run(
        up, {{up_end, clear_end}, {o_mask, o_mask + mask_bytes, 0xff}}, L.end,
        [&](char *d, auto &&mark) {
            const FeItem *dfi = (const FeItem *)(d + o_fi);
            TrkItem *dti = (TrkItem *)(d + o_ti);
            FeCount *dfc = (FeCount *)(d + o_fc);
            auto no_mark = [] {};
            hipLaunchKernelGGL(k_fe_begin, dim3(m), dim3(kLanes), 0, stream, dfi, dti, h->S, (float *)(d + o_fp), P);
            trk_enqueue_pyramids(trk, eq, (const TrkJob *)(d + o_job), m, (const uint8_t *)(d + o_img), eq ? (uint8_t *)(d + o_lut) : nullptr, maxLev, maxLW, maxLH, no_mark);
            mark();
            trk_enqueue_track(trk, dti, m, any_flow ? P : 0, (const float *)(d + o_fp), (float *)(d + o_cp), (float *)(d + o_un), (float *)(d + o_er), (uint8_t *)(d + o_fl));
            hipLaunchKernelGGL(k_fe_after_flow, dim3(m), dim3(kLanes), 0, stream, dfi, (const TrkItem *)dti, h->S, (const float *)(d + o_fp), (const float *)(d + o_cp),
                               (const uint8_t *)(d + o_fl), (RejHdr *)(d + o_rh), (float *)(d + o_rp), (int32_t *)(d + o_aid), (int32_t *)(d + o_acn), (float *)(d + o_apu),
                               (uint8_t *)(d + o_ama), dfc, P);
            mark();
            rej_enqueue(h->rej, (const RejHdr *)(d + o_rh), m, P, (const float *)(d + o_rp), (isv_rej_result_t *)(d + o_rr), (uint8_t *)(d + o_rs));
            hipLaunchKernelGGL(k_fe_after_reject, dim3(m), dim3(kLanes), 0, stream, dfi, dfc, (const uint8_t *)(d + o_rs), (const float *)(d + o_rp),
                               (const int32_t *)(d + o_acn), (DetItem *)(d + o_di), (DetPoint *)(d + o_dp), C, P);
            mark();
            det_enqueue(h->det, (const DetItem *)(d + o_di), m, (const DetPoint *)(d + o_dp), (const uint8_t *)(d + o_hw), d, (DetCount *)(d + o_dc),
                        (int32_t *)(d + o_kept), (float *)(d + o_np), (float *)(d + o_nu), any_new, detW, detH, maxPix, no_mark);
            const FeOut O{(isv_fe_result_t *)(d + o_res), (int32_t *)(d + o_mid), (double *)(d + o_mpt), (float *)(d + o_muv), (float *)(d + o_mve),
                          (float *)(d + o_lcp), (float *)(d + o_lun), (int32_t *)(d + o_lid), (int32_t *)(d + o_lcn), (float *)(d + o_lve)};
            hipLaunchKernelGGL(k_fe_finish, dim3(m), dim3(kLanes), 0, stream, dfi, (const FeCount *)dfc, (const DetCount *)(d + o_dc), (const int32_t *)(d + o_kept),
                               (const float *)(d + o_np), (const isv_rej_result_t *)(d + o_rr), (const float *)(d + o_rp), (const int32_t *)(d + o_aid),
                               (const int32_t *)(d + o_acn), (const float *)(d + o_apu), (const uint8_t *)(d + o_ama), h->S, trk->cam, O, C, P);
        },
        {{res.data(), o_res, sizeof(isv_fe_result_t) * m}, {dl.data() + b_mid, o_mid, 4 * mp}, {dl.data() + b_mpt, o_mpt, 24 * mp}, {dl.data() + b_muv, o_muv, 8 * mp},
         {dl.data() + b_mve, o_mve, 8 * mp}, {to(b_lcp, cur_pts), o_lcp, 8 * mp}, {to(b_lun, cur_un_pts), o_lun, 8 * mp}, {to(b_lid, ids), o_lid, 4 * mp},
         {to(b_lcn, track_cnt), o_lcn, 4 * mp}, {to(b_lve, pts_velocity), o_lve, 8 * mp}},
        [&] {
            for (int i = 0; i < n; i++)
                if (status[i] != ISV_TRK_OK) refuse(i);
            for (int k = 0; k < m; k++) {
                const int i = who[k], sl = fi[k].slot;
                const isv_fe_result_t &r = res[k];
                const size_t at = (size_t)k * P, nm = (size_t)r.n_msg, np = (size_t)r.n_points;
                results[i] = r;
                if (nm) {
                    memcpy(feature_id[i], dl.data() + b_mid + 4 * at, 4 * nm);
                    memcpy(point[i], dl.data() + b_mpt + 24 * at, 24 * nm);
                    memcpy(uv[i], dl.data() + b_muv + 8 * at, 8 * nm);
                    memcpy(velocity[i], dl.data() + b_mve + 8 * at, 8 * nm);
                }
                if (lists && np) {
                    if (cur_pts && cur_pts[i]) memcpy(cur_pts[i], dl.data() + b_lcp + 8 * at, 8 * np);
                    if (cur_un_pts && cur_un_pts[i]) memcpy(cur_un_pts[i], dl.data() + b_lun + 8 * at, 8 * np);
                    if (ids && ids[i]) memcpy(ids[i], dl.data() + b_lid + 4 * at, 4 * np);
                    if (track_cnt && track_cnt[i]) memcpy(track_cnt[i], dl.data() + b_lcn + 4 * at, 4 * np);
                    if (pts_velocity && pts_velocity[i]) memcpy(pts_velocity[i], dl.data() + b_lve + 8 * at, 8 * np);
                }
                trk->slots[sl] = TrkSlot{fi[k].W, fi[k].H, (int32_t)((ti[k].cur_off - trk->store_off(sl, 0)) / trk->slot_bytes), 1, tag};
                h->seen[sl] = ++trk->gen[sl];
                h->seq[sl] = 1;
            }
            return hipSuccess;
        });
    if (rc != ISV_OK) {                            // what the kernels left in the buffers is unknown
        for (int k = 0; k < m; k++) {
            trk->slots[fi[k].slot] = TrkSlot{};
            trk->gen[fi[k].slot]++;
            h->seq[fi[k].slot] = 0;
        }
    }
    return rc;
}
