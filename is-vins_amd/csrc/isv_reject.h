/*
 * isv_reject.h -- internal to the outlier rejection (isv_reject.hip), outside include/: what the kernel k_rej_f shares with its CPU
 * restatement tests/native/isv_rej_oracle.c, as plain C that compiles as HIP device code (ISV_HD) or as host C, beside the serial
 * pieces of isv_init_common.h: the lift to the virtual pinhole, the LMedS iteration count, median and sigma, and the item check
 * (host).  Every includer turns FP contraction off for its whole translation unit.  The quirks J1..J6 are those of
 * include/isvins_reject.h.  Below, for HIP only, the rejector handle.
 */
#ifndef ISV_REJECT_H
#define ISV_REJECT_H
#include <string.h>
#include "../../include/isvins_reject.h"
#include "isv_init_common.h"
#include "isv_pinhole.h"

#define REJ_MAX_MODEL_PTS (ISV_REJ_RANSAC_MIN - 1)   /* LMedS sees at most 14 points */

/* rejectWithF's lift of one pixel (feature_tracker_simple.cpp:161-165): liftProjective in doubles, b.z = 1.0, then the virtual
 * pinhole, then cv::Point2f (J1) */
ISV_HD void rej_lift(const PinholeCam *cam, double focal, double half_w, double half_h, float px, float py, float *ox, float *oy) {
    double bx, by;
    pinhole_lift_d(cam, (double)px, (double)py, &bx, &by);
    const double x = focal * bx / 1.0 + half_w, y = focal * by / 1.0 + half_h;
    *ox = (float)x; *oy = (float)y;
}

/* LMeDSPointSetRegistrator::run: niters = max(RANSACUpdateNumIters(confidence, 0.45, modelPoints, maxIters), 3) */
ISV_HD int rej_lmeds_niters(void) {
    const int n = rp_update_num_iters(RP_CONFIDENCE, 0.45, 7, RP_MAX_ITERS);
    return n > 3 ? n : 3;
}

/* the median of count float32 errors (e is sorted in place), as LMeDSPointSetRegistrator::run takes it:
 * std::sort(errf.ptr<int>(), errf.ptr<int>() + count), that is the 32-bit patterns as signed integers (J4; an insertion sort: the
 * order of integers is total, so every sort gives this result), then the middle entry or the float32 sum of the two middle entries
 * times 0.5 in double */
ISV_HD double rej_median(float *e, int count) {
    for (int i = 1; i < count; i++) {
        const float v = e[i];
        int32_t vi, ui;
        memcpy(&vi, &v, 4);
        int j = i - 1;
        for (; j >= 0; j--) {
            memcpy(&ui, &e[j], 4);
            if (!(ui > vi)) break;
            e[j + 1] = e[j];
        }
        e[j + 1] = v;
    }
    return count % 2 != 0 ? (double)e[count / 2] : (double)(float)(e[count / 2 - 1] + e[count / 2]) * 0.5;
}

/* the inlier threshold LMedS derives from its best median: sigma = 2.5 * 1.4826 * (1 + 5. / (count - modelPoints)) * sqrt(minMedian),
 * at least 0.001 */
ISV_HD double rej_sigma(int count, double min_median) {
    double sigma = 2.5 * 1.4826 * (1 + 5. / (count - 7)) * sqrt(min_median);
    sigma = sigma > 0.001 ? sigma : 0.001;   /* MAX(sigma, 0.001) */
    return sigma;
}

#define REJ_FINITE(v) ((v) - (v) == 0)   /* neither an infinity nor a NaN */

/* the per-item refusals of isv_rej_reject_batch, in their order; `out` is the item's status array */
static int rej_check_item(const isv_rej_config_t *cfg, const isv_rej_item_t *it, const uint8_t *out) {
    if (it->width < 1 || it->width > 8192 || it->height < 1 || it->height > 8192 || it->n_points < 0) return ISV_TRK_INPUT;
    if (it->n_points > cfg->max_points) return ISV_TRK_CAPACITY;
    if (it->n_points > 0 && (!it->prev_pts || !it->cur_pts || !out)) return ISV_TRK_INPUT;
    for (int k = 0; k < 2 * it->n_points; k++)
        if (!REJ_FINITE(it->prev_pts[k]) || !REJ_FINITE(it->cur_pts[k])) return ISV_TRK_INPUT;
    return ISV_TRK_OK;
}

/* isv_rej_create's refusals that need no tracker */
static int rej_check_config(const isv_rej_config_t *c) {
    return c->max_items >= 1 && c->max_items <= 65535 && c->max_points >= 1 && c->max_points <= ISV_REJ_MAX_POINTS && REJ_FINITE(c->focal_length) &&
           c->focal_length > 0.0 && REJ_FINITE(c->f_threshold) && c->f_threshold > 0.0;
}

#ifdef __HIPCC__
#include "isv_tracker.h"

struct isv_rej {
    isv_rej_config_t cfg;
    isv_trk *trk = nullptr;
    std::string err;
    StageSlot slot;               // the call's device block (grow-only), events and times
    double pack_ms = 0;
    StageCtx ctx() { return StageCtx{trk->device, trk->stream, &slot, &err}; }   // (the device and the stream are the tracker's)
    std::vector<char> up;
};

struct RejHdr {                   // per-item record
    int64_t pt_off;               // the item's first point: into the points (4 floats each) and into the status bytes
    int32_t n, pad;
    double half_w, half_h;        // COL / 2.0, ROW / 2.0
};

// k_rej_f on `m` device-resident records, on the tracker's stream (isv_rej_reject_batch's launch, and isv_frontend.hip's): the points of
// record k are d_pts + 4 * pt_off, prev [n][2] then cur [n][2]; max_n bounds every record's n (the kernel's dynamic LDS)
void rej_enqueue(isv_rej *h, const RejHdr *d_hdrs, int m, int max_n, const float *d_pts, isv_rej_result_t *d_results, uint8_t *d_status);
#endif
#endif /* ISV_REJECT_H */
