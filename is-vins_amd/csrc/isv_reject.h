/*
 * isv_reject.h -- internal to the outlier rejection (isv_reject.hip), outside include/: what the kernel k_rej_f shares with its CPU
 * restatement tests/native/isv_rej_oracle.c, as plain C that compiles as HIP device code (ISV_HD) or as host C, beside the serial
 * pieces of isv_init_common.h: the lift to the virtual pinhole, the LMedS iteration count, median and sigma, and the item check
 * (host).  Every includer turns FP contraction off for its whole translation unit.  The quirks J1..J6 are those of
 * include/isvins_reject.h.  Below, for HIP only, the estimator as one device routine (k_rej_f's and k_exr_calibrate's) and the
 * rejector handle.
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

constexpr int kRejLanes = 64;

// the estimator's LDS, one per workgroup: a chunk of up to 64 hypotheses, then what the estimator leaves
struct RejEstLds {
    int16_t sub[kRejLanes][7];    // the chunk's subsets
    double F[kRejLanes][27];      // their models
    double med[kRejLanes][3];     // LMedS: their medians
    int nm[kRejLanes], good[kRejLanes][3];
    double best[9];               // the kept model
    double min_median;            // LMedS: its median (DBL_MAX when nothing was kept)
    float bound;                  // the kept model's float32 inlier bound
    int cnt, more;
    int kept, iters, max_good;    // a model was kept; the RANSAC iterations run, or the LMedS niters; RANSAC: the kept model's inliers
};

// OpenCV 3.2's cv::findFundamentalMat(m1, m2, FM_RANSAC, thresh, 0.99) on `count` >= 8 float32 correspondences (x0 y0 x1 y1) in LDS,
// without the mask: k_rej_f's estimator (isv_reject.hip has the account) and k_exr_calibrate's (isv_exrot.hip).  Every lane of the
// 64-lane workgroup calls it, the points being visible to all; behind its last barrier E.kept, E.best, E.bound, E.iters, E.max_good and
// E.min_median hold.  RANSAC from 15 points on, LMedS below; speculative chunks of up to 64 hypotheses, committed by lane 0 in serial
// order; a fresh RNG((uint64)-1); float32 errors against float32 bounds; no refit.
static __device__ void rej_estimate(const float4 *Lp, int count, double thresh, RejEstLds &E) {
    const int t = threadIdx.x;
    const bool lmeds = count < ISV_REJ_RANSAC_MIN;     // J3
    const float tf = (float)(thresh * thresh);         // J2
    uint64_t rng = ~0ull;                      // lane 0's: RNG((uint64)-1), fresh per call (J6)
    int iter = 0, niters = lmeds && t == 0 ? rej_lmeds_niters() : RP_MAX_ITERS, max_good = 0, kept = 0;   // lane 0's
    double min_median = DBL_MAX;               // lane 0's
    for (;;) {
        if (t == 0) {
            const int cnt = niters - iter < kRejLanes ? niters - iter : kRejLanes;
            for (int h = 0; h < cnt; h++) {
                int idx[7];
                rp_subset(&rng, count, idx);
                for (int k = 0; k < 7; k++) E.sub[h][k] = (int16_t)idx[k];
            }
            E.cnt = cnt;
        }
        __syncthreads();
        const int cnt = E.cnt;
        if (t < cnt) {
            double p[28];
            for (int k = 0; k < 7; k++) {
                const float4 v = Lp[E.sub[t][k]];
                p[4 * k] = v.x; p[4 * k + 1] = v.y; p[4 * k + 2] = v.z; p[4 * k + 3] = v.w;
            }
            int nm = rp_run7point(p, E.F[t]);
            nm = nm < 1 || nm > 3 ? 0 : nm;
            E.nm[t] = nm;
            for (int m = 0; m < nm; m++) {
                double F[9];
                for (int k = 0; k < 9; k++) F[k] = E.F[t][9 * m + k];
                if (lmeds) {
                    float e[REJ_MAX_MODEL_PTS];
                    for (int j = 0; j < count; j++) {
                        const float4 v = Lp[j];
                        e[j] = (float)rp_fm_error(F, v.x, v.y, v.z, v.w);
                    }
                    E.med[t][m] = rej_median(e, count);             // J4
                } else {
                    int g = 0;
                    for (int j = 0; j < count; j++) {
                        const float4 v = Lp[j];
                        g += (float)rp_fm_error(F, v.x, v.y, v.z, v.w) <= tf;   // J2
                    }
                    E.good[t][m] = g;
                }
            }
        }
        __syncthreads();
        if (t == 0) {   // the serial loop over this chunk, in iteration order
            for (int h = 0; h < cnt && iter < niters; h++, iter++)
                for (int m = 0; m < E.nm[h]; m++) {
                    if (lmeds) {
                        const double median = E.med[h][m];
                        if (median < min_median) {
                            min_median = median;
                            for (int k = 0; k < 9; k++) E.best[k] = E.F[h][9 * m + k];
                            kept = 1;
                        }
                    } else {
                        const int g = E.good[h][m];
                        if (g > (max_good > 6 ? max_good : 6)) {
                            for (int k = 0; k < 9; k++) E.best[k] = E.F[h][9 * m + k];
                            max_good = g;
                            kept = 1;
                            niters = rp_update_num_iters(RP_CONFIDENCE, (double)(count - g) / count, 7, niters);
                        }
                    }
                }
            E.more = iter < niters;
        }
        __syncthreads();
        if (!E.more) break;
    }
    if (t == 0) {
        float bound = tf;
        if (lmeds && kept) {
            const double sigma = rej_sigma(count, min_median);
            bound = (float)(sigma * sigma);
        }
        E.bound = bound;
        E.kept = kept; E.iters = lmeds ? niters : iter; E.max_good = max_good; E.min_median = min_median;
    }
    __syncthreads();
}

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
