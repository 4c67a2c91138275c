/*
 * isv_rej_oracle.c -- the serial CPU restatement of include/isvins_reject.h: FeatureTracker::rejectWithF of one item, that is the lift
 * of both point sets to the virtual pinhole and cv::findFundamentalMat(m1, m2, FM_RANSAC, f_threshold, 0.99, status) of OpenCV 3.2.0
 * (RANSAC from 15 points on, LMedS below), as plain serial loops in the order the header states them (J1..J6 marked).  It pins the
 * kernel k_rej_f of is-vins_amd/csrc/isv_reject.hip; tests/test_rej_oracle.py pins it against numpy statements and against the
 * Python-integer reading of tests/relpose_highprec.py.  TEST INFRASTRUCTURE ONLY: built by the tests into a temporary directory with
 *   gcc -O2 -ffp-contract=off -shared -fPIC
 * and never linked into the library.  The serial pieces are the kernel's own text (isv_init_common.h, isv_pinhole.h, isv_reject.h)
 * compiled for the host, so the two differ only where libm and the device math library round acos / cos / pow / log apart.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../is-vins_amd/csrc/isv_init_common.h"
#include "../../is-vins_amd/csrc/isv_pinhole.h"
#include "../../is-vins_amd/csrc/isv_reject.h"

/* test hook: a set bit replaces a reproduced quirk by the "obvious" behaviour, so that the tests can show each quirk matters.
 * 1: J1, the estimator sees the double points; 2: J2, the error stays double (in the LMedS median too) against the double
 * bound; 4: J3, RANSAC below 15 points too; 8: J4, the errors are sorted as floats (an insertion sort by `<`: a NaN stays where it stands). */
static int g_quirk_off = 0;
void isvo_rej_set_quirks_off(int mask) { g_quirk_off = mask; }

/* the iterations at which the last isvo_rej_reject kept a model (the first REJ_KEEPS of them), for the case table's edges */
#define REJ_KEEPS 64
static int g_keeps[REJ_KEEPS], g_n_keeps = 0;
int isvo_rej_last_keeps(int32_t *out, int cap) {
    const int n = g_n_keeps < REJ_KEEPS ? g_n_keeps : REJ_KEEPS;
    for (int i = 0; i < n && i < cap; i++) out[i] = g_keeps[i];
    return g_n_keeps;
}
static void note_keep(int iter) {
    if (g_n_keeps < REJ_KEEPS) g_keeps[g_n_keeps] = iter;
    g_n_keeps++;
}

int isvo_rej_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(isv_rej_config_t);
    case 1: return (int)sizeof(isv_rej_item_t);
    case 2: return (int)sizeof(isv_rej_result_t);
    default: return -1;
    }
}

static PinholeCam cam_of(const isv_trk_config_t *t) { return pinhole_make(t->fx, t->fy, t->cx, t->cy, t->k1, t->k2, t->p1, t->p2); }

/* 1 when isv_rej_create accepts the configuration on a tracker of `trk_max_points` */
int isvo_rej_check_config(const isv_rej_config_t *c, int trk_max_points) { return c && rej_check_config(c) && c->max_points <= trk_max_points; }

/* the status isv_rej_reject_batch gives an item (has_out: its status array is not null) */
int isvo_rej_check(const isv_rej_config_t *c, const isv_rej_item_t *it, int has_out) {
    static const uint8_t some = 0;
    return rej_check_item(c, it, has_out ? &some : NULL);
}

/* the lift of n pixels [n][2] -> out [n][2] float32 (J1) */
void isvo_rej_lift(const isv_trk_config_t *t, const isv_rej_config_t *c, int width, int height, int n, const float *px, float *out) {
    const PinholeCam cam = cam_of(t);
    for (int i = 0; i < n; i++) rej_lift(&cam, c->focal_length, width / 2.0, height / 2.0, px[2 * i], px[2 * i + 1], &out[2 * i], &out[2 * i + 1]);
}

int isvo_rej_lmeds_niters(void) { return rej_lmeds_niters(); }
double isvo_rej_sigma(int count, double min_median) { return rej_sigma(count, min_median); }
uint32_t isvo_rej_uniform(uint64_t *state, uint32_t n) { return rp_uniform(state, n); }
/* n_sub successive subsets of 7 out of count from `*state` on: idx [n_sub][7] */
void isvo_rej_subsets(uint64_t *state, int count, int n_sub, int32_t *idx) {
    for (int s = 0; s < n_sub; s++) {
        int v[7];
        rp_subset(state, count, v);
        for (int k = 0; k < 7; k++) idx[7 * s + k] = v[k];
    }
}

/* the LMedS median of count errors (e is reordered) */
double isvo_rej_median(float *e, int count) {
    if (!(g_quirk_off & 8)) return rej_median(e, count);   /* J4 */
    for (int i = 1; i < count; i++) {
        const float v = e[i];
        int j = i - 1;
        for (; j >= 0 && v < e[j]; j--) e[j + 1] = e[j];
        e[j + 1] = v;
    }
    return count % 2 != 0 ? (double)e[count / 2] : (double)(float)(e[count / 2 - 1] + e[count / 2]) * 0.5;
}

/* with the hook for J2: the median of the double errors, sorted as doubles */
static double median_double(double *e, int count) {
    for (int i = 1; i < count; i++) {
        const double v = e[i];
        int j = i - 1;
        for (; j >= 0 && v < e[j]; j--) e[j + 1] = e[j];
        e[j + 1] = v;
    }
    return count % 2 != 0 ? e[count / 2] : (e[count / 2 - 1] + e[count / 2]) * 0.5;
}

/* computeError of one correspondence as the registrators read it: float32 (J2), or double with the hook */
static double err_of(const double *F, const double *q) {
    const double e = rp_fm_error(F, q[0], q[1], q[2], q[3]);
    return (g_quirk_off & 2) ? e : (double)(float)e;
}
static double bound_of(double thresh) { return (g_quirk_off & 2) ? thresh * thresh : (double)(float)(thresh * thresh); }

/* rejectWithF of one item.  status: [n_points] (may be NULL when n_points is 0).  Returns the item's status. */
int isvo_rej_reject(const isv_trk_config_t *t, const isv_rej_config_t *c, const isv_rej_item_t *it, isv_rej_result_t *res, uint8_t *status) {
    memset(res, 0, sizeof(*res));
    res->min_median = -1.0;
    res->n_points = it->n_points;
    res->status = rej_check_item(c, it, status);
    if (res->status != ISV_TRK_OK) return res->status;
    const int count = it->n_points;
    if (count < ISV_REJ_MIN_POINTS) {                  /* prev_pts.size() >= 8 */
        for (int j = 0; j < count; j++) status[j] = 1;
        res->n_kept = count;
        return ISV_TRK_OK;
    }
    const PinholeCam cam = cam_of(t);
    double *pts = (double *)malloc(sizeof(double) * 4 * (size_t)count);
    for (int j = 0; j < count; j++)
        for (int side = 0; side < 2; side++) {
            const float *px = (side ? it->cur_pts : it->prev_pts) + 2 * j;   /* m1 = prev, m2 = cur */
            if (g_quirk_off & 1) {
                double bx, by;
                pinhole_lift_d(&cam, (double)px[0], (double)px[1], &bx, &by);
                pts[4 * j + 2 * side] = c->focal_length * bx / 1.0 + it->width / 2.0;
                pts[4 * j + 2 * side + 1] = c->focal_length * by / 1.0 + it->height / 2.0;
            } else {
                float x, y;
                rej_lift(&cam, c->focal_length, it->width / 2.0, it->height / 2.0, px[0], px[1], &x, &y);   /* J1 */
                pts[4 * j + 2 * side] = x; pts[4 * j + 2 * side + 1] = y;
            }
        }
    const int lmeds = count < ISV_REJ_RANSAC_MIN && !(g_quirk_off & 4);   /* J3 */
    uint64_t rng = ~0ull;                                                 /* J6: RNG((uint64)-1) in every call */
    double F[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bound = bound_of(c->f_threshold), min_median = DBL_MAX;
    int niters = lmeds ? rej_lmeds_niters() : RP_MAX_ITERS, max_good = 0, kept = 0, iter;
    float e[REJ_MAX_MODEL_PTS];
    double ed[REJ_MAX_MODEL_PTS];
    g_n_keeps = 0;
    for (iter = 0; iter < niters; iter++) {
        int idx[7];
        double sub[28], Fm[27];
        rp_subset(&rng, count, idx);
        for (int k = 0; k < 7; k++) memcpy(sub + 4 * k, pts + 4 * idx[k], 4 * sizeof(double));
        const int nm = rp_run7point(sub, Fm);
        if (nm < 1 || nm > 3) continue;
        for (int m = 0; m < nm; m++) {
            if (lmeds) {
                double median;
                if (g_quirk_off & 2) {
                    for (int j = 0; j < count; j++) ed[j] = rp_fm_error(Fm + 9 * m, pts[4 * j], pts[4 * j + 1], pts[4 * j + 2], pts[4 * j + 3]);
                    median = median_double(ed, count);
                } else {
                    for (int j = 0; j < count; j++) e[j] = (float)rp_fm_error(Fm + 9 * m, pts[4 * j], pts[4 * j + 1], pts[4 * j + 2], pts[4 * j + 3]);   /* J2 */
                    median = isvo_rej_median(e, count);
                }
                if (median < min_median) {
                    min_median = median;
                    memcpy(F, Fm + 9 * m, sizeof(F));
                    kept = 1;
                    note_keep(iter);
                }
            } else {
                int g = 0;
                for (int j = 0; j < count; j++) g += err_of(Fm + 9 * m, pts + 4 * j) <= bound;   /* J2 */
                if (g > (max_good > 6 ? max_good : 6)) {
                    memcpy(F, Fm + 9 * m, sizeof(F));
                    max_good = g;
                    kept = 1;
                    note_keep(iter);
                    niters = rp_update_num_iters(RP_CONFIDENCE, (double)(count - g) / count, 7, niters);
                }
            }
        }
    }
    if (lmeds && kept) {
        const double sigma = rej_sigma(count, min_median);
        bound = bound_of(sigma);
    }
    int n_kept = 0;
    for (int j = 0; j < count; j++) {
        status[j] = kept && err_of(F, pts + 4 * j) <= bound;   /* J5: nothing kept, every point rejected */
        n_kept += status[j];
    }
    free(pts);
    res->n_kept = n_kept;
    res->method = lmeds ? ISV_REJ_LMEDS : ISV_REJ_RANSAC;
    res->iters = lmeds ? niters : iter;
    res->best_inliers = kept ? (lmeds ? n_kept : max_good) : 0;
    res->min_median = lmeds && kept ? min_median : -1.0;
    return ISV_TRK_OK;
}
