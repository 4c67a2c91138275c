/*
 * isv_exr_oracle.c -- the serial CPU restatement of include/isvins_exrot.h: InitialEXRotation::CalibrationExRotation with
 * solveRelativeR, testTriangulation and decomposeE (src/initial/initial_ex_rotation.cpp), one call per item over a host-side slot
 * store, as plain serial loops in the order the header states them (X1..X8 marked).  It pins the kernel k_exr_calibrate of
 * is-vins_amd/csrc/isv_exrot.hip; tests/test_exr_oracle.py pins it against numpy statements and against the Python-integer reading
 * of tests/relpose_highprec.py, tests/exr_highprec.py against a 40-digit reading.  TEST INFRASTRUCTURE ONLY: built by the tests into
 * a temporary directory with
 *   gcc -O2 -ffp-contract=off -shared -fPIC
 * and never linked into the library.  The serial pieces are the kernel's own text (isv_init_common.h, isv_reject.h, isv_exrot.h)
 * compiled for the host, so the two differ only where libm and the device math library round acos / cos / pow / log / atan2 apart.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../is-vins_amd/csrc/isv_init_common.h"
#include "../../is-vins_amd/csrc/isv_reject.h"
#include "../../is-vins_amd/csrc/isv_exrot.h"

/* test hook: a set bit replaces a reproduced quirk by the "obvious" behaviour, so that the tests can show each quirk matters.
 * 1: X1, the estimator and the triangulation see the double correspondences; 2: X4, no float32 anywhere in testTriangulation (the
 * camera, the homogeneous point and the depths stay double). */
static int g_quirk_off = 0;
void isvo_exr_set_quirks_off(int mask) { g_quirk_off = mask; }

/* what the last isvo_exr_calibrate_batch's last good item left, for the case table's edges and the high-precision reading */
static struct {
    int keep_iter, n_keeps, subset[7];
    double F[9], R1[9], R2[9], t[3], det_first;
    double *A; int rows;           /* A as built, before the QR */
} g_last;

int isvo_exr_last(int32_t *keep_iter, int32_t *n_keeps, int32_t *subset, double *F, double *R1, double *R2, double *t, double *det_first) {
    *keep_iter = g_last.keep_iter; *n_keeps = g_last.n_keeps;
    for (int k = 0; k < 7; k++) subset[k] = g_last.subset[k];
    memcpy(F, g_last.F, sizeof(g_last.F)); memcpy(R1, g_last.R1, 72); memcpy(R2, g_last.R2, 72); memcpy(t, g_last.t, 24);
    *det_first = g_last.det_first;
    return g_last.rows;
}
/* A [rows][4] of that item, before the QR */
void isvo_exr_last_A(double *out) { if (g_last.rows) memcpy(out, g_last.A, sizeof(double) * 4 * (size_t)g_last.rows); }

int isvo_exr_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(isv_exr_config_t);
    case 1: return (int)sizeof(isv_exr_item_t);
    case 2: return (int)sizeof(isv_exr_result_t);
    default: return -1;
    }
}

int isvo_exr_check_config(const isv_exr_config_t *c) { return c && exr_check_config(c); }
int isvo_exr_check(const isv_exr_config_t *c, const isv_exr_item_t *it, const int32_t *frame_counts, const uint8_t *named) {
    return exr_check_item(c, it, frame_counts, named);
}

/* ---- the pieces, one by one ---- */
int isvo_exr_method(int n) { return n < ISV_EXR_MIN_CORRES ? ISV_EXR_NONE : n < ISV_EXR_RANSAC_MIN ? ISV_EXR_LMEDS : ISV_EXR_RANSAC; }
uint32_t isvo_exr_uniform(uint64_t *state, uint32_t n) { return rp_uniform(state, n); }
void isvo_exr_subsets(uint64_t *state, int count, int n_sub, int32_t *idx) {
    for (int s = 0; s < n_sub; s++) {
        int v[7];
        rp_subset(state, count, v);
        for (int k = 0; k < 7; k++) idx[7 * s + k] = v[k];
    }
}
void isvo_exr_q_from_R(const double *m, double *q) { exr_q_from_R(m, q); }
void isvo_exr_q_to_R(const double *q, double *R) { exr_q_to_R(q, R); }
void isvo_exr_inv3(const double *m, double *o) { exr_inv3(m, o); }
void isvo_exr_imu_rows(const double *ric, const double *dq, double *Rimu, double *Rc_g) { exr_imu_rows(ric, dq, Rimu, Rc_g); }
void isvo_exr_row(const double *Rc, const double *Rimu, const double *Rc_g, double *angle, double *huber, double *blk) { exr_row(Rc, Rimu, Rc_g, angle, huber, blk); }
int isvo_exr_calibrated(int frame_count, int vo_size, const double *singular) { return exr_calibrated(frame_count, vo_size, singular); }
int isvo_exr_decompose(const double *E, double *R1, double *R2, double *t) { return exr_decompose_signed(E, R1, R2, t); }
int isvo_exr_choose(const int32_t *front, int n) { int f[4] = {front[0], front[1], front[2], front[3]}; return exr_choose(f, n); }
/* testTriangulation's front count of n correspondences [n][4] (as the estimator saw them) against [R | sign t] */
int isvo_exr_front_count(const double *R, const double *t, double sign, int n, const double *pts) {
    double P[12];
    int front = 0;
    exr_camera(R, t, sign, (g_quirk_off & 2) != 0, P);
    for (int j = 0; j < n; j++) front += exr_front(P, pts[4 * j], pts[4 * j + 1], pts[4 * j + 2], pts[4 * j + 3], (g_quirk_off & 2) != 0);
    return front;
}
/* X8 on A [rows][4] (overwritten): the serial QR, then the singular values and ric */
void isvo_exr_solve(int rows, double *A, double *singular, double *ric) {
    for (int k = 0; k < 4; k++) {
        double alpha, vv;
        if (!exr_qr_begin(rows, A, k, &alpha, &vv)) continue;
        for (int c = k + 1; c < 4; c++) exr_qr_apply(rows, A, k, c, alpha, vv);
        exr_qr_apply(rows, A, k, k, alpha, vv);
    }
    exr_solve_ric(A, singular, ric);
}

/* solveRelativeR (:68-98) from 9 correspondences on; pts [n][4] as the estimator sees them.  0: no model was kept. */
static int solve_relative_r(int count, const double *pts, isv_exr_result_t *res, double *Rc) {
    const int lmeds = count < ISV_EXR_RANSAC_MIN;                          /* X2 */
    const double tf = (double)(float)(EXR_F_THRESH * EXR_F_THRESH);
    uint64_t rng = ~0ull;
    double F[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, min_median = DBL_MAX, bound = tf;
    int niters = lmeds ? rej_lmeds_niters() : RP_MAX_ITERS, max_good = 0, kept = 0, iter;
    float e[REJ_MAX_MODEL_PTS];
    g_last.n_keeps = 0; g_last.keep_iter = -1;
    for (iter = 0; iter < niters; iter++) {
        int idx[7];
        double sub[28], Fm[27];
        rp_subset(&rng, count, idx);
        for (int k = 0; k < 7; k++) memcpy(sub + 4 * k, pts + 4 * idx[k], 4 * sizeof(double));
        const int nm = rp_run7point(sub, Fm);
        if (nm < 1 || nm > 3) continue;
        for (int m = 0; m < nm; m++) {
            int keep = 0;
            if (lmeds) {
                for (int j = 0; j < count; j++) e[j] = (float)rp_fm_error(Fm + 9 * m, pts[4 * j], pts[4 * j + 1], pts[4 * j + 2], pts[4 * j + 3]);
                const double median = rej_median(e, count);
                if (median < min_median) { min_median = median; keep = 1; }
            } else {
                int g = 0;
                for (int j = 0; j < count; j++) g += (double)(float)rp_fm_error(Fm + 9 * m, pts[4 * j], pts[4 * j + 1], pts[4 * j + 2], pts[4 * j + 3]) <= tf;
                if (g > (max_good > 6 ? max_good : 6)) {
                    max_good = g; keep = 1;
                    niters = rp_update_num_iters(RP_CONFIDENCE, (double)(count - g) / count, 7, niters);
                }
            }
            if (keep) {
                memcpy(F, Fm + 9 * m, sizeof(F));
                kept = 1;
                g_last.keep_iter = iter; g_last.n_keeps++;
                for (int k = 0; k < 7; k++) g_last.subset[k] = idx[k];
            }
        }
    }
    res->method = lmeds ? ISV_EXR_LMEDS : ISV_EXR_RANSAC;
    res->iters = lmeds ? niters : iter;
    if (!kept) return 0;
    if (lmeds) {
        const double sigma = rej_sigma(count, min_median);
        bound = (double)(float)(sigma * sigma);
        int g = 0;
        for (int j = 0; j < count; j++) g += (double)(float)rp_fm_error(F, pts[4 * j], pts[4 * j + 1], pts[4 * j + 2], pts[4 * j + 3]) <= bound;
        res->best_inliers = g;
    } else
        res->best_inliers = max_good;
    double R1[9], R2[9], t[3];
    exr_decompose(F, R1, R2, t);
    g_last.det_first = rp_det3(R1);
    res->negated = exr_decompose_signed(F, R1, R2, t);                     /* X3 */
    memcpy(g_last.F, F, sizeof(F)); memcpy(g_last.R1, R1, 72); memcpy(g_last.R2, R2, 72); memcpy(g_last.t, t, 24);
    for (int s = 0; s < 4; s++) res->front[s] = isvo_exr_front_count(s < 2 ? R1 : R2, t, (s & 1) ? -1.0 : 1.0, count, pts);   /* X4 */
    int front[4] = {res->front[0], res->front[1], res->front[2], res->front[3]};
    res->choice = exr_choose(front, count);
    const double *R = res->choice == 1 ? R1 : R2;
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) Rc[a * 3 + b] = R[b * 3 + a];
    return 1;
}

/* One isv_exr_calibrate_batch over a host-side slot store: frame_counts [max_slots], rics [max_slots][9],
 * hists [max_slots][max_frames][27].  named [max_slots] is scratch, zero on entry and on return. */
void isvo_exr_calibrate_batch(const isv_exr_config_t *cfg, int n, const isv_exr_item_t *const *items, isv_exr_result_t *results, int32_t *frame_counts,
                              double *rics, double *hists, uint8_t *named) {
    for (int i = 0; i < n; i++) {
        const isv_exr_item_t *it = items[i];
        isv_exr_result_t *res = results + i;
        const int s = exr_check_item(cfg, it, frame_counts, named);
        const int in_range = it->slot >= 0 && it->slot < cfg->max_slots;
        if (in_range) named[it->slot] = 1;
        if (s != ISV_EXR_OK) { exr_refuse(res, s, in_range ? frame_counts[it->slot] : -1); continue; }
        const int count = it->n_corres, F = frame_counts[it->slot] + 1;
        double *ric = rics + 9 * (size_t)it->slot, *hs = hists + (size_t)it->slot * cfg->max_frames * EXR_HIST;
        memset(res, 0, sizeof(*res));
        double Rc[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};                        /* X5 */
        if (count >= ISV_EXR_MIN_CORRES) {
            double *pts = (double *)malloc(sizeof(double) * 4 * (size_t)count);
            for (int k = 0; k < 4 * count; k++) pts[k] = (g_quirk_off & 1) ? it->corres[k] : (double)(float)it->corres[k];   /* X1 */
            const int ok = solve_relative_r(count, pts, res, Rc);
            free(pts);
            if (!ok) { exr_refuse(res, ISV_EXR_NO_MODEL, F - 1); continue; }
        }
        double *row = hs + (size_t)(F - 1) * EXR_HIST;
        memcpy(row, Rc, sizeof(Rc));
        exr_imu_rows(ric, it->delta_q, row + 9, row + 18);                 /* X6: the ric from before this call */
        double *A = (double *)malloc(sizeof(double) * 16 * (size_t)F);
        for (int f = 0; f < F; f++) {                                      /* X7 */
            double ang, hub;
            exr_row(hs + (size_t)f * EXR_HIST, hs + (size_t)f * EXR_HIST + 9, hs + (size_t)f * EXR_HIST + 18, &ang, &hub, A + 16 * (size_t)f);
            if (f == F - 1) { res->angle_deg = ang; res->huber = hub; }
        }
        free(g_last.A);
        g_last.A = (double *)malloc(sizeof(double) * 16 * (size_t)F);
        memcpy(g_last.A, A, sizeof(double) * 16 * (size_t)F);
        g_last.rows = 4 * F;
        isvo_exr_solve(4 * F, A, res->singular, ric);                      /* X8 */
        free(A);
        res->status = ISV_EXR_OK; res->frame_count = F;
        res->calibrated = exr_calibrated(F, cfg->vo_size, res->singular);
        memcpy(res->Rc, Rc, sizeof(Rc)); memcpy(res->ric, ric, 72);
        frame_counts[it->slot] = F;
    }
    for (int i = 0; i < n; i++)
        if (items[i]->slot >= 0 && items[i]->slot < cfg->max_slots) {
            named[items[i]->slot] = 0;
            if (results[i].status != ISV_EXR_OK) results[i].frame_count = frame_counts[items[i]->slot];   /* the slot's count after the call */
        }
}

void isvo_exr_free(void) { free(g_last.A); g_last.A = NULL; g_last.rows = 0; }
