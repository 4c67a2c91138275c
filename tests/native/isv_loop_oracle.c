/*
 * isv_loop_oracle.c -- CPU restatement of the loop-closure verification (include/isvins_loop.h), KeyFrame::findConnection of
 * src/pose_graph/keyframe.cpp:231-295: the brute-force BRIEF matching (:77-126, :298-303), PnPRANSAC (:155-228, OpenCV 3.2's
 * cv::solvePnPRansac as restated in the header), the relative pose, the gate and loop_weight.  Serial, one pair per call.
 *
 * Its numerical pieces (EPnP, the DLT, Rodrigues, the projection and the LM step, the Jacobi SVD / eigen-solver, the RNG, the
 * subset draw and the iteration update, the tail) are the kernel's own text -- is-vins_amd/csrc/isv_loop_common.h, isv_pnp.h,
 * isv_init_common.h -- compiled for the host; what is written here is what the kernel spreads over its lanes, with every
 * cross-lane sum in the order the kernel's lane 0 takes it.  So the GPU and this file perform the same operations in the same
 * order, and only libm can round apart.  Built with gcc -O2 -ffp-contract=off by tests/loop_oracle.py.
 *
 * isvo_loop_set_quirks_off(mask): bit k - 1 switches the reference quirk Lk off (L1, L3, L5, L6 have an effect), so that a
 * test can show each is there:
 *   L1  10..15 matches run PnPRANSAC instead of ending as ISV_LOOP_UNDEFINED_POSE
 *   L3  loop_weight's residual is the normalised reprojection residual of R_pnp p + T_pnp against uv, not divided by FOCAL_LENGTH
 *   L5  the RANSAC's reprojection error is formed and compared in doubles
 *   L6  an old corner is matched by one window point only: its closest claimant, the first of equals
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int g_quirks_off = 0;
#define LP_QUIRKS_OFF g_quirks_off
#include "../../is-vins_amd/csrc/isv_loop_common.h"

void isvo_loop_set_quirks_off(int mask) { g_quirks_off = mask; }

int isvo_loop_sizeof(int which) {
    return which == 0 ? (int)sizeof(isv_loop_config_t) : which == 1 ? (int)sizeof(isv_loop_pair_t) : which == 2 ? (int)sizeof(isv_loop_result_t)
                                                                                                                   : (int)sizeof(lp_match_t);
}

/* HammingDis (:298-303) */
static int hamming(const uint64_t *a, const uint64_t *b) {
    return __builtin_popcountll(a[0] ^ b[0]) + __builtin_popcountll(a[1] ^ b[1]) + __builtin_popcountll(a[2] ^ b[2]) + __builtin_popcountll(a[3] ^ b[3]);
}

/* searchByBRIEFDes / searchInAera (:77-126) and the first reduceVector (:249-254): match_index / match_dist [n_points] (may be
 * NULL), list [n_points]; returns the number of matches */
int isvo_loop_match(const isv_loop_config_t *cfg, const isv_loop_pair_t *p, int32_t *match_index, int32_t *match_dist, lp_match_t *list) {
    int32_t *mi = (int32_t *)malloc(sizeof(int32_t) * (p->n_points + 1)), *md = (int32_t *)malloc(sizeof(int32_t) * (p->n_points + 1));
    for (int i = 0; i < p->n_points; i++) {
        int bestDist = cfg->match_max_dist, bestIndex = -1;   /* L2 */
        for (int k = 0; k < p->n_keypoints; k++) {
            const int dis = hamming(p->window_brief + 4 * (size_t)i, p->brief + 4 * (size_t)k);
            if (dis < bestDist) { bestDist = dis; bestIndex = k; }
        }
        mi[i] = bestIndex; md[i] = bestDist;
    }
    int n = 0;
    for (int i = 0; i < p->n_points; i++) {
        int ok = mi[i] != -1 && md[i] < cfg->match_accept_dist;
        if (ok && LP_OFF(6))   /* L6 off: only the closest claimant of an old corner, the first of equals */
            for (int j = 0; j < p->n_points; j++)
                if (j != i && mi[j] == mi[i] && (md[j] < md[i] || (md[j] == md[i] && j < i))) ok = 0;
        if (!ok) continue;
        lp_match_t *m = list + n++;
        for (int c = 0; c < 3; c++) m->X[c] = p->point_3d[3 * (size_t)i + c];
        m->uv[0] = p->keypoints_norm[2 * (size_t)mi[i]]; m->uv[1] = p->keypoints_norm[2 * (size_t)mi[i] + 1];
        m->src = i;
    }
    if (match_index) memcpy(match_index, mi, sizeof(int32_t) * p->n_points);
    if (match_dist) memcpy(match_dist, md, sizeof(int32_t) * p->n_points);
    free(mi); free(md);
    return n;
}

/* ---- CvLevMarq over pts [n][LP_PT], serially: the sums of isv_pnp.h's pnp_eval in its lanes' order (points in order, row 0
 * then row 1) ---- */
static double o_pnp_eval(int n, const double *pts, double *pm, int wantJ) {
    double R[9], dRdr[27], e2 = 0, JtJ[36], JtE[6];
    rodrigues_v2m(pm + P_PAR, R, wantJ ? dRdr : NULL);
    for (int k = 0; k < 36; k++) JtJ[k] = 0;
    for (int k = 0; k < 6; k++) JtE[k] = 0;
    for (int i = 0; i < n; i++) {
        double e[2], J[12];
        const double *P = pts + (size_t)i * LP_PT;
        pnp_project(R, dRdr, pm + P_PAR + 3, P, P + 3, e, wantJ ? J : NULL);
        for (int r = 0; r < 2; r++) {
            e2 += e[r] * e[r];
            if (!wantJ) continue;
            for (int a = 0; a < 6; a++) {
                for (int b = 0; b <= a; b++) JtJ[a * 6 + b] += J[r * 6 + a] * J[r * 6 + b];
                JtE[a] += J[r * 6 + a] * e[r];
            }
        }
    }
    pm[P_E] = e2;
    if (wantJ) {
        for (int a = 0; a < 6; a++) for (int b = 0; b <= a; b++) pm[P_JTJ + a * 6 + b] = JtJ[a * 6 + b];
        for (int a = 0; a < 6; a++) pm[P_JTE + a] = JtE[a];
    }
    return sqrt(pm[P_E]);
}
static int o_pnp_solve(int n, const double *pts, double *pm) {
    int lambdaLg10 = -3, iters = 0;
    double prevErrNorm = 0, errNorm;
    for (;;) {
        const double e = o_pnp_eval(n, pts, pm, 1);
        for (int k = 0; k < 6; k++) pm[P_PREV + k] = pm[P_PAR + k];
        pnp_step(pm + P_JTJ, pm + P_JTE, lambdaLg10, pm + P_PREV, pm + P_PAR);
        if (iters == 0) prevErrNorm = e;
        for (;;) {
            errNorm = o_pnp_eval(n, pts, pm, 0);
            if (errNorm > prevErrNorm && ++lambdaLg10 <= 16) {
                pnp_step(pm + P_JTJ, pm + P_JTE, lambdaLg10, pm + P_PREV, pm + P_PAR);
                continue;
            }
            break;
        }
        lambdaLg10 = lambdaLg10 - 1 > -16 ? lambdaLg10 - 1 : -16;
        double dn = 0, pn = 0;
        for (int k = 0; k < 6; k++) { double d = pm[P_PAR + k] - pm[P_PREV + k]; dn += d * d; pn += pm[P_PREV + k] * pm[P_PREV + k]; }
        if (++iters >= 20 || sqrt(dn) / (sqrt(pn) + DBL_EPSILON) < FLT_EPSILON) break;
        prevErrNorm = errNorm;
    }
    return iters;
}

/* solvePnP(SOLVEPNP_ITERATIVE, no guess) on pts [n][LP_PT]: 1 = planar (refused), else rvec / tvec and the LM's iterations */
int isvo_lp_iterative(int n, const double *pts, double *rvec, double *tvec, int *iters) {
    double LA[144], LV[144], pm[P_END];
    if (lp_dlt_planar(n, pts)) return 1;
    for (int a = 0; a < 12; a++) for (int b = 0; b <= a; b++) LA[12 * a + b] = lp_dlt_entry(n, pts, a, b);
    lp_dlt_pose(LA, LV, pm + P_PAR, pm + P_PAR + 3);
    *iters = o_pnp_solve(n, pts, pm);
    for (int k = 0; k < 3; k++) { rvec[k] = pm[P_PAR + k]; tvec[k] = pm[P_PAR + 3 + k]; }
    return 0;
}

/* ---- unit entries ---- */
void isvo_lp_epnp(int n, const double *X, const double *uv, double *R, double *t) {
    double work[288];
    lp_epnp(n, X, uv, R, t, work);
}
/* debug entry for the 40-digit EPnP stage test (tests/loop_highprec.py): lp_epnp's result and the basis it used.  vv [4][12]: the
 * eigenvectors of the four smallest eigenvalues, smallest first, read back from lp_epnp's work array (it leaves them at work + 144).
 * cws [4][3]: the control points, by choose_control_points' statements on the same input (the same routine on the same numbers, so
 * the same axes and signs).  The shared header is not touched: the kernel's code object cannot change. */
void isvo_lp_epnp_basis(int n, const double *X, const double *uv, double *R, double *t, double *cws, double *vv) {
    double work[288], CC[9], w3[3], V3[9];
    lp_epnp(n, X, uv, R, t, work);
    for (int i = 0; i < 4; i++) for (int k = 0; k < 12; k++) vv[12 * i + k] = work[144 + 12 * k + (11 - i)];
    for (int k = 0; k < 3; k++) cws[k] = 0.0;
    for (int i = 0; i < n; i++) for (int k = 0; k < 3; k++) cws[k] += X[3 * i + k];
    for (int k = 0; k < 3; k++) cws[k] /= n;
    for (int k = 0; k < 9; k++) CC[k] = 0.0;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 3; j++)
            for (int k = 0; k < 3; k++) CC[3 * j + k] += (X[3 * i + j] - cws[j]) * (X[3 * i + k] - cws[k]);
    svd_jacobi(3, CC, w3, 0, V3);
    for (int i = 1; i < 4; i++) {
        const double s = sqrt(w3[i - 1] / n);
        for (int j = 0; j < 3; j++) cws[3 * i + j] = cws[j] + s * V3[3 * j + (i - 1)];
    }
}
void isvo_eig_jacobi_sym(int n, double *A, double *w, double *V) { eig_jacobi_sym(n, A, w, V); }
void isvo_rodrigues_v2m(const double *rv, double *R) { rodrigues_v2m(rv, R, NULL); }
void isvo_rodrigues_v2m_J(const double *rv, double *R, double *J) { rodrigues_v2m(rv, R, J); }   /* J: 3 x 9, d R / d r_i */
void isvo_rodrigues_m2v(const double *R, double *rv) { rodrigues_m2v(R, rv); }
/* cvProjectPoints2 of one point from rvec / tvec: err [2] and J [2 x 6] */
void isvo_pnp_project(const double *rvec, const double *tvec, const double *X, const double *m, double *err, double *J) {
    double R[9], dRdr[27];
    rodrigues_v2m(rvec, R, dRdr);
    pnp_project(R, dRdr, tvec, X, m, err, J);
}
/* CvLevMarq::step: JtJ 6 x 6 (its lower triangle is read), JtE [6] */
void isvo_pnp_step(const double *JtJ, const double *JtE, int lambdaLg10, const double *prev, double *param) { pnp_step(JtJ, JtE, lambdaLg10, prev, param); }
double isvo_lp_point_error(const double *rvec, const double *tvec, const float *X, const float *uv) {
    double R[9];
    lp_match_t m;
    for (int k = 0; k < 3; k++) m.X[k] = X[k];
    m.uv[0] = uv[0]; m.uv[1] = uv[1]; m.src = 0;
    rodrigues_v2m(rvec, R, NULL);
    return lp_point_error(R, tvec, &m);
}

static int finite_f(const float *v, size_t n) {
    for (size_t k = 0; k < n; k++) if (!(v[k] - v[k] == 0.0f)) return 0;
    return 1;
}
static int check_pair(const isv_loop_config_t *c, const isv_loop_pair_t *p) {
    if (p->n_points < 0 || p->n_keypoints < 0) return ISV_LOOP_INPUT;
    if (p->n_points > 0 && (!p->window_brief || !p->point_3d)) return ISV_LOOP_INPUT;
    if (p->n_keypoints > 0 && (!p->brief || !p->keypoints_norm)) return ISV_LOOP_INPUT;
    if (p->n_points > c->max_points || p->n_keypoints > c->max_keypoints) return ISV_LOOP_CAPACITY;
    if (!finite_f(p->point_3d, 3 * (size_t)p->n_points) || !finite_f(p->keypoints_norm, 2 * (size_t)p->n_keypoints) ||
        !lp_finite(p->origin_vio_T, 3) || !lp_finite(p->origin_vio_R, 9)) return ISV_LOOP_INPUT;
    return ISV_LOOP_OK;
}

/* findConnection of one pair; match_index / match_dist / inlier [n_points] (each may be NULL).  Returns the status. */
int isvo_loop_verify(const isv_loop_config_t *cfg, const isv_loop_pair_t *p, isv_loop_result_t *res, int32_t *match_index, int32_t *match_dist,
                     int32_t *inlier) {
    memset(res, 0, sizeof(*res));
    res->ransac_iters = -1; res->pnp_iterations = -1; res->loop_index = -1;
    const int st = check_pair(cfg, p);
    if (st != ISV_LOOP_OK) return res->status = st;
    const int np = p->n_points;
    lp_match_t *pts = (lp_match_t *)malloc(sizeof(lp_match_t) * (np + 1));
    int32_t *inl = (int32_t *)malloc(sizeof(int32_t) * (np + 1));
    double *pp = (double *)malloc(sizeof(double) * LP_PT * (np + 1)), *term = (double *)malloc(sizeof(double) * (np + 1));
    const int n = isvo_loop_match(cfg, p, match_index, match_dist, pts);
    res->n_matched = n; res->n_final = n;
    for (int i = 0; i < np; i++) inl[i] = -1;
    int status = lp_match_gate(cfg, n);   /* L1 */
    if (status != ISV_LOOP_OK) goto done;
    {
        const double td = cfg->ransac_threshold * cfg->ransac_threshold;
        const float tf = (float)td;
        /* RANSACPointSetRegistrator::run */
        uint64_t rng = ~0ull;
        int iter = 0, niters = cfg->ransac_iterations, max_good = 0;
        double best[6], work[288];
        for (; iter < niters; iter++) {
            int idx[5];
            double model[6];
            rp_subset_m(&rng, n, 5, idx);
            const int g = lp_ransac_model(pts, idx, model, work) ? lp_count_inliers(model, n, pts, tf, td) : 0;   /* L4: no guess */
            if (g > (max_good > 4 ? max_good : 4)) {
                for (int k = 0; k < 6; k++) best[k] = model[k];
                max_good = g;
                niters = rp_update_num_iters(cfg->ransac_confidence, (double)(n - g) / n, 5, niters);
            }
        }
        res->ransac_iters = iter; res->ransac_inliers = max_good;
        if (max_good <= 0) {
            for (int j = 0; j < n; j++) inl[pts[j].src] = 0;
            res->n_final = 0;
            status = ISV_LOOP_PNP_FAILED;
            goto done;
        }
        double Rb[9];
        int cnt_in = 0;
        rodrigues_v2m(best, Rb, NULL);
        for (int j = 0; j < n; j++) {
            const int q = lp_is_inlier(Rb, best + 3, pts + j, tf, td);
            inl[pts[j].src] = q;
            if (!q) continue;
            double *P = pp + LP_PT * (size_t)cnt_in++;
            P[0] = pts[j].X[0]; P[1] = pts[j].X[1]; P[2] = pts[j].X[2]; P[3] = pts[j].uv[0]; P[4] = pts[j].uv[1];
        }
        res->n_final = cnt_in;
        if (!((double)cnt_in > 0.6 * cfg->min_loop_num)) { status = ISV_LOOP_PNP_FAILED; goto done; }
        double rvec[3], tvec[3], LR[9], LT[3];
        int iters = 0;
        if (isvo_lp_iterative(cnt_in, pp, rvec, tvec, &iters)) { status = ISV_LOOP_PLANAR; goto done; }
        res->pnp_iterations = iters;
        lp_old_pose(rvec, tvec, LR, LT);
        for (int j = 0; j < n; j++)
            if (inl[pts[j].src] == 1) term[j] = lp_weight_term(LR, LT, tvec, pts + j, cfg->focal_length);   /* L3 */
        double sum = 0;
        int m = 0;
        for (int j = 0; j < n; j++)
            if (inl[pts[j].src] == 1) { m++; sum += term[j]; }
        lp_finish(cfg, LR, LT, p->origin_vio_T, p->origin_vio_R, sum, m, p->old_index, res);
        status = res->status;
    }
done:
    res->status = status;
    if (inlier) memcpy(inlier, inl, sizeof(int32_t) * np);
    free(pts); free(inl); free(pp); free(term);
    return status;
}
