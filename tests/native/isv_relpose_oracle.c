/*
 * isv_relpose_oracle.c -- CPU restatement of the relative-pose stage of the initialisation (is-vins_amd/csrc/isv_relpose.h:
 * IMU excitation, relativePose's candidates, findFundamentalMat's RANSAC, the reference's recoverPose), the checker of
 * k_relpose.  TEST INFRASTRUCTURE ONLY: built by the tests into a temporary directory with
 *   gcc -O2 -ffp-contract=off -shared -fPIC
 * and never linked into the library.  The RANSAC is the plain serial loop of RANSACPointSetRegistrator::run (one subset, its
 * models, their inlier counts, the keep rule, the niters update, in that order), recoverPose a plain loop over the
 * correspondences.  The serial pieces (OpenCV's RNG, getSubset, run7Point, solveCubic, computeError, RANSACUpdateNumIters,
 * decomposeEssentialMat, the cheirality test) are the kernel's own text, is-vins_amd/csrc/isv_init_common.h, compiled for the
 * host; so the two differ only where libm and the device math library round acos / cos / pow / log apart.  Quirks R1..R5 are
 * described in isv_relpose.h and marked where they happen.
 *
 * Restated (the reference cannot be built without Eigen and OpenCV): src/estimator.cpp:213-238 and 431-456,
 * src/initial/solve_5pts.cpp, src/feature_tracker/feature_manager.cpp:124-143.
 */
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "../../is-vins_amd/csrc/isv_relpose.h"
#include "../../is-vins_amd/csrc/isv_init_common.h"

#define NT ISV_SFM_MAX_TRACKS

/* test hook: a set bit replaces a reproduced quirk by the "obvious" behaviour, so that the tests can show each quirk matters.
 * 1: R1, RANSAC and recoverPose see the double points; 2: R2, the RANSAC error stays double against thresh^2 in double;
 * 4: R4, one RNG per problem, continued from candidate to candidate; 8: R5, i = n_window - 2 is tried too.  (R3 changes no
 * result: decomposeEssentialMat reads only the singular vectors.) */
static int g_quirk_off = 0;
void isvo_relpose_set_quirks_off(int mask) { g_quirk_off = mask; }
#define FR(x) ((g_quirk_off & 1) ? (x) : (double)(float)(x))

static int is_inlier(const double *F, const double *q) {
    const double e = rp_fm_error(F, q[0], q[1], q[2], q[3]);
    if (g_quirk_off & 2) return e <= RP_THRESH * RP_THRESH;
    return (float)e <= (float)(RP_THRESH * RP_THRESH);   /* R2 */
}

/* the host-side refusals of isv_sfm.h, l aside */
static int check(const isv_sfm_problem_t *p) {
    if (p->n_window > ISV_ALIGN_MAX_WINDOW || p->n_frames > ISV_ALIGN_MAX_FRAMES || p->n_tracks > ISV_SFM_MAX_TRACKS || p->n_obs > ISV_SFM_MAX_OBS)
        return ISV_RELPOSE_REFUSED_CAPACITY;
    if (p->n_window < 2 || p->n_frames < 2 || p->n_tracks < 0 || p->n_obs < 0 || p->n_pts < 0) return ISV_RELPOSE_REFUSED_INPUT;
    if ((p->n_tracks && (!p->tracks || !p->obs)) || !p->pt_off || (p->n_pts && (!p->pt_id || !p->pt_uv)) || !p->delta_v || !p->sum_dt)
        return ISV_RELPOSE_REFUSED_INPUT;
    if (p->n_tracks && (!p->position || !p->state)) return ISV_RELPOSE_REFUSED_INPUT;
    for (int i = 0; i < p->n_window; i++) {
        int w = p->window_frame[i];
        if (w < 0 || w >= p->n_frames || (i > 0 && w <= p->window_frame[i - 1])) return ISV_RELPOSE_REFUSED_INPUT;
    }
    if (p->window_frame[p->n_window - 1] != p->n_frames - 1) return ISV_RELPOSE_REFUSED_INPUT;
    for (int j = 0; j < p->n_tracks; j++) {
        const isv_sfm_track_t *T = &p->tracks[j];
        if (T->n_obs < 1 || T->start_frame < 0 || T->start_frame + T->n_obs > p->n_window || T->obs_off < 0 || T->obs_off + T->n_obs > p->n_obs)
            return ISV_RELPOSE_REFUSED_INPUT;
    }
    if (p->pt_off[0] != 0 || p->pt_off[p->n_frames] != p->n_pts) return ISV_RELPOSE_REFUSED_INPUT;
    for (int f = 0; f < p->n_frames; f++) {
        if (p->pt_off[f + 1] < p->pt_off[f]) return ISV_RELPOSE_REFUSED_INPUT;
        for (int k = p->pt_off[f] + 1; k < p->pt_off[f + 1]; k++)
            if (p->pt_id[k] <= p->pt_id[k - 1]) return ISV_RELPOSE_REFUSED_INPUT;
    }
    return ISV_RELPOSE_OK;
}

/* findFundamentalMat(FM_RANSAC): returns maxGoodCount (0: no model; F untouched), the iterations in *iters */
static int ransac(const double *pts, int count, uint64_t *rng, double *F, int *iters) {
    int niters = RP_MAX_ITERS, max_good = 0, iter;
    for (iter = 0; iter < niters; iter++) {
        int idx[7];
        double sub[28], Fm[27];
        rp_subset(rng, count, idx);
        for (int k = 0; k < 7; k++) memcpy(sub + 4 * k, pts + 4 * idx[k], 4 * sizeof(double));
        const int nm = rp_run7point(sub, Fm);
        if (nm < 1 || nm > 3) continue;
        for (int m = 0; m < nm; m++) {
            int g = 0;
            for (int j = 0; j < count; j++) g += is_inlier(Fm + 9 * m, pts + 4 * j);
            if (g > (max_good > 6 ? max_good : 6)) {
                memcpy(F, Fm + 9 * m, 9 * sizeof(double));
                max_good = g;
                niters = rp_update_num_iters(RP_CONFIDENCE, (double)(count - g) / count, 7, niters);
            }
        }
    }
    *iters = iter;
    return max_good;
}

int isvo_relpose(const isv_sfm_problem_t *p, isv_relpose_result_t *res, int32_t *mask) {
    memset(res, 0, sizeof(*res));
    res->l = -1;
    for (int i = 0; i < ISV_ALIGN_MAX_WINDOW; i++) {
        res->n_corres[i] = res->ransac_iters[i] = res->ransac_inliers[i] = res->recover_inliers[i] = res->solution[i] = -1;
        res->parallax[i] = -1.0;
    }
    res->status = check(p);
    if (res->status != ISV_RELPOSE_OK) return res->status;
    if (mask) for (int j = 0; j < p->n_tracks; j++) mask[j] = -1;
    /* ---- stage 0: checkIMUExcitation ---- */
    res->excitation_var = isv_excitation_var(p->n_frames, p->delta_v, p->sum_dt);
    if (res->excitation_var < 0.25) return res->status = ISV_RELPOSE_REFUSED_EXCITATION;
    /* ---- stage 1: relativePose ---- */
    static double pts[4 * NT];
    static int trk[NT], cm[NT];
    const int nw = p->n_window, last = nw - 1;
    const int n_cand = (g_quirk_off & 8) ? nw - 1 : nw - 2;   /* R5 */
    uint64_t rng_problem = ~0ull;
    for (int i = 0; i < n_cand; i++) {
        int count = 0;
        double sum = 0;
        for (int j = 0; j < p->n_tracks; j++) {   /* getCorresponding(i, last) */
            const isv_sfm_track_t *T = &p->tracks[j];
            if (!(T->start_frame <= i && T->start_frame + T->n_obs - 1 >= last)) continue;
            const double *a = p->obs + 2 * (T->obs_off + i - T->start_frame), *b = p->obs + 2 * (T->obs_off + last - T->start_frame);
            pts[4 * count] = FR(a[0]); pts[4 * count + 1] = FR(a[1]); pts[4 * count + 2] = FR(b[0]); pts[4 * count + 3] = FR(b[1]);   /* R1 */
            trk[count++] = j;
        }
        res->n_candidates = i + 1;
        res->n_corres[i] = count;
        if (count <= 20) continue;
        for (int k = 0; k < count; k++) {   /* the parallax of the doubles, in correspondence order */
            const isv_sfm_track_t *T = &p->tracks[trk[k]];
            const double *a = p->obs + 2 * (T->obs_off + i - T->start_frame), *b = p->obs + 2 * (T->obs_off + last - T->start_frame);
            const double dx = a[0] - b[0], dy = a[1] - b[1];
            sum = sum + sqrt(dx * dx + dy * dy);
        }
        const double avg = 1.0 * sum / count;
        res->parallax[i] = avg;
        if (!(avg * 460 > 30)) continue;
        /* ---- solveRelativeRT ---- */
        uint64_t rng_fresh = ~0ull;   /* R4: RNG((uint64)-1) in every call */
        uint64_t *rng = (g_quirk_off & 4) ? &rng_problem : &rng_fresh;
        double F[9], P[48];
        int iters;
        const int max_good = ransac(pts, count, rng, F, &iters);
        res->ransac_iters[i] = iters;
        res->ransac_inliers[i] = max_good;
        if (max_good == 0) continue;   /* (the reference aborts in decomposeEssentialMat) */
        rp_decompose(F, P);            /* R3: F of normalised points, as it is */
        int good[4] = {0, 0, 0, 0};
        for (int j = 0; j < count; j++) {
            const double *q = pts + 4 * j;
            int bits = 0;
            if (is_inlier(F, q)) {
                bits = 1;
                for (int s = 0; s < 4; s++) bits |= rp_cheirality(P + 12 * s, q[0], q[1], q[2], q[3]) << (1 + s);
            }
            cm[j] = bits;
            for (int s = 0; s < 4; s++) good[s] += (bits >> (1 + s)) & 1;
        }
        const int g1 = good[0], g2 = good[1], g3 = good[2], g4 = good[3];
        const int s = (g1 >= g2 && g1 >= g3 && g1 >= g4) ? 0 : (g2 >= g1 && g2 >= g3 && g2 >= g4) ? 1 : (g3 >= g1 && g3 >= g2 && g3 >= g4) ? 2 : 3;
        res->recover_inliers[i] = good[s];
        res->solution[i] = s + 1;
        if (good[s] > 12) {
            const double *Pc = P + 12 * s;
            for (int a = 0; a < 3; a++)
                for (int c = 0; c < 3; c++) res->relative_R[a * 3 + c] = Pc[c * 4 + a];   /* Rotation = R^T */
            for (int a = 0; a < 3; a++) res->relative_T[a] = (-Pc[a]) * Pc[3] + (-Pc[4 + a]) * Pc[7] + (-Pc[8 + a]) * Pc[11];
            res->l = i;
            if (mask) for (int j = 0; j < count; j++) mask[trk[j]] = (cm[j] & 1) && ((cm[j] >> (1 + s)) & 1);
            return res->status = ISV_RELPOSE_OK;
        }
    }
    return res->status = ISV_RELPOSE_NO_RELATIVE_POSE;
}

/* the serial pieces, for the unit tests */
int isvo_rp_solve_cubic(const double *c, double *r) { return rp_solve_cubic(c, r); }
int isvo_rp_run7point(const double *p, double *F) { return rp_run7point(p, F); }
int isvo_rp_update_num_iters(double p, double ep, int model_points, int max_iters) { return rp_update_num_iters(p, ep, model_points, max_iters); }
int isvo_rp_is_inlier(const double *F, const double *q) { return is_inlier(F, q); }

int isvo_relpose_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(isv_sfm_problem_t);
    case 1: return (int)sizeof(isv_relpose_result_t);
    default: return -1;
    }
}
