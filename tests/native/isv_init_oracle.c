/*
 * isv_init_oracle.c -- CPU restatement of the visual-inertial alignment (is-vins_amd/csrc/isv_initial.h), the checker of
 * k_visual_imu_align.  TEST INFRASTRUCTURE ONLY: built by the tests into a temporary directory with
 *   gcc -O2 -ffp-contract=off -shared -fPIC
 * and never linked into the library.  Operation order follows the kernel (serial dot products in index order, blocks
 * added pair by pair), so the two differ only where libm and the device math library round sin / cos / atan2 apart.
 *
 * Restated (the reference cannot be built without Eigen): src/initial/initial_aligment.cpp:3-208,
 * src/estimator.cpp:357-429, include/factor/integration_base.h:38-158, src/utility/utility.cpp:3-13.
 */
#include <float.h>
#include <math.h>
#include <string.h>
#include "../../oracle/isvo_math.h"
#include "../../is-vins_amd/csrc/isv_initial.h"

#define MAXN (3 * ISV_ALIGN_MAX_FRAMES + 4)

/* Eigen 3.3 LDLT<MatrixXd, Lower>: ldlt_inplace<Lower>::unblocked + LDLT::_solve_impl.  A is n x n row-major, only its lower
 * triangle is read; b is overwritten with the solution. */
static void ldlt_solve(double *A, int n, double *b) {
    int tr[MAXN];
    double temp[MAXN];
    for (int k = 0; k < n; k++) {
        /* largest |diagonal| of the trailing block, first on ties (maxCoeff): the diagonal there is not yet updated */
        int p = k;
        double best = fabs(A[k * n + k]);
        for (int i = k + 1; i < n; i++)
            if (fabs(A[i * n + i]) > best) { best = fabs(A[i * n + i]); p = i; }
        tr[k] = p;
        if (p != k) {
            for (int j = 0; j < k; j++) { double t = A[k * n + j]; A[k * n + j] = A[p * n + j]; A[p * n + j] = t; }
            for (int i = p + 1; i < n; i++) { double t = A[i * n + k]; A[i * n + k] = A[i * n + p]; A[i * n + p] = t; }
            { double t = A[k * n + k]; A[k * n + k] = A[p * n + p]; A[p * n + p] = t; }
            for (int i = k + 1; i < p; i++) { double t = A[i * n + k]; A[i * n + k] = A[p * n + i]; A[p * n + i] = t; }
        }
        for (int j = 0; j < k; j++) temp[j] = A[j * n + j] * A[k * n + j];
        double dot = 0;
        for (int j = 0; j < k; j++) dot += A[k * n + j] * temp[j];
        A[k * n + k] -= dot;
        for (int i = k + 1; i < n; i++) {
            double s = 0;
            for (int j = 0; j < k; j++) s += A[i * n + j] * temp[j];
            A[i * n + k] -= s;
        }
        double akk = A[k * n + k];
        if (fabs(akk) > 0.0)
            for (int i = k + 1; i < n; i++) A[i * n + k] /= akk;
    }
    for (int k = 0; k < n; k++) { double t = b[k]; b[k] = b[tr[k]]; b[tr[k]] = t; }
    for (int i = 0; i < n; i++) { double s = 0; for (int j = 0; j < i; j++) s += A[i * n + j] * b[j]; b[i] -= s; }
    for (int i = 0; i < n; i++) b[i] = fabs(A[i * n + i]) > DBL_MIN ? b[i] / A[i * n + i] : 0.0;
    for (int i = n - 1; i >= 0; i--) { double s = 0; for (int j = i + 1; j < n; j++) s += A[j * n + i] * b[j]; b[i] -= s; }
    for (int k = n - 1; k >= 0; k--) { double t = b[k]; b[k] = b[tr[k]]; b[tr[k]] = t; }
}

static double norm3(const double *v) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
/* Eigen normalized(): v / sqrt(squaredNorm) when the norm is positive */
static void normalized3(const double *v, double *o) {
    double z = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    if (z > 0) { double n = sqrt(z); o[0] = v[0] / n; o[1] = v[1] / n; o[2] = v[2] / n; }
    else { o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; }
}

/* IntegrationBase::repropagate(0, bg) (integration_base.h:38-52) through propagate / midPointIntegration (:54-158), the deltas
 * and sum_dt only */
static void repropagate(const isv_align_frame_t *f, const double *imu, const double *bg, double *dp, double *dq4, double *dv,
                        double *sum_dt) {
    double acc_0[3], gyr_0[3];
    memcpy(acc_0, f->linearized_acc, sizeof(acc_0));
    memcpy(gyr_0, f->linearized_gyr, sizeof(gyr_0));
    quat_t dq = {1, 0, 0, 0};
    double p[3] = {0, 0, 0}, v[3] = {0, 0, 0}, sdt = 0.0;
    for (int s = 0; s < f->imu_count; s++) {
        const double *row = imu + 7 * (size_t)(f->imu_begin + s);
        double dt = row[0];
        const double *acc_1 = row + 1, *gyr_1 = row + 4;
        double a0[3], a1[3], ung[3], u0[3], u1[3];
        for (int k = 0; k < 3; k++) { a0[k] = acc_0[k] - 0.0; a1[k] = acc_1[k] - 0.0; ung[k] = 0.5 * (gyr_0[k] + gyr_1[k]) - bg[k]; }
        q_rot(dq, a0, u0);
        quat_t inc = {1, ung[0] * dt / 2, ung[1] * dt / 2, ung[2] * dt / 2};
        quat_t rdq = q_mul(dq, inc);
        q_rot(rdq, a1, u1);
        for (int k = 0; k < 3; k++) {
            double un = 0.5 * (u0[k] + u1[k]);
            double rp = p[k] + v[k] * dt + 0.5 * un * dt * dt;
            double rv = v[k] + un * dt;
            p[k] = rp; v[k] = rv;
        }
        dq = q_normalized(rdq);
        sdt += dt;
        for (int k = 0; k < 3; k++) { acc_0[k] = acc_1[k]; gyr_0[k] = gyr_1[k]; }
    }
    memcpy(dp, p, sizeof(p)); memcpy(dv, v, sizeof(v));
    dq4[0] = dq.x; dq4[1] = dq.y; dq4[2] = dq.z; dq4[3] = dq.w;
    *sum_dt = sdt;
}

/* the 6 x m block (rows 0..5) of one frame pair and its right-hand side; returns r_A = tA^T tA (m x m) and r_b = tA^T tb */
static void pair_normal(const double *tA, const double *tb, int m, double *rA, double *rb) {
    for (int i = 0; i < m; i++) {
        for (int j = 0; j < m; j++) { double s = 0; for (int r = 0; r < 6; r++) s += tA[r * m + i] * tA[r * m + j]; rA[i * m + j] = s; }
        double s = 0; for (int r = 0; r < 6; r++) s += tA[r * m + i] * tb[r]; rb[i] = s;
    }
}

/* LinearAlignment (g = 3 free, m = 10) or one RefineGravity pass (g = 2 on the tangent basis, m = 9): tmp_A / tmp_b of pair i */
static void pair_rows(const isv_align_frame_t *fi, const isv_align_frame_t *fj, const double *dp, const double *dv, double dt,
                      const double *tic, const double *lxly /* NULL: LinearAlignment */, const double *g0, double *tA, double *tb) {
    int m = lxly ? 9 : 10;
    double RiT[9], RiTRj[9], M2[9], M1[9], dT[3], t3[3], t4[3];
    m3_t(fi->R, RiT);
    mm(RiT, fj->R, RiTRj, 3, 3, 3);
    for (int k = 0; k < 9; k++) { M2[k] = RiT[k] * dt * dt / 2; M1[k] = RiT[k] * dt; }
    for (int k = 0; k < 3; k++) dT[k] = fj->T[k] - fi->T[k];
    m3v(RiT, dT, t3);
    m3v(RiTRj, tic, t4);
    memset(tA, 0, sizeof(double) * 6 * m);
    for (int a = 0; a < 3; a++) {
        tA[a * m + a] = -dt;
        tA[(3 + a) * m + a] = -1.0;
        for (int b = 0; b < 3; b++) tA[(3 + a) * m + 3 + b] = RiTRj[a * 3 + b];
        if (!lxly) {
            for (int b = 0; b < 3; b++) { tA[a * m + 6 + b] = M2[a * 3 + b]; tA[(3 + a) * m + 6 + b] = M1[a * 3 + b]; }
            tA[a * m + 9] = t3[a] / 100.0;
            tb[a] = dp[a] + t4[a] - tic[a];
            tb[3 + a] = dv[a];
        } else {
            for (int b = 0; b < 2; b++) {
                double s2 = 0, s1 = 0;
                for (int k = 0; k < 3; k++) { s2 += M2[a * 3 + k] * lxly[k * 2 + b]; s1 += M1[a * 3 + k] * lxly[k * 2 + b]; }
                tA[a * m + 6 + b] = s2; tA[(3 + a) * m + 6 + b] = s1;
            }
            tA[a * m + 8] = t3[a] / 100.0;
            double g2 = 0, g1 = 0;
            for (int k = 0; k < 3; k++) { g2 += M2[a * 3 + k] * g0[k]; g1 += M1[a * 3 + k] * g0[k]; }
            tb[a] = dp[a] + t4[a] - tic[a] - g2;
            tb[3 + a] = dv[a] - g1;
        }
    }
}

/* A.block<6,6>(3i,3i), the trailing (m-6) square, and the two off-diagonal strips += the pair's r_A (same for b) */
static void pair_add(double *A, double *b, int n, int i, int m, const double *rA, const double *rb) {
    int t = m - 6;
    for (int r = 0; r < 6; r++) {
        for (int c = 0; c < 6; c++) A[(3 * i + r) * n + 3 * i + c] += rA[r * m + c];
        b[3 * i + r] += rb[r];
    }
    for (int r = 0; r < t; r++) {
        for (int c = 0; c < t; c++) A[(n - t + r) * n + n - t + c] += rA[(6 + r) * m + 6 + c];
        b[n - t + r] += rb[6 + r];
    }
    for (int r = 0; r < 6; r++) for (int c = 0; c < t; c++) A[(3 * i + r) * n + n - t + c] += rA[r * m + 6 + c];
    for (int r = 0; r < t; r++) for (int c = 0; c < 6; c++) A[(n - t + r) * n + 3 * i + c] += rA[(6 + r) * m + c];
}

/* TangentBasis  initial_aligment.cpp:40-53 ; lxly is 3 x 2 row-major */
static void tangent_basis(const double *g0, double *lxly) {
    double a[3], tmp[3] = {0, 0, 1}, b[3], c[3], t[3];
    normalized3(g0, a);
    if (a[0] == tmp[0] && a[1] == tmp[1] && a[2] == tmp[2]) { tmp[0] = 1; tmp[2] = 0; }
    double d = a[0] * tmp[0] + a[1] * tmp[1] + a[2] * tmp[2];
    for (int k = 0; k < 3; k++) t[k] = tmp[k] - a[k] * d;
    normalized3(t, b);
    cross3(a, b, c);
    for (int k = 0; k < 3; k++) { lxly[k * 2] = b[k]; lxly[k * 2 + 1] = c[k]; }
}

static int check_input(const isv_align_problem_t *p) {
    if (p->n_frames > ISV_ALIGN_MAX_FRAMES || p->n_window > ISV_ALIGN_MAX_WINDOW) return ISV_ALIGN_REFUSED_CAPACITY;
    if (p->n_frames < 2 || p->n_window < 1) return ISV_ALIGN_REFUSED_INPUT;
    int kf = 0;
    for (int i = 0; i < p->n_window; i++) {
        int w = p->window_frame[i];
        if (w < 0 || w >= p->n_frames || (i > 0 && w <= p->window_frame[i - 1])) return ISV_ALIGN_REFUSED_INPUT;
    }
    for (int f = 0, wi = 0; f < p->n_frames; f++) {
        int in_window = wi < p->n_window && p->window_frame[wi] == f;
        if (in_window) wi++;
        if (in_window || p->frames[f].is_key_frame) kf++;
        if (f > 0) {
            const isv_align_frame_t *fr = &p->frames[f];
            if (fr->imu_begin < 0 || fr->imu_count < 0 || (int64_t)fr->imu_begin + fr->imu_count > p->n_imu) return ISV_ALIGN_REFUSED_INPUT;
        }
    }
    return kf == p->n_window ? ISV_ALIGN_OK : ISV_ALIGN_REFUSED_INPUT;
}

int isvo_visual_imu_align(const isv_align_problem_t *p, isv_align_result_t *r) {
    static double A[MAXN * MAXN];
    double b[MAXN];
    memset(r, 0, sizeof(*r));
    r->status = check_input(p);
    if (r->status != ISV_ALIGN_OK) return r->status;
    const int nf = p->n_frames, nw = p->n_window;
    const isv_align_frame_t *F = p->frames;
    const double Gn = norm3(p->G);

    /* ---- solveGyroscopeBias (initial_aligment.cpp:3-37) ---- */
    double A3[9] = {0}, b3[3] = {0};
    for (int i = 0; i + 1 < nf; i++) {
        const isv_align_frame_t *fi = &F[i], *fj = &F[i + 1];
        double RiT[9], Rij[9];
        m3_t(fi->R, RiT);
        mm(RiT, fj->R, Rij, 3, 3, 3);
        quat_t qij = q_from_R(Rij);
        quat_t dq = {fj->delta_q[3], fj->delta_q[0], fj->delta_q[1], fj->delta_q[2]};
        quat_t e = q_mul(q_inv(qij), dq);
        double tb[3] = {-2.0 * e.x, -2.0 * e.y, -2.0 * e.z};
        const double *tA = fj->jac_rr;           /* quirk Q1: jacobian.block<3,3>(3,3) */
        for (int a = 0; a < 3; a++) {
            for (int c = 0; c < 3; c++) { double s = 0; for (int k = 0; k < 3; k++) s += tA[k * 3 + a] * tA[k * 3 + c]; A3[a * 3 + c] += s; }
            double s = 0; for (int k = 0; k < 3; k++) s += tA[k * 3 + a] * tb[k]; b3[a] += s;
        }
    }
    ldlt_solve(A3, 3, b3);
    memcpy(r->delta_bg, b3, sizeof(b3));
    for (int i = 0; i < nw; i++) for (int k = 0; k < 3; k++) r->Bgs[i][k] = p->Bgs[i][k] + b3[k];
    for (int j = 1; j < nf; j++)
        repropagate(&F[j], p->imu, r->Bgs[0], r->rp_delta_p[j], r->rp_delta_q[j], r->rp_delta_v[j], &r->rp_sum_dt[j]);

    /* ---- LinearAlignment (:128-202) ---- */
    int n = 3 * nf + 4;
    r->n_state = n;
    double tA[6 * 10], tb[6], rA[100], rb[10];
    memset(A, 0, sizeof(double) * n * n); memset(b, 0, sizeof(double) * n);
    for (int i = 0; i + 1 < nf; i++) {
        pair_rows(&F[i], &F[i + 1], r->rp_delta_p[i + 1], r->rp_delta_v[i + 1], r->rp_sum_dt[i + 1], p->tic, NULL, NULL, tA, tb);
        pair_normal(tA, tb, 10, rA, rb);
        pair_add(A, b, n, i, 10, rA, rb);
    }
    for (int k = 0; k < n * n; k++) A[k] = A[k] * 1000.0;
    for (int k = 0; k < n; k++) b[k] = b[k] * 1000.0;
    ldlt_solve(A, n, b);
    double s = b[n - 1] / 100.0, g[3] = {b[n - 4], b[n - 3], b[n - 2]};
    memcpy(r->g_linear, g, sizeof(g)); r->s_linear = s;
    if (fabs(norm3(g) - Gn) > 1.0) return r->status = ISV_ALIGN_REFUSED_GRAVITY;
    if (s < 0) return r->status = ISV_ALIGN_REFUSED_SCALE;

    /* ---- RefineGravity (:56-126) ---- */
    double g0[3], lxly[6];
    normalized3(g, g0);
    for (int k = 0; k < 3; k++) g0[k] = g0[k] * Gn;
    n = 3 * nf + 3;
    double x[MAXN];
    memset(A, 0, sizeof(double) * n * n); memset(b, 0, sizeof(double) * n);   /* quirk Q2: once, before the passes */
    for (int pass = 0; pass < 4; pass++) {
        tangent_basis(g0, lxly);
        for (int i = 0; i + 1 < nf; i++) {
            pair_rows(&F[i], &F[i + 1], r->rp_delta_p[i + 1], r->rp_delta_v[i + 1], r->rp_sum_dt[i + 1], p->tic, lxly, g0, tA, tb);
            pair_normal(tA, tb, 9, rA, rb);
            pair_add(A, b, n, i, 9, rA, rb);
        }
        for (int k = 0; k < n * n; k++) A[k] = A[k] * 1000.0;
        for (int k = 0; k < n; k++) b[k] = b[k] * 1000.0;
        static double L[MAXN * MAXN];
        memcpy(L, A, sizeof(double) * n * n);
        memcpy(x, b, sizeof(double) * n);
        ldlt_solve(L, n, x);
        double gn[3];
        for (int k = 0; k < 3; k++) gn[k] = g0[k] + (lxly[k * 2] * x[n - 3] + lxly[k * 2 + 1] * x[n - 2]);
        normalized3(gn, g0);
        for (int k = 0; k < 3; k++) g0[k] = g0[k] * Gn;
    }
    s = x[n - 1] / 100.0;
    x[n - 1] = s;
    memcpy(r->g_c0, g0, sizeof(g0));
    memcpy(r->x, x, sizeof(double) * n);
    if (s < 0.0) return r->status = ISV_ALIGN_REFUSED_REFINED_SCALE;

    /* ---- visualInitialAlign's state rebuild (estimator.cpp:367-429) ---- */
    double R0[9];
    {   /* Utility::g2R (utility.cpp:3-13): Quaterniond::FromTwoVectors(g, z), then the yaw removed */
        /* ng1 = g.normalized(); FromTwoVectors(ng1, (0,0,1)) normalises again: c = v1.dot(v0) = v0.z, axis = v0 x v1 */
        double ng1[3], v0[3];
        normalized3(g0, ng1);
        normalized3(ng1, v0);
        double c = v0[2];
        if (c < -1.0 + 1e-12) return r->status = ISV_ALIGN_REFUSED_ANTIPARALLEL;
        double ax[3] = {v0[1], -v0[0], 0.0};
        double sq = sqrt((1.0 + c) * 2.0), invs = 1.0 / sq;
        quat_t q = {sq * 0.5, ax[0] * invs, ax[1] * invs, ax[2] * invs};
        double Rq[9], ypr[3], Ry[9];
        q_to_R(q, Rq);
        R2ypr(Rq, ypr);
        double my[3] = {-ypr[0], 0, 0};
        ypr2R(my, Ry);
        mm(Ry, Rq, R0, 3, 3, 3);
    }
    double Ps[ISV_ALIGN_MAX_WINDOW][3], Rs[ISV_ALIGN_MAX_WINDOW][9], Vs[ISV_ALIGN_MAX_WINDOW][3];
    for (int i = 0; i < nw; i++) { memcpy(Ps[i], F[p->window_frame[i]].T, 24); memcpy(Rs[i], F[p->window_frame[i]].R, 72); }
    double Rt0[3];
    m3v(Rs[0], p->tic, Rt0);
    double P0[3];
    for (int k = 0; k < 3; k++) P0[k] = s * Ps[0][k] - Rt0[k];
    for (int i = nw - 1; i >= 0; i--) {
        double Rt[3];
        m3v(Rs[i], p->tic, Rt);
        for (int k = 0; k < 3; k++) Ps[i][k] = s * Ps[i][k] - Rt[k] - P0[k];
    }
    /* quirk Q3: kv counts keyframes (the window's frames after :371), x is indexed by the frames of all_image_frame */
    for (int f = 0, kv = -1, wi = 0; f < nf; f++) {
        int in_window = wi < nw && p->window_frame[wi] == f;
        if (in_window) wi++;
        if (in_window || F[f].is_key_frame) { kv++; m3v(F[f].R, x + 3 * kv, Vs[kv]); }
    }
    {
        double RR[9], ypr[3], Ry[9], T[9];
        mm(R0, Rs[0], RR, 3, 3, 3);
        R2ypr(RR, ypr);
        double my[3] = {-ypr[0], 0, 0};
        ypr2R(my, Ry);
        mm(Ry, R0, T, 3, 3, 3);
        memcpy(R0, T, sizeof(T));
    }
    m3v(R0, g0, r->g);
    r->s = s;
    memcpy(r->R0, R0, sizeof(R0));
    for (int i = 0; i < nw; i++) {
        m3v(R0, Ps[i], r->Ps[i]);
        mm(R0, Rs[i], r->Rs[i], 3, 3, 3);
        m3v(R0, Vs[i], r->Vs[i]);
    }
    return r->status = ISV_ALIGN_OK;
}
