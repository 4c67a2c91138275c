/*
 * isv_sfm_oracle.c -- CPU restatement of the SfM stage of the initialisation (is-vins_amd/csrc/isv_sfm.h: IMU excitation,
 * GlobalSFM::construct with its BA, solveFrameByPnP, the all-frame PnP), the checker of k_sfm.  TEST INFRASTRUCTURE ONLY:
 * built by the tests into a temporary directory with
 *   gcc -O2 -ffp-contract=off -shared -fPIC
 * and never linked into the library.  Every sum runs in the kernel's order (serial, in index order; the BA's cost, model cost
 * and norms per point, then over points), so the two differ only where libm and the device math library round
 * sin / cos / acos / exp apart.  Quirks S1..S8 are described in isv_sfm.h and marked where they happen.
 *
 * Restated (the reference cannot be built without Eigen, Ceres and OpenCV): src/estimator.cpp:213-347,
 * src/initial/initial_sfm.cpp, include/initial/initial_sfm.h.
 */
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "../../is-vins_amd/csrc/isv_sfm.h"

#define NW ISV_ALIGN_MAX_WINDOW
#define NT ISV_SFM_MAX_TRACKS
#define MAXC (6 * NW)

/* test hook: a set bit replaces a reproduced quirk by the "obvious" behaviour, so that the tests can show each quirk matters.
 * 1: S1, sum_g starts at (1, 1, 1) instead of zero; 2: S2, no float32 rounding of the PnP points; 4: S4, a non-keyframe
 * guesses from the previous keyframe; 8: S5, step 5 leaves a point behind either camera untriangulated. */
static int g_quirk_off = 0;
void isvo_sfm_set_quirks_off(int mask) { g_quirk_off = mask; }
#define FR(x) ((g_quirk_off & 2) ? (x) : (double)(float)(x))
/* test hook: the BA's max_num_iterations (the library's ISV_DEBUG_SFM_BA_ITERS); outside 0..50 means the default, 50 */
static int g_ba_max_it = 50;
void isvo_sfm_set_ba_max_iterations(int k) { g_ba_max_it = (k >= 0 && k <= 50) ? k : 50; }

/* ---------------- Eigen 3.3 JacobiSVD, square n x n (n <= 6), no QR preconditioner ---------------- */
/* A row-major, overwritten; w: singular values (sorted, descending); U (may be NULL), V: n x n row-major */
static void svd_jacobi(int n, double *A, double *w, double *U, double *V) {
    double scale = 0;
    for (int k = 0; k < n * n; k++) scale = fabs(A[k]) > scale ? fabs(A[k]) : scale;
    if (scale == 0.0) scale = 1.0;
    for (int k = 0; k < n * n; k++) A[k] /= scale;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            V[i * n + j] = i == j ? 1.0 : 0.0;
            if (U) U[i * n + j] = i == j ? 1.0 : 0.0;
        }
    const double considerAsZero = DBL_MIN, precision = 2.0 * DBL_EPSILON;
    double maxDiag = 0;
    for (int i = 0; i < n; i++) maxDiag = fabs(A[i * n + i]) > maxDiag ? fabs(A[i * n + i]) : maxDiag;
    int finished = 0;
    for (int sweep = 0; !finished && sweep < 64; sweep++) {   /* (Eigen has no sweep cap; 64 is never reached on finite input) */
        finished = 1;
        for (int p = 1; p < n; p++)
            for (int q = 0; q < p; q++) {
                double thr = precision * maxDiag > considerAsZero ? precision * maxDiag : considerAsZero;
                if (!(fabs(A[p * n + q]) > thr || fabs(A[q * n + p]) > thr)) continue;
                finished = 0;
                /* real_2x2_jacobi_svd */
                double m00 = A[p * n + p], m01 = A[p * n + q], m10 = A[q * n + p], m11 = A[q * n + q];
                double c1, s1;
                double t = m00 + m11, d = m10 - m01;
                if (fabs(d) < DBL_MIN) { s1 = 0.0; c1 = 1.0; }
                else { double u = t / d, tmp = sqrt(1.0 + u * u); s1 = 1.0 / tmp; c1 = u / tmp; }
                { double a0 = m00, a1 = m01, b0 = m10, b1 = m11;   /* m.applyOnTheLeft(0, 1, rot1) */
                  m00 = c1 * a0 + s1 * b0; m01 = c1 * a1 + s1 * b1; m10 = -s1 * a0 + c1 * b0; m11 = -s1 * a1 + c1 * b1; }
                double cr, sr;   /* j_right.makeJacobi(m, 0, 1) */
                {
                    double deno = 2.0 * fabs(m01);
                    if (deno < DBL_MIN) { cr = 1.0; sr = 0.0; }
                    else {
                        double tau = (m00 - m11) / deno, ww = sqrt(tau * tau + 1.0), tt;
                        tt = tau > 0.0 ? 1.0 / (tau + ww) : 1.0 / (tau - ww);
                        double sign_t = tt > 0.0 ? 1.0 : -1.0, nn = 1.0 / sqrt(tt * tt + 1.0);
                        sr = -sign_t * (m01 / fabs(m01)) * fabs(tt) * nn;
                        cr = nn;
                    }
                }
                /* j_left = rot1 * j_right.transpose() */
                const double so = -sr;
                const double cl = c1 * cr - s1 * so, sl = c1 * so + s1 * cr;
                for (int k = 0; k < n; k++) {   /* A.applyOnTheLeft(p, q, j_left) */
                    double x = A[p * n + k], y = A[q * n + k];
                    A[p * n + k] = cl * x + sl * y; A[q * n + k] = -sl * x + cl * y;
                }
                if (U) for (int k = 0; k < n; k++) {   /* U.applyOnTheRight(p, q, j_left.transpose()) */
                    double x = U[k * n + p], y = U[k * n + q];
                    U[k * n + p] = cl * x + sl * y; U[k * n + q] = -sl * x + cl * y;
                }
                for (int k = 0; k < n; k++) {   /* A.applyOnTheRight(p, q, j_right) */
                    double x = A[k * n + p], y = A[k * n + q];
                    A[k * n + p] = cr * x + so * y; A[k * n + q] = -so * x + cr * y;
                }
                for (int k = 0; k < n; k++) {   /* V.applyOnTheRight(p, q, j_right) */
                    double x = V[k * n + p], y = V[k * n + q];
                    V[k * n + p] = cr * x + so * y; V[k * n + q] = -so * x + cr * y;
                }
                double ap = fabs(A[p * n + p]), aq = fabs(A[q * n + q]);
                double mx = ap > aq ? ap : aq;
                maxDiag = maxDiag > mx ? maxDiag : mx;
            }
    }
    for (int i = 0; i < n; i++) {
        double a = A[i * n + i];
        w[i] = fabs(a);
        if (U && a < 0.0) for (int k = 0; k < n; k++) U[k * n + i] = -U[k * n + i];
    }
    for (int i = 0; i < n; i++) w[i] *= scale;
    for (int i = 0; i < n; i++) {   /* sort: tail(n - i).maxCoeff(&pos), first on ties */
        int pos = i;
        for (int k = i + 1; k < n; k++) if (w[k] > w[pos]) pos = k;
        if (w[pos] == 0.0) break;
        if (pos != i) {
            double tw = w[i]; w[i] = w[pos]; w[pos] = tw;
            for (int k = 0; k < n; k++) {
                double tv = V[k * n + i]; V[k * n + i] = V[k * n + pos]; V[k * n + pos] = tv;
                if (U) { double tu = U[k * n + i]; U[k * n + i] = U[k * n + pos]; U[k * n + pos] = tu; }
            }
        }
    }
}

/* GlobalSFM::triangulatePoint: P0 / P1 are 3 x 4 row-major [R | t] */
static void triangulate(const double *P0, const double *P1, const double *x0, const double *x1, double *out) {
    double A[16], w[4], V[16];
    for (int k = 0; k < 4; k++) {
        A[k] = x0[0] * P0[8 + k] - P0[k];
        A[4 + k] = x0[1] * P0[8 + k] - P0[4 + k];
        A[8 + k] = x1[0] * P1[8 + k] - P1[k];
        A[12 + k] = x1[1] * P1[8 + k] - P1[4 + k];
    }
    svd_jacobi(4, A, w, NULL, V);
    out[0] = V[0 * 4 + 3] / V[3 * 4 + 3];
    out[1] = V[1 * 4 + 3] / V[3 * 4 + 3];
    out[2] = V[2 * 4 + 3] / V[3 * 4 + 3];
}

/* ---------------- Eigen quaternion pieces (w x y z here) ---------------- */
static void eq_from_R(const double *m, double *q) {   /* Quaternion(Matrix3d) */
    double t = m[0] + m[4] + m[8];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[0] = 0.5 * t; t = 0.5 / t;
        q[1] = (m[7] - m[5]) * t; q[2] = (m[2] - m[6]) * t; q[3] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[i * 4]) i = 2;
        int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1.0);
        q[1 + i] = 0.5 * t; t = 0.5 / t;
        q[0] = (m[k * 3 + j] - m[j * 3 + k]) * t;
        q[1 + j] = (m[j * 3 + i] + m[i * 3 + j]) * t;
        q[1 + k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
    }
}
static void eq_to_R(const double *q, double *r) {     /* toRotationMatrix (no normalisation) */
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    r[0] = 1.0 - (tyy + tzz); r[1] = txy - twz; r[2] = txz + twy;
    r[3] = txy + twz; r[4] = 1.0 - (txx + tzz); r[5] = tyz - twx;
    r[6] = txz - twy; r[7] = tyz + twx; r[8] = 1.0 - (txx + tyy);
}
static void eq_inv(const double *q, double *o) {      /* inverse(): conjugate / squaredNorm (S6) */
    double n2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3] + q[0] * q[0];
    if (n2 > 0.0) { o[0] = q[0] / n2; o[1] = -q[1] / n2; o[2] = -q[2] / n2; o[3] = -q[3] / n2; }
    else { o[0] = o[1] = o[2] = o[3] = 0.0; }
}
static void eq_mul(const double *a, const double *b, double *o) {
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
    o[3] = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
}
static void eq_transform(const double *q, const double *v, double *o) {   /* _transformVector: assumes |q| = 1 (S6) */
    double uv[3] = {q[2] * v[2] - q[3] * v[1], q[3] * v[0] - q[1] * v[2], q[1] * v[1] - q[2] * v[0]};
    for (int k = 0; k < 3; k++) uv[k] += uv[k];
    double c[3] = {q[2] * uv[2] - q[3] * uv[1], q[3] * uv[0] - q[1] * uv[2], q[1] * uv[1] - q[2] * uv[0]};
    for (int k = 0; k < 3; k++) o[k] = v[k] + q[0] * uv[k] + c[k];
}
static void mv3(const double *M, const double *v, double *o) {
    for (int a = 0; a < 3; a++) o[a] = M[a * 3] * v[0] + M[a * 3 + 1] * v[1] + M[a * 3 + 2] * v[2];
}
static void mmT3(const double *A, const double *B, double *C) {   /* A * B^T */
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j * 3] + A[i * 3 + 1] * B[j * 3 + 1] + A[i * 3 + 2] * B[j * 3 + 2];
}

/* ---------------- OpenCV 3.2 Rodrigues and the iterative PnP ---------------- */
static void rodrigues_v2m(const double *rv, double *R, double *J) {   /* J: 3 x 9 (d R / d r_i), may be NULL */
    double rx = rv[0], ry = rv[1], rz = rv[2];
    double theta = sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < DBL_EPSILON) {
        for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
        if (J) { memset(J, 0, 27 * sizeof(double)); J[5] = J[15] = J[19] = -1; J[7] = J[11] = J[21] = 1; }
        return;
    }
    const double c = cos(theta), s = sin(theta), c1 = 1. - c, itheta = theta ? 1. / theta : 0.;
    rx *= itheta; ry *= itheta; rz *= itheta;
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double rx_[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
    for (int k = 0; k < 9; k++) R[k] = c * I[k] + c1 * rrt[k] + s * rx_[k];
    if (J) {
        const double drrt[27] = {rx + rx, ry, rz, ry, 0, 0, rz, 0, 0, 0, rx, 0, rx, ry + ry, rz, 0, rz, 0, 0, 0, rx, 0, 0, ry, rx, ry, rz + rz};
        const double drx[27] = {0, 0, 0, 0, 0, -1, 0, 1, 0, 0, 0, 1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 1, 0, 0, 0, 0, 0};
        for (int i = 0; i < 3; i++) {
            double ri = i == 0 ? rx : i == 1 ? ry : rz;
            double a0 = -s * ri, a1 = (s - 2 * c1 * itheta) * ri, a2 = c1 * itheta, a3 = (c - s * itheta) * ri, a4 = s * itheta;
            for (int k = 0; k < 9; k++) J[i * 9 + k] = a0 * I[k] + a1 * rrt[k] + a2 * drrt[i * 9 + k] + a3 * rx_[k] + a4 * drx[i * 9 + k];
        }
    }
}
static void rodrigues_m2v(const double *R, double *rv) {   /* (the SVD re-orthonormalisation is dropped: isv_sfm.h) */
    double r[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    double s = sqrt((r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1) * 0.5;
    c = c > 1. ? 1. : c < -1. ? -1. : c;
    double theta = acos(c);
    if (s < 1e-5) {
        if (c > 0) { r[0] = r[1] = r[2] = 0; }
        else {
            double t;
            t = (R[0] + 1) * 0.5; r[0] = sqrt(t > 0. ? t : 0.);
            t = (R[4] + 1) * 0.5; r[1] = sqrt(t > 0. ? t : 0.) * (R[1] < 0 ? -1. : 1.);
            t = (R[8] + 1) * 0.5; r[2] = sqrt(t > 0. ? t : 0.) * (R[2] < 0 ? -1. : 1.);
            if (fabs(r[0]) < fabs(r[1]) && fabs(r[0]) < fabs(r[2]) && (R[5] > 0) != (r[1] * r[2] > 0)) r[2] = -r[2];
            theta /= sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
            for (int k = 0; k < 3; k++) r[k] *= theta;
        }
    } else {
        double vth = 1 / (2 * s);
        vth *= theta;
        for (int k = 0; k < 3; k++) r[k] *= vth;
    }
    for (int k = 0; k < 3; k++) rv[k] = r[k];
}
/* cvProjectPoints2 of one point (K = I, no distortion): err = projection - observation, J: 2 x 6 (dp/dr | dp/dt) */
static void pnp_project(const double *R, const double *dRdr, const double *tv, const double *X, const double *m, double *err, double *J) {
    const double x0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + tv[0];
    const double y0 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + tv[1];
    double z = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + tv[2];
    z = z ? 1. / z : 1;
    const double x = x0 * z, y = y0 * z;
    err[0] = x - m[0]; err[1] = y - m[1];
    if (!J) return;
    for (int j = 0; j < 3; j++) {
        double dx0 = X[0] * dRdr[9 * j + 0] + X[1] * dRdr[9 * j + 1] + X[2] * dRdr[9 * j + 2];
        double dy0 = X[0] * dRdr[9 * j + 3] + X[1] * dRdr[9 * j + 4] + X[2] * dRdr[9 * j + 5];
        double dz0 = X[0] * dRdr[9 * j + 6] + X[1] * dRdr[9 * j + 7] + X[2] * dRdr[9 * j + 8];
        J[j] = z * (dx0 - x * dz0);
        J[6 + j] = z * (dy0 - y * dz0);
    }
    J[3] = z; J[4] = 0; J[5] = -x * z;
    J[9] = 0; J[10] = z; J[11] = -y * z;
}
/* err and, if J, JtJ (lower 21) / JtErr over the points in order; returns |err|_2 */
static double pnp_eval(int n, const double *P3, const double *P2, const double *param, double *JtJ, double *JtE) {
    double R[9], dRdr[27];
    rodrigues_v2m(param, R, JtJ ? dRdr : NULL);
    double e2 = 0;
    if (JtJ) { memset(JtJ, 0, 36 * sizeof(double)); memset(JtE, 0, 6 * sizeof(double)); }
    for (int i = 0; i < n; i++) {
        double err[2], J[12];
        pnp_project(R, dRdr, param + 3, P3 + 3 * i, P2 + 2 * i, err, JtJ ? J : NULL);
        for (int r = 0; r < 2; r++) {
            e2 += err[r] * err[r];
            if (!JtJ) continue;
            for (int a = 0; a < 6; a++) {
                for (int b = 0; b <= a; b++) JtJ[a * 6 + b] += J[r * 6 + a] * J[r * 6 + b];
                JtE[a] += J[r * 6 + a] * err[r];
            }
        }
    }
    return sqrt(e2);
}
/* CvLevMarq::step: param = prev - solve_svd(JtJ with diag *= 1 + lambda, JtErr) */
static void pnp_step(const double *JtJ, const double *JtE, int lambdaLg10, const double *prev, double *param) {
    const double lambda = exp(lambdaLg10 * log(10.));
    double A[36], U[36], V[36], w[6], x[6];
    for (int a = 0; a < 6; a++)
        for (int b = 0; b < 6; b++) A[a * 6 + b] = a >= b ? JtJ[a * 6 + b] : JtJ[b * 6 + a];
    for (int a = 0; a < 6; a++) A[a * 6 + a] *= 1. + lambda;
    svd_jacobi(6, A, w, U, V);
    double thr = 0;
    for (int i = 0; i < 6; i++) thr += w[i];
    thr *= DBL_EPSILON * 2;
    double ub[6];
    for (int i = 0; i < 6; i++) {
        double s = 0;
        for (int k = 0; k < 6; k++) s += U[k * 6 + i] * JtE[k];
        ub[i] = w[i] > thr ? s / w[i] : 0.0;
    }
    for (int k = 0; k < 6; k++) {
        double s = 0;
        for (int i = 0; i < 6; i++) s += V[k * 6 + i] * ub[i];
        x[k] = s;
    }
    for (int k = 0; k < 6; k++) param[k] = prev[k] - x[k];
}
/* cvFindExtrinsicCameraParams2 with useExtrinsicGuess: CvLevMarq (max_iter 20, eps FLT_EPSILON); returns the iterations */
static int pnp_solve(int n, const double *P3, const double *P2, double *rvec, double *tvec) {
    double param[6] = {rvec[0], rvec[1], rvec[2], tvec[0], tvec[1], tvec[2]}, prev[6], JtJ[36], JtE[6];
    int lambdaLg10 = -3, iters = 0;
    double prevErrNorm = 0, errNorm;
    for (;;) {
        double e = pnp_eval(n, P3, P2, param, JtJ, JtE);    /* CALC_J */
        memcpy(prev, param, sizeof(prev));
        pnp_step(JtJ, JtE, lambdaLg10, prev, param);
        if (iters == 0) prevErrNorm = e;
        for (;;) {                                            /* CHECK_ERR */
            errNorm = pnp_eval(n, P3, P2, param, NULL, NULL);
            if (errNorm > prevErrNorm && ++lambdaLg10 <= 16) { pnp_step(JtJ, JtE, lambdaLg10, prev, param); continue; }
            break;
        }
        lambdaLg10 = lambdaLg10 - 1 > -16 ? lambdaLg10 - 1 : -16;
        double dn = 0, pn = 0;
        for (int k = 0; k < 6; k++) { double d = param[k] - prev[k]; dn += d * d; pn += prev[k] * prev[k]; }
        if (++iters >= 20 || sqrt(dn) / (sqrt(pn) + DBL_EPSILON) < FLT_EPSILON) break;
        prevErrNorm = errNorm;
    }
    for (int k = 0; k < 3; k++) { rvec[k] = param[k]; tvec[k] = param[3 + k]; }
    return iters;
}

/* ---------------- the BA (Ceres 2.0 LM over DENSE_SCHUR) ---------------- */
typedef struct {
    int nw, ntr, nc, l;
    const isv_sfm_track_t *tr;
    const double *obs;
    const int *act;               /* active (triangulated) tracks, in order */
    int nact;
    int coff[NW], ncf[NW];        /* first reduced column and free column count (0, 3 or 6) of each frame */
} ba_t;

/* QuaternionRotatePoint + translation + projection; J* unscaled (2 x 3 each); q w x y z */
static void ba_obs(const double *q, const double *t, const double *X, const double *uv, double *r, double *Jq, double *Jt, double *JX) {
    const double sc = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double u[4] = {sc * q[0], sc * q[1], sc * q[2], sc * q[3]};
    const double t2 = u[0] * u[1], t3 = u[0] * u[2], t4 = u[0] * u[3], t5 = -u[1] * u[1], t6 = u[1] * u[2], t7 = u[1] * u[3];
    const double t8 = -u[2] * u[2], t9 = u[2] * u[3], t1 = -u[3] * u[3];
    double RX[3];
    RX[0] = 2.0 * ((t8 + t1) * X[0] + (t6 - t4) * X[1] + (t3 + t7) * X[2]) + X[0];
    RX[1] = 2.0 * ((t4 + t6) * X[0] + (t5 + t1) * X[1] + (t9 - t2) * X[2]) + X[1];
    RX[2] = 2.0 * ((t7 - t3) * X[0] + (t2 + t9) * X[1] + (t5 + t8) * X[2]) + X[2];
    const double p0 = RX[0] + t[0], p1 = RX[1] + t[1], p2 = RX[2] + t[2];
    const double xp = p0 / p2, yp = p1 / p2;
    r[0] = xp - uv[0]; r[1] = yp - uv[1];
    if (!Jq) return;
    const double iz = 1.0 / p2;
    const double Jp[6] = {iz, 0.0, -xp * iz, 0.0, iz, -yp * iz};
    const double M[9] = {2.0 * (t8 + t1) + 1.0, 2.0 * (t6 - t4), 2.0 * (t3 + t7), 2.0 * (t4 + t6), 2.0 * (t5 + t1) + 1.0,
                         2.0 * (t9 - t2), 2.0 * (t7 - t3), 2.0 * (t2 + t9), 2.0 * (t5 + t8) + 1.0};
    const double S[9] = {0.0, -RX[2], RX[1], RX[2], 0.0, -RX[0], -RX[1], RX[0], 0.0};   /* d(R X)/d delta = -2 [R X]x */
    for (int a = 0; a < 2; a++)
        for (int c = 0; c < 3; c++) {
            Jt[a * 3 + c] = Jp[a * 3 + c];
            JX[a * 3 + c] = Jp[a * 3] * M[c] + Jp[a * 3 + 1] * M[3 + c] + Jp[a * 3 + 2] * M[6 + c];
            Jq[a * 3 + c] = -2.0 * (Jp[a * 3] * S[c] + Jp[a * 3 + 1] * S[3 + c] + Jp[a * 3 + 2] * S[6 + c]);
        }
}
/* scaled E (2 x 3) and F (2 x ncf) of one observation; r the residual */
static void ba_EF(const ba_t *B, const double *cq, const double *ct, const double *X, int f, const double *uv, const double *psc,
                  const double *csc, double *r, double *E, double *F) {
    double Jq[6], Jt[6], JX[6];
    ba_obs(cq + 4 * f, ct + 3 * f, X, uv, r, Jq, Jt, JX);
    for (int a = 0; a < 2; a++) {
        for (int k = 0; k < 3; k++) E[a * 3 + k] = JX[a * 3 + k] * psc[k];
        for (int c = 0; c < B->ncf[f]; c++) F[a * 6 + c] = (c < 3 ? Jq[a * 3 + c] : Jt[a * 3 + c - 3]) * csc[B->coff[f] + c];
    }
}
static void quat_plus(const double *x, const double *d, double *o) {   /* QuaternionParameterization::Plus */
    const double nd = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (nd > 0.0) {
        const double sdd = sin(nd) / nd;
        const double qd[4] = {cos(nd), sdd * d[0], sdd * d[1], sdd * d[2]};
        eq_mul(qd, x, o);
    } else memcpy(o, x, 4 * sizeof(double));
}
static double ba_cost(const ba_t *B, const double *cq, const double *ct, const double *X) {
    double cost = 0;
    for (int a = 0; a < B->nact; a++) {
        const isv_sfm_track_t *T = &B->tr[B->act[a]];
        double cp = 0;
        for (int k = 0; k < T->n_obs; k++) {
            double r[2];
            ba_obs(cq + 4 * (T->start_frame + k), ct + 3 * (T->start_frame + k), X + 3 * B->act[a], B->obs + 2 * (T->obs_off + k), r, NULL, NULL, NULL);
            cp += 0.5 * (r[0] * r[0] + r[1] * r[1]);
        }
        cost += cp;
    }
    return cost;
}
/* column sums of squares of the Jacobian scaled by psc / csc (unscaled: both 1), and, if g, the unscaled gradient J^T r */
static void ba_colnorm(const ba_t *B, const double *cq, const double *ct, const double *X, const double *psc, const double *csc,
                       double *pn, double *cn, double *pg, double *cg) {
    for (int a = 0; a < B->nact; a++) {
        const int p = B->act[a];
        const isv_sfm_track_t *T = &B->tr[p];
        double s[3] = {0, 0, 0}, g[3] = {0, 0, 0};
        for (int k = 0; k < T->n_obs; k++) {
            double r[2], Jq[6], Jt[6], JX[6];
            ba_obs(cq + 4 * (T->start_frame + k), ct + 3 * (T->start_frame + k), X + 3 * p, B->obs + 2 * (T->obs_off + k), r, Jq, Jt, JX);
            for (int row = 0; row < 2; row++)
                for (int c = 0; c < 3; c++) {
                    double e = JX[row * 3 + c] * psc[3 * p + c];
                    s[c] += e * e;
                    g[c] += JX[row * 3 + c] * r[row];
                }
        }
        for (int c = 0; c < 3; c++) { pn[3 * p + c] = s[c]; if (pg) pg[3 * p + c] = g[c]; }
    }
    for (int f = 0; f < B->nw; f++) {
        double s[6] = {0}, g[6] = {0};
        for (int a = 0; a < B->nact; a++) {
            const int p = B->act[a];
            const isv_sfm_track_t *T = &B->tr[p];
            if (f < T->start_frame || f >= T->start_frame + T->n_obs) continue;
            double r[2], Jq[6], Jt[6], JX[6];
            ba_obs(cq + 4 * f, ct + 3 * f, X + 3 * p, B->obs + 2 * (T->obs_off + f - T->start_frame), r, Jq, Jt, JX);
            for (int row = 0; row < 2; row++)
                for (int c = 0; c < B->ncf[f]; c++) {
                    double j = c < 3 ? Jq[row * 3 + c] : Jt[row * 3 + c - 3];
                    double e = j * csc[B->coff[f] + c];
                    s[c] += e * e;
                    g[c] += j * r[row];
                }
        }
        for (int c = 0; c < B->ncf[f]; c++) { cn[B->coff[f] + c] = s[c]; if (cg) cg[B->coff[f] + c] = g[c]; }
    }
}
/* the ambient state's squared norm (points in track order, then the free camera blocks), or of x - y */
static double ba_norm2(const ba_t *B, const double *cq, const double *ct, const double *X, const double *cq2, const double *ct2, const double *X2) {
    double s = 0;
    for (int a = 0; a < B->nact; a++) {
        const int p = B->act[a];
        double pp = 0;
        for (int k = 0; k < 3; k++) { double d = X[3 * p + k] - (X2 ? X2[3 * p + k] : 0.0); pp += d * d; }
        s += pp;
    }
    for (int f = 0; f < B->nw; f++) {
        if (B->ncf[f] >= 3) for (int k = 0; k < 4; k++) { double d = cq[4 * f + k] - (cq2 ? cq2[4 * f + k] : 0.0); s += d * d; }
        if (B->ncf[f] == 6) for (int k = 0; k < 3; k++) { double d = ct[3 * f + k] - (ct2 ? ct2[3 * f + k] : 0.0); s += d * d; }
    }
    return s;
}
/* x (+) delta over the free blocks */
static void ba_plus(const ba_t *B, const double *cq, const double *ct, const double *X, const double *dp, const double *dc,
                    double *oq, double *ot, double *oX) {
    for (int a = 0; a < B->nact; a++) { const int p = B->act[a]; for (int k = 0; k < 3; k++) oX[3 * p + k] = X[3 * p + k] + dp[3 * p + k]; }
    for (int f = 0; f < B->nw; f++) {
        if (B->ncf[f] >= 3) quat_plus(cq + 4 * f, dc + B->coff[f], oq + 4 * f); else memcpy(oq + 4 * f, cq + 4 * f, 32);
        if (B->ncf[f] == 6) for (int k = 0; k < 3; k++) ot[3 * f + k] = ct[3 * f + k] + dc[B->coff[f] + 3 + k];
        else memcpy(ot + 3 * f, ct + 3 * f, 24);
    }
}
static double ba_gmax(const ba_t *B, const double *cq, const double *ct, const double *X, const double *pg, const double *cg) {
    double m = 0;
    for (int a = 0; a < B->nact; a++) {
        const int p = B->act[a];
        for (int k = 0; k < 3; k++) { double v = fabs(X[3 * p + k] - (X[3 * p + k] + -pg[3 * p + k])); m = v > m ? v : m; }
    }
    for (int f = 0; f < B->nw; f++) {
        if (B->ncf[f] >= 3) {
            double ng[3] = {-cg[B->coff[f]], -cg[B->coff[f] + 1], -cg[B->coff[f] + 2]}, qp[4];
            quat_plus(cq + 4 * f, ng, qp);
            for (int k = 0; k < 4; k++) { double v = fabs(cq[4 * f + k] - qp[k]); m = v > m ? v : m; }
        }
        if (B->ncf[f] == 6)
            for (int k = 0; k < 3; k++) { double v = fabs(ct[3 * f + k] - (ct[3 * f + k] + -cg[B->coff[f] + 3 + k])); m = v > m ? v : m; }
    }
    return m;
}
/* 3 x 3 LLT and its inverse (solve against the identity, column by column) */
static void inv3_llt(const double *A, double *W) {
    double L[9] = {0};
    for (int j = 0; j < 3; j++) {
        double s = A[j * 3 + j];
        for (int k = 0; k < j; k++) s -= L[j * 3 + k] * L[j * 3 + k];
        L[j * 3 + j] = sqrt(s);
        for (int i = j + 1; i < 3; i++) {
            double v = A[i * 3 + j];
            for (int k = 0; k < j; k++) v -= L[i * 3 + k] * L[j * 3 + k];
            L[i * 3 + j] = v / L[j * 3 + j];
        }
    }
    for (int c = 0; c < 3; c++) {
        double y[3];
        for (int i = 0; i < 3; i++) { double v = i == c ? 1.0 : 0.0; for (int k = 0; k < i; k++) v -= L[i * 3 + k] * y[k]; y[i] = v / L[i * 3 + i]; }
        for (int i = 2; i >= 0; i--) { double v = y[i]; for (int k = i + 1; k < 3; k++) v -= L[k * 3 + i] * W[k * 3 + c]; W[i * 3 + c] = v / L[i * 3 + i]; }
    }
}
static int pk(int r, int c) { return r * (r + 1) / 2 + c; }

/* one LM step's linear system: fills the step (pdx per point, cdx per column, both the NEGATED Schur solution, scaled space);
 * returns 1 when the Cholesky of the reduced system failed */
static int ba_schur(const ba_t *B, const double *cq, const double *ct, const double *X, const double *psc, const double *csc,
                    const double *pD, const double *cD, double *Wp, double *gp, double *S, double *rhs, double *pdx, double *cdx) {
    const int nc = B->nc;
    for (int a = 0; a < B->nact; a++) {   /* point blocks: ete = D^2 + sum E^T E, its inverse, g = E^T r */
        const int p = B->act[a];
        const isv_sfm_track_t *T = &B->tr[p];
        double ete[9] = {0}, g[3] = {0, 0, 0};
        for (int k = 0; k < 3; k++) ete[k * 4] = pD[3 * p + k] * pD[3 * p + k];
        for (int k = 0; k < T->n_obs; k++) {
            const int f = T->start_frame + k;
            double r[2], E[6], F[12];
            ba_EF(B, cq, ct, X + 3 * p, f, B->obs + 2 * (T->obs_off + k), psc + 3 * p, csc, r, E, F);
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) ete[i * 3 + j] += E[i] * E[j] + E[3 + i] * E[3 + j];
                g[i] += E[i] * r[0] + E[3 + i] * r[1];
            }
        }
        inv3_llt(ete, Wp + 9 * p);
        for (int k = 0; k < 3; k++) gp[3 * p + k] = g[k];
    }
    int fr[MAXC];
    for (int f = 0; f < B->nw; f++) for (int c = 0; c < B->ncf[f]; c++) fr[B->coff[f] + c] = f;
    /* S = D^2 + sum over points (track order) of F^T F - (E^T F)^T W (E^T F), one frame-pair block at a time (every entry
     * still adds its points in order) */
    for (int fa = 0; fa < B->nw; fa++)
        for (int fb = 0; fb <= fa; fb++) {
            const int na = B->ncf[fa], nb = B->ncf[fb];
            if (!na || !nb) continue;
            double s[36];
            for (int a = 0; a < na; a++) for (int b = 0; b < nb; b++) s[a * 6 + b] = (fa == fb && a == b) ? cD[B->coff[fa] + a] * cD[B->coff[fa] + a] : 0.0;
            for (int q = 0; q < B->nact; q++) {
                const int p = B->act[q];
                const isv_sfm_track_t *T = &B->tr[p];
                if (fa < T->start_frame || fa >= T->start_frame + T->n_obs || fb < T->start_frame || fb >= T->start_frame + T->n_obs) continue;
                double r[2], Ea[6], Fa[12], Eb[6], Fb[12], Ba[18], Bb[18];
                ba_EF(B, cq, ct, X + 3 * p, fa, B->obs + 2 * (T->obs_off + fa - T->start_frame), psc + 3 * p, csc, r, Ea, Fa);
                ba_EF(B, cq, ct, X + 3 * p, fb, B->obs + 2 * (T->obs_off + fb - T->start_frame), psc + 3 * p, csc, r, Eb, Fb);
                for (int c = 0; c < 6; c++)
                    for (int k = 0; k < 3; k++) {
                        if (c < na) Ba[k * 6 + c] = Ea[k] * Fa[c] + Ea[3 + k] * Fa[6 + c];
                        if (c < nb) Bb[k * 6 + c] = Eb[k] * Fb[c] + Eb[3 + k] * Fb[6 + c];
                    }
                const double *W = Wp + 9 * p;
                for (int b = 0; b < nb; b++) {
                    double wb[3];
                    for (int k = 0; k < 3; k++) wb[k] = W[k * 3] * Bb[b] + W[k * 3 + 1] * Bb[6 + b] + W[k * 3 + 2] * Bb[12 + b];
                    for (int a = 0; a < na; a++) {
                        if (fa == fb && b > a) continue;
                        double v = s[a * 6 + b];
                        if (fa == fb) v += Fa[a] * Fa[b] + Fa[6 + a] * Fa[6 + b];
                        v -= Ba[a] * wb[0] + Ba[6 + a] * wb[1] + Ba[12 + a] * wb[2];
                        s[a * 6 + b] = v;
                    }
                }
            }
            for (int a = 0; a < na; a++)
                for (int b = 0; b < nb; b++)
                    if (fa != fb || b <= a) S[pk(B->coff[fa] + a, B->coff[fb] + b)] = s[a * 6 + b];
        }
    for (int ra = 0; ra < nc; ra++) {
        const int fa = fr[ra], a = ra - B->coff[fa];
        double s = 0;
        for (int q = 0; q < B->nact; q++) {
            const int p = B->act[q];
            const isv_sfm_track_t *T = &B->tr[p];
            if (fa < T->start_frame || fa >= T->start_frame + T->n_obs) continue;
            double r[2], E[6], F[12], Ba[3], wg[3];
            ba_EF(B, cq, ct, X + 3 * p, fa, B->obs + 2 * (T->obs_off + fa - T->start_frame), psc + 3 * p, csc, r, E, F);
            s += F[a] * r[0] + F[6 + a] * r[1];
            const double *W = Wp + 9 * p, *g = gp + 3 * p;
            for (int k = 0; k < 3; k++) { Ba[k] = E[k] * F[a] + E[3 + k] * F[6 + a]; wg[k] = W[k * 3] * g[0] + W[k * 3 + 1] * g[1] + W[k * 3 + 2] * g[2]; }
            s -= Ba[0] * wg[0] + Ba[1] * wg[1] + Ba[2] * wg[2];
        }
        rhs[ra] = s;
    }
    /* dense Cholesky (left-looking, unblocked) of the packed reduced system, then the two triangular solves */
    for (int j = 0; j < nc; j++) {
        double s = S[pk(j, j)];
        for (int k = 0; k < j; k++) s -= S[pk(j, k)] * S[pk(j, k)];
        if (!(s > 0.0)) return 1;
        S[pk(j, j)] = sqrt(s);
        for (int i = j + 1; i < nc; i++) {
            double v = S[pk(i, j)];
            for (int k = 0; k < j; k++) v -= S[pk(i, k)] * S[pk(j, k)];
            S[pk(i, j)] = v / S[pk(j, j)];
        }
    }
    for (int i = 0; i < nc; i++) { double v = rhs[i]; for (int k = 0; k < i; k++) v -= S[pk(i, k)] * rhs[k]; rhs[i] = v / S[pk(i, i)]; }
    for (int i = nc - 1; i >= 0; i--) { double v = rhs[i]; for (int k = i + 1; k < nc; k++) v -= S[pk(k, i)] * rhs[k]; rhs[i] = v / S[pk(i, i)]; }
    for (int c = 0; c < nc; c++) cdx[c] = -rhs[c];
    /* back-substitution: z = ete^-1 sum E^T (r - F y) */
    for (int a = 0; a < B->nact; a++) {
        const int p = B->act[a];
        const isv_sfm_track_t *T = &B->tr[p];
        double v[3] = {0, 0, 0};
        for (int k = 0; k < T->n_obs; k++) {
            const int f = T->start_frame + k;
            double r[2], E[6], F[12], sj[2];
            ba_EF(B, cq, ct, X + 3 * p, f, B->obs + 2 * (T->obs_off + k), psc + 3 * p, csc, r, E, F);
            for (int row = 0; row < 2; row++) {
                double fy = 0;
                for (int c = 0; c < B->ncf[f]; c++) fy += F[row * 6 + c] * rhs[B->coff[f] + c];
                sj[row] = r[row] - fy;
            }
            for (int i = 0; i < 3; i++) v[i] += E[i] * sj[0] + E[3 + i] * sj[1];
        }
        const double *W = Wp + 9 * p;
        for (int i = 0; i < 3; i++) pdx[3 * p + i] = -(W[i * 3] * v[0] + W[i * 3 + 1] * v[1] + W[i * 3 + 2] * v[2]);
    }
    return 0;
}
/* -(J dx) . (r + J dx / 2), per point then over points */
static double ba_model(const ba_t *B, const double *cq, const double *ct, const double *X, const double *psc, const double *csc,
                       const double *pdx, const double *cdx) {
    double mc = 0;
    for (int a = 0; a < B->nact; a++) {
        const int p = B->act[a];
        const isv_sfm_track_t *T = &B->tr[p];
        double mp = 0;
        for (int k = 0; k < T->n_obs; k++) {
            const int f = T->start_frame + k;
            double r[2], E[6], F[12];
            ba_EF(B, cq, ct, X + 3 * p, f, B->obs + 2 * (T->obs_off + k), psc + 3 * p, csc, r, E, F);
            for (int row = 0; row < 2; row++) {
                double m = E[row * 3] * pdx[3 * p] + E[row * 3 + 1] * pdx[3 * p + 1] + E[row * 3 + 2] * pdx[3 * p + 2];
                double fy = 0;
                for (int c = 0; c < B->ncf[f]; c++) fy += F[row * 6 + c] * cdx[B->coff[f] + c];
                m += fy;
                mp += m * (r[row] + m / 2.0);
            }
        }
        mc += mp;
    }
    return -mc;
}

static void ba_solve(const ba_t *B, double *cq, double *ct, double *X, isv_sfm_result_t *out) {
    const int nc = B->nc;
    static double psc[3 * NT], pD[3 * NT], pdiag[3 * NT], pg[3 * NT], pdx[3 * NT], pdel[3 * NT], Xc[3 * NT], Wp[9 * NT], gp[3 * NT];
    static double csc[MAXC], cD[MAXC], cdiag[MAXC], cg[MAXC], cdx[MAXC], cdel[MAXC], rhs[MAXC], S[MAXC * (MAXC + 1) / 2];
    double cqc[4 * NW], ctc[3 * NW];
    double radius = 1e4, decrease_factor = 2.0;
    int reuse = 0, invalid = 0, it = 0, term = ISV_TERM_RUNNING, nsucc = 0;
    for (int k = 0; k < 3 * B->ntr; k++) psc[k] = 1.0;
    for (int k = 0; k < nc; k++) csc[k] = 1.0;
    double x_cost = ba_cost(B, cq, ct, X);
    ba_colnorm(B, cq, ct, X, psc, csc, pdiag, cdiag, pg, cg);
    for (int a = 0; a < B->nact; a++) for (int k = 0; k < 3; k++) { const int i = 3 * B->act[a] + k; psc[i] = 1.0 / (1.0 + sqrt(pdiag[i])); }
    for (int k = 0; k < nc; k++) csc[k] = 1.0 / (1.0 + sqrt(cdiag[k]));
    double gmax = ba_gmax(B, cq, ct, X, pg, cg);
    double x_norm = sqrt(ba_norm2(B, cq, ct, X, NULL, NULL, NULL));
    out->ba_initial_cost = x_cost;
    for (;;) {
        if (it >= g_ba_max_it) { term = ISV_TERM_MAX_ITERATIONS; break; }
        if (gmax <= 1e-10) { term = ISV_TERM_GRADIENT_TOL; break; }
        if (radius <= 1e-32) { term = ISV_TERM_MIN_RADIUS; break; }
        it++;
        if (!reuse) {
            ba_colnorm(B, cq, ct, X, psc, csc, pdiag, cdiag, NULL, NULL);
            for (int a = 0; a < B->nact; a++) for (int k = 0; k < 3; k++) { const int i = 3 * B->act[a] + k; pdiag[i] = fmin(fmax(pdiag[i], 1e-6), 1e32); }
            for (int k = 0; k < nc; k++) cdiag[k] = fmin(fmax(cdiag[k], 1e-6), 1e32);
        }
        reuse = 1;
        for (int a = 0; a < B->nact; a++) for (int k = 0; k < 3; k++) { const int i = 3 * B->act[a] + k; pD[i] = sqrt(pdiag[i] / radius); }
        for (int k = 0; k < nc; k++) cD[k] = sqrt(cdiag[k] / radius);
        int ls_fail = ba_schur(B, cq, ct, X, psc, csc, pD, cD, Wp, gp, S, rhs, pdx, cdx);
        if (!ls_fail) {
            for (int a = 0; a < B->nact; a++) for (int k = 0; k < 3; k++) if (!isfinite(pdx[3 * B->act[a] + k])) ls_fail = 1;
            for (int k = 0; k < nc; k++) if (!isfinite(cdx[k])) ls_fail = 1;
        }
        double mcc = 0;
        int valid = 0;
        if (!ls_fail) { mcc = ba_model(B, cq, ct, X, psc, csc, pdx, cdx); valid = mcc > 0.0; }
        if (!valid) {
            if (++invalid >= 5) { term = ls_fail ? ISV_TERM_LINEAR_SOLVER : ISV_TERM_INVALID_STEPS; break; }
            radius /= decrease_factor; decrease_factor *= 2.0; reuse = 1;
            continue;
        }
        invalid = 0;
        for (int a = 0; a < B->nact; a++) for (int k = 0; k < 3; k++) { const int i = 3 * B->act[a] + k; pdel[i] = pdx[i] * psc[i]; }
        for (int k = 0; k < nc; k++) cdel[k] = cdx[k] * csc[k];
        ba_plus(B, cq, ct, X, pdel, cdel, cqc, ctc, Xc);
        const double cand_cost = ba_cost(B, cqc, ctc, Xc);
        const double step_norm = sqrt(ba_norm2(B, cq, ct, X, cqc, ctc, Xc));
        if (step_norm <= 1e-8 * (x_norm + 1e-8)) { term = ISV_TERM_PARAMETER_TOL; break; }
        if (fabs(x_cost - cand_cost) <= 1e-6 * x_cost) { term = ISV_TERM_FUNCTION_TOL; break; }
        const double rel = (x_cost - cand_cost) / mcc;
        if (rel > 1e-3) {
            memcpy(cq, cqc, sizeof(double) * 4 * B->nw); memcpy(ct, ctc, sizeof(double) * 3 * B->nw);
            for (int a = 0; a < B->nact; a++) for (int k = 0; k < 3; k++) X[3 * B->act[a] + k] = Xc[3 * B->act[a] + k];
            x_norm = sqrt(ba_norm2(B, cq, ct, X, NULL, NULL, NULL));
            x_cost = cand_cost;
            ba_colnorm(B, cq, ct, X, psc, csc, pdiag, cdiag, pg, cg);
            gmax = ba_gmax(B, cq, ct, X, pg, cg);
            radius = radius / fmax(1.0 / 3.0, 1.0 - pow(2.0 * rel - 1.0, 3.0));
            radius = fmin(1e16, radius); decrease_factor = 2.0; reuse = 0;
            nsucc++;
        } else { radius /= decrease_factor; decrease_factor *= 2.0; reuse = 1; }
    }
    out->ba_iterations = it; out->ba_termination = term; out->ba_final_cost = x_cost; out->ba_successful = nsucc;
}

/* ---------------- stages 0-4 ---------------- */
static int check(const isv_sfm_problem_t *p) {
    if (p->n_window > ISV_ALIGN_MAX_WINDOW || p->n_frames > ISV_ALIGN_MAX_FRAMES || p->n_tracks > ISV_SFM_MAX_TRACKS || p->n_obs > ISV_SFM_MAX_OBS)
        return ISV_SFM_REFUSED_CAPACITY;
    if (p->n_window < 2 || p->n_frames < 2 || p->l < 0 || p->l >= p->n_window - 1 || p->n_tracks < 0 || p->n_obs < 0 || p->n_pts < 0)
        return ISV_SFM_REFUSED_INPUT;
    if ((p->n_tracks && (!p->tracks || !p->obs)) || !p->pt_off || (p->n_pts && (!p->pt_id || !p->pt_uv)) || !p->delta_v || !p->sum_dt)
        return ISV_SFM_REFUSED_INPUT;
    if (p->n_tracks && (!p->position || !p->state)) return ISV_SFM_REFUSED_INPUT;
    for (int i = 0; i < p->n_window; i++) {
        int w = p->window_frame[i];
        if (w < 0 || w >= p->n_frames || (i > 0 && w <= p->window_frame[i - 1])) return ISV_SFM_REFUSED_INPUT;
    }
    if (p->window_frame[p->n_window - 1] != p->n_frames - 1) return ISV_SFM_REFUSED_INPUT;
    for (int j = 0; j < p->n_tracks; j++) {
        const isv_sfm_track_t *T = &p->tracks[j];
        if (T->n_obs < 1 || T->start_frame < 0 || T->start_frame + T->n_obs > p->n_window || T->obs_off < 0 || T->obs_off + T->n_obs > p->n_obs)
            return ISV_SFM_REFUSED_INPUT;
    }
    if (p->pt_off[0] != 0 || p->pt_off[p->n_frames] != p->n_pts) return ISV_SFM_REFUSED_INPUT;
    for (int f = 0; f < p->n_frames; f++) {
        if (p->pt_off[f + 1] < p->pt_off[f]) return ISV_SFM_REFUSED_INPUT;
        for (int k = p->pt_off[f] + 1; k < p->pt_off[f + 1]; k++)
            if (p->pt_id[k] <= p->pt_id[k - 1]) return ISV_SFM_REFUSED_INPUT;
    }
    return ISV_SFM_OK;
}

static int in_frame(const isv_sfm_track_t *T, int f) { return f >= T->start_frame && f < T->start_frame + T->n_obs; }

/* solveFrameByPnP(i): the tracks with a position, in track order (S8), seen in frame i; float-rounded (S2) */
static int sfm_pnp(const isv_sfm_problem_t *p, const int *st, const double *pos, int i, double *Rc, double *tc, int *iters, int *npts) {
    static double P3[3 * NT], P2[2 * NT];
    int n = 0;
    for (int j = 0; j < p->n_tracks; j++) {
        const isv_sfm_track_t *T = &p->tracks[j];
        if (!st[j] || !in_frame(T, i)) continue;
        const double *uv = p->obs + 2 * (T->obs_off + i - T->start_frame);
        for (int k = 0; k < 3; k++) P3[3 * n + k] = FR(pos[3 * j + k]);   /* S2 */
        P2[2 * n] = FR(uv[0]); P2[2 * n + 1] = FR(uv[1]);
        n++;
    }
    *npts = n;
    if (n < 10) return 0;   /* S3 */
    double rv[3];
    rodrigues_m2v(Rc, rv);
    *iters = pnp_solve(n, P3, P2, rv, tc);
    rodrigues_v2m(rv, Rc, NULL);
    return 1;
}

static void tri_two(const isv_sfm_problem_t *p, int *st, double *pos, int f0, const double *P0, int f1, const double *P1) {
    for (int j = 0; j < p->n_tracks; j++) {
        const isv_sfm_track_t *T = &p->tracks[j];
        if (st[j] || !in_frame(T, f0) || !in_frame(T, f1)) continue;
        triangulate(P0, P1, p->obs + 2 * (T->obs_off + f0 - T->start_frame), p->obs + 2 * (T->obs_off + f1 - T->start_frame), pos + 3 * j);
        st[j] = 1;
    }
}

static void set_pose(double *P, const double *R, const double *t) {
    for (int a = 0; a < 3; a++) { for (int b = 0; b < 3; b++) P[a * 4 + b] = R[a * 3 + b]; P[a * 4 + 3] = t[a]; }
}

int isvo_sfm(const isv_sfm_problem_t *p, isv_sfm_result_t *res) {
    memset(res, 0, sizeof(*res));
    res->fail_frame = -1;
    res->status = check(p);
    if (res->status != ISV_SFM_OK) return res->status;
    const int nw = p->n_window, nf = p->n_frames, l = p->l, last = nw - 1;
    /* ---- stage 0: checkIMUExcitation ---- */
    {
        const double g0 = (g_quirk_off & 1) ? 1.0 : 0.0;
        double sum_g[3] = {g0, g0, g0};   /* S1: never initialised in the reference; zero here */
        for (int f = 1; f < nf; f++) for (int k = 0; k < 3; k++) sum_g[k] += p->delta_v[3 * f + k] / p->sum_dt[f];
        double aver[3];
        for (int k = 0; k < 3; k++) aver[k] = sum_g[k] * 1.0 / (double)(nf - 1);
        double var = 0;
        for (int f = 1; f < nf; f++) {
            double d[3];
            for (int k = 0; k < 3; k++) d[k] = p->delta_v[3 * f + k] / p->sum_dt[f] - aver[k];
            var += d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        }
        var = sqrt(var / (double)(nf - 1));
        res->excitation_var = var;
        if (var < 0.25) return res->status = ISV_SFM_REFUSED_EXCITATION;
    }
    /* ---- stage 1: construct ---- */
    static int st[NT];
    static double pos[3 * NT];
    double cR[NW][9], ct[NW][3], cq[NW][4], Pose[NW][12];
    memset(st, 0, sizeof(int) * p->n_tracks);
    {
        double ql[4] = {1, 0, 0, 0}, qr[4], qlast[4];
        eq_from_R(p->relative_R, qr);
        eq_mul(ql, qr, qlast);
        eq_inv(ql, cq[l]);
        eq_to_R(cq[l], cR[l]);
        const double zero[3] = {0, 0, 0};
        double v[3];
        mv3(cR[l], zero, v);
        for (int k = 0; k < 3; k++) ct[l][k] = -1.0 * v[k];
        set_pose(Pose[l], cR[l], ct[l]);
        eq_inv(qlast, cq[last]);
        eq_to_R(cq[last], cR[last]);
        mv3(cR[last], p->relative_T, v);
        for (int k = 0; k < 3; k++) ct[last][k] = -1.0 * v[k];
        set_pose(Pose[last], cR[last], ct[last]);
    }
    for (int i = l; i < last; i++) {
        if (i > l) {
            double R[9], t[3];
            memcpy(R, cR[i - 1], sizeof(R)); memcpy(t, ct[i - 1], sizeof(t));
            if (!sfm_pnp(p, st, pos, i, R, t, &res->sfm_pnp_iterations[i], &res->sfm_pnp_points[i])) { res->fail_frame = i; return res->status = ISV_SFM_REFUSED_SFM_PNP_POINTS; }
            memcpy(cR[i], R, sizeof(R)); memcpy(ct[i], t, sizeof(t));
            eq_from_R(cR[i], cq[i]);
            set_pose(Pose[i], cR[i], ct[i]);
        }
        tri_two(p, st, pos, i, Pose[i], last, Pose[last]);
    }
    for (int i = l + 1; i < last; i++) tri_two(p, st, pos, l, Pose[l], i, Pose[i]);
    for (int i = l - 1; i >= 0; i--) {
        double R[9], t[3];
        memcpy(R, cR[i + 1], sizeof(R)); memcpy(t, ct[i + 1], sizeof(t));
        if (!sfm_pnp(p, st, pos, i, R, t, &res->sfm_pnp_iterations[i], &res->sfm_pnp_points[i])) { res->fail_frame = i; return res->status = ISV_SFM_REFUSED_SFM_PNP_POINTS; }
        memcpy(cR[i], R, sizeof(R)); memcpy(ct[i], t, sizeof(t));
        eq_from_R(cR[i], cq[i]);
        set_pose(Pose[i], cR[i], ct[i]);
        tri_two(p, st, pos, i, Pose[i], l, Pose[l]);
    }
    for (int j = 0; j < p->n_tracks; j++) {   /* step 5: first and last observation, no cheirality check (S5) */
        const isv_sfm_track_t *T = &p->tracks[j];
        if (st[j] || T->n_obs < 2) continue;
        const int f0 = T->start_frame, f1 = T->start_frame + T->n_obs - 1;
        triangulate(Pose[f0], Pose[f1], p->obs + 2 * T->obs_off, p->obs + 2 * (T->obs_off + T->n_obs - 1), pos + 3 * j);
        if (g_quirk_off & 8) {
            double z0 = Pose[f0][8] * pos[3 * j] + Pose[f0][9] * pos[3 * j + 1] + Pose[f0][10] * pos[3 * j + 2] + Pose[f0][11];
            double z1 = Pose[f1][8] * pos[3 * j] + Pose[f1][9] * pos[3 * j + 1] + Pose[f1][10] * pos[3 * j + 2] + Pose[f1][11];
            if (!(z0 > 0 && z1 > 0)) continue;
        }
        st[j] = 1;
    }
    /* ---- stage 2: the full BA ---- */
    static int act[NT];
    ba_t B;
    memset(&B, 0, sizeof(B));
    B.nw = nw; B.ntr = p->n_tracks; B.l = l; B.tr = p->tracks; B.obs = p->obs; B.act = act;
    for (int j = 0; j < p->n_tracks; j++) if (st[j]) { act[B.nact++] = j; res->ba_residuals += 2 * p->tracks[j].n_obs; }
    for (int f = 0; f < nw; f++) { B.coff[f] = B.nc; B.ncf[f] = f == l ? 0 : f == last ? 3 : 6; B.nc += B.ncf[f]; }
    res->n_triangulated = B.nact; res->n_ba_cols = B.nc;
    double bq[4 * NW], bt[3 * NW];
    for (int f = 0; f < nw; f++) { for (int k = 0; k < 4; k++) bq[4 * f + k] = cq[f][k]; for (int k = 0; k < 3; k++) bt[3 * f + k] = ct[f][k]; }
    ba_solve(&B, bq, bt, pos, res);
    for (int j = 0; j < p->n_tracks; j++) {
        p->state[j] = st[j];
        for (int k = 0; k < 3; k++) p->position[3 * j + k] = st[j] ? pos[3 * j + k] : 0.0;
    }
    const int conv = res->ba_termination == ISV_TERM_GRADIENT_TOL || res->ba_termination == ISV_TERM_PARAMETER_TOL ||
                     res->ba_termination == ISV_TERM_FUNCTION_TOL || res->ba_termination == ISV_TERM_MIN_RADIUS;
    if (!(conv || res->ba_final_cost < 5e-3)) return res->status = ISV_SFM_REFUSED_BA_NOT_CONVERGED;
    double Q[NW][4], T[NW][3];
    for (int f = 0; f < nw; f++) {   /* q = q.inverse() (S6); T = -(q * t) */
        eq_inv(bq + 4 * f, Q[f]);
        double v[3];
        eq_transform(Q[f], bt + 3 * f, v);
        for (int k = 0; k < 3; k++) T[f][k] = -1.0 * v[k];
        res->Q[f][0] = Q[f][1]; res->Q[f][1] = Q[f][2]; res->Q[f][2] = Q[f][3]; res->Q[f][3] = Q[f][0];
        for (int k = 0; k < 3; k++) res->T[f][k] = T[f][k];
    }
    /* ---- stage 4: the all-frame PnP ---- */
    static double P3[3 * NT], P2[2 * NT];
    for (int f = 0, i = 0; f < nf; f++) {
        if (f == p->window_frame[i]) {
            double R[9], RicT[9];
            eq_to_R(Q[i], R);
            mmT3(R, p->RIC, RicT);
            memcpy(res->R[f], RicT, sizeof(RicT));
            memcpy(res->Tf[f], T[i], 3 * sizeof(double));
            res->is_key_frame[f] = 1;
            i++;
            continue;
        }
        if (f > p->window_frame[i]) i++;   /* S4 (never true on valid input: i already names the next keyframe) */
        const int gi = ((g_quirk_off & 4) && i > 0) ? i - 1 : i;
        double qi[4], Ri[9], Pi[3], rv[3], tv[3];
        eq_inv(Q[gi], qi);
        eq_to_R(qi, Ri);
        mv3(Ri, T[gi], Pi);
        for (int k = 0; k < 3; k++) tv[k] = -Pi[k];
        rodrigues_m2v(Ri, rv);
        int n = 0;
        for (int k = p->pt_off[f]; k < p->pt_off[f + 1]; k++) {   /* ascending feature_id (S8) */
            int j = -1;
            for (int m = 0; m < p->n_tracks; m++) if (p->tracks[m].id == p->pt_id[k]) j = m;   /* map assignment: the last track wins */
            if (j < 0 || !st[j]) continue;
            for (int c = 0; c < 3; c++) P3[3 * n + c] = FR(pos[3 * j + c]);   /* S2 */
            P2[2 * n] = FR(p->pt_uv[2 * k]); P2[2 * n + 1] = FR(p->pt_uv[2 * k + 1]);
            n++;
        }
        res->pnp_points[f] = n;
        if (n < 6) { res->fail_frame = f; return res->status = ISV_SFM_REFUSED_ALL_PNP_POINTS; }   /* S3 */
        res->pnp_iterations[f] = pnp_solve(n, P3, P2, rv, tv);
        double r[9], Rp[9], Tp[3], mt[3];
        rodrigues_v2m(rv, r, NULL);
        for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) Rp[a * 3 + b] = r[b * 3 + a];
        for (int k = 0; k < 3; k++) mt[k] = -tv[k];
        mv3(Rp, mt, Tp);
        mmT3(Rp, p->RIC, res->R[f]);
        memcpy(res->Tf[f], Tp, sizeof(Tp));
        res->is_key_frame[f] = 0;
    }
    return res->status = ISV_SFM_OK;
}

/* unit entry: one observation's residual and its unscaled 2 x 3 Jacobians (quaternion tangent, translation, point); q w x y z */
void isvo_sfm_ba_obs(const double *q, const double *t, const double *X, const double *uv, double *r, double *Jq, double *Jt, double *JX) {
    ba_obs(q, t, X, uv, r, Jq, Jt, JX);
}

int isvo_sfm_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(isv_sfm_track_t);
    case 1: return (int)sizeof(isv_sfm_problem_t);
    case 2: return (int)sizeof(isv_sfm_result_t);
    default: return -1;
    }
}
