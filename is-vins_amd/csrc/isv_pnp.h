/*
 * isv_pnp.h -- OpenCV 3.2's iterative PnP as the initialisation and loop-closure kernels run it (isv_sfm.hip, isv_loop.hip):
 * Rodrigues both ways, cvProjectPoints2 of one point with its 2 x 6 Jacobian, CvLevMarq::step, and Eigen's matrix ->
 * quaternion.  These serial pieces are plain C that compiles as HIP device code or as host C (ISV_HD), so the CPU restatements
 * can include them.  The workgroup form of the CvLevMarq loop (pnp_eval / pnp_solve: 64 lanes, rows staged 64 points at a
 * time, every cross-lane sum on one lane in point order) is device only.  Includers turn FP contraction off.
 */
#ifndef ISV_PNP_H
#define ISV_PNP_H
#include "isv_init_common.h"

#define ISV_PNP_LANES 64

ISV_HD void eq_from_R(const double *m, double *q) {   /* Quaternion(Matrix3d) */
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

/* ---------------- OpenCV 3.2 Rodrigues and the iterative PnP ---------------- */
ISV_HD void rodrigues_v2m(const double *rv, double *R, double *J) {   /* J: 3 x 9 (d R / d r_i), may be NULL */
    double rx = rv[0], ry = rv[1], rz = rv[2];
    double theta = sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < DBL_EPSILON) {
        for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
        if (J) { for (int k = 0; k < 27; k++) J[k] = 0.0; J[5] = J[15] = J[19] = -1; J[7] = J[11] = J[21] = 1; }
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
ISV_HD void rodrigues_m2v(const double *R, double *rv) {   /* (the SVD re-orthonormalisation is dropped: isv_sfm.h) */
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
ISV_HD void pnp_project(const double *R, const double *dRdr, const double *tv, const double *X, const double *m, double *err, double *J) {
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
/* CvLevMarq::step: param = prev - solve_svd(JtJ with diag *= 1 + lambda, JtErr) */
ISV_HD void pnp_step(const double *JtJ, const double *JtE, int lambdaLg10, const double *prev, double *param) {
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

// PnP block (doubles): param 0..5, prev 6..11, JtE 12..17, JtJ 18..53, e2 54
enum { P_PAR = 0, P_PREV = 6, P_JTE = 12, P_JTJ = 18, P_E = 54, P_END = 55 };

#if defined(__HIPCC__)
// ---- OpenCV's iterative PnP on the workgroup: point i at pts + i * stride (X Y Z u v, float-rounded), the
// guess / result in pm[P_PAR..P_PAR+5]; rows staged 64 points at a time in `stage` (64 x 14 doubles) ----
static __device__ double pnp_eval(int n, const double *pts, int stride, double *pm, double *stage, bool wantJ) {
    const int t = threadIdx.x;
    double param[6], R[9], dRdr[27];
    for (int k = 0; k < 6; k++) param[k] = pm[P_PAR + k];
    rodrigues_v2m(param, R, wantJ ? dRdr : nullptr);
    // lanes 0..20: JtJ (a >= b), 21..26: JtErr, 27: |err|^2
    int ea = 0, eb = 0;
    if (t < 21) { while ((ea + 1) * (ea + 2) / 2 <= t) ea++; eb = t - ea * (ea + 1) / 2; }
    double acc = 0;
    for (int c0 = 0; c0 < n; c0 += ISV_PNP_LANES) {
        const int i = c0 + t;
        if (i < n) {
            const double *P = pts + (size_t)i * stride;
            pnp_project(R, dRdr, param + 3, P, P + 3, stage + t * 14, wantJ ? stage + t * 14 + 2 : nullptr);
        }
        __syncthreads();
        const int m = min(ISV_PNP_LANES, n - c0);
        if (t == 27 || (wantJ && t < 27)) {
            for (int ii = 0; ii < m; ii++) {
                const double *e = stage + ii * 14, *J = e + 2;
                for (int r = 0; r < 2; r++) {
                    if (t == 27) acc += e[r] * e[r];
                    else if (t < 21) acc += J[r * 6 + ea] * J[r * 6 + eb];
                    else acc += J[r * 6 + t - 21] * e[r];
                }
            }
        }
        __syncthreads();
    }
    if (t == 27) pm[P_E] = acc;
    else if (wantJ && t < 21) pm[P_JTJ + ea * 6 + eb] = acc;
    else if (wantJ && t < 27) pm[P_JTE + t - 21] = acc;
    __syncthreads();
    return sqrt(pm[P_E]);
}

static __device__ int pnp_solve(int n, const double *pts, int stride, double *pm, double *stage) {
    const int t = threadIdx.x;
    int lambdaLg10 = -3, iters = 0;
    double prevErrNorm = 0, errNorm;
    for (;;) {
        const double e = pnp_eval(n, pts, stride, pm, stage, true);
        if (t == 0) {
            for (int k = 0; k < 6; k++) pm[P_PREV + k] = pm[P_PAR + k];
            pnp_step(pm + P_JTJ, pm + P_JTE, lambdaLg10, pm + P_PREV, pm + P_PAR);
        }
        __syncthreads();
        if (iters == 0) prevErrNorm = e;
        for (;;) {
            errNorm = pnp_eval(n, pts, stride, pm, stage, false);
            if (errNorm > prevErrNorm && ++lambdaLg10 <= 16) {
                if (t == 0) pnp_step(pm + P_JTJ, pm + P_JTE, lambdaLg10, pm + P_PREV, pm + P_PAR);
                __syncthreads();
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
    __syncthreads();
    return iters;
}
#endif /* __HIPCC__ */

#endif /* ISV_PNP_H */
