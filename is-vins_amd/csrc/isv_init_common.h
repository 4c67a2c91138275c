/*
 * isv_init_common.h -- serial pieces shared by the initialisation kernels (isv_sfm.hip, isv_relpose.hip), the loop-closure
 * kernel (isv_loop.hip) and the CPU restatements of the relative-pose stage and of the loop verification
 * (tests/native/isv_relpose_oracle.c, tests/native/isv_loop_oracle.c).  Plain C that compiles as HIP device code
 * (ISV_HD) or as host C.  Every includer turns FP contraction off for its whole translation unit (#pragma clang fp
 * contract(off) in the kernels, gcc -ffp-contract=off for the restatement): the operations below then round the same way on
 * both sides, and only the device and host libm (sqrt is exact; acos / cos / pow / log) can round apart.
 *
 *   svd_jacobi            Eigen 3.3 JacobiSVD of a square matrix (two-sided 2 x 2 Jacobi sweeps, no QR preconditioner)
 *   eig_jacobi_sym        cyclic Jacobi eigen-decomposition of a symmetric matrix (EPnP's M^T M, the DLT's L^T L: isv_loop_common.h)
 *   isv_excitation_var    Estimator::checkIMUExcitation's var (src/estimator.cpp:213-238), the first stage of both kernels
 *   rp_*                  the relative-pose RANSAC (isv_relpose.h): OpenCV 3.2's cv::RNG, RANSACPointSetRegistrator's
 *                         getSubset and RANSACUpdateNumIters, fundam.cpp's run7Point / computeError, cv::solveCubic,
 *                         cvTriangulatePoints (rp_triangulate, which the rotation calibration's testTriangulation shares:
 *                         isv_exrot.h) and the reference's own decomposeEssentialMat / recoverPose cheirality test
 *                         (src/initial/solve_5pts.cpp).  Restated from the published OpenCV 3.2 sources; the restatement pins
 *                         the GPU, not the reference.
 */
#ifndef ISV_INIT_COMMON_H
#define ISV_INIT_COMMON_H
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ISV_HD static __device__
#else
#define ISV_HD static
#endif

/* ---------------- Eigen 3.3 JacobiSVD, square n x n (n <= 9), no QR preconditioner ---------------- */
/* A row-major, overwritten; w: singular values (sorted, descending); U (may be NULL), V: n x n row-major */
ISV_HD void svd_jacobi(int n, double *A, double *w, double *U, double *V) {
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


/* ---------------- symmetric eigen-decomposition, cyclic Jacobi (n <= 12) ---------------- */
/* A row-major symmetric, overwritten; w: eigenvalues, descending (first on ties); V: n x n row-major, COLUMN k the eigenvector
 * of w[k].  A rotation is skipped when |A_pq| <= 2 eps max|A_ii| (the largest diagonal seen so far, as svd_jacobi does), so a
 * null space comes out as whatever orthonormal basis the sweeps leave. */
ISV_HD void eig_jacobi_sym(int n, double *A, double *w, double *V) {
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) V[i * n + j] = i == j ? 1.0 : 0.0;
    double maxDiag = 0;
    for (int i = 0; i < n; i++) maxDiag = fabs(A[i * n + i]) > maxDiag ? fabs(A[i * n + i]) : maxDiag;
    int finished = 0;
    for (int sweep = 0; !finished && sweep < 64; sweep++) {
        finished = 1;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                const double apq = A[p * n + q];
                const double thr = 2.0 * DBL_EPSILON * maxDiag > DBL_MIN ? 2.0 * DBL_EPSILON * maxDiag : DBL_MIN;
                if (!(fabs(apq) > thr)) continue;
                finished = 0;
                const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
                for (int k = 0; k < n; k++) {   /* A <- A J */
                    const double x = A[k * n + p], y = A[k * n + q];
                    A[k * n + p] = c * x - s * y; A[k * n + q] = s * x + c * y;
                }
                for (int k = 0; k < n; k++) {   /* A <- J^T A */
                    const double x = A[p * n + k], y = A[q * n + k];
                    A[p * n + k] = c * x - s * y; A[q * n + k] = s * x + c * y;
                }
                for (int k = 0; k < n; k++) {   /* V <- V J */
                    const double x = V[k * n + p], y = V[k * n + q];
                    V[k * n + p] = c * x - s * y; V[k * n + q] = s * x + c * y;
                }
                const double ap = fabs(A[p * n + p]), aq = fabs(A[q * n + q]), mx = ap > aq ? ap : aq;
                maxDiag = maxDiag > mx ? maxDiag : mx;
            }
    }
    for (int i = 0; i < n; i++) w[i] = A[i * n + i];
    for (int i = 0; i < n; i++) {
        int pos = i;
        for (int k = i + 1; k < n; k++) if (w[k] > w[pos]) pos = k;
        if (pos != i) {
            const double tw = w[i]; w[i] = w[pos]; w[pos] = tw;
            for (int k = 0; k < n; k++) { const double tv = V[k * n + i]; V[k * n + i] = V[k * n + pos]; V[k * n + pos] = tv; }
        }
    }
}

/* checkIMUExcitation: the spread of delta_v / sum_dt over all_image_frame's entries 1 .. nf-1 (dv [nf][3], sdt [nf]) */
ISV_HD double isv_excitation_var(int nf, const double *dv, const double *sdt) {
    double sum_g[3] = {0, 0, 0};   /* S1: never initialised in the reference; zero here */
    for (int f = 1; f < nf; f++) for (int k = 0; k < 3; k++) sum_g[k] += dv[3 * f + k] / sdt[f];
    double aver[3];
    for (int k = 0; k < 3; k++) aver[k] = sum_g[k] * 1.0 / (double)(nf - 1);
    double var = 0;
    for (int f = 1; f < nf; f++) {
        double d[3];
        for (int k = 0; k < 3; k++) d[k] = dv[3 * f + k] / sdt[f] - aver[k];
        var += d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    }
    return sqrt(var / (double)(nf - 1));
}

/* ---------------- the relative-pose RANSAC (isv_relpose.h, quirks R1..R5) ---------------- */
#define RP_MAX_ITERS 1000
#define RP_CONFIDENCE 0.99
#define RP_THRESH (0.3 / 460)

/* cv::RNG::next + uniform(0, n): state = (uint64)(unsigned)state * 4164903690U + (unsigned)(state >> 32) */
ISV_HD uint32_t rp_uniform(uint64_t *state, uint32_t n) {
    uint64_t s = *state;
    s = (uint64_t)(uint32_t)s * 4164903690U + (uint32_t)(s >> 32);
    *state = s;
    return (uint32_t)s % n;
}

/* RANSACPointSetRegistrator::getSubset for m points: distinct indices, a repeated draw is drawn again.  Neither 3.2's
 * FMEstimatorCallback (m = 7) nor its PnPRansacCallback (m = 5) overrides checkSubset (no collinearity test) and
 * checkPartialSubsets is false, so one subset is exactly its draws. */
ISV_HD void rp_subset_m(uint64_t *state, int count, int m, int *idx) {
    for (int i = 0; i < m; i++)
        for (;;) {
            const int v = (int)rp_uniform(state, (uint32_t)count);
            int j = 0;
            while (j < i && idx[j] != v) j++;
            if (j == i) { idx[i] = v; break; }
        }
}
ISV_HD void rp_subset(uint64_t *state, int count, int *idx) { rp_subset_m(state, count, 7, idx); }

/* RANSACUpdateNumIters(p, ep, modelPoints, maxIters); cvRound is round-half-even (rint) */
ISV_HD int rp_update_num_iters(double p, double ep, int model_points, int max_iters) {
    p = p > 0. ? p : 0.; p = p < 1. ? p : 1.;
    ep = ep > 0. ? ep : 0.; ep = ep < 1. ? ep : 1.;
    double num = 1. - p > DBL_MIN ? 1. - p : DBL_MIN;
    double denom = 1. - pow(1. - ep, (double)model_points);
    if (denom < DBL_MIN) return 0;
    num = log(num);
    denom = log(denom);
    return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)rint(num / denom);
}

/* cv::solveCubic on c[0] x^3 + c[1] x^2 + c[2] x + c[3]; returns the root count (-1: every x), roots in r[0..2] */
ISV_HD int rp_solve_cubic(const double *c, double *r) {
    double a0 = c[0], a1 = c[1], a2 = c[2], a3 = c[3];
    double x0 = 0., x1 = 0., x2 = 0.;
    int n = 0;
    if (a0 == 0) {
        if (a1 == 0) {
            if (a2 == 0) n = a3 == 0 ? -1 : 0;
            else { x0 = -a3 / a2; n = 1; }   /* linear */
        } else {                              /* quadratic */
            double d = a2 * a2 - 4 * a1 * a3;
            if (d >= 0) {
                d = sqrt(d);
                double q = (-a2 + (a2 < 0 ? -d : d)) * 0.5;
                x0 = q / a1;
                x1 = a3 / q;
                n = d > 0 ? 2 : 1;
            }
        }
    } else {
        a0 = 1. / a0;
        a1 *= a0; a2 *= a0; a3 *= a0;
        double Q = (a1 * a1 - 3 * a2) * (1. / 9);
        double R = (2 * a1 * a1 * a1 - 9 * a1 * a2 + 27 * a3) * (1. / 54);
        double Qcubed = Q * Q * Q;
        double d = Qcubed - R * R;
        if (d >= 0) {                         /* three real roots */
            double theta = acos(R / sqrt(Qcubed));
            double sqrtQ = sqrt(Q);
            double t0 = -2 * sqrtQ, t1 = theta * (1. / 3), t2 = a1 * (1. / 3);
            x0 = t0 * cos(t1) - t2;
            x1 = t0 * cos(t1 + (2. * 3.1415926535897932384626433832795 / 3)) - t2;
            x2 = t0 * cos(t1 + (4. * 3.1415926535897932384626433832795 / 3)) - t2;
            n = 3;
        } else {                              /* one real root */
            double e;
            d = sqrt(-d);
            e = pow(d + fabs(R), 0.333333333333);
            if (R > 0) e = -e;
            x0 = (e + Q / e) - a1 * (1. / 3);
            n = 1;
        }
    }
    r[0] = x0; r[1] = x1; r[2] = x2;
    return n;
}

/* fundam.cpp run7Point: p [7][4] = (x0, y0, x1, y1) per correspondence (m1 = x0 y0, m2 = x1 y1), F [3][9] row-major; returns
 * the model count (solveCubic's; outside 1..3 no model).  Deviation: the 7 x 9 system's null space comes from svd_jacobi of
 * the system padded with two zero rows, not OpenCV's one-sided SVD; the roots do not depend on the basis up to rounding. */
ISV_HD int rp_run7point(const double *p, double *F) {
    double a[81], w[9], v[81], c[4], r[3], f1[9], f2[9];
    for (int i = 0; i < 7; i++) {
        const double x0 = p[4 * i], y0 = p[4 * i + 1], x1 = p[4 * i + 2], y1 = p[4 * i + 3];
        double *ai = a + 9 * i;
        ai[0] = x1 * x0; ai[1] = x1 * y0; ai[2] = x1; ai[3] = y1 * x0; ai[4] = y1 * y0; ai[5] = y1; ai[6] = x0; ai[7] = y0; ai[8] = 1;
    }
    for (int k = 63; k < 81; k++) a[k] = 0.0;
    svd_jacobi(9, a, w, 0, v);
    for (int i = 0; i < 9; i++) { f1[i] = v[i * 9 + 7]; f2[i] = v[i * 9 + 8]; }
    for (int i = 0; i < 9; i++) f1[i] -= f2[i];
    double t0 = f2[4] * f2[8] - f2[5] * f2[7];
    double t1 = f2[3] * f2[8] - f2[5] * f2[6];
    double t2 = f2[3] * f2[7] - f2[4] * f2[6];
    c[3] = f2[0] * t0 - f2[1] * t1 + f2[2] * t2;
    c[2] = f1[0] * t0 - f1[1] * t1 + f1[2] * t2 -
           f1[3] * (f2[1] * f2[8] - f2[2] * f2[7]) +
           f1[4] * (f2[0] * f2[8] - f2[2] * f2[6]) -
           f1[5] * (f2[0] * f2[7] - f2[1] * f2[6]) +
           f1[6] * (f2[1] * f2[5] - f2[2] * f2[4]) -
           f1[7] * (f2[0] * f2[5] - f2[2] * f2[3]) +
           f1[8] * (f2[0] * f2[4] - f2[1] * f2[3]);
    t0 = f1[4] * f1[8] - f1[5] * f1[7];
    t1 = f1[3] * f1[8] - f1[5] * f1[6];
    t2 = f1[3] * f1[7] - f1[4] * f1[6];
    c[1] = f2[0] * t0 - f2[1] * t1 + f2[2] * t2 -
           f2[3] * (f1[1] * f1[8] - f1[2] * f1[7]) +
           f2[4] * (f1[0] * f1[8] - f1[2] * f1[6]) -
           f2[5] * (f1[0] * f1[7] - f1[1] * f1[6]) +
           f2[6] * (f1[1] * f1[5] - f1[2] * f1[4]) -
           f2[7] * (f1[0] * f1[5] - f1[2] * f1[3]) +
           f2[8] * (f1[0] * f1[4] - f1[1] * f1[3]);
    c[0] = f1[0] * t0 - f1[1] * t1 + f1[2] * t2;
    const int n = rp_solve_cubic(c, r);
    if (n < 1 || n > 3) return n;
    for (int k = 0; k < n; k++) {
        double *fm = F + 9 * k;
        double lambda = r[k], mu = 1.;
        const double s = f1[8] * r[k] + f2[8];
        if (fabs(s) > DBL_EPSILON) {   /* F(3,3) = 1 */
            mu = 1. / s;
            lambda *= mu;
            fm[8] = 1.;
        } else fm[8] = 0.;
        for (int i = 0; i < 8; i++) fm[i] = f1[i] * lambda + f2[i] * mu;
    }
    return n;
}

/* FMEstimatorCallback::computeError of one correspondence (before its float32 store, R2) */
ISV_HD double rp_fm_error(const double *F, double x0, double y0, double x1, double y1) {
    double a, b, c, d1, d2, s1, s2;
    a = F[0] * x0 + F[1] * y0 + F[2];
    b = F[3] * x0 + F[4] * y0 + F[5];
    c = F[6] * x0 + F[7] * y0 + F[8];
    s2 = 1. / (a * a + b * b);
    d2 = x1 * a + y1 * b + c;
    a = F[0] * x1 + F[3] * y1 + F[6];
    b = F[1] * x1 + F[4] * y1 + F[7];
    c = F[2] * x1 + F[5] * y1 + F[8];
    s1 = 1. / (a * a + b * b);
    d1 = x0 * a + y0 * b + c;
    const double e1 = d1 * d1 * s1, e2 = d2 * d2 * s2;
    return e1 < e2 ? e2 : e1;   /* std::max(e1, e2) */
}

ISV_HD double rp_det3(const double *m) {   /* cv::determinant, 3 x 3 */
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

/* solve_5pts.cpp decomposeEssentialMat: E row-major -> the 3 x 4 cameras [R1 | t], [R2 | t], [R1 | -t], [R2 | -t] (P [4][12]) */
ISV_HD void rp_decompose(const double *E, double *P) {
    double A[9], w[3], U[9], V[9], Vt[9], UW[9], UWt[9], R1[9], R2[9];
    for (int k = 0; k < 9; k++) A[k] = E[k];
    svd_jacobi(3, A, w, U, V);
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) Vt[a * 3 + b] = V[b * 3 + a];
    if (rp_det3(U) < 0) for (int k = 0; k < 9; k++) U[k] *= -1.;
    if (rp_det3(Vt) < 0) for (int k = 0; k < 9; k++) Vt[k] *= -1.;
    const double W[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            UW[a * 3 + b] = U[a * 3] * W[b] + U[a * 3 + 1] * W[3 + b] + U[a * 3 + 2] * W[6 + b];
            UWt[a * 3 + b] = U[a * 3] * W[3 * b] + U[a * 3 + 1] * W[3 * b + 1] + U[a * 3 + 2] * W[3 * b + 2];
        }
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            R1[a * 3 + b] = UW[a * 3] * Vt[b] + UW[a * 3 + 1] * Vt[3 + b] + UW[a * 3 + 2] * Vt[6 + b];
            R2[a * 3 + b] = UWt[a * 3] * Vt[b] + UWt[a * 3 + 1] * Vt[3 + b] + UWt[a * 3 + 2] * Vt[6 + b];
        }
    for (int s = 0; s < 4; s++)
        for (int a = 0; a < 3; a++) {
            const double *R = (s & 1) ? R2 : R1;
            for (int b = 0; b < 3; b++) P[12 * s + a * 4 + b] = R[a * 3 + b];
            P[12 * s + a * 4 + 3] = (s < 2 ? 1.0 : -1.0) * (U[a * 3 + 2] * 1.0);
        }
}

/* cvTriangulatePoints of one correspondence against camera P (3 x 4, the other is [I | 0]): the 6 x 4 system (three rows per
 * view) and its last right singular vector Q = (X Y Z W).  Deviation: the right singular vectors come from a Householder QR of
 * the 6 x 4 system and svd_jacobi of its 4 x 4 R factor (as Eigen's QR-preconditioned JacobiSVD), not OpenCV's one-sided SVD. */
ISV_HD void rp_triangulate(const double *P, double x0, double y0, double x1, double y1, double *Q) {
    const double P0[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    double A[24], Rm[16], w[4], V[16];
    for (int j = 0; j < 2; j++) {
        const double *M = j ? P : P0;
        const double x = j ? x1 : x0, y = j ? y1 : y0;
        for (int k = 0; k < 4; k++) {
            A[(j * 3 + 0) * 4 + k] = x * M[8 + k] - M[k];
            A[(j * 3 + 1) * 4 + k] = y * M[8 + k] - M[4 + k];
            A[(j * 3 + 2) * 4 + k] = x * M[4 + k] - y * M[k];
        }
    }
    for (int k = 0; k < 4; k++) {   /* Householder QR, column k */
        double nx = 0;
        for (int i = k; i < 6; i++) nx += A[i * 4 + k] * A[i * 4 + k];
        nx = sqrt(nx);
        if (nx == 0.0) continue;
        const double alpha = A[k * 4 + k] > 0 ? -nx : nx;
        double v[6];
        for (int i = k; i < 6; i++) v[i] = A[i * 4 + k];
        v[k] -= alpha;
        double vv = 0;
        for (int i = k; i < 6; i++) vv += v[i] * v[i];
        if (vv == 0.0) continue;
        for (int c = k; c < 4; c++) {
            double s = 0;
            for (int i = k; i < 6; i++) s += v[i] * A[i * 4 + c];
            s = 2.0 * s / vv;
            for (int i = k; i < 6; i++) A[i * 4 + c] -= s * v[i];
        }
    }
    for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) Rm[a * 4 + b] = b >= a ? A[a * 4 + b] : 0.0;
    svd_jacobi(4, Rm, w, 0, V);
    Q[0] = V[3]; Q[1] = V[7]; Q[2] = V[11]; Q[3] = V[15];
}

/* recoverPose's cheirality test of one correspondence against camera P: the triangulated Q, then Z W > 0, Z / W < dist and
 * 0 < (P Q / W).z < dist */
ISV_HD int rp_cheirality(const double *P, double x0, double y0, double x1, double y1) {
    double Q[4];
    rp_triangulate(P, x0, y0, x1, y1, Q);
    const double X = Q[0], Y = Q[1], Z = Q[2], Wh = Q[3];
    const double dist = 50.0;
    int ok = Z * Wh > 0;
    const double Xn = X / Wh, Yn = Y / Wh, Zn = Z / Wh, Wn = Wh / Wh;
    ok = (Zn < dist) & ok;
    const double z = P[8] * Xn + P[9] * Yn + P[10] * Zn + P[11] * Wn;
    ok = (z > 0) & ok;
    ok = (z < dist) & ok;
    return ok;
}

#endif /* ISV_INIT_COMMON_H */
