/*
 * isv_loop_common.h -- serial pieces of the loop-closure verification (include/isvins_loop.h has the contract, the reference
 * lines, the quirks L1..L6 and the deviations), shared by the kernel k_loop_pnp (isv_loop.hip) and its CPU restatement
 * (tests/native/isv_loop_oracle.c).  Plain C that compiles as HIP device code or as host C (ISV_HD); every includer turns FP
 * contraction off, so both sides round the same way and only libm (cos / sin / acos / atan2 / exp / log / pow) can round apart.
 *
 *   lp_epnp            OpenCV 3.2 epnp.cpp (epnp::compute_pose) on n points, K = I
 *   lp_ransac_*        PnPRansacCallback: runKernel (EPnP on five points, Rodrigues) and computeError
 *   lp_dlt_*           cvFindExtrinsicCameraParams2's planarity test and non-planar DLT initialisation (calibration.cpp)
 *   lp_old_pose / lp_weight_term / lp_finish      keyframe.cpp:200-227 and :274-292
 * Restated from the published OpenCV 3.2.0 sources; the restatement pins the GPU, not OpenCV.
 */
#ifndef ISV_LOOP_COMMON_H
#define ISV_LOOP_COMMON_H
#include "../../include/isvins_loop.h"
#include "isv_pnp.h"

/* the restatement's quirk hooks (bit k - 1 switches Lk off); the kernels compile with every quirk on */
#ifndef LP_QUIRKS_OFF
#define LP_QUIRKS_OFF 0
#endif
#define LP_OFF(k) ((LP_QUIRKS_OFF >> ((k) - 1)) & 1)

/* a matched point as the PnP reads it (L5: float32): the 3-D point, the matched old corner, the window point it came from */
typedef struct lp_match { float X[3], uv[2]; int32_t src; } lp_match_t;
#define LP_PT 5   /* doubles of a point of the final solve: X Y Z u v */

ISV_HD int lp_finite(const double *v, int n) {
    for (int k = 0; k < n; k++) if (!(v[k] - v[k] == 0.0)) return 0;
    return 1;
}
ISV_HD void lp_inv3(const double *m, double *o) {
    const double c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
    const double id = 1.0 / (m[0] * c0 + m[1] * c1 + m[2] * c2);
    o[0] = c0 * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    o[3] = c1 * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    o[6] = c2 * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}
/* least squares min |A x - b| by Householder QR: A m x n row-major (m <= 6, n <= 5), A and b overwritten; a zero pivot gives x_k = 0 */
ISV_HD void lp_ls_qr(int m, int n, double *A, double *b, double *x) {
    for (int k = 0; k < n; k++) {
        double nx = 0;
        for (int i = k; i < m; i++) nx += A[i * n + k] * A[i * n + k];
        nx = sqrt(nx);
        if (nx == 0.0) continue;
        const double alpha = A[k * n + k] > 0 ? -nx : nx;
        double v[6];
        for (int i = k; i < m; i++) v[i] = A[i * n + k];
        v[k] -= alpha;
        double vv = 0;
        for (int i = k; i < m; i++) vv += v[i] * v[i];
        if (vv == 0.0) continue;
        for (int c = k; c < n; c++) {
            double s = 0;
            for (int i = k; i < m; i++) s += v[i] * A[i * n + c];
            s = 2.0 * s / vv;
            for (int i = k; i < m; i++) A[i * n + c] -= s * v[i];
        }
        double s = 0;
        for (int i = k; i < m; i++) s += v[i] * b[i];
        s = 2.0 * s / vv;
        for (int i = k; i < m; i++) b[i] -= s * v[i];
    }
    for (int k = n - 1; k >= 0; k--) {
        double s = b[k];
        for (int j = k + 1; j < n; j++) s -= A[k * n + j] * x[j];
        x[k] = A[k * n + k] != 0.0 ? s / A[k * n + k] : 0.0;
    }
}

/* ---------------- EPnP (epnp.cpp), K = I: fu = fv = 1, uc = vc = 0 ---------------- */
/* the barycentric coordinates of X (compute_barycentric_coordinates) */
ISV_HD void lp_epnp_alpha(const double *cws, const double *CCi, const double *X, double *a) {
    const double d[3] = {X[0] - cws[0], X[1] - cws[1], X[2] - cws[2]};
    for (int j = 0; j < 3; j++) a[1 + j] = CCi[3 * j] * d[0] + CCi[3 * j + 1] * d[1] + CCi[3 * j + 2] * d[2];
    a[0] = 1.0 - a[1] - a[2] - a[3];
}
/* compute_ccs / compute_pcs / solve_for_sign / estimate_R_and_t / reprojection_error for one set of betas; vv [4][12] are the
 * eigenvectors of the four smallest eigenvalues, smallest first */
ISV_HD double lp_epnp_Rt(int n, const double *X, const double *uv, const double *cws, const double *CCi, const double *vv, const double *betas,
                         double *R, double *t) {
    double ccs[12], a[4], pc[3];
    for (int k = 0; k < 12; k++) ccs[k] = 0.0;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
            for (int k = 0; k < 3; k++) ccs[3 * j + k] += betas[i] * vv[12 * i + 3 * j + k];
    /* solve_for_sign: the first point's depth */
    lp_epnp_alpha(cws, CCi, X, a);
    double z0 = a[0] * ccs[2] + a[1] * ccs[5] + a[2] * ccs[8] + a[3] * ccs[11];
    if (z0 < 0.0) for (int k = 0; k < 12; k++) ccs[k] = -ccs[k];
    double pc0[3] = {0, 0, 0}, pw0[3] = {0, 0, 0};
    for (int i = 0; i < n; i++) {
        lp_epnp_alpha(cws, CCi, X + 3 * i, a);
        for (int k = 0; k < 3; k++) {
            pc[k] = a[0] * ccs[k] + a[1] * ccs[3 + k] + a[2] * ccs[6 + k] + a[3] * ccs[9 + k];
            pc0[k] += pc[k]; pw0[k] += X[3 * i + k];
        }
    }
    for (int k = 0; k < 3; k++) { pc0[k] /= n; pw0[k] /= n; }
    double abt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, w[3], U[9], V[9];
    for (int i = 0; i < n; i++) {
        lp_epnp_alpha(cws, CCi, X + 3 * i, a);
        for (int k = 0; k < 3; k++) pc[k] = a[0] * ccs[k] + a[1] * ccs[3 + k] + a[2] * ccs[6 + k] + a[3] * ccs[9 + k];
        for (int j = 0; j < 3; j++)
            for (int k = 0; k < 3; k++) abt[3 * j + k] += (pc[j] - pc0[j]) * (X[3 * i + k] - pw0[k]);
    }
    svd_jacobi(3, abt, w, U, V);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1] + U[3 * i + 2] * V[3 * j + 2];
    if (rp_det3(R) < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
    for (int k = 0; k < 3; k++) t[k] = pc0[k] - (R[3 * k] * pw0[0] + R[3 * k + 1] * pw0[1] + R[3 * k + 2] * pw0[2]);
    double sum = 0;   /* reprojection_error */
    for (int i = 0; i < n; i++) {
        const double *P = X + 3 * i;
        const double Xc = R[0] * P[0] + R[1] * P[1] + R[2] * P[2] + t[0], Yc = R[3] * P[0] + R[4] * P[1] + R[5] * P[2] + t[1];
        const double iz = 1.0 / (R[6] * P[0] + R[7] * P[1] + R[8] * P[2] + t[2]);
        const double du = uv[2 * i] - Xc * iz, dv = uv[2 * i + 1] - Yc * iz;
        sum += sqrt(du * du + dv * dv);
    }
    return sum / n;
}
/* gauss_newton: five iterations on the four betas (compute_A_and_b_gauss_newton, the 6 x 4 system by Householder QR) */
ISV_HD void lp_epnp_gauss_newton(const double *L, const double *rho, double *b) {
    for (int it = 0; it < 5; it++) {
        double A[24], r[6], x[4];
        for (int i = 0; i < 6; i++) {
            const double *l = L + 10 * i;
            A[4 * i + 0] = 2 * l[0] * b[0] + l[1] * b[1] + l[3] * b[2] + l[6] * b[3];
            A[4 * i + 1] = l[1] * b[0] + 2 * l[2] * b[1] + l[4] * b[2] + l[7] * b[3];
            A[4 * i + 2] = l[3] * b[0] + l[4] * b[1] + 2 * l[5] * b[2] + l[8] * b[3];
            A[4 * i + 3] = l[6] * b[0] + l[7] * b[1] + l[8] * b[2] + 2 * l[9] * b[3];
            r[i] = rho[i] - (l[0] * b[0] * b[0] + l[1] * b[0] * b[1] + l[2] * b[1] * b[1] + l[3] * b[0] * b[2] + l[4] * b[1] * b[2] +
                             l[5] * b[2] * b[2] + l[6] * b[0] * b[3] + l[7] * b[1] * b[3] + l[8] * b[2] * b[3] + l[9] * b[3] * b[3]);
        }
        lp_ls_qr(6, 4, A, r, x);
        for (int k = 0; k < 4; k++) b[k] += x[k];
    }
}
/* epnp::compute_pose on n >= 4 points: X [n][3], uv [n][2] -> R (row-major), t.  work: 288 doubles (M^T M and its eigenvectors). */
ISV_HD void lp_epnp(int n, const double *X, const double *uv, double *R, double *t, double *work) {
    double cws[12], CC[9], CCi[9], w3[3], V3[9], a[4];
    /* choose_control_points: the centroid, then the principal axes scaled by sqrt(eigenvalue / n) */
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
    for (int i = 0; i < 3; i++)
        for (int j = 1; j < 4; j++) CC[3 * i + j - 1] = cws[3 * j + i] - cws[i];
    lp_inv3(CC, CCi);
    /* fill_M and M^T M (lower triangle, then mirrored) */
    double *MtM = work, *V = work + 144;
    for (int k = 0; k < 144; k++) MtM[k] = 0.0;
    for (int i = 0; i < n; i++) {
        double r0[12], r1[12];
        lp_epnp_alpha(cws, CCi, X + 3 * i, a);
        for (int j = 0; j < 4; j++) {
            r0[3 * j] = a[j]; r0[3 * j + 1] = 0.0; r0[3 * j + 2] = a[j] * (0.0 - uv[2 * i]);
            r1[3 * j] = 0.0; r1[3 * j + 1] = a[j]; r1[3 * j + 2] = a[j] * (0.0 - uv[2 * i + 1]);
        }
        for (int p = 0; p < 12; p++)
            for (int q = 0; q <= p; q++) { MtM[12 * p + q] += r0[p] * r0[q]; MtM[12 * p + q] += r1[p] * r1[q]; }
    }
    for (int p = 0; p < 12; p++) for (int q = 0; q < p; q++) MtM[12 * q + p] = MtM[12 * p + q];
    double w12[12], vv[48];
    eig_jacobi_sym(12, MtM, w12, V);
    for (int i = 0; i < 4; i++) for (int k = 0; k < 12; k++) vv[12 * i + k] = V[12 * k + (11 - i)];
    /* compute_L_6x10, compute_rho */
    double L[60], rho[6], dv[4][6][3];
    {
        for (int i = 0; i < 4; i++) {
            int p = 0, q = 1;
            for (int j = 0; j < 6; j++) {
                for (int k = 0; k < 3; k++) dv[i][j][k] = vv[12 * i + 3 * p + k] - vv[12 * i + 3 * q + k];
                q++;
                if (q > 3) { p++; q = p + 1; }
            }
        }
        int p = 0, q = 1;
        for (int i = 0; i < 6; i++) {
            double *row = L + 10 * i;
#define LP_DOT(x, y) (dv[x][i][0] * dv[y][i][0] + dv[x][i][1] * dv[y][i][1] + dv[x][i][2] * dv[y][i][2])
            row[0] = LP_DOT(0, 0); row[1] = 2.0 * LP_DOT(0, 1); row[2] = LP_DOT(1, 1); row[3] = 2.0 * LP_DOT(0, 2); row[4] = 2.0 * LP_DOT(1, 2);
            row[5] = LP_DOT(2, 2); row[6] = 2.0 * LP_DOT(0, 3); row[7] = 2.0 * LP_DOT(1, 3); row[8] = 2.0 * LP_DOT(2, 3); row[9] = LP_DOT(3, 3);
#undef LP_DOT
            const double d0 = cws[3 * p] - cws[3 * q], d1 = cws[3 * p + 1] - cws[3 * q + 1], d2 = cws[3 * p + 2] - cws[3 * q + 2];
            rho[i] = d0 * d0 + d1 * d1 + d2 * d2;
            q++;
            if (q > 3) { p++; q = p + 1; }
        }
    }
    /* find_betas_approx_1 / _2 / _3, each refined and scored; the lowest reprojection error wins (N = 1, then 2, then 3) */
    double best = 0;
    for (int N = 1; N <= 3; N++) {
        const int nc = N == 1 ? 4 : N == 2 ? 3 : 5;
        const int col1[4] = {0, 1, 3, 6};
        double A[30], r[6], x[5], b[4], Rn[9], tn[3];
        for (int i = 0; i < 6; i++) {
            for (int c = 0; c < nc; c++) A[nc * i + c] = L[10 * i + (N == 1 ? col1[c] : c)];
            r[i] = rho[i];
        }
        lp_ls_qr(6, nc, A, r, x);
        if (N == 1) {
            if (x[0] < 0) { b[0] = sqrt(-x[0]); b[1] = -x[1] / b[0]; b[2] = -x[2] / b[0]; b[3] = -x[3] / b[0]; }
            else { b[0] = sqrt(x[0]); b[1] = x[1] / b[0]; b[2] = x[2] / b[0]; b[3] = x[3] / b[0]; }
        } else {
            if (x[0] < 0) { b[0] = sqrt(-x[0]); b[1] = x[2] < 0 ? sqrt(-x[2]) : 0.0; }
            else { b[0] = sqrt(x[0]); b[1] = x[2] > 0 ? sqrt(x[2]) : 0.0; }
            if (x[1] < 0) b[0] = -b[0];
            b[2] = N == 3 ? x[3] / b[0] : 0.0;
            b[3] = 0.0;
        }
        lp_epnp_gauss_newton(L, rho, b);
        const double e = lp_epnp_Rt(n, X, uv, cws, CCi, vv, b, Rn, tn);
        if (N == 1 || e < best) {
            best = e;
            for (int k = 0; k < 9; k++) R[k] = Rn[k];
            for (int k = 0; k < 3; k++) t[k] = tn[k];
        }
    }
}

/* ---------------- PnPRansacCallback (solvepnp.cpp) ---------------- */
/* runKernel: EPnP on the subset's five points (L4: the guess is ignored), then Rodrigues; model = rvec, tvec.  0: a non-finite
 * model (no inliers). */
ISV_HD int lp_ransac_model(const lp_match_t *pts, const int *idx, double *model, double *work) {
    double X[15], uv[10], R[9];
    for (int k = 0; k < 5; k++) {
        const lp_match_t *m = pts + idx[k];
        for (int c = 0; c < 3; c++) X[3 * k + c] = m->X[c];
        uv[2 * k] = m->uv[0]; uv[2 * k + 1] = m->uv[1];
    }
    lp_epnp(5, X, uv, R, model + 3, work);
    rodrigues_m2v(R, model);
    return lp_finite(model, 6);
}
/* computeError of one point against R, t: projectPoints into float32, the squared float32 distance (L5) */
ISV_HD double lp_point_error(const double *R, const double *t, const lp_match_t *m) {
    const double x0 = R[0] * m->X[0] + R[1] * m->X[1] + R[2] * m->X[2] + t[0];
    const double y0 = R[3] * m->X[0] + R[4] * m->X[1] + R[5] * m->X[2] + t[1];
    double z = R[6] * m->X[0] + R[7] * m->X[1] + R[8] * m->X[2] + t[2];
    z = z ? 1. / z : 1;
    if (LP_OFF(5)) {
        const double dx = m->uv[0] - x0 * z, dy = m->uv[1] - y0 * z;
        return dx * dx + dy * dy;
    }
    const float px = (float)(x0 * z), py = (float)(y0 * z);
    const float dx = m->uv[0] - px, dy = m->uv[1] - py;
    const float e = dx * dx + dy * dy;
    return (double)e;
}
/* findInliers' test: the float32 error against the float32 squared threshold tf (as k_relpose's R2; td: the same in doubles) */
ISV_HD int lp_is_inlier(const double *R, const double *t, const lp_match_t *m, float tf, double td) {
    const double e = lp_point_error(R, t, m);
    return LP_OFF(5) ? e <= td : (float)e <= tf;
}
ISV_HD int lp_count_inliers(const double *model, int n, const lp_match_t *pts, float tf, double td) {
    double R[9];
    rodrigues_v2m(model, R, 0);
    int g = 0;
    for (int j = 0; j < n; j++) g += lp_is_inlier(R, model + 3, pts + j, tf, td);
    return g;
}

/* ---------------- cvFindExtrinsicCameraParams2 (calibration.cpp): the initialisation of SOLVEPNP_ITERATIVE ---------------- */
/* the planarity test on the object points' scatter about their mean: W[2] / W[1] < 1e-3 (pts: LP_PT doubles per point) */
ISV_HD int lp_dlt_planar(int n, const double *pts) {
    double Mc[3] = {0, 0, 0}, MM[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, w[3], V[9];
    for (int i = 0; i < n; i++) for (int k = 0; k < 3; k++) Mc[k] += pts[LP_PT * i + k];
    for (int k = 0; k < 3; k++) Mc[k] /= n;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 3; j++)
            for (int k = 0; k < 3; k++) MM[3 * j + k] += (pts[LP_PT * i + j] - Mc[j]) * (pts[LP_PT * i + k] - Mc[k]);
    svd_jacobi(3, MM, w, 0, V);
    return w[2] / w[1] < 1e-3;
}
/* entry (a, b) of L^T L: the sum over the points, in order, of their two rows' products
 * (row 0: X Y Z 1 0 0 0 0 -uX -uY -uZ -u; row 1: 0 0 0 0 X Y Z 1 -vX -vY -vZ -v) */
ISV_HD double lp_dlt_entry(int n, const double *pts, int a, int b) {
    double acc = 0;
    for (int i = 0; i < n; i++) {
        const double *P = pts + LP_PT * i;
        const double h[4] = {P[0], P[1], P[2], 1.0};
        const double x = -P[3], y = -P[4];
        const double r0a = a < 4 ? h[a] : a < 8 ? 0.0 : x * h[a - 8], r0b = b < 4 ? h[b] : b < 8 ? 0.0 : x * h[b - 8];
        const double r1a = a < 4 ? 0.0 : a < 8 ? h[a - 4] : y * h[a - 8], r1b = b < 4 ? 0.0 : b < 8 ? h[b - 4] : y * h[b - 8];
        acc += r0a * r0b;
        acc += r1a * r1b;
    }
    return acc;
}
/* from L^T L (lower triangle valid; overwritten) to rvec, tvec: its smallest eigenvector as a 3 x 4 [RR | tt], the sign by the
 * determinant, the rotation by the 3 x 3 SVD, tt rescaled by |R| / |RR|, Rodrigues.  V: 144 doubles of work. */
ISV_HD void lp_dlt_pose(double *LtL, double *V, double *rvec, double *tvec) {
    double w12[12], RR[9], tt[3], A[9], w[3], U[9], V3[9], R[9];
    for (int p = 0; p < 12; p++) for (int q = 0; q < p; q++) LtL[12 * q + p] = LtL[12 * p + q];
    eig_jacobi_sym(12, LtL, w12, V);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) RR[3 * i + j] = V[12 * (4 * i + j) + 11];
        tt[i] = V[12 * (4 * i + 3) + 11];
    }
    if (rp_det3(RR) < 0) { for (int k = 0; k < 9; k++) RR[k] = -RR[k]; for (int k = 0; k < 3; k++) tt[k] = -tt[k]; }
    double sc = 0, nr = 0;
    for (int k = 0; k < 9; k++) sc += RR[k] * RR[k];
    sc = sqrt(sc);
    for (int k = 0; k < 9; k++) A[k] = RR[k];
    svd_jacobi(3, A, w, U, V3);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = U[3 * i] * V3[3 * j] + U[3 * i + 1] * V3[3 * j + 1] + U[3 * i + 2] * V3[3 * j + 2];
    for (int k = 0; k < 9; k++) nr += R[k] * R[k];
    nr = sqrt(nr);
    for (int k = 0; k < 3; k++) tvec[k] = tt[k] * (nr / sc);
    rodrigues_m2v(R, rvec);
}

/* ---------------- keyframe.cpp:200-227, :274-292 ---------------- */
/* :200-206: R_pnp = Rodrigues(rvec), T_w_c_old = R_pnp^T (-T_pnp) */
ISV_HD void lp_old_pose(const double *rvec, const double *tvec, double *R_pnp, double *T_w_c_old) {
    rodrigues_v2m(rvec, R_pnp, 0);
    for (int a = 0; a < 3; a++) T_w_c_old[a] = R_pnp[a] * (-tvec[0]) + R_pnp[3 + a] * (-tvec[1]) + R_pnp[6 + a] * (-tvec[2]);
}
/* :216-220 for one inlier (L3: the normalised residual divided by FOCAL_LENGTH, the point formed as R_pnp (p - T_w_c_old)) */
ISV_HD double lp_weight_term(const double *R_pnp, const double *T_w_c_old, const double *tvec, const lp_match_t *m, double focal) {
    double p[3], q[3];
    if (LP_OFF(3)) { for (int k = 0; k < 3; k++) q[k] = R_pnp[3 * k] * m->X[0] + R_pnp[3 * k + 1] * m->X[1] + R_pnp[3 * k + 2] * m->X[2] + tvec[k]; }
    else {
        for (int k = 0; k < 3; k++) p[k] = (double)m->X[k] - T_w_c_old[k];
        for (int k = 0; k < 3; k++) q[k] = R_pnp[3 * k] * p[0] + R_pnp[3 * k + 1] * p[1] + R_pnp[3 * k + 2] * p[2];
    }
    const double s = 1.0 / q[2];
    for (int k = 0; k < 3; k++) q[k] = s * q[k];
    const double f = LP_OFF(3) ? 1.0 : focal;
    const double d0 = ((double)m->uv[0] - q[0]) / f, d1 = ((double)m->uv[1] - q[1]) / f, d2 = (1.0 - q[2]) / f;
    return sqrt(d0 * d0 + d1 * d1 + d2 * d2);
}
/* Utility::R2ypr(R).x(), degrees (utility.h:66-83) and Utility::normalizeAngle (utility.h:131-139).  isv_device_math.h has R2ypr
 * for the kernels, but it is device-only C++ and this text also compiles as host C for the restatement, so the yaw is restated
 * here (the same expression: atan2(R10, R00) / pi * 180). */
ISV_HD double lp_yaw_deg(const double *R) { return atan2(R[3], R[0]) / 3.14159265358979323846 * 180.0; }
ISV_HD double lp_normalize_angle(double a) {
    const double two_pi = 2.0 * 180;
    return a > 0 ? a - two_pi * floor((a + 180.0) / two_pi) : a + two_pi * floor((-a + 180.0) / two_pi);
}
/* :208-209, :223-227, :274-292: the old keyframe's pose, loop_weight (res, m: the inliers' residual sum and count), the
 * relative pose and the gate.  Writes the result's pose, res, loop_weight, loop_info, has_loop, loop_index and status. */
ISV_HD void lp_finish(const isv_loop_config_t *cfg, const double *R_pnp, const double *T_w_c_old, const double *oT, const double *oR,
                      double res, int m, int old_index, isv_loop_result_t *out) {
    double Rw[9], Ro[9], To[3], rel[9], rt[3], q[4];
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) Rw[3 * a + b] = R_pnp[3 * b + a];
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) Ro[3 * a + b] = Rw[3 * a] * cfg->ric[3 * b] + Rw[3 * a + 1] * cfg->ric[3 * b + 1] + Rw[3 * a + 2] * cfg->ric[3 * b + 2];
    for (int a = 0; a < 3; a++) To[a] = T_w_c_old[a] - (Ro[3 * a] * cfg->tic[0] + Ro[3 * a + 1] * cfg->tic[1] + Ro[3 * a + 2] * cfg->tic[2]);
    for (int k = 0; k < 9; k++) out->PnP_R_old[k] = Ro[k];
    for (int k = 0; k < 3; k++) out->PnP_T_old[k] = To[k];
    out->res = res;
    out->loop_weight = (res > 0 && m > 6) ? (m - 6) / (res * res) : 0.0;
    const double d[3] = {oT[0] - To[0], oT[1] - To[1], oT[2] - To[2]};
    for (int a = 0; a < 3; a++) rt[a] = Ro[a] * d[0] + Ro[3 + a] * d[1] + Ro[6 + a] * d[2];
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) rel[3 * a + b] = Ro[a] * oR[b] + Ro[3 + a] * oR[3 + b] + Ro[6 + a] * oR[6 + b];
    eq_from_R(rel, q);
    const double yaw = lp_normalize_angle(lp_yaw_deg(oR) - lp_yaw_deg(Ro));
    if (fabs(yaw) < cfg->max_yaw_deg && sqrt(rt[0] * rt[0] + rt[1] * rt[1] + rt[2] * rt[2]) < cfg->max_distance) {
        out->has_loop = 1; out->loop_index = old_index;
        for (int k = 0; k < 3; k++) out->loop_info[k] = rt[k];
        for (int k = 0; k < 4; k++) out->loop_info[3 + k] = q[k];
        out->loop_info[7] = yaw;
        out->status = ISV_LOOP_OK;
    } else out->status = ISV_LOOP_GATE;
}

/* the first gates of findConnection on the number of descriptor matches (:262, :274): 0 = run PnPRANSAC */
ISV_HD int lp_match_gate(const isv_loop_config_t *cfg, int n_matched) {
    if (!((double)n_matched > 0.6 * cfg->min_loop_num)) return ISV_LOOP_FEW_MATCHES;
    if (!(n_matched > cfg->min_loop_num) && !LP_OFF(1)) return ISV_LOOP_UNDEFINED_POSE;   /* L1 */
    return ISV_LOOP_OK;
}

#endif /* ISV_LOOP_COMMON_H */
