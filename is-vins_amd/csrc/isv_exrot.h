/*
 * isv_exrot.h -- internal to the camera-IMU rotation calibration (isv_exrot.hip), outside include/: what the kernel k_exr_calibrate
 * shares with its CPU restatement tests/native/isv_exr_oracle.c, as plain C that compiles as HIP device code (ISV_HD) or as host C,
 * beside the serial pieces of isv_init_common.h (the RNG, the subsets, run7Point, computeError, rp_triangulate, svd_jacobi).  Every
 * includer turns FP contraction off for its whole translation unit.  The quirks X1..X8 are those of include/isvins_exrot.h; the line
 * numbers are those of src/initial/initial_ex_rotation.cpp.  Eigen's fixed-size sums and products are read left to right, as
 * everywhere in this project (isv_device_math.h).  Below, for HIP only, the calibrator handle.
 */
#ifndef ISV_EXROT_H
#define ISV_EXROT_H
#include <string.h>
#include "../../include/isvins_exrot.h"
#include "isv_init_common.h"

#define EXR_F_THRESH 3.0          /* findFundamentalMat's default param1 (X2) */
#define EXR_HIST 27               /* doubles per recorded frame: Rc, Rimu, Rc_g */
#define EXR_PI 3.14159265358979323846   /* M_PI */
#define EXR_FINITE(v) ((v) - (v) == 0)  /* neither an infinity nor a NaN */

ISV_HD void exr_mul3(const double *A, const double *B, double *C) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}

/* Eigen 3.3 Quaternion(Matrix3d) (quaternionbase_assign_impl<Other, 3, 3>): q = (w, x, y, z) */
ISV_HD void exr_q_from_R(const double *m, double *q) {
    double t = m[0] + m[4] + m[8];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[1] = (m[7] - m[5]) * t;
        q[2] = (m[2] - m[6]) * t;
        q[3] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[i * 3 + i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(m[i * 3 + i] - m[j * 3 + j] - m[k * 3 + k] + 1.0);
        q[1 + i] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[k * 3 + j] - m[j * 3 + k]) * t;
        q[1 + j] = (m[j * 3 + i] + m[i * 3 + j]) * t;
        q[1 + k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
    }
}

/* Eigen 3.3 QuaternionBase::toRotationMatrix of q = (w, x, y, z), as given (no normalisation) */
ISV_HD void exr_q_to_R(const double *q, double *R) {
    const double tx = 2.0 * q[1], ty = 2.0 * q[2], tz = 2.0 * q[3];
    const double twx = tx * q[0], twy = ty * q[0], twz = tz * q[0];
    const double txx = tx * q[1], txy = ty * q[1], txz = tz * q[1];
    const double tyy = ty * q[2], tyz = tz * q[2], tzz = tz * q[3];
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
    R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}

/* Eigen 3.3 Matrix3d::inverse() (compute_inverse<MatrixType, ResultType, 3>): by cofactors, inverse(r, c) = cofactor<c, r> / det */
ISV_HD double exr_cofactor(const double *m, int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[i1 * 3 + j1] * m[i2 * 3 + j2] - m[i1 * 3 + j2] * m[i2 * 3 + j1];
}
ISV_HD void exr_inv3(const double *m, double *o) {
    const double c0 = exr_cofactor(m, 0, 0), c1 = exr_cofactor(m, 1, 0), c2 = exr_cofactor(m, 2, 0);
    const double det = c0 * m[0] + c1 * m[3] + c2 * m[6];
    const double invdet = 1.0 / det;
    o[0] = c0 * invdet; o[1] = c1 * invdet; o[2] = c2 * invdet;
    for (int r = 1; r < 3; r++)
        for (int c = 0; c < 3; c++) o[r * 3 + c] = exr_cofactor(m, c, r) * invdet;
}

/* X3: decomposeE (:126-141).  E row-major -> R1 = U W Vt, R2 = U Wt Vt, t = u3 (t1 = t, t2 = -t).  Deviation: svd_jacobi, not cv::SVD. */
ISV_HD void exr_decompose(const double *E, double *R1, double *R2, double *t) {
    double A[9], w[3], U[9], V[9], Vt[9], UW[9], UWt[9];
    for (int k = 0; k < 9; k++) A[k] = E[k];
    svd_jacobi(3, A, w, U, V);
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) Vt[a * 3 + b] = V[b * 3 + a];
    const double W[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, Wt[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};
    exr_mul3(U, W, UW); exr_mul3(UW, Vt, R1);
    exr_mul3(U, Wt, UWt); exr_mul3(UWt, Vt, R2);
    for (int a = 0; a < 3; a++) t[a] = U[a * 3 + 2];
}

/* solveRelativeR's use of it (:80-86): returns 1 when the E = -E branch was taken */
ISV_HD int exr_decompose_signed(const double *E, double *R1, double *R2, double *t) {
    exr_decompose(E, R1, R2, t);
    if (rp_det3(R1) + 1.0 < 1e-09) {
        double En[9];
        for (int k = 0; k < 9; k++) En[k] = -E[k];
        exr_decompose(En, R1, R2, t);
        return 1;
    }
    return 0;
}

/* X4: testTriangulation's P1 = [R | sign * t] (:108-110), rounded to float32 (cv::Matx34f) unless `keep_double` (the restatement's hook) */
ISV_HD void exr_camera(const double *R, const double *t, double sign, int keep_double, double *P) {
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) P[a * 4 + b] = keep_double ? R[a * 3 + b] : (double)(float)R[a * 3 + b];
        const double tv = sign < 0 ? -t[a] : t[a];
        P[a * 4 + 3] = keep_double ? tv : (double)(float)tv;
    }
}

/* X4: one point of testTriangulation (:111-120) against camera P (the other is [I | 0]): 1 when it lies in front of both.  The
 * homogeneous point is stored as float32; alpha = 1. / normal_factor scales the float32 gemm's double accumulator, whose result is
 * stored as float32 (the reading include/isvins_exrot.h states).  `keep_double`: no float32 store anywhere (the hook). */
ISV_HD int exr_front(const double *P, double x0, double y0, double x1, double y1, int keep_double) {
    double Q[4];
    rp_triangulate(P, x0, y0, x1, y1, Q);
    if (!keep_double) for (int k = 0; k < 4; k++) Q[k] = (double)(float)Q[k];
    const double alpha = 1. / Q[3];
    double sl = 0.0, sr = 0.0;
    sl += 0.0 * Q[0]; sl += 0.0 * Q[1]; sl += 1.0 * Q[2]; sl += 0.0 * Q[3];
    for (int k = 0; k < 4; k++) sr += P[8 + k] * Q[k];
    double zl = sl * alpha, zr = sr * alpha;
    if (!keep_double) { zl = (double)(float)zl; zr = (double)(float)zr; }
    return zl > 0 && zr > 0;
}

/* :87-89: front [4] of (R1,t1), (R1,t2), (R2,t1), (R2,t2) over n points -> 1 (R1) or 2 (R2); a tie gives R2 */
ISV_HD int exr_choose(const int *front, int n) {
    const double r0 = 1.0 * front[0] / n, r1 = 1.0 * front[1] / n, r2 = 1.0 * front[2] / n, r3 = 1.0 * front[3] / n;
    const double ratio1 = r0 < r1 ? r1 : r0, ratio2 = r2 < r3 ? r3 : r2;   /* std::max(a, b) = a < b ? b : a */
    return ratio1 > ratio2 ? 1 : 2;
}

/* X6 (:15-16): Rimu = delta_q.toRotationMatrix(), Rc_g = ric.inverse() * delta_q * ric = (ric^-1 * Rimu) * ric */
ISV_HD void exr_imu_rows(const double *ric, const double *dq, double *Rimu, double *Rc_g) {
    double inv[9], T[9];
    exr_q_to_R(dq, Rimu);
    exr_inv3(ric, inv);
    exr_mul3(inv, Rimu, T);
    exr_mul3(T, ric, Rc_g);
}

/* X7 (:23-48): one frame's angle (degrees), weight and 4 x 4 block huber * (L - R), row-major */
ISV_HD void exr_row(const double *Rc, const double *Rimu, const double *Rc_g, double *angle_deg, double *huber_out, double *blk) {
    double r1[4], r2[4], qi[4], d[4];
    exr_q_from_R(Rc, r1);
    exr_q_from_R(Rc_g, r2);
    /* r1 * r2.conjugate() */
    const double bw = r2[0], bx = -r2[1], by = -r2[2], bz = -r2[3];
    d[0] = r1[0] * bw - r1[1] * bx - r1[2] * by - r1[3] * bz;
    d[1] = r1[0] * bx + r1[1] * bw + r1[2] * bz - r1[3] * by;
    d[2] = r1[0] * by + r1[2] * bw + r1[3] * bx - r1[1] * bz;
    d[3] = r1[0] * bz + r1[3] * bw + r1[1] * by - r1[2] * bx;
    const double ang = 2.0 * atan2(sqrt(d[1] * d[1] + d[2] * d[2] + d[3] * d[3]), fabs(d[0]));   /* Eigen 3.3.4 angularDistance */
    const double angular_distance = 180 / EXR_PI * ang;
    const double huber = angular_distance > 5.0 ? 5.0 / angular_distance : 1.0;
    exr_q_from_R(Rimu, qi);
    const double *q[2] = {r1, qi};
    double LR[2][16];
    for (int s = 0; s < 2; s++) {   /* s = 0: L of Rc, w I + skew(q); s = 1: R of Rimu, w I - skew(q) */
        const double w = q[s][0], x = q[s][1], y = q[s][2], z = q[s][3];
        const double S[9] = {0, -z, y, z, 0, -x, -y, x, 0};
        double *M = LR[s];
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) M[a * 4 + b] = s ? w * (a == b ? 1.0 : 0.0) - S[a * 3 + b] : w * (a == b ? 1.0 : 0.0) + S[a * 3 + b];
            M[a * 4 + 3] = q[s][1 + a];
            M[12 + a] = -q[s][1 + a];
        }
        M[15] = w;
    }
    for (int k = 0; k < 16; k++) blk[k] = huber * (LR[0][k] - LR[1][k]);
    *angle_deg = angular_distance; *huber_out = huber;
}

/* X8: the Householder QR of A [rows][4] (rows >= 4), column by column in rp_triangulate's serial order, in steps so that the
 * kernel can give each column's update to a lane: exr_qr_begin(k) gives the reflector of column k (0: the column is skipped);
 * exr_qr_apply(k, c) applies it to column c >= k.  The reflector v is column k from row k down with v[k] -= alpha; it is read from
 * A, so column k itself is applied LAST (the restatement's order; the kernel's barrier). */
ISV_HD int exr_qr_begin(int rows, const double *A, int k, double *alpha_out, double *vv_out) {
    double nx = 0;
    for (int i = k; i < rows; i++) nx += A[i * 4 + k] * A[i * 4 + k];
    nx = sqrt(nx);
    if (nx == 0.0) return 0;
    const double alpha = A[k * 4 + k] > 0 ? -nx : nx;
    double vv = 0;
    for (int i = k; i < rows; i++) {
        const double v = i == k ? A[i * 4 + k] - alpha : A[i * 4 + k];
        vv += v * v;
    }
    if (vv == 0.0) return 0;
    *alpha_out = alpha; *vv_out = vv;
    return 1;
}
ISV_HD void exr_qr_apply(int rows, double *A, int k, int c, double alpha, double vv) {
    double s = 0;
    for (int i = k; i < rows; i++) {
        const double v = i == k ? A[i * 4 + k] - alpha : A[i * 4 + k];
        s += v * A[i * 4 + c];
    }
    s = 2.0 * s / vv;
    for (int i = k; i < rows; i++) {
        const double v = i == k ? A[i * 4 + k] - alpha : A[i * 4 + k];
        A[i * 4 + c] -= s * v;
    }
}

/* X8 (:51-59): from the QR's 4 x 4 factor (the first four rows of A, its upper triangle) the singular values, descending, and
 * ric = toRotationMatrix(V.col(3) as x, y, z, w).inverse() */
ISV_HD void exr_solve_ric(const double *A, double *singular, double *ric) {
    double Rm[16], V[16], R[9], q[4];
    for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) Rm[a * 4 + b] = b >= a ? A[a * 4 + b] : 0.0;
    svd_jacobi(4, Rm, singular, 0, V);
    q[0] = V[15]; q[1] = V[3]; q[2] = V[7]; q[3] = V[11];
    exr_q_to_R(q, R);
    exr_inv3(R, ric);
}

ISV_HD int exr_calibrated(int frame_count, int vo_size, const double *singular) { return frame_count >= vo_size && singular[2] > 0.25; }

/* ---------------- host: the refusals ---------------- */
static int exr_check_config(const isv_exr_config_t *c) {
    return c->max_slots >= 1 && c->max_slots <= 65535 && c->max_frames >= 8 && c->max_frames <= ISV_EXR_MAX_FRAMES &&
           c->max_corres >= ISV_EXR_MIN_CORRES && c->max_corres <= ISV_EXR_MAX_CORRES && c->vo_size >= 2;
}

/* the per-item refusals of isv_exr_calibrate_batch, in their order.  frame_counts [max_slots]: the slots' counts before the call;
 * named [max_slots]: non-zero where an earlier item of the call named the slot (a refused one too). */
static int exr_check_item(const isv_exr_config_t *cfg, const isv_exr_item_t *it, const int32_t *frame_counts, const uint8_t *named) {
    if (it->slot < 0 || it->slot >= cfg->max_slots || it->n_corres < 0) return ISV_EXR_INPUT;
    if (named[it->slot]) return ISV_EXR_INPUT;
    if (it->n_corres > cfg->max_corres) return ISV_EXR_CAPACITY;
    if (it->n_corres > 0 && !it->corres) return ISV_EXR_INPUT;
    for (int k = 0; k < 4 * it->n_corres; k++)
        if (!EXR_FINITE(it->corres[k])) return ISV_EXR_INPUT;
    double n2 = 0;
    for (int k = 0; k < 4; k++) {
        if (!EXR_FINITE(it->delta_q[k])) return ISV_EXR_INPUT;
        n2 += it->delta_q[k] * it->delta_q[k];
    }
    if (!(n2 > 0.0) || !EXR_FINITE(n2)) return ISV_EXR_INPUT;
    if (frame_counts[it->slot] >= cfg->max_frames) return ISV_EXR_CAPACITY;
    return ISV_EXR_OK;
}

/* a refused item's result: zero apart from status and frame_count (the host's refusals and the kernel's) */
#if defined(__HIPCC__)
__host__
#endif
ISV_HD void exr_refuse(isv_exr_result_t *res, int status, int frame_count) {
    memset(res, 0, sizeof(*res));
    res->status = status; res->frame_count = frame_count;
}

#ifdef __HIPCC__
#include "isv_stage_launch.h"

struct ExrSlotHdr {               // a slot's head on the device
    int32_t frame_count, pad;
    double ric[9];
};

struct ExrHdr {                   // per-item record
    int64_t pt_off;               // the item's first correspondence, into the call's points (4 doubles each)
    int32_t slot, n;
    double dq[4];
};

struct isv_exr : StageHandle {
    isv_exr_config_t cfg;
    ExrSlotHdr *d_head = nullptr; // [max_slots]
    double *d_hist = nullptr;     // [max_slots][max_frames][EXR_HIST]
    double *d_A = nullptr;        // [max_slots][4 * max_frames][4]: the call's A, scratch
    int32_t *d_list = nullptr;    // [max_slots]: isv_exr_reset's slots
    std::vector<int32_t> fc;      // [max_slots]: the slots' frame counts, mirrored (the CAPACITY check needs them before the launch)
    std::vector<uint8_t> named;   // [max_slots]: scratch of a call's duplicate check, all zero between calls
    std::vector<char> up;
};
#endif
#endif /* ISV_EXROT_H */
