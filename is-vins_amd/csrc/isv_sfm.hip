// isv_sfm.hip -- the SfM stage of the initialisation, batched: IMU excitation, GlobalSFM::construct (PnP + triangulation
// sweeps, the full BA), the all-frame PnP; one 64-lane workgroup per problem (isv_sfm.h -- internal, not part of the public
// ABI -- has the contract, the reference lines, the restatements and the quirks S1..S8).
//
// Per problem, in LDS (dynamic, sized by the batch's largest problem): the track observations, the points, the packed reduced
// camera system of the BA (the PnP's 64-point row staging shares its space), the camera blocks and their columns' scale /
// diagonal / gradient / step.  In global memory, a per-track block of 40 doubles in the handle's device block: the point
// blocks (E^T E + D^2)^-1 and E^T r, the point columns' scale / diagonal / gradient / step, the candidate point, a partial sum,
// and the PnP's float-rounded point list.
// Lanes: one per track (triangulation, the point blocks, the back-substitution, the per-point parts of every cost and norm),
// one per (frame pair, column) of the reduced system and one per reduced column of its right-hand side, row-strided for the
// Cholesky's columns, one per JtJ / JtErr entry of the PnP (the 6 x 6 LM of OpenCV) over rows staged 64 points at a time.
// The PnPs of stage 4 run one after another on the problem's workgroup.  Sums that cross lanes run on lane 0 in index order
// (per-point partials in track order), so the result does not depend on the batch, and matches
// tests/native/isv_sfm_oracle.c operation by operation.  No atomics.  Contraction is off for the whole translation unit.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <float.h>
#include <string.h>
#include <unordered_map>
#include <vector>
#include "isv_stage_launch.h"
#include "isv_sfm.h"
#include "isv_init_common.h"
#include "isv_pnp.h"

namespace {

constexpr int kLanes = 64;
constexpr int kNC = 6 * ISV_ALIGN_MAX_WINDOW;   // reduced columns, upper bound
constexpr int kScr = 40;                        // doubles of the per-track global block
// per-track block: W 0..8, E^T r 9..11, scale 12..14, diag 15..17, D 18..20, gradient 21..23, step 24..26, delta 27..29,
// candidate 30..32, partial sum 33 (indexed by the active point), PnP point n 34..38 (indexed by n)
enum { O_W = 0, O_G = 9, O_SC = 12, O_DG = 15, O_D = 18, O_PG = 21, O_DX = 24, O_DL = 27, O_XC = 30, O_PART = 33, O_PNP = 34 };

struct SfmHdr {                   // host-packed per-problem record
    int32_t status, nw, nf, l, ntr, nobs, npts;
    int32_t trk_off, obs_off, pt_off_off, pt_base, frame_off;
    int64_t scr_off;
    int32_t win[ISV_ALIGN_MAX_WINDOW];
    double relR[9], relT[3], RIC[9];
};

// the restatement's per-lane serial pieces (Eigen JacobiSVD / quaternion, Ceres' rotation, Plus and the 3 x 3 LLT inverse); the
// same text as tests/native/isv_sfm_oracle.c (svd_jacobi and the excitation check are in isv_init_common.h, shared with
// isv_relpose.hip; OpenCV's Rodrigues / projection / LM step, the workgroup's CvLevMarq loop and Eigen's matrix -> quaternion are
// in isv_pnp.h, shared with isv_loop.hip)
/* GlobalSFM::triangulatePoint: P0 / P1 are 3 x 4 row-major [R | t] */
static __device__ void triangulate(const double *P0, const double *P1, const double *x0, const double *x1, double *out) {
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

/* ---------------- Eigen quaternion pieces (w x y z here; eq_from_R is in isv_pnp.h) ---------------- */
static __device__ void eq_to_R(const double *q, double *r) {     /* toRotationMatrix (no normalisation) */
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    r[0] = 1.0 - (tyy + tzz); r[1] = txy - twz; r[2] = txz + twy;
    r[3] = txy + twz; r[4] = 1.0 - (txx + tzz); r[5] = tyz - twx;
    r[6] = txz - twy; r[7] = tyz + twx; r[8] = 1.0 - (txx + tyy);
}
static __device__ void eq_inv(const double *q, double *o) {      /* inverse(): conjugate / squaredNorm (S6) */
    double n2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3] + q[0] * q[0];
    if (n2 > 0.0) { o[0] = q[0] / n2; o[1] = -q[1] / n2; o[2] = -q[2] / n2; o[3] = -q[3] / n2; }
    else { o[0] = o[1] = o[2] = o[3] = 0.0; }
}
static __device__ void eq_mul(const double *a, const double *b, double *o) {
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
    o[3] = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
}
static __device__ void eq_transform(const double *q, const double *v, double *o) {   /* _transformVector: assumes |q| = 1 (S6) */
    double uv[3] = {q[2] * v[2] - q[3] * v[1], q[3] * v[0] - q[1] * v[2], q[1] * v[1] - q[2] * v[0]};
    for (int k = 0; k < 3; k++) uv[k] += uv[k];
    double c[3] = {q[2] * uv[2] - q[3] * uv[1], q[3] * uv[0] - q[1] * uv[2], q[1] * uv[1] - q[2] * uv[0]};
    for (int k = 0; k < 3; k++) o[k] = v[k] + q[0] * uv[k] + c[k];
}
static __device__ void mv3(const double *M, const double *v, double *o) {
    for (int a = 0; a < 3; a++) o[a] = M[a * 3] * v[0] + M[a * 3 + 1] * v[1] + M[a * 3 + 2] * v[2];
}
static __device__ void mmT3(const double *A, const double *B, double *C) {   /* A * B^T */
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j * 3] + A[i * 3 + 1] * B[j * 3 + 1] + A[i * 3 + 2] * B[j * 3 + 2];
}

/* QuaternionRotatePoint + translation + projection; J* unscaled (2 x 3 each); q w x y z */
static __device__ void ba_obs(const double *q, const double *t, const double *X, const double *uv, double *r, double *Jq, double *Jt, double *JX) {
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
static __device__ void quat_plus(const double *x, const double *d, double *o) {   /* QuaternionParameterization::Plus */
    const double nd = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (nd > 0.0) {
        const double sdd = sin(nd) / nd;
        const double qd[4] = {cos(nd), sdd * d[0], sdd * d[1], sdd * d[2]};
        eq_mul(qd, x, o);
    } else { for (int k = 0; k < 4; k++) o[k] = x[k]; }
}
/* 3 x 3 LLT and its inverse (solve against the identity, column by column) */
static __device__ void inv3_llt(const double *A, double *W) {
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

__device__ __forceinline__ int pk(int r, int c) { return r * (r + 1) / 2 + c; }
__device__ __forceinline__ bool in_frame(const isv_sfm_track_t &T, int f) { return f >= T.start_frame && f < T.start_frame + T.n_obs; }

// misc slots (LDS doubles); the PnP block at M_PNP is isv_pnp.h's P_*
enum { M_SCAL = 0, M_FLAG = 1, M_N = 2, M_CP = 8, M_PNP = 32, M_END = 96 };

struct BA {
    const isv_sfm_track_t *tr;
    const double *obs;            // LDS [n_obs][2]
    double *X;                    // LDS [n_tracks][3]
    double *scr;                  // the problem's per-track blocks
    const int16_t *act;
    int nact, nw, l, nc;
    double *cq, *ct, *cqc, *ctc, *csc, *cD, *cdiag, *cg, *cdx, *cdel, *rhs, *S, *misc;
    __device__ int ncf(int f) const { return f == l ? 0 : f == nw - 1 ? 3 : 6; }
    __device__ int coff(int f) const { return 6 * f - (f > l ? 6 : 0); }
    __device__ double &sc(int j, int o) const { return scr[(size_t)j * kScr + o]; }
    __device__ const double *uv(const isv_sfm_track_t &T, int f) const { return obs + 2 * (T.obs_off + f - T.start_frame); }
    // scaled E (2 x 3) and F (2 x ncf) of one observation (the restatement's ba_EF)
    __device__ void EF(const double *q4, const double *t3, const double *Xp, int j, int f, const double *uvp, double *r, double *E, double *F) const {
        double Jq[6], Jt[6], JX[6];
        ba_obs(q4 + 4 * f, t3 + 3 * f, Xp, uvp, r, Jq, Jt, JX);
        const int nf = ncf(f), co = coff(f);
        for (int a = 0; a < 2; a++) {
            for (int k = 0; k < 3; k++) E[a * 3 + k] = JX[a * 3 + k] * sc(j, O_SC + k);
            for (int c = 0; c < nf; c++) F[a * 6 + c] = (c < 3 ? Jq[a * 3 + c] : Jt[a * 3 + c - 3]) * csc[co + c];
        }
    }
};

// ---- the BA's pieces; every function is entered by all lanes and ends with a barrier ----
// X / xs: the points and their stride (LDS, 3) or the candidates (global block, kScr)
__device__ double ba_cost(const BA &B, const double *cq, const double *ct, const double *X, int xs) {
    const int t = threadIdx.x;
    for (int a = t; a < B.nact; a += kLanes) {
        const int j = B.act[a];
        const isv_sfm_track_t &T = B.tr[j];
        double cp = 0;
        for (int k = 0; k < T.n_obs; k++) {
            double r[2];
            ba_obs(cq + 4 * (T.start_frame + k), ct + 3 * (T.start_frame + k), X + (size_t)xs * j, B.obs + 2 * (T.obs_off + k), r, nullptr, nullptr, nullptr);
            cp += 0.5 * (r[0] * r[0] + r[1] * r[1]);
        }
        B.sc(a, O_PART) = cp;
    }
    __syncthreads();
    if (t == 0) {
        double c = 0;
        for (int a = 0; a < B.nact; a++) c += B.sc(a, O_PART);
        B.misc[M_SCAL] = c;
    }
    __syncthreads();
    return B.misc[M_SCAL];
}

// column sums of squares of the scaled Jacobian (into O_DG / cn) and, if grad, the unscaled gradient (O_PG / cg)
__device__ void ba_colnorm(const BA &B, bool grad) {
    const int t = threadIdx.x;
    for (int a = t; a < B.nact; a += kLanes) {
        const int j = B.act[a];
        const isv_sfm_track_t &T = B.tr[j];
        double s[3] = {0, 0, 0}, g[3] = {0, 0, 0};
        for (int k = 0; k < T.n_obs; k++) {
            double r[2], Jq[6], Jt[6], JX[6];
            ba_obs(B.cq + 4 * (T.start_frame + k), B.ct + 3 * (T.start_frame + k), B.X + 3 * j, B.obs + 2 * (T.obs_off + k), r, Jq, Jt, JX);
            for (int row = 0; row < 2; row++)
                for (int c = 0; c < 3; c++) {
                    double e = JX[row * 3 + c] * B.sc(j, O_SC + c);
                    s[c] += e * e;
                    g[c] += JX[row * 3 + c] * r[row];
                }
        }
        for (int c = 0; c < 3; c++) { B.sc(j, O_DG + c) = s[c]; if (grad) B.sc(j, O_PG + c) = g[c]; }
    }
    for (int f = t; f < B.nw; f += kLanes) {
        const int nf = B.ncf(f), co = B.coff(f);
        double s[6] = {0, 0, 0, 0, 0, 0}, g[6] = {0, 0, 0, 0, 0, 0};
        for (int a = 0; a < B.nact; a++) {
            const int j = B.act[a];
            const isv_sfm_track_t &T = B.tr[j];
            if (!in_frame(T, f) || !nf) continue;
            double r[2], Jq[6], Jt[6], JX[6];
            ba_obs(B.cq + 4 * f, B.ct + 3 * f, B.X + 3 * j, B.uv(T, f), r, Jq, Jt, JX);
            for (int row = 0; row < 2; row++)
                for (int c = 0; c < nf; c++) {
                    double jj = c < 3 ? Jq[row * 3 + c] : Jt[row * 3 + c - 3];
                    double e = jj * B.csc[co + c];
                    s[c] += e * e;
                    g[c] += jj * r[row];
                }
        }
        for (int c = 0; c < nf; c++) { B.cdiag[co + c] = s[c]; if (grad) B.cg[co + c] = g[c]; }
    }
    __syncthreads();
}

__device__ double ba_norm2(const BA &B, const double *cq, const double *ct, const double *X, int xs, const double *cq2, const double *ct2, const double *X2, int x2s) {
    const int t = threadIdx.x;
    for (int a = t; a < B.nact; a += kLanes) {
        const int j = B.act[a];
        double pp = 0;
        for (int k = 0; k < 3; k++) { double d = X[(size_t)xs * j + k] - (X2 ? X2[(size_t)x2s * j + k] : 0.0); pp += d * d; }
        B.sc(a, O_PART) = pp;
    }
    __syncthreads();
    if (t == 0) {
        double s = 0;
        for (int a = 0; a < B.nact; a++) s += B.sc(a, O_PART);
        for (int f = 0; f < B.nw; f++) {
            if (B.ncf(f) >= 3) for (int k = 0; k < 4; k++) { double d = cq[4 * f + k] - (cq2 ? cq2[4 * f + k] : 0.0); s += d * d; }
            if (B.ncf(f) == 6) for (int k = 0; k < 3; k++) { double d = ct[3 * f + k] - (ct2 ? ct2[3 * f + k] : 0.0); s += d * d; }
        }
        B.misc[M_SCAL] = s;
    }
    __syncthreads();
    return B.misc[M_SCAL];
}

__device__ double ba_gmax(const BA &B) {
    const int t = threadIdx.x;
    for (int a = t; a < B.nact; a += kLanes) {
        const int j = B.act[a];
        double m = 0;
        for (int k = 0; k < 3; k++) { double v = fabs(B.X[3 * j + k] - (B.X[3 * j + k] + -B.sc(j, O_PG + k))); m = v > m ? v : m; }
        B.sc(a, O_PART) = m;
    }
    for (int f = t; f < B.nw; f += kLanes) {
        double m = 0;
        const int co = B.coff(f);
        if (B.ncf(f) >= 3) {
            double ng[3] = {-B.cg[co], -B.cg[co + 1], -B.cg[co + 2]}, qp[4];
            quat_plus(B.cq + 4 * f, ng, qp);
            for (int k = 0; k < 4; k++) { double v = fabs(B.cq[4 * f + k] - qp[k]); m = v > m ? v : m; }
        }
        if (B.ncf(f) == 6)
            for (int k = 0; k < 3; k++) { double v = fabs(B.ct[3 * f + k] - (B.ct[3 * f + k] + -B.cg[co + 3 + k])); m = v > m ? v : m; }
        B.misc[M_CP + f] = m;
    }
    __syncthreads();
    if (t == 0) {   // a maximum: the order of the parts does not matter
        double m = 0;
        for (int a = 0; a < B.nact; a++) { double v = B.sc(a, O_PART); m = v > m ? v : m; }
        for (int f = 0; f < B.nw; f++) { double v = B.misc[M_CP + f]; m = v > m ? v : m; }
        B.misc[M_SCAL] = m;
    }
    __syncthreads();
    return B.misc[M_SCAL];
}

// the LM step's linear system (the restatement's ba_schur); returns 1 when the reduced system's Cholesky failed
__device__ int ba_schur(const BA &B) {
    const int t = threadIdx.x;
    for (int a = t; a < B.nact; a += kLanes) {   // point blocks
        const int j = B.act[a];
        const isv_sfm_track_t &T = B.tr[j];
        double ete[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, W[9];
        for (int k = 0; k < 3; k++) ete[k * 4] = B.sc(j, O_D + k) * B.sc(j, O_D + k);
        for (int k = 0; k < T.n_obs; k++) {
            const int f = T.start_frame + k;
            double r[2], E[6], F[12];
            B.EF(B.cq, B.ct, B.X + 3 * j, j, f, B.obs + 2 * (T.obs_off + k), r, E, F);
            for (int i = 0; i < 3; i++) {
                for (int jj = 0; jj < 3; jj++) ete[i * 3 + jj] += E[i] * E[jj] + E[3 + i] * E[3 + jj];
                g[i] += E[i] * r[0] + E[3 + i] * r[1];
            }
        }
        inv3_llt(ete, W);
        for (int k = 0; k < 9; k++) B.sc(j, O_W + k) = W[k];
        for (int k = 0; k < 3; k++) B.sc(j, O_G + k) = g[k];
    }
    __syncthreads();
    // reduced system: one lane per (fa >= fb, column b of fb's block), its column of the block in point order
    const int nitems = B.nw * (B.nw + 1) / 2 * 6;
    for (int it = t; it < nitems; it += kLanes) {
        int pr = it / 6, b = it % 6, fa = 0;
        while ((fa + 1) * (fa + 2) / 2 <= pr) fa++;
        const int fb = pr - fa * (fa + 1) / 2;
        const int na = B.ncf(fa), nb = B.ncf(fb);
        if (!na || b >= nb) continue;
        const int ca = B.coff(fa), cb = B.coff(fb);
        double s[6];
        for (int a = 0; a < na; a++) s[a] = (fa == fb && a == b) ? B.cD[ca + a] * B.cD[ca + a] : 0.0;
        for (int q = 0; q < B.nact; q++) {
            const int j = B.act[q];
            const isv_sfm_track_t &T = B.tr[j];
            if (!in_frame(T, fa) || !in_frame(T, fb)) continue;
            double r[2], Ea[6], Fa[12], Eb[6], Fb[12], Ba[18], Bb[3], wb[3];
            B.EF(B.cq, B.ct, B.X + 3 * j, j, fa, B.uv(T, fa), r, Ea, Fa);
            B.EF(B.cq, B.ct, B.X + 3 * j, j, fb, B.uv(T, fb), r, Eb, Fb);
            for (int c = 0; c < na; c++)
                for (int k = 0; k < 3; k++) Ba[k * 6 + c] = Ea[k] * Fa[c] + Ea[3 + k] * Fa[6 + c];
            for (int k = 0; k < 3; k++) Bb[k] = Eb[k] * Fb[b] + Eb[3 + k] * Fb[6 + b];
            const double *W = &B.sc(j, O_W);
            for (int k = 0; k < 3; k++) wb[k] = W[k * 3] * Bb[0] + W[k * 3 + 1] * Bb[1] + W[k * 3 + 2] * Bb[2];
            for (int a = 0; a < na; a++) {
                if (fa == fb && b > a) continue;
                double v = s[a];
                if (fa == fb) v += Fa[a] * Fa[b] + Fa[6 + a] * Fa[6 + b];
                v -= Ba[a] * wb[0] + Ba[6 + a] * wb[1] + Ba[12 + a] * wb[2];
                s[a] = v;
            }
        }
        for (int a = 0; a < na; a++)
            if (fa != fb || b <= a) B.S[pk(ca + a, cb + b)] = s[a];
    }
    for (int ra = t; ra < B.nc; ra += kLanes) {   // right-hand side, a lane per reduced column
        int fa = 0;
        while (!(B.ncf(fa) && ra >= B.coff(fa) && ra < B.coff(fa) + B.ncf(fa))) fa++;
        const int a = ra - B.coff(fa);
        double s = 0;
        for (int q = 0; q < B.nact; q++) {
            const int j = B.act[q];
            const isv_sfm_track_t &T = B.tr[j];
            if (!in_frame(T, fa)) continue;
            double r[2], E[6], F[12], Ba[3], wg[3];
            B.EF(B.cq, B.ct, B.X + 3 * j, j, fa, B.uv(T, fa), r, E, F);
            s += F[a] * r[0] + F[6 + a] * r[1];
            const double *W = &B.sc(j, O_W), *g = &B.sc(j, O_G);
            for (int k = 0; k < 3; k++) { Ba[k] = E[k] * F[a] + E[3 + k] * F[6 + a]; wg[k] = W[k * 3] * g[0] + W[k * 3 + 1] * g[1] + W[k * 3 + 2] * g[2]; }
            s -= Ba[0] * wg[0] + Ba[1] * wg[1] + Ba[2] * wg[2];
        }
        B.rhs[ra] = s;
    }
    __syncthreads();
    const int nc = B.nc;
    double *S = B.S;
    for (int j = 0; j < nc; j++) {   // left-looking Cholesky: the pivot on lane 0, the column's rows strided over the lanes
        if (t == 0) {
            double s = S[pk(j, j)];
            for (int k = 0; k < j; k++) s -= S[pk(j, k)] * S[pk(j, k)];
            B.misc[M_FLAG] = (s > 0.0) ? 0.0 : 1.0;
            S[pk(j, j)] = (s > 0.0) ? sqrt(s) : s;
        }
        __syncthreads();
        if (B.misc[M_FLAG] != 0.0) return 1;
        for (int i = j + 1 + t; i < nc; i += kLanes) {
            double v = S[pk(i, j)];
            for (int k = 0; k < j; k++) v -= S[pk(i, k)] * S[pk(j, k)];
            S[pk(i, j)] = v / S[pk(j, j)];
        }
        __syncthreads();
    }
    if (t == 0) {
        double *rhs = B.rhs;
        for (int i = 0; i < nc; i++) { double v = rhs[i]; for (int k = 0; k < i; k++) v -= S[pk(i, k)] * rhs[k]; rhs[i] = v / S[pk(i, i)]; }
        for (int i = nc - 1; i >= 0; i--) { double v = rhs[i]; for (int k = i + 1; k < nc; k++) v -= S[pk(k, i)] * rhs[k]; rhs[i] = v / S[pk(i, i)]; }
        for (int c = 0; c < nc; c++) B.cdx[c] = -rhs[c];
    }
    __syncthreads();
    for (int a = t; a < B.nact; a += kLanes) {   // back-substitution
        const int j = B.act[a];
        const isv_sfm_track_t &T = B.tr[j];
        double v[3] = {0, 0, 0};
        for (int k = 0; k < T.n_obs; k++) {
            const int f = T.start_frame + k, co = B.coff(f), nf = B.ncf(f);
            double r[2], E[6], F[12], sj[2];
            B.EF(B.cq, B.ct, B.X + 3 * j, j, f, B.obs + 2 * (T.obs_off + k), r, E, F);
            for (int row = 0; row < 2; row++) {
                double fy = 0;
                for (int c = 0; c < nf; c++) fy += F[row * 6 + c] * B.rhs[co + c];
                sj[row] = r[row] - fy;
            }
            for (int i = 0; i < 3; i++) v[i] += E[i] * sj[0] + E[3 + i] * sj[1];
        }
        const double *W = &B.sc(j, O_W);
        for (int i = 0; i < 3; i++) B.sc(j, O_DX + i) = -(W[i * 3] * v[0] + W[i * 3 + 1] * v[1] + W[i * 3 + 2] * v[2]);
    }
    __syncthreads();
    return 0;
}

// 1 when every step entry is finite
__device__ bool ba_finite(const BA &B) {
    const int t = threadIdx.x;
    for (int a = t; a < B.nact; a += kLanes) {
        const int j = B.act[a];
        B.sc(a, O_PART) = (isfinite(B.sc(j, O_DX)) && isfinite(B.sc(j, O_DX + 1)) && isfinite(B.sc(j, O_DX + 2))) ? 1.0 : 0.0;
    }
    __syncthreads();
    if (t == 0) {
        bool ok = true;
        for (int a = 0; a < B.nact; a++) ok = ok && B.sc(a, O_PART) != 0.0;
        for (int c = 0; c < B.nc; c++) ok = ok && isfinite(B.cdx[c]);
        B.misc[M_FLAG] = ok ? 1.0 : 0.0;
    }
    __syncthreads();
    return B.misc[M_FLAG] != 0.0;
}

__device__ double ba_model(const BA &B) {
    const int t = threadIdx.x;
    for (int a = t; a < B.nact; a += kLanes) {
        const int j = B.act[a];
        const isv_sfm_track_t &T = B.tr[j];
        double mp = 0;
        for (int k = 0; k < T.n_obs; k++) {
            const int f = T.start_frame + k, co = B.coff(f), nf = B.ncf(f);
            double r[2], E[6], F[12];
            B.EF(B.cq, B.ct, B.X + 3 * j, j, f, B.obs + 2 * (T.obs_off + k), r, E, F);
            for (int row = 0; row < 2; row++) {
                double m = E[row * 3] * B.sc(j, O_DX) + E[row * 3 + 1] * B.sc(j, O_DX + 1) + E[row * 3 + 2] * B.sc(j, O_DX + 2);
                double fy = 0;
                for (int c = 0; c < nf; c++) fy += F[row * 6 + c] * B.cdx[co + c];
                m += fy;
                mp += m * (r[row] + m / 2.0);
            }
        }
        B.sc(a, O_PART) = mp;
    }
    __syncthreads();
    if (t == 0) {
        double mc = 0;
        for (int a = 0; a < B.nact; a++) mc += B.sc(a, O_PART);
        B.misc[M_SCAL] = -mc;
    }
    __syncthreads();
    return B.misc[M_SCAL];
}

// TrustRegionMinimizer + LevenbergMarquardtStrategy (the restatement's ba_solve); every lane keeps the same scalar state
__device__ void ba_solve(const BA &B, isv_sfm_result_t *out, int max_it) {
    const int t = threadIdx.x, nc = B.nc;
    double radius = 1e4, decrease_factor = 2.0;
    int reuse = 0, invalid = 0, it = 0, term = ISV_TERM_RUNNING, nsucc = 0;
    for (int a = t; a < B.nact; a += kLanes) for (int k = 0; k < 3; k++) B.sc(B.act[a], O_SC + k) = 1.0;
    for (int k = t; k < nc; k += kLanes) B.csc[k] = 1.0;
    __syncthreads();
    double x_cost = ba_cost(B, B.cq, B.ct, B.X, 3);
    ba_colnorm(B, true);
    for (int a = t; a < B.nact; a += kLanes) for (int k = 0; k < 3; k++) { const int j = B.act[a]; B.sc(j, O_SC + k) = 1.0 / (1.0 + sqrt(B.sc(j, O_DG + k))); }
    for (int k = t; k < nc; k += kLanes) B.csc[k] = 1.0 / (1.0 + sqrt(B.cdiag[k]));
    __syncthreads();
    double gmax = ba_gmax(B);
    double x_norm = sqrt(ba_norm2(B, B.cq, B.ct, B.X, 3, nullptr, nullptr, nullptr, 0));
    if (t == 0) out->ba_initial_cost = x_cost;
    for (;;) {
        if (it >= max_it) { term = ISV_TERM_MAX_ITERATIONS; break; }   // 50, or the handle's ISV_DEBUG_SFM_BA_ITERS
        if (gmax <= 1e-10) { term = ISV_TERM_GRADIENT_TOL; break; }
        if (radius <= 1e-32) { term = ISV_TERM_MIN_RADIUS; break; }
        it++;
        if (!reuse) {
            ba_colnorm(B, false);
            for (int a = t; a < B.nact; a += kLanes) for (int k = 0; k < 3; k++) { const int j = B.act[a]; B.sc(j, O_DG + k) = fmin(fmax(B.sc(j, O_DG + k), 1e-6), 1e32); }
            for (int k = t; k < nc; k += kLanes) B.cdiag[k] = fmin(fmax(B.cdiag[k], 1e-6), 1e32);
        }
        reuse = 1;
        for (int a = t; a < B.nact; a += kLanes) for (int k = 0; k < 3; k++) { const int j = B.act[a]; B.sc(j, O_D + k) = sqrt(B.sc(j, O_DG + k) / radius); }
        for (int k = t; k < nc; k += kLanes) B.cD[k] = sqrt(B.cdiag[k] / radius);
        __syncthreads();
        bool ls_fail = ba_schur(B) != 0;
        if (!ls_fail) ls_fail = !ba_finite(B);
        double mcc = 0;
        bool valid = false;
        if (!ls_fail) { mcc = ba_model(B); valid = mcc > 0.0; }
        if (!valid) {
            if (++invalid >= 5) { term = ls_fail ? ISV_TERM_LINEAR_SOLVER : ISV_TERM_INVALID_STEPS; break; }
            radius /= decrease_factor; decrease_factor *= 2.0; reuse = 1;
            continue;
        }
        invalid = 0;
        for (int a = t; a < B.nact; a += kLanes) {   // delta = step * scale, candidate points
            const int j = B.act[a];
            for (int k = 0; k < 3; k++) { B.sc(j, O_DL + k) = B.sc(j, O_DX + k) * B.sc(j, O_SC + k); B.sc(j, O_XC + k) = B.X[3 * j + k] + B.sc(j, O_DL + k); }
        }
        for (int k = t; k < nc; k += kLanes) B.cdel[k] = B.cdx[k] * B.csc[k];
        __syncthreads();
        for (int f = t; f < B.nw; f += kLanes) {
            const int co = B.coff(f);
            if (B.ncf(f) >= 3) quat_plus(B.cq + 4 * f, B.cdel + co, B.cqc + 4 * f); else for (int k = 0; k < 4; k++) B.cqc[4 * f + k] = B.cq[4 * f + k];
            if (B.ncf(f) == 6) for (int k = 0; k < 3; k++) B.ctc[3 * f + k] = B.ct[3 * f + k] + B.cdel[co + 3 + k];
            else for (int k = 0; k < 3; k++) B.ctc[3 * f + k] = B.ct[3 * f + k];
        }
        __syncthreads();
        const double cand_cost = ba_cost(B, B.cqc, B.ctc, B.scr + O_XC, kScr);
        const double step_norm = sqrt(ba_norm2(B, B.cq, B.ct, B.X, 3, B.cqc, B.ctc, B.scr + O_XC, kScr));
        if (step_norm <= 1e-8 * (x_norm + 1e-8)) { term = ISV_TERM_PARAMETER_TOL; break; }
        if (fabs(x_cost - cand_cost) <= 1e-6 * x_cost) { term = ISV_TERM_FUNCTION_TOL; break; }
        const double rel = (x_cost - cand_cost) / mcc;
        if (rel > 1e-3) {
            for (int a = t; a < B.nact; a += kLanes) { const int j = B.act[a]; for (int k = 0; k < 3; k++) B.X[3 * j + k] = B.sc(j, O_XC + k); }
            for (int k = t; k < 4 * B.nw; k += kLanes) B.cq[k] = B.cqc[k];
            for (int k = t; k < 3 * B.nw; k += kLanes) B.ct[k] = B.ctc[k];
            __syncthreads();
            x_norm = sqrt(ba_norm2(B, B.cq, B.ct, B.X, 3, nullptr, nullptr, nullptr, 0));
            x_cost = cand_cost;
            ba_colnorm(B, true);
            gmax = ba_gmax(B);
            radius = radius / fmax(1.0 / 3.0, 1.0 - pow(2.0 * rel - 1.0, 3.0));
            radius = fmin(1e16, radius); decrease_factor = 2.0; reuse = 0;
            nsucc++;
        } else { radius /= decrease_factor; decrease_factor *= 2.0; reuse = 1; }
    }
    if (t == 0) { out->ba_iterations = it; out->ba_termination = term; out->ba_final_cost = x_cost; out->ba_successful = nsucc; }
    __syncthreads();
}

__device__ void pose12(const double *R, const double *t, double *P) {
    for (int a = 0; a < 3; a++) { for (int b = 0; b < 3; b++) P[a * 4 + b] = R[a * 3 + b]; P[a * 4 + 3] = t[a]; }
}

}  // namespace

extern __shared__ double isv_sfm_lds[];

__global__ void __launch_bounds__(kLanes) k_sfm(const SfmHdr *__restrict__ hdrs, const isv_sfm_track_t *__restrict__ tracks, const double *__restrict__ obs_g,
                                                const int32_t *__restrict__ pt_off_g, const int32_t *__restrict__ pt_trk_g, const double *__restrict__ pt_uv_g,
                                                const double *__restrict__ dv_g, const double *__restrict__ sdt_g, double *__restrict__ scratch,
                                                isv_sfm_result_t *__restrict__ results, double *__restrict__ pos_out, int32_t *__restrict__ st_out,
                                                int nt_max, int no_max, int nS, int ba_max_it) {
    const SfmHdr &H = hdrs[blockIdx.x];
    isv_sfm_result_t *res = results + blockIdx.x;
    const int t = threadIdx.x;
    if (t == 0) res->fail_frame = -1;
    if (H.status != ISV_SFM_OK) {
        if (t == 0) res->status = H.status;
        return;
    }
    const int nw = H.nw, nf = H.nf, l = H.l, last = nw - 1, ntr = H.ntr;
    const isv_sfm_track_t *tr = tracks + H.trk_off;
    double *scr = scratch + H.scr_off;
    // LDS carve-up for the batch's largest problem (the launch sized it the same way)
    double *Lobs = isv_sfm_lds, *X = Lobs + 2 * no_max, *S = X + 3 * nt_max, *cq = S + nS, *ct = cq + 4 * ISV_ALIGN_MAX_WINDOW;
    double *cqc = ct + 3 * ISV_ALIGN_MAX_WINDOW, *ctc = cqc + 4 * ISV_ALIGN_MAX_WINDOW, *cR = ctc + 3 * ISV_ALIGN_MAX_WINDOW;
    double *Qo = cR + 9 * ISV_ALIGN_MAX_WINDOW, *To = Qo + 4 * ISV_ALIGN_MAX_WINDOW, *csc = To + 3 * ISV_ALIGN_MAX_WINDOW;
    double *cD = csc + kNC, *cdiag = cD + kNC, *cg = cdiag + kNC, *cdx = cg + kNC, *cdel = cdx + kNC, *rhs = cdel + kNC, *misc = rhs + kNC;
    int16_t *act = (int16_t *)(misc + M_END);
    uint8_t *st = (uint8_t *)(act + ((nt_max + 3) & ~3));
    double *pm = misc + M_PNP;

    for (int k = t; k < 2 * H.nobs; k += kLanes) Lobs[k] = obs_g[2 * (size_t)H.obs_off + k];
    for (int j = t; j < ntr; j += kLanes) st[j] = 0;

    // ---- stage 0: checkIMUExcitation (lane 0) ----
    if (t == 0) {
        const double var = isv_excitation_var(nf, dv_g + 3 * (size_t)H.frame_off, sdt_g + H.frame_off);   // S1 (isv_init_common.h)
        res->excitation_var = var;
        misc[M_FLAG] = var < 0.25 ? 1.0 : 0.0;
        // ---- stage 1 set-up: frames l and last ----
        double ql[4] = {1, 0, 0, 0}, qr[4], qlast[4], v[3];
        const double zero[3] = {0, 0, 0};
        eq_from_R(H.relR, qr);
        eq_mul(ql, qr, qlast);
        eq_inv(ql, cq + 4 * l);
        eq_to_R(cq + 4 * l, cR + 9 * l);
        mv3(cR + 9 * l, zero, v);
        for (int k = 0; k < 3; k++) ct[3 * l + k] = -1.0 * v[k];
        eq_inv(qlast, cq + 4 * last);
        eq_to_R(cq + 4 * last, cR + 9 * last);
        mv3(cR + 9 * last, H.relT, v);
        for (int k = 0; k < 3; k++) ct[3 * last + k] = -1.0 * v[k];
    }
    __syncthreads();
    if (misc[M_FLAG] != 0.0) {
        if (t == 0) res->status = ISV_SFM_REFUSED_EXCITATION;
        return;
    }

    // solveFrameByPnP(i) guessing from frame g (lanes: the LM); false below 10 points (S3)
    auto sfm_pnp = [&](int i, int g) -> bool {
        if (t == 0) {   // tracks with a position seen in frame i, in track order (S8), float-rounded (S2)
            int n = 0;
            for (int j = 0; j < ntr; j++) {
                const isv_sfm_track_t &T = tr[j];
                if (!st[j] || !in_frame(T, i)) continue;
                const double *uv = Lobs + 2 * (T.obs_off + i - T.start_frame);
                double *P = scr + (size_t)n * kScr + O_PNP;
                for (int k = 0; k < 3; k++) P[k] = (double)(float)X[3 * j + k];
                P[3] = (double)(float)uv[0]; P[4] = (double)(float)uv[1];
                n++;
            }
            misc[M_N] = n;
            res->sfm_pnp_points[i] = n;
            rodrigues_m2v(cR + 9 * g, pm + P_PAR);
            for (int k = 0; k < 3; k++) pm[P_PAR + 3 + k] = ct[3 * g + k];
        }
        __syncthreads();
        const int n = (int)misc[M_N];
        if (n < 10) return false;
        const int iters = pnp_solve(n, scr + O_PNP, kScr, pm, S);
        if (t == 0) {
            res->sfm_pnp_iterations[i] = iters;
            rodrigues_v2m(pm + P_PAR, cR + 9 * i, nullptr);
            for (int k = 0; k < 3; k++) ct[3 * i + k] = pm[P_PAR + 3 + k];
            eq_from_R(cR + 9 * i, cq + 4 * i);
        }
        __syncthreads();
        return true;
    };
    // triangulateTwoFrames(f0, f1): a lane per track
    auto tri_two = [&](int f0, int f1) {
        double P0[12], P1[12];
        pose12(cR + 9 * f0, ct + 3 * f0, P0);
        pose12(cR + 9 * f1, ct + 3 * f1, P1);
        for (int j = t; j < ntr; j += kLanes) {
            const isv_sfm_track_t &T = tr[j];
            if (st[j] || !in_frame(T, f0) || !in_frame(T, f1)) continue;
            triangulate(P0, P1, Lobs + 2 * (T.obs_off + f0 - T.start_frame), Lobs + 2 * (T.obs_off + f1 - T.start_frame), X + 3 * j);
            st[j] = 1;
        }
        __syncthreads();
    };

    // ---- stage 1: GlobalSFM::construct, steps 1-5 ----
    for (int i = l; i < last; i++) {
        if (i > l && !sfm_pnp(i, i - 1)) {
            if (t == 0) { res->fail_frame = i; res->status = ISV_SFM_REFUSED_SFM_PNP_POINTS; }
            return;
        }
        tri_two(i, last);
    }
    for (int i = l + 1; i < last; i++) tri_two(l, i);
    for (int i = l - 1; i >= 0; i--) {
        if (!sfm_pnp(i, i + 1)) {
            if (t == 0) { res->fail_frame = i; res->status = ISV_SFM_REFUSED_SFM_PNP_POINTS; }
            return;
        }
        tri_two(i, l);
    }
    for (int j = t; j < ntr; j += kLanes) {   // step 5: first and last observation, no cheirality check (S5)
        const isv_sfm_track_t &T = tr[j];
        if (st[j] || T.n_obs < 2) continue;
        const int f0 = T.start_frame, f1 = T.start_frame + T.n_obs - 1;
        double P0[12], P1[12];
        pose12(cR + 9 * f0, ct + 3 * f0, P0);
        pose12(cR + 9 * f1, ct + 3 * f1, P1);
        triangulate(P0, P1, Lobs + 2 * T.obs_off, Lobs + 2 * (T.obs_off + T.n_obs - 1), X + 3 * j);
        st[j] = 1;
    }
    __syncthreads();

    // ---- stage 2: the full BA ----
    if (t == 0) {
        int na = 0, nres = 0;
        for (int j = 0; j < ntr; j++) if (st[j]) { act[na++] = (int16_t)j; nres += 2 * tr[j].n_obs; }
        misc[M_N] = na;
        res->ba_residuals = nres;
        res->n_triangulated = na;
        res->n_ba_cols = 6 * nw - 9;
    }
    __syncthreads();
    BA B;
    B.tr = tr; B.obs = Lobs; B.X = X; B.scr = scr; B.act = act;
    B.nact = (int)misc[M_N]; B.nw = nw; B.l = l; B.nc = 6 * nw - 9;
    B.cq = cq; B.ct = ct; B.cqc = cqc; B.ctc = ctc; B.csc = csc; B.cD = cD; B.cdiag = cdiag; B.cg = cg; B.cdx = cdx; B.cdel = cdel;
    B.rhs = rhs; B.S = S; B.misc = misc;
    ba_solve(B, res, ba_max_it);
    for (int j = t; j < ntr; j += kLanes) {
        st_out[H.trk_off + j] = st[j];
        for (int k = 0; k < 3; k++) pos_out[3 * ((size_t)H.trk_off + j) + k] = st[j] ? X[3 * j + k] : 0.0;
    }
    {
        const int term = res->ba_termination;   // written by lane 0 before ba_solve's last barrier
        const bool conv = term == ISV_TERM_GRADIENT_TOL || term == ISV_TERM_PARAMETER_TOL || term == ISV_TERM_FUNCTION_TOL || term == ISV_TERM_MIN_RADIUS;
        if (!(conv || res->ba_final_cost < 5e-3)) {
            if (t == 0) res->status = ISV_SFM_REFUSED_BA_NOT_CONVERGED;
            return;
        }
    }
    if (t == 0)
        for (int f = 0; f < nw; f++) {   // q = q.inverse() (S6); T = -(q * t)
            double v[3];
            eq_inv(cq + 4 * f, Qo + 4 * f);
            eq_transform(Qo + 4 * f, ct + 3 * f, v);
            for (int k = 0; k < 3; k++) To[3 * f + k] = -1.0 * v[k];
            res->Q[f][0] = Qo[4 * f + 1]; res->Q[f][1] = Qo[4 * f + 2]; res->Q[f][2] = Qo[4 * f + 3]; res->Q[f][3] = Qo[4 * f];
            for (int k = 0; k < 3; k++) res->T[f][k] = To[3 * f + k];
        }
    __syncthreads();

    // ---- stage 4: the all-frame PnP, frame after frame ----
    const int32_t *poff = pt_off_g + H.pt_off_off;
    const int32_t *ptrk = pt_trk_g + H.pt_base;
    const double *puv = pt_uv_g + 2 * (size_t)H.pt_base;
    for (int f = 0, i = 0; f < nf; f++) {
        if (f == H.win[i]) {
            if (t == 0) {
                double R[9];
                eq_to_R(Qo + 4 * i, R);
                mmT3(R, H.RIC, res->R[f]);
                for (int k = 0; k < 3; k++) res->Tf[f][k] = To[3 * i + k];
                res->is_key_frame[f] = 1;
            }
            i++;
            continue;
        }
        if (f > H.win[i]) i++;   // S4 (never true on valid input: i already names the next keyframe)
        if (t == 0) {
            double qi[4], Ri[9], Pi[3];
            eq_inv(Qo + 4 * i, qi);
            eq_to_R(qi, Ri);
            mv3(Ri, To + 3 * i, Pi);
            for (int k = 0; k < 3; k++) pm[P_PAR + 3 + k] = -Pi[k];
            rodrigues_m2v(Ri, pm + P_PAR);
            int n = 0;
            for (int k = poff[f]; k < poff[f + 1]; k++) {   // ascending feature_id (S8)
                const int j = ptrk[k];
                if (j < 0 || !st[j]) continue;
                double *P = scr + (size_t)n * kScr + O_PNP;
                for (int c = 0; c < 3; c++) P[c] = (double)(float)X[3 * j + c];   // S2
                P[3] = (double)(float)puv[2 * k]; P[4] = (double)(float)puv[2 * k + 1];
                n++;
            }
            misc[M_N] = n;
            res->pnp_points[f] = n;
        }
        __syncthreads();
        const int n = (int)misc[M_N];
        if (n < 6) {   // S3
            if (t == 0) { res->fail_frame = f; res->status = ISV_SFM_REFUSED_ALL_PNP_POINTS; }
            return;
        }
        const int iters = pnp_solve(n, scr + O_PNP, kScr, pm, S);
        if (t == 0) {
            double r[9], Rp[9], Tp[3], mt[3];
            res->pnp_iterations[f] = iters;
            rodrigues_v2m(pm + P_PAR, r, nullptr);
            for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) Rp[a * 3 + b] = r[b * 3 + a];
            for (int k = 0; k < 3; k++) mt[k] = -pm[P_PAR + 3 + k];
            mv3(Rp, mt, Tp);
            mmT3(Rp, H.RIC, res->R[f]);
            for (int k = 0; k < 3; k++) res->Tf[f][k] = Tp[k];
            res->is_key_frame[f] = 0;
        }
        __syncthreads();
    }
    if (t == 0) res->status = ISV_SFM_OK;
}

namespace {

size_t lds_bytes(int nt_max, int no_max, int nS) {
    return sizeof(double) * ((size_t)2 * no_max + 3 * (size_t)nt_max + nS + 30 * ISV_ALIGN_MAX_WINDOW + 7 * kNC + M_END) +
           sizeof(int16_t) * (size_t)((nt_max + 3) & ~3) + (size_t)nt_max;
}

}  // namespace

// the host-side refusals: capacity, then the shape of the input (isv_sfm.h); the relative-pose stage (isv_relpose.hip) runs
// the same checks with_l = false, as it does not read l
int isv_sfm_check_problem(const isv_sfm_problem_t *p, bool with_l) {
    if (p->n_window > ISV_ALIGN_MAX_WINDOW || p->n_frames > ISV_ALIGN_MAX_FRAMES || p->n_tracks > ISV_SFM_MAX_TRACKS || p->n_obs > ISV_SFM_MAX_OBS)
        return ISV_SFM_REFUSED_CAPACITY;
    if (p->n_window < 2 || p->n_frames < 2 || (with_l && (p->l < 0 || p->l >= p->n_window - 1)) || p->n_tracks < 0 || p->n_obs < 0 || p->n_pts < 0)
        return ISV_SFM_REFUSED_INPUT;
    if ((p->n_tracks && (!p->tracks || !p->obs)) || !p->pt_off || (p->n_pts && (!p->pt_id || !p->pt_uv)) || !p->delta_v || !p->sum_dt)
        return ISV_SFM_REFUSED_INPUT;
    if (p->n_tracks && (!p->position || !p->state)) return ISV_SFM_REFUSED_INPUT;
    for (int i = 0; i < p->n_window; i++) {
        const int w = p->window_frame[i];
        if (w < 0 || w >= p->n_frames || (i > 0 && w <= p->window_frame[i - 1])) return ISV_SFM_REFUSED_INPUT;
    }
    if (p->window_frame[p->n_window - 1] != p->n_frames - 1) return ISV_SFM_REFUSED_INPUT;
    for (int j = 0; j < p->n_tracks; j++) {
        const isv_sfm_track_t &T = p->tracks[j];
        if (T.n_obs < 1 || T.start_frame < 0 || T.start_frame + T.n_obs > p->n_window || T.obs_off < 0 || T.obs_off + T.n_obs > p->n_obs)
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

extern "C" int isv_internal_sfm_last_ms(isv_backend_t *h, double out_ms[2]) { return init_last_ms(h, ISV_INIT_SFM, out_ms); }

extern "C" int isv_internal_sfm_batch(isv_backend_t *h, int32_t n, const isv_sfm_problem_t *const *problems, isv_sfm_result_t *results) {
    StageCall call{init_ctx(h, ISV_INIT_SFM), "isv_internal_sfm_batch"};
    if (const int rc = call.enter(n, problems, results); rc != ISV_OK || n == 0) return rc;
    std::vector<SfmHdr> hd(n);
    size_t n_tr = 0, n_obs = 0, n_poff = 0, n_pts = 0, n_fr = 0;
    int nt_max = 1, no_max = 1, nw_max = 2;
    for (int i = 0; i < n; i++) {
        const isv_sfm_problem_t *p = problems[i];
        SfmHdr &H = hd[i];
        memset(&H, 0, sizeof(H));
        H.status = isv_sfm_check_problem(p, true);
        if (H.status != ISV_SFM_OK) continue;
        H.nw = p->n_window; H.nf = p->n_frames; H.l = p->l; H.ntr = p->n_tracks; H.nobs = p->n_obs; H.npts = p->n_pts;
        H.trk_off = (int32_t)n_tr; H.obs_off = (int32_t)n_obs; H.pt_off_off = (int32_t)n_poff; H.pt_base = (int32_t)n_pts; H.frame_off = (int32_t)n_fr;
        H.scr_off = (int64_t)n_tr * kScr;
        for (int k = 0; k < H.nw; k++) H.win[k] = p->window_frame[k];
        for (int k = 0; k < 9; k++) { H.relR[k] = p->relative_R[k]; H.RIC[k] = p->RIC[k]; }
        for (int k = 0; k < 3; k++) H.relT[k] = p->relative_T[k];
        n_tr += p->n_tracks; n_obs += p->n_obs; n_poff += p->n_frames + 1; n_pts += p->n_pts; n_fr += p->n_frames;
        nt_max = std::max(nt_max, (int)p->n_tracks); no_max = std::max(no_max, (int)p->n_obs); nw_max = std::max(nw_max, (int)p->n_window);
    }
    if (n_tr > INT32_MAX || n_obs > INT32_MAX || n_pts > INT32_MAX || n_poff > INT32_MAX) return call.fail(ISV_ERR_CAPACITY, "batch too large");
    // one upload block: [headers | tracks | obs | dv | sdt | pt_uv | pt_off | pt_trk]; then, device only: results, positions,
    // states (the three zeroed before the launch), the per-track blocks
    BlockLayout L;
    const size_t o_hd = L.add(sizeof(SfmHdr) * n), o_tr = L.add(sizeof(isv_sfm_track_t) * (n_tr + 1)), o_obs = L.add(16 * (n_obs + 1));
    const size_t o_dv = L.add(24 * (n_fr + 1)), o_sdt = L.add(8 * (n_fr + 1)), o_uv = L.add(16 * (n_pts + 1)), o_poff = L.add(4 * (n_poff + 1));
    const size_t o_ptrk = L.add(4 * (n_pts + 1));
    std::vector<char> up(L.end);
    const size_t o_res = L.add(sizeof(isv_sfm_result_t) * n), o_pos = L.add(24 * (n_tr + 1)), o_st = L.add(4 * (n_tr + 1));
    const size_t o_scr = L.add(sizeof(double) * kScr * (n_tr + 1));
    memcpy(up.data() + o_hd, hd.data(), sizeof(SfmHdr) * n);
    std::unordered_map<int32_t, int32_t> last_of;
    for (int i = 0; i < n; i++) {
        const SfmHdr &H = hd[i];
        if (H.status != ISV_SFM_OK) continue;
        const isv_sfm_problem_t *p = problems[i];
        if (H.ntr) memcpy(up.data() + o_tr + sizeof(isv_sfm_track_t) * H.trk_off, p->tracks, sizeof(isv_sfm_track_t) * H.ntr);
        if (H.nobs) memcpy(up.data() + o_obs + 16 * (size_t)H.obs_off, p->obs, 16 * (size_t)H.nobs);
        memcpy(up.data() + o_dv + 24 * (size_t)H.frame_off, p->delta_v, 24 * (size_t)H.nf);
        memcpy(up.data() + o_sdt + 8 * (size_t)H.frame_off, p->sum_dt, 8 * (size_t)H.nf);
        if (H.npts) memcpy(up.data() + o_uv + 16 * (size_t)H.pt_base, p->pt_uv, 16 * (size_t)H.npts);
        memcpy(up.data() + o_poff + 4 * (size_t)H.pt_off_off, p->pt_off, 4 * (size_t)(H.nf + 1));
        // sfm_tracked_points.find(feature_id): the track of that id (a map assignment: the last track of an id wins)
        last_of.clear();
        for (int j = 0; j < H.ntr; j++) last_of[p->tracks[j].id] = j;
        int32_t *trk = (int32_t *)(up.data() + o_ptrk) + H.pt_base;
        for (int k = 0; k < H.npts; k++) {
            auto it = last_of.find(p->pt_id[k]);
            trk[k] = it == last_of.end() ? -1 : it->second;
        }
    }
    const int nc_max = 6 * nw_max - 9;
    const int nS = std::max(nc_max * (nc_max + 1) / 2, kLanes * 14);
    const size_t lds = lds_bytes(nt_max, no_max, nS);
    HIPCHK(h, isv_raise_dynamic_lds((const void *)k_sfm, h->device, lds));
    std::vector<double> pos(3 * (n_tr + 1));
    std::vector<int32_t> st(n_tr + 1);
    return call.run(
        up, {{up.size(), o_scr}}, L.end,
        [&](char *d, auto &&) {
            hipLaunchKernelGGL(k_sfm, dim3(n), dim3(kLanes), lds, h->stream, (const SfmHdr *)(d + o_hd), (const isv_sfm_track_t *)(d + o_tr),
                               (const double *)(d + o_obs), (const int32_t *)(d + o_poff), (const int32_t *)(d + o_ptrk), (const double *)(d + o_uv),
                               (const double *)(d + o_dv), (const double *)(d + o_sdt), (double *)(d + o_scr), (isv_sfm_result_t *)(d + o_res),
                               (double *)(d + o_pos), (int32_t *)(d + o_st), nt_max, no_max, nS, h->sfm_ba_iters);
        },
        {{results, o_res, sizeof(isv_sfm_result_t) * n}, {pos.data(), o_pos, 24 * n_tr}, {st.data(), o_st, 4 * n_tr}},
        [&] {
            for (int i = 0; i < n; i++) {   // per-track outputs of the problems that reached the BA
                const SfmHdr &H = hd[i];
                const int s = results[i].status;
                if (H.status != ISV_SFM_OK || !(s == ISV_SFM_OK || s == ISV_SFM_REFUSED_BA_NOT_CONVERGED || s == ISV_SFM_REFUSED_ALL_PNP_POINTS)) continue;
                memcpy(problems[i]->position, pos.data() + 3 * (size_t)H.trk_off, 24 * (size_t)H.ntr);
                memcpy(problems[i]->state, st.data() + H.trk_off, 4 * (size_t)H.ntr);
            }
            return hipSuccess;
        });
}
