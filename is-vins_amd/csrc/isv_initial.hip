// isv_initial.hip -- VisualIMUAlignment + the state rebuild of visualInitialAlign, batched: one 64-lane workgroup per problem
// (isv_initial.h -- internal, not part of the public ABI -- has the contract, the reference lines and the quirks Q1-Q3).
//
// Per problem, in LDS (dynamic, sized by the batch's largest all_image_frame):
//   the frames' R / T and repropagated delta_p / delta_v / sum_dt; the per-pair normal blocks r_A / r_b; the reduced system
//   A (packed lower triangle, kept across RefineGravity's passes: quirk Q2) and its LDLT factor, which shares its space with
//   the pair blocks (they are dead once assembled).
// Lanes: one per frame (repropagation), one per frame pair (the 6 x m rows and their normal blocks), entry-strided for the
// assembly, row-strided for the LDLT's column updates; the pivot search, the dot products of the triangular solves and the
// small closed-form steps run on lane 0.  Every sum runs serially in index order and every assembled entry adds its pairs in
// pair order, so the result does not depend on the batch, and matches tests/native/isv_init_oracle.c operation by operation.
// No atomics.  Contraction is off for the whole translation unit, the included quaternion / rotation helpers of
// isv_device_math.h included, as the restatement is built with -ffp-contract=off.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <float.h>
#include <string.h>
#include <vector>
#include "isv_stage_launch.h"
#include "isv_device_math.h"
#include "isv_initial.h"

namespace {

constexpr int kLanes = 64;

struct ProbHdr {                  // host-packed per-problem record
    int32_t status;               // ISV_ALIGN_OK or the host-side refusal (capacity / input)
    int32_t nf, nw;
    int32_t frame_off;            // into the batch's frame array
    int32_t imu_off;              // into the batch's imu rows
    int32_t kv_frame[ISV_ALIGN_MAX_WINDOW];   // all_image_frame index of the kv-th keyframe (quirk Q3)
    int32_t win[ISV_ALIGN_MAX_WINDOW];
    int32_t _pad;
    double G[3], tic[3];
    double Bgs[ISV_ALIGN_MAX_WINDOW][3];
};

__device__ __forceinline__ int pk(int r, int c) { return r * (r + 1) / 2 + c; }   // packed lower, r >= c

__device__ __forceinline__ void normalized3(const double *v, double *o) {   // Eigen normalized()
    double z = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    if (z > 0) { double n = sqrt(z); o[0] = v[0] / n; o[1] = v[1] / n; o[2] = v[2] / n; }
    else { o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; }
}

// Eigen 3.3 LDLT<Lower> (ldlt_inplace<Lower>::unblocked) on the packed n x n matrix L, then its solve of x in place.
// tr: n ints, temp: n doubles of LDS.
__device__ void ldlt_solve_wg(double *L, int n, double *x, int *tr, double *temp) {
    const int t = threadIdx.x;
    for (int k = 0; k < n; k++) {
        if (t == 0) {   // largest |diagonal| of the trailing block (not yet updated), first on ties
            int p = k;
            double best = fabs(L[pk(k, k)]);
            for (int i = k + 1; i < n; i++) {
                double v = fabs(L[pk(i, i)]);
                if (v > best) { best = v; p = i; }
            }
            tr[k] = p;
        }
        __syncthreads();
        const int p = tr[k];
        if (p != k) {   // the transposition, lower triangle only; the four element sets are disjoint
            for (int j = t; j < k; j += kLanes) { double a = L[pk(k, j)]; L[pk(k, j)] = L[pk(p, j)]; L[pk(p, j)] = a; }
            for (int i = p + 1 + t; i < n; i += kLanes) { double a = L[pk(i, k)]; L[pk(i, k)] = L[pk(i, p)]; L[pk(i, p)] = a; }
            for (int i = k + 1 + t; i < p; i += kLanes) { double a = L[pk(i, k)]; L[pk(i, k)] = L[pk(p, i)]; L[pk(p, i)] = a; }
            if (t == 0) { double a = L[pk(k, k)]; L[pk(k, k)] = L[pk(p, p)]; L[pk(p, p)] = a; }
            __syncthreads();
        }
        for (int j = t; j < k; j += kLanes) temp[j] = L[pk(j, j)] * L[pk(k, j)];
        __syncthreads();
        if (t == 0) {
            double dot = 0;
            for (int j = 0; j < k; j++) dot += L[pk(k, j)] * temp[j];
            L[pk(k, k)] -= dot;
        }
        for (int i = k + 1 + t; i < n; i += kLanes) {
            double s = 0;
            for (int j = 0; j < k; j++) s += L[pk(i, j)] * temp[j];
            L[pk(i, k)] -= s;
        }
        __syncthreads();
        const double akk = L[pk(k, k)];
        if (fabs(akk) > 0.0)
            for (int i = k + 1 + t; i < n; i += kLanes) L[pk(i, k)] /= akk;
        __syncthreads();
    }
    if (t == 0) {   // P, L^-1, D^+ (|d| <= DBL_MIN -> 0), L^-T, P^T
        for (int k = 0; k < n; k++) { double a = x[k]; x[k] = x[tr[k]]; x[tr[k]] = a; }
        for (int i = 0; i < n; i++) { double s = 0; for (int j = 0; j < i; j++) s += L[pk(i, j)] * x[j]; x[i] -= s; }
        for (int i = 0; i < n; i++) { double d = L[pk(i, i)]; x[i] = fabs(d) > DBL_MIN ? x[i] / d : 0.0; }
        for (int i = n - 1; i >= 0; i--) { double s = 0; for (int j = i + 1; j < n; j++) s += L[pk(j, i)] * x[j]; x[i] -= s; }
        for (int k = n - 1; k >= 0; k--) { double a = x[k]; x[k] = x[tr[k]]; x[tr[k]] = a; }
    }
    __syncthreads();
}

// tmp_A (6 x M) / tmp_b of frame pair (i, i+1) and their normal blocks r_A = tmp_A^T tmp_A (M x M), r_b = tmp_A^T tmp_b.
// M = 10: LinearAlignment (initial_aligment.cpp:147-180); M = 9: a RefineGravity pass on the tangent basis lxly (:71-108).
template <int M>
__device__ void pair_normal(const double *Ri, const double *Rj, const double *Ti, const double *Tj, const double *dp, const double *dv,
                            double dt, const double *tic, const double *lxly, const double *g0, double *rA, double *rb) {
    double tA[6][M], tb[6];
    double RiT[9], RiTRj[9], M2[9], M1[9], dT[3], t3[3], t4[3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) RiT[a * 3 + b] = Ri[b * 3 + a];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += RiT[a * 3 + k] * Rj[k * 3 + b];
            RiTRj[a * 3 + b] = s;
        }
#pragma unroll
    for (int k = 0; k < 9; k++) { M2[k] = RiT[k] * dt * dt / 2; M1[k] = RiT[k] * dt; }
#pragma unroll
    for (int k = 0; k < 3; k++) dT[k] = Tj[k] - Ti[k];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        double s = 0, u = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) { s += RiT[a * 3 + k] * dT[k]; u += RiTRj[a * 3 + k] * tic[k]; }
        t3[a] = s; t4[a] = u;
    }
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = 0; c < M; c++) tA[r][c] = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        tA[a][a] = -dt;
        tA[3 + a][a] = -1.0;
#pragma unroll
        for (int b = 0; b < 3; b++) tA[3 + a][3 + b] = RiTRj[a * 3 + b];
        if (M == 10) {
#pragma unroll
            for (int b = 0; b < 3; b++) { tA[a][6 + b] = M2[a * 3 + b]; tA[3 + a][6 + b] = M1[a * 3 + b]; }
            tA[a][M - 1] = t3[a] / 100.0;
            tb[a] = dp[a] + t4[a] - tic[a];
            tb[3 + a] = dv[a];
        } else {
#pragma unroll
            for (int b = 0; b < 2; b++) {
                double s2 = 0, s1 = 0;
#pragma unroll
                for (int k = 0; k < 3; k++) { s2 += M2[a * 3 + k] * lxly[k * 2 + b]; s1 += M1[a * 3 + k] * lxly[k * 2 + b]; }
                tA[a][6 + b] = s2; tA[3 + a][6 + b] = s1;
            }
            tA[a][M - 1] = t3[a] / 100.0;
            double g2 = 0, g1 = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) { g2 += M2[a * 3 + k] * g0[k]; g1 += M1[a * 3 + k] * g0[k]; }
            tb[a] = dp[a] + t4[a] - tic[a] - g2;
            tb[3 + a] = dv[a] - g1;
        }
    }
#pragma unroll
    for (int i = 0; i < M; i++) {
#pragma unroll
        for (int j = 0; j < M; j++) {
            double s = 0;
#pragma unroll
            for (int r = 0; r < 6; r++) s += tA[r][i] * tA[r][j];
            rA[i * M + j] = s;
        }
        double s = 0;
#pragma unroll
        for (int r = 0; r < 6; r++) s += tA[r][i] * tb[r];
        rb[i] = s;
    }
}

// A (packed, n x n) += the pair blocks in pair order, then A *= 1000 (same for b); the pair blocks have stride PS doubles
// (M * M of r_A, then M of r_b).  An entry of the velocity part is touched by at most two pairs, the trailing (M - 6) rows by
// all of them.  A starts at 0 for LinearAlignment and at the previous pass's sum for RefineGravity (quirk Q2).
template <int M>
__device__ void assemble(double *A, double *b, int n, int nf, const double *pairs, int PS) {
    const int T = M - 6, nt = n - T, np = nf - 1;
    const int nA = n * (n + 1) / 2;
    for (int e = threadIdx.x; e < nA + n; e += kLanes) {
        if (e < nA) {
            int r = (int)((sqrt(8.0 * e + 1.0) - 1.0) / 2.0);
            while (r * (r + 1) / 2 > e) r--;
            while ((r + 1) * (r + 2) / 2 <= e) r++;
            const int c = e - r * (r + 1) / 2;
            double acc = A[e];
            if (r >= nt && c >= nt) {
                for (int i = 0; i < np; i++) acc += pairs[i * PS + (6 + r - nt) * M + 6 + c - nt];
            } else if (r >= nt) {       // bottom-left strip of the pairs whose 6 columns hold c
                for (int i = max(0, c / 3 - 1); i <= min(np - 1, c / 3); i++)
                    if (c >= 3 * i && c < 3 * i + 6) acc += pairs[i * PS + (6 + r - nt) * M + c - 3 * i];
            } else {
                for (int i = max(0, r / 3 - 1); i <= min(np - 1, r / 3); i++)
                    if (r >= 3 * i && r < 3 * i + 6 && c >= 3 * i && c < 3 * i + 6) acc += pairs[i * PS + (r - 3 * i) * M + c - 3 * i];
            }
            A[e] = acc * 1000.0;
        } else {
            const int r = e - nA;
            double acc = b[r];
            if (r >= nt) {
                for (int i = 0; i < np; i++) acc += pairs[i * PS + M * M + 6 + r - nt];
            } else {
                for (int i = max(0, r / 3 - 1); i <= min(np - 1, r / 3); i++)
                    if (r >= 3 * i && r < 3 * i + 6) acc += pairs[i * PS + M * M + r - 3 * i];
            }
            b[r] = acc * 1000.0;
        }
    }
    __syncthreads();
}

__device__ void tangent_basis(const double *g0, double *lxly) {   // TangentBasis  initial_aligment.cpp:40-53
    double a[3], tmp[3] = {0, 0, 1}, bb[3], t[3];
    normalized3(g0, a);
    if (a[0] == tmp[0] && a[1] == tmp[1] && a[2] == tmp[2]) { tmp[0] = 1; tmp[2] = 0; }
    double d = a[0] * tmp[0] + a[1] * tmp[1] + a[2] * tmp[2];
    for (int k = 0; k < 3; k++) t[k] = tmp[k] - a[k] * d;
    normalized3(t, bb);
    double c0 = a[1] * bb[2] - a[2] * bb[1], c1 = a[2] * bb[0] - a[0] * bb[2], c2 = a[0] * bb[1] - a[1] * bb[0];
    lxly[0] = bb[0]; lxly[2] = bb[1]; lxly[4] = bb[2];
    lxly[1] = c0; lxly[3] = c1; lxly[5] = c2;
}

__device__ void m3mul(const double *A, const double *B, double *C) {   // serial-sum 3x3 product (the oracle's mm)
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += A[i * 3 + k] * B[k * 3 + j];
            C[i * 3 + j] = s;
        }
}

}  // namespace

extern __shared__ double isv_align_lds[];

__global__ void __launch_bounds__(kLanes) k_visual_imu_align(const ProbHdr *__restrict__ hdrs, const isv_align_frame_t *__restrict__ frames,
                                                             const double *__restrict__ imu, isv_align_result_t *__restrict__ results, int nf_max) {
    double *lds = isv_align_lds;
    const ProbHdr &H = hdrs[blockIdx.x];
    isv_align_result_t *res = results + blockIdx.x;
    const int t = threadIdx.x;
    if (H.status != ISV_ALIGN_OK) {
        if (t == 0) res->status = H.status;
        return;
    }
    const int nf = H.nf, nw = H.nw, np = nf - 1;
    const isv_align_frame_t *F = frames + H.frame_off;
    const double *I = imu + 7 * (size_t)H.imu_off;
    const double Gn = sqrt(H.G[0] * H.G[0] + H.G[1] * H.G[1] + H.G[2] * H.G[2]);

    // LDS carve-up for nf_max frames (the launch sized it the same way)
    const int nmax = 3 * nf_max + 4, nA_max = nmax * (nmax + 1) / 2, PS = 10 * 10 + 10;
    double *fR = lds, *fT = fR + 9 * nf_max, *fdp = fT + 3 * nf_max, *fdv = fdp + 3 * nf_max, *fdt = fdv + 3 * nf_max;
    double *A = fdt + nf_max;
    double *U = A + nA_max;                                    // pair blocks, then the factor of A
    const int nU = nA_max > (nf_max - 1) * PS ? nA_max : (nf_max - 1) * PS;
    double *b = U + nU, *x = b + nmax, *temp = x + nmax, *misc = temp + nmax;   // misc: g0[3], lxly[6], bg0[3], flag
    int *tr = (int *)(misc + 16);

    for (int f = t; f < nf; f += kLanes) {
        for (int k = 0; k < 9; k++) fR[f * 9 + k] = F[f].R[k];
        for (int k = 0; k < 3; k++) fT[f * 3 + k] = F[f].T[k];
    }
    __syncthreads();

    // ---- solveGyroscopeBias (initial_aligment.cpp:3-37): pair blocks on their lanes, summed in pair order on lane 0 ----
    for (int i = t; i < np; i += kLanes) {
        const double *Ri = fR + i * 9, *Rj = fR + (i + 1) * 9;
        double Rij[9];
        for (int a = 0; a < 3; a++)
            for (int c = 0; c < 3; c++) {
                double s = 0;
                for (int k = 0; k < 3; k++) s += Ri[k * 3 + a] * Rj[k * 3 + c];
                Rij[a * 3 + c] = s;
            }
        Quat qij = q_from_R(Rij);
        const double *q4 = F[i + 1].delta_q;
        Quat e = q_mul(q_inv(qij), Quat{q4[3], q4[0], q4[1], q4[2]});
        double tb[3] = {-2.0 * e.x, -2.0 * e.y, -2.0 * e.z};
        const double *tA = F[i + 1].jac_rr;      // quirk Q1: jacobian.block<3,3>(3,3)
        double *o = U + i * 12;
        for (int a = 0; a < 3; a++) {
            for (int c = 0; c < 3; c++) { double s = 0; for (int k = 0; k < 3; k++) s += tA[k * 3 + a] * tA[k * 3 + c]; o[a * 3 + c] = s; }
            double s = 0; for (int k = 0; k < 3; k++) s += tA[k * 3 + a] * tb[k]; o[9 + a] = s;
        }
    }
    __syncthreads();
    if (t == 0) {
        double A3[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, b3[3] = {0, 0, 0};
        for (int i = 0; i < np; i++) {
            for (int k = 0; k < 9; k++) A3[k] += U[i * 12 + k];
            for (int k = 0; k < 3; k++) b3[k] += U[i * 12 + 9 + k];
        }
        for (int r = 0; r < 3; r++) for (int c = 0; c <= r; c++) A[pk(r, c)] = A3[r * 3 + c];
        for (int k = 0; k < 3; k++) x[k] = b3[k];
    }
    __syncthreads();
    ldlt_solve_wg(A, 3, x, tr, temp);
    if (t == 0)
        for (int k = 0; k < 3; k++) { res->delta_bg[k] = x[k]; misc[9 + k] = H.Bgs[0][k] + x[k]; }
    for (int i = t; i < nw; i += kLanes)
        for (int k = 0; k < 3; k++) res->Bgs[i][k] = H.Bgs[i][k] + x[k];
    __syncthreads();

    // ---- repropagate(0, Bgs[0]) of every frame after the first (integration_base.h:38-158, deltas only), a lane per frame ----
    for (int j = 1 + t; j < nf; j += kLanes) {
        const isv_align_frame_t &fr = F[j];
        const double bg[3] = {misc[9], misc[10], misc[11]};
        double acc_0[3] = {fr.linearized_acc[0], fr.linearized_acc[1], fr.linearized_acc[2]};
        double gyr_0[3] = {fr.linearized_gyr[0], fr.linearized_gyr[1], fr.linearized_gyr[2]};
        Quat dq{1, 0, 0, 0};
        double p[3] = {0, 0, 0}, v[3] = {0, 0, 0}, sdt = 0.0;
        for (int s = 0; s < fr.imu_count; s++) {
            const double *row = I + 7 * (size_t)(fr.imu_begin + s);
            const double dt = row[0];
            const double acc_1[3] = {row[1], row[2], row[3]}, gyr_1[3] = {row[4], row[5], row[6]};
            double a0[3], a1[3], ung[3], u0[3], u1[3];
            for (int k = 0; k < 3; k++) { a0[k] = acc_0[k] - 0.0; a1[k] = acc_1[k] - 0.0; ung[k] = 0.5 * (gyr_0[k] + gyr_1[k]) - bg[k]; }
            q_rot(dq, a0, u0);
            Quat rdq = q_mul(dq, Quat{1, ung[0] * dt / 2, ung[1] * dt / 2, ung[2] * dt / 2});
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
        for (int k = 0; k < 3; k++) {
            fdp[j * 3 + k] = p[k]; fdv[j * 3 + k] = v[k];
            res->rp_delta_p[j][k] = p[k]; res->rp_delta_v[j][k] = v[k];
        }
        fdt[j] = sdt; res->rp_sum_dt[j] = sdt;
        res->rp_delta_q[j][0] = dq.x; res->rp_delta_q[j][1] = dq.y; res->rp_delta_q[j][2] = dq.z; res->rp_delta_q[j][3] = dq.w;
    }
    __syncthreads();

    // ---- LinearAlignment (:128-202) ----
    int n = 3 * nf + 4;
    for (int i = t; i < np; i += kLanes)
        pair_normal<10>(fR + i * 9, fR + (i + 1) * 9, fT + i * 3, fT + (i + 1) * 3, fdp + (i + 1) * 3, fdv + (i + 1) * 3, fdt[i + 1], H.tic,
                        nullptr, nullptr, U + i * PS, U + i * PS + 100);
    for (int e = t; e < n * (n + 1) / 2; e += kLanes) A[e] = 0.0;
    for (int e = t; e < n; e += kLanes) b[e] = 0.0;
    __syncthreads();
    assemble<10>(A, b, n, nf, U, PS);
    for (int e = t; e < n; e += kLanes) x[e] = b[e];
    __syncthreads();
    ldlt_solve_wg(A, n, x, tr, temp);      // A is not needed again: factored in place
    if (t == 0) {
        const double s = x[n - 1] / 100.0, g[3] = {x[n - 4], x[n - 3], x[n - 2]};
        for (int k = 0; k < 3; k++) res->g_linear[k] = g[k];
        res->s_linear = s;
        res->n_state = n;
        int st = ISV_ALIGN_OK;
        if (fabs(sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]) - Gn) > 1.0) st = ISV_ALIGN_REFUSED_GRAVITY;
        else if (s < 0) st = ISV_ALIGN_REFUSED_SCALE;
        misc[15] = (double)st;
        double g0[3];
        normalized3(g, g0);
        for (int k = 0; k < 3; k++) misc[k] = g0[k] * Gn;
    }
    __syncthreads();
    if (misc[15] != 0.0) {
        if (t == 0) res->status = (int)misc[15];
        return;
    }

    // ---- RefineGravity (:56-126): A and b zeroed once (quirk Q2) ----
    n = 3 * nf + 3;
    for (int e = t; e < n * (n + 1) / 2; e += kLanes) A[e] = 0.0;
    for (int e = t; e < n; e += kLanes) b[e] = 0.0;
    for (int pass = 0; pass < 4; pass++) {
        if (t == 0) tangent_basis(misc, misc + 3);
        __syncthreads();
        for (int i = t; i < np; i += kLanes)
            pair_normal<9>(fR + i * 9, fR + (i + 1) * 9, fT + i * 3, fT + (i + 1) * 3, fdp + (i + 1) * 3, fdv + (i + 1) * 3, fdt[i + 1], H.tic,
                           misc + 3, misc, U + i * PS, U + i * PS + 81);
        __syncthreads();
        assemble<9>(A, b, n, nf, U, PS);
        for (int e = t; e < n * (n + 1) / 2; e += kLanes) U[e] = A[e];
        for (int e = t; e < n; e += kLanes) x[e] = b[e];
        __syncthreads();
        ldlt_solve_wg(U, n, x, tr, temp);
        if (t == 0) {
            double gn[3], g0[3];
            for (int k = 0; k < 3; k++) gn[k] = misc[k] + (misc[3 + k * 2] * x[n - 3] + misc[3 + k * 2 + 1] * x[n - 2]);
            normalized3(gn, g0);
            for (int k = 0; k < 3; k++) misc[k] = g0[k] * Gn;
        }
        __syncthreads();
    }
    if (t == 0) x[n - 1] = x[n - 1] / 100.0;
    __syncthreads();
    const double s = x[n - 1];
    for (int e = t; e < n; e += kLanes) res->x[e] = x[e];
    if (t != 0) return;
    for (int k = 0; k < 3; k++) res->g_c0[k] = misc[k];
    if (s < 0.0) { res->status = ISV_ALIGN_REFUSED_REFINED_SCALE; return; }

    // ---- visualInitialAlign's state rebuild (estimator.cpp:367-429) and Utility::g2R (utility.cpp:3-13), lane 0 ----
    const double g0[3] = {misc[0], misc[1], misc[2]};
    double R0[9];
    {
        // ng1 = g.normalized(); FromTwoVectors(ng1, (0,0,1)) normalises again: c = v1.dot(v0) = v0.z, axis = v0 x v1
        double ng1[3], v0[3];
        normalized3(g0, ng1);
        normalized3(ng1, v0);
        const double cz = v0[2];
        if (cz < -1.0 + 1e-12) { res->status = ISV_ALIGN_REFUSED_ANTIPARALLEL; return; }
        const double ax[3] = {v0[1], -v0[0], 0.0};
        const double sq = sqrt((1.0 + cz) * 2.0), invs = 1.0 / sq;
        Quat q{sq * 0.5, ax[0] * invs, ax[1] * invs, ax[2] * invs};
        double Rq[9], ypr[3], Ry[9];
        q_to_R(q, Rq);
        R2ypr(Rq, ypr);
        const double my[3] = {-ypr[0], 0, 0};
        ypr2R(my, Ry);
        m3mul(Ry, Rq, R0);
    }
    double Ps[ISV_ALIGN_MAX_WINDOW][3], Vs[ISV_ALIGN_MAX_WINDOW][3];
    const double *tic = H.tic;
    double Rt0[3], P0[3];
    const double *R00 = fR + H.win[0] * 9;
    for (int a = 0; a < 3; a++) Rt0[a] = R00[a * 3] * tic[0] + R00[a * 3 + 1] * tic[1] + R00[a * 3 + 2] * tic[2];
    for (int k = 0; k < 3; k++) P0[k] = s * fT[H.win[0] * 3 + k] - Rt0[k];
    for (int i = nw - 1; i >= 0; i--) {
        const double *Ri = fR + H.win[i] * 9;
        double Rt[3];
        for (int a = 0; a < 3; a++) Rt[a] = Ri[a * 3] * tic[0] + Ri[a * 3 + 1] * tic[1] + Ri[a * 3 + 2] * tic[2];
        for (int k = 0; k < 3; k++) Ps[i][k] = s * fT[H.win[i] * 3 + k] - Rt[k] - P0[k];
    }
    for (int kv = 0; kv < nw; kv++) {   // quirk Q3: the kv-th keyframe's R times x.segment<3>(3 kv)
        const double *Rk = fR + H.kv_frame[kv] * 9;
        for (int a = 0; a < 3; a++) Vs[kv][a] = Rk[a * 3] * x[3 * kv] + Rk[a * 3 + 1] * x[3 * kv + 1] + Rk[a * 3 + 2] * x[3 * kv + 2];
    }
    {
        double RR[9], ypr[3], Ry[9], T[9];
        m3mul(R0, R00, RR);
        R2ypr(RR, ypr);
        const double my[3] = {-ypr[0], 0, 0};
        ypr2R(my, Ry);
        m3mul(Ry, R0, T);
        for (int k = 0; k < 9; k++) R0[k] = T[k];
    }
    for (int a = 0; a < 3; a++) res->g[a] = R0[a * 3] * g0[0] + R0[a * 3 + 1] * g0[1] + R0[a * 3 + 2] * g0[2];
    res->s = s;
    for (int k = 0; k < 9; k++) res->R0[k] = R0[k];
    for (int i = 0; i < nw; i++) {
        for (int a = 0; a < 3; a++) {
            res->Ps[i][a] = R0[a * 3] * Ps[i][0] + R0[a * 3 + 1] * Ps[i][1] + R0[a * 3 + 2] * Ps[i][2];
            res->Vs[i][a] = R0[a * 3] * Vs[i][0] + R0[a * 3 + 1] * Vs[i][1] + R0[a * 3 + 2] * Vs[i][2];
        }
        double Rr[9];
        m3mul(R0, fR + H.win[i] * 9, Rr);
        for (int k = 0; k < 9; k++) res->Rs[i][k] = Rr[k];
    }
    res->status = ISV_ALIGN_OK;
}

namespace {

size_t lds_bytes(int nf_max) {
    const int nmax = 3 * nf_max + 4, nA = nmax * (nmax + 1) / 2, PS = 110;
    const int nU = nA > (nf_max - 1) * PS ? nA : (nf_max - 1) * PS;
    return sizeof(double) * ((size_t)19 * nf_max + nA + nU + 3 * nmax + 16) + sizeof(int) * nmax;
}

// the host-side refusals: capacity, then the shape of the input (isv_initial.h); fills the kv -> frame map
int check_problem(const isv_align_problem_t *p, ProbHdr *hd) {
    if (p->n_frames > ISV_ALIGN_MAX_FRAMES || p->n_window > ISV_ALIGN_MAX_WINDOW) return ISV_ALIGN_REFUSED_CAPACITY;
    if (p->n_frames < 2 || p->n_window < 1 || !p->frames || (p->n_imu > 0 && !p->imu) || p->n_imu < 0) return ISV_ALIGN_REFUSED_INPUT;
    for (int i = 0; i < p->n_window; i++) {
        int w = p->window_frame[i];
        if (w < 0 || w >= p->n_frames || (i > 0 && w <= p->window_frame[i - 1])) return ISV_ALIGN_REFUSED_INPUT;
    }
    int kf = 0;
    for (int f = 0, wi = 0; f < p->n_frames; f++) {
        const bool in_window = wi < p->n_window && p->window_frame[wi] == f;
        if (in_window) wi++;
        if (in_window || p->frames[f].is_key_frame) {
            if (kf >= p->n_window) return ISV_ALIGN_REFUSED_INPUT;
            hd->kv_frame[kf++] = f;
        }
        if (f > 0) {
            const isv_align_frame_t &fr = p->frames[f];
            if (fr.imu_begin < 0 || fr.imu_count < 0 || (int64_t)fr.imu_begin + fr.imu_count > p->n_imu) return ISV_ALIGN_REFUSED_INPUT;
        }
    }
    return kf == p->n_window ? ISV_ALIGN_OK : ISV_ALIGN_REFUSED_INPUT;
}

}  // namespace

extern "C" int isv_internal_align_last_ms(isv_backend_t *h, double out_ms[2]) { return init_last_ms(h, ISV_INIT_ALIGN, out_ms); }

extern "C" int isv_internal_visual_imu_align_batch(isv_backend_t *h, int32_t n, const isv_align_problem_t *const *problems, isv_align_result_t *results) {
    StageCall call{init_ctx(h, ISV_INIT_ALIGN), "isv_internal_visual_imu_align_batch"};
    if (const int rc = call.enter(n, problems, results); rc != ISV_OK || n == 0) return rc;
    std::vector<ProbHdr> hd(n);
    size_t n_frames = 0, n_imu = 0;
    int nf_max = 2;
    for (int i = 0; i < n; i++) {
        const isv_align_problem_t *p = problems[i];
        ProbHdr &H = hd[i];
        memset(&H, 0, sizeof(H));
        H.status = check_problem(p, &H);
        if (H.status != ISV_ALIGN_OK) continue;
        H.nf = p->n_frames; H.nw = p->n_window;
        H.frame_off = (int32_t)n_frames; H.imu_off = (int32_t)n_imu;
        for (int k = 0; k < H.nw; k++) H.win[k] = p->window_frame[k];
        for (int k = 0; k < 3; k++) { H.G[k] = p->G[k]; H.tic[k] = p->tic[k]; }
        for (int w = 0; w < H.nw; w++) for (int k = 0; k < 3; k++) H.Bgs[w][k] = p->Bgs[w][k];
        n_frames += p->n_frames; n_imu += p->n_imu;
        if (p->n_frames > nf_max) nf_max = p->n_frames;
    }
    if (n_frames > INT32_MAX || n_imu > INT32_MAX) return call.fail(ISV_ERR_CAPACITY, "batch too large");
    // one upload block: [headers | frames | imu rows]; then, device only: results
    BlockLayout L;
    const size_t o_hd = L.add(sizeof(ProbHdr) * n), o_fr = L.add(sizeof(isv_align_frame_t) * n_frames), o_imu = L.add(sizeof(double) * 7 * (n_imu ? n_imu : 1));
    std::vector<char> up(L.end);
    const size_t o_res = L.add(sizeof(isv_align_result_t) * n);
    memcpy(up.data() + o_hd, hd.data(), sizeof(ProbHdr) * n);
    for (int i = 0; i < n; i++) {
        if (hd[i].status != ISV_ALIGN_OK) continue;
        const isv_align_problem_t *p = problems[i];
        memcpy(up.data() + o_fr + sizeof(isv_align_frame_t) * hd[i].frame_off, p->frames, sizeof(isv_align_frame_t) * p->n_frames);
        if (p->n_imu) memcpy(up.data() + o_imu + sizeof(double) * 7 * hd[i].imu_off, p->imu, sizeof(double) * 7 * p->n_imu);
    }
    const size_t lds = lds_bytes(nf_max);
    HIPCHK(h, isv_raise_dynamic_lds((const void *)k_visual_imu_align, h->device, lds));
    return call.run(
        up, {{up.size(), L.end}}, L.end,
        [&](char *d, auto &&) {
            hipLaunchKernelGGL(k_visual_imu_align, dim3(n), dim3(kLanes), lds, h->stream, (const ProbHdr *)(d + o_hd), (const isv_align_frame_t *)(d + o_fr),
                               (const double *)(d + o_imu), (isv_align_result_t *)(d + o_res), nf_max);
        },
        {{results, o_res, sizeof(isv_align_result_t) * n}}, [] { return hipSuccess; });
}
