// isv_posegraph.hip -- PoseGraph::optimizeCS on the MI355X (reference src/pose_graph/pose_graph.cpp:234-428), the consumer
// of the CombinedFactors the sliding-window backend emits (C ABI: include/isvins_posegraph.h).
//
// The problem (Ceres 2.0.0 in the reference: SPARSE_NORMAL_CHOLESKY, LEVENBERG_MARQUARDT, <= 10 iterations): the poses
// of the keyframes first_looped_index .. cur_index; RelativePoseFactor chain + RollPitchFactor per keyframe + loop-closure
// RelativePoseFactors under HuberLoss(0.1); then ceres::Covariance of every pose block.
//
// Device design.  The normal equations are BLOCK SPARSE: a block-tridiagonal chain plus one long row per loop closure.
// With the keyframes in their natural order a Cholesky factor fills only inside the row ENVELOPE (row r: columns
// start[r] .. r, start[r] = its earliest neighbour), so the matrices live in skyline storage of 6x6 blocks: K chain
// blocks + sum over loop edges of (later - earlier).  ONE WAVEFRONT per pose graph runs the whole optimisation -- the
// factorisation is a recurrence along the chain, there is nothing for a second wavefront to do -- and a batch of graphs
// (one per sequence) fills the GPU: grid = graphs.  Inside the wavefront: lane per residual block for the
// linearisation (RelativePoseFactor / RollPitchFactor::Evaluate + Corrector), lane per pose for the assembly (owner
// computes, fixed adjacency order: bitwise reproducible), 36 lanes per 6x6 block product in the factorisation, the
// triangular solves and the selected inversion.  Marginal covariances = the diagonal blocks of H^-1 by the Takahashi
// recurrence on the same envelope (never a dense inverse).
// This is latency-bound sparse work (dependent 6x6 block recurrences through L2); it is not reshaped into dense GEMMs.
#include <hip/hip_runtime.h>
#include <cstdio>
#include "isv_pgo_host.h"      // the host half of the call (and PgEdge / PgGraph: isv_pgo_types.h)
#include "isv_device_math.h"
#include "isv_prior_factor.h"

// LDS-only ordering inside the wavefront (the 6x6 tiles T0 / T1 / T2): the LDS executes one wavefront's accesses in issue order,
// so all that is needed is that the compiler neither reorders them nor keeps tile values in registers.  Unlike a release
// fence this does NOT wait for outstanding global loads and stores (vmcnt): with ISV_WSYNC every step of the factorisation
// paid the latency of its own L-block store and of the next row's prefetch.
#define PG_LSYNC() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); } while (0)
// make this wavefront's global stores visible to its own later loads (other lanes read what a lane wrote)
#define PG_GSYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); } while (0)

struct PgDev {
    PgGraph *graphs;
    double *pose, *cand;         // [poses][7]
    int32_t *free_of;            // [poses] free index of a local pose or -1
    PgEdge *edges;
    double *eres, *ejac;         // [edges][6], [edges][72]: corrected residual, Jacobians (block a | block b), Jacobi-scaled
    double *Bt;                  // [free poses][36]: B_c = L_cc^-1 L(c, c-1) of every chain row c (factor(): a loop row's step through column c)
    double *red;                 // [edges][6]: per-item terms of the sums a multi-wavefront launch hands to wavefront 0 (k_pgo<4>)
    int32_t *adj_ptr, *adj;      // per free pose: the residual blocks touching it, (edge << 1) | side
    int32_t *start, *rowptr;     // skyline: first column of row r, block offset of row r   (per free pose; rowptr has nf + 1)
    int32_t *colptr, *colrows;   // column pattern: rows i > j with start[i] <= j, ascending
    double *H, *L, *Z;           // [blocks][36]
    double *scale, *diag, *grad, *step, *ysol;   // [6 nf] each
    double *cov;                 // [poses][36] tangent-space marginal covariance (zero for constant poses)
    isv_pgo_result_t *res;
    int32_t idx_lds_rows, idx_lds_cols;   // capacity of the LDS copies of start / rowptr / colptr and of colrows (0: read them from global memory)
    int32_t g0, _pad;                     // first graph of this launch (a batch call launches its graphs in chunks, round 4)
};

// ---- 6x6 helpers: lane e < 36 owns element (a, b) = (e / 6, e % 6) -------------------------------------------------
// D (6x6 SPD, row-major in LDS tile T, lower part valid) -> T = inverse of its Cholesky factor (lower); returns false if not SPD.
// chol_inv_block<6> (isv_device_math.h) with PG_LSYNC instead of ISV_WSYNC, whose fences would also wait for global memory.
DEV bool pg_chol_inv6(double *T, int lane) {
    double row[6], dinv[6], x[6];
#pragma unroll
    for (int k = 0; k < 6; k++) row[k] = lane < 6 ? T[lane * 6 + k] : 0.0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double s = row[j];
#pragma unroll
        for (int k = 0; k < j; k++) s -= row[k] * readlane_d(row[k], j);
        const double sj = readlane_d(s, j);
        if (!(sj > 0.0)) bad = true;
        dinv[j] = rsqrt_nr2(sj);
        row[j] = (lane == j) ? sj * dinv[j] : s * dinv[j];
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {                      // lane c solves L x = e_c
        double s = (lane == i) ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < i; k++) s -= readlane_d(row[k], i) * x[k];
        x[i] = s * dinv[i];
    }
    PG_LSYNC();
    if (lane < 6) {
#pragma unroll
        for (int k = 0; k < 6; k++) T[k * 6 + lane] = x[k];      // x[k] = Linv[k][lane], zero for k < lane
    }
    PG_LSYNC();
    return !bad;
}

// RelativePoseFactor::Evaluate (include/factor/relative_pose_factor.h:27-70) / RollPitchFactor::Evaluate
// (rollpitch_factor.h:26-57) of one residual block at `pose`, HuberLoss corrector applied; returns rho(s) / 2
// Every global input is read into registers before the first store and the outputs are stored at the very end: the
// compiler must keep loads behind earlier stores that may alias them, and a store -> dependent load round trip per matrix
// entry is what the first version of this kernel spent most of its time on.
DEV double pg_edge_eval(const PgEdge &E, const double *pose, double huber, double *__restrict__ r_out, double *__restrict__ Ja, double *__restrict__ Jb, bool jac) {
    double raw[6], rJa[36], rJb[36], Sq[36];
    const double *pa = pose + 7 * E.a, *pb = pose + 7 * E.b;
    const int dim = E.dim, kind = E.kind, robust = E.robust;
    // (fixed 6 x 6 shapes, zero-padded for the 2-row roll/pitch factor: constant loop bounds keep the arrays in registers,
    //  and the padding adds exact zeros to the sums)
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int k = 0; k < 6; k++) Sq[a * 6 + k] = (a < dim && k < dim) ? E.sqrt_info[a * dim + k] : 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) raw[k] = 0.0;
    if (kind == 0) {
        Quat Rq = q_normalized(q_from_pose(pa)), Rm = q_from_R(E.meas_R);
        double nZ[3] = {0, 0, -1.0}, v[3];
        q_rot(so3_mul(Rm, q_conj(Rq)), nZ, v);
        raw[0] = v[0]; raw[1] = v[1];
        if (jac) {
            double S[9], Rmm[9], Bm[9];
            skew3(v, S); q_to_R(Rm, Rmm); m3_mul(S, Rmm, Bm);
            for (int k = 0; k < 36; k++) rJa[k] = 0;
            for (int a = 0; a < 2; a++) for (int b = 0; b < 3; b++) rJa[a * 6 + 3 + b] = Bm[a * 3 + b];
        }
    } else {
        relpose_jac(E.meas_t, E.meas_R, pa, pb, raw, rJa, rJb);
    }
    double r[6];
#pragma unroll
    for (int a = 0; a < 6; a++) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < 6; k++) s += Sq[a * 6 + k] * raw[k];
        r[a] = s;
    }
    double sq = 0;
#pragma unroll
    for (int a = 0; a < 6; a++) sq += r[a] * r[a];
    double rho = sq, sc = 1.0;
    if (robust) {                                    // HuberLoss(a): rho = s (s <= a^2), 2 a sqrt(s) - a^2 beyond; Corrector scales by sqrt(rho')
        const double b2 = huber * huber;
        if (sq > b2) { const double rr = sqrt(sq); rho = 2.0 * huber * rr - b2; sc = sqrt(fmax(2.2250738585072014e-308, huber / rr)); }
    }
    if (jac) {
        double oa[36], ob[36];
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double s = 0;
#pragma unroll
                for (int k = 0; k < 6; k++) s += Sq[a * 6 + k] * rJa[k * 6 + c];
                oa[a * 6 + c] = s * sc;
            }
        if (kind != 0) {
#pragma unroll
            for (int a = 0; a < 6; a++)
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    double s = 0;
#pragma unroll
                    for (int k = 0; k < 6; k++) s += Sq[a * 6 + k] * rJb[k * 6 + c];
                    ob[a * 6 + c] = s * sc;
                }
        }
#pragma unroll
        for (int a = 0; a < 6; a++) if (a < dim) r_out[a] = r[a] * sc;
#pragma unroll
        for (int q = 0; q < 36; q++) if (q < dim * 6) Ja[q] = oa[q];
        if (kind != 0) {
#pragma unroll
            for (int q = 0; q < 36; q++) Jb[q] = ob[q];
        }
    }
    return 0.5 * rho;
}

// NW wavefronts per pose graph (round 5).  NW = 1: the batch form, a graph per wavefront.  NW = 4: a call with few graphs -- what
// PoseGraph::optimizeCS is in the reference: ONE graph, when a loop closes -- leaves the GPU idle around one wavefront per graph, so
// the loops that are lane-per-residual-block or lane-per-pose (evaluation + linearisation, column norms, scaling, gradient, assembly,
// candidate, the element-wise passes, the covariance read-out) stride over four wavefronts; the block recurrences (factor, solve,
// the selected inverse) stay on wavefront 0: row r needs row r - 1.  SAME BITS as NW = 1: the owner-computes loops have no
// cross-lane sum, and every sum over items is taken by wavefront 0 over the stored per-item terms in the order NW = 1 adds them.
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_pgo(PgDev dv) {
    __shared__ double T0[36], T1[36], T2[36];
    __shared__ double bcast_[2 + NW];
    constexpr int NT = 64 * NW;
    const int gid = blockIdx.x + dv.g0;
    const PgGraph G = dv.graphs[gid];
    const int tid = threadIdx.x, lane = tid & 63, wv = NW > 1 ? __builtin_amdgcn_readfirstlane(tid >> 6) : 0, nf = G.nf, n = 6 * nf;
    // block-wide ordering of global + LDS traffic (NW = 1: the wavefront's own)
#define PG_BSYNC() do { if constexpr (NW > 1) __syncthreads(); else PG_GSYNC(); } while (0)
    // a value wavefront 0 holds -> every wavefront
    auto bc = [&](double v) -> double {
        if constexpr (NW == 1) return v;
        if (tid == 0) bcast_[0] = v;
        __syncthreads();
        const double r = bcast_[0];
        __syncthreads();
        return r;
    };
    auto block_max = [&](double m) -> double {          // (a maximum does not depend on the order)
        m = wave_max(m);
        if constexpr (NW == 1) return m;
        if (lane == 0) bcast_[2 + wv] = m;
        __syncthreads();
        double r = bcast_[2];
        for (int k = 1; k < NW; k++) r = fmax(r, bcast_[2 + k]);
        __syncthreads();
        return r;
    };
    double *red = dv.red + (size_t)G.edge0 * 6;
    double *Bt = dv.Bt + (size_t)G.vec0 * 6;
    double *pose = dv.pose + (size_t)G.pose0 * 7, *cand = dv.cand + (size_t)G.pose0 * 7;
    const int32_t *free_of = dv.free_of + G.pose0;
    PgEdge *edges = dv.edges + G.edge0;
    double *eres = dv.eres + (size_t)G.edge0 * 6, *ejac = dv.ejac + (size_t)G.edge0 * 72;
    const int32_t *adj_ptr = dv.adj_ptr + G.free0 + gid, *adj = dv.adj + G.adj0;
    const int32_t *start = dv.start + G.free0, *rowptr = dv.rowptr + G.free0 + gid;
    const int32_t *colptr = dv.colptr + G.free0 + gid, *colrows = dv.colrows + G.col0;
    double *H = dv.H + (size_t)G.blk0 * 36, *L = dv.L + (size_t)G.blk0 * 36, *Z = dv.Z + (size_t)G.blk0 * 36;
    double *scale = dv.scale + G.vec0, *diag = dv.diag + G.vec0, *grad = dv.grad + G.vec0, *step = dv.step + G.vec0, *ysol = dv.ysol + G.vec0;
    isv_pgo_result_t &res = dv.res[gid];
    const int e = lane, ea = e / 6, eb = e - 6 * ea;    // my element of a 6x6 block (lanes 0..35)
    // the envelope's index arrays in LDS when they fit (every block address of the factorisation / substitution recurrences
    // starts from them: one LDS read instead of a dependent global load per step)
    extern __shared__ int32_t dyn_idx[];
    const bool idx_lds = dv.idx_lds_rows > 0;          // (sized by the host for the largest graph of the batch)
    const int IR = dv.idx_lds_rows;
    if (idx_lds) {
        const int nc = colptr[nf];
        for (int q = tid; q < nf; q += NT) { dyn_idx[q] = start[q]; dyn_idx[IR + q] = rowptr[q]; }
        for (int q = tid; q <= nf; q += NT) dyn_idx[2 * IR + q] = colptr[q];
        for (int q = tid; q < nc; q += NT) dyn_idx[3 * IR + 1 + q] = colrows[q];
        if constexpr (NW > 1) __syncthreads(); else ISV_WSYNC();
    }
    // (explicit LDS reads: a pointer that may be LDS or global becomes a FLAT access, which waits for every outstanding
    //  global load and store as well)
    auto ST = [&](int r) -> int { return idx_lds ? dyn_idx[r] : start[r]; };
    auto RP = [&](int r) -> int { return idx_lds ? dyn_idx[IR + r] : rowptr[r]; };
    auto CP = [&](int r) -> int { return idx_lds ? dyn_idx[2 * IR + r] : colptr[r]; };
    auto CR = [&](int q) -> int { return idx_lds ? dyn_idx[3 * IR + 1 + q] : colrows[q]; };
    auto BLK = [&](double *M, int r, int c) -> double * { return M + (size_t)(RP(r) + (c - ST(r))) * 36; };

    // ---- evaluation of every residual block at x (and linearisation) ------------------------------------------------
    auto evaluate = [&](const double *x, bool jac) -> double {
        double c = 0;
        if constexpr (NW == 1) {
            for (int q = lane; q < G.ne; q += 64) c += pg_edge_eval(edges[q], x, G.huber, eres + 6 * q, ejac + 72 * q, ejac + 72 * q + 36, jac);
            PG_GSYNC();
            return wave_sum(c);
        } else {
            for (int q = tid; q < G.ne; q += NT) red[q] = pg_edge_eval(edges[q], x, G.huber, eres + 6 * q, ejac + 72 * q, ejac + 72 * q + 36, jac);
            __syncthreads();
            if (wv == 0) { for (int q = lane; q < G.ne; q += 64) c += red[q]; c = wave_sum(c); }
            return bc(c);
        }
    };
    // squared column norms of the (current) Jacobian, owner computes: lane per free pose
    auto colnorm2 = [&](double *out) {
        for (int f = tid; f < nf; f += NT) {
            double s[6] = {0, 0, 0, 0, 0, 0};
            for (int q = adj_ptr[f]; q < adj_ptr[f + 1]; q++) {
                const int ed = adj[q] >> 1, side = adj[q] & 1, dim = edges[ed].dim;
                const double *J = ejac + 72 * ed + 36 * side;
                for (int a = 0; a < dim; a++) for (int c = 0; c < 6; c++) s[c] += J[a * 6 + c] * J[a * 6 + c];
            }
            for (int c = 0; c < 6; c++) out[6 * f + c] = s[c];
        }
        PG_BSYNC();
    };
    auto scale_jac = [&]() {                           // J <- J diag(scale), lane per residual block
        for (int q = tid; q < G.ne; q += NT) {
            const PgEdge &E = edges[q];
            for (int side = 0; side < (E.kind == 0 ? 1 : 2); side++) {
                const int f = side ? E.fb : E.fa;
                if (f < 0) continue;
                double *J = ejac + 72 * q + 36 * side;
                double sc6[6], Jl[36];
                const int nq = E.dim * 6;
#pragma unroll
                for (int c = 0; c < 6; c++) sc6[c] = scale[6 * f + c];
#pragma unroll
                for (int k = 0; k < 36; k++) Jl[k] = k < nq ? J[k] : 0.0;
#pragma unroll
                for (int k = 0; k < 36; k++) if (k < nq) J[k] = Jl[k] * sc6[k % 6];
            }
        }
        PG_BSYNC();
    };
    // gradient g = J^T r (scaled Jacobian), lane per free pose; returns nothing
    auto gradient = [&]() {
        for (int f = tid; f < nf; f += NT) {
            double s[6] = {0, 0, 0, 0, 0, 0};
            for (int q = adj_ptr[f]; q < adj_ptr[f + 1]; q++) {
                const int ed = adj[q] >> 1, side = adj[q] & 1, dim = edges[ed].dim;
                const double *J = ejac + 72 * ed + 36 * side, *r = eres + 6 * ed;
                for (int a = 0; a < dim; a++) for (int c = 0; c < 6; c++) s[c] += J[a * 6 + c] * r[a];
            }
            for (int c = 0; c < 6; c++) grad[6 * f + c] = s[c];
        }
        PG_BSYNC();
    };
    // gradient_max_norm = |x - Plus(x, -g_unscaled)|_inf over the free blocks
    auto gmax_of = [&]() -> double {
        double m = 0;
        for (int k = tid; k < G.P1; k += NT) {
            const int f = free_of[k];
            if (f < 0) continue;
            double ng[6], xp[7];
            for (int c = 0; c < 6; c++) ng[c] = -grad[6 * f + c] / scale[6 * f + c];
            pose_plus(pose + 7 * k, ng, xp);
            for (int c = 0; c < 7; c++) m = fmax(m, fabs(pose[7 * k + c] - xp[c]));
        }
        return block_max(m);
    };
    auto xnorm_of = [&](const double *x) -> double {
        double s = 0;
        if (wv == 0) { for (int k = lane; k < G.P1; k += 64) if (free_of[k] >= 0) for (int c = 0; c < 7; c++) s += x[7 * k + c] * x[7 * k + c]; s = wave_sum(s); }
        return sqrt(bc(s));
    };
    // H = J^T J on the envelope, lane per free pose (row): its diagonal block and the blocks towards EARLIER neighbours
    auto assemble = [&]() {
        for (int q = tid; q < G.nblk * 36; q += NT) H[q] = 0.0;
        PG_BSYNC();
        for (int f = tid; f < nf; f += NT) {
            for (int q = adj_ptr[f]; q < adj_ptr[f + 1]; q++) {
                const int ed = adj[q] >> 1, side = adj[q] & 1;
                const PgEdge &E = edges[ed];
                const double *J = ejac + 72 * ed + 36 * side;
                const int dim = E.dim, kind = E.kind, other = kind != 0 ? (side ? E.fa : E.fb) : -1;
                double Jl[36], blk[36], old[36];
#pragma unroll
                for (int k = 0; k < 36; k++) Jl[k] = k < dim * 6 ? J[k] : 0.0;     // (rows beyond dim: exact zeros in the sums)
                double *D = BLK(H, f, f);
#pragma unroll
                for (int k = 0; k < 36; k++) old[k] = D[k];
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int b = 0; b <= a; b++) {
                        double s = 0;
#pragma unroll
                        for (int k = 0; k < 6; k++) s += Jl[k * 6 + a] * Jl[k * 6 + b];
                        blk[a * 6 + b] = s; blk[b * 6 + a] = s;
                    }
#pragma unroll
                for (int k = 0; k < 36; k++) D[k] = old[k] + blk[k];
                if (other >= 0 && other < f) {                 // the later endpoint owns the off-diagonal block (f, other)
                    const double *Jo = ejac + 72 * ed + 36 * (1 - side);
                    double Jol[36];
#pragma unroll
                    for (int k = 0; k < 36; k++) Jol[k] = Jo[k];
                    double *O = BLK(H, f, other);
#pragma unroll
                    for (int k = 0; k < 36; k++) old[k] = O[k];
#pragma unroll
                    for (int a = 0; a < 6; a++)
#pragma unroll
                        for (int b = 0; b < 6; b++) {
                            double s = 0;
#pragma unroll
                            for (int k = 0; k < 6; k++) s += Jl[k * 6 + a] * Jol[k * 6 + b];
                            blk[a * 6 + b] = s;
                        }
#pragma unroll
                    for (int k = 0; k < 36; k++) O[k] = old[k] + blk[k];
                }
            }
        }
        PG_BSYNC();
    };
    // L L^T = H + diag(damp) on the envelope; diagonal slots hold L_rr^-1.  Returns false when a pivot is not positive.
    // The recurrence runs through LDS: a CHAIN row (its envelope starts at r - 1) needs L_{r-1,r-1}^-1 (still in T2 from the
    // previous row) and its own new block (T1), nothing from global memory that this wavefront wrote since the last fence;
    // its two blocks of H are loaded one row ahead.  Only a LOOP row (longer envelope) reads earlier rows' blocks of L back
    // from global memory and pays for a fence: one when it starts, one before its diagonal block, and one per step whose
    // column is itself a loop row.
    auto factor = [&](const double *damp) -> bool {
        bool ok = true;                                // (every block of L is written before it is read: A comes from H)
        double nx_rc = 0, nx_rr = 0;                   // H(r, r-1)[e], H(r, r)[e] (+ damping) of the NEXT row when it is a chain row
        bool have_nx = false;
        for (int r = 0; r < nf && ok; r++) {
            const int s0 = ST(r);
            const bool loop_row = s0 < r - 1;
            const double a_rc = nx_rc, a_rr = nx_rr;
            const bool pre = have_nx;
            have_nx = false;
            if (r + 1 < nf && ST(r + 1) == r) {        // prefetch the next chain row's blocks
                if (e < 36) { nx_rc = BLK(H, r + 1, r)[e]; nx_rr = BLK(H, r + 1, r + 1)[e] + (ea == eb ? damp[6 * (r + 1) + ea] : 0.0); }
                have_nx = true;
            }
            if (loop_row) PG_GSYNC();                  // blocks of earlier rows written since the last fence
            // one column of row r the general way: S = A(r,c) - sum_{m = max(start[r], start[c])}^{c-1} L(r,m) L(c,m)^T ;  L(r,c) = S L_cc^-T
            auto general_step = [&](int c) {
                const int sc = ST(c), m0 = s0 > sc ? s0 : sc;
                if (m0 < c - 1) PG_GSYNC();            // several blocks of THIS row are read back (column c is a loop row)
                double acc = 0;
                if (e < 36) {
                    acc = (pre && c == r - 1) ? a_rc : BLK(H, r, c)[e];
                    for (int m = m0; m < c - 1; m++) {
                        const double *X = BLK(L, r, m), *Y = BLK(L, c, m);
                        for (int k = 0; k < 6; k++) acc -= X[ea * 6 + k] * Y[eb * 6 + k];
                    }
                    if (m0 < c) {                      // m = c - 1: the block L(r, c-1) of the previous step is in T1 (LDS)
                        const double *Y = BLK(L, c, c - 1);
                        for (int k = 0; k < 6; k++) acc -= T1[ea * 6 + k] * Y[eb * 6 + k];
                    }
                }
                PG_LSYNC();
                if (e < 36) T0[e] = acc;
                PG_LSYNC();
                double x = 0;
                if (e < 36) {
                    if (c == r - 1) { for (int k = 0; k <= eb; k++) x += T0[ea * 6 + k] * T2[eb * 6 + k]; }       // L_cc^-1 of the previous row (LDS)
                    else { const double *Li = BLK(L, c, c); for (int k = 0; k <= eb; k++) x += T0[ea * 6 + k] * Li[eb * 6 + k]; }
                }
                PG_LSYNC();
                if (e < 36) { T1[e] = x; BLK(L, r, c)[e] = x; }
                PG_LSYNC();
            };
            if (!loop_row) { for (int c = s0; c < r; c++) general_step(c); }
            else {
                // (round 5) A loop closure's row walks its envelope column by column, every step waiting for the one before: ~900 of the
                // dependent block steps of a factorisation of 200 keyframes / 5 loops, and each took one memory latency (its operands were
                // loaded ONE step ahead: 0.45 us per step whatever the arithmetic).  An interior column c is a chain row this row has no
                // factor with -- H(r,c) = 0 --, so L(r,c) = -L(r,c-1) L(c,c-1)^T L_cc^-T = -L(r,c-1) B_c^T with B_c left behind by row c:
                // ONE 6 x 6 product and two LDS hand-overs.  H(r,c) and B_c are loaded PD steps ahead into a register ring (the
                // envelope is contiguous in both); any other column takes general_step (it loads what it needs itself).
                constexpr int PD = 8;
                double rA[PD], rB[PD][6];
                // (the row's blocks of H and L and the chain rows' B are contiguous in c: one base address each, no index look-ups per step)
                const int el = e < 36 ? e : 0;
                const double *const Hr = BLK(H, r, s0) + el, *const Br = Bt + (size_t)s0 * 36 + (el % 6) * 6;
                double *const Lr = BLK(L, r, s0) + el;
                auto prefetch = [&](double &pa, double *pb, int c) {
                    const int dc = (c < r ? c : r - 1) - s0;                            // (past the row: a valid address, never used)
                    pa = Hr[dc * 36];
                    for (int k = 0; k < 6; k++) pb[k] = Br[dc * 36 + k];
                };
                general_step(s0);
#pragma unroll
                for (int u = 0; u < PD; u++) prefetch(rA[u], rB[u], s0 + 1 + u);
                for (int cb = s0 + 1; cb < r; cb += PD) {
#pragma unroll
                    for (int u = 0; u < PD; u++) {
                        const int c = cb + u;
                        if (c < r) {
                            const double cA = rA[u];
                            double cB[6];
                            for (int k = 0; k < 6; k++) cB[k] = rB[u][k];
                            prefetch(rA[u], rB[u], c + PD);
                            if (ST(c) == c - 1 && __all(e >= 36 || cA == 0.0)) {
                                double x = 0;
                                if (e < 36) { for (int k = 0; k < 6; k++) x -= T1[ea * 6 + k] * cB[k]; }
                                PG_LSYNC();
                                if (e < 36) { T1[e] = x; Lr[(c - s0) * 36] = x; }
                                PG_LSYNC();
                            } else general_step(c);
                        }
                    }
                }
            }
            // diagonal: D = A(r,r) + damp - sum_m L(r,m) L(r,m)^T
            if (loop_row) PG_GSYNC();
            double acc = 0;
            if (e < 36) {
                acc = pre ? a_rr : BLK(H, r, r)[e] + (ea == eb ? damp[6 * r + ea] : 0.0);
                for (int m = s0; m < r - 1; m++) { const double *X = BLK(L, r, m); for (int k = 0; k < 6; k++) acc -= X[ea * 6 + k] * X[eb * 6 + k]; }
                if (s0 < r) { for (int k = 0; k < 6; k++) acc -= T1[ea * 6 + k] * T1[eb * 6 + k]; }                // m = r - 1
            }
            PG_LSYNC();                                // (T2 = L_{r-1,r-1}^-1 has been read by every lane)
            if (e < 36) T2[e] = acc;
            PG_LSYNC();
            ok = pg_chol_inv6(T2, lane);
            if (e < 36) {
                BLK(L, r, r)[e] = T2[e];
                // B_r = L_rr^-1 L(r, r-1) for the loop rows that will pass through column r (zero where row r has no earlier block)
                double b = 0;
                if (s0 == r - 1) { for (int k = 0; k <= ea; k++) b += T2[ea * 6 + k] * T1[k * 6 + eb]; }
                Bt[(size_t)r * 36 + e] = b;
            }
        }
        PG_GSYNC();
        return ok;
    };
    // x = (L L^T)^-1 b  -> xs ; lanes 0..5 own the components of a block.  The previous block of the recurrence stays in
    // registers (v_readlane); only loop rows exchange through global memory (fences as in factor()).
    // (round 5) The blocks of L a row needs -- its diagonal block and the one towards its chain neighbour -- and its right-hand side
    // are loaded PS rows AHEAD into a register ring: with the loads one row ahead (forward) or not ahead at all (backward) every one
    // of the 2 nf steps waited for a memory latency, 0.74 us per step for a few dozen FMAs.  The backward pass re-reads the ring's
    // right-hand sides after a loop row has updated them.
    auto solve = [&](const double *b, double *xs) {
        const int ln = lane < 6 ? lane : 0;
        constexpr int PS = 8;
        double prev = 0;                               // y_{r-1} (forward) / x_{r+1} (backward), component = lane
        {
            double fX[PS][6], fLi[PS][6], fb[PS];      // row ln of L(r, r-1), row ln of L_rr^-1, b_r of the rows r .. r + PS - 1
            auto fpf = [&](double *X6, double *Li6, double &bb, int rr) {
                const int q = rr < nf ? rr : nf - 1;
                const double *Li = BLK(L, q, q), *X = ST(q) < q ? BLK(L, q, q - 1) : Li;          // (no earlier block: a valid address, never used)
                for (int k = 0; k < 6; k++) { X6[k] = X[ln * 6 + k]; Li6[k] = Li[ln * 6 + k]; }
                bb = b[6 * q + ln];
            };
#pragma unroll
            for (int u = 0; u < PS; u++) fpf(fX[u], fLi[u], fb[u], u);
            for (int r0 = 0; r0 < nf; r0 += PS) {      // forward: y_r = L_rr^-1 (b_r - sum_{m<r} L(r,m) y_m)
#pragma unroll
                for (int u = 0; u < PS; u++) {
                    const int r = r0 + u;
                    if (r < nf) {
                        const int s0 = ST(r);
                        double cX[6], cLi[6];
                        const double cb = fb[u];
                        for (int k = 0; k < 6; k++) { cX[k] = fX[u][k]; cLi[k] = fLi[u][k]; }
                        fpf(fX[u], fLi[u], fb[u], r + PS);
                        if (s0 < r - 1) PG_GSYNC();
                        double pv[6];
                        for (int k = 0; k < 6; k++) pv[k] = readlane_d(prev, k);
                        double v = cb;
                        if (s0 == r - 1) { for (int k = 0; k < 6; k++) v -= cX[k] * pv[k]; }
                        else {
                            for (int m = s0; m < r; m++) {
                                const double *X = BLK(L, r, m);
                                if (m == r - 1) { for (int k = 0; k < 6; k++) v -= X[ln * 6 + k] * pv[k]; }
                                else { for (int k = 0; k < 6; k++) v -= X[ln * 6 + k] * ysol[6 * m + k]; }
                            }
                        }
                        double y = 0;
                        for (int k = 0; k < 6; k++) { const double vk = readlane_d(v, k); if (k <= ln) y += cLi[k] * vk; }
                        if (lane < 6) ysol[6 * r + lane] = y;
                        prev = y;
                    }
                }
            }
        }
        PG_GSYNC();
        // backward: x_r = L_rr^-T (y_r - sum_{i in colpat(r)} L(i,r)^T x_i).  A loop row i subtracts its L(i,c)^T x_i from y_c of
        // every column c it covers as soon as x_i is known (lanes over the span); what is left for a row is the term of row
        // r + 1 when that is a chain row, from registers.
        prev = 0;
        {
            double gLi[PS][6], gX[PS][6], gy[PS];      // column ln of L_rr^-1, column ln of L(r+1, r), y_r of the rows r .. r - PS + 1
            auto bpf = [&](double *Li6, double *X6, double &yy, int rr) {
                const int q = rr >= 0 ? rr : 0;
                const double *Li = BLK(L, q, q), *X = (q + 1 < nf && ST(q + 1) == q) ? BLK(L, q + 1, q) : Li;      // (row q + 1 not a chain row: never used)
                for (int k = 0; k < 6; k++) { Li6[k] = Li[k * 6 + ln]; X6[k] = X[k * 6 + ln]; }
                yy = ysol[6 * q + ln];
            };
#pragma unroll
            for (int u = 0; u < PS; u++) bpf(gLi[u], gX[u], gy[u], nf - 1 - u);
            bool next_is_chain = false;                // row r + 1 exists and its envelope starts at r
            for (int r0 = nf - 1; r0 >= 0; r0 -= PS) {
#pragma unroll
                for (int u = 0; u < PS; u++) {
                    const int r = r0 - u;
                    if (r >= 0) {
                        double cLi[6], cX[6];
                        double v = gy[u];
                        for (int k = 0; k < 6; k++) { cLi[k] = gLi[u][k]; cX[k] = gX[u][k]; }
                        bpf(gLi[u], gX[u], gy[u], r - PS);
                        double pv[6];
                        for (int k = 0; k < 6; k++) pv[k] = readlane_d(prev, k);
                        if (next_is_chain) { for (int k = 0; k < 6; k++) v -= cX[k] * pv[k]; }
                        double x = 0;
                        for (int k = 0; k < 6; k++) { const double vk = readlane_d(v, k); if (k >= ln) x += cLi[k] * vk; }
                        if (lane < 6) xs[6 * r + lane] = x;
                        prev = x;
                        const int s0 = ST(r);
                        next_is_chain = s0 == r - 1;
                        if (s0 < r - 1) {              // loop row: y_c -= L(r,c)^T x_r for c in [s0, r)
                            double xr[6];
                            for (int k = 0; k < 6; k++) xr[k] = readlane_d(x, k);
                            PG_GSYNC();
                            for (int q = lane; q < (r - s0) * 6; q += 64) {
                                const int c = s0 + q / 6, comp = q % 6;
                                const double *X = BLK(L, r, c);
                                double a = ysol[6 * c + comp];
                                for (int k = 0; k < 6; k++) a -= X[k * 6 + comp] * xr[k];
                                ysol[6 * c + comp] = a;
                            }
                            PG_GSYNC();
                            // the ring's right-hand sides were read before this update: slot j holds row r0 - j (j > u) or r0 - PS - j (already refilled)
#pragma unroll
                            for (int j = 0; j < PS; j++) { const int rowj = j <= u ? r0 - PS - j : r0 - j; gy[j] = ysol[6 * (rowj >= 0 ? rowj : 0) + ln]; }
                        }
                    }
                }
            }
        }
        PG_GSYNC();
    };

    // ================= TrustRegionMinimizer::Minimize + LevenbergMarquardtStrategy (Ceres 2.0.0 defaults) =============
    if (tid == 0) { res.status = ISV_OK; res.num_successful = 0; res.n_loop_edges = 0; res._pad = 0;     // (every byte of the record is defined: callers compare records)
                    for (int k = 0; k < ISV_MAX_TRACE; k++) { res.trace_cost[k] = 0; res.trace_accepted[k] = 0; } }
    double x_cost = evaluate(pose, true);
    int it = 0, term = ISV_TERM_RUNNING, nsucc = 0;
    if (nf > 0) {
        colnorm2(scale);
        for (int q = tid; q < n; q += NT) scale[q] = 1.0 / (1.0 + sqrt(scale[q]));
        PG_BSYNC();
        scale_jac();
        gradient();
        double gmax = gmax_of(), x_norm = xnorm_of(pose);
        double radius = 1e4, decrease = 2.0;
        bool reuse_diag = false;
        int invalid = 0;
        if (tid == 0) { res.initial_cost = x_cost; res.trace_cost[0] = x_cost; }
        for (;;) {
            if (it >= G.max_iter) { term = ISV_TERM_MAX_ITERATIONS; break; }
            if (gmax <= 1e-10) { term = ISV_TERM_GRADIENT_TOL; break; }
            if (radius <= 1e-32) { term = ISV_TERM_MIN_RADIUS; break; }
            it++;
            if (!reuse_diag) {                         // diagonal_ = clamp(squared column norms)
                colnorm2(diag);
                for (int q = tid; q < n; q += NT) diag[q] = fmin(fmax(diag[q], 1e-6), 1e32);
                PG_BSYNC();
            }
            reuse_diag = true;
            assemble();
            for (int q0 = tid; q0 < n; q0 += 4 * NT) {   // D^2 = diagonal / radius (step[] as scratch); four loads in flight per lane
                double v[4];
                for (int u = 0; u < 4; u++) v[u] = q0 + NT * u < n ? diag[q0 + NT * u] : 0.0;
                for (int u = 0; u < 4; u++) if (q0 + NT * u < n) step[q0 + NT * u] = v[u] / radius;
            }
            PG_BSYNC();
            bool ok = false;
            if (wv == 0) ok = factor(step);               // (the recurrences: wavefront 0)
            if (wv == 0 && ok) solve(grad, step);
            ok = bc(ok ? 1.0 : 0.0) != 0.0;               // (NW > 1: also the barrier that hands wavefront 0's stores to the others)
            if (ok) {
                double bad = 0;
                for (int q0 = tid; q0 < n; q0 += 4 * NT) {
                    double v[4];
                    for (int u = 0; u < 4; u++) v[u] = q0 + NT * u < n ? step[q0 + NT * u] : 0.0;
                    for (int u = 0; u < 4; u++) if (q0 + NT * u < n) { if (!(v[u] - v[u] == 0.0)) bad = 1; step[q0 + NT * u] = -v[u]; }
                }
                PG_BSYNC();
                if (block_max(bad) > 0) ok = false;
            }
            bool valid = false;
            double model_cost_change = 0;
            if (ok) {                                  // -(J step)^T (r + J step / 2)
                // (the term of a residual row is rounded before it is added -- no fused multiply-add across the two: what NW > 1 adds
                //  is the stored term)
                double mc = 0;
                for (int q = tid; q < G.ne; q += NT) {
                    const PgEdge &E = edges[q];
                    for (int a = 0; a < E.dim; a++) {
                        double m = 0;
                        if (E.fa >= 0) for (int c = 0; c < 6; c++) m += ejac[72 * q + a * 6 + c] * step[6 * E.fa + c];
                        if (E.kind != 0 && E.fb >= 0) for (int c = 0; c < 6; c++) m += ejac[72 * q + 36 + a * 6 + c] * step[6 * E.fb + c];
                        double term = m * (eres[6 * q + a] + m / 2.0);
                        asm volatile("" : "+v"(term));
                        if constexpr (NW == 1) mc += term; else red[6 * q + a] = term;
                    }
                }
                if constexpr (NW > 1) {
                    __syncthreads();
                    if (wv == 0) for (int q = lane; q < G.ne; q += 64) { const int dim = edges[q].dim; for (int a = 0; a < dim; a++) mc += red[6 * q + a]; }
                }
                model_cost_change = -bc(wave_sum(mc));
                valid = model_cost_change > 0.0;
            }
            if (!valid) {
                if (++invalid >= 5) { term = ok ? ISV_TERM_INVALID_STEPS : ISV_TERM_LINEAR_SOLVER; break; }
                radius /= decrease; decrease *= 2.0; reuse_diag = true;        // StepIsInvalid == StepRejected
                if (tid == 0 && it < ISV_MAX_TRACE) { res.trace_cost[it] = x_cost; res.trace_accepted[it] = 0; }
                continue;
            }
            invalid = 0;
            double dn = 0;
            for (int k = tid; k < G.P1; k += NT) {     // candidate = Plus(x, step * scale)
                const int f = free_of[k];
                if (f < 0) { double x0[7]; for (int c = 0; c < 7; c++) x0[c] = pose[7 * k + c]; for (int c = 0; c < 7; c++) cand[7 * k + c] = x0[c]; continue; }
                double dl[6], xp[7], x0[7];
                for (int c = 0; c < 6; c++) dl[c] = step[6 * f + c] * scale[6 * f + c];
                for (int c = 0; c < 7; c++) x0[c] = pose[7 * k + c];
                pose_plus(x0, dl, xp);
                if constexpr (NW == 1) { for (int c = 0; c < 7; c++) { const double df = x0[c] - xp[c]; dn = __builtin_fma(df, df, dn); } }
                for (int c = 0; c < 7; c++) cand[7 * k + c] = xp[c];
            }
            PG_BSYNC();
            if constexpr (NW > 1) {                    // |x - candidate|^2 in NW = 1's order, from the stored candidate
                if (wv == 0) for (int k = lane; k < G.P1; k += 64) {
                    if (free_of[k] < 0) continue;
                    for (int c = 0; c < 7; c++) { const double df = pose[7 * k + c] - cand[7 * k + c]; dn = __builtin_fma(df, df, dn); }
                }
            }
            const double step_norm = sqrt(bc(wave_sum(dn)));
            const double cand_cost = evaluate(cand, false);
            bool stop = false, accepted = false;
            if (step_norm <= 1e-8 * (x_norm + 1e-8)) { term = ISV_TERM_PARAMETER_TOL; stop = true; }
            else if (fabs(x_cost - cand_cost) <= 1e-6 * x_cost) { term = ISV_TERM_FUNCTION_TOL; stop = true; }
            if (stop) { if (tid == 0 && it < ISV_MAX_TRACE) { res.trace_cost[it] = x_cost; res.trace_accepted[it] = 0; } break; }
            const double rel = (x_cost - cand_cost) / model_cost_change;
            if (rel > 1e-3) {
                accepted = true;
                for (int q0 = tid; q0 < 7 * G.P1; q0 += 4 * NT) {
                    double v[4];
                    for (int u = 0; u < 4; u++) v[u] = q0 + NT * u < 7 * G.P1 ? cand[q0 + NT * u] : 0.0;
                    for (int u = 0; u < 4; u++) if (q0 + NT * u < 7 * G.P1) pose[q0 + NT * u] = v[u];
                }
                PG_BSYNC();
                x_norm = xnorm_of(pose);
                x_cost = evaluate(pose, true);
                scale_jac();
                gradient();
                gmax = gmax_of();
                radius = radius / fmax(1.0 / 3.0, 1.0 - pow(2.0 * rel - 1.0, 3.0));
                radius = fmin(1e16, radius); decrease = 2.0; reuse_diag = false;
                nsucc++;
            } else { radius /= decrease; decrease *= 2.0; reuse_diag = true; }
            if (tid == 0 && it < ISV_MAX_TRACE) { res.trace_cost[it] = accepted ? x_cost : cand_cost; res.trace_accepted[it] = accepted ? 1 : 0; }
        }
    } else {
        term = ISV_TERM_GRADIENT_TOL;
        if (tid == 0) res.initial_cost = x_cost;
    }
    if (tid == 0) { res.iterations = it; res.termination = term; res.final_cost = x_cost; res.num_successful = nsucc; res.n_poses = G.P1; res.n_free = nf; }

    // ================= ceres::Covariance: diagonal blocks of (J^T J)^-1 at the solution, tangent space ==================
    double *cov = dv.cov + (size_t)G.pose0 * 36;
    for (int q = tid; q < G.P1 * 36; q += NT) cov[q] = 0.0;
    PG_BSYNC();
    if (nf == 0) return;
    // the stored Jacobian is the Jacobi-scaled one at x: H_s = S H S, so H^-1 = S H_s^-1 S
    assemble();
    for (int q = tid; q < n; q += NT) step[q] = 0.0;
    PG_BSYNC();
    bool fok = false;
    if (wv == 0) fok = factor(step);
    if (bc(fok ? 1.0 : 0.0) == 0.0) { if (tid == 0) res.status = ISV_ERR_NONFINITE; return; }
    // Takahashi recurrence on the envelope, columns from the last to the first:
    //   Z(i,j) = [delta_ij L_jj^-T - sum_{k in colpat(j)} Z(i,k) L(k,j)] L_jj^-1      for i in {j} U colpat(j)
    // (a recurrence over the columns: wavefront 0)
    // (round 5) A column that only its chain neighbour reaches down into -- colpat(j) = {j + 1} -- needs Z(j+1,j+1) (the diagonal block the
    // previous column ended with) and Z(j+1,j) (what its first step produces): both stay in LDS tiles (T1, T2), so such a column reads no
    // block of Z back from global memory and needs none of the two fences of the general column (each a memory round trip: 6.4 us per
    // column before); its blocks of L are loaded one column ahead.  Same operations in the same order as the general column: same bits.
    if (wv == 0) {
        bool dirty = false, have_pf = false;           // dirty: blocks of Z written since the last fence; have_pf: pLk / pLi / pLt hold column j's operands
        double pLk[6] = {0, 0, 0, 0, 0, 0}, pLi[6] = {0, 0, 0, 0, 0, 0}, pLt = 0;
        for (int j = nf - 1; j >= 0; j--) {
            const double *Li = BLK(L, j, j);
            const int c0 = CP(j), c1 = CP(j + 1);
            const bool fast = j + 1 < nf && c1 - c0 == 1 && CR(c0) == j + 1;      // (T1 = Z(j+1,j+1): every column leaves its diagonal block there)
            double lk[6], li[6], lt = pLt;
            for (int m = 0; m < 6; m++) { lk[m] = pLk[m]; li[m] = pLi[m]; }
            const bool pre = have_pf;
            have_pf = false;
            if (j >= 1 && ST(j) == j - 1 && e < 36) {                          // column j - 1's operands: L(j, j-1) (column eb), L_{j-1,j-1}^-1 (column eb; entry (eb, ea))
                const double *Ln = BLK(L, j, j - 1), *Lin = BLK(L, j - 1, j - 1);
                for (int m = 0; m < 6; m++) { pLk[m] = Ln[m * 6 + eb]; pLi[m] = Lin[m * 6 + eb]; }
                pLt = Lin[eb * 6 + ea];
            }
            if (j >= 1 && ST(j) == j - 1) have_pf = true;
            if (fast) {
                if (!pre && e < 36) {
                    const double *Lkj = BLK(L, j + 1, j);
                    for (int m = 0; m < 6; m++) { lk[m] = Lkj[m * 6 + eb]; li[m] = Li[m * 6 + eb]; }
                    lt = Li[eb * 6 + ea];
                }
                double acc = 0, x = 0;
                if (e < 36) { for (int m = 0; m < 6; m++) acc -= T1[ea * 6 + m] * lk[m]; }                 // Z(j+1,j) = -Z(j+1,j+1) L(j+1,j) L_jj^-1
                PG_LSYNC();
                if (e < 36) T0[e] = acc;
                PG_LSYNC();
                if (e < 36) { for (int m = eb; m < 6; m++) x += T0[ea * 6 + m] * li[m]; BLK(Z, j + 1, j)[e] = x; T2[e] = x; }
                PG_LSYNC();
                acc = lt; x = 0;                                                                             // Z(j,j) = (L_jj^-T - Z(j+1,j)^T L(j+1,j)) L_jj^-1
                if (e < 36) { for (int m = 0; m < 6; m++) acc -= T2[m * 6 + ea] * lk[m]; }
                if (e < 36) T0[e] = acc;
                PG_LSYNC();
                if (e < 36) { for (int m = eb; m < 6; m++) x += T0[ea * 6 + m] * li[m]; BLK(Z, j, j)[e] = x; T1[e] = x; }
                PG_LSYNC();
                dirty = true;
                continue;
            }
            if (dirty) { PG_GSYNC(); dirty = false; }
            for (int qi = c0; qi <= c1; qi++) {            // the rows below j first: Z(j,j) needs Z(k,j), k in colpat(j)
                const int i = qi < c1 ? CR(qi) : j;
                if (qi == c1) PG_GSYNC();
                double acc = 0;
                if (e < 36) {
                    if (i == j) acc = Li[eb * 6 + ea];                                   // L_jj^-T
                    for (int q = c0; q < c1; q++) {
                        const int k = CR(q);
                        const double *Lkj = BLK(L, k, j);
                        if (i >= k) { const double *Zik = BLK(Z, i, k); for (int m = 0; m < 6; m++) acc -= Zik[ea * 6 + m] * Lkj[m * 6 + eb]; }
                        else { const double *Zki = BLK(Z, k, i); for (int m = 0; m < 6; m++) acc -= Zki[m * 6 + ea] * Lkj[m * 6 + eb]; }
                    }
                }
                PG_LSYNC();
                if (e < 36) T0[e] = acc;
                PG_LSYNC();
                if (e < 36) {
                    double x = 0;
                    for (int m = eb; m < 6; m++) x += T0[ea * 6 + m] * Li[m * 6 + eb];   // times L_jj^-1 (lower)
                    BLK(Z, i, j)[e] = x;
                    if (i == j) T1[e] = x;
                }
            }
            PG_GSYNC();
        }
        if (dirty) PG_GSYNC();
    }
    if constexpr (NW > 1) __syncthreads();
    for (int k = tid; k < G.P1; k += NT) {
        const int f = free_of[k];
        if (f < 0) continue;
        const double *Zd = BLK(Z, f, f);
        for (int a = 0; a < 6; a++) for (int b = 0; b < 6; b++) cov[k * 36 + a * 6 + b] = scale[6 * f + a] * Zd[a * 6 + b] * scale[6 * f + b];
    }
}

// =====================================================================================================================
// host side
// (structure record, analysis, numbers, the table of the call's arrays, layout, write-back, thread team and the pipeline's control
//  flow: isv_pgo_host.h.  Here: the handle, the HIP calls of a chunk and the entry points.)
struct isv_pgo {
    std::vector<PgStructure> cache;               // [max_graphs] the structure of every graph slot as the last call analysed it
    int64_t cache_hits = 0;
    isv_pgo_config_t cfg;
    std::string err;
    int device = 0, n_cus = 256;
    // No work is ever put on `stream`, but it is NOT dead: created ahead of the four chunk streams, it shifts which hardware queues
    // those land on.  Measured with and without it, all else equal, in a process that already holds other streams (bench.py --full,
    // 1024 graphs, cached calls): last enqueue -> last drain 17.4 / 22.7 ms with it, 30.8 / 33.3 ms without; k_pgo's span 19.3 ms
    // against 31.2-31.7; the call 29.8-30.9 ms against 39.7-41.2.  In a process of its own (scripts/pgo_probe.py) there is no
    // difference.  It stays until the chunk streams' placement is understood.
    hipStream_t stream = nullptr;
    PgDev d{};
    std::vector<void *> allocs;
    PgCaps cap{};
    void *pin = nullptr; size_t pin_cap = 0;      // pinned staging of a batch call's arrays (grown on demand, kept)
    // a batch call goes to the device in up to PG_MAX_CHUNKS chunks of graphs, each on a stream of its own: chunk c + 1 is assembled and
    // copied while chunk c is being solved, and chunk c is written back while chunk c + 1 still runs (round 4)
    hipStream_t cstream[PG_MAX_CHUNKS] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t kev[PG_MAX_CHUNKS][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};     // around every chunk's k_pgo
    double last_kernel_ms = -1;                   // first chunk's kernel start -> last chunk's kernel end of the last call
    double last_blocks = 0;                       // skyline blocks of the last batch (all graphs)
};

// (msg) = "<call>: <HIP's error string>" and return ISV_ERR_DEVICE when a HIP call fails
#define PMSG(msg, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { (msg) = std::string(#call) + ": " + hipGetErrorString(e_); return ISV_ERR_DEVICE; } } while (0)
#define PCHK(h, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { (h)->err = std::string(#call) + ": " + hipGetErrorString(e_); return ISV_ERR_DEVICE; } } while (0)
template <typename T> static int pal(isv_pgo *h, T **p, size_t n) {
    void *q = nullptr;
    PCHK(h, hipMalloc(&q, (n ? n : 1) * sizeof(T)));
    h->allocs.push_back(q); *p = (T *)q;
    return ISV_OK;
}
#define PTRY(x) do { int rc_ = (x); if (rc_ != ISV_OK) return rc_; } while (0)

extern "C" const char *isv_pgo_last_error(const isv_pgo_t *h) { return h ? h->err.c_str() : "null handle"; }
// measurement: duration of k_pgo in the last optimize call (HIP events on the chunks' streams) and the number of 6x6 skyline
// blocks its graphs held
extern "C" int64_t isv_pgo_structure_cache_hits(const isv_pgo_t *h) { return h ? h->cache_hits : 0; }
extern "C" int isv_pgo_last_kernel_ms(isv_pgo_t *h, double *ms, double *skyline_blocks) {
    if (!h || !ms || h->last_kernel_ms < 0) return ISV_ERR_INVALID_ARG;
    *ms = h->last_kernel_ms;
    if (skyline_blocks) *skyline_blocks = h->last_blocks;
    return ISV_OK;
}

extern "C" void isv_pgo_destroy(isv_pgo_t *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    for (void *p : h->allocs) (void)hipFree(p);
    if (h->pin) (void)hipHostFree(h->pin);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    for (auto &cs : h->cstream) if (cs) (void)hipStreamDestroy(cs);
    for (auto &ke : h->kev) for (auto &e : ke) if (e) (void)hipEventDestroy(e);
    delete h;
}

static int pgo_create_impl(isv_pgo *h) {
    int ndev = 0;
    PCHK(h, hipGetDeviceCount(&ndev));
    if (ndev <= 0) { h->err = "no HIP device"; return ISV_ERR_DEVICE; }
    PCHK(h, hipGetDevice(&h->device));
    { int cu = 0; if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && cu > 0) h->n_cus = cu; else (void)hipGetLastError(); }
    PCHK(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));       // (the spacer: see isv_pgo::stream)
    for (auto &cs : h->cstream) PCHK(h, hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    for (auto &ke : h->kev) for (auto &e : ke) PCHK(h, hipEventCreate(&e));
    const size_t G = h->cfg.max_graphs, K = h->cfg.max_keyframes;
    PgCaps &cap = h->cap;
    cap.pose = G * K; cap.edge = G * 3 * K; cap.blk = G * (2 * K + (size_t)h->cfg.max_loop_blocks);
    cap.adj = 2 * cap.edge; cap.col = cap.blk;
    PgDev &d = h->d;
    PTRY(pal(h, &d.graphs, G)); PTRY(pal(h, &d.pose, cap.pose * 7)); PTRY(pal(h, &d.cand, cap.pose * 7)); PTRY(pal(h, &d.free_of, cap.pose));
    PTRY(pal(h, &d.edges, cap.edge)); PTRY(pal(h, &d.eres, cap.edge * 6)); PTRY(pal(h, &d.ejac, cap.edge * 72)); PTRY(pal(h, &d.red, cap.edge * 6)); PTRY(pal(h, &d.Bt, cap.pose * 36));
    PTRY(pal(h, &d.adj_ptr, cap.pose + G)); PTRY(pal(h, &d.adj, cap.adj));
    PTRY(pal(h, &d.start, cap.pose)); PTRY(pal(h, &d.rowptr, cap.pose + G)); PTRY(pal(h, &d.colptr, cap.pose + G)); PTRY(pal(h, &d.colrows, cap.col));
    PTRY(pal(h, &d.H, cap.blk * 36)); PTRY(pal(h, &d.L, cap.blk * 36)); PTRY(pal(h, &d.Z, cap.blk * 36));
    PTRY(pal(h, &d.scale, cap.pose * 6)); PTRY(pal(h, &d.diag, cap.pose * 6)); PTRY(pal(h, &d.grad, cap.pose * 6));
    PTRY(pal(h, &d.step, cap.pose * 6)); PTRY(pal(h, &d.ysol, cap.pose * 6));
    PTRY(pal(h, &d.cov, cap.pose * 36)); PTRY(pal(h, &d.res, G));
    return ISV_OK;
}

extern "C" int isv_pgo_create(const isv_pgo_config_t *cfg, isv_pgo_t **out) {
    if (!cfg || !out) return ISV_ERR_INVALID_ARG;
    *out = nullptr;
    if (cfg->max_keyframes < 2 || cfg->max_graphs < 1 || cfg->max_loop_blocks < 0 || cfg->max_iterations < 0 || cfg->max_iterations >= ISV_MAX_TRACE ||
        !(cfg->huber_delta > 0)) return ISV_ERR_INVALID_ARG;
    isv_pgo *h = new isv_pgo();
    h->cfg = *cfg;
    const int rc = pgo_create_impl(h);
    if (rc != ISV_OK) { fprintf(stderr, "isv_pgo_create: %s\n", h->err.c_str()); isv_pgo_destroy(h); return rc; }
    *out = h;
    return ISV_OK;
}

// CombinedFactors::operator+ (include/factor/pose_graph_factors.h:27-51); host arithmetic on 6x6 matrices
extern "C" int isv_combined_factors_add(isv_combined_factors_t *acc, int32_t *acc_length, int64_t *acc_vio_index,
                                        const isv_combined_factors_t *other, int64_t other_vio_index) {
    if (!acc || !acc_length || !acc_vio_index || !other) return ISV_ERR_INVALID_ARG;
    const double *R0 = acc->relative_pose.delta_R, *t0 = acc->relative_pose.delta_t;
    const double *R1 = other->relative_pose.delta_R, *t1 = other->relative_pose.delta_t, *S = other->relative_pose.sqrt_info;
    double W[36], cov1[36], Adj[36] = {0}, T[36], info[36];
    for (int a = 0; a < 6; a++) for (int b = 0; b < 6; b++) { double s = 0; for (int k = 0; k < 6; k++) s += S[k * 6 + a] * S[k * 6 + b]; W[a * 6 + b] = s; }
    h_inv6(W, cov1);
    // Sophus::SE3d::Adj(): [[R, [t]x R], [0, R]]
    const double Sk[9] = {0, -t0[2], t0[1], t0[2], 0, -t0[0], -t0[1], t0[0], 0};
    double SR[9]; h_mm(Sk, R0, SR);
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) { Adj[a * 6 + b] = R0[a * 3 + b]; Adj[a * 6 + 3 + b] = SR[a * 3 + b]; Adj[(3 + a) * 6 + 3 + b] = R0[a * 3 + b]; }
    for (int a = 0; a < 6; a++) for (int b = 0; b < 6; b++) { double s = 0; for (int k = 0; k < 6; k++) s += Adj[a * 6 + k] * cov1[k * 6 + b]; T[a * 6 + b] = s; }
    for (int a = 0; a < 6; a++) for (int b = 0; b < 6; b++) { double s = 0; for (int k = 0; k < 6; k++) s += T[a * 6 + k] * Adj[b * 6 + k]; acc->covRel[a * 6 + b] += s; }
    acc->has_rollpitch = other->has_rollpitch; acc->rollpitch = other->rollpitch;
    double Rn[9], tn[3], v[3];
    h_mm(R0, R1, Rn); h_mv(R0, t1, v);
    for (int k = 0; k < 3; k++) tn[k] = v[k] + t0[k];
    memcpy(acc->relative_pose.delta_R, Rn, sizeof(Rn)); memcpy(acc->relative_pose.delta_t, tn, sizeof(tn));
    h_inv6(acc->covRel, info);
    double Lm[36]; memcpy(Lm, info, sizeof(Lm));                 // LLT (lower, reads the lower triangle), sqrt_info = L^T
    for (int j = 0; j < 6; j++) {
        double dd = Lm[j * 6 + j];
        for (int k = 0; k < j; k++) dd -= Lm[j * 6 + k] * Lm[j * 6 + k];
        Lm[j * 6 + j] = std::sqrt(dd);
        for (int i = j + 1; i < 6; i++) { double s = Lm[i * 6 + j]; for (int k = 0; k < j; k++) s -= Lm[i * 6 + k] * Lm[j * 6 + k]; Lm[i * 6 + j] = s / Lm[j * 6 + j]; }
    }
    for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) acc->relative_pose.sqrt_info[i * 6 + j] = j >= i ? Lm[j * 6 + i] : 0.0;
    acc->distance = std::sqrt(tn[0] * tn[0] + tn[1] * tn[1] + tn[2] * tn[2]);
    (*acc_length)++;
    if (*acc_vio_index == -1) { memcpy(acc->ti, other->ti, 24); memcpy(acc->Ri, other->Ri, 72); *acc_vio_index = other_vio_index; acc->ts = other->ts; }
    return ISV_OK;
}

// ---- the HIP side of a call -------------------------------------------------------------------------------------------
// step 4: the batch's arrays live in ONE pinned staging area kept with the handle (no zero-initialised vectors per call, and the
// copies to and from the device run at the pinned rate); it grows by a quarter more than is needed
static int pgo_stage(isv_pgo *h, PgCall &call) {
    const size_t need = call.sec_off[PGA_COUNT];
    if (need > h->pin_cap) {
        if (h->pin) (void)hipHostFree(h->pin);
        h->pin = nullptr; h->pin_cap = 0;
        PCHK(h, hipHostMalloc(&h->pin, need + need / 4, hipHostMallocDefault));
        h->pin_cap = need + need / 4;
    }
    pg_carve(call, h->pin);
    return ISV_OK;
}

// chunk c's range of every array of direction `dir` on the chunk's stream: staging -> device (PG_UP) or back (PG_DOWN)
static hipError_t pgo_copy_chunk(isv_pgo *h, const PgCall &call, int c, unsigned dir) {
    const auto &lo = call.off[call.chunk_lo(c)], &hi = call.off[call.chunk_lo(c + 1)];
    hipError_t e = hipSuccess;
    pg_for_each_array(call, h->d, PG_NO_GRAPH, [&](int a, unsigned role, auto *sp, auto *dp, size_t, const auto *) {
        if (!(role & dir) || hi[a] <= lo[a] || e != hipSuccess) return;
        const size_t bytes = sizeof(*sp) * (hi[a] - lo[a]);
        e = dir == PG_UP ? hipMemcpyAsync(dp + lo[a], sp + lo[a], bytes, hipMemcpyHostToDevice, h->cstream[c])
                         : hipMemcpyAsync(sp + lo[a], dp + lo[a], bytes, hipMemcpyDeviceToHost, h->cstream[c]);
    });
    return e;
}

// [uploads -> k_pgo between the chunk's two events -> results into the staging] on the chunk's stream
// (round 5) a call that leaves CUs idle gives every graph four wavefronts -- the same bits (k_pgo's header); ISV_PGO_WAVES=1 / 4 forces a form
static int pgo_enqueue_chunk(isv_pgo *h, const PgCall &call, int c, bool waves4, std::atomic<int> &first_chunk, std::string &msg) {
    const int g0 = call.chunk_lo(c), g1 = call.chunk_lo(c + 1);
    hipStream_t st = h->cstream[c];
    PMSG(msg, hipSetDevice(h->device));
    PMSG(msg, hipMemcpyAsync(h->d.graphs + g0, call.graphs.data() + g0, sizeof(PgGraph) * (size_t)(g1 - g0), hipMemcpyHostToDevice, st));     // (pageable, 80 B per graph)
    PMSG(msg, pgo_copy_chunk(h, call, c, PG_UP));
    PgDev dv = h->d; dv.g0 = g0;
    PMSG(msg, hipEventRecord(h->kev[c][0], st));
    if (waves4) hipLaunchKernelGGL(k_pgo<4>, dim3(g1 - g0), dim3(256), call.idx_bytes, st, dv);
    else hipLaunchKernelGGL(k_pgo<1>, dim3(g1 - g0), dim3(64), call.idx_bytes, st, dv);
    PMSG(msg, hipGetLastError());
    PMSG(msg, hipEventRecord(h->kev[c][1], st));
    PMSG(msg, pgo_copy_chunk(h, call, c, PG_DOWN));
    int exp = -1; first_chunk.compare_exchange_strong(exp, c);
    return ISV_OK;
}

static int pgo_drain_chunk(isv_pgo *h, const PgCall &call, int c, std::string &msg) {
    const hipError_t e1 = hipSetDevice(h->device), e2 = e1 == hipSuccess ? hipStreamSynchronize(h->cstream[c]) : e1;
    if (e2 != hipSuccess) { msg = std::string("hipStreamSynchronize: ") + hipGetErrorString(e2); return ISV_ERR_DEVICE; }
    pg_publish_results(call, c);
    return ISV_OK;
}

// step 6: the span of the chunks' kernels (the chunk enqueued first, fc, starts first), and the ISV_TRACE_HANDOVER lines
static void pgo_kernel_time(isv_pgo *h, int C, int fc) {
    float best = 0;
    for (int c = 0; c < C; c++) { float f = 0; if (hipEventElapsedTime(&f, h->kev[fc][0], h->kev[c][1]) == hipSuccess) best = std::max(best, f); else (void)hipGetLastError(); }
    h->last_kernel_ms = best;
}
static void pgo_trace(isv_pgo *h, const PgCall &call, const PgPipeTimes &tm, int fc, std::chrono::steady_clock::time_point tp0, std::chrono::steady_clock::time_point tp1) {
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const auto tp2 = tm.enq[call.C - 1], tp3 = tm.done[call.C - 1];      // the last chunk's enqueue, the last chunk's drain
    fprintf(stderr, "isv pgo batch: %d graphs: analysis %.2f ms, assembly %.2f ms, H2D + kernel + D2H %.2f ms (%.1f MB up), write-back %.2f ms\n", call.ng, ms(tp0, tp1), ms(tp1, tp2), ms(tp2, tp3),
            pg_upload_bytes(call, h->d) / 1e6, ms(tp3, std::chrono::steady_clock::now()));
    for (int c = 0; c < call.C; c++) {       // every chunk's kernel on the first chunk's clock, and when the host enqueued / found it drained
        float a = 0, b = 0;
        (void)hipEventElapsedTime(&a, h->kev[fc][0], h->kev[c][0]); (void)hipEventElapsedTime(&b, h->kev[fc][0], h->kev[c][1]); (void)hipGetLastError();
        fprintf(stderr, "  chunk %d: graphs [%d, %d): enqueued at %.2f ms, k_pgo %.2f .. %.2f ms after the first chunk's start, drained at %.2f ms\n", c, call.chunk_lo(c), call.chunk_lo(c + 1),
                ms(tp0, tm.enq[c]), a, b, ms(tp0, tm.done[c]));
    }
}

extern "C" int isv_pgo_optimize_batch(isv_pgo_t *h, int32_t ng, const int32_t *ns, isv_pg_keyframe_t *const *kfs, const int32_t *firsts,
                                      const int32_t *curs, isv_pgo_result_t *results) {
    // 1. the arguments
    if (!h || ng < 1 || !ns || !kfs || !firsts || !curs || !results) return ISV_ERR_INVALID_ARG;
    PCHK(h, hipSetDevice(h->device));
    if (ng > h->cfg.max_graphs) { h->err = "more graphs than max_graphs"; return ISV_ERR_CAPACITY; }
    if (h->cache.size() < (size_t)h->cfg.max_graphs) h->cache.resize((size_t)h->cfg.max_graphs);
    static const bool no_cache = getenv("ISV_PGO_NO_CACHE") != nullptr;       // (A/B and test hook; PROCESS-wide: read once, at the first call)
    PgCall call;
    call.ng = ng; call.ns = ns; call.kfs = kfs; call.firsts = firsts; call.curs = curs; call.results = results; call.slots = h->cache.data();
    call.T = pg_host_threads(ng); call.C = pg_chunk_count(ng);
    // 2. structure (the slot's, or analysed into it) and numbers of every graph, on the team
    const auto tp0 = std::chrono::steady_clock::now();
    int64_t hits = 0;
    PTRY(pg_prepare_batch(call, h->cfg, no_cache, h->err, &hits));
    const auto tp1 = std::chrono::steady_clock::now();
    h->cache_hits += hits;
    // 3. + 4. the graphs laid end to end, the staging grown and carved
    PTRY(pg_layout(call, h->d, h->cfg, h->cap, getenv("ISV_PGO_IDX_GLOBAL") != nullptr, h->err));
    PTRY(pgo_stage(h, call));
    h->d.idx_lds_rows = call.idx_lds_rows; h->d.idx_lds_cols = call.idx_lds_cols;
    h->last_blocks = (double)call.nblk_tot;
    // 5. the chunk pipeline
    bool waves4 = ng <= h->n_cus;
    if (const char *ev = getenv("ISV_PGO_WAVES")) waves4 = atoi(ev) > 1;
    std::atomic<int> first_chunk{-1};
    PgPipeTimes tm;
    const int rc = pg_run_pipeline(call, tm, h->err, [&](int g) { pg_assemble(call, h->d, g); },
                                   [&](int c, std::string &msg) { return pgo_enqueue_chunk(h, call, c, waves4, first_chunk, msg); },
                                   [&](int c, std::string &msg) { return pgo_drain_chunk(h, call, c, msg); }, [&](int g) { pg_write_back(call, g); });
    if (rc != ISV_OK) {
        for (int c = 0; c < call.C; c++) (void)hipStreamSynchronize(h->cstream[c]);      // nothing of this call stays in flight
        return rc;
    }
    // 6. kernel time, trace
    const int fc = first_chunk.load() < 0 ? 0 : first_chunk.load();
    pgo_kernel_time(h, call.C, fc);
    if (getenv("ISV_TRACE_HANDOVER")) pgo_trace(h, call, tm, fc, tp0, tp1);
    // 7. per-graph status
    return pg_batch_status(call, h->err);
}

extern "C" int isv_pgo_optimize(isv_pgo_t *h, int32_t n, isv_pg_keyframe_t *kf, int32_t first_looped_index, int32_t cur_index, isv_pgo_result_t *result) {
    isv_pg_keyframe_t *kfs[1] = {kf};
    return isv_pgo_optimize_batch(h, 1, &n, kfs, &first_looped_index, &cur_index, result);
}

// ./loop_pose_output.txt (pose_graph.cpp:412-423): `fixed` stream formatting (6 decimals)
extern "C" int isv_pgo_write_loop_pose_output(const char *path, int32_t n, const isv_pg_keyframe_t *kf) {
    if (!path || n < 0 || (n > 0 && !kf)) return ISV_ERR_INVALID_ARG;
    FILE *f = fopen(path, "w");
    if (!f) return ISV_ERR_INVALID_ARG;
    for (int k = 0; k < n; k++) {
        const HQ q = h_R2q(kf[k].R_w_i);
        fprintf(f, "%.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f\n", kf[k].time_stamp, kf[k].T_w_i[0], kf[k].T_w_i[1], kf[k].T_w_i[2], q.w, q.x, q.y, q.z);
    }
    fclose(f);
    return ISV_OK;
}
