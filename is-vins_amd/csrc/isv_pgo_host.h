// isv_pgo_host.h -- the host half of the pose-graph call (isv_pgo_optimize_batch, isv_posegraph.hip): small 3x3 / SO(3) arithmetic,
// the structure record of a graph slot and its analysis, the per-call numbers, the ONE table of the call's arrays, the layout, the
// write-back, the host-thread team and the control flow of the chunk pipeline.  No HIP here: the device work of a chunk comes in as
// two callables (enqueue, drain), so tests/native/pgo_host_sanitize.cpp drives all of this with a stand-in device.  The library
// compiles this header as part of isv_posegraph.hip, so its arithmetic keeps that file's compiler and options.
#pragma once
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "../../include/isvins_posegraph.h"
#include "isv_pgo_types.h"

// ---- small host 3x3 / SO(3) arithmetic for the write-back (RelativePoseFactor::update, drift) ----------------------
namespace {
struct HQ { double w, x, y, z; };
void h_q2R(HQ q, double *R) {
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z, twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x, tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy; R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
HQ h_R2q(const double *m) {      // Eigen matrix -> quaternion
    HQ q; double t = m[0] + m[4] + m[8];
    if (t > 0) { t = std::sqrt(t + 1.0); q.w = 0.5 * t; t = 0.5 / t; q.x = (m[7] - m[5]) * t; q.y = (m[2] - m[6]) * t; q.z = (m[3] - m[1]) * t; return q; }
    int i = 0; if (m[4] > m[0]) i = 1; if (m[8] > m[i * 4]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1.0);
    double v[3]; v[i] = 0.5 * t; t = 0.5 / t;
    q.w = (m[k * 3 + j] - m[j * 3 + k]) * t; v[j] = (m[j * 3 + i] + m[i * 3 + j]) * t; v[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
    q.x = v[0]; q.y = v[1]; q.z = v[2];
    return q;
}
HQ h_qn(HQ a) { const double n = std::sqrt(a.w * a.w + a.x * a.x + a.y * a.y + a.z * a.z); return HQ{a.w / n, a.x / n, a.y / n, a.z / n}; }
HQ h_qinv(HQ a) { const double n2 = a.w * a.w + a.x * a.x + a.y * a.y + a.z * a.z; return HQ{a.w / n2, -a.x / n2, -a.y / n2, -a.z / n2}; }
HQ h_qmul(HQ a, HQ b) { return HQ{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z, a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x}; }
void h_mm(const double *A, const double *B, double *C) { for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { double s = 0; for (int k = 0; k < 3; k++) s += A[i * 3 + k] * B[k * 3 + j]; C[i * 3 + j] = s; } }
void h_mv(const double *A, const double *v, double *o) { for (int i = 0; i < 3; i++) o[i] = A[i * 3] * v[0] + A[i * 3 + 1] * v[1] + A[i * 3 + 2] * v[2]; }
void h_mtv(const double *A, const double *v, double *o) { for (int i = 0; i < 3; i++) o[i] = A[i] * v[0] + A[3 + i] * v[1] + A[6 + i] * v[2]; }
void h_log(HQ q, double *om) {   // Sophus SO3::log of a unit quaternion
    const double n2 = q.x * q.x + q.y * q.y + q.z * q.z, n = std::sqrt(n2);
    double f;
    if (n2 < 1e-20) f = 2.0 / q.w - 2.0 / 3.0 * n2 / (q.w * q.w * q.w);
    else if (std::fabs(q.w) < 1e-10) f = (q.w > 0 ? M_PI : -M_PI) / n;
    else f = 2.0 * std::atan(n / q.w) / n;
    om[0] = f * q.x; om[1] = f * q.y; om[2] = f * q.z;
}
HQ h_exp(const double *om) {
    const double t2 = om[0] * om[0] + om[1] * om[1] + om[2] * om[2], t = std::sqrt(t2);
    double im, re;
    if (t2 < 1e-20) { const double t4 = t2 * t2; im = 0.5 - t2 / 48.0 + t4 / 3840.0; re = 1.0 - t2 / 8.0 + t4 / 384.0; }
    else { im = std::sin(0.5 * t) / t; re = std::cos(0.5 * t); }
    return HQ{re, im * om[0], im * om[1], im * om[2]};
}
void h_R2ypr(const double *R, double *ypr) {     // Utility::R2ypr, degrees
    const double y = std::atan2(R[3], R[0]), p = std::atan2(-R[6], R[0] * std::cos(y) + R[3] * std::sin(y));
    const double r = std::atan2(R[2] * std::sin(y) - R[5] * std::cos(y), -R[1] * std::sin(y) + R[4] * std::cos(y));
    ypr[0] = y / M_PI * 180.0; ypr[1] = p / M_PI * 180.0; ypr[2] = r / M_PI * 180.0;
}
// RelativePoseFactor::update, solver overload (include/factor/relative_pose_factor.h:103-117)
void h_relpose_update(isv_relpose_t *f, const double *ti, const double *Ri, const double *tj, const double *Rj, const double *PSi, const double *PSj) {
    const HQ Qi{PSi[6], PSi[3], PSi[4], PSi[5]}, Qj{PSj[6], PSj[3], PSj[4], PSj[5]};
    double d_tj[3], d_ti[3], Qm[9], A[9], B[9], lgi[3], lgj[3], v1[3], v2[3];
    for (int k = 0; k < 3; k++) { d_tj[k] = PSj[k] - tj[k]; d_ti[k] = PSi[k] - ti[k]; }
    h_q2R(h_qinv(Qj), Qm); h_mm(Qm, Rj, A); h_log(h_qn(h_R2q(A)), lgj);
    h_q2R(h_qinv(Qi), Qm); h_mm(Qm, Ri, B); h_log(h_qn(h_R2q(B)), lgi);
    h_mtv(Ri, d_tj, v1); h_mtv(Ri, d_ti, v2);
    const double *t = f->delta_t;
    const double v3[3] = {t[1] * lgi[2] - t[2] * lgi[1], t[2] * lgi[0] - t[0] * lgi[2], t[0] * lgi[1] - t[1] * lgi[0]};     // skew(delta_t) * log
    for (int k = 0; k < 3; k++) f->delta_t[k] += v1[k] - v2[k] + v3[k];
    double Ji[9], w[3], E[9], T[9];
    h_q2R(h_qmul(h_qinv(Qj), Qi), Ji);
    for (int k = 0; k < 9; k++) Ji[k] = -Ji[k];
    h_mv(Ji, lgi, w);
    h_q2R(h_exp(w), E); h_mm(f->delta_R, E, T); memcpy(f->delta_R, T, sizeof(T));
    h_q2R(h_exp(lgj), E); h_mm(f->delta_R, E, T); memcpy(f->delta_R, T, sizeof(T));
}
void h_inv6(const double *Ain, double *Inv) {    // PartialPivLU inverse of a 6x6 (Eigen MatrixXd::inverse)
    double A[36]; memcpy(A, Ain, sizeof(A));
    int perm[6]; for (int i = 0; i < 6; i++) perm[i] = i;
    for (int k = 0; k < 6; k++) {
        int p = k; double best = std::fabs(A[k * 6 + k]);
        for (int i = k + 1; i < 6; i++) if (std::fabs(A[i * 6 + k]) > best) { best = std::fabs(A[i * 6 + k]); p = i; }
        if (p != k) { for (int j = 0; j < 6; j++) std::swap(A[k * 6 + j], A[p * 6 + j]); std::swap(perm[k], perm[p]); }
        for (int i = k + 1; i < 6; i++) { A[i * 6 + k] /= A[k * 6 + k]; for (int j = k + 1; j < 6; j++) A[i * 6 + j] -= A[i * 6 + k] * A[k * 6 + j]; }
    }
    for (int c = 0; c < 6; c++) {
        double x[6];
        for (int i = 0; i < 6; i++) x[i] = perm[i] == c ? 1.0 : 0.0;
        for (int i = 0; i < 6; i++) { double s = x[i]; for (int k = 0; k < i; k++) s -= A[i * 6 + k] * x[k]; x[i] = s; }
        for (int i = 5; i >= 0; i--) { double s = x[i]; for (int k = i + 1; k < 6; k++) s -= A[i * 6 + k] * x[k]; x[i] = s / A[i * 6 + i]; }
        for (int i = 0; i < 6; i++) Inv[i * 6 + c] = x[i];
    }
}
}  // namespace

// ---- the arrays of a call, by index (the table itself: pg_for_each_array below) -------------------------------------
// In the order of their sections in the pinned staging.  The seven from PGA_INDEX0 on are the index arrays of the structure.
enum PgArray { PGA_POSE, PGA_COV, PGA_EDGES, PGA_RES, PGA_FREE_OF, PGA_ADJ_PTR, PGA_ADJ, PGA_START, PGA_ROWPTR, PGA_COLPTR, PGA_COLROWS, PGA_COUNT, PGA_INDEX0 = PGA_FREE_OF };
enum : unsigned { PG_UP = 1, PG_DOWN = 2 };      // staging -> device before the kernel, device -> staging after it
constexpr int PG_MAX_CHUNKS = 4;

// ---- the STRUCTURE of one graph slot as the last call analysed it ---------------------------------------------------
// PoseGraph::optimizeCS re-optimises a graph that grew by at most one keyframe since the last loop closure; a batch that is
// optimised again -- the benchmark, a replay -- has the same topology slot by slot.  The record holds the parameter-block map, the
// free indices, adjacency, skyline, column patterns and the edges' integer fields, keyed by a hash of everything they depend on.
// It lives in the handle's slot: the analysis writes it there, a later call with the same key reads it there, and the assembly
// copies from there into the staging.  The numbers (poses, measurements, sqrt_info) are PgNumbers, refreshed every call.
struct PgEdgeTpl { int32_t kind, a, b, fa, fb, dim, robust, src; };     // src: the keyframe whose factor this residual block is
struct alignas(64) PgStructure {      // (a cache line of its own: neighbouring slots are written by different threads at the same time)
    uint64_t key = 0; bool valid = false;
    std::vector<uint64_t> raw;                    // the key tuple itself: a hash match alone would reuse another topology's structure on a collision
    std::vector<int> loc;                         // keyframe -> local pose index, -1 outside first_looped_index .. cur_index
    int cur_pos = -1, n_loops = 0;
    int32_t P1 = 0, nf = 0, nblk = 0;             // poses, free poses, skyline blocks
    std::vector<int32_t> index[PGA_COUNT - PGA_INDEX0];
    std::vector<PgEdgeTpl> edges;
    std::vector<int32_t> &ix(int a) { return index[a - PGA_INDEX0]; }
    const std::vector<int32_t> &ix(int a) const { return index[a - PGA_INDEX0]; }
};
// what one call adds to a slot's structure: the poses, read (and checked) before the staging exists and released once they are in
// it.  The PgEdge records -- ~240 KB per graph -- have no buffer of their own: the assembly fills them in place (pg_fill_edges).
struct alignas(64) PgNumbers {        // (as PgStructure: no two graphs' records in one cache line)
    std::vector<double> pose;
    const char *err = nullptr; int rc = ISV_OK; bool hit = false;
};

// the key of a keyframe list: everything the structure depends on (the hash only short-cuts the comparison: the tuple decides)
inline uint64_t pg_structure_key(int n, const isv_pg_keyframe_t *kf, int32_t first, int32_t cur, std::vector<uint64_t> &raw) {
    uint64_t key = 1469598103934665603ull;
    raw.clear(); raw.reserve(3 + 2 * (size_t)n);
    auto mix = [&](uint64_t v) { raw.push_back(v); key ^= v + 0x9e3779b97f4a7c15ull + (key << 6) + (key >> 2); };
    mix((uint64_t)n); mix((uint64_t)(uint32_t)first); mix((uint64_t)(uint32_t)cur);
    for (int k = 0; k < n; k++) {
        mix(((uint64_t)(uint32_t)kf[k].index << 32) | (uint32_t)kf[k].sequence);
        mix(((uint64_t)(kf[k].has_rollpitch != 0) << 33) | ((uint64_t)(kf[k].has_loop != 0) << 32) | (uint32_t)(kf[k].has_loop ? kf[k].loop_index : 0));
    }
    return key;
}

// parameter blocks: keyframes first_looped_index .. cur_index in list order (pose_graph.cpp:277-306); the first one and every
// keyframe of sequence 0 are constant
inline int pg_analyse_blocks(PgStructure &S, const isv_pgo_config_t &cfg, int n, const isv_pg_keyframe_t *kf, int32_t first, int32_t cur, const char **err) {
    S.loc.assign(n, -1); S.cur_pos = -1; S.n_loops = 0; S.edges.clear();
    for (auto &v : S.index) v.clear();
    int pi = 0;
    for (int k = 0; k < n; k++) {
        if (kf[k].index < first || S.cur_pos >= 0) continue;
        S.loc[k] = pi++;
        if (kf[k].index == cur) S.cur_pos = k;
    }
    if (S.cur_pos < 0) { *err = "cur_index is not in the keyframe list (or lies before first_looped_index)"; return ISV_ERR_INVALID_ARG; }
    if (pi > cfg.max_keyframes) { *err = "more keyframes than max_keyframes"; return ISV_ERR_CAPACITY; }
    S.P1 = pi;
    std::vector<int32_t> &free_of = S.ix(PGA_FREE_OF);
    free_of.assign(pi, -1);
    int nf = 0;
    for (int k = 0; k < n; k++) {
        if (S.loc[k] < 0) continue;
        const bool constant = kf[k].index == first || kf[k].sequence == 0;
        free_of[S.loc[k]] = constant ? -1 : nf++;
    }
    S.nf = nf;
    return ISV_OK;
}

// residual blocks of the keyframes BEFORE cur (pose_graph.cpp:309-339), then skyline + adjacency + column patterns
inline int pg_analyse_edges(PgStructure &S, const isv_pgo_config_t &cfg, int n, const isv_pg_keyframe_t *kf, const char **err) {
    const std::vector<int32_t> &fo = S.ix(PGA_FREE_OF);
    std::vector<int32_t> &adj_ptr = S.ix(PGA_ADJ_PTR), &adj = S.ix(PGA_ADJ), &start = S.ix(PGA_START), &rowptr = S.ix(PGA_ROWPTR), &colptr = S.ix(PGA_COLPTR), &colrows = S.ix(PGA_COLROWS);
    const int nf = S.nf, param_index = S.P1 - 1;
    std::vector<std::vector<int32_t>> adjl(nf);
    std::vector<int> st(nf);
    for (int f = 0; f < nf; f++) st[f] = f;
    auto add_edge = [&](int32_t kind, int32_t a, int32_t b, int32_t dim, int32_t robust, int32_t src) {
        const int32_t fa = fo[a], fb = kind == 0 ? -1 : fo[b];
        const int id = (int)S.edges.size();
        if (fa >= 0) adjl[fa].push_back((id << 1) | 0);
        if (kind != 0 && fb >= 0) adjl[fb].push_back((id << 1) | 1);
        if (kind != 0 && fa >= 0 && fb >= 0) { const int lo = std::min(fa, fb), hi = std::max(fa, fb); st[hi] = std::min(st[hi], lo); }
        S.edges.push_back(PgEdgeTpl{kind, a, b, fa, fb, dim, robust, src});
    };
    for (int k = 0; k < n; k++) {
        const int li = S.loc[k]; if (li < 0 || k == S.cur_pos) continue;
        if (kf[k].has_rollpitch) add_edge(0, li, li, 2, 0, k);
        if (li + 1 <= param_index) add_edge(1, li, li + 1, 6, 0, k);
        if (kf[k].has_loop) {
            int conn = -1;
            for (int m = 0; m < n; m++) if (kf[m].index == kf[k].loop_index) conn = S.loc[m];
            if (conn < 0) { *err = "loop_index outside the optimised range (the reference asserts loop_index >= first_looped_index)"; return ISV_ERR_INVALID_ARG; }
            add_edge(2, conn, li, 6, 1, k);
            S.n_loops++;
        }
    }
    int nb = 0;
    for (int f = 0; f < nf; f++) { adj_ptr.push_back((int32_t)adj.size()); adj.insert(adj.end(), adjl[f].begin(), adjl[f].end()); start.push_back(st[f]); rowptr.push_back(nb); nb += f - st[f] + 1; }
    adj_ptr.push_back((int32_t)adj.size()); rowptr.push_back(nb);
    S.nblk = nb;
    if (nb - 2 * nf > cfg.max_loop_blocks) { *err = "loop closures span more blocks than max_loop_blocks"; return ISV_ERR_CAPACITY; }
    std::vector<std::vector<int32_t>> cp(nf);
    for (int i = 0; i < nf; i++) for (int j = st[i]; j < i; j++) cp[j].push_back(i);
    for (int j = 0; j < nf; j++) { colptr.push_back((int32_t)colrows.size()); colrows.insert(colrows.end(), cp[j].begin(), cp[j].end()); }
    colptr.push_back((int32_t)colrows.size());
    return ISV_OK;
}

// ---- the numbers of a call: the poses (with THE non-finite check) and the residual blocks' records, written where `out` says ----
inline int pg_fill_poses(const PgStructure &S, int n, const isv_pg_keyframe_t *kf, PgNumbers &N) {
    N.pose.clear(); N.pose.reserve((size_t)S.P1 * 7);
    for (int k = 0; k < n; k++) {
        if (S.loc[k] < 0) continue;
        for (int c = 0; c < 9; c++) if (!(kf[k].vio_R_w_i[c] - kf[k].vio_R_w_i[c] == 0.0)) { N.err = "non-finite keyframe pose"; return ISV_ERR_NONFINITE; }
        const HQ q = h_qn(h_R2q(kf[k].vio_R_w_i));                    // tmp_q = tmp_r; tmp_q.normalize()
        N.pose.insert(N.pose.end(), {kf[k].vio_T_w_i[0], kf[k].vio_T_w_i[1], kf[k].vio_T_w_i[2], q.x, q.y, q.z, q.w});
    }
    return ISV_OK;
}
inline void pg_fill_edges(const PgStructure &S, const isv_pg_keyframe_t *kf, PgEdge *out) {
    for (size_t e = 0; e < S.edges.size(); e++) {
        const PgEdgeTpl &T = S.edges[e];
        const isv_pg_keyframe_t &k = kf[T.src];
        PgEdge &E = out[e];
        memset(&E, 0, sizeof(E));
        E.kind = T.kind; E.a = T.a; E.b = T.b; E.fa = T.fa; E.fb = T.fb; E.dim = T.dim; E.robust = T.robust;
        if (E.kind == 0) { memcpy(E.meas_R, k.rollpitch.R, 72); memcpy(E.sqrt_info, k.rollpitch.sqrt_info, 32); }
        else if (E.kind == 1) { memcpy(E.meas_t, k.relative_pose.delta_t, 24); memcpy(E.meas_R, k.relative_pose.delta_R, 72); memcpy(E.sqrt_info, k.relative_pose.sqrt_info, 288); }
        else {
            memcpy(E.meas_t, k.loop_info, 24);
            h_q2R(HQ{k.loop_info[3], k.loop_info[4], k.loop_info[5], k.loop_info[6]}, E.meas_R);
            for (int dd = 0; dd < 6; dd++) E.sqrt_info[dd * 6 + dd] = std::sqrt(k.loop_weight);
        }
    }
}

// One graph of a call, up to the point where it can no longer be refused: the slot's structure when nothing it depends on has
// changed (a hit), else analysed into the slot, with the poses read in between.  Hit and miss run the same sequence, so a graph is
// refused in the same order of checks either way: cur present, max_keyframes, non-finite pose, loop partner, max_loop_blocks.  A
// refusal leaves the slot invalid.  no_cache: the slot is storage but is never trusted.
inline int pg_prepare_graph(PgStructure &S, PgNumbers &N, const isv_pgo_config_t &cfg, int n, const isv_pg_keyframe_t *kf, int32_t first, int32_t cur, bool no_cache) {
    if (n < 1 || !kf) return ISV_ERR_INVALID_ARG;
    std::vector<uint64_t> raw;
    const uint64_t key = pg_structure_key(n, kf, first, cur, raw);
    N.hit = !no_cache && S.valid && S.key == key && (int)S.loc.size() == n && S.raw == raw;
    S.valid = false;
    int rc = ISV_OK;
    if (!N.hit && (rc = pg_analyse_blocks(S, cfg, n, kf, first, cur, &N.err)) != ISV_OK) return rc;
    if ((rc = pg_fill_poses(S, n, kf, N)) != ISV_OK) return rc;
    if (!N.hit && (rc = pg_analyse_edges(S, cfg, n, kf, &N.err)) != ISV_OK) return rc;
    if (!N.hit) { S.key = key; S.raw.swap(raw); }
    S.valid = true;
    return ISV_OK;
}

// ---- the host-thread team ------------------------------------------------------------------------------------------
// min(16, cores, graphs) threads; ISV_HOST_THREADS overrides the first two (read per call, here only)
inline int pg_host_threads(int ng) {
    int T = (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (const char *ev = getenv("ISV_HOST_THREADS")) T = atoi(ev);
    return std::max(1, std::min(T, ng));
}
// fn(0) .. fn(n_tasks - 1), handed out in order by an atomic counter to T threads (T == 1: the caller's)
template <typename Fn> inline void pg_team(int T, int n_tasks, Fn fn) {
    std::atomic<int> next{0};
    auto worker = [&] { for (int id; (id = next.fetch_add(1)) < n_tasks; ) fn(id); };
    if (T == 1) { worker(); return; }
    std::vector<std::thread> th;
    for (int k = 0; k < T; k++) th.emplace_back(worker);
    for (auto &x : th) x.join();
}

// ---- one call -------------------------------------------------------------------------------------------------------
struct PgCaps { size_t pose, edge, blk, adj, col; };       // what the handle's device pools hold
struct PgCall {
    int ng = 0; const int32_t *ns = nullptr; isv_pg_keyframe_t *const *kfs = nullptr; const int32_t *firsts = nullptr, *curs = nullptr;
    isv_pgo_result_t *results = nullptr;
    PgStructure *slots = nullptr;                          // [ng] the handle's
    int T = 1, C = 1;                                      // host threads, chunks
    std::vector<PgNumbers> nums;                           // [ng]
    std::vector<PgGraph> graphs;                           // [ng]
    std::vector<std::array<size_t, PGA_COUNT>> off;        // [ng + 1] element offset of graph g in every array; [ng]: the totals
    size_t sec_off[PGA_COUNT + 1] = {};                    // byte offset of every array's section in the staging; [PGA_COUNT]: its size
    char *sec[PGA_COUNT] = {};                             // the sections, once the staging is there (pg_carve)
    size_t nblk_tot = 0;
    int32_t idx_lds_rows = 0, idx_lds_cols = 0; size_t idx_bytes = 0;      // LDS copies of the envelope's index arrays (0: read from global memory)
    int chunk_lo(int c) const { return (int)((int64_t)ng * c / C); }
    int chunk_of(int g) const { int c = (int)(((int64_t)g * C) / ng); while (c + 1 < C && g >= chunk_lo(c + 1)) c++; while (c > 0 && g < chunk_lo(c)) c--; return c; }
};
// a batch of >= 64 graphs goes to the device in four chunks (ISV_PGO_CHUNKS overrides, read per call)
inline int pg_chunk_count(int ng) {
    int C = ng >= 64 ? PG_MAX_CHUNKS : 1;
    if (const char *ev = getenv("ISV_PGO_CHUNKS")) { C = atoi(ev); if (C < 1) C = 1; if (C > PG_MAX_CHUNKS) C = PG_MAX_CHUNKS; if (C > ng) C = ng; }
    return C;
}

// THE table of a call's arrays: visit(index, direction, staging section, device pointer, graph g's element count, graph g's host
// source or null) for every array, typed by its element.  `d` is the device's pointer record (PgDev; the stand-alone test's
// stand-in).  The layout, the assembly, the uploads, the downloads and the trace's byte count walk it; a walk that wants only the
// types and the pointers passes PG_NO_GRAPH and gets zero counts and null sources (it touches no graph's data).  A source-less
// upload (the edges) is filled in place by the assembly.  A new array is one line here (plus its member in PgDev and its use).
constexpr int PG_NO_GRAPH = -1;
template <typename Dev, typename Visit> inline void pg_for_each_array(const PgCall &call, Dev &d, int g, Visit visit) {
    const PgStructure *S = g < 0 ? nullptr : &call.slots[g];
    const double *pose_src = g < 0 ? nullptr : call.nums[g].pose.data();
#define PG_ARR(A, name, dir, T, cnt, src) visit((int)(A), (unsigned)(dir), (T *)call.sec[A], d.name, S ? (size_t)(cnt) : (size_t)0, (const T *)(S ? (src) : nullptr))
#define PG_IDX(A, name) PG_ARR(A, name, PG_UP, int32_t, S->ix(A).size(), S->ix(A).data())
    PG_ARR(PGA_POSE, pose, PG_UP | PG_DOWN, double, S->P1 * 7, pose_src);
    PG_ARR(PGA_COV, cov, PG_DOWN, double, S->P1 * 36, nullptr);
    PG_ARR(PGA_EDGES, edges, PG_UP, PgEdge, S->edges.size(), nullptr);
    PG_ARR(PGA_RES, res, PG_DOWN, isv_pgo_result_t, 1, nullptr);
    PG_IDX(PGA_FREE_OF, free_of); PG_IDX(PGA_ADJ_PTR, adj_ptr); PG_IDX(PGA_ADJ, adj); PG_IDX(PGA_START, start);
    PG_IDX(PGA_ROWPTR, rowptr); PG_IDX(PGA_COLPTR, colptr); PG_IDX(PGA_COLROWS, colrows);
#undef PG_IDX
#undef PG_ARR
}

// step 2: every graph's structure and numbers, on the team; the first refused graph in index order reports.  hits: graphs whose
// structure was reused (counted by the caller only when the whole batch passed)
inline int pg_prepare_batch(PgCall &call, const isv_pgo_config_t &cfg, bool no_cache, std::string &err, int64_t *hits) {
    call.nums.assign((size_t)call.ng, PgNumbers());
    pg_team(call.T, call.ng, [&](int g) { call.nums[g].rc = pg_prepare_graph(call.slots[g], call.nums[g], cfg, call.ns[g], call.kfs[g], call.firsts[g], call.curs[g], no_cache); });
    *hits = 0;
    for (int g = 0; g < call.ng; g++) {
        if (call.nums[g].rc != ISV_OK) { if (call.nums[g].err) err = call.nums[g].err; return call.nums[g].rc; }
        *hits += call.nums[g].hit;
    }
    return ISV_OK;
}

// step 3: the graphs laid end to end (serial, integers only): every array's offsets, the PgGraph records, the capacity check,
// the staging's sections (64-byte aligned) and whether the largest graph's index arrays fit into 48 KB of LDS
// (idx_global: test hook for the path graphs too large for the LDS copies take)
template <typename Dev> inline int pg_layout(PgCall &call, Dev &d, const isv_pgo_config_t &cfg, const PgCaps &cap, bool idx_global, std::string &err) {
    const int ng = call.ng;
    call.graphs.resize((size_t)ng);
    call.off.assign((size_t)ng + 1, std::array<size_t, PGA_COUNT>{});
    size_t nblk_tot = 0, nfree_tot = 0, max_nf = 0, max_cols = 0;
    for (int g = 0; g < ng; g++) {
        const PgStructure &S = call.slots[g]; const auto &o = call.off[g];
        PgGraph &G = call.graphs[g];
        memset(&G, 0, sizeof(G));
        G.P1 = S.P1; G.nf = S.nf; G.ne = (int32_t)S.edges.size(); G.nblk = S.nblk; G.max_iter = cfg.max_iterations; G.huber = cfg.huber_delta;
        G.pose0 = (int32_t)(o[PGA_POSE] / 7); G.free0 = (int32_t)nfree_tot; G.edge0 = (int32_t)o[PGA_EDGES]; G.blk0 = (int32_t)nblk_tot;
        G.adj0 = (int32_t)o[PGA_ADJ]; G.col0 = (int32_t)o[PGA_COLROWS]; G.vec0 = (int32_t)(6 * nfree_tot);
        pg_for_each_array(call, d, g, [&](int a, unsigned, auto *, auto *, size_t cnt, const auto *) { call.off[g + 1][a] = o[a] + cnt; });
        nblk_tot += (size_t)S.nblk; nfree_tot += (size_t)S.nf;
        max_nf = std::max(max_nf, (size_t)S.nf); max_cols = std::max(max_cols, (size_t)(S.nblk - S.nf));
    }
    const auto &e = call.off[ng];
    if (e[PGA_POSE] / 7 > cap.pose || e[PGA_EDGES] > cap.edge || nblk_tot > cap.blk || e[PGA_ADJ] > cap.adj || e[PGA_COLROWS] > cap.col) {
        err = "pose graphs exceed the handle's capacity"; return ISV_ERR_CAPACITY;
    }
    call.nblk_tot = nblk_tot;
    size_t q = 0;
    pg_for_each_array(call, d, PG_NO_GRAPH, [&](int a, unsigned, auto *sp, auto *, size_t, const auto *) { call.sec_off[a] = q; q += (e[a] * sizeof(*sp) + 63) & ~(size_t)63; });
    call.sec_off[PGA_COUNT] = q;
    call.idx_bytes = (3 * max_nf + 1 + max_cols) * sizeof(int32_t);
    call.idx_lds_rows = call.idx_lds_cols = 0;
    if (max_nf > 0 && call.idx_bytes <= 48 * 1024 && !idx_global) { call.idx_lds_rows = (int32_t)max_nf; call.idx_lds_cols = (int32_t)max_cols; } else call.idx_bytes = 0;
    return ISV_OK;
}
// step 4, once the staging block holds sec_off[PGA_COUNT] bytes
inline void pg_carve(PgCall &call, void *staging) { for (int a = 0; a < PGA_COUNT; a++) call.sec[a] = (char *)staging + call.sec_off[a]; }
// bytes that go up, for the trace line
template <typename Dev> inline size_t pg_upload_bytes(const PgCall &call, Dev &d) {
    size_t b = 0;
    pg_for_each_array(call, d, PG_NO_GRAPH, [&](int a, unsigned dir, auto *sp, auto *, size_t, const auto *) { if (dir & PG_UP) b += call.off[call.ng][a] * sizeof(*sp); });
    return b;
}

// graph g's arrays into their place in the staging: the ones with a host source are copied, the edge records are written there
// directly (no per-graph buffer of ~240 KB, no second pass over it)
template <typename Dev> inline void pg_assemble(PgCall &call, Dev &d, int g) {
    pg_for_each_array(call, d, g, [&](int a, unsigned dir, auto *sp, auto *, size_t cnt, const auto *src) { if ((dir & PG_UP) && cnt && src) memcpy(sp + call.off[g][a], src, sizeof(*sp) * cnt); });
    pg_fill_edges(call.slots[g], call.kfs[g], (PgEdge *)call.sec[PGA_EDGES] + call.off[g][PGA_EDGES]);
    call.nums[g] = PgNumbers();
}

// write back (pose_graph.cpp:362-407): updatePose, updateCov, the update() calls, drift, the keyframes after cur
inline void pg_write_back(PgCall &call, int g) {
    const int n = call.ns[g]; isv_pg_keyframe_t *kf = call.kfs[g];
    const PgStructure &S = call.slots[g]; const PgGraph &G = call.graphs[g];
    const double *pose = (const double *)call.sec[PGA_POSE], *cov = (const double *)call.sec[PGA_COV];
    isv_pgo_result_t &R = call.results[g];
    R.n_loop_edges = S.n_loops;
    const int param_index = G.P1 - 1;
    isv_pg_keyframe_t *last = nullptr; const double *last_pose = nullptr;
    for (int k = 0; k < n; k++) {
        const int li = S.loc[k]; if (li < 0) continue;
        const double *p = pose + (size_t)(G.pose0 + li) * 7;
        memcpy(kf[k].T_w_i, p, 24); h_q2R(HQ{p[6], p[3], p[4], p[5]}, kf[k].R_w_i);
        // (a graph whose covariance factorisation failed -- status ISV_ERR_NONFINITE -- keeps its keyframes' cov /
        // cov_computed as they were: the reference does not check ceres::Covariance::Compute's result and would
        // store whatever GetCovarianceBlock left; zeros marked "computed" are worse than no covariance)
        if (li < param_index && R.status == ISV_OK) {
            // ceres::Covariance::GetCovarianceBlock returns the 7x7 AMBIENT block [Sigma 0; 0 0]; the reference receives it in a
            // 36-double buffer and maps that as a column-major 6x6 (pose_graph.cpp:346-350): reproduced, stored row-major
            double c7[49] = {0};
            const double *S6 = cov + (size_t)(G.pose0 + li) * 36;
            for (int a = 0; a < 6; a++) for (int b = 0; b < 6; b++) c7[a * 7 + b] = S6[a * 6 + b];
            for (int a = 0; a < 6; a++) for (int b = 0; b < 6; b++) kf[k].cov[a * 6 + b] = c7[a + 6 * b];
            kf[k].cov_computed = 1;
        }
        if (last) h_relpose_update(&last->relative_pose, last->T_w_i, last->R_w_i, kf[k].T_w_i, kf[k].R_w_i, last_pose, p);
        last = &kf[k]; last_pose = p;
    }
    const isv_pg_keyframe_t &c = kf[S.cur_pos];
    double yc[3], yv[3], vT[9], t[3];
    h_R2ypr(c.R_w_i, yc); h_R2ypr(c.vio_R_w_i, yv);
    R.yaw_drift = yc[0] - yv[0];
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) vT[a * 3 + b] = c.vio_R_w_i[b * 3 + a];
    h_mm(c.R_w_i, vT, R.r_drift);
    h_mv(R.r_drift, c.vio_T_w_i, t);
    for (int k = 0; k < 3; k++) R.t_drift[k] = c.T_w_i[k] - t[k];
    for (int k = S.cur_pos + 1; k < n; k++) {
        double Pn[3], Rn[9];
        h_mv(R.r_drift, kf[k].vio_T_w_i, Pn); for (int dd = 0; dd < 3; dd++) Pn[dd] += R.t_drift[dd];
        h_mm(R.r_drift, kf[k].vio_R_w_i, Rn);
        memcpy(kf[k].T_w_i, Pn, 24); memcpy(kf[k].R_w_i, Rn, 72);
    }
}

// ---- the chunked pipeline: [assemble chunk c into the staging -> H2D -> k_pgo -> D2H] on stream c, then write-back ----
// One team of host threads walks 2 ng tasks in order: task g < ng is assemble(g), and the thread that completes a chunk's last
// graph enqueues the chunk; task ng + g is write_back(g), after the chunk has drained (the first thread to need a chunk drains it,
// the others wait for it).  Chunks are contiguous graph ranges, so every array of a chunk is ONE range of the batch's arrays and the
// offsets the kernel uses are the batch's.  enqueue(c, msg) / drain(c, msg) return a status and, on failure, its message: after the
// first failure nothing more is assembled, enqueued, drained or written back, and the call returns that status with err set.
struct PgPipeTimes { std::chrono::steady_clock::time_point enq[PG_MAX_CHUNKS], done[PG_MAX_CHUNKS]; };     // (trace) when the host had enqueued / found drained
template <typename Assemble, typename Enqueue, typename Drain, typename WriteBack>
inline int pg_run_pipeline(const PgCall &call, PgPipeTimes &tm, std::string &err, Assemble assemble, Enqueue enqueue, Drain drain, WriteBack write_back) {
    const int ng = call.ng, C = call.C;
    std::vector<std::atomic<int>> left((size_t)C), enq((size_t)C), done((size_t)C);
    for (int c = 0; c < C; c++) { left[c].store(call.chunk_lo(c + 1) - call.chunk_lo(c)); enq[c].store(0); done[c].store(0); }
    std::atomic<int> fail_rc{ISV_OK};
    std::mutex err_mu, done_mu[PG_MAX_CHUNKS];
    auto device_step = [&](auto &step, int c) {
        if (fail_rc.load() != ISV_OK) return;
        std::string msg;
        const int rc = step(c, msg);
        if (rc == ISV_OK) return;
        std::lock_guard<std::mutex> lk(err_mu);
        if (fail_rc.load() == ISV_OK) { fail_rc.store(rc); err = msg; }
    };
    pg_team(call.T, 2 * ng, [&](int id) {
        if (id < ng) {
            const int g = id, c = call.chunk_of(g);
            if (fail_rc.load() == ISV_OK) assemble(g);
            if (left[c].fetch_sub(1) == 1) {
                device_step(enqueue, c);
                tm.enq[c] = std::chrono::steady_clock::now();
                enq[c].store(1);
            }
        } else {
            const int g = id - ng, c = call.chunk_of(g);
            if (!done[c].load()) {
                std::lock_guard<std::mutex> lk(done_mu[c]);
                if (!done[c].load()) {
                    while (!enq[c].load()) std::this_thread::yield();
                    device_step(drain, c);
                    tm.done[c] = std::chrono::steady_clock::now();
                    done[c].store(1);
                }
            }
            if (fail_rc.load() == ISV_OK) write_back(g);
        }
    });
    return fail_rc.load();
}

// the last act of a drain: the result records come back through the staging and go to the caller's (pageable) array from there
inline void pg_publish_results(const PgCall &call, int c) {
    const int g0 = call.chunk_lo(c), g1 = call.chunk_lo(c + 1);
    memcpy(call.results + g0, (const isv_pgo_result_t *)call.sec[PGA_RES] + g0, sizeof(isv_pgo_result_t) * (size_t)(g1 - g0));
}

// step 7: per-graph failures surface in the return value too (every graph has been written back by now; results[g].status says which)
inline int pg_batch_status(const PgCall &call, std::string &err) {
    for (int g = 0; g < call.ng; g++) if (call.results[g].status != ISV_OK) { err = "pose graph " + std::to_string(g) + ": the covariance factorisation failed (poses written, covariances left untouched)"; return call.results[g].status; }
    return ISV_OK;
}
