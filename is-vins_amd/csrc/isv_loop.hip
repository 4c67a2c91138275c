// isv_loop.hip -- batched loop-closure verification, KeyFrame::findConnection for many keyframe pairs in one call
// (include/isvins_loop.h has the contract, the reference lines, the restated OpenCV pieces, the quirks L1..L6 and the
// deviations; the serial pieces are isv_loop_common.h / isv_pnp.h / isv_init_common.h, shared with the CPU restatement
// tests/native/isv_loop_oracle.c).  One packed upload, two kernels, one download (isv_stage_launch.h).
//
// k_loop_match: one workgroup of four wavefronts per pair, integers only.  The old keyframe's descriptors pass through an LDS
// tile of kTile descriptors, stored as two planes of 16 bytes per descriptor so that consecutive lanes read consecutive
// 16-byte slots (a [kTile][32 B] array read with 128-bit loads would be 2-way bank conflicted).  A wavefront takes one window
// descriptor at a time (wave-uniform), its lanes stride over the tile: XOR, popcount, a running key (dist << 20) | index.  The
// wave-wide minimum of the keys is the serial loop's answer (L2: smallest distance, then smallest index) and is carried
// across tiles in a per-point word.  Wavefront 0 then compacts the accepted matches in point order by a ballot prefix.
//
// k_loop_pnp: one 64-lane workgroup per pair, FP64, no atomics, contraction off for the translation unit.  The RANSAC runs
// speculatively in chunks of up to 64 hypotheses as k_relpose does: lane 0 draws the chunk's subsets from the serial RNG
// stream, a lane per hypothesis runs EPnP on its five points and counts its inliers, lane 0 replays the serial loop over the
// chunk in iteration order.  The kept model's mask is a lane per point, its inliers are compacted by a ballot prefix; L^T L of
// the DLT is a lane per entry over the points in order, its eigen-decomposition and the pose are lane 0's; the CvLevMarq loop
// is isv_pnp.h's workgroup form; loop_weight's residuals are a lane per point and lane 0 sums them in point order.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "isv_stage_launch.h"
#include "isv_loop_common.h"

struct isv_loop : StageHandle {
    isv_loop_config_t cfg;
};

namespace {

constexpr int kLanes = 64;
constexpr int kMatchWaves = 4, kMatchThreads = kMatchWaves * kLanes;
constexpr int kTile = 512;        // descriptors per LDS tile: 2 planes x 16 B x 512 = 16 KiB, several workgroups per CU
constexpr int kIndexBits = 20;    // key = (dist << 20) | index: max_keypoints <= 2^20, dist <= 256

struct LpHdr {                    // host-packed per-pair record
    int32_t status, np, nk, old_index, pt_off, kp_off, pad[2];
    double oT[3], oR[9];
};

enum { SH_CNT = 0, SH_MORE, SH_FLAG, SH_END };

}  // namespace

__global__ void __launch_bounds__(kMatchThreads) k_loop_match(const LpHdr *__restrict__ hdrs, const uint64_t *__restrict__ wbrief,
                                                              const float *__restrict__ p3d, const uint64_t *__restrict__ kbrief,
                                                              const float *__restrict__ kpn, uint32_t *__restrict__ keys,
                                                              int32_t *__restrict__ match_index, int32_t *__restrict__ match_dist,
                                                              lp_match_t *__restrict__ list, isv_loop_result_t *__restrict__ results,
                                                              int max_dist, int accept_dist) {
    __shared__ ulonglong2 La[kTile], Lb[kTile];   // words 0 1 / words 2 3 of the tile's descriptors
    const LpHdr &H = hdrs[blockIdx.x];
    if (H.status != ISV_LOOP_OK) return;
    const int t = threadIdx.x, lane = t & (kLanes - 1), wv = t / kLanes;
    const int np = H.np, nk = H.nk;
    const uint64_t *wb = wbrief + 4 * (size_t)H.pt_off, *kb = kbrief + 4 * (size_t)H.kp_off;
    uint32_t *key = keys + H.pt_off;
    const uint32_t none = (uint32_t)max_dist << kIndexBits;   // L2: bestDist = max_dist, bestIndex = -1
    for (int i = t; i < np; i += kMatchThreads) key[i] = none;
    for (int k0 = 0; k0 < nk; k0 += kTile) {
        const int cnt = min(kTile, nk - k0);
        __syncthreads();
        for (int j = t; j < cnt; j += kMatchThreads) {
            const uint64_t *d = kb + 4 * (size_t)(k0 + j);
            La[j] = make_ulonglong2(d[0], d[1]);
            Lb[j] = make_ulonglong2(d[2], d[3]);
        }
        __syncthreads();
        for (int i = wv; i < np; i += kMatchWaves) {   // point i stays with wavefront i % kMatchWaves in every tile
            const uint64_t *w = wb + 4 * (size_t)i;
            const uint64_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
            uint32_t best = none;
            for (int j = lane; j < cnt; j += kLanes) {
                const ulonglong2 a = La[j], b = Lb[j];
                const uint32_t dist = __popcll(a.x ^ w0) + __popcll(a.y ^ w1) + __popcll(b.x ^ w2) + __popcll(b.y ^ w3);
                const uint32_t k = (dist << kIndexBits) | (uint32_t)(k0 + j);
                best = k < best ? k : best;   // a candidate counts only below max_dist: every other key is >= none
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(best, off); best = o < best ? o : best; }
            if (lane == 0) { const uint32_t old = key[i]; key[i] = best < old ? best : old; }
        }
    }
    __syncthreads();
    if (wv != 0) return;
    // searchByBRIEFDes' status and reduceVector, in point order
    const float *X = p3d + 3 * (size_t)H.pt_off, *kp = kpn + 2 * (size_t)H.kp_off;
    int32_t *mi = match_index + H.pt_off, *md = match_dist + H.pt_off;
    lp_match_t *out = list + H.pt_off;
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    int count = 0;
    for (int b = 0; b < np; b += kLanes) {
        const int i = b + lane;
        bool q = false;
        int idx = -1;
        if (i < np) {
            const uint32_t k = key[i];
            const int dist = (int)(k >> kIndexBits);
            const bool found = dist < max_dist;
            idx = found ? (int)(k & ((1u << kIndexBits) - 1)) : -1;
            mi[i] = idx;
            md[i] = found ? dist : max_dist;
            q = found && dist < accept_dist;
        }
        const unsigned long long bal = __ballot(q);
        if (q) {   // L6: no uniqueness test
            lp_match_t m;
            m.X[0] = X[3 * i]; m.X[1] = X[3 * i + 1]; m.X[2] = X[3 * i + 2];
            m.uv[0] = kp[2 * idx]; m.uv[1] = kp[2 * idx + 1];
            m.src = i;
            out[count + __popcll(bal & lt)] = m;
        }
        count += __popcll(bal);
    }
    if (lane == 0) results[blockIdx.x].n_matched = count;
}

__global__ void __launch_bounds__(kLanes) k_loop_pnp(const isv_loop_config_t cfg, const LpHdr *__restrict__ hdrs, const lp_match_t *__restrict__ list,
                                                     isv_loop_result_t *__restrict__ results, int32_t *__restrict__ inlier,
                                                     double *__restrict__ pnp_pts, double *__restrict__ terms) {
    __shared__ int Lsub[kLanes][5];               // the chunk's subsets
    __shared__ double Lmod[kLanes][6];            // their models (rvec, tvec)
    __shared__ int Lgood[kLanes];
    __shared__ double Lbest[6], LA[144], LV[144], pm[P_END], stage[kLanes * 14], LR[9], LT[3];
    __shared__ int sh[SH_END];

    const LpHdr &H = hdrs[blockIdx.x];
    isv_loop_result_t *res = results + blockIdx.x;
    const int t = threadIdx.x;
    const int n = res->n_matched;                 // k_loop_match's (0 for a refused pair)
    __syncthreads();
    if (t == 0) { res->ransac_iters = -1; res->pnp_iterations = -1; res->loop_index = -1; res->n_final = n; }
    if (H.status != ISV_LOOP_OK) {
        if (t == 0) res->status = H.status;
        return;
    }
    int32_t *inl = inlier + H.pt_off;
    for (int i = t; i < H.np; i += kLanes) inl[i] = -1;
    const int gate = lp_match_gate(&cfg, n);      // L1
    if (gate != ISV_LOOP_OK) {
        if (t == 0) res->status = gate;
        return;
    }
    const lp_match_t *pts = list + H.pt_off;
    double *pp = pnp_pts + LP_PT * (size_t)H.pt_off, *term = terms + H.pt_off;
    const double td = cfg.ransac_threshold * cfg.ransac_threshold;
    const float tf = (float)td;
    const unsigned long long lt = t ? (~0ull >> (64 - t)) : 0ull;
    __syncthreads();

    // ---- solvePnPRansac: RANSACPointSetRegistrator::run, speculative chunks ----
    uint64_t rng = ~0ull;                         // lane 0's: RNG((uint64)-1), fresh per call
    int iter = 0, niters = cfg.ransac_iterations, max_good = 0;   // lane 0's
    for (;;) {
        if (t == 0) {
            const int cnt = niters - iter < kLanes ? niters - iter : kLanes;
            for (int h = 0; h < cnt; h++) rp_subset_m(&rng, n, 5, Lsub[h]);
            sh[SH_CNT] = cnt;
        }
        __syncthreads();
        const int cnt = sh[SH_CNT];
        if (t < cnt) {
            double model[6], work[288];
            int idx[5];
            for (int k = 0; k < 5; k++) idx[k] = Lsub[t][k];
            const int ok = lp_ransac_model(pts, idx, model, work);   // L4: no guess
            Lgood[t] = ok ? lp_count_inliers(model, n, pts, tf, td) : 0;
            for (int k = 0; k < 6; k++) Lmod[t][k] = model[k];
        }
        __syncthreads();
        if (t == 0) {   // the serial loop over this chunk, in iteration order
            for (int h = 0; h < cnt && iter < niters; h++, iter++) {
                const int g = Lgood[h];
                if (g > (max_good > 4 ? max_good : 4)) {
                    for (int k = 0; k < 6; k++) Lbest[k] = Lmod[h][k];
                    max_good = g;
                    niters = rp_update_num_iters(cfg.ransac_confidence, (double)(n - g) / n, 5, niters);
                }
            }
            sh[SH_MORE] = iter < niters;
        }
        __syncthreads();
        if (!sh[SH_MORE]) break;
    }
    if (t == 0) {
        res->ransac_iters = iter;
        res->ransac_inliers = max_good;
        sh[SH_FLAG] = max_good > 0;
    }
    __syncthreads();
    if (!sh[SH_FLAG]) {   // no model: solvePnPRansac returns false with an empty inlier list
        for (int j = t; j < n; j += kLanes) inl[pts[j].src] = 0;
        if (t == 0) { res->status = ISV_LOOP_PNP_FAILED; res->n_final = 0; }
        return;
    }

    // ---- the kept model's mask; its inliers compacted in order, as doubles, for the final solve ----
    int cnt_in = 0;
    {
        double Rb[9], mb[6];
        for (int k = 0; k < 6; k++) mb[k] = Lbest[k];
        rodrigues_v2m(mb, Rb, nullptr);
        for (int b = 0; b < n; b += kLanes) {
            const int j = b + t;
            bool q = false;
            if (j < n) {
                q = lp_is_inlier(Rb, mb + 3, pts + j, tf, td);
                inl[pts[j].src] = q;
            }
            const unsigned long long bal = __ballot(q);
            if (q) {
                double *P = pp + LP_PT * (size_t)(cnt_in + __popcll(bal & lt));
                P[0] = pts[j].X[0]; P[1] = pts[j].X[1]; P[2] = pts[j].X[2]; P[3] = pts[j].uv[0]; P[4] = pts[j].uv[1];
            }
            cnt_in += __popcll(bal);
        }
    }
    if (t == 0) res->n_final = cnt_in;
    if (!((double)cnt_in > 0.6 * cfg.min_loop_num)) {   // findConnection returns false whatever the final solve yields
        if (t == 0) res->status = ISV_LOOP_PNP_FAILED;
        return;
    }
    __syncthreads();

    // ---- solvePnP(SOLVEPNP_ITERATIVE) over the inliers: planarity, the DLT, CvLevMarq ----
    if (t == 0) sh[SH_FLAG] = lp_dlt_planar(cnt_in, pp);
    __syncthreads();
    if (sh[SH_FLAG]) {
        if (t == 0) res->status = ISV_LOOP_PLANAR;
        return;
    }
    for (int e = t; e < 78; e += kLanes) {   // the lower triangle of L^T L
        int a = 0;
        while ((a + 1) * (a + 2) / 2 <= e) a++;
        const int b = e - a * (a + 1) / 2;
        LA[12 * a + b] = lp_dlt_entry(cnt_in, pp, a, b);
    }
    __syncthreads();
    if (t == 0) lp_dlt_pose(LA, LV, pm + P_PAR, pm + P_PAR + 3);
    __syncthreads();
    const int iters = pnp_solve(cnt_in, pp, LP_PT, pm, stage);

    // ---- keyframe.cpp:200-227, :274-292 ----
    if (t == 0) {
        res->pnp_iterations = iters;
        lp_old_pose(pm + P_PAR, pm + P_PAR + 3, LR, LT);
    }
    __syncthreads();
    for (int j = t; j < n; j += kLanes)
        if (inl[pts[j].src] == 1) term[j] = lp_weight_term(LR, LT, pm + P_PAR + 3, pts + j, cfg.focal_length);   // L3
    __syncthreads();
    if (t == 0) {
        double sum = 0;
        int m = 0;
        for (int j = 0; j < n; j++)
            if (inl[pts[j].src] == 1) { m++; sum += term[j]; }
        lp_finish(&cfg, LR, LT, H.oT, H.oR, sum, m, H.old_index, res);
    }
}

namespace {

bool finite_f(const float *v, size_t n) {
    for (size_t k = 0; k < n; k++) if (!std::isfinite(v[k])) return false;
    return true;
}
bool finite_d(const double *v, size_t n) {
    for (size_t k = 0; k < n; k++) if (!std::isfinite(v[k])) return false;
    return true;
}

int check_pair(const isv_loop_config_t &c, const isv_loop_pair_t *p) {
    if (p->n_points < 0 || p->n_keypoints < 0) return ISV_LOOP_INPUT;
    if (p->n_points > 0 && (!p->window_brief || !p->point_3d)) return ISV_LOOP_INPUT;
    if (p->n_keypoints > 0 && (!p->brief || !p->keypoints_norm)) return ISV_LOOP_INPUT;
    if (p->n_points > c.max_points || p->n_keypoints > c.max_keypoints) return ISV_LOOP_CAPACITY;
    if (!finite_f(p->point_3d, 3 * (size_t)p->n_points) || !finite_f(p->keypoints_norm, 2 * (size_t)p->n_keypoints) ||
        !finite_d(p->origin_vio_T, 3) || !finite_d(p->origin_vio_R, 9)) return ISV_LOOP_INPUT;
    return ISV_LOOP_OK;
}

}  // namespace

extern "C" const char *isv_loop_last_error(const isv_loop_t *h) { return h ? h->err.c_str() : "null handle"; }

extern "C" void isv_loop_destroy(isv_loop_t *h) {
    if (!h) return;
    h->close();
    delete h;
}

extern "C" int isv_loop_create(const isv_loop_config_t *c, isv_loop_t **out) {
    if (!c || !out) return ISV_ERR_INVALID_ARG;
    *out = nullptr;
    // (min_loop_num >= 9: more than 0.6 min_loop_num matches are then more than the RANSAC's five model points)
    if (c->max_pairs < 1 || c->max_points < 1 || c->max_keypoints < 1 || c->max_keypoints > (1 << kIndexBits) || c->min_loop_num < 9 ||
        c->ransac_iterations < 1 || c->match_accept_dist < 1 || c->match_accept_dist > c->match_max_dist || c->match_max_dist > 256 ||
        !finite_d(c->ric, 9) || !finite_d(c->tic, 3) || !(c->focal_length > 0) || !(c->ransac_threshold > 0) ||
        !(c->ransac_confidence > 0 && c->ransac_confidence < 1) || !(c->max_yaw_deg > 0) || !(c->max_distance > 0))
        return ISV_ERR_INVALID_ARG;
    isv_loop *h = new isv_loop();
    h->cfg = *c;
    if (stage_open_failed("isv_loop_create", h->open())) {
        isv_loop_destroy(h);
        return ISV_ERR_DEVICE;
    }
    *out = h;
    return ISV_OK;
}

extern "C" int isv_loop_last_ms(isv_loop_t *h, double out_ms[3]) {
    if (!h || !out_ms) return ISV_ERR_INVALID_ARG;
    out_ms[0] = h->slot.call_ms; out_ms[1] = h->slot.part_ms[0]; out_ms[2] = h->slot.part_ms[1];
    return ISV_OK;
}

extern "C" int isv_loop_apply(const isv_loop_result_t *r, isv_pg_keyframe_t *cur) {
    if (!r || !cur) return ISV_ERR_INVALID_ARG;
    cur->loop_weight = r->loop_weight;            // keyframe.cpp:223-227 (0 where PnPRANSAC did not run)
    if (r->status != ISV_LOOP_OK) return ISV_OK;
    cur->has_loop = 1;                            // :285-289
    cur->loop_index = r->loop_index;
    memcpy(cur->loop_info, r->loop_info, sizeof(cur->loop_info));
    return ISV_OK;
}

extern "C" int isv_loop_verify_batch(isv_loop_t *h, int32_t n, const isv_loop_pair_t *const *pairs, isv_loop_result_t *results,
                                     int32_t *const *match_index, int32_t *const *match_dist, int32_t *const *inlier) {
    StageCall call{h ? h->ctx() : StageCtx{}, "isv_loop_verify_batch"};
    if (const int rc = call.enter(n, pairs, results); rc != ISV_OK || n == 0) return rc;
    if (n > h->cfg.max_pairs) return call.fail(ISV_ERR_CAPACITY, "more pairs than max_pairs");
    std::vector<LpHdr> hd(n);
    size_t n_pt = 0, n_kp = 0;
    for (int i = 0; i < n; i++) {
        const isv_loop_pair_t *p = pairs[i];
        LpHdr &H = hd[i];
        memset(&H, 0, sizeof(H));
        H.status = check_pair(h->cfg, p);
        if (H.status != ISV_LOOP_OK) continue;
        H.np = p->n_points; H.nk = p->n_keypoints; H.old_index = p->old_index;
        H.pt_off = (int32_t)n_pt; H.kp_off = (int32_t)n_kp;
        memcpy(H.oT, p->origin_vio_T, sizeof(H.oT)); memcpy(H.oR, p->origin_vio_R, sizeof(H.oR));
        n_pt += p->n_points; n_kp += p->n_keypoints;
    }
    if (n_pt > INT32_MAX || n_kp > INT32_MAX) return call.fail(ISV_ERR_CAPACITY, "batch too large");
    // one upload block: [headers | window descriptors | 3-D points | old descriptors | old corners]; then, device only: results
    // (zeroed before the launch), the per-point keys / outputs, the matched list, the final solve's points, the residual terms
    BlockLayout L;
    const size_t o_hd = L.add(sizeof(LpHdr) * n), o_wb = L.add(32 * (n_pt + 1)), o_x = L.add(12 * (n_pt + 1));
    const size_t o_kb = L.add(32 * (n_kp + 1)), o_kp = L.add(8 * (n_kp + 1));
    std::vector<char> up(L.end);
    const size_t o_res = L.add(sizeof(isv_loop_result_t) * n), o_key = L.add(4 * (n_pt + 1)), o_mi = L.add(4 * (n_pt + 1));
    const size_t o_md = L.add(4 * (n_pt + 1)), o_in = L.add(4 * (n_pt + 1)), o_list = L.add(sizeof(lp_match_t) * (n_pt + 1));
    const size_t o_pp = L.add(8 * LP_PT * (n_pt + 1)), o_term = L.add(8 * (n_pt + 1));
    memcpy(up.data() + o_hd, hd.data(), sizeof(LpHdr) * n);
    for (int i = 0; i < n; i++) {
        const LpHdr &H = hd[i];
        if (H.status != ISV_LOOP_OK) continue;
        const isv_loop_pair_t *p = pairs[i];
        if (H.np) {
            memcpy(up.data() + o_wb + 32 * (size_t)H.pt_off, p->window_brief, 32 * (size_t)H.np);
            memcpy(up.data() + o_x + 12 * (size_t)H.pt_off, p->point_3d, 12 * (size_t)H.np);
        }
        if (H.nk) {
            memcpy(up.data() + o_kb + 32 * (size_t)H.kp_off, p->brief, 32 * (size_t)H.nk);
            memcpy(up.data() + o_kp + 8 * (size_t)H.kp_off, p->keypoints_norm, 8 * (size_t)H.nk);
        }
    }
    std::vector<int32_t> mi(match_index ? n_pt + 1 : 0), md(match_dist ? n_pt + 1 : 0), in(inlier ? n_pt + 1 : 0);
    const isv_loop_config_t cfg = h->cfg;
    hipStream_t stream = h->stream;
    return call.run(
        up, {{up.size(), o_key}}, L.end,
        [&](char *d, auto &&mark) {
            hipLaunchKernelGGL(k_loop_match, dim3(n), dim3(kMatchThreads), 0, stream, (const LpHdr *)(d + o_hd), (const uint64_t *)(d + o_wb),
                               (const float *)(d + o_x), (const uint64_t *)(d + o_kb), (const float *)(d + o_kp), (uint32_t *)(d + o_key),
                               (int32_t *)(d + o_mi), (int32_t *)(d + o_md), (lp_match_t *)(d + o_list), (isv_loop_result_t *)(d + o_res),
                               (int)cfg.match_max_dist, (int)cfg.match_accept_dist);
            mark();
            hipLaunchKernelGGL(k_loop_pnp, dim3(n), dim3(kLanes), 0, stream, cfg, (const LpHdr *)(d + o_hd), (const lp_match_t *)(d + o_list),
                               (isv_loop_result_t *)(d + o_res), (int32_t *)(d + o_in), (double *)(d + o_pp), (double *)(d + o_term));
        },
        {{results, o_res, sizeof(isv_loop_result_t) * n}, {match_index ? mi.data() : nullptr, o_mi, 4 * n_pt},
         {match_dist ? md.data() : nullptr, o_md, 4 * n_pt}, {inlier ? in.data() : nullptr, o_in, 4 * n_pt}},
        [&] {
            for (int i = 0; i < n; i++) {
                const LpHdr &H = hd[i];
                if (H.status != ISV_LOOP_OK || !H.np) continue;   // (a refused pair's n_points is not trusted)
                if (match_index && match_index[i]) memcpy(match_index[i], mi.data() + H.pt_off, 4 * (size_t)H.np);
                if (match_dist && match_dist[i]) memcpy(match_dist[i], md.data() + H.pt_off, 4 * (size_t)H.np);
                if (inlier && inlier[i]) memcpy(inlier[i], in.data() + H.pt_off, 4 * (size_t)H.np);
            }
            return hipSuccess;
        });
}
