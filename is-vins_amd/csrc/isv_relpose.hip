// isv_relpose.hip -- the relative-pose stage of the initialisation, batched: IMU excitation, then relativePose's candidates in
// order, each a cv::findFundamentalMat RANSAC and the reference's recoverPose; one 64-lane workgroup per problem
// (isv_relpose.h -- internal, not part of the public ABI -- has the contract, the reference lines, the restatements and the
// quirks R1..R5; the serial pieces are isv_init_common.h, shared with the CPU restatement tests/native/isv_relpose_oracle.c).
//
// Per candidate i: the correspondences of frames i and n_window - 1 are compacted into LDS in track order (a ballot prefix over
// 64 tracks at a time), as float32 (R1) with their double parallax.  Lane 0 sums the parallax in correspondence order.  The
// RANSAC runs speculatively in chunks of up to 64 hypotheses: its subsets do not depend on the models, so lane 0 draws the next
// chunk's subsets from the serial RNG stream (R4), each lane solves one 7-point system and counts the inliers of its <= 3
// models over the LDS points, and lane 0 then scans the chunk in iteration order, applying the keep rule and the niters update
// exactly as the serial loop does, and stops where it stops.  The kept model's mask and the four cheirality tests of
// recoverPose run a lane per correspondence; the counts are ballot popcounts.  Candidates run one after another.  No atomics;
// contraction is off for the whole translation unit.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "isv_stage_launch.h"
#include "isv_relpose.h"
#include "isv_init_common.h"

int isv_sfm_check_problem(const isv_sfm_problem_t *p, bool with_l);   // isv_sfm.hip

namespace {

constexpr int kLanes = 64;
constexpr int kMaxC = ISV_SFM_MAX_TRACKS;   // a track is a correspondence at most once

struct RpHdr {                    // host-packed per-problem record
    int32_t status, nw, nf, ntr, trk_off, obs_off, frame_off, pad;
};

enum { SH_FLAG = 0, SH_CNT, SH_MORE, SH_CHOSEN, SH_SOL, SH_END };

}  // namespace

__global__ void __launch_bounds__(kLanes) k_relpose(const RpHdr *__restrict__ hdrs, const isv_sfm_track_t *__restrict__ tracks,
                                                    const double *__restrict__ obs_g, const double *__restrict__ dv_g,
                                                    const double *__restrict__ sdt_g, isv_relpose_result_t *__restrict__ results,
                                                    int32_t *__restrict__ mask_out) {
    __shared__ float4 Lp[kMaxC];               // correspondence (x0 y0 x1 y1), float32 (R1)
    __shared__ double Lpar[kMaxC];             // its parallax |a.xy - b.xy| in doubles
    __shared__ int16_t Ltrk[kMaxC];            // its track
    __shared__ uint8_t Lm[kMaxC];              // bit 0: the kept model's inlier; bit 1 + s: cheirality of solution s
    __shared__ int16_t Lsub[kLanes][7];        // the chunk's subsets
    __shared__ double LF[kLanes][27];          // their models
    __shared__ int Lnm[kLanes], Lgood[kLanes][3];
    __shared__ double Lbest[9], LP[48];
    __shared__ int sh[SH_END];

    const RpHdr &H = hdrs[blockIdx.x];
    isv_relpose_result_t *res = results + blockIdx.x;
    const int t = threadIdx.x;
    if (t < ISV_ALIGN_MAX_WINDOW) {
        res->n_corres[t] = res->ransac_iters[t] = res->ransac_inliers[t] = res->recover_inliers[t] = res->solution[t] = -1;
        res->parallax[t] = -1.0;
    }
    if (t == 0) { res->l = -1; res->n_candidates = 0; }
    if (H.status != ISV_RELPOSE_OK) {
        if (t == 0) res->status = H.status;
        return;
    }
    const int nw = H.nw, last = nw - 1, ntr = H.ntr;
    const isv_sfm_track_t *tr = tracks + H.trk_off;
    const double *obs = obs_g + 2 * (size_t)H.obs_off;
    int32_t *mo = mask_out + H.trk_off;
    for (int j = t; j < ntr; j += kLanes) mo[j] = -1;

    // ---- stage 0: checkIMUExcitation (lane 0), before relativePose as in initialStructure ----
    if (t == 0) {
        const double var = isv_excitation_var(H.nf, dv_g + 3 * (size_t)H.frame_off, sdt_g + H.frame_off);
        res->excitation_var = var;
        sh[SH_FLAG] = var < 0.25;
        sh[SH_CHOSEN] = -1;
    }
    __syncthreads();
    if (sh[SH_FLAG]) {
        if (t == 0) res->status = ISV_RELPOSE_REFUSED_EXCITATION;
        return;
    }
    const float tf = (float)(RP_THRESH * RP_THRESH);   // R2
    const unsigned long long lt = t ? (~0ull >> (64 - t)) : 0ull;

    for (int i = 0; i < nw - 2; i++) {   // R5: i = n_window - 2 is never tried
        // ---- getCorresponding(i, last), compacted in track order ----
        int count = 0;
        for (int b = 0; b < ntr; b += kLanes) {
            const int j = b + t;
            bool q = false;
            if (j < ntr) { const isv_sfm_track_t T = tr[j]; q = T.start_frame <= i && T.start_frame + T.n_obs - 1 >= last; }
            const unsigned long long bal = __ballot(q);
            if (q) {
                const isv_sfm_track_t T = tr[j];
                const int pos = count + __popcll(bal & lt);
                const double *a = obs + 2 * (T.obs_off + i - T.start_frame), *c = obs + 2 * (T.obs_off + last - T.start_frame);
                Lp[pos] = make_float4((float)a[0], (float)a[1], (float)c[0], (float)c[1]);
                const double dx = a[0] - c[0], dy = a[1] - c[1];
                Lpar[pos] = sqrt(dx * dx + dy * dy);
                Ltrk[pos] = (int16_t)j;
            }
            count += __popcll(bal);
        }
        __syncthreads();
        if (t == 0) { res->n_candidates = i + 1; res->n_corres[i] = count; }
        if (count <= 20) continue;
        if (t == 0) {
            double sum = 0;
            for (int k = 0; k < count; k++) sum = sum + Lpar[k];
            const double avg = 1.0 * sum / count;
            res->parallax[i] = avg;
            sh[SH_FLAG] = avg * 460 > 30;
        }
        __syncthreads();
        if (!sh[SH_FLAG]) continue;

        // ---- findFundamentalMat: RANSACPointSetRegistrator::run, speculative chunks ----
        uint64_t rng = ~0ull;             // lane 0's: RNG((uint64)-1), fresh per call (R4)
        int iter = 0, niters = RP_MAX_ITERS, max_good = 0;   // lane 0's
        for (;;) {
            if (t == 0) {
                const int cnt = niters - iter < kLanes ? niters - iter : kLanes;
                for (int h = 0; h < cnt; h++) {
                    int idx[7];
                    rp_subset(&rng, count, idx);
                    for (int k = 0; k < 7; k++) Lsub[h][k] = (int16_t)idx[k];
                }
                sh[SH_CNT] = cnt;
            }
            __syncthreads();
            const int cnt = sh[SH_CNT];
            if (t < cnt) {
                double p[28];
                for (int k = 0; k < 7; k++) {
                    const float4 v = Lp[Lsub[t][k]];
                    p[4 * k] = v.x; p[4 * k + 1] = v.y; p[4 * k + 2] = v.z; p[4 * k + 3] = v.w;
                }
                int nm = rp_run7point(p, LF[t]);
                nm = nm < 1 || nm > 3 ? 0 : nm;
                Lnm[t] = nm;
                for (int m = 0; m < nm; m++) {
                    double F[9];
                    for (int k = 0; k < 9; k++) F[k] = LF[t][9 * m + k];
                    int g = 0;
                    for (int j = 0; j < count; j++) {
                        const float4 v = Lp[j];
                        g += (float)rp_fm_error(F, v.x, v.y, v.z, v.w) <= tf;   // R2
                    }
                    Lgood[t][m] = g;
                }
            }
            __syncthreads();
            if (t == 0) {   // the serial loop over this chunk, in iteration order
                for (int h = 0; h < cnt && iter < niters; h++, iter++)
                    for (int m = 0; m < Lnm[h]; m++) {
                        const int g = Lgood[h][m];
                        if (g > (max_good > 6 ? max_good : 6)) {
                            for (int k = 0; k < 9; k++) Lbest[k] = LF[h][9 * m + k];
                            max_good = g;
                            niters = rp_update_num_iters(RP_CONFIDENCE, (double)(count - g) / count, 7, niters);
                        }
                    }
                sh[SH_MORE] = iter < niters;
            }
            __syncthreads();
            if (!sh[SH_MORE]) break;
        }
        if (t == 0) {
            res->ransac_iters[i] = iter;
            res->ransac_inliers[i] = max_good;
            sh[SH_FLAG] = max_good > 0;
            if (max_good > 0) rp_decompose(Lbest, LP);   // R3: F of normalised points, as it is
        }
        __syncthreads();
        if (!sh[SH_FLAG]) continue;   // no model kept: the candidate fails (the reference would abort)

        // ---- the kept model's mask, then recoverPose's cheirality masks ANDed with it ----
        int good[4] = {0, 0, 0, 0};
        for (int b = 0; b < count; b += kLanes) {
            const int j = b + t;
            int bits = 0;
            if (j < count) {
                const float4 v = Lp[j];
                if ((float)rp_fm_error(Lbest, v.x, v.y, v.z, v.w) <= tf) {
                    bits = 1;
                    for (int s = 0; s < 4; s++) bits |= rp_cheirality(LP + 12 * s, v.x, v.y, v.z, v.w) << (1 + s);
                }
                Lm[j] = (uint8_t)bits;
            }
            for (int s = 0; s < 4; s++) good[s] += __popcll(__ballot((bits >> (1 + s)) & 1));
        }
        if (t == 0) {
            const int g1 = good[0], g2 = good[1], g3 = good[2], g4 = good[3];
            const int s = (g1 >= g2 && g1 >= g3 && g1 >= g4) ? 0 : (g2 >= g1 && g2 >= g3 && g2 >= g4) ? 1
                        : (g3 >= g1 && g3 >= g2 && g3 >= g4) ? 2 : 3;
            const int cnt_in = good[s];
            res->recover_inliers[i] = cnt_in;
            res->solution[i] = s + 1;
            if (cnt_in > 12) {
                const double *P = LP + 12 * s;
                for (int a = 0; a < 3; a++)
                    for (int c = 0; c < 3; c++) res->relative_R[a * 3 + c] = P[c * 4 + a];   // Rotation = R^T
                for (int a = 0; a < 3; a++)                                                   // Translation = -R^T t
                    res->relative_T[a] = (-P[a]) * P[3] + (-P[4 + a]) * P[7] + (-P[8 + a]) * P[11];
                res->l = i;
                res->status = ISV_RELPOSE_OK;
                sh[SH_CHOSEN] = i;
                sh[SH_SOL] = s;
            }
        }
        __syncthreads();
        if (sh[SH_CHOSEN] >= 0) {
            const int s = sh[SH_SOL];
            for (int j = t; j < count; j += kLanes) mo[Ltrk[j]] = (Lm[j] & 1) && ((Lm[j] >> (1 + s)) & 1);
            return;
        }
    }
    if (t == 0) res->status = ISV_RELPOSE_NO_RELATIVE_POSE;
}

namespace {

int map_status(int sfm_status) {
    return sfm_status == ISV_SFM_OK ? ISV_RELPOSE_OK : sfm_status == ISV_SFM_REFUSED_CAPACITY ? ISV_RELPOSE_REFUSED_CAPACITY
                                                                                              : ISV_RELPOSE_REFUSED_INPUT;
}

}  // namespace

extern "C" int isv_internal_relpose_last_ms(isv_backend_t *h, double out_ms[2]) { return init_last_ms(h, ISV_INIT_RELPOSE, out_ms); }

extern "C" int isv_internal_relpose_batch(isv_backend_t *h, int32_t n, const isv_sfm_problem_t *const *problems, isv_relpose_result_t *results,
                                          int32_t *const *masks) {
    StageCall call{init_ctx(h, ISV_INIT_RELPOSE), "isv_internal_relpose_batch"};
    if (const int rc = call.enter(n, problems, results); rc != ISV_OK || n == 0) return rc;
    std::vector<RpHdr> hd(n);
    size_t n_tr = 0, n_obs = 0, n_fr = 0;
    for (int i = 0; i < n; i++) {
        const isv_sfm_problem_t *p = problems[i];
        RpHdr &H = hd[i];
        memset(&H, 0, sizeof(H));
        H.status = map_status(isv_sfm_check_problem(p, false));
        if (H.status != ISV_RELPOSE_OK) continue;
        H.nw = p->n_window; H.nf = p->n_frames; H.ntr = p->n_tracks;
        H.trk_off = (int32_t)n_tr; H.obs_off = (int32_t)n_obs; H.frame_off = (int32_t)n_fr;
        n_tr += p->n_tracks; n_obs += p->n_obs; n_fr += p->n_frames;
    }
    if (n_tr > INT32_MAX || n_obs > INT32_MAX || n_fr > INT32_MAX) return call.fail(ISV_ERR_CAPACITY, "batch too large");
    // one upload block: [headers | tracks | obs | dv | sdt]; then, device only: results (zeroed before the launch), per-track masks
    BlockLayout L;
    const size_t o_hd = L.add(sizeof(RpHdr) * n), o_tr = L.add(sizeof(isv_sfm_track_t) * (n_tr + 1)), o_obs = L.add(16 * (n_obs + 1));
    const size_t o_dv = L.add(24 * (n_fr + 1)), o_sdt = L.add(8 * (n_fr + 1));
    std::vector<char> up(L.end);
    const size_t o_res = L.add(sizeof(isv_relpose_result_t) * n), o_mask = L.add(4 * (n_tr + 1));
    memcpy(up.data() + o_hd, hd.data(), sizeof(RpHdr) * n);
    for (int i = 0; i < n; i++) {
        const RpHdr &H = hd[i];
        if (H.status != ISV_RELPOSE_OK) continue;
        const isv_sfm_problem_t *p = problems[i];
        if (H.ntr) memcpy(up.data() + o_tr + sizeof(isv_sfm_track_t) * H.trk_off, p->tracks, sizeof(isv_sfm_track_t) * H.ntr);
        if (p->n_obs) memcpy(up.data() + o_obs + 16 * (size_t)H.obs_off, p->obs, 16 * (size_t)p->n_obs);
        memcpy(up.data() + o_dv + 24 * (size_t)H.frame_off, p->delta_v, 24 * (size_t)H.nf);
        memcpy(up.data() + o_sdt + 8 * (size_t)H.frame_off, p->sum_dt, 8 * (size_t)H.nf);
    }
    std::vector<int32_t> mk(n_tr + 1);
    return call.run(
        up, {{up.size(), o_mask}}, L.end,
        [&](char *d, auto &&) {
            hipLaunchKernelGGL(k_relpose, dim3(n), dim3(kLanes), 0, h->stream, (const RpHdr *)(d + o_hd), (const isv_sfm_track_t *)(d + o_tr),
                               (const double *)(d + o_obs), (const double *)(d + o_dv), (const double *)(d + o_sdt),
                               (isv_relpose_result_t *)(d + o_res), (int32_t *)(d + o_mask));
        },
        {{results, o_res, sizeof(isv_relpose_result_t) * n}, {masks ? mk.data() : nullptr, o_mask, 4 * n_tr}},
        [&] {
            if (masks)
                for (int i = 0; i < n; i++) {
                    if (!masks[i]) continue;
                    const RpHdr &H = hd[i];
                    if (H.status == ISV_RELPOSE_OK) memcpy(masks[i], mk.data() + H.trk_off, 4 * (size_t)H.ntr);   // (a refused input's n_tracks is not trusted)
                }
            return hipSuccess;
        });
}
