// isv_keyframe.hip -- batched keyframe extraction: cv::FAST, the BRIEF descriptors of the corners and of the window points and
// liftProjective of every corner, for many 8-bit images in one call (include/isvins_keyframe.h has the contract, the reference
// lines, the restated OpenCV pieces and the quirks K1..K6; the serial CPU restatement is tests/native/isv_kf_oracle.c).
// One packed upload, four kernels, one download (isv_stage_launch.h).  Integers everywhere except the lift.
//
// k_kf_blur: one workgroup per 64 x 16 tile.  The tile and a 4-pixel halo go into LDS with BORDER_REFLECT_101 applied on the way
// in, so that neither pass sees a border; the row pass fills a 16-bit LDS plane of (16 + 8) x 64, the column pass reads it.
// k_kf_fast: the same tiling with a 3-pixel halo (zero outside the image: no candidate's circle reaches it).  A lane per pixel:
// OpenCV's early-out on the compass pairs, then the arc test on two 16-bit masks, then the score by windowed minima.  It writes
// a byte per pixel of the image: the score, 0 where there is no corner.
// k_kf_select: one workgroup per image.  The non-maximum suppression against the score map, counted per row by ballots, an
// exclusive scan over the rows, then the ordered write of (x, y, score) by ballot prefix within the row: row-major order without
// an atomic.  The count is written even when it exceeds max_keypoints; nothing else is written then.
// k_kf_brief: one wavefront per corner or window point.  Lane l evaluates tests 64 w + l for w = 0..3 on the blurred image (global
// memory: an image stays in L2); the four ballots ARE the descriptor's words.  Lane 0 lifts a corner.  An image's corners go to
// the compact output arrays behind those of the images before it (their counts are summed by wavefront 0 of each workgroup).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "isv_stage_launch.h"
#include "isv_keyframe.h"
#include "isv_pinhole.h"

namespace {

constexpr int kLanes = 64;
constexpr int kTW = 64, kTH = 16, kThreads = 256;     // the blur's and FAST's tile, their workgroup
constexpr int kSelThreads = 512;                       // k_kf_select: eight wavefronts share an image's rows
constexpr int kBriefBlocks = 16, kBriefWaves = 4;      // k_kf_brief: 64 wavefronts stride over an image's points
constexpr int kMaxSide = 8192;                         // x and y share a 32-bit word; the row offsets fit 32 KiB of LDS

struct KfHdr {                    // host-packed per-item record
    int32_t status, W, H, np;
    int32_t pt_off, slot_off, pad[2];   // into the window points; into the per-image corner lists
    uint64_t img_off;             // into the packed images (and the blurred images, and the score maps)
};

struct KfLast { int32_t status, W, H; uint64_t img_off; };

}  // namespace

struct isv_kf : StageHandle {
    isv_kf_config_t cfg;
    PinholeCam cam;
    double pack_ms = 0;           // the host's packing of the last successful call
    int8_t *d_pattern = nullptr;  // [4][256]: x1, y1, x2, y2
    std::vector<char> up;         // the upload block's host image (grow-only: an image batch is large)
    std::vector<KfLast> last;     // the last successful call's items, for the debug read-back
    size_t last_blur = 0, last_smap = 0;
};

// BORDER_REFLECT_101 (cv::borderInterpolate): always inside [0, len)
__device__ __forceinline__ int kf_reflect(int p, int len) {
    if (len == 1) return 0;
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}

__global__ void __launch_bounds__(kThreads) k_kf_blur(const KfHdr *__restrict__ hdrs, const uint8_t *__restrict__ img, uint8_t *__restrict__ blur) {
    constexpr int K[9] = {7, 17, 32, 46, 52, 46, 32, 17, 7};
    __shared__ uint8_t raw[kTH + 8][kTW + 8];
    __shared__ uint16_t rowp[kTH + 8][kTW];
    const KfHdr &H = hdrs[blockIdx.z];
    if (H.status != ISV_KF_OK) return;
    const int W = H.W, Hh = H.H, x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH, t = threadIdx.x;
    if (x0 >= W || y0 >= Hh) return;
    const uint8_t *src = img + H.img_off;
    uint8_t *dst = blur + H.img_off;
    for (int idx = t; idx < (kTH + 8) * (kTW + 8); idx += kThreads) {
        const int ly = idx / (kTW + 8), lx = idx % (kTW + 8);
        raw[ly][lx] = src[(size_t)kf_reflect(y0 + ly - 4, Hh) * W + kf_reflect(x0 + lx - 4, W)];
    }
    __syncthreads();
    for (int idx = t; idx < (kTH + 8) * kTW; idx += kThreads) {
        const int ly = idx / kTW, lx = idx % kTW;
        int s = 0;
#pragma unroll
        for (int k = 0; k < 9; k++) s += K[k] * raw[ly][lx + k];
        rowp[ly][lx] = (uint16_t)s;               // at most 255 * 256
    }
    __syncthreads();
    for (int idx = t; idx < kTH * kTW; idx += kThreads) {
        const int ly = idx / kTW, lx = idx % kTW, gx = x0 + lx, gy = y0 + ly;
        if (gx >= W || gy >= Hh) continue;
        int s = 0;
#pragma unroll
        for (int k = 0; k < 9; k++) s += K[k] * rowp[ly + k][lx];
        dst[(size_t)gy * W + gx] = (uint8_t)((s + 32768) >> 16);
    }
}

// 9 contiguous bits of the 16-bit circular mask m
__device__ __forceinline__ bool kf_arc9(uint32_t m) {
    const uint32_t m32 = m | (m << 16);
    uint32_t r = m32 & (m32 >> 1);
    r &= r >> 2;
    r &= r >> 4;                                  // bit i: bits i .. i + 7
    return ((r & (m32 >> 8)) & 0xFFFFu) != 0;
}

__global__ void __launch_bounds__(kThreads) k_kf_fast(const KfHdr *__restrict__ hdrs, const uint8_t *__restrict__ img, uint8_t *__restrict__ smap, int thr) {
    constexpr int OX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    constexpr int OY[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
    __shared__ uint8_t raw[kTH + 6][kTW + 6];
    const KfHdr &H = hdrs[blockIdx.z];
    if (H.status != ISV_KF_OK) return;
    const int W = H.W, Hh = H.H, x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH, t = threadIdx.x;
    if (x0 >= W || y0 >= Hh) return;
    const uint8_t *src = img + H.img_off;         // K4: the raw image
    uint8_t *dst = smap + H.img_off;
    for (int idx = t; idx < (kTH + 6) * (kTW + 6); idx += kThreads) {
        const int ly = idx / (kTW + 6), lx = idx % (kTW + 6), gy = y0 + ly - 3, gx = x0 + lx - 3;
        raw[ly][lx] = (gx >= 0 && gx < W && gy >= 0 && gy < Hh) ? src[(size_t)gy * W + gx] : 0;
    }
    __syncthreads();
    for (int idx = t; idx < kTH * kTW; idx += kThreads) {
        const int ly = idx / kTW, lx = idx % kTW, gx = x0 + lx, gy = y0 + ly;
        if (gx >= W || gy >= Hh) continue;
        int score = 0;
        if (gx >= 3 && gx < W - 3 && gy >= 3 && gy < Hh - 3) {
            const int v = raw[ly + 3][lx + 3];
            int p[16];
#pragma unroll
            for (int k = 0; k < 16; k++) p[k] = raw[ly + 3 + OY[k]][lx + 3 + OX[k]];
            // 1: darker than v - t, 2: brighter than v + t (OpenCV's threshold table)
#define KF_CLS(k) (p[k] < v - thr ? 1 : p[k] > v + thr ? 2 : 0)
            int d = KF_CLS(0) | KF_CLS(8);
            if (d) d &= (KF_CLS(2) | KF_CLS(10)) & (KF_CLS(4) | KF_CLS(12)) & (KF_CLS(6) | KF_CLS(14));
            if (d) d &= (KF_CLS(1) | KF_CLS(9)) & (KF_CLS(3) | KF_CLS(11)) & (KF_CLS(5) | KF_CLS(13)) & (KF_CLS(7) | KF_CLS(15));
#undef KF_CLS
            if (d) {
                uint32_t dark = 0, bright = 0;
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    dark |= (uint32_t)(p[k] < v - thr) << k;
                    bright |= (uint32_t)(p[k] > v + thr) << k;
                }
                if (((d & 1) && kf_arc9(dark)) || ((d & 2) && kf_arc9(bright))) {
                    // K3: cornerScore<16>.  lo[k] / hi[k]: the minimum / maximum of d over the arc k .. k + 8
                    int lo[16], hi[16], q[16];
#pragma unroll
                    for (int k = 0; k < 16; k++) q[k] = v - p[k];
#pragma unroll
                    for (int k = 0; k < 16; k++) { lo[k] = min(q[k], q[(k + 1) & 15]); hi[k] = max(q[k], q[(k + 1) & 15]); }
                    int lo4[16], hi4[16];
#pragma unroll
                    for (int k = 0; k < 16; k++) { lo4[k] = min(lo[k], lo[(k + 2) & 15]); hi4[k] = max(hi[k], hi[(k + 2) & 15]); }
                    int a0 = thr, b0 = -thr;
#pragma unroll
                    for (int k = 0; k < 16; k++) {
                        const int a = min(min(lo4[k], lo4[(k + 4) & 15]), q[(k + 8) & 15]);
                        const int b = max(max(hi4[k], hi4[(k + 4) & 15]), q[(k + 8) & 15]);
                        a0 = max(a0, a);
                        b0 = min(b0, b);
                    }
                    score = max(a0, -b0) - 1;     // in [thr, 254]
                }
            }
        }
        dst[(size_t)gy * W + gx] = (uint8_t)score;
    }
}

// the corner at (x, y) with score s > 0 survives: K2, strictly greater than all eight neighbours (they are inside the image: a
// non-zero score sits at least 3 pixels from every border)
__device__ __forceinline__ bool kf_keeps(const uint8_t *sm, int W, int x, int y, int s) {
    const uint8_t *c = sm + (size_t)y * W + x;
    return s > c[-1] && s > c[1] && s > c[-W - 1] && s > c[-W] && s > c[-W + 1] && s > c[W - 1] && s > c[W] && s > c[W + 1];
}

__global__ void __launch_bounds__(kSelThreads) k_kf_select(const KfHdr *__restrict__ hdrs, const uint8_t *__restrict__ smap, uint32_t *__restrict__ kp_xy,
                                                            uint8_t *__restrict__ kp_sc, isv_kf_result_t *__restrict__ results, int max_keypoints) {
    extern __shared__ int rowoff[];               // [H]: the row's count, then its exclusive offset
    __shared__ int s_total;
    const KfHdr &H = hdrs[blockIdx.x];
    if (H.status != ISV_KF_OK) return;
    const int W = H.W, Hh = H.H, t = threadIdx.x, lane = t & (kLanes - 1), wv = t / kLanes;
    constexpr int nw = kSelThreads / kLanes;
    const uint8_t *sm = smap + H.img_off;
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int y = wv; y < Hh; y += nw) {
        int cnt = 0;
        if (y >= 3 && y < Hh - 3)
            for (int xb = 0; xb < W; xb += kLanes) {
                const int x = xb + lane;
                const int s = x < W ? sm[(size_t)y * W + x] : 0;
                if (__ballot(s != 0) == 0) continue;
                cnt += __popcll(__ballot(s != 0 && kf_keeps(sm, W, x, y, s)));
            }
        if (lane == 0) rowoff[y] = cnt;
    }
    __syncthreads();
    if (wv == 0) {
        int carry = 0;
        for (int yb = 0; yb < Hh; yb += kLanes) {
            const int y = yb + lane;
            const int c = y < Hh ? rowoff[y] : 0;
            int inc = c;
#pragma unroll
            for (int off = 1; off < kLanes; off <<= 1) { const int o = __shfl_up(inc, off); if (lane >= off) inc += o; }
            if (y < Hh) rowoff[y] = carry + inc - c;
            carry += __shfl(inc, kLanes - 1);
        }
        if (lane == 0) s_total = carry;
    }
    __syncthreads();
    const int total = s_total;
    const bool fits = total <= max_keypoints;
    if (t == 0) {
        isv_kf_result_t r;
        r.status = fits ? ISV_KF_OK : ISV_KF_CAPACITY; r.n_keypoints = total; r.n_points = H.np; r._pad = 0;
        results[blockIdx.x] = r;
    }
    if (!fits) return;
    uint32_t *oxy = kp_xy + H.slot_off;
    uint8_t *osc = kp_sc + H.slot_off;
    for (int y = 3 + wv; y < Hh - 3; y += nw) {
        int at = rowoff[y];
        if (at == (y + 1 < Hh ? rowoff[y + 1] : total)) continue;      // an empty row
        for (int xb = 0; xb < W; xb += kLanes) {
            const int x = xb + lane;
            const int s = x < W ? sm[(size_t)y * W + x] : 0;
            if (__ballot(s != 0) == 0) continue;
            const bool keep = s != 0 && kf_keeps(sm, W, x, y, s);
            const unsigned long long bal = __ballot(keep);
            if (keep) {
                const int o = at + __popcll(bal & lt);
                oxy[o] = (uint32_t)x | ((uint32_t)y << 16);
                osc[o] = (uint8_t)s;
            }
            at += __popcll(bal);
        }
    }
}

// (int) of a float32, toward zero (K1); a value outside int's range is outside every image
__device__ __forceinline__ int kf_trunc(float f) { return (f > -2147483648.0f && f < 2147483648.0f) ? (int)f : -1; }

__global__ void __launch_bounds__(kBriefWaves * kLanes) k_kf_brief(const KfHdr *__restrict__ hdrs, const isv_kf_result_t *__restrict__ results,
                                                                    const uint8_t *__restrict__ blur, const int8_t *__restrict__ pattern,
                                                                    const float *__restrict__ pts, const uint32_t *__restrict__ kp_xy,
                                                                    const uint8_t *__restrict__ kp_sc, const PinholeCam cam, uint64_t *__restrict__ brief,
                                                                    float *__restrict__ uv, float *__restrict__ norm, uint8_t *__restrict__ score,
                                                                    uint64_t *__restrict__ wbrief) {
    __shared__ int8_t pat[4][256];
    __shared__ int s_off;
    const int item = blockIdx.y;
    const KfHdr &H = hdrs[item];
    if (H.status != ISV_KF_OK || results[item].status != ISV_KF_OK) return;
    const int t = threadIdx.x, lane = t & (kLanes - 1), wv = t / kLanes;
    for (int i = t; i < 1024; i += kBriefWaves * kLanes) pat[i >> 8][i & 255] = pattern[i];
    if (wv == 0) {                                // the corners of the images before this one
        int sum = 0;
        for (int j = lane; j < item; j += kLanes)
            if (hdrs[j].status == ISV_KF_OK && results[j].status == ISV_KF_OK) sum += results[j].n_keypoints;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == 0) s_off = sum;
    }
    __syncthreads();
    const int W = H.W, Hh = H.H, nk = results[item].n_keypoints, np = H.np;
    const uint8_t *im = blur + H.img_off;         // K4: the blurred image
    const size_t k_off = (size_t)s_off;
    for (int j = blockIdx.x * kBriefWaves + wv; j < nk + np; j += gridDim.x * kBriefWaves) {
        const bool corner = j < nk;
        float px, py;
        uint32_t xy = 0;
        if (corner) {
            xy = kp_xy[H.slot_off + j];
            px = (float)(xy & 0xFFFFu); py = (float)(xy >> 16);
        } else {
            const float *p = pts + 2 * (size_t)(H.pt_off + (j - nk));
            px = p[0]; py = p[1];
        }
        unsigned long long word = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const int i = 64 * w + lane;
            const int x1 = kf_trunc(px + (float)pat[0][i]), y1 = kf_trunc(py + (float)pat[1][i]);
            const int x2 = kf_trunc(px + (float)pat[2][i]), y2 = kf_trunc(py + (float)pat[3][i]);
            bool bit = false;                     // K5: an end outside the image leaves the bit 0
            if (x1 >= 0 && x1 < W && y1 >= 0 && y1 < Hh && x2 >= 0 && x2 < W && y2 >= 0 && y2 < Hh)
                bit = im[(size_t)y1 * W + x1] < im[(size_t)y2 * W + x2];
            const unsigned long long bal = __ballot(bit);
            if (lane == w) word = bal;
        }
        uint64_t *dst = corner ? brief + 4 * (k_off + j) : wbrief + 4 * (size_t)(H.pt_off + (j - nk));
        if (lane < 4) dst[lane] = word;
        if (corner && lane == 0) {
            const size_t o = k_off + j;
            uv[2 * o] = px; uv[2 * o + 1] = py;
            score[o] = kp_sc[H.slot_off + j];
            pinhole_lift(cam, px, py, &norm[2 * o], &norm[2 * o + 1]);       // PinholeCamera::liftProjective (isv_pinhole.h)
        }
    }
}

namespace {

int check_item(const isv_kf_config_t &c, const isv_kf_item_t *it) {
    if (it->width < 0 || it->height < 0 || it->n_points < 0 || it->stride < it->width) return ISV_KF_INPUT;
    if (it->width > 0 && it->height > 0 && !it->image) return ISV_KF_INPUT;
    if (it->n_points > 0 && !it->point_2d_uv) return ISV_KF_INPUT;
    if (it->width > c.max_width || it->height > c.max_height || it->n_points > c.max_points) return ISV_KF_CAPACITY;
    for (size_t k = 0; k < 2 * (size_t)it->n_points; k++)
        if (!std::isfinite(it->point_2d_uv[k])) return ISV_KF_INPUT;
    return ISV_KF_OK;
}

}  // namespace

extern "C" const char *isv_kf_last_error(const isv_kf_t *h) { return h ? h->err.c_str() : "null handle"; }

extern "C" void isv_kf_destroy(isv_kf_t *h) {
    if (!h) return;
    h->close();
    if (h->d_pattern) (void)hipFree(h->d_pattern);
    delete h;
}

extern "C" int isv_kf_create(const isv_kf_config_t *c, isv_kf_t **out) {
    if (!c || !out) return ISV_ERR_INVALID_ARG;
    *out = nullptr;
    if (c->max_items < 1 || c->max_items > 65535 || c->max_width < 1 || c->max_width > kMaxSide || c->max_height < 1 || c->max_height > kMaxSide ||
        c->max_keypoints < 1 || c->max_points < 1 || c->fast_threshold < 1 || c->fast_threshold > 254)
        return ISV_ERR_INVALID_ARG;
    for (int i = 0; i < ISV_KF_PATTERN_BITS; i++)
        for (const int8_t v : {c->x1[i], c->y1[i], c->x2[i], c->y2[i]})
            if (v < -ISV_KF_PATTERN_RADIUS || v > ISV_KF_PATTERN_RADIUS) return ISV_ERR_INVALID_ARG;
    for (const double v : {c->fx, c->fy, c->cx, c->cy, c->k1, c->k2, c->p1, c->p2})
        if (!std::isfinite(v)) return ISV_ERR_INVALID_ARG;
    if (!(c->fx > 0) || !(c->fy > 0)) return ISV_ERR_INVALID_ARG;
    isv_kf *h = new isv_kf();
    h->cfg = *c;
    h->cam = pinhole_make(c->fx, c->fy, c->cx, c->cy, c->k1, c->k2, c->p1, c->p2);
    hipError_t e = h->open();
    if (e == hipSuccess) e = hipMalloc(&h->d_pattern, 4 * ISV_KF_PATTERN_BITS);
    if (e == hipSuccess) {
        int8_t pat[4 * ISV_KF_PATTERN_BITS];
        memcpy(pat, c->x1, 256); memcpy(pat + 256, c->y1, 256); memcpy(pat + 512, c->x2, 256); memcpy(pat + 768, c->y2, 256);
        e = hipMemcpy(h->d_pattern, pat, sizeof(pat), hipMemcpyHostToDevice);
    }
    if (stage_open_failed("isv_kf_create", e)) {
        isv_kf_destroy(h);
        return ISV_ERR_DEVICE;
    }
    *out = h;
    return ISV_OK;
}

extern "C" int isv_kf_last_ms(isv_kf_t *h, double out_ms[7]) {
    if (!h || !out_ms) return ISV_ERR_INVALID_ARG;
    out_ms[0] = h->slot.call_ms;
    for (int i = 0; i < 4; i++) out_ms[1 + i] = h->slot.part_ms[i];   // blur, FAST, select, BRIEF
    out_ms[5] = h->slot.upload_ms; out_ms[6] = h->pack_ms;
    return ISV_OK;
}

extern "C" int isv_kf_extract_batch(isv_kf_t *h, int32_t n, const isv_kf_item_t *const *items, isv_kf_result_t *results, uint64_t *const *brief,
                                    float *const *keypoints_uv, float *const *keypoints_norm, uint8_t *const *score, uint64_t *const *window_brief) {
    StageCall call{h ? h->ctx() : StageCtx{}, "isv_kf_extract_batch"};
    if (const int rc = call.enter(n, items, results); rc != ISV_OK || n == 0) return rc;
    if (n > h->cfg.max_items) return call.fail(ISV_ERR_CAPACITY, "more items than max_items");
    if (!brief || !keypoints_uv || !keypoints_norm || !score || !window_brief) return call.fail(ISV_ERR_INVALID_ARG, "null output arrays");
    const isv_kf_config_t &cfg = h->cfg;
    std::vector<KfHdr> hd(n);
    size_t n_px = 0, n_pt = 0, n_slot = 0;
    int maxW = 0, maxH = 0;
    for (int i = 0; i < n; i++) {
        const isv_kf_item_t *it = items[i];
        KfHdr &H = hd[i];
        memset(&H, 0, sizeof(H));
        H.status = check_item(cfg, it);
        if (H.status == ISV_KF_OK) {
            const size_t cand = it->width > 6 && it->height > 6 ? (size_t)(it->width - 6) * (it->height - 6) : 0;
            const size_t cap = cand < (size_t)cfg.max_keypoints ? cand : (size_t)cfg.max_keypoints;
            const bool out_ok = (!cap || (brief[i] && keypoints_uv[i] && keypoints_norm[i] && score[i])) && (!it->n_points || window_brief[i]);
            if (!out_ok) H.status = ISV_KF_INPUT;
            else {
                H.W = it->width; H.H = it->height; H.np = it->n_points;
                H.img_off = n_px; H.pt_off = (int32_t)n_pt; H.slot_off = (int32_t)n_slot;
                n_px += (size_t)it->width * it->height; n_pt += it->n_points; n_slot += cap;
                if (it->width > maxW) maxW = it->width;
                if (it->height > maxH) maxH = it->height;
            }
        }
        if (n_pt > INT32_MAX || n_slot > INT32_MAX) return call.fail(ISV_ERR_CAPACITY, "batch too large");
    }
    // one upload block: [headers | images, packed without their strides | window points]; then, device only: results (zeroed before
    // the launch), the blurred images, the score maps, the per-image corner lists, the compact output arrays
    BlockLayout L;
    const size_t o_hd = L.add(sizeof(KfHdr) * n), o_img = L.add(n_px + 1), o_pt = L.add(8 * (n_pt + 1));
    const size_t up_end = L.end;
    const size_t o_res = L.add(sizeof(isv_kf_result_t) * n);
    const size_t clear_end = L.end;
    const size_t o_blur = L.add(n_px + 1), o_smap = L.add(n_px + 1), o_kxy = L.add(4 * (n_slot + 1)), o_ksc = L.add(n_slot + 1);
    const size_t o_br = L.add(32 * (n_slot + 1)), o_uv = L.add(8 * (n_slot + 1)), o_nm = L.add(8 * (n_slot + 1)), o_sc = L.add(n_slot + 1);
    const size_t o_wb = L.add(32 * (n_pt + 1));
    const auto t_pack = std::chrono::steady_clock::now();
    std::vector<char> &up = h->up;
    up.resize(up_end);
    memcpy(up.data() + o_hd, hd.data(), sizeof(KfHdr) * n);
    for (int i = 0; i < n; i++) {
        const KfHdr &H = hd[i];
        if (H.status != ISV_KF_OK) continue;
        const isv_kf_item_t *it = items[i];
        char *dst = up.data() + o_img + H.img_off;
        if (it->stride == it->width) { if (H.W && H.H) memcpy(dst, it->image, (size_t)H.W * H.H); }
        else for (int y = 0; y < H.H; y++) memcpy(dst + (size_t)y * H.W, it->image + (size_t)y * it->stride, H.W);
        if (H.np) memcpy(up.data() + o_pt + 8 * (size_t)H.pt_off, it->point_2d_uv, 8 * (size_t)H.np);
    }
    const double pack_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_pack).count();
    hipStream_t stream = h->stream;
    std::vector<char> dl;
    const int rc = call.run(
        up, {{up.size(), clear_end}}, L.end,
        [&](char *d, auto &&mark) {
            const KfHdr *dh = (const KfHdr *)(d + o_hd);
            isv_kf_result_t *dr = (isv_kf_result_t *)(d + o_res);
            if (maxW > 0 && maxH > 0) {
                const dim3 grid((maxW + kTW - 1) / kTW, (maxH + kTH - 1) / kTH, n);
                hipLaunchKernelGGL(k_kf_blur, grid, dim3(kThreads), 0, stream, dh, (const uint8_t *)(d + o_img), (uint8_t *)(d + o_blur));
                mark();
                hipLaunchKernelGGL(k_kf_fast, grid, dim3(kThreads), 0, stream, dh, (const uint8_t *)(d + o_img), (uint8_t *)(d + o_smap), (int)cfg.fast_threshold);
            } else mark();
            mark();
            hipLaunchKernelGGL(k_kf_select, dim3(n), dim3(kSelThreads), sizeof(int) * (size_t)(maxH > 0 ? maxH : 1), stream, dh, (const uint8_t *)(d + o_smap),
                               (uint32_t *)(d + o_kxy), (uint8_t *)(d + o_ksc), dr, (int)cfg.max_keypoints);
            mark();
            hipLaunchKernelGGL(k_kf_brief, dim3(kBriefBlocks, n), dim3(kBriefWaves * kLanes), 0, stream, dh, dr, (const uint8_t *)(d + o_blur), h->d_pattern,
                               (const float *)(d + o_pt), (const uint32_t *)(d + o_kxy), (const uint8_t *)(d + o_ksc), h->cam, (uint64_t *)(d + o_br),
                               (float *)(d + o_uv), (float *)(d + o_nm), (uint8_t *)(d + o_sc), (uint64_t *)(d + o_wb));
        },
        {{results, o_res, sizeof(isv_kf_result_t) * n}},
        [&] {
            // the counts are known now: the download of what was written, then the scatter into the callers' arrays
            size_t n_k = 0;
            for (int i = 0; i < n; i++) {
                if (hd[i].status != ISV_KF_OK) results[i] = isv_kf_result_t{hd[i].status, 0, items[i]->n_points, 0};
                else if (results[i].status == ISV_KF_OK) n_k += results[i].n_keypoints;
            }
            const char *d = (const char *)h->slot.d;
            const size_t b_br = 0, b_uv = 32 * n_k, b_nm = b_uv + 8 * n_k, b_sc = b_nm + 8 * n_k, b_wb = (b_sc + n_k + 7) & ~(size_t)7;
            dl.resize(b_wb + 32 * n_pt + 8);
            hipError_t e = hipSuccess;
            if (n_k) {
                e = hipMemcpyAsync(dl.data() + b_br, d + o_br, 32 * n_k, hipMemcpyDeviceToHost, stream);
                if (e == hipSuccess) e = hipMemcpyAsync(dl.data() + b_uv, d + o_uv, 8 * n_k, hipMemcpyDeviceToHost, stream);
                if (e == hipSuccess) e = hipMemcpyAsync(dl.data() + b_nm, d + o_nm, 8 * n_k, hipMemcpyDeviceToHost, stream);
                if (e == hipSuccess) e = hipMemcpyAsync(dl.data() + b_sc, d + o_sc, n_k, hipMemcpyDeviceToHost, stream);
            }
            if (e == hipSuccess && n_pt) e = hipMemcpyAsync(dl.data() + b_wb, d + o_wb, 32 * n_pt, hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return e;
            size_t at = 0;
            for (int i = 0; i < n; i++) {
                if (hd[i].status != ISV_KF_OK || results[i].status != ISV_KF_OK) continue;
                const size_t nk = results[i].n_keypoints, np = hd[i].np;
                if (nk) {
                    memcpy(brief[i], dl.data() + b_br + 32 * at, 32 * nk);
                    memcpy(keypoints_uv[i], dl.data() + b_uv + 8 * at, 8 * nk);
                    memcpy(keypoints_norm[i], dl.data() + b_nm + 8 * at, 8 * nk);
                    memcpy(score[i], dl.data() + b_sc + at, nk);
                }
                if (np) memcpy(window_brief[i], dl.data() + b_wb + 32 * (size_t)hd[i].pt_off, 32 * np);
                at += nk;
            }
            return hipSuccess;
        });
    if (rc != ISV_OK) { h->last.clear(); return rc; }
    h->pack_ms = pack_ms;
    h->last.resize(n);
    for (int i = 0; i < n; i++) h->last[i] = KfLast{hd[i].status, hd[i].W, hd[i].H, hd[i].img_off};
    h->last_blur = o_blur; h->last_smap = o_smap;
    return ISV_OK;
}

extern "C" int isv_internal_kf_read_back(isv_kf_t *h, int32_t index, uint8_t *blurred, uint8_t *score_map) {
    if (!h || index < 0 || (size_t)index >= h->last.size() || h->last[index].status != ISV_KF_OK) return ISV_ERR_INVALID_ARG;
    const KfLast &it = h->last[index];
    const size_t bytes = (size_t)it.W * it.H;
    if (!bytes) return ISV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const char *d = (const char *)h->slot.d;
    if (blurred) HIPCHK(h, hipMemcpyAsync(blurred, d + h->last_blur + it.img_off, bytes, hipMemcpyDeviceToHost, h->stream));
    if (score_map) HIPCHK(h, hipMemcpyAsync(score_map, d + h->last_smap + it.img_off, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ISV_OK;
}
