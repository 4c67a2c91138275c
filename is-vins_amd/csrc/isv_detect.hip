// isv_detect.hip -- batched feature detection on the tracker's slots: FeatureTracker::setMask and cv::goodFeaturesToTrack(blockSize 3,
// Sobel 3, minimum eigenvalue) with the lift of every new corner, for many sequences in one call (include/isvins_detect.h has the
// contract, the reference lines, the restated OpenCV pieces and the deviations G1..G4; the serial CPU restatement is
// tests/native/isv_det_oracle.c).  The image is level 0 of a slot's resident pyramid (csrc/isv_tracker.h): no image moves.  One
// packed upload (the points, ordered on the host by track_cnt descending, input order among equals: G1), four kernels, one download.
// Every refusal is decided on the host before anything is launched: a refused item is not on the device at all.
//
// k_det_mask: one workgroup per item walks the ordered points.  A point whose pixel still reads 255 in the item's mask plane is kept
// and its disc is drawn by the whole workgroup from the per-|dy| half-width table (built on the host from the midpoint recurrence);
// the plane was set to 255 by a memset before the launch.  The walk is serial, as setMask is; only the drawing is parallel.
// k_det_eig: one workgroup per 32 x 16 tile.  The tile and a 2-pixel halo go into LDS, the Sobel pair of the 34 x 18 positions the
// box sums need is formed there (a position outside the image is the position its index reflects to), then the three box sums as
// exact integers and the response, written as a float32 plane.  The masked maximum is reduced per workgroup and merged per item with
// one vector atomic max on an order-preserving integer key.
// k_det_cand: threshold, 3 x 3 maximum, mask and interior test per pixel; survivors are appended (one atomic per wavefront) to the
// item's list as unique 64-bit keys (ordered float bits of v, y, x): descending keys are descending v, then descending raster index (G2).
// k_det_select: one workgroup per item.  Per accepted corner one pass over the list: every live key within min_dist of the corner
// accepted last is cleared, the largest live key is reduced over the workgroup and accepted.  That is the serial greedy order
// exactly: the next corner is the best candidate that no accepted corner suppresses.  A thread owns the keys it reads and clears:
// the first 16384 keys of the list live in registers (sixteen per thread), the rest stay in HBM (a plateau makes the list as long as
// the image), and nothing is sorted.  One barrier per pass.  The accepted corners are lifted at the end.
// Every pixel read goes through the reflection, a clamp or an explicit bounds test: no kernel reads outside a slot's level 0 or an
// item's planes.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "isv_stage_launch.h"
#include "isv_tracker.h"
#include "isv_detect.h"
#include "isv_pinhole.h"

namespace {

constexpr int kLanes = 64;
constexpr int kTW = 32, kTH = 16, kThreads = 256;             // k_det_eig's tile, the workgroup of all kernels but k_det_select
static_assert(kThreads * 2 == kTW * kTH, "k_det_eig: two pixels per thread");
constexpr int kRawW = kTW + 4, kRawH = kTH + 4, kDW = kTW + 2, kDH = kTH + 2;
constexpr int kSelThreads = 1024, kSelWaves = kSelThreads / kLanes, kSelRegs = 16;
constexpr int kCandBlocks = 4096;                             // k_det_cand: at most this many workgroups per item, each strides
constexpr int kMaxR = kDetMaxR;

}  // namespace

// BORDER_REFLECT_101, the general loop: always inside [0, len)
__device__ __forceinline__ int det_reflect(int p, int len) {
    if (len == 1) return 0;
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}
__device__ __forceinline__ int det_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// the float32 encodings in their total order, as unsigned integers; 0 encodes nothing
__device__ __forceinline__ uint32_t det_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float det_unkey(uint32_t k) {
    if (k == 0) return 0.f;
    return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k);
}

__global__ void __launch_bounds__(kThreads) k_det_mask(const DetItem *__restrict__ items, const DetPoint *__restrict__ pts, const uint8_t *__restrict__ hw_g,
                                                      char *block, DetCount *__restrict__ counts, int32_t *__restrict__ kept, int r) {
    __shared__ uint8_t hw[kMaxR + 1];
    __shared__ int s_keep;
    const DetItem &T = items[blockIdx.x];
    const int t = threadIdx.x, W = T.W, H = T.H, side = 2 * r + 1;
    uint8_t *mask = (uint8_t *)(block + T.mask_off);
    const volatile uint8_t *vmask = mask;         // thread 0's reads see the discs the workgroup drew before the barrier
    hw[t] = hw_g[t];
    int nk = 0;
    for (int p = 0; p < T.np; p++) {
        const DetPoint q = pts[(size_t)T.pt_off + p];
        __syncthreads();                          // the previous disc is drawn (and hw is filled)
        if (t == 0) s_keep = vmask[(size_t)q.y * W + q.x] != 0;
        __syncthreads();
        if (!s_keep) continue;
        for (int idx = t; idx < side * side; idx += kThreads) {
            const int dy = idx / side - r, dx = idx % side - r, x = q.x + dx, y = q.y + dy;
            if ((dx < 0 ? -dx : dx) <= hw[dy < 0 ? -dy : dy] && x >= 0 && x < W && y >= 0 && y < H) mask[(size_t)y * W + x] = 0;
        }
        if (t == 0) kept[(size_t)T.pt_off + nk] = q.idx;
        nk++;
    }
    if (t == 0) counts[blockIdx.x].n_kept = nk;
}

__global__ void __launch_bounds__(kThreads) k_det_eig(const DetItem *__restrict__ items, const uint8_t *__restrict__ store, char *__restrict__ block,
                                                     DetCount *__restrict__ counts) {
    __shared__ uint8_t raw[kRawH][kRawW];         // the image at (x0 - 2 + lx, y0 - 2 + ly), clamped into it
    __shared__ uint32_t sd[kDH][kDW];             // the Sobel pair at (x0 - 1 + lx, y0 - 1 + ly), reflected into the image: Dx low, Dy high
    __shared__ uint32_t wmax[kThreads / kLanes];
    const DetItem &T = items[blockIdx.x];
    if (T.max_new == 0) return;
    const int W = T.W, H = T.H, x0 = blockIdx.y * kTW, y0 = blockIdx.z * kTH, t = threadIdx.x;
    if (x0 >= W || y0 >= H) return;
    const uint8_t *img = store + T.img_off, *mask = (const uint8_t *)(block + T.mask_off);
    float *eig = (float *)(block + T.eig_off);
    for (int idx = t; idx < kRawH * kRawW; idx += kThreads) {
        const int ly = idx / kRawW, lx = idx % kRawW;
        raw[ly][lx] = img[(size_t)det_clamp(y0 - 2 + ly, 0, H - 1) * W + det_clamp(x0 - 2 + lx, 0, W - 1)];
    }
    __syncthreads();
    for (int idx = t; idx < kDH * kDW; idx += kThreads) {
        const int ly = idx / kDW, lx = idx % kDW, gx = x0 - 1 + lx, gy = y0 - 1 + ly;
        int dx = 0, dy = 0;
        if (gx <= W && gy <= H) {                 // beyond that no pixel of the image needs it
            // the position the index reflects to, and its neighbours: all within the image, and within 2 of the tile
            const int rx = det_reflect(gx, W), ry = det_reflect(gy, H);
            const int xm = det_clamp(det_reflect(rx - 1, W) - (x0 - 2), 0, kRawW - 1), xc = det_clamp(rx - (x0 - 2), 0, kRawW - 1),
                      xp = det_clamp(det_reflect(rx + 1, W) - (x0 - 2), 0, kRawW - 1);
            const int ym = det_clamp(det_reflect(ry - 1, H) - (y0 - 2), 0, kRawH - 1), yc = det_clamp(ry - (y0 - 2), 0, kRawH - 1),
                      yp = det_clamp(det_reflect(ry + 1, H) - (y0 - 2), 0, kRawH - 1);
            dx = (raw[ym][xp] - raw[ym][xm]) + 2 * (raw[yc][xp] - raw[yc][xm]) + (raw[yp][xp] - raw[yp][xm]);
            dy = (raw[yp][xm] - raw[ym][xm]) + 2 * (raw[yp][xc] - raw[ym][xc]) + (raw[yp][xp] - raw[ym][xp]);
        }
        sd[ly][lx] = ((uint32_t)dx & 0xffffu) | ((uint32_t)dy << 16);       // |Dx|, |Dy| <= 1020
    }
    __syncthreads();
    const float k = (float)(1.0 / (3060.0 * 3060.0));
    uint32_t best = 0;
    // a thread has two pixels, one above the other: the row sums of the four rows of products they share are formed once
    const int lx = t % kTW, ly = 2 * (t / kTW), x = x0 + lx;
    int rxx[4], rxy[4], ryy[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        rxx[j] = rxy[j] = ryy[j] = 0;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const uint32_t pk = sd[ly + j][lx + i];
            const int dx = (int16_t)(pk & 0xffffu), dy = (int)pk >> 16;
            rxx[j] += dx * dx; rxy[j] += dx * dy; ryy[j] += dy * dy;
        }
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int y = y0 + ly + q;
        if (x >= W || y >= H) continue;
        const int sxx = rxx[q] + rxx[q + 1] + rxx[q + 2], sxy = rxy[q] + rxy[q + 1] + rxy[q + 2], syy = ryy[q] + ryy[q + 1] + ryy[q + 2];
        const float a = (float)sxx * k * 0.5f, b = (float)sxy * k, c = (float)syy * k * 0.5f;
        const float e = (a + c) - (float)sqrt((double)((a - c) * (a - c) + b * b));
        const size_t p = (size_t)y * W + x;
        eig[p] = e;
        if (mask[p]) { const uint32_t ke = det_key(e); best = ke > best ? ke : best; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(best, off); best = o > best ? o : best; }
    if ((t & (kLanes - 1)) == 0) wmax[t / kLanes] = best;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kThreads / kLanes; w++) best = wmax[w] > best ? wmax[w] : best;
        if (best) atomicMax(&counts[blockIdx.x].max_key, best);
    }
}

__global__ void __launch_bounds__(kThreads) k_det_cand(const DetItem *__restrict__ items, char *__restrict__ block, DetCount *__restrict__ counts, double quality) {
    const DetItem &T = items[blockIdx.x];
    if (T.max_new == 0) return;
    const int W = T.W, H = T.H, t = threadIdx.x, lane = t & (kLanes - 1);
    const size_t npix = (size_t)W * H;
    const float *eig = (const float *)(block + T.eig_off);
    const uint8_t *mask = (const uint8_t *)(block + T.mask_off);
    unsigned long long *keys = (unsigned long long *)(block + T.key_off);
    const float thr = (float)((double)det_unkey(counts[blockIdx.x].max_key) * quality);
    for (size_t base = (size_t)blockIdx.y * kThreads; base < npix; base += (size_t)gridDim.y * kThreads) {     // uniform per workgroup
        const size_t p = base + t;
        bool cand = false;
        float v = 0.f;
        int x = 0, y = 0;
        if (p < npix) {
            x = (int)(p % W); y = (int)(p / W);
            if (x >= 1 && x < W - 1 && y >= 1 && y < H - 1) {
                const float e = eig[p];
                v = e > thr ? e : 0.f;
                if (v != 0.f && mask[p]) {
                    cand = true;
#pragma unroll
                    for (int j = -1; j <= 1; j++)
#pragma unroll
                        for (int i = -1; i <= 1; i++) {
                            const float en = eig[(size_t)(y + j) * W + (x + i)], vn = en > thr ? en : 0.f;
                            cand = cand && !(vn > v);
                        }
                }
            }
        }
        const unsigned long long ballot = __ballot(cand);
        if (ballot) {
            const int leader = __ffsll((long long)ballot) - 1;
            uint32_t at = 0;
            if (lane == leader) at = atomicAdd(&counts[blockIdx.x].n_cand, (uint32_t)__popcll(ballot));
            at = __shfl(at, leader);
            // at most (W - 2)(H - 2) candidates exist, and the list holds W H keys
            if (cand) keys[at + __popcll(ballot & ((1ull << lane) - 1))] = ((unsigned long long)det_key(v) << 32) | ((unsigned)y << 16) | (unsigned)x;
        }
    }
}

__global__ void __launch_bounds__(kSelThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) k_det_select(const DetItem *__restrict__ items, char *__restrict__ block, DetCount *__restrict__ counts,
                                                           const PinholeCam cam, float *__restrict__ new_pts, float *__restrict__ new_un, int min_dist) {
    __shared__ unsigned long long wbest[2][kSelWaves];
    const int max_new = items[blockIdx.x].max_new, out_off = items[blockIdx.x].out_off;       // read once: the loop below stores
    if (max_new == 0) return;
    const int t = threadIdx.x;
    const uint32_t n = counts[blockIdx.x].n_cand;
    unsigned long long *keys = (unsigned long long *)(block + items[blockIdx.x].key_off);
    const int md2 = min_dist * min_dist;
    // a thread owns the keys t, t + 1024, ...: the first kSelRegs of them live in registers, the rest stay in the list
    unsigned long long rk[kSelRegs];
#pragma unroll
    for (int r = 0; r < kSelRegs; r++) {
        const uint32_t i = (uint32_t)t + (uint32_t)r * kSelThreads;
        rk[r] = i < n ? keys[i] : 0;
    }
    int nacc = 0, lx = 0, ly = 0;
    while (nacc < max_new) {
        unsigned long long best = 0;
        auto near_last = [&](unsigned long long key) {
            const int dx = (int)(key & 0xffff) - lx, dy = (int)((key >> 16) & 0xffff) - ly;
            return nacc > 0 && dx * dx + dy * dy < md2;
        };
#pragma unroll
        for (int r = 0; r < kSelRegs; r++) {
            if (rk[r] && near_last(rk[r])) rk[r] = 0;
            best = rk[r] > best ? rk[r] : best;
        }
        for (uint32_t i = (uint32_t)t + (uint32_t)kSelRegs * kSelThreads; i < n; i += kSelThreads) {
            const unsigned long long key = keys[i];
            if (!key) continue;
            if (near_last(key)) { keys[i] = 0; continue; }
            best = key > best ? key : best;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(best, off); best = o > best ? o : best; }
        // the partials alternate between two rows: a row is rewritten two passes later, behind the next pass's barrier
        unsigned long long *wb = wbest[nacc & 1];
        if ((t & (kLanes - 1)) == 0) wb[t / kLanes] = best;
        __syncthreads();
        unsigned long long b = wb[0];
#pragma unroll
        for (int w = 1; w < kSelWaves; w++) b = wb[w] > b ? wb[w] : b;
        if (!b) break;                            // the list is exhausted (uniform)
        lx = (int)(b & 0xffff); ly = (int)((b >> 16) & 0xffff);
        if (t == 0) {
            const size_t o = (size_t)out_off + nacc;
            new_pts[2 * o] = (float)lx; new_pts[2 * o + 1] = (float)ly;
        }
        nacc++;
    }
    if (t == 0) counts[blockIdx.x].n_new = nacc;
    __syncthreads();                              // thread 0's new_pts are visible to the workgroup
    for (int j = t; j < nacc; j += kSelThreads) {
        const size_t o = (size_t)out_off + j;
        const volatile float *np = new_pts;
        float ux, uy;
        pinhole_lift(cam, np[2 * o], np[2 * o + 1], &ux, &uy);
        new_un[2 * o] = ux; new_un[2 * o + 1] = uy;
    }
}

namespace {

// the disc of cv::circle(thickness -1): the half-width per |dy| from the midpoint recurrence (every interval is centred)
void disc_table(int r, uint8_t hw[kMaxR + 1]) {
    memset(hw, 0, kMaxR + 1);
    int err = 0, dx = r, dy = 0, plus = 1, minus = 2 * r - 1;
    while (dx >= dy) {
        if (dx > hw[dy]) hw[dy] = (uint8_t)dx;
        if (dy > hw[dx]) hw[dx] = (uint8_t)dy;
        dy++; err += plus; plus += 2;
        if (err > 0) { err -= minus; dx--; minus -= 2; }
    }
}

}  // namespace

extern "C" const char *isv_det_last_error(const isv_det_t *h) { return h ? h->err.c_str() : "null handle"; }

extern "C" void isv_det_destroy(isv_det_t *h) {
    if (!h) return;
    (void)hipSetDevice(h->trk->device);
    stage_slot_free(h->slot);
    delete h;
}

extern "C" int isv_det_create(isv_trk_t *trk, const isv_det_config_t *c, isv_det_t **out) {
    if (!c || !out) return ISV_ERR_INVALID_ARG;
    *out = nullptr;
    if (!trk) return ISV_ERR_INVALID_ARG;
    if (c->max_items < 1 || c->max_items > 65535 || c->max_points < 1 || c->max_points > 65535 || c->max_corners < 1 || c->max_corners > 65535 ||
        c->min_dist < 1 || c->min_dist > kMaxR || !(c->quality_level > 0.0) || !(c->quality_level <= 1.0))
        return ISV_ERR_INVALID_ARG;
    isv_det *h = new isv_det();
    h->cfg = *c;
    h->trk = trk;
    disc_table(c->min_dist, h->hw);
    h->named.assign(trk->cfg.max_slots, 0);
    h->stamp.assign(trk->cfg.max_slots, 0);
    if (stage_open_failed("isv_det_create", hipSetDevice(trk->device))) {
        isv_det_destroy(h);
        return ISV_ERR_DEVICE;
    }
    *out = h;
    return ISV_OK;
}

extern "C" int isv_det_last_ms(isv_det_t *h, double out_ms[5]) {
    if (!h || !out_ms) return ISV_ERR_INVALID_ARG;
    const StageSlot &s = h->slot;      // the marks: after k_det_mask, after k_det_eig
    out_ms[0] = s.call_ms; out_ms[1] = s.part_ms[1]; out_ms[2] = s.part_ms[0]; out_ms[3] = s.part_ms[2]; out_ms[4] = s.upload_ms + s.download_ms;
    return ISV_OK;
}

void det_enqueue(isv_det *h, const DetItem *di, int m, const DetPoint *d_pts, const uint8_t *d_hw, char *d, DetCount *dc, int32_t *d_kept, float *d_new, float *d_un,
                 int any_new, int maxW, int maxH, size_t maxPix, const std::function<void()> &mark) {
    isv_trk *trk = h->trk;
    hipStream_t stream = trk->stream;
    hipLaunchKernelGGL(k_det_mask, dim3(m), dim3(kThreads), 0, stream, di, d_pts, d_hw, d, dc, d_kept, h->cfg.min_dist);
    mark();
    if (any_new) {
        const size_t cb = (maxPix + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(k_det_eig, dim3(m, (maxW + kTW - 1) / kTW, (maxH + kTH - 1) / kTH), dim3(kThreads), 0, stream, di, (const uint8_t *)trk->d_store, d, dc);
        mark();
        hipLaunchKernelGGL(k_det_cand, dim3(m, (unsigned)(cb < (size_t)kCandBlocks ? cb : (size_t)kCandBlocks)), dim3(kThreads), 0, stream, di, d, dc, h->cfg.quality_level);
        hipLaunchKernelGGL(k_det_select, dim3(m), dim3(kSelThreads), 0, stream, di, d, dc, trk->cam, d_new, d_un, h->cfg.min_dist);
    } else mark();
}

extern "C" int isv_det_detect_batch(isv_det_t *h, int32_t n, const isv_det_item_t *const *items, isv_det_result_t *results, int32_t *const *kept_index,
                                    float *const *new_pts, float *const *new_un_pts) {
    StageCall call{h ? h->ctx() : StageCtx{}, "isv_det_detect_batch"};
    call.time_download = true;
    if (const int rc = call.enter(n, items, results); rc != ISV_OK || n == 0) return rc;
    if (n > h->cfg.max_items) return call.fail(ISV_ERR_CAPACITY, "more items than max_items");
    if (!kept_index || !new_pts || !new_un_pts) return call.fail(ISV_ERR_INVALID_ARG, "null output arrays");
    const isv_det_config_t &cfg = h->cfg;
    isv_trk *trk = h->trk;
    // every refusal, on the host (tests/native/isv_det_oracle.c has the same checks in the same order, but for the slots)
    std::vector<int32_t> status(n);
    std::vector<std::vector<DetPoint>> pix(n);
    const int64_t serial = ++h->serial;
    for (int i = 0; i < n; i++) {
        const isv_det_item_t *it = items[i];
        int s = ISV_DET_OK;
        if (it->slot < 0 || it->slot >= trk->cfg.max_slots || !trk->slots[it->slot].valid || it->n_points < 0 || it->max_new < 0) s = ISV_DET_INPUT;
        else if (it->n_points > 0 && (!it->cur_pts || !it->track_cnt || !kept_index[i])) s = ISV_DET_INPUT;
        else if (it->max_new > 0 && (!new_pts[i] || !new_un_pts[i])) s = ISV_DET_INPUT;
        else if (it->n_points > cfg.max_points || it->max_new > cfg.max_corners) s = ISV_DET_CAPACITY;
        if (s == ISV_DET_OK) {
            const TrkSlot &sl = trk->slots[it->slot];
            pix[i].resize(it->n_points);
            for (int p = 0; p < it->n_points && s == ISV_DET_OK; p++) {
                const float x = it->cur_pts[2 * p], y = it->cur_pts[2 * p + 1];
                int rx, ry;
                if (!std::isfinite(x) || !std::isfinite(y) || !det_round_coord(x, &rx) || !det_round_coord(y, &ry) || rx < 0 || rx >= sl.W || ry < 0 || ry >= sl.H)
                    s = ISV_DET_INPUT;
                else pix[i][p] = DetPoint{rx, ry, p, 0};
            }
        }
        status[i] = s;
    }
    for (int i = 0; i < n; i++) {
        if (status[i] != ISV_DET_OK) continue;
        const int sl = items[i]->slot;
        if (h->stamp[sl] != serial) { h->stamp[sl] = serial; h->named[sl] = 0; }
        h->named[sl]++;
    }
    for (int i = 0; i < n; i++)                     // every item of a slot named twice, so that the order does not matter
        if (status[i] == ISV_DET_OK && h->named[items[i]->slot] > 1) status[i] = ISV_DET_INPUT;
    std::vector<DetItem> dev;
    std::vector<int> who;                          // dev[k] is items[who[k]]
    size_t n_pt = 0, n_out = 0, mask_bytes = 0, plane_bytes = 0;
    int maxW = 0, maxH = 0, any_new = 0;
    size_t maxPix = 0;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    for (int i = 0; i < n; i++) {
        if (status[i] != ISV_DET_OK) continue;
        const isv_det_item_t *it = items[i];
        const TrkSlot &sl = trk->slots[it->slot];
        const size_t px = (size_t)sl.W * sl.H;
        DetItem T;
        memset(&T, 0, sizeof(T));
        T.img_off = trk->store_off(it->slot, sl.par);
        T.W = sl.W; T.H = sl.H; T.np = it->n_points; T.pt_off = (int32_t)n_pt; T.max_new = it->max_new; T.out_off = (int32_t)n_out;
        T.mask_off = mask_bytes; mask_bytes += al(px);             // relative: the sections' starts are added below
        if (it->max_new > 0) {
            T.eig_off = plane_bytes; plane_bytes += al(4 * px);
            T.key_off = plane_bytes; plane_bytes += al(8 * px);
            any_new = 1;
            if (sl.W > maxW) maxW = sl.W;
            if (sl.H > maxH) maxH = sl.H;
            if (px > maxPix) maxPix = px;
        }
        n_pt += it->n_points; n_out += it->max_new;
        if (n_pt > INT32_MAX || n_out > INT32_MAX) return call.fail(ISV_ERR_CAPACITY, "batch too large");
        dev.push_back(T); who.push_back(i);
    }
    const int m = (int)dev.size();
    auto refuse = [&](int i) { results[i] = isv_det_result_t{status[i], items[i]->n_points, 0, 0, 0, 0.f}; };
    if (m == 0) {
        for (int i = 0; i < n; i++) refuse(i);
        h->last.assign(n, DetLast{});
        return ISV_OK;
    }
    // one block: [items | the disc table | the ordered points], uploaded; [counts], zeroed; [kept | new_pts | new_un_pts], downloaded
    // with the counts; [the mask planes], set to 255; [the response planes and the key lists]
    BlockLayout L;
    const size_t o_it = L.add(sizeof(DetItem) * m), o_hw = L.add(kMaxR + 1), o_pt = L.add(sizeof(DetPoint) * (n_pt + 1));
    const size_t up_end = L.end;
    const size_t o_cnt = L.add(sizeof(DetCount) * m);
    const size_t clear_end = L.end;
    const size_t o_kept = L.add(4 * (n_pt + 1)), o_np = L.add(8 * (n_out + 1)), o_un = L.add(8 * (n_out + 1));
    const size_t o_mask = L.add(mask_bytes), o_plane = L.add(plane_bytes + 256);
    for (DetItem &T : dev) {
        T.mask_off += o_mask;
        if (T.max_new > 0) { T.eig_off += o_plane; T.key_off += o_plane; }
    }
    std::vector<char> &up = h->up;
    up.assign(up_end, 0);
    memcpy(up.data() + o_it, dev.data(), sizeof(DetItem) * m);
    memcpy(up.data() + o_hw, h->hw, kMaxR + 1);
    for (int k = 0; k < m; k++) {
        std::vector<DetPoint> &p = pix[who[k]];
        const int32_t *cnt = items[who[k]]->track_cnt;
        std::stable_sort(p.begin(), p.end(), [cnt](const DetPoint &a, const DetPoint &b) { return cnt[a.idx] > cnt[b.idx]; });     // G1
        if (!p.empty()) memcpy(up.data() + o_pt + sizeof(DetPoint) * (size_t)dev[k].pt_off, p.data(), sizeof(DetPoint) * p.size());
    }
    std::vector<DetCount> cnt(m);
    std::vector<int32_t> dl_kept(n_pt + 1);
    std::vector<float> dl_np(2 * (n_out + 1)), dl_un(2 * (n_out + 1));
    const int rc = call.run(
        up, {{up_end, clear_end}, {o_mask, o_mask + mask_bytes, 0xff}}, L.end,
        [&](char *d, auto &&mark) {
            det_enqueue(h, (const DetItem *)(d + o_it), m, (const DetPoint *)(d + o_pt), (const uint8_t *)(d + o_hw), d, (DetCount *)(d + o_cnt), (int32_t *)(d + o_kept),
                        (float *)(d + o_np), (float *)(d + o_un), any_new, maxW, maxH, maxPix, mark);
        },
        {{cnt.data(), o_cnt, sizeof(DetCount) * m}, {n_pt ? dl_kept.data() : nullptr, o_kept, 4 * n_pt}, {n_out ? dl_np.data() : nullptr, o_np, 8 * n_out},
         {n_out ? dl_un.data() : nullptr, o_un, 8 * n_out}},
        [&] {
            h->last.assign(n, DetLast{});
            for (int i = 0; i < n; i++)
                if (status[i] != ISV_DET_OK) refuse(i);
            for (int k = 0; k < m; k++) {
                const int i = who[k];
                const DetItem &T = dev[k];
                const DetCount &c = cnt[k];
                if (c.n_kept) memcpy(kept_index[i], dl_kept.data() + T.pt_off, 4 * (size_t)c.n_kept);
                if (c.n_new) {
                    memcpy(new_pts[i], dl_np.data() + 2 * (size_t)T.out_off, 8 * (size_t)c.n_new);
                    memcpy(new_un_pts[i], dl_un.data() + 2 * (size_t)T.out_off, 8 * (size_t)c.n_new);
                }
                float mv = 0.f;
                if (c.max_key) {
                    const uint32_t u = (c.max_key >> 31) ? (c.max_key & 0x7fffffffu) : ~c.max_key;
                    memcpy(&mv, &u, 4);
                }
                results[i] = isv_det_result_t{ISV_DET_OK, T.np, c.n_kept, c.n_new, (int32_t)c.n_cand, mv};
                DetLast &l = h->last[i];
                l.W = T.W; l.H = T.H; l.valid = 1; l.has_eig = T.max_new > 0; l.n_cand = (int32_t)c.n_cand; l.mask_off = T.mask_off; l.eig_off = T.eig_off;
            }
            return hipSuccess;
        });
    if (rc != ISV_OK) h->last.clear();
    return rc;
}

extern "C" int isv_internal_det_read_plane(isv_det_t *h, int32_t item, int32_t which, void *out, int32_t *width, int32_t *height, int32_t *n_candidates) {
    if (!h || item < 0 || (size_t)item >= h->last.size() || which < 0 || which > 1 || !h->last[item].valid) return ISV_ERR_INVALID_ARG;
    const DetLast &l = h->last[item];
    if (which == 0 && !l.has_eig) return ISV_ERR_INVALID_ARG;
    if (width) *width = l.W;
    if (height) *height = l.H;
    if (n_candidates) *n_candidates = l.n_cand;
    if (!out) return ISV_OK;
    HIPCHK(h, hipSetDevice(h->trk->device));
    const size_t px = (size_t)l.W * l.H;
    HIPCHK(h, hipMemcpyAsync(out, (char *)h->slot.d + (which == 0 ? l.eig_off : l.mask_off), which == 0 ? 4 * px : px, hipMemcpyDeviceToHost, h->trk->stream));
    HIPCHK(h, hipStreamSynchronize(h->trk->stream));
    return ISV_OK;
}
