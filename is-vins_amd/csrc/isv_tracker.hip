// isv_tracker.hip -- batched feature tracking: cv::calcOpticalFlowPyrLK(21 x 21, 3 levels down), inBorder and liftProjective of every
// tracked point for many sequences in one call (include/isvins_tracker.h has the contract, the reference lines, the restated OpenCV
// pieces, the quirks T1..T4 and the deviations D1, D2; the serial CPU restatement is tests/native/isv_trk_oracle.c).
// One packed upload, the pyramid kernels, one tracking kernel, one download (isv_stage_launch.h).  Integers everywhere except the
// 2 x 2 solve of a step (float32, one fixed order) and the lift (isv_pinhole.h).
//
// A slot owns two pyramid buffers in the handle's store, allocated at creation: the resident one (the last cur image's) and the one
// the next cur image is built into; a successful item swaps them.  An uploaded prev is built over the resident one, which it
// replaces anyway.  Every refusal is decided on the host before anything is launched: a refused item is not on the device at all.
//
// The call's body is trk_track_batch: isv_trk_track_batch runs it as it is, isv_eq_track_batch (isv_equalize.hip) with the CLAHE
// kernels in place of k_trk_level0.  A slot remembers in its tag which of the two wrote its resident image.
//
// k_trk_level0: copies an uploaded image into level 0 of its pyramid buffer (16-byte words, then the tail).
// k_trk_pyrdown: one workgroup per 32 x 16 tile of level l; the 67 x 35 source pixels of level l - 1 go into LDS with
// BORDER_REFLECT_101 applied on the way in, the row pass fills a 16-bit LDS plane of 35 x 32, the column pass reads it.  One launch per
// level: level l reads all of level l - 1.
// k_trk_track: one wavefront per point through all of its levels, one workgroup per wavefront.  Per level the 24 x 24 patch of prev
// (the 22 x 22 window support and a 1-pixel halo, reflected) goes into LDS, the Scharr derivatives of the 22 x 22 support are formed
// there (zero outside the level, T4): no derivative image exists in HBM.  Lane l holds the window values 64 m + l, m = 0..6, of I,
// dIx and dIy in registers.  Per step the 22 x 22 support of cur goes into LDS; a lane's seven products go into 32-bit partials (7 x
// 8160 x 4080 < 2^31), the wavefront's sums are 64-bit butterflies (D1: exact, so every lane holds the same sums and every branch
// below is uniform).  No atomics; every global read goes through the reflection, so none leaves its level.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "isv_stage_launch.h"
#include "isv_tracker.h"
#include "isv_equalize.h"
#include "isv_pinhole.h"

namespace {

constexpr int kLanes = 64;
constexpr int kWin = ISV_TRK_WIN, kNWin = kWin * kWin, kSup = kWin + 1, kPatch = kWin + 3;   // 21, 441, 22, 24
constexpr int kPerLane = (kNWin + kLanes - 1) / kLanes;                                       // 7
constexpr int kLevels = kTrkLevels;
constexpr int kPW = 32, kPH = 16, kPThreads = 256;    // k_trk_pyrdown's output tile, its workgroup
constexpr int kSrcW = 2 * kPW + 3, kSrcH = 2 * kPH + 3;
constexpr int kCopyThreads = 256, kCopyBlocks = 32;   // k_trk_level0: blocks per image
constexpr int kMaxSide = 8192, kMaxSlots = 65536, kMaxPoints = 65535;

}  // namespace

TrkShape trk_make_shape(int W, int H) {
    TrkShape s;
    memset(&s, 0, sizeof(s));
    s.lw[0] = W; s.lh[0] = H; s.nlev = 1;
    for (int l = 0; l < ISV_TRK_MAX_LEVEL; l++) {
        const int w = (s.lw[l] + 1) / 2, h = (s.lh[l] + 1) / 2;
        if (w <= kWin || h <= kWin) break;
        s.lw[l + 1] = w; s.lh[l + 1] = h; s.lo[l + 1] = s.lo[l] + (uint32_t)s.lw[l] * (uint32_t)s.lh[l];
        s.nlev++;
    }
    return s;
}

namespace {

TrkShape make_shape(int W, int H) { return trk_make_shape(W, H); }
size_t shape_bytes(const TrkShape &s) { return (size_t)s.lo[s.nlev - 1] + (size_t)s.lw[s.nlev - 1] * s.lh[s.nlev - 1]; }

}  // namespace

// BORDER_REFLECT_101 (cv::borderInterpolate), the general loop: always inside [0, len)
__device__ __forceinline__ int trk_reflect(int p, int len) {
    if (len == 1) return 0;
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}

__global__ void __launch_bounds__(kCopyThreads) k_trk_level0(const TrkJob *__restrict__ jobs, const uint8_t *__restrict__ img, uint8_t *__restrict__ store) {
    const TrkJob &J = jobs[blockIdx.x];
    const size_t bytes = (size_t)J.s.lw[0] * J.s.lh[0], words = bytes / 16;
    const uint8_t *src = img + J.src_off;             // 16-byte aligned: the host packs it so
    uint8_t *dst = store + J.dst_off;                 // 256-byte aligned
    const size_t t = (size_t)blockIdx.y * kCopyThreads + threadIdx.x, step = (size_t)gridDim.y * kCopyThreads;
    for (size_t i = t; i < words; i += step) ((uint4 *)dst)[i] = ((const uint4 *)src)[i];
    for (size_t i = 16 * words + t; i < bytes; i += step) dst[i] = src[i];
}

__global__ void __launch_bounds__(kPThreads) k_trk_pyrdown(const TrkJob *__restrict__ jobs, uint8_t *__restrict__ store, int level) {
    constexpr int K[5] = {1, 4, 6, 4, 1};
    __shared__ uint8_t raw[kSrcH][kSrcW + 1];
    __shared__ uint16_t rowp[kSrcH][kPW];
    const TrkJob &J = jobs[blockIdx.x];
    if (level >= J.s.nlev) return;
    const int sw = J.s.lw[level - 1], sh = J.s.lh[level - 1], dw = J.s.lw[level], dh = J.s.lh[level];
    const int x0 = blockIdx.y * kPW, y0 = blockIdx.z * kPH, t = threadIdx.x;
    if (x0 >= dw || y0 >= dh) return;
    const uint8_t *src = store + J.dst_off + J.s.lo[level - 1];
    uint8_t *dst = store + J.dst_off + J.s.lo[level];
    for (int idx = t; idx < kSrcH * kSrcW; idx += kPThreads) {
        const int ly = idx / kSrcW, lx = idx % kSrcW;
        raw[ly][lx] = src[(size_t)trk_reflect(2 * y0 + ly - 2, sh) * sw + trk_reflect(2 * x0 + lx - 2, sw)];
    }
    __syncthreads();
    for (int idx = t; idx < kSrcH * kPW; idx += kPThreads) {
        const int ly = idx / kPW, lx = idx % kPW;
        int s = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) s += K[k] * raw[ly][2 * lx + k];
        rowp[ly][lx] = (uint16_t)s;               // at most 255 * 16
    }
    __syncthreads();
    for (int idx = t; idx < kPH * kPW; idx += kPThreads) {
        const int ly = idx / kPW, lx = idx % kPW, gx = x0 + lx, gy = y0 + ly;
        if (gx >= dw || gy >= dh) continue;
        int s = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) s += K[k] * rowp[2 * ly + k][lx];
        dst[(size_t)gy * dw + gx] = (uint8_t)((s + 128) >> 8);
    }
}

// floor of a float32; D2: outside int's range it does not exist
__device__ __forceinline__ bool trk_floor(float f, int *out) {
    if (!(f >= -2147483648.0f && f < 2147483648.0f)) return false;
    *out = (int)floorf(f);
    return true;
}
// cvRound of a float32, half to even; D2 as above
__device__ __forceinline__ bool trk_round(float f, int *out) {
    if (!(f >= -2147483648.0f && f < 2147483648.0f)) return false;
    *out = (int)rintf(f);
    return true;
}
// the range test on floor(x, y).  T4: the window may hang up to 21 pixels outside the level
__device__ __forceinline__ bool trk_in_range(float x, float y, int W, int H, int *ix, int *iy) {
    if (!trk_floor(x, ix) || !trk_floor(y, iy)) return false;
    return !(*ix < -kWin || *ix >= W || *iy < -kWin || *iy >= H);
}
__device__ __forceinline__ void trk_weights(float a, float b, int iw[4]) {
    iw[0] = (int)rintf((1.f - a) * (1.f - b) * 16384.f);
    iw[1] = (int)rintf(a * (1.f - b) * 16384.f);
    iw[2] = (int)rintf((1.f - a) * b * 16384.f);
    iw[3] = 16384 - iw[0] - iw[1] - iw[2];
}
__device__ __forceinline__ long long trk_wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// (float) of an integer below 2^53 in magnitude: through double, one rounding
__device__ __forceinline__ float trk_to_float(long long v) { return (float)(double)v; }

#define TRK_DESCALE(v, n) (((v) + (1 << ((n) - 1))) >> (n))

// The 22 x 22 support of `im` at (ix, iy) into LDS, then sum diff dIx, sum diff dIy, sum |diff| over the window.  Uniform.
__device__ __forceinline__ void trk_sums(const uint8_t *__restrict__ im, int W, int H, int ix, int iy, float a, float b, uint8_t *jp, const int (&I)[kPerLane],
                                         const int (&dIx)[kPerLane], const int (&dIy)[kPerLane], int lane, long long *T1, long long *T2, long long *Tabs) {
    int iw[4];
    trk_weights(a, b, iw);
    __syncthreads();                              // the previous step's reads of jp are done
    for (int idx = lane; idx < kSup * kSup; idx += kLanes) {
        const int j = idx / kSup, i = idx % kSup;
        jp[idx] = im[(size_t)trk_reflect(iy + j, H) * W + trk_reflect(ix + i, W)];
    }
    __syncthreads();
    int t1 = 0, t2 = 0, ta = 0;
#pragma unroll
    for (int m = 0; m < kPerLane; m++) {
        const int k = kLanes * m + lane;
        if (k < kNWin) {
            const int y = k / kWin, x = k % kWin;
            const uint8_t *p = jp + y * kSup + x;
            const int diff = TRK_DESCALE(p[0] * iw[0] + p[1] * iw[1] + p[kSup] * iw[2] + p[kSup + 1] * iw[3], 9) - I[m];
            t1 += diff * dIx[m]; t2 += diff * dIy[m];
            ta += diff < 0 ? -diff : diff;
        }
    }
    *T1 = trk_wave_sum(t1); *T2 = trk_wave_sum(t2); *Tabs = trk_wave_sum(ta);
}

__global__ void __launch_bounds__(kLanes) k_trk_track(const TrkItem *__restrict__ items, const float *__restrict__ pts, const uint8_t *__restrict__ store,
                                                     const PinholeCam cam, float *__restrict__ cur_pts, float *__restrict__ cur_un, float *__restrict__ err,
                                                     uint8_t *__restrict__ flags) {
    __shared__ uint8_t patch[kPatch * kPatch];    // prev at (ip - 1 + i, ip - 1 + j), reflected
    __shared__ int16_t sIx[kSup * kSup], sIy[kSup * kSup];
    __shared__ uint8_t jp[kSup * kSup];
    const TrkItem &T = items[blockIdx.y];
    const int pi = blockIdx.x, lane = threadIdx.x;
    if (pi >= T.np) return;
    const size_t o = (size_t)T.pt_off + pi;
    const float ptx = pts[2 * o], pty = pts[2 * o + 1];
    const int nlev = T.s.nlev;
    int st = 1;
    float e = 0.f, qox = 0.f, qoy = 0.f;
    int I[kPerLane], dIx[kPerLane], dIy[kPerLane];
    for (int l = nlev - 1; l >= 0; l--) {
        const int W = T.s.lw[l], H = T.s.lh[l];
        const uint8_t *P = store + T.prev_off + T.s.lo[l], *J = store + T.cur_off + T.s.lo[l];
        const float scale = 1.f / (float)(1 << l);
        float px = ptx * scale, py = pty * scale, qx, qy;
        if (l == nlev - 1) { qx = px; qy = py; }
        else { qx = qox * 2.f; qy = qoy * 2.f; }
        qox = qx; qoy = qy;
        px -= 10.f; py -= 10.f;
        int ipx, ipy;
        if (!trk_in_range(px, py, W, H, &ipx, &ipy)) {         // T1: a failure only at level 0
            if (l == 0) st = 0;
            continue;
        }
        __syncthreads();                          // the previous level's reads of the LDS planes are done
        for (int idx = lane; idx < kPatch * kPatch; idx += kLanes) {
            const int j = idx / kPatch, i = idx % kPatch;
            patch[idx] = P[(size_t)trk_reflect(ipy - 1 + j, H) * W + trk_reflect(ipx - 1 + i, W)];
        }
        __syncthreads();
        for (int idx = lane; idx < kSup * kSup; idx += kLanes) {
            const int j = idx / kSup, i = idx % kSup, gx = ipx + i, gy = ipy + j;
            int ix = 0, iy = 0;                   // T4: zero outside the level
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const uint8_t *r0 = patch + j * kPatch + i, *r1 = r0 + kPatch, *r2 = r1 + kPatch;
                const int t0a = 3 * (r0[0] + r2[0]) + 10 * r1[0], t0c = 3 * (r0[2] + r2[2]) + 10 * r1[2];
                const int t1a = r2[0] - r0[0], t1b = r2[1] - r0[1], t1c = r2[2] - r0[2];
                ix = t0c - t0a;
                iy = 3 * (t1a + t1c) + 10 * t1b;
            }
            sIx[idx] = (int16_t)ix; sIy[idx] = (int16_t)iy;
        }
        __syncthreads();
        int iw[4];
        trk_weights(px - (float)ipx, py - (float)ipy, iw);
        int s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
        for (int m = 0; m < kPerLane; m++) {
            const int k = kLanes * m + lane;
            I[m] = dIx[m] = dIy[m] = 0;
            if (k < kNWin) {
                const int y = k / kWin, x = k % kWin;
                const uint8_t *p = patch + (y + 1) * kPatch + x + 1;
                const int16_t *gxp = sIx + y * kSup + x, *gyp = sIy + y * kSup + x;
                I[m] = TRK_DESCALE(p[0] * iw[0] + p[1] * iw[1] + p[kPatch] * iw[2] + p[kPatch + 1] * iw[3], 9);
                dIx[m] = TRK_DESCALE(gxp[0] * iw[0] + gxp[1] * iw[1] + gxp[kSup] * iw[2] + gxp[kSup + 1] * iw[3], 14);
                dIy[m] = TRK_DESCALE(gyp[0] * iw[0] + gyp[1] * iw[1] + gyp[kSup] * iw[2] + gyp[kSup + 1] * iw[3], 14);
                s11 += dIx[m] * dIx[m]; s12 += dIx[m] * dIy[m]; s22 += dIy[m] * dIy[m];
            }
        }
        const float FLT_SCALE = 1.f / (float)(1 << 20);
        const float A11 = trk_to_float(trk_wave_sum(s11)) * FLT_SCALE, A12 = trk_to_float(trk_wave_sum(s12)) * FLT_SCALE,
                    A22 = trk_to_float(trk_wave_sum(s22)) * FLT_SCALE;
        const float D = A11 * A22 - A12 * A12;
        // sqrt and the divisions through double: correctly rounded float32 results whatever the compiler's float32 division mode
        const float root = (float)sqrt((double)((A11 - A22) * (A11 - A22) + 4.f * A12 * A12));
        const float minEig = (float)((double)(A22 + A11 - root) / 882.0);
        if ((double)minEig < 1e-4 || D < FLT_EPSILON) {
            if (l == 0) st = 0;
            continue;
        }
        const float Dinv = (float)(1.0 / (double)D);
        qx -= 10.f; qy -= 10.f;
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < ISV_TRK_MAX_ITER; j++) {
            int iqx, iqy;
            if (!trk_in_range(qx, qy, W, H, &iqx, &iqy)) {
                if (l == 0) st = 0;
                break;
            }
            long long T1, T2, Tabs;
            trk_sums(J, W, H, iqx, iqy, qx - (float)iqx, qy - (float)iqy, jp, I, dIx, dIy, lane, &T1, &T2, &Tabs);
            const float b1 = trk_to_float(T1) * FLT_SCALE, b2 = trk_to_float(T2) * FLT_SCALE;
            const float dx = (A12 * b2 - A22 * b1) * Dinv, dy = (A12 * b1 - A11 * b2) * Dinv;
            qx += dx; qy += dy;
            qox = qx + 10.f; qoy = qy + 10.f;
            if ((double)dx * (double)dx + (double)dy * (double)dy <= 0.01 * 0.01) break;
            if (j > 0 && (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + pdy) < 0.01) {       // T3
                qox -= dx * 0.5f; qoy -= dy * 0.5f;
                break;
            }
            pdx = dx; pdy = dy;
        }
        if (l == 0 && st) {
            int iqx, iqy;
            const float nx = qox - 10.f, ny = qoy - 10.f;
            if (!trk_in_range(nx, ny, W, H, &iqx, &iqy)) st = 0;                                   // T2
            else {
                long long T1, T2, Tabs;
                trk_sums(J, W, H, iqx, iqy, nx - (float)iqx, ny - (float)iqy, jp, I, dIx, dIy, lane, &T1, &T2, &Tabs);
                e = (float)((double)trk_to_float(Tabs) / 14112.0);
            }
        }
    }
    if (lane == 0) {
        int rx, ry;
        const bool inb = trk_round(qox, &rx) && trk_round(qoy, &ry) && 1 <= rx && rx < T.s.lw[0] - 1 && 1 <= ry && ry < T.s.lh[0] - 1;
        float ux = 0.f, uy = 0.f;
        if (st) pinhole_lift(cam, qox, qoy, &ux, &uy);
        cur_pts[2 * o] = qox; cur_pts[2 * o + 1] = qoy;
        cur_un[2 * o] = ux; cur_un[2 * o + 1] = uy;
        err[o] = st ? e : 0.f;
        flags[o] = (uint8_t)((st ? ISV_TRK_FLAG_STATUS : 0) | (inb ? ISV_TRK_FLAG_BORDER : 0));
    }
}

namespace {

// the checks that do not involve a slot's state (tests/native/isv_trk_oracle.c has the same)
int check_item(const isv_trk_config_t &c, const isv_trk_item_t *it) {
    if (it->width < 1 || it->height < 1 || it->n_points < 0 || it->stride < it->width) return ISV_TRK_INPUT;
    if (it->slot < 0 || it->slot >= c.max_slots || !it->cur) return ISV_TRK_INPUT;
    if (it->n_points > 0 && !it->prev_pts) return ISV_TRK_INPUT;
    if (it->width > c.max_width || it->height > c.max_height || it->n_points > c.max_points) return ISV_TRK_CAPACITY;
    for (size_t k = 0; k < 2 * (size_t)it->n_points; k++)
        if (!std::isfinite(it->prev_pts[k])) return ISV_TRK_INPUT;
    return ISV_TRK_OK;
}

void pack_image(char *dst, const uint8_t *src, int W, int H, int stride) {
    if (stride == W) memcpy(dst, src, (size_t)W * H);
    else for (int y = 0; y < H; y++) memcpy(dst + (size_t)y * W, src + (size_t)y * stride, W);
}

}  // namespace

extern "C" const char *isv_trk_last_error(const isv_trk_t *h) { return h ? h->err.c_str() : "null handle"; }

extern "C" void isv_trk_destroy(isv_trk_t *h) {
    if (!h) return;
    h->close();
    if (h->d_store) (void)hipFree(h->d_store);
    delete h;
}

extern "C" int isv_trk_create(const isv_trk_config_t *c, isv_trk_t **out) {
    if (!c || !out) return ISV_ERR_INVALID_ARG;
    *out = nullptr;
    if (c->max_slots < 1 || c->max_slots > kMaxSlots || c->max_items < 1 || c->max_items > 65535 || c->max_width < 1 || c->max_width > kMaxSide ||
        c->max_height < 1 || c->max_height > kMaxSide || c->max_points < 1 || c->max_points > kMaxPoints)
        return ISV_ERR_INVALID_ARG;
    if (c->win != ISV_TRK_WIN || c->max_level != ISV_TRK_MAX_LEVEL) return ISV_ERR_INVALID_ARG;
    for (const double v : {c->fx, c->fy, c->cx, c->cy, c->k1, c->k2, c->p1, c->p2})
        if (!std::isfinite(v)) return ISV_ERR_INVALID_ARG;
    if (!(c->fx > 0) || !(c->fy > 0)) return ISV_ERR_INVALID_ARG;
    isv_trk *h = new isv_trk();
    h->cfg = *c;
    h->cam = pinhole_make(c->fx, c->fy, c->cx, c->cy, c->k1, c->k2, c->p1, c->p2);
    h->slot_bytes = (shape_bytes(make_shape(c->max_width, c->max_height)) + 255) & ~(size_t)255;
    h->slots.resize(c->max_slots);
    h->named.assign(c->max_slots, 0);
    h->stamp.assign(c->max_slots, 0);
    h->gen.assign(c->max_slots, 0);
    hipError_t e = h->open();
    if (e == hipSuccess) e = hipMalloc(&h->d_store, h->slot_bytes * 2 * (size_t)c->max_slots);
    if (stage_open_failed("isv_trk_create", e)) {
        isv_trk_destroy(h);
        return ISV_ERR_DEVICE;
    }
    *out = h;
    return ISV_OK;
}

extern "C" int isv_trk_last_ms(isv_trk_t *h, double out_ms[5]) {
    if (!h || !out_ms) return ISV_ERR_INVALID_ARG;
    out_ms[0] = h->slot.call_ms; out_ms[1] = h->slot.part_ms[0]; out_ms[2] = h->slot.part_ms[1];
    out_ms[3] = h->slot.upload_ms; out_ms[4] = h->pack_ms;
    return ISV_OK;
}

extern "C" int isv_trk_slot_reset(isv_trk_t *h, int32_t slot) {
    if (!h || slot < 0 || slot >= h->cfg.max_slots) return ISV_ERR_INVALID_ARG;
    h->slots[slot] = TrkSlot{};
    h->gen[slot]++;
    return ISV_OK;
}

extern "C" int isv_trk_track_batch(isv_trk_t *h, int32_t n, const isv_trk_item_t *const *items, isv_trk_result_t *results, float *const *cur_pts,
                                   uint8_t *const *flags, float *const *err, float *const *cur_un_pts) {
    return trk_track_batch(h, nullptr, "isv_trk_track_batch", n, items, results, cur_pts, flags, err, cur_un_pts);
}

void trk_enqueue_pyramids(isv_trk *h, isv_eq *eq, const TrkJob *dj, int nj, const uint8_t *d_img, uint8_t *d_lut, int maxLev, const int *maxLW, const int *maxLH,
                          const std::function<void()> &mark) {
    hipStream_t stream = h->stream;
    if (eq) {
        eq_launch(*eq, stream, dj, nj, d_img, h->d_store, d_lut, maxLW[0], maxLH[0]);
        mark();
    } else
        hipLaunchKernelGGL(k_trk_level0, dim3(nj, kCopyBlocks), dim3(kCopyThreads), 0, stream, dj, d_img, h->d_store);
    for (int l = 1; l < maxLev; l++)
        hipLaunchKernelGGL(k_trk_pyrdown, dim3(nj, (maxLW[l] + kPW - 1) / kPW, (maxLH[l] + kPH - 1) / kPH), dim3(kPThreads), 0, stream, dj, h->d_store, l);
}

void trk_enqueue_track(isv_trk *h, const TrkItem *d_items, int m, int max_np, const float *d_pts, float *d_cur, float *d_un, float *d_err, uint8_t *d_flags) {
    if (max_np > 0)
        hipLaunchKernelGGL(k_trk_track, dim3(max_np, m), dim3(kLanes), 0, h->stream, d_items, d_pts, (const uint8_t *)h->d_store, h->cam, d_cur, d_un, d_err, d_flags);
}

int trk_track_batch(isv_trk *h, isv_eq *eq, const char *entry, int32_t n, const isv_trk_item_t *const *items, isv_trk_result_t *results,
                    float *const *cur_pts, uint8_t *const *flags, float *const *err, float *const *cur_un_pts) {
    StageCall call{eq ? eq->ctx() : h ? h->ctx() : StageCtx{}, entry};
    const int32_t tag = eq ? eq->id : 0;           // what the call writes into a slot, and what a resident prev has to be
    if (const int rc = call.enter(n, items, results); rc != ISV_OK || n == 0) return rc;
    if (n > h->cfg.max_items) return call.fail(ISV_ERR_CAPACITY, "more items than max_items");
    if (!cur_pts || !flags || !err || !cur_un_pts) return call.fail(ISV_ERR_INVALID_ARG, "null output arrays");
    const isv_trk_config_t &cfg = h->cfg;
    // every refusal, on the host: the item's own checks, its slot's state, then the slots named twice among the items still good
    std::vector<int32_t> status(n);
    const int64_t serial = ++h->serial;
    for (int i = 0; i < n; i++) {
        const isv_trk_item_t *it = items[i];
        int s = check_item(cfg, it);
        if (s == ISV_TRK_OK && it->n_points > 0 && (!cur_pts[i] || !flags[i] || !err[i] || !cur_un_pts[i])) s = ISV_TRK_INPUT;
        if (s == ISV_TRK_OK && !it->prev) {
            const TrkSlot &sl = h->slots[it->slot];
            if (!sl.valid || sl.W != it->width || sl.H != it->height || sl.tag != tag) s = ISV_TRK_INPUT;
        }
        status[i] = s;
    }
    for (int i = 0; i < n; i++) {
        if (status[i] != ISV_TRK_OK) continue;
        const int sl = items[i]->slot;
        if (h->stamp[sl] != serial) { h->stamp[sl] = serial; h->named[sl] = 0; }
        h->named[sl]++;
    }
    for (int i = 0; i < n; i++)                     // every item of a slot named twice, so that the order does not matter
        if (status[i] == ISV_TRK_OK && h->named[items[i]->slot] > 1) status[i] = ISV_TRK_INPUT;
    std::vector<TrkItem> dev;
    std::vector<TrkJob> jobs;
    std::vector<int> who, cur_job;                 // dev[k] is items[who[k]]; its cur image is jobs[cur_job[k]]
    size_t n_pt = 0, n_img = 0;
    int maxNp = 0, maxLev = 1, maxLW[kLevels] = {}, maxLH[kLevels] = {};
    for (int i = 0; i < n; i++) {
        if (status[i] != ISV_TRK_OK) continue;
        const isv_trk_item_t *it = items[i];
        const TrkSlot &sl = h->slots[it->slot];
        const int par = sl.valid ? sl.par : 0;
        TrkItem T;
        memset(&T, 0, sizeof(T));
        T.s = make_shape(it->width, it->height);
        T.prev_off = h->store_off(it->slot, par); T.cur_off = h->store_off(it->slot, par ^ 1);
        T.np = it->n_points; T.pt_off = (int32_t)n_pt;
        n_pt += it->n_points;
        if (n_pt > INT32_MAX) return call.fail(ISV_ERR_CAPACITY, "batch too large");
        const size_t px = ((size_t)it->width * it->height + 15) & ~(size_t)15;
        if (it->prev) { jobs.push_back(TrkJob{n_img, T.prev_off, T.s}); n_img += px; }
        cur_job.push_back((int)jobs.size());
        jobs.push_back(TrkJob{n_img, T.cur_off, T.s}); n_img += px;
        dev.push_back(T); who.push_back(i);
        if (T.np > maxNp) maxNp = T.np;
        if (T.s.nlev > maxLev) maxLev = T.s.nlev;
        for (int l = 0; l < T.s.nlev; l++) {
            if (T.s.lw[l] > maxLW[l]) maxLW[l] = T.s.lw[l];
            if (T.s.lh[l] > maxLH[l]) maxLH[l] = T.s.lh[l];
        }
    }
    const int m = (int)dev.size(), nj = (int)jobs.size();
    auto refuse = [&](int i) { results[i] = isv_trk_result_t{status[i], items[i]->n_points, 0, 0}; };
    if (m == 0) {
        for (int i = 0; i < n; i++) refuse(i);
        if (eq) eq->last.assign(n, EqLast{});
        return ISV_OK;
    }
    // one upload block: [items | jobs | points | images, packed without their strides, each 16-byte aligned]; then, device only: a
    // zeroed guard, cur_pts, cur_un_pts, err, flags of all points; with an equaliser, the LUTs of every job's tiles
    BlockLayout L;
    const size_t o_it = L.add(sizeof(TrkItem) * m), o_job = L.add(sizeof(TrkJob) * nj), o_pt = L.add(8 * (n_pt + 1)), o_img = L.add(n_img + 16);
    const size_t up_end = L.end;
    (void)L.add(16);
    const size_t clear_end = L.end;
    const size_t o_cp = L.add(8 * (n_pt + 1)), o_un = L.add(8 * (n_pt + 1)), o_er = L.add(4 * (n_pt + 1)), o_fl = L.add(n_pt + 1);
    const size_t o_lut = eq ? L.add(eq->lut_bytes() * nj) : 0;
    const auto t_pack = std::chrono::steady_clock::now();
    std::vector<char> &up = h->up;
    up.resize(up_end);
    memcpy(up.data() + o_it, dev.data(), sizeof(TrkItem) * m);
    memcpy(up.data() + o_job, jobs.data(), sizeof(TrkJob) * nj);
    for (int k = 0, j = 0; k < m; k++) {
        const isv_trk_item_t *it = items[who[k]];
        if (it->n_points) memcpy(up.data() + o_pt + 8 * (size_t)dev[k].pt_off, it->prev_pts, 8 * (size_t)it->n_points);
        if (it->prev) pack_image(up.data() + o_img + jobs[j++].src_off, it->prev, it->width, it->height, it->stride);
        pack_image(up.data() + o_img + jobs[j++].src_off, it->cur, it->width, it->height, it->stride);
    }
    const double pack_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_pack).count();
    std::vector<char> dl(21 * n_pt + 32);
    const size_t b_cp = 0, b_un = 8 * n_pt, b_er = 16 * n_pt, b_fl = 20 * n_pt;
    const int rc = call.run(
        up, {{up.size(), clear_end}}, L.end,
        [&](char *d, auto &&mark) {
            trk_enqueue_pyramids(h, eq, (const TrkJob *)(d + o_job), nj, (const uint8_t *)(d + o_img), eq ? (uint8_t *)(d + o_lut) : nullptr, maxLev, maxLW, maxLH, mark);
            mark();
            trk_enqueue_track(h, (const TrkItem *)(d + o_it), m, maxNp, (const float *)(d + o_pt), (float *)(d + o_cp), (float *)(d + o_un), (float *)(d + o_er),
                              (uint8_t *)(d + o_fl));
        },
        {{n_pt ? dl.data() + b_cp : nullptr, o_cp, 8 * n_pt}, {n_pt ? dl.data() + b_un : nullptr, o_un, 8 * n_pt}, {n_pt ? dl.data() + b_er : nullptr, o_er, 4 * n_pt},
         {n_pt ? dl.data() + b_fl : nullptr, o_fl, n_pt}},
        [&] {
            for (int i = 0; i < n; i++)
                if (status[i] != ISV_TRK_OK) refuse(i);
            for (int k = 0; k < m; k++) {
                const int i = who[k];
                const size_t np = dev[k].np, at = dev[k].pt_off;
                int kept = 0;
                if (np) {
                    memcpy(cur_pts[i], dl.data() + b_cp + 8 * at, 8 * np);
                    memcpy(cur_un_pts[i], dl.data() + b_un + 8 * at, 8 * np);
                    memcpy(err[i], dl.data() + b_er + 4 * at, 4 * np);
                    memcpy(flags[i], dl.data() + b_fl + at, np);
                    for (size_t p = 0; p < np; p++) kept += flags[i][p] == (ISV_TRK_FLAG_STATUS | ISV_TRK_FLAG_BORDER);
                }
                results[i] = isv_trk_result_t{ISV_TRK_OK, (int32_t)np, kept, dev[k].s.nlev};
                h->slots[items[i]->slot] = TrkSlot{items[i]->width, items[i]->height, (int32_t)((dev[k].cur_off - h->store_off(items[i]->slot, 0)) / h->slot_bytes), 1, tag};
                h->gen[items[i]->slot]++;
            }
            if (eq) {
                eq->last.assign(n, EqLast{});
                for (int k = 0; k < m; k++) {
                    EqLast &l = eq->last[who[k]];
                    l.lut_off[0] = (int64_t)(o_lut + eq->lut_bytes() * cur_job[k]);
                    if (items[who[k]]->prev) l.lut_off[1] = (int64_t)(o_lut + eq->lut_bytes() * (cur_job[k] - 1));
                }
            }
            return hipSuccess;
        });
    if (rc != ISV_OK) {                            // what the kernels left in the buffers is unknown
        for (int k = 0; k < m; k++) { h->slots[items[who[k]]->slot] = TrkSlot{}; h->gen[items[who[k]]->slot]++; }
        if (eq) eq->last.clear();
        return rc;
    }
    (eq ? eq->pack_ms : h->pack_ms) = pack_ms;
    return ISV_OK;
}

extern "C" int isv_internal_trk_read_level(isv_trk_t *h, int32_t slot, int32_t which, int32_t level, uint8_t *out, int32_t *width, int32_t *height) {
    if (!h || slot < 0 || slot >= h->cfg.max_slots || which < 0 || which > 1 || level < 0 || !h->slots[slot].valid) return ISV_ERR_INVALID_ARG;
    const TrkSlot &sl = h->slots[slot];
    const TrkShape s = make_shape(sl.W, sl.H);
    if (level >= s.nlev) return ISV_ERR_INVALID_ARG;
    if (width) *width = s.lw[level];
    if (height) *height = s.lh[level];
    if (!out) return ISV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(out, h->d_store + h->store_off(slot, sl.par ^ which) + s.lo[level], (size_t)s.lw[level] * s.lh[level], hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ISV_OK;
}
