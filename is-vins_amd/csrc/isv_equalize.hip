// isv_equalize.hip -- batched CLAHE: cv::createCLAHE(clip_limit, Size(tiles_x, tiles_y))->apply on 8-bit images for many sequences in
// one call (include/isvins_equalize.h has the contract, the reference lines, the restated OpenCV arithmetic, the quirk K1, the
// version-dependent rules E1, E2 and the deviation E3; the serial CPU restatement is tests/native/isv_eq_oracle.c).  An equaliser is
// bound to a tracker handle: isv_eq_track_batch is the tracker's call (trk_track_batch, isv_tracker.hip) with the two kernels below in
// place of its level-0 copy, isv_eq_apply_batch runs them from an upload block into an output block.  Integers everywhere except
// lutScale and the bilinear blend (float32, one fixed order).
//
// k_eq_lut: one workgroup per (job, tile).  The tile's histogram goes into one LDS sub-histogram per wavefront with LDS atomics
// (integer counts: any order; a constant image sends every lane of a wavefront to one counter, which the atomics serialise); a pixel
// of the extension (K1) is read through the reflect-101 index, no extended image exists.  Thread t then owns bin t: the clip, the
// workgroup's sum of the excess, the redistribution (E1), a 256-entry scan, the LUT entry.
// k_eq_interp: one workgroup per (job, band of 16 rows), a thread per pixel of a row: four LUT entries and the float32 blend (E2).  The
// two tile rows of LUTs that the workgroup's current image row reads are staged in LDS (at most 16 KB; restaged when the row's pair
// changes, once or twice per band); reading them through L1 from the image's table instead was measured and is slower (DESIGN
// section 19).  Every read is bounded by the reflection or a clamp, every write lies inside [0, W H) of its destination, LUT and
// histogram indices come from a uint8_t.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <chrono>
#include <vector>
#include "isv_stage_launch.h"
#include "isv_equalize.h"

namespace {

constexpr int kLanes = 64, kEqThreads = 256, kEqWaves = kEqThreads / kLanes;
constexpr int kEqRows = 16;                            // k_eq_interp: image rows per workgroup
constexpr int kEqBins = 256;

struct EqParams { double clip_limit; int32_t tiles_x, tiles_y; };
struct EqGrid { int tw, th, clip; float lut_scale; };

}  // namespace

// BORDER_REFLECT_101 (cv::borderInterpolate), the general loop: always inside [0, len)
__device__ __forceinline__ int eq_reflect(int p, int len) {
    if (len == 1) return 0;
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}
// cvRound, half to even, saturated to 8 bits
__device__ __forceinline__ uint8_t eq_sat_u8(float f) {
    const int r = (int)rintf(f);
    return (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
}
// the tile grid of a W x H image.  The divisions go through double: correctly rounded float32 results whatever the compiler's
// float32 division mode
__device__ __forceinline__ EqGrid eq_grid(int W, int H, const EqParams &P) {
    int ew = W, eh = H;
    if (W % P.tiles_x != 0 || H % P.tiles_y != 0) {    // K1: both axes, also the one that divides
        ew = W + P.tiles_x - W % P.tiles_x;
        eh = H + P.tiles_y - H % P.tiles_y;
    }
    EqGrid g;
    g.tw = ew / P.tiles_x; g.th = eh / P.tiles_y;
    const int area = g.tw * g.th;
    g.clip = 0;
    if (P.clip_limit > 0.0) {
        const double v = P.clip_limit * (double)area / 256.0;
        g.clip = (int)(v < (double)area ? v : (double)area);       // E3
        if (g.clip < 1) g.clip = 1;
    }
    g.lut_scale = (float)(255.0 / (double)(float)area);
    return g;
}

__global__ void __launch_bounds__(kEqThreads) k_eq_lut(const TrkJob *__restrict__ jobs, const uint8_t *__restrict__ img, uint8_t *__restrict__ lut, const EqParams P) {
    __shared__ unsigned int hist[kEqWaves][kEqBins];
    __shared__ int wsum[kEqWaves];
    const TrkJob &J = jobs[blockIdx.x];
    const int W = J.s.lw[0], H = J.s.lh[0], t = threadIdx.x, wave = t / kLanes, lane = t % kLanes;
    const EqGrid g = eq_grid(W, H, P);
    const int tile = blockIdx.y, x0 = (tile % P.tiles_x) * g.tw, y0 = (tile / P.tiles_x) * g.th;
    const uint8_t *src = img + J.src_off;
    for (int i = t; i < kEqWaves * kEqBins; i += kEqThreads) (&hist[0][0])[i] = 0;
    __syncthreads();
    // a wavefront per row, a lane per column: the tile's pixels, those of the extension through the reflection
    for (int r = wave; r < g.th; r += kEqWaves) {
        const uint8_t *row = src + (size_t)eq_reflect(y0 + r, H) * W;
        for (int c = lane; c < g.tw; c += kLanes) atomicAdd(&hist[wave][row[eq_reflect(x0 + c, W)]], 1u);
    }
    __syncthreads();
    // thread t owns bin t
    int h = 0;
#pragma unroll
    for (int w = 0; w < kEqWaves; w++) h += (int)hist[w][t];
    int excess = 0;
    if (g.clip > 0 && h > g.clip) { excess = h - g.clip; h = g.clip; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) excess += __shfl_xor(excess, off);
    if (lane == 0) wsum[wave] = excess;
    __syncthreads();
    int clipped = 0;
#pragma unroll
    for (int w = 0; w < kEqWaves; w++) clipped += wsum[w];
    if (g.clip > 0) {
        const int batch = clipped / kEqBins, residual = clipped - batch * kEqBins;
        h += batch;
        if (residual != 0) {                           // E1: bins 0, step, 2 step, ..., residual of them
            const int step = kEqBins / residual > 1 ? kEqBins / residual : 1;
            if (t % step == 0 && t / step < residual) h++;
        }
    }
    int s = h;                                         // the inclusive scan: within the wavefront, then over the wavefronts' totals
#pragma unroll
    for (int off = 1; off < kLanes; off <<= 1) {
        const int up = __shfl_up(s, off);
        if (lane >= off) s += up;
    }
    __syncthreads();                                   // wsum's reads above are done
    if (lane == kLanes - 1) wsum[wave] = s;
    __syncthreads();
    for (int w = 0; w < wave; w++) s += wsum[w];
    lut[((size_t)blockIdx.x * (P.tiles_x * P.tiles_y) + tile) * kEqBins + t] = eq_sat_u8((float)s * g.lut_scale);
}

// a tile axis at pixel p: the two tile indices, clamped into the grid, and the weight of the second
__device__ __forceinline__ void eq_axis(int p, float inv_t, int tiles, int *t1, int *t2, float *a) {
    const float f = (float)p * inv_t - 0.5f;           // E2
    const int i1 = (int)floorf(f);
    *a = f - (float)i1;
    *t1 = i1 < 0 ? 0 : (i1 > tiles - 1 ? tiles - 1 : i1);          // (the upper bound is never reached: p < tiles * t; it bounds the index)
    *t2 = i1 + 1 > tiles - 1 ? tiles - 1 : i1 + 1;
}

__global__ void __launch_bounds__(kEqThreads) k_eq_interp(const TrkJob *__restrict__ jobs, const uint8_t *__restrict__ img, const uint8_t *__restrict__ lut,
                                                         uint8_t *__restrict__ dst_base, const EqParams P) {
    __shared__ uint32_t staged[2 * ISV_EQ_MAX_TILES * kEqBins / 4];
    const TrkJob &J = jobs[blockIdx.x];
    const int W = J.s.lw[0], H = J.s.lh[0], t = threadIdx.x;
    const int y0 = blockIdx.y * kEqRows, y1 = y0 + kEqRows < H ? y0 + kEqRows : H;
    if (y0 >= H) return;
    const EqGrid g = eq_grid(W, H, P);
    const float inv_tw = (float)(1.0 / (double)g.tw), inv_th = (float)(1.0 / (double)g.th);
    const uint8_t *src = img + J.src_off;
    const uint8_t *L = lut + (size_t)blockIdx.x * (P.tiles_x * P.tiles_y) * kEqBins;
    uint8_t *dst = dst_base + J.dst_off;
    const int row_bytes = P.tiles_x * kEqBins;
    int s1 = -1, s2 = -1;                              // the tile rows in `staged`
    for (int y = y0; y < y1; y++) {                    // uniform over the workgroup
        int ty1, ty2;
        float ya;
        eq_axis(y, inv_th, P.tiles_y, &ty1, &ty2, &ya);
        const float ya1 = 1.0f - ya;
        if (ty1 != s1 || ty2 != s2) {
            const uint32_t *g1 = (const uint32_t *)(L + (size_t)ty1 * row_bytes), *g2 = (const uint32_t *)(L + (size_t)ty2 * row_bytes);
            __syncthreads();                           // the previous rows' reads of `staged` are done
            for (int i = t; i < row_bytes / 4; i += kEqThreads) {
                staged[i] = g1[i];
                staged[row_bytes / 4 + i] = g2[i];
            }
            __syncthreads();
            s1 = ty1; s2 = ty2;
        }
        const uint8_t *r1 = (const uint8_t *)staged, *r2 = r1 + row_bytes;
        for (int x = t; x < W; x += kEqThreads) {
            int tx1, tx2;
            float xa;
            eq_axis(x, inv_tw, P.tiles_x, &tx1, &tx2, &xa);
            const float xa1 = 1.0f - xa;
            const int v = src[(size_t)y * W + x];
            const float res = ((float)r1[tx1 * kEqBins + v] * xa1 + (float)r1[tx2 * kEqBins + v] * xa) * ya1 +
                              ((float)r2[tx1 * kEqBins + v] * xa1 + (float)r2[tx2 * kEqBins + v] * xa) * ya;
            dst[(size_t)y * W + x] = eq_sat_u8(res);
        }
    }
}

void eq_launch(const isv_eq &e, hipStream_t stream, const TrkJob *jobs, int nj, const uint8_t *img, uint8_t *dst, uint8_t *lut, int maxW, int maxH) {
    const EqParams P{e.cfg.clip_limit, e.cfg.tiles_x, e.cfg.tiles_y};
    (void)maxW;
    hipLaunchKernelGGL(k_eq_lut, dim3(nj, e.cfg.tiles_x * e.cfg.tiles_y), dim3(kEqThreads), 0, stream, jobs, img, lut, P);
    hipLaunchKernelGGL(k_eq_interp, dim3(nj, (maxH + kEqRows - 1) / kEqRows), dim3(kEqThreads), 0, stream, jobs, img, (const uint8_t *)lut, dst, P);
}

extern "C" const char *isv_eq_last_error(const isv_eq_t *h) { return h ? h->err.c_str() : "null handle"; }

extern "C" void isv_eq_destroy(isv_eq_t *h) {
    if (!h) return;
    (void)hipSetDevice(h->trk->device);
    stage_slot_free(h->slot);
    delete h;
}

extern "C" int isv_eq_create(isv_trk_t *trk, const isv_eq_config_t *c, isv_eq_t **out) {
    if (!c || !out) return ISV_ERR_INVALID_ARG;
    *out = nullptr;
    if (!trk) return ISV_ERR_INVALID_ARG;
    if (!std::isfinite(c->clip_limit) || !(c->clip_limit >= 0.0) || c->tiles_x < 1 || c->tiles_x > ISV_EQ_MAX_TILES || c->tiles_y < 1 ||
        c->tiles_y > ISV_EQ_MAX_TILES || c->max_items < 1 || c->max_items > 65535)
        return ISV_ERR_INVALID_ARG;
    isv_eq *h = new isv_eq();
    h->cfg = *c;
    h->trk = trk;
    if (stage_open_failed("isv_eq_create", hipSetDevice(trk->device))) {
        isv_eq_destroy(h);
        return ISV_ERR_DEVICE;
    }
    h->id = ++trk->eq_ids;
    *out = h;
    return ISV_OK;
}

extern "C" int isv_eq_last_ms(isv_eq_t *h, double out_ms[6]) {
    if (!h || !out_ms) return ISV_ERR_INVALID_ARG;
    const StageSlot &s = h->slot;      // the marks of a tracking call: after the CLAHE kernels, after the pyramid kernels
    out_ms[0] = s.call_ms; out_ms[1] = s.part_ms[0]; out_ms[2] = s.part_ms[1]; out_ms[3] = s.part_ms[2]; out_ms[4] = s.upload_ms; out_ms[5] = h->pack_ms;
    return ISV_OK;
}

extern "C" int isv_eq_track_batch(isv_eq_t *h, int32_t n, const isv_trk_item_t *const *items, isv_trk_result_t *results, float *const *cur_pts,
                                  uint8_t *const *flags, float *const *err, float *const *cur_un_pts) {
    if (!h) return ISV_ERR_INVALID_ARG;
    return trk_track_batch(h->trk, h, "isv_eq_track_batch", n, items, results, cur_pts, flags, err, cur_un_pts);
}

extern "C" int isv_eq_apply_batch(isv_eq_t *h, int32_t n, const isv_eq_image_t *const *items, int32_t *status, uint8_t *const *out) {
    StageCall call{h ? h->ctx() : StageCtx{}, "isv_eq_apply_batch"};
    if (const int rc = call.enter(n, items, status); rc != ISV_OK || n == 0) return rc;
    if (n > h->cfg.max_items) return call.fail(ISV_ERR_CAPACITY, "more items than max_items");
    if (!out) return call.fail(ISV_ERR_INVALID_ARG, "null output array");
    const isv_trk_config_t &lim = h->trk->cfg;
    // the refusals: the tracker's size and stride checks (tests/native/isv_eq_oracle.c has the same)
    std::vector<TrkJob> jobs;
    std::vector<int> who;                          // jobs[k] is items[who[k]]
    size_t n_img = 0;
    int maxW = 0, maxH = 0;
    for (int i = 0; i < n; i++) {
        const isv_eq_image_t *it = items[i];
        int s = ISV_TRK_OK;
        if (it->width < 1 || it->height < 1 || it->stride < it->width || !it->data || !out[i]) s = ISV_TRK_INPUT;
        else if (it->width > lim.max_width || it->height > lim.max_height) s = ISV_TRK_CAPACITY;
        status[i] = s;
        if (s != ISV_TRK_OK) continue;
        TrkJob J;
        memset(&J, 0, sizeof(J));
        J.src_off = J.dst_off = n_img;             // the output block mirrors the upload block's images
        J.s.lw[0] = it->width; J.s.lh[0] = it->height; J.s.nlev = 1;
        n_img += ((size_t)it->width * it->height + 15) & ~(size_t)15;
        jobs.push_back(J); who.push_back(i);
        if (it->width > maxW) maxW = it->width;
        if (it->height > maxH) maxH = it->height;
    }
    const int m = (int)jobs.size();
    h->last.assign(n, EqLast{});
    if (m == 0) return ISV_OK;
    // one upload block: [jobs | images, packed without their strides, each 16-byte aligned]; then, device only: the equalised images at
    // the same offsets, the LUTs of every job's tiles
    BlockLayout L;
    const size_t o_job = L.add(sizeof(TrkJob) * m), o_img = L.add(n_img + 16);
    const size_t up_end = L.end;
    const size_t o_out = L.add(n_img + 16), o_lut = L.add(h->lut_bytes() * m);
    const auto t_pack = std::chrono::steady_clock::now();
    std::vector<char> &up = h->up;
    up.resize(up_end);
    memcpy(up.data() + o_job, jobs.data(), sizeof(TrkJob) * m);
    for (int k = 0; k < m; k++) {
        const isv_eq_image_t *it = items[who[k]];
        char *dst = up.data() + o_img + jobs[k].src_off;
        if (it->stride == it->width) memcpy(dst, it->data, (size_t)it->width * it->height);
        else for (int y = 0; y < it->height; y++) memcpy(dst + (size_t)y * it->width, it->data + (size_t)y * it->stride, it->width);
    }
    const double pack_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_pack).count();
    hipStream_t stream = h->trk->stream;
    char *block = nullptr;
    const int rc = call.run(
        up, {}, L.end,
        [&](char *d, auto &&) {
            block = d;
            eq_launch(*h, stream, (const TrkJob *)(d + o_job), m, (const uint8_t *)(d + o_img), (uint8_t *)(d + o_out), (uint8_t *)(d + o_lut), maxW, maxH);
        },
        {},
        [&] {                                      // the images, each straight into its caller's array
            hipError_t e = hipSuccess;
            for (int k = 0; k < m && e == hipSuccess; k++)
                e = hipMemcpyAsync(out[who[k]], block + o_out + jobs[k].dst_off, (size_t)jobs[k].s.lw[0] * jobs[k].s.lh[0], hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            return e;
        });
    if (rc != ISV_OK) return rc;
    for (int k = 0; k < m; k++) h->last[who[k]].lut_off[0] = (int64_t)(o_lut + h->lut_bytes() * k);
    h->pack_ms = pack_ms;
    return ISV_OK;
}

extern "C" int isv_internal_eq_read_luts(isv_eq_t *h, int32_t item, int32_t which, uint8_t *out, int32_t *tiles_x, int32_t *tiles_y) {
    if (!h || item < 0 || (size_t)item >= h->last.size() || which < 0 || which > 1 || h->last[item].lut_off[which] < 0) return ISV_ERR_INVALID_ARG;
    if (tiles_x) *tiles_x = h->cfg.tiles_x;
    if (tiles_y) *tiles_y = h->cfg.tiles_y;
    if (!out) return ISV_OK;
    HIPCHK(h, hipSetDevice(h->trk->device));
    HIPCHK(h, hipMemcpyAsync(out, (const char *)h->slot.d + h->last[item].lut_off[which], h->lut_bytes(), hipMemcpyDeviceToHost, h->trk->stream));
    HIPCHK(h, hipStreamSynchronize(h->trk->stream));
    return ISV_OK;
}
