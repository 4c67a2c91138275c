/* isv_eq_oracle.c -- the serial CPU restatement of include/isvins_equalize.h: CLAHE on one 8-bit image, one tile and one pixel at a
 * time, in the order the header states it (K1, E1, E2, E3 marked).  It pins the GPU kernels of csrc/isv_equalize.hip bit for bit;
 * tests/test_eq_oracle.py pins it against an independent numpy statement.  Built with -ffp-contract=off. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "isvins_equalize.h"

enum { EQ_CLIPPED, EQ_RESIDUAL, EQ_EVEN, EQ_UNCLIPPED, EQ_PAD_COLS, EQ_PAD_ROWS, EQ_COUNTERS };

int isvo_eq_sizeof(int which) { return which == 0 ? (int)sizeof(isv_eq_config_t) : which == 1 ? (int)sizeof(isv_eq_image_t) : -1; }

/* BORDER_REFLECT_101 (cv::borderInterpolate), the general loop: always inside [0, len) */
static int reflect101(int p, int len) {
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}

/* cvRound of a float32, half to even (the default rounding mode), saturated to 8 bits */
static uint8_t sat_u8(float f) {
    const long r = lrintf(f);
    return (uint8_t)(r < 0 ? 0 : r > 255 ? 255 : r);
}

/* the tile grid of a W x H image: grid[0..5] = tw, th, the extended width and height, clip, area; *lut_scale.  0, or -1 for a bad
 * configuration or size */
int isvo_eq_grid(const isv_eq_config_t *c, int W, int H, int32_t grid[6], float *lut_scale) {
    if (!c || W < 1 || H < 1 || c->tiles_x < 1 || c->tiles_x > ISV_EQ_MAX_TILES || c->tiles_y < 1 || c->tiles_y > ISV_EQ_MAX_TILES ||
        !(c->clip_limit >= 0.0) || !isfinite(c->clip_limit))
        return -1;
    int ew = W, eh = H;
    if (W % c->tiles_x != 0 || H % c->tiles_y != 0) {          /* K1: both axes, also the one that divides */
        ew = W + c->tiles_x - W % c->tiles_x;
        eh = H + c->tiles_y - H % c->tiles_y;
    }
    const int tw = ew / c->tiles_x, th = eh / c->tiles_y, area = tw * th;
    int clip = 0;
    if (c->clip_limit > 0.0) {
        const double v = c->clip_limit * area / 256;
        clip = (int)(v < (double)area ? v : (double)area);     /* E3 */
        if (clip < 1) clip = 1;
    }
    grid[0] = tw; grid[1] = th; grid[2] = ew; grid[3] = eh; grid[4] = clip; grid[5] = area;
    *lut_scale = (float)255 / area;
    return 0;
}

/* the tracker's size and stride checks, as isv_eq_apply_batch makes them */
int isvo_eq_check(const isv_trk_config_t *t, const isv_eq_image_t *im) {
    if (im->width < 1 || im->height < 1 || im->stride < im->width || !im->data) return ISV_TRK_INPUT;
    if (im->width > t->max_width || im->height > t->max_height) return ISV_TRK_CAPACITY;
    return ISV_TRK_OK;
}

/* CLAHE of img [H][stride] -> out [H][W] packed (or NULL); luts [tiles_y][tiles_x][256] (or NULL); bins [tiles_y][tiles_x][256]: the
 * histograms after the redistribution (or NULL); counters [EQ_COUNTERS] are added to (or NULL).  0, or -1 as isvo_eq_grid. */
int isvo_eq_apply(const isv_eq_config_t *c, const uint8_t *img, int W, int H, int stride, uint8_t *out, uint8_t *luts, int32_t *bins, int64_t *counters) {
    int32_t g[6];
    float lut_scale;
    if (!img || stride < W || isvo_eq_grid(c, W, H, g, &lut_scale) != 0) return -1;
    const int tw = g[0], th = g[1], clip = g[4], tx_n = c->tiles_x, ty_n = c->tiles_y;
    uint8_t *L = luts ? luts : (uint8_t *)malloc((size_t)tx_n * ty_n * 256);
    if (!L) return -1;
    if (counters) { counters[EQ_PAD_COLS] += g[2] - W; counters[EQ_PAD_ROWS] += g[3] - H; }
    for (int ty = 0; ty < ty_n; ty++)
        for (int tx = 0; tx < tx_n; tx++) {
            int hist[256];
            memset(hist, 0, sizeof(hist));
            for (int y = ty * th; y < (ty + 1) * th; y++)
                for (int x = tx * tw; x < (tx + 1) * tw; x++) hist[img[(size_t)reflect101(y, H) * stride + reflect101(x, W)]]++;
            int clipped = 0;
            if (clip > 0) {
                for (int i = 0; i < 256; i++)
                    if (hist[i] > clip) { clipped += hist[i] - clip; hist[i] = clip; }
                const int batch = clipped / 256;
                int residual = clipped - batch * 256;
                for (int i = 0; i < 256; i++) hist[i] += batch;
                if (counters) {
                    if (clipped > 0) counters[EQ_CLIPPED]++;
                    if (residual != 0) counters[EQ_RESIDUAL]++;
                    if (residual == 0 && clipped > 0) counters[EQ_EVEN]++;
                }
                if (residual != 0) {                           /* E1 */
                    const int step = 256 / residual > 1 ? 256 / residual : 1;
                    for (int i = 0; i < 256 && residual > 0; i += step, residual--) hist[i]++;
                }
            }
            if (counters && clipped == 0) counters[EQ_UNCLIPPED]++;
            uint8_t *lut = L + ((size_t)ty * tx_n + tx) * 256;
            int sum = 0;
            for (int i = 0; i < 256; i++) {
                sum += hist[i];
                lut[i] = sat_u8((float)sum * lut_scale);
            }
            if (bins) memcpy(bins + ((size_t)ty * tx_n + tx) * 256, hist, sizeof(hist));
        }
    if (out) {
        const float inv_tw = 1.0f / tw, inv_th = 1.0f / th;
        for (int y = 0; y < H; y++) {
            const float tyf = y * inv_th - 0.5f;
            int ty1 = (int)floorf(tyf), ty2 = ty1 + 1;
            const float ya = tyf - ty1, ya1 = 1.0f - ya;
            if (ty1 < 0) ty1 = 0;
            if (ty1 > ty_n - 1) ty1 = ty_n - 1;                /* never taken (y < H <= tiles_y th): a bound for the index, as in the kernel */
            if (ty2 > ty_n - 1) ty2 = ty_n - 1;
            for (int x = 0; x < W; x++) {
                const float txf = x * inv_tw - 0.5f;           /* E2 */
                int tx1 = (int)floorf(txf), tx2 = tx1 + 1;
                const float xa = txf - tx1, xa1 = 1.0f - xa;
                if (tx1 < 0) tx1 = 0;
                if (tx1 > tx_n - 1) tx1 = tx_n - 1;
                if (tx2 > tx_n - 1) tx2 = tx_n - 1;
                const int v = img[(size_t)y * stride + x];
                const uint8_t *r1 = L + (size_t)ty1 * tx_n * 256 + v, *r2 = L + (size_t)ty2 * tx_n * 256 + v;
                const float res = (r1[tx1 * 256] * xa1 + r1[tx2 * 256] * xa) * ya1 + (r2[tx1 * 256] * xa1 + r2[tx2 * 256] * xa) * ya;
                out[(size_t)y * W + x] = sat_u8(res);
            }
        }
    }
    if (!luts) free(L);
    return 0;
}
