// eq_oracle_sanitize.cpp -- stand-alone AddressSanitizer / UBSan run of the serial restatement of CLAHE (tests/native/isv_eq_oracle.c,
// compiled together with this file): images from 1 x 1 up to 64 x 48, strides larger than the width, every parameter set of the tests
// (and the largest grid, a clip limit beyond int's range and a tiny one), five contents.  Every image, LUT table, histogram table and
// output is an exact-size heap block -- an image ends at the last row's width, not at its stride -- so that one byte read or written
// too far is seen.  Built and run as a child process by tests/test_eq_sanitize.py; prints "ok: ..." and exits 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "isvins_equalize.h"

extern "C" {
int isvo_eq_grid(const isv_eq_config_t *c, int W, int H, int32_t grid[6], float *lut_scale);
int isvo_eq_check(const isv_trk_config_t *t, const isv_eq_image_t *im);
int isvo_eq_apply(const isv_eq_config_t *c, const uint8_t *img, int W, int H, int stride, uint8_t *out, uint8_t *luts, int32_t *bins, int64_t *counters);
}

namespace {

template <typename T> T *exact(size_t n) { return (T *)malloc(n ? n * sizeof(T) : 1); }

uint8_t pixel(int kind, int x, int y) {
    switch (kind) {
        case 0: return 93;                                                       // a constant
        case 1: return (uint8_t)(((x + y) & 1) * 255);                           // a 0 / 255 checkerboard
        case 2: return (uint8_t)((x * 5 + y * 3) % 256);                         // a ramp
        case 3: return (uint8_t)(28.0 + 9.0 * std::sin(0.9 * x + 0.4 * y) + 5.0 * std::cos(0.7 * y - 0.3 * x));   // dark, low contrast
        default: return (uint8_t)((x * 2654435761u + y * 40503u + (unsigned)(x * y) * 69069u) >> 13);            // scrambled bytes
    }
}

int g_runs = 0;
long long g_pad = 0, g_clipped = 0;

bool run(const isv_eq_config_t &cfg, int W, int H, int stride, int kind) {
    const size_t bytes = (size_t)(H - 1) * stride + W, tiles = (size_t)cfg.tiles_x * cfg.tiles_y;
    uint8_t *img = exact<uint8_t>(bytes);
    memset(img, 0xEE, bytes);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) img[(size_t)y * stride + x] = pixel(kind, x, y);
    uint8_t *out = exact<uint8_t>((size_t)W * H), *luts = exact<uint8_t>(tiles * 256);
    int32_t *bins = exact<int32_t>(tiles * 256);
    int64_t counters[6] = {0, 0, 0, 0, 0, 0};
    int32_t g[6];
    float scale;
    bool ok = isvo_eq_grid(&cfg, W, H, g, &scale) == 0 && isvo_eq_apply(&cfg, img, W, H, stride, out, luts, bins, counters) == 0;
    for (size_t t = 0; ok && t < tiles; t++) {
        long long sum = 0;
        for (int i = 0; i < 256; i++) sum += bins[t * 256 + i];
        ok = sum == g[5] && luts[t * 256 + 255] == 255;
    }
    // the same without the optional outputs: the restatement's own LUT table
    uint8_t *again = exact<uint8_t>((size_t)W * H);
    ok = ok && isvo_eq_apply(&cfg, img, W, H, stride, again, nullptr, nullptr, nullptr) == 0 && memcmp(out, again, (size_t)W * H) == 0;
    ok = ok && isvo_eq_apply(&cfg, img, W, H, stride, nullptr, luts, nullptr, nullptr) == 0;
    if (kind == 0)
        for (size_t i = 0; ok && i < (size_t)W * H; i++) ok = out[i] == out[0];
    g_pad += counters[4] + counters[5]; g_clipped += counters[0];
    g_runs++;
    free(img); free(out); free(luts); free(bins); free(again);
    if (!ok) fprintf(stderr, "failed: %d x %d stride %d kind %d clip %g grid %d x %d\n", W, H, stride, kind, cfg.clip_limit, cfg.tiles_x, cfg.tiles_y);
    return ok;
}

}  // namespace

int main() {
    const isv_eq_config_t params[] = {{3.0, 8, 8, 1, 0}, {0.0, 8, 8, 1, 0}, {40.0, 2, 3, 1, 0}, {3.0, 1, 1, 1, 0}, {3.0, 32, 32, 1, 0}, {1e300, 8, 8, 1, 0},
                                      {1e-9, 3, 5, 1, 0}};
    const int sizes[][3] = {{1, 1, 1}, {1, 7, 1}, {7, 1, 7}, {1, 7, 5}, {3, 3, 3}, {3, 3, 9}, {8, 8, 8}, {9, 9, 9}, {9, 8, 16}, {8, 9, 8}, {15, 17, 15}, {15, 17, 32},
                            {33, 31, 40}, {64, 48, 64}, {61, 47, 64}};
    bool ok = true;
    for (const isv_eq_config_t &cfg : params)
        for (const auto &s : sizes)
            for (int kind = 0; kind < 5; kind++) ok = run(cfg, s[0], s[1], s[2], kind) && ok;
    // the refusals read nothing of the image
    isv_trk_config_t lim;
    memset(&lim, 0, sizeof(lim));
    lim.max_width = 64; lim.max_height = 48;
    uint8_t *one = exact<uint8_t>(1);
    const isv_eq_image_t cases[] = {{0, 1, 1, 0, one}, {1, 0, 1, 0, one}, {2, 1, 1, 0, one}, {1, 1, 1, 0, nullptr}, {65, 1, 65, 0, one}, {1, 49, 1, 0, one}, {1, 1, 1, 0, one}};
    const int want[] = {ISV_TRK_INPUT, ISV_TRK_INPUT, ISV_TRK_INPUT, ISV_TRK_INPUT, ISV_TRK_CAPACITY, ISV_TRK_CAPACITY, ISV_TRK_OK};
    for (int i = 0; i < 7; i++) ok = ok && isvo_eq_check(&lim, &cases[i]) == want[i];
    int32_t g[6];
    float scale;
    const isv_eq_config_t bad = {-1.0, 8, 8, 1, 0};
    ok = ok && isvo_eq_grid(&bad, 8, 8, g, &scale) == -1 && isvo_eq_apply(&bad, one, 1, 1, 1, one, nullptr, nullptr, nullptr) == -1;
    free(one);
    if (!ok || g_pad == 0 || g_clipped == 0) {
        fprintf(stderr, "eq_oracle_sanitize: failed (%d runs, %lld padded, %lld clipped)\n", g_runs, g_pad, g_clipped);
        return 1;
    }
    printf("ok: %d runs, %lld padded columns and rows, %lld clipped tiles\n", g_runs, g_pad, g_clipped);
    return 0;
}
