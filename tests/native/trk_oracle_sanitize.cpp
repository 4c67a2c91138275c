// trk_oracle_sanitize.cpp -- stand-alone AddressSanitizer / UBSan run of the serial restatement of the feature tracking
// (tests/native/isv_trk_oracle.c, compiled together with this file) on its border scenarios: images from 1 x 1 up to 200 x 120, a
// stride larger than the width, points on, at and beyond every edge (ip = -21 and -22, W - 1 and W), far outside and beyond the
// range of int, each quirk hook, each capacity and each malformed item.  Every image and every output array is an exact-size heap
// block, so that one byte read or written too far is seen.  Built and run as a child process by tests/test_trk_sanitize.py; prints
// "ok: ..." and exits 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "isvins_tracker.h"

extern "C" {
void isvo_trk_track(const isv_trk_config_t *c, const isv_trk_item_t *it, isv_trk_result_t *r, float *cur_pts, uint8_t *flags, float *err,
                    float *cur_un_pts, int32_t *term, uint8_t *pyr_prev, uint8_t *pyr_cur);
int isvo_trk_levels(int W, int H, int32_t lw[4], int32_t lh[4], int64_t loff[4]);
void isvo_trk_scharr(const uint8_t *img, int W, int H, int16_t *ix, int16_t *iy);
void isvo_trk_set_quirks_off(int bits);
}

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }

int g_runs = 0, g_tracked = 0, g_levels_seen = 0;

template <typename T> T *exact(size_t n) { return (T *)malloc(n ? n * sizeof(T) : 1); }

// a smooth image and the same image one pixel to the right, so that some points do track
uint8_t *image(int W, int H, int stride, size_t bytes, int shift) {
    uint8_t *img = exact<uint8_t>(bytes);
    for (size_t i = 0; i < bytes; i++) img[i] = 0xEE;
    for (int y = 0; bytes && y < H; y++)
        for (int x = 0; x < W; x++)
            img[(size_t)y * stride + x] = (uint8_t)(128.0 + 60.0 * std::sin(0.31 * (x - shift) + 0.2 * y) + 50.0 * std::cos(0.23 * y - 0.11 * (x - shift)));
    return img;
}

// one item through the restatement; returns whether its status is the expected one and its outputs are sane
bool run(const isv_trk_config_t &cfg, int W, int H, int stride, const std::vector<float> &pts, int want, int null_which = 0, int n_points_override = -2, int slot = 0) {
    const size_t bytes = H > 0 && W > 0 && stride >= W ? (size_t)(H - 1) * stride + W : 0;     // the last row ends at its width, not its stride
    uint8_t *prev = image(W, H, stride, bytes, 0), *cur = image(W, H, stride, bytes, 1);
    const int np = (int)pts.size() / 2;
    float *p = exact<float>(pts.size());
    if (!pts.empty()) memcpy(p, pts.data(), pts.size() * sizeof(float));
    isv_trk_item_t it{slot, W, H, stride, n_points_override != -2 ? n_points_override : np, 0, null_which == 1 ? nullptr : cur, null_which == 2 ? nullptr : prev, p};
    int32_t lw[4], lh[4];
    int64_t lo[4];
    size_t pyr = 0;
    if (W > 0 && H > 0 && W <= cfg.max_width && H <= cfg.max_height) {
        const int n = isvo_trk_levels(W, H, lw, lh, lo);
        pyr = (size_t)(lo[n - 1] + (int64_t)lw[n - 1] * lh[n - 1]);
        g_levels_seen |= 1 << n;
    }
    float *cp = exact<float>(2 * (size_t)np), *un = exact<float>(2 * (size_t)np), *er = exact<float>(np);
    uint8_t *fl = exact<uint8_t>(np), *pp = exact<uint8_t>(pyr), *pc = exact<uint8_t>(pyr);
    int32_t *term = exact<int32_t>(4 * (size_t)np);
    isv_trk_result_t r;
    isvo_trk_track(&cfg, &it, &r, cp, fl, er, un, term, pp, pc);
    int status = r.status;
    if (status == ISV_TRK_OK) {
        int kept = 0;
        for (int k = 0; k < np; k++) {
            if (fl[k] > 3 || !std::isfinite(cp[2 * k]) || !std::isfinite(cp[2 * k + 1]) || !std::isfinite(er[k]) || er[k] < 0) status = -1;
            if (!(fl[k] & 1) && (er[k] != 0 || un[2 * k] != 0 || un[2 * k + 1] != 0)) status = -1;
            kept += fl[k] == 3;
        }
        if (kept != r.n_kept || r.n_points != np) status = -1;
        g_tracked += kept;
    }
    if (W > 0 && H > 0 && W <= 64 && H <= 64 && stride == W) {              // the derivative image of small levels, edges included
        int16_t *ix = exact<int16_t>((size_t)W * H), *iy = exact<int16_t>((size_t)W * H);
        isvo_trk_scharr(prev, W, H, ix, iy);
        free(ix); free(iy);
    }
    free(prev); free(cur); free(p); free(cp); free(un); free(er); free(fl); free(pp); free(pc); free(term);
    g_runs++;
    if (status != want) printf("FAILED: %d x %d stride %d, %d points: status %d, expected %d\n", W, H, stride, np, status, want);
    return status == want;
}

}  // namespace

int main() {
    isv_trk_config_t cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.max_slots = 4; cfg.max_items = 1; cfg.max_width = 200; cfg.max_height = 120; cfg.max_points = 64; cfg.win = ISV_TRK_WIN; cfg.max_level = ISV_TRK_MAX_LEVEL;
    cfg.fx = 461.6; cfg.fy = 460.3; cfg.cx = 363.0; cfg.cy = 248.1; cfg.k1 = -0.2917; cfg.k2 = 0.08228; cfg.p1 = 5.333e-05; cfg.p2 = -1.578e-04;
    bool ok = true;
    const float big = 3.0e9f, huge = std::numeric_limits<float>::max();
    auto points = [&](int W, int H) {
        std::vector<float> p{-10.5f, H * 0.5f, -11.5f, H * 0.5f, W + 9.5f, H * 0.5f, W + 10.0f, H * 0.5f, W * 0.5f, -10.25f, W * 0.5f, -11.0f, W * 0.5f, H + 9.99f,
                             W * 0.5f, H + 10.0f, -11.0f, -11.0f, W + 9.999f, H + 9.999f, 0.0f, 0.0f, W - 1.0f, H - 1.0f, (float)W, (float)H, -0.5f, -0.5f,
                             W * 0.3f, H * 0.6f, W * 0.5f + 0.25f, H * 0.5f - 0.75f, 10.0f, 10.0f, W - 11.0f, H - 11.0f, 1.0e6f, -1.0e6f, big, 5.0f, 5.0f, -big, huge, -huge,
                             -huge, huge, 2147483648.0f, 1.0f, -2147483904.0f, 1.0f, 2147483520.0f, -2147483648.0f};
        for (int k = 0; k < 12; k++) { p.push_back((float)((double)(rnd() % 4096) / 4096.0 * (W + 44) - 22.0)); p.push_back((float)((double)(rnd() % 4096) / 4096.0 * (H + 44) - 22.0)); }
        return p;
    };
    const int sizes[][3] = {{1, 1, 1}, {1, 9, 3}, {9, 1, 9}, {2, 2, 5}, {3, 2, 3}, {5, 5, 5}, {21, 21, 21}, {22, 22, 22}, {24, 23, 24}, {43, 42, 43}, {43, 43, 50}, {44, 45, 44},
                            {64, 48, 64}, {97, 61, 104}, {85, 86, 85}, {200, 120, 200}, {175, 120, 177}, {199, 119, 199}};
    for (int quirks : {0, 1, 2, 4, 8})
        for (const auto &s : sizes) {
            isvo_trk_set_quirks_off(quirks);
            ok &= run(cfg, s[0], s[1], s[2], points(s[0], s[1]), ISV_TRK_OK);
            ok &= run(cfg, s[0], s[1], s[2], {}, ISV_TRK_OK);
        }
    isvo_trk_set_quirks_off(0);
    ok &= run(cfg, 201, 10, 201, {}, ISV_TRK_CAPACITY);
    ok &= run(cfg, 10, 121, 10, {}, ISV_TRK_CAPACITY);
    ok &= run(cfg, 30, 30, 30, std::vector<float>(130, 14.0f), ISV_TRK_CAPACITY);      // 65 points
    ok &= run(cfg, 30, 30, 29, points(30, 30), ISV_TRK_INPUT);
    ok &= run(cfg, 0, 30, 30, {}, ISV_TRK_INPUT);
    ok &= run(cfg, 30, 0, 30, {}, ISV_TRK_INPUT);
    ok &= run(cfg, -1, 30, 30, {}, ISV_TRK_INPUT);
    ok &= run(cfg, 30, 30, 30, {}, ISV_TRK_INPUT, 1);
    ok &= run(cfg, 30, 30, 30, {}, ISV_TRK_INPUT, 2);
    ok &= run(cfg, 30, 30, 30, {}, ISV_TRK_INPUT, 0, -1);
    ok &= run(cfg, 30, 30, 30, {}, ISV_TRK_INPUT, 0, -2, 4);
    ok &= run(cfg, 30, 30, 30, {}, ISV_TRK_INPUT, 0, -2, -1);
    ok &= run(cfg, 30, 30, 30, {1.0f, std::numeric_limits<float>::quiet_NaN()}, ISV_TRK_INPUT);
    ok &= run(cfg, 30, 30, 30, {std::numeric_limits<float>::infinity(), 2.0f}, ISV_TRK_INPUT);
    cfg.k1 = cfg.k2 = cfg.p1 = cfg.p2 = 0.0;
    ok &= run(cfg, 200, 120, 200, points(200, 120), ISV_TRK_OK);
    if (!ok || g_tracked < 200 || (g_levels_seen & 0x1E) != 0xE) { printf("FAILED (%d runs, %d tracked, levels %x)\n", g_runs, g_tracked, g_levels_seen); return 1; }
    printf("ok: %d runs, %d points tracked\n", g_runs, g_tracked);
    return 0;
}
