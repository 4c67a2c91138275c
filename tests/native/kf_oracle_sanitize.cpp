// kf_oracle_sanitize.cpp -- stand-alone AddressSanitizer / UBSan run of the serial restatement of the keyframe extraction
// (tests/native/isv_kf_oracle.c, compiled together with this file) on its border scenarios: the tiny images (1 x 1, 1 x 9, 6 x 40,
// 7 x 7, empty), a stride larger than the width, window points on, across and far beyond the border and beyond the range of int,
// each capacity and each malformed item.  Every image and every output array is an exact-size heap block, so that one byte read or
// written too far is seen.  Built and run as a child process by tests/test_kf_sanitize.py; prints "ok: ..." and exits 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "isvins_keyframe.h"

extern "C" {
void isvo_kf_extract(const isv_kf_config_t *c, const isv_kf_item_t *it, isv_kf_result_t *r, uint64_t *brief, float *keypoints_uv,
                     float *keypoints_norm, uint8_t *score, uint64_t *window_brief, uint8_t *blurred, uint8_t *score_map);
int isvo_kf_kernel(int32_t out[9]);
void isvo_kf_set_quirks_off(int bits);
}

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }

int g_runs = 0, g_corners = 0;

template <typename T> T *exact(size_t n) { return (T *)malloc(n ? n * sizeof(T) : 1); }

// one item through the restatement; returns its status, or -1 when a guard value was overwritten
int run(const isv_kf_config_t &cfg, int W, int H, int stride, const std::vector<float> &pts, int want, bool contrast, bool null_image = false,
        int n_points_override = -2) {
    const size_t bytes = H > 0 ? (size_t)(H - 1) * stride + (W > 0 ? W : 0) : 0;     // the last row ends at its width, not its stride
    uint8_t *img = exact<uint8_t>(bytes);
    for (size_t i = 0; i < bytes; i++) img[i] = contrast ? (uint8_t)(rnd() >> 56) : (uint8_t)(100 + (rnd() >> 61));
    const int np = (int)pts.size() / 2;
    float *p = exact<float>(pts.size());
    if (!pts.empty()) memcpy(p, pts.data(), pts.size() * sizeof(float));
    isv_kf_item_t it{W, H, stride, n_points_override != -2 ? n_points_override : np, null_image ? nullptr : img, p};
    const size_t cand = W > 6 && H > 6 ? (size_t)(W - 6) * (H - 6) : 0, cap = cand < (size_t)cfg.max_keypoints ? cand : (size_t)cfg.max_keypoints;
    const size_t px = W > 0 && H > 0 ? (size_t)W * H : 0;
    uint64_t *br = exact<uint64_t>(4 * cap), *wb = exact<uint64_t>(4 * (size_t)np);
    float *uv = exact<float>(2 * cap), *nm = exact<float>(2 * cap);
    uint8_t *sc = exact<uint8_t>(cap), *blur = exact<uint8_t>(px), *smap = exact<uint8_t>(px);
    isv_kf_result_t r;
    isvo_kf_extract(&cfg, &it, &r, br, uv, nm, sc, wb, blur, smap);
    int status = r.status;
    if (status == ISV_KF_OK) {
        g_corners += r.n_keypoints;
        if ((size_t)r.n_keypoints > cap) status = -1;
        for (int k = 0; k < r.n_keypoints; k++)
            if (!(uv[2 * k] >= 3 && uv[2 * k] < W - 3 && uv[2 * k + 1] >= 3 && uv[2 * k + 1] < H - 3) || !std::isfinite(nm[2 * k]) || sc[k] < cfg.fast_threshold) status = -1;
    }
    free(img); free(p); free(br); free(wb); free(uv); free(nm); free(sc); free(blur); free(smap);
    g_runs++;
    if (status != want) printf("FAILED: %d x %d stride %d, %d points: status %d, expected %d\n", W, H, stride, np, status, want);
    return status == want;
}

}  // namespace

int main() {
    isv_kf_config_t cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.max_items = 1; cfg.max_width = 200; cfg.max_height = 120; cfg.max_keypoints = 300; cfg.max_points = 32; cfg.fast_threshold = 20;
    for (int i = 0; i < ISV_KF_PATTERN_BITS; i++) {
        cfg.x1[i] = (int8_t)((int)(rnd() % 49) - 24); cfg.y1[i] = (int8_t)((int)(rnd() % 49) - 24);
        cfg.x2[i] = (int8_t)((int)(rnd() % 49) - 24); cfg.y2[i] = (int8_t)((int)(rnd() % 49) - 24);
    }
    cfg.x1[0] = cfg.y1[0] = -24; cfg.x2[0] = cfg.y2[0] = 24;
    cfg.fx = 461.6; cfg.fy = 460.3; cfg.cx = 363.0; cfg.cy = 248.1; cfg.k1 = -0.2917; cfg.k2 = 0.08228; cfg.p1 = 5.333e-05; cfg.p2 = -1.578e-04;
    int32_t K[9];
    bool ok = isvo_kf_kernel(K) == 1;
    const float big = 3.0e9f, huge = std::numeric_limits<float>::max();
    auto points = [&](int W, int H) {
        return std::vector<float>{-0.5f, H * 0.5f, W * 0.5f, -0.25f, W - 0.4f, H - 0.7f, (float)W, (float)H, -1.0f, -1.0f, 1.0e6f, -1.0e6f, big, 5.0f,
                                  5.0f, -big, huge, -huge, 0.0f, 0.0f, W - 1.0f, H - 1.0f, -24.5f, -24.5f, W + 23.5f, H + 23.5f, W * 0.3f, H * 0.6f};
    };
    const int sizes[][3] = {{7, 7, 7}, {6, 40, 6}, {40, 6, 41}, {1, 1, 1}, {1, 9, 3}, {9, 1, 9}, {2, 2, 5}, {5, 5, 5}, {8, 8, 8}, {64, 48, 64},
                            {97, 61, 104}, {0, 0, 0}, {0, 5, 0}, {5, 0, 8}, {200, 120, 200}};
    for (int quirks : {0, 1, 2, 4})
        for (const auto &s : sizes) {
            isvo_kf_set_quirks_off(quirks);
            ok &= run(cfg, s[0], s[1], s[2], points(s[0], s[1]), ISV_KF_OK, false);
            ok &= run(cfg, s[0], s[1], s[2], {}, ISV_KF_OK, false);
        }
    isvo_kf_set_quirks_off(0);
    ok &= run(cfg, 130, 67, 130, points(130, 67), ISV_KF_CAPACITY, true);            // more corners than max_keypoints
    ok &= run(cfg, 201, 10, 201, {}, ISV_KF_CAPACITY, false);
    ok &= run(cfg, 10, 121, 10, {}, ISV_KF_CAPACITY, false);
    ok &= run(cfg, 20, 20, 20, std::vector<float>(66, 4.0f), ISV_KF_CAPACITY, false);   // 33 points
    ok &= run(cfg, 20, 20, 19, points(20, 20), ISV_KF_INPUT, false);
    ok &= run(cfg, -1, 20, 20, {}, ISV_KF_INPUT, false);
    ok &= run(cfg, 20, 20, 20, {}, ISV_KF_INPUT, false, true);
    ok &= run(cfg, 20, 20, 20, {}, ISV_KF_INPUT, false, false, -1);
    ok &= run(cfg, 20, 20, 20, {1.0f, std::numeric_limits<float>::quiet_NaN()}, ISV_KF_INPUT, false);
    ok &= run(cfg, 20, 20, 20, {std::numeric_limits<float>::infinity(), 2.0f}, ISV_KF_INPUT, false);
    cfg.k1 = cfg.k2 = cfg.p1 = cfg.p2 = 0.0;
    cfg.max_keypoints = 100000;
    ok &= run(cfg, 130, 67, 130, points(130, 67), ISV_KF_OK, true);
    if (!ok || g_corners < 200) { printf("FAILED (%d runs, %d corners)\n", g_runs, g_corners); return 1; }
    printf("ok: %d runs, %d corners\n", g_runs, g_corners);
    return 0;
}
