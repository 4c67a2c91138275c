// det_oracle_sanitize.cpp -- stand-alone AddressSanitizer / UBSan run of the serial restatement of the feature detection
// (tests/native/isv_det_oracle.c, compiled together with this file) on its border scenarios: images from 1 x 1 up to 64 x 48, a stride
// larger than the width, points on every edge and in every corner whose discs the image clips, radii from 1 to 255 (far larger than
// the image), max_new of 0, 1 and more than there are candidates, a constant image, each capacity and each malformed item.  Every
// image and every output array is an exact-size heap block, so that one byte read or written too far is seen.  Built and run as a
// child process by tests/test_det_sanitize.py; prints "ok: ..." and exits 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "isvins_detect.h"

extern "C" {
void isvo_det_detect(const isv_det_config_t *c, const isv_trk_config_t *cam, const uint8_t *img, int W, int H, int stride, const isv_det_item_t *it,
                     isv_det_result_t *r, int32_t *kept_index, float *new_pts, float *new_un_pts, float *eig_out, uint8_t *mask_out, int64_t *counters);
int isvo_det_disc(uint8_t *mask, int W, int H, int cx, int cy, int r);
void isvo_det_response(const uint8_t *img, int W, int H, int stride, float *eig);
}

namespace {

int g_runs = 0, g_corners = 0, g_kept = 0, g_clipped = 0;

template <typename T> T *exact(size_t n) { return (T *)malloc(n ? n * sizeof(T) : 1); }

uint8_t *image(int W, int H, int stride, size_t bytes, bool constant) {
    uint8_t *img = exact<uint8_t>(bytes);
    for (size_t i = 0; i < bytes; i++) img[i] = 0xEE;
    for (int y = 0; bytes && y < H; y++)
        for (int x = 0; x < W; x++)
            img[(size_t)y * stride + x] = constant ? 77 : (uint8_t)(128.0 + 60.0 * std::sin(0.9 * x + 0.4 * y) + 50.0 * std::cos(0.7 * y - 0.3 * x));
    return img;
}

isv_trk_config_t camera() {
    isv_trk_config_t c;
    memset(&c, 0, sizeof(c));
    c.fx = 461.6; c.fy = 460.3; c.cx = 363.0; c.cy = 248.1; c.k1 = -0.2917; c.k2 = 0.08228; c.p1 = 5.333e-05; c.p2 = -1.578e-04;
    return c;
}

// one item through the restatement; returns whether its status is the expected one and its outputs are sane
bool run(const isv_det_config_t &cfg, int W, int H, int stride, const std::vector<float> &pts, int max_new, int want, bool constant = false, int null_which = 0,
         int n_points_override = -2) {
    const size_t bytes = H > 0 && W > 0 && stride >= W ? (size_t)(H - 1) * stride + W : 0;     // the last row ends at its width, not its stride
    uint8_t *img = image(W, H, stride, bytes, constant);
    const int np = (int)pts.size() / 2;
    float *p = exact<float>(pts.size());
    int32_t *cnt = exact<int32_t>(np);
    if (!pts.empty()) memcpy(p, pts.data(), pts.size() * sizeof(float));
    for (int i = 0; i < np; i++) cnt[i] = 1 + (i * 7) % 3;
    isv_det_item_t it{0, n_points_override != -2 ? n_points_override : np, max_new, 0, null_which == 1 ? nullptr : p, null_which == 2 ? nullptr : cnt};
    const size_t px = W > 0 && H > 0 ? (size_t)W * H : 0, cap = max_new > 0 && max_new <= cfg.max_corners ? (size_t)max_new : 0;
    int32_t *kept = exact<int32_t>(np);
    float *nw = exact<float>(2 * cap), *un = exact<float>(2 * cap), *eig = exact<float>(px);
    uint8_t *mask = exact<uint8_t>(px);
    int64_t counters[8];
    isv_det_result_t r;
    const isv_trk_config_t cam = camera();
    isvo_det_detect(&cfg, &cam, img, W, H, stride, &it, &r, null_which == 3 ? nullptr : kept, null_which == 4 ? nullptr : nw, un, eig, mask, counters);
    bool ok = r.status == want;
    if (r.status == ISV_DET_OK) {
        ok = ok && r.n_kept >= 0 && r.n_kept <= np && r.n_new >= 0 && r.n_new <= max_new && r.n_candidates >= r.n_new;
        for (int k = 0; k < r.n_kept; k++) ok = ok && kept[k] >= 0 && kept[k] < np;
        for (int k = 0; k < r.n_new; k++) ok = ok && nw[2 * k] >= 1 && nw[2 * k] < W - 1 && nw[2 * k + 1] >= 1 && nw[2 * k + 1] < H - 1 && std::isfinite(un[2 * k]);
        g_corners += r.n_new; g_kept += r.n_kept; g_clipped += (int)counters[1];
    } else ok = ok && r.n_kept == 0 && r.n_new == 0;
    g_runs++;
    free(img); free(p); free(cnt); free(kept); free(nw); free(un); free(eig); free(mask);
    if (!ok) fprintf(stderr, "run %d: %d x %d stride %d, %d points, max_new %d: status %d, wanted %d\n", g_runs, W, H, stride, np, max_new, r.status, want);
    return ok;
}

}  // namespace

int main() {
    bool ok = true;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int sizes[][3] = {{1, 1, 1}, {1, 7, 1}, {7, 1, 7}, {2, 5, 2}, {5, 2, 9}, {3, 3, 3}, {4, 3, 4}, {24, 23, 24}, {33, 17, 40}, {64, 48, 64}};
    for (const int r : {1, 2, 3, 30, 255}) {
        isv_det_config_t cfg{4, 16, 500, r, 0.01};
        for (const auto &s : sizes) {
            const int W = s[0], H = s[1], stride = s[2];
            const float x1 = (float)(W - 1), y1 = (float)(H - 1);
            // every corner, the middle of every edge, the centre; some of them twice (a dropped point)
            const std::vector<float> pts = {0.f, 0.f, x1, 0.f, 0.f, y1, x1, y1, x1 * 0.5f, 0.f, x1 * 0.5f, y1, 0.f, y1 * 0.5f, x1, y1 * 0.5f,
                                            x1 * 0.5f, y1 * 0.5f, 0.25f, 0.25f, x1 - 0.25f, y1 + 0.25f, -0.5f, y1 + 0.5f - (H % 2 ? 0.f : 1.f)};
            for (const int max_new : {0, 1, 500}) {
                ok = run(cfg, W, H, stride, {}, max_new, ISV_DET_OK) && ok;
                ok = run(cfg, W, H, stride, {pts[16], pts[17]}, max_new, ISV_DET_OK) && ok;
                ok = run(cfg, W, H, stride, pts, max_new, ISV_DET_OK) && ok;
            }
            ok = run(cfg, W, H, stride, {}, 20, ISV_DET_OK, true) && ok;
        }
    }
    // the disc alone, far larger than its image and centred on each corner
    for (const int r : {1, 7, 40, 255})
        for (const int c : {0, 1, 2, 3}) {
            const int W = 9, H = 6;
            uint8_t *m = exact<uint8_t>((size_t)W * H);
            memset(m, 255, (size_t)W * H);
            g_clipped += isvo_det_disc(m, W, H, c & 1 ? W - 1 : 0, c & 2 ? H - 1 : 0, r);
            free(m);
        }
    // the refusals: each leaves every array untouched (they are exact-size blocks of no or few bytes)
    isv_det_config_t cfg{4, 4, 10, 3, 0.01};
    const std::vector<float> four = {3.f, 3.f, 10.f, 4.f, 20.f, 20.f, 5.f, 18.f};
    ok = run(cfg, 24, 23, 24, four, 10, ISV_DET_OK) && ok;
    ok = run(cfg, 24, 23, 24, {3.f, 3.f, 10.f, 4.f, 20.f, 20.f, 5.f, 18.f, 7.f, 7.f}, 10, ISV_DET_CAPACITY) && ok;
    ok = run(cfg, 24, 23, 24, four, 11, ISV_DET_CAPACITY) && ok;
    ok = run(cfg, 24, 23, 24, four, -1, ISV_DET_INPUT) && ok;
    ok = run(cfg, 24, 23, 24, four, 10, ISV_DET_INPUT, false, 0, -1) && ok;
    ok = run(cfg, 24, 23, 23, four, 10, ISV_DET_INPUT) && ok;
    ok = run(cfg, 0, 23, 24, {}, 10, ISV_DET_INPUT) && ok;
    ok = run(cfg, 24, -2, 24, {}, 10, ISV_DET_INPUT) && ok;
    for (const int null_which : {1, 2, 3, 4}) ok = run(cfg, 24, 23, 24, four, 10, ISV_DET_INPUT, false, null_which) && ok;
    for (const float bad : {nan, inf, -inf, 3.0e9f, -3.0e9f, 23.6f, -0.6f, 24.f, 22.5f})
        for (const int at : {0, 3, 7}) {
            std::vector<float> p = four;
            p[at] = bad;
            ok = run(cfg, 24, 23, 24, p, 10, bad == 22.5f ? ISV_DET_OK : ISV_DET_INPUT) && ok;
        }
    if (!ok || g_corners < 50 || g_kept < 100 || g_clipped < 100) {
        fprintf(stderr, "failed: ok %d, corners %d, kept %d, clipped %d\n", (int)ok, g_corners, g_kept, g_clipped);
        return 1;
    }
    printf("ok: %d runs, %d corners, %d kept points, %d clipped discs\n", g_runs, g_corners, g_kept, g_clipped);
    return 0;
}
