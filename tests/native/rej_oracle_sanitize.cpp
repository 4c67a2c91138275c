// rej_oracle_sanitize.cpp -- stand-alone AddressSanitizer / UBSan run of the serial restatement of the outlier rejection
// (tests/native/isv_rej_oracle.c, compiled together with this file): synthetic two-view scenes of 0 .. 300 points with and without
// outliers, random unrelated points, every hook, and the degenerate inputs (all points equal, prev == cur, collinear points, 8 points
// with 7 coincident), whose 7-point systems are rank deficient.  Every point array and every status array is an exact-size heap block,
// so that one element read or written too far is seen.  Built and run as a child process by tests/test_rej_sanitize.py; prints
// "ok: ..." and exits 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "isvins_reject.h"

extern "C" {
void isvo_rej_set_quirks_off(int mask);
int isvo_rej_check(const isv_rej_config_t *c, const isv_rej_item_t *it, int has_out);
int isvo_rej_reject(const isv_trk_config_t *t, const isv_rej_config_t *c, const isv_rej_item_t *it, isv_rej_result_t *res, uint8_t *status);
double isvo_rej_median(float *e, int count);
int isvo_rej_last_keeps(int32_t *out, int cap);
}

namespace {

template <typename T> T *exact(size_t n) { return (T *)malloc(n ? n * sizeof(T) : 1); }

uint32_t g_lcg = 12345u;
double unit() { g_lcg = g_lcg * 1664525u + 1013904223u; return (g_lcg >> 8) / 16777216.0; }

int g_runs = 0, g_lmeds = 0, g_ransac = 0, g_none = 0, g_all_rejected = 0;

// kind 0: a two-view scene, projected without the distortion (the lift runs its eight steps on the distorted camera all the same: here
// only memory matters), every fifth point an outlier; 1: unrelated points; 2: all points equal; 3: prev == cur; 4: collinear; 5: the
// first 7 coincident
bool run(const isv_trk_config_t &cam, const isv_rej_config_t &cfg, int n, int kind, int hook) {
    float *prev = exact<float>(2 * (size_t)n), *cur = exact<float>(2 * (size_t)n);
    uint8_t *status = exact<uint8_t>((size_t)n);
    for (int i = 0; i < n; i++) {
        const double x = -0.5 + unit(), y = -0.35 + 0.7 * unit(), z = 2.0 + 6.0 * unit();
        const double X = x * z + 0.3, Y = y * z - 0.05, Z = z + 0.1, c = std::cos(0.04), s = std::sin(0.04);
        double x2 = (c * X + s * Z) / (-s * X + c * Z), y2 = Y / (-s * X + c * Z);
        if (kind == 0 && i % 5 == 4) y2 += 0.05;
        if (kind == 1) { x2 = -0.5 + unit(); y2 = -0.35 + 0.7 * unit(); }
        prev[2 * i] = (float)(cam.fx * x + cam.cx); prev[2 * i + 1] = (float)(cam.fy * y + cam.cy);
        cur[2 * i] = (float)(cam.fx * x2 + cam.cx); cur[2 * i + 1] = (float)(cam.fy * y2 + cam.cy);
        if (kind == 2) { prev[2 * i] = cur[2 * i] = 200.5f; prev[2 * i + 1] = cur[2 * i + 1] = 150.25f; }
        if (kind == 3) { cur[2 * i] = prev[2 * i]; cur[2 * i + 1] = prev[2 * i + 1]; }
        if (kind == 4) { prev[2 * i] = 100.f + 21.f * i; prev[2 * i + 1] = 80.f + 13.f * i; cur[2 * i] = 104.f + 21.f * i; cur[2 * i + 1] = 83.f + 13.f * i; }
        if (kind == 5 && i > 0 && i < 7) { prev[2 * i] = prev[0]; prev[2 * i + 1] = prev[1]; cur[2 * i] = cur[0]; cur[2 * i + 1] = cur[1]; }
    }
    const isv_rej_item_t it = {752, 480, n, 0, prev, cur};
    isv_rej_result_t res;
    memset(status, 0xEE, (size_t)n);
    bool ok = isvo_rej_reject(&cam, &cfg, &it, &res, status) == ISV_TRK_OK && res.n_points == n;
    int sum = 0;
    for (int i = 0; ok && i < n; i++) { ok = status[i] <= 1; sum += status[i]; }
    ok = ok && sum == res.n_kept;
    ok = ok && res.method == (n < ISV_REJ_MIN_POINTS ? ISV_REJ_NONE : n < ISV_REJ_RANSAC_MIN && !(hook & 4) ? ISV_REJ_LMEDS : ISV_REJ_RANSAC);
    int32_t keeps[8];
    ok = ok && isvo_rej_last_keeps(keeps, 8) >= 0;
    g_runs++;
    g_none += res.method == ISV_REJ_NONE; g_lmeds += res.method == ISV_REJ_LMEDS; g_ransac += res.method == ISV_REJ_RANSAC;
    g_all_rejected += n >= ISV_REJ_MIN_POINTS && res.n_kept == 0;
    free(prev); free(cur); free(status);
    if (!ok) fprintf(stderr, "failed: n %d kind %d\n", n, kind);
    return ok;
}

}  // namespace

int main() {
    isv_trk_config_t cam;
    memset(&cam, 0, sizeof(cam));
    cam.fx = 461.6; cam.fy = 460.3; cam.cx = 363.0; cam.cy = 248.1; cam.k1 = -0.2917; cam.k2 = 0.08228; cam.p1 = 5.333e-05; cam.p2 = -1.578e-04;
    const isv_rej_config_t cfg = {1, 300, 460.0, 1.0};
    const int counts[] = {0, 1, 7, 8, 9, 13, 14, 15, 16, 63, 64, 65, 129, 300};
    bool ok = true;
    for (int hook = 0; hook < 16; hook = hook ? hook * 2 : 1) {
        isvo_rej_set_quirks_off(hook);
        for (int n : counts)
            for (int kind = 0; kind < 5; kind++) ok = run(cam, cfg, n, kind, hook) && ok;
        ok = run(cam, cfg, 8, 5, hook) && ok;
    }
    isvo_rej_set_quirks_off(0);
    // the median on exact-size blocks, a NaN and an infinity among the errors
    for (int n = 1; n <= 14; n++) {
        float *e = exact<float>((size_t)n);
        for (int i = 0; i < n; i++) e[i] = i == 2 ? NAN : i == 5 ? INFINITY : (float)((i * 7) % 5);
        const double m = isvo_rej_median(e, n);
        ok = ok && (n <= 3 || m == m);                 // from four errors on the NaN, sorted to the top, is never the middle
        free(e);
    }
    // the refusals read no point
    float *one = exact<float>(2);
    one[0] = one[1] = 1.f;
    const isv_rej_item_t cases[] = {{0, 480, 1, 0, one, one}, {752, 0, 1, 0, one, one}, {8193, 480, 1, 0, one, one}, {752, 480, -1, 0, one, one},
                                    {752, 480, 301, 0, nullptr, nullptr}, {752, 480, 1, 0, nullptr, one}, {752, 480, 1, 0, one, nullptr}, {752, 480, 1, 0, one, one}};
    const int want[] = {ISV_TRK_INPUT, ISV_TRK_INPUT, ISV_TRK_INPUT, ISV_TRK_INPUT, ISV_TRK_CAPACITY, ISV_TRK_INPUT, ISV_TRK_INPUT, ISV_TRK_OK};
    for (int i = 0; i < 8; i++) ok = ok && isvo_rej_check(&cfg, &cases[i], 1) == want[i];
    ok = ok && isvo_rej_check(&cfg, &cases[7], 0) == ISV_TRK_INPUT;
    free(one);
    if (!ok || g_lmeds == 0 || g_ransac == 0 || g_none == 0) {
        fprintf(stderr, "rej_oracle_sanitize: failed (%d runs, %d none, %d lmeds, %d ransac)\n", g_runs, g_none, g_lmeds, g_ransac);
        return 1;
    }
    printf("ok: %d runs, %d without a method, %d LMedS, %d RANSAC, %d with every point rejected\n", g_runs, g_none, g_lmeds, g_ransac, g_all_rejected);
    return 0;
}
