// exr_oracle_sanitize.cpp -- stand-alone AddressSanitizer / UBSan run of the serial restatement of the rotation calibration
// (tests/native/isv_exr_oracle.c, compiled together with this file): synthetic two-view scenes of 0 .. 300 correspondences with and
// without mismatches, unrelated points, both hooks, the degenerate inputs (all points equal, first == second, collinear points, all zero: no model), a
// slot filled to max_frames and refused beyond, and every item refusal.  Every correspondence array and every slot store is an
// exact-size heap block, so that one element read or written too far is seen.  Built and run as a child process by
// tests/test_exr_sanitize.py; prints "ok: ..." and exits 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "isvins_exrot.h"

extern "C" {
void isvo_exr_set_quirks_off(int mask);
void isvo_exr_calibrate_batch(const isv_exr_config_t *cfg, int n, const isv_exr_item_t *const *items, isv_exr_result_t *results, int32_t *frame_counts,
                              double *rics, double *hists, uint8_t *named);
int isvo_exr_last(int32_t *keep_iter, int32_t *n_keeps, int32_t *subset, double *F, double *R1, double *R2, double *t, double *det_first);
void isvo_exr_last_A(double *out);
void isvo_exr_free(void);
}

namespace {

template <typename T> T *exact(size_t n) { return (T *)calloc(n ? n : 1, n ? sizeof(T) : 1); }

uint32_t g_lcg = 12345u;
double unit() { g_lcg = g_lcg * 1664525u + 1013904223u; return (g_lcg >> 8) / 16777216.0; }

int g_runs = 0, g_none = 0, g_lmeds = 0, g_ransac = 0, g_no_model = 0, g_capacity = 0;

struct Store {                    // a slot store of exact size
    isv_exr_config_t cfg;
    int32_t *fc; double *rics, *hists; uint8_t *named;
    explicit Store(const isv_exr_config_t &c) : cfg(c) {
        fc = exact<int32_t>(c.max_slots); rics = exact<double>(9 * (size_t)c.max_slots);
        hists = exact<double>(27 * (size_t)c.max_slots * c.max_frames); named = exact<uint8_t>(c.max_slots);
        for (int s = 0; s < c.max_slots; s++) for (int k = 0; k < 9; k++) rics[9 * s + k] = k % 4 == 0;
    }
    ~Store() { free(fc); free(rics); free(hists); free(named); }
};

// kind 0: a two-view scene, every tenth correspondence a mismatch; 1: unrelated points; 2: all equal; 3: first == second; 4: collinear;
// 5: all zero (the 7-point system has no model: ISV_EXR_NO_MODEL)
double *scene(int n, int kind, double angle) {
    double *c = exact<double>(4 * (size_t)n);
    for (int i = 0; i < n && kind != 5; i++) {
        const double x = -0.5 + unit(), y = -0.35 + 0.7 * unit(), z = 2.0 + 18.0 * unit();
        const double X = x * z - 0.25, Y = y * z + 0.08, Z = z - 0.1, cs = std::cos(angle), sn = std::sin(angle);
        double x2 = (cs * X + sn * Z) / (-sn * X + cs * Z), y2 = Y / (-sn * X + cs * Z);
        if (kind == 0 && i % 10 == 9) y2 += 0.2;
        if (kind == 1) { x2 = -0.5 + unit(); y2 = -0.35 + 0.7 * unit(); }
        c[4 * i] = x; c[4 * i + 1] = y; c[4 * i + 2] = x2; c[4 * i + 3] = y2;
        if (kind == 2) { c[4 * i] = c[4 * i + 2] = 0.125; c[4 * i + 1] = c[4 * i + 3] = -0.25; }
        if (kind == 3) { c[4 * i + 2] = x; c[4 * i + 3] = y; }
        if (kind == 4) { c[4 * i] = -0.4 + 0.002 * i; c[4 * i + 1] = -0.3 + 0.001 * i; c[4 * i + 2] = -0.39 + 0.002 * i; c[4 * i + 3] = -0.29 + 0.001 * i; }
    }
    return c;
}

bool run(Store &S, int slot, int n, int kind, double angle) {
    double *c = scene(n, kind, angle);
    isv_exr_item_t it;
    memset(&it, 0, sizeof(it));
    it.slot = slot; it.n_corres = n; it.corres = n ? c : nullptr;
    it.delta_q[0] = std::cos(angle / 2); it.delta_q[2] = std::sin(angle / 2);
    const isv_exr_item_t *items[1] = {&it};
    isv_exr_result_t res;
    const int before = S.fc[slot];
    isvo_exr_calibrate_batch(&S.cfg, 1, items, &res, S.fc, S.rics, S.hists, S.named);
    bool ok = true;
    if (res.status == ISV_EXR_OK) {
        ok = res.frame_count == before + 1 && S.fc[slot] == before + 1 &&
             res.method == (n < ISV_EXR_MIN_CORRES ? ISV_EXR_NONE : n < ISV_EXR_RANSAC_MIN ? ISV_EXR_LMEDS : ISV_EXR_RANSAC);
        for (int s = 0; ok && s < 4; s++) ok = res.front[s] >= 0 && res.front[s] <= n;
        g_none += res.method == ISV_EXR_NONE; g_lmeds += res.method == ISV_EXR_LMEDS; g_ransac += res.method == ISV_EXR_RANSAC;
        int32_t ki, nk, sub[7];
        double F[9], R1[9], R2[9], t[3], det;
        const int rows = isvo_exr_last(&ki, &nk, sub, F, R1, R2, t, &det);
        double *A = exact<double>(4 * (size_t)rows);
        isvo_exr_last_A(A);
        ok = ok && rows == 4 * res.frame_count;
        free(A);
    } else {
        ok = S.fc[slot] == before && res.frame_count == before && (res.status == ISV_EXR_NO_MODEL || res.status == ISV_EXR_CAPACITY);
        g_no_model += res.status == ISV_EXR_NO_MODEL; g_capacity += res.status == ISV_EXR_CAPACITY;
    }
    g_runs++;
    free(c);
    if (!ok) fprintf(stderr, "failed: n %d kind %d status %d\n", n, kind, res.status);
    return ok;
}

}  // namespace

int main() {
    const isv_exr_config_t cfg = {4, 16, 300, 8};
    const int counts[] = {0, 1, 8, 9, 10, 13, 14, 15, 16, 63, 64, 65, 129, 300};
    bool ok = true;
    for (int hook = 0; hook < 4; hook++) {
        isvo_exr_set_quirks_off(hook);
        for (int kind = 0; kind < 5; kind++) {
            Store S(cfg);
            int k = 0;
            for (int n : counts) {
                ok = run(S, 1 + k % 3, n, kind, 0.05 + 0.02 * k) && ok;
                k++;
            }
        }
    }
    isvo_exr_set_quirks_off(0);
    {   // no model, LMedS and RANSAC, on a slot that holds frames: the slot stays as it is (run() checks the count)
        Store S(cfg);
        ok = run(S, 2, 30, 0, 0.07) && ok;
        const int before = g_no_model;
        const int zero_counts[] = {9, 12, 14, 15, 20, 65};
        for (int n : zero_counts) ok = run(S, 2, n, 5, 0.05) && ok;
        ok = ok && g_no_model == before + 6 && S.fc[2] == 1;
    }
    {   // the history up to max_frames, then the refusal; the last slot of the store, so that its end is the block's end
        Store S(cfg);
        for (int f = 0; f < cfg.max_frames + 2; f++) ok = run(S, cfg.max_slots - 1, 20 + f, 0, 0.05 + 0.01 * f) && ok;
        ok = ok && S.fc[cfg.max_slots - 1] == cfg.max_frames && g_capacity == 2;
    }
    {   // the refusals read no correspondence
        Store S(cfg);
        double *one = exact<double>(4);
        isv_exr_item_t cases[8];
        memset(cases, 0, sizeof(cases));
        for (auto &c : cases) { c.slot = 1; c.n_corres = 1; c.corres = one; c.delta_q[0] = 1.0; }
        cases[0].slot = -1; cases[1].slot = cfg.max_slots; cases[2].n_corres = -1; cases[3].n_corres = 301; cases[3].corres = nullptr;
        cases[4].corres = nullptr; cases[5].delta_q[0] = 0.0; cases[6].delta_q[1] = NAN;
        const int want[8] = {ISV_EXR_INPUT, ISV_EXR_INPUT, ISV_EXR_INPUT, ISV_EXR_CAPACITY, ISV_EXR_INPUT, ISV_EXR_INPUT, ISV_EXR_INPUT, ISV_EXR_OK};
        for (int i = 0; i < 8; i++) {
            const isv_exr_item_t *items[1] = {&cases[i]};
            isv_exr_result_t res;
            isvo_exr_calibrate_batch(&cfg, 1, items, &res, S.fc, S.rics, S.hists, S.named);
            ok = ok && res.status == want[i];
        }
        const isv_exr_item_t *dup[2] = {&cases[7], &cases[7]};
        isv_exr_result_t two[2];
        isvo_exr_calibrate_batch(&cfg, 2, dup, two, S.fc, S.rics, S.hists, S.named);
        ok = ok && two[0].status == ISV_EXR_OK && two[1].status == ISV_EXR_INPUT && S.fc[1] == 2;
        free(one);
    }
    isvo_exr_free();
    if (!ok || g_lmeds == 0 || g_ransac == 0 || g_none == 0 || g_no_model == 0) {
        fprintf(stderr, "exr_oracle_sanitize: failed (%d runs, %d none, %d lmeds, %d ransac)\n", g_runs, g_none, g_lmeds, g_ransac);
        return 1;
    }
    printf("ok: %d runs, %d without a method, %d LMedS, %d RANSAC, %d without a model, %d refused for capacity\n", g_runs, g_none, g_lmeds, g_ransac, g_no_model, g_capacity);
    return 0;
}
