// pre_oracle_sanitize.cpp -- stand-alone AddressSanitizer / UBSan run of the serial restatement of the IMU pre-integration
// (tests/native/isv_pre_oracle.c, compiled together with this file) over the shapes of the case table tests/pre_cases.py: reset PUSH
// items of 0, 1, 2, 10, 64, 65 and max_samples samples with and without the nav state and the record copy, zero gyro, a rotation of
// about 1 rad per step, dt = 0; split pushes, repropagate (also of an empty buffer), merge (also from an empty source and up to the
// cap exactly), a reset on a used slot; and every refusal.  Every sample array is an exact-size heap block and the store's arrays are
// the restatement's own exact-size blocks, so that one element read or written too far is seen.  Built and run as a child process by
// tests/test_pre_sanitize.py; prints "ok: ..." and exits 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include "isvins_preint.h"

extern "C" {
struct isvo_pre;
isvo_pre *isvo_pre_new(const isv_pre_config_t *c);
void isvo_pre_free(isvo_pre *o);
int isvo_pre_run_batch(isvo_pre *o, int32_t n, const isv_pre_item_t *const *items, isv_pre_result_t *results);
}

namespace {

template <typename T> T *exact(size_t n) { return (T *)calloc(n ? n : 1, n ? sizeof(T) : 1); }

uint32_t g_lcg = 2024u;
double unit() { g_lcg = g_lcg * 1664525u + 1013904223u; return (g_lcg >> 8) / 16777216.0; }

int g_items = 0, g_status[4] = {0, 0, 0, 0};

struct Samples {                  // exact-size arrays of n samples
    int n; double *dt, *acc, *gyr;
    // motion 0: ordinary; 1: zero gyro; 2: |w| dt about 1; 3: dt = 0 inside and at the end
    Samples(int n_, int motion) : n(n_), dt(exact<double>(n_)), acc(exact<double>(3 * (size_t)n_)), gyr(exact<double>(3 * (size_t)n_)) {
        for (int i = 0; i < n; i++) {
            dt[i] = motion == 2 ? 0.01 : 0.002 + 0.008 * unit();
            if (motion == 3 && (i == n / 3 || i == n - 1)) dt[i] = 0.0;
            for (int k = 0; k < 3; k++) {
                acc[3 * i + k] = 4.0 * unit() - 2.0 + (k == 2 ? 9.8 : 0.0);
                gyr[3 * i + k] = motion == 1 ? 0.0 : (motion == 2 ? 115.0 : 1.0) * (unit() - 0.5);
            }
        }
    }
    ~Samples() { free(dt); free(acc); free(gyr); }
};

isv_pre_item_t push(int slot, const Samples &s, int lo, int hi, int reset, const isv_pre_nav_t *nav, isv_imu_t *rec) {
    isv_pre_item_t it;
    memset(&it, 0, sizeof(it));
    it.op = ISV_PRE_PUSH; it.slot = slot; it.src_slot = -1; it.reset = reset; it.n_samples = hi - lo;
    it.dt = s.dt + lo; it.acc = s.acc + 3 * lo; it.gyr = s.gyr + 3 * lo;
    for (int k = 0; k < 3; k++) { it.acc_0[k] = k == 2 ? 9.7 : 0.1; it.gyr_0[k] = 0.01 * (k + 1); it.ba[k] = 0.02 * k; it.bg[k] = -0.003 * k; }
    it.nav = nav; it.want_record = rec != nullptr; it.record = rec;
    return it;
}

isv_pre_item_t other(int op, int slot, int src, isv_imu_t *rec) {
    isv_pre_item_t it;
    memset(&it, 0, sizeof(it));
    it.op = op; it.slot = slot; it.src_slot = src; it.ba[0] = 0.01; it.bg[2] = 0.002;
    it.want_record = rec != nullptr; it.record = rec;
    return it;
}

// one call of one item; exits on an unexpected status or a non-finite record
int run(isvo_pre *o, const isv_pre_item_t &it, int want, int want_count) {
    const isv_pre_item_t *p = &it;
    isv_pre_result_t *res = exact<isv_pre_result_t>(1);
    if (isvo_pre_run_batch(o, 1, &p, res) != 0) { printf("the call was refused\n"); exit(2); }
    g_items++; g_status[res->status & 3]++;
    if (res->status != want || res->n_buffered != want_count) { printf("item %d: status %d count %d, expected %d %d\n", g_items, res->status, res->n_buffered, want, want_count); exit(3); }
    if (want == ISV_PRE_OK && it.record)
        for (int k = 0; k < (int)(sizeof(isv_imu_t) / sizeof(double)); k++)
            if (!std::isfinite(((const double *)it.record)[k])) { printf("item %d: record not finite at %d\n", g_items, k); exit(4); }
    const int nb = res->n_buffered;
    free(res);
    return nb;
}

}  // namespace

int main() {
    const int M = 96, S = 8;
    isv_pre_config_t cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.max_slots = S; cfg.max_samples = M; cfg.max_items = 4;
    cfg.acc_n = 0.08; cfg.gyr_n = 0.004; cfg.acc_w = 0.00004; cfg.gyr_w = 2.0e-6; cfg.gravity[2] = 9.81;
    isvo_pre *o = isvo_pre_new(&cfg);
    if (!o) { printf("no store\n"); return 1; }
    isv_pre_nav_t *nav = exact<isv_pre_nav_t>(1);
    nav->R[0] = nav->R[4] = nav->R[8] = 1.0; nav->V[0] = 0.5; nav->Ba[1] = 0.01; nav->Bg[2] = -0.002;
    isv_imu_t *rec = exact<isv_imu_t>(1);
    // the sample counts, the motions, the nav state and the record copy
    const int counts[7] = {0, 1, 2, 10, 64, 65, M};
    for (int c = 0; c < 7; c++)
        for (int motion = 0; motion < 4; motion++) {
            if (motion == 3 && counts[c] == 0) continue;
            Samples s(counts[c], motion);
            run(o, push(c % S, s, 0, s.n, 1, (c + motion) % 2 ? nav : nullptr, motion % 2 ? nullptr : rec), ISV_PRE_OK, s.n);
        }
    // state across calls: 5 + 5, repropagate, an empty buffer, merge, an empty source, a merge up to the cap exactly, a reset on a used slot
    Samples a(10, 0), b(4, 0), fill(M - 14, 0);
    run(o, push(0, a, 0, 5, 1, nav, nullptr), ISV_PRE_OK, 5);
    run(o, push(0, a, 5, 10, 0, nav, rec), ISV_PRE_OK, 10);
    run(o, other(ISV_PRE_REPROPAGATE, 0, -1, rec), ISV_PRE_OK, 10);
    run(o, push(1, b, 0, 0, 1, nullptr, nullptr), ISV_PRE_OK, 0);
    run(o, other(ISV_PRE_REPROPAGATE, 1, -1, rec), ISV_PRE_OK, 0);
    run(o, other(ISV_PRE_MERGE, 0, 1, rec), ISV_PRE_OK, 10);
    run(o, push(1, b, 0, 4, 0, nullptr, nullptr), ISV_PRE_OK, 4);
    run(o, other(ISV_PRE_MERGE, 0, 1, rec), ISV_PRE_OK, 14);
    run(o, push(2, fill, 0, fill.n, 1, nullptr, nullptr), ISV_PRE_OK, M - 14);
    run(o, other(ISV_PRE_MERGE, 2, 0, rec), ISV_PRE_OK, M);
    run(o, push(2, b, 0, 4, 1, nav, rec), ISV_PRE_OK, 4);
    run(o, push(3, fill, 0, fill.n, 1, nullptr, nullptr), ISV_PRE_OK, M - 14);
    run(o, push(3, a, 0, 10, 0, nullptr, nullptr), ISV_PRE_OK, M - 4);
    // the refusals: slot 3 holds M - 4 samples, slot 0 holds 14, slot 1 holds 4, slot 7 is not constructed
    Samples big(M + 1, 0), bad(4, 0);
    run(o, push(7, big, 0, M + 1, 1, nullptr, nullptr), ISV_PRE_CAPACITY, -1);
    run(o, push(3, a, 0, 5, 0, nullptr, nullptr), ISV_PRE_CAPACITY, M - 4);
    run(o, other(ISV_PRE_MERGE, 3, 0, nullptr), ISV_PRE_CAPACITY, M - 4);
    bad.gyr[11] = std::numeric_limits<double>::quiet_NaN();
    run(o, push(1, bad, 0, 4, 0, nullptr, nullptr), ISV_PRE_INPUT, 4);
    bad.gyr[11] = 0.0; bad.dt[0] = std::numeric_limits<double>::infinity();
    run(o, push(1, bad, 0, 4, 1, nullptr, nullptr), ISV_PRE_INPUT, 4);
    isv_pre_item_t it = push(1, b, 0, 4, 0, nullptr, nullptr);
    it.acc = nullptr;
    run(o, it, ISV_PRE_INPUT, 4);
    it = push(1, b, 0, 4, 0, nullptr, nullptr); it.n_samples = -1;
    run(o, it, ISV_PRE_INPUT, 4);
    it = push(1, b, 0, 4, 0, nullptr, nullptr); it.want_record = 1;
    run(o, it, ISV_PRE_INPUT, 4);
    it = push(1, b, 0, 4, 0, nullptr, nullptr); it.op = 7;
    run(o, it, ISV_PRE_INPUT, 4);
    run(o, push(-1, b, 0, 4, 1, nullptr, nullptr), ISV_PRE_INPUT, -1);
    run(o, push(S, b, 0, 4, 1, nullptr, nullptr), ISV_PRE_INPUT, -1);
    run(o, other(ISV_PRE_MERGE, 0, 0, nullptr), ISV_PRE_INPUT, 14);
    run(o, other(ISV_PRE_MERGE, 0, S, nullptr), ISV_PRE_INPUT, 14);
    run(o, other(ISV_PRE_MERGE, 0, -1, nullptr), ISV_PRE_INPUT, 14);
    run(o, push(7, b, 0, 4, 0, nullptr, nullptr), ISV_PRE_UNSET, -1);
    run(o, other(ISV_PRE_REPROPAGATE, 7, -1, nullptr), ISV_PRE_UNSET, -1);
    run(o, other(ISV_PRE_MERGE, 7, 0, nullptr), ISV_PRE_UNSET, -1);
    run(o, other(ISV_PRE_MERGE, 0, 7, nullptr), ISV_PRE_UNSET, 14);
    // one call of four items: a slot named twice, a MERGE whose source is another item's slot
    isv_pre_item_t four[4] = {push(6, b, 0, 4, 1, nullptr, nullptr), push(6, b, 0, 4, 1, nullptr, nullptr), other(ISV_PRE_MERGE, 0, 6, nullptr), other(ISV_PRE_MERGE, 0, 1, rec)};
    const isv_pre_item_t *ptrs[4] = {&four[0], &four[1], &four[2], &four[3]};
    isv_pre_result_t *res = exact<isv_pre_result_t>(4);
    if (isvo_pre_run_batch(o, 4, ptrs, res) != 0 || res[0].status != ISV_PRE_OK || res[1].status != ISV_PRE_INPUT || res[2].status != ISV_PRE_INPUT ||
        res[3].status != ISV_PRE_INPUT || res[3].n_buffered != 14) { printf("the call of four\n"); return 5; }
    if (isvo_pre_run_batch(o, 5, ptrs, res) != -1 || isvo_pre_run_batch(o, 0, nullptr, nullptr) != 0) { printf("the entry point's refusals\n"); return 6; }
    free(res); free(rec); free(nav);
    isvo_pre_free(o);
    printf("ok: %d items (OK %d, CAPACITY %d, INPUT %d, UNSET %d)\n", g_items, g_status[0], g_status[1], g_status[2], g_status[3]);
    return 0;
}
