/*
 * isv_pre_oracle.c -- the serial CPU restatement of include/isvins_preint.h: IntegrationBase's constructor, push_back, repropagate,
 * processIMU's propagation and slideWindow's merge (include/factor/integration_base.h:13-158, src/estimator.cpp:91-124, :1660-1675),
 * one operation per item over a host-side slot store, with the statuses and the refusal rules of isv_pre_run_batch.  It pins the
 * kernel k_pre_integrate of is-vins_amd/csrc/isv_preint.hip; tests/test_pre_oracle.py pins it, bit for bit, against the window
 * manager's host code and, at 1e-12, against the oracle's dense restatement.  TEST INFRASTRUCTURE ONLY: built by the tests into a
 * temporary directory with
 *   gcc -O2 -ffp-contract=off -shared -fPIC
 * and never linked into the library.  The recurrence and the checks are the kernel's own text (isv_preint.h) compiled for the host.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../is-vins_amd/csrc/isv_preint.h"

typedef struct isvo_pre {         /* the slot store: the device's three arrays, on the host */
    isv_pre_config_t cfg;
    isv_imu_t *rec;               /* [max_slots] */
    PreSlotHead *head;            /* [max_slots] */
    double *buf;                  /* [max_slots][max_samples][PRE_SAMPLE] */
    int32_t *n_buf;               /* [max_slots]: the counts the checks read, -1 for a slot that is not constructed */
    uint8_t *named;               /* [max_slots] */
} isvo_pre_t;

int isvo_pre_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(isv_pre_config_t);
    case 1: return (int)sizeof(isv_pre_nav_t);
    case 2: return (int)sizeof(isv_pre_item_t);
    case 3: return (int)sizeof(isv_pre_result_t);
    case 4: return (int)sizeof(isv_imu_t);
    case 5: return (int)sizeof(PreSlotHead);
    default: return -1;
    }
}

int isvo_pre_check_config(const isv_pre_config_t *c) { return c && pre_check_config(c); }

void isvo_pre_free(isvo_pre_t *o) {
    if (!o) return;
    free(o->rec); free(o->head); free(o->buf); free(o->n_buf); free(o->named);
    free(o);
}

isvo_pre_t *isvo_pre_new(const isv_pre_config_t *c) {
    if (!isvo_pre_check_config(c)) return NULL;
    isvo_pre_t *o = (isvo_pre_t *)calloc(1, sizeof(*o));
    if (!o) return NULL;
    const size_t S = (size_t)c->max_slots;
    o->cfg = *c;
    o->rec = (isv_imu_t *)calloc(S, sizeof(isv_imu_t));
    o->head = (PreSlotHead *)calloc(S, sizeof(PreSlotHead));
    o->buf = (double *)calloc(S * c->max_samples * PRE_SAMPLE, sizeof(double));
    o->n_buf = (int32_t *)malloc(S * sizeof(int32_t));
    o->named = (uint8_t *)calloc(S, 1);
    if (!o->rec || !o->head || !o->buf || !o->n_buf || !o->named) { isvo_pre_free(o); return NULL; }
    for (size_t s = 0; s < S; s++) o->n_buf[s] = -1;
    return o;
}

/* the store's arrays, for the tests to read: 0 rec, 1 head, 2 buf */
void *isvo_pre_array(isvo_pre_t *o, int which) { return which == 0 ? (void *)o->rec : which == 1 ? (void *)o->head : (void *)o->buf; }

/* one good item */
static void run_item(isvo_pre_t *o, const isv_pre_item_t *it, isv_pre_result_t *res) {
    const isv_pre_config_t *c = &o->cfg;
    isv_imu_t *rec = o->rec + it->slot;
    PreSlotHead *head = o->head + it->slot;
    double *own = o->buf + (size_t)it->slot * c->max_samples * PRE_SAMPLE;
    const int fresh = it->op == ISV_PRE_PUSH && it->reset;
    const int n0 = fresh || it->op == ISV_PRE_REPROPAGATE ? 0 : head->n_buffered;
    const int n = it->op == ISV_PRE_PUSH ? it->n_samples : it->op == ISV_PRE_MERGE ? o->head[it->src_slot].n_buffered : head->n_buffered;
    const double *src = it->op == ISV_PRE_MERGE ? o->buf + (size_t)it->src_slot * c->max_samples * PRE_SAMPLE : own;
    PreState s;
    double J[225], C[225], nd[6];
    double R[9] = {0}, P[3] = {0}, V[3] = {0};
    pre_noise(c, nd);
    if (fresh) {
        pre_reset(&s, J, C, it->acc_0, it->gyr_0, it->ba, it->bg);
        for (int k = 0; k < 3; k++) { head->lin_acc[k] = it->acc_0[k]; head->lin_gyr[k] = it->gyr_0[k]; }
    } else if (it->op == ISV_PRE_REPROPAGATE)
        pre_reset(&s, J, C, head->lin_acc, head->lin_gyr, it->ba, it->bg);
    else {
        for (int k = 0; k < 3; k++) {
            s.dp[k] = rec->delta_p[k]; s.dv[k] = rec->delta_v[k]; s.ba[k] = rec->linearized_ba[k]; s.bg[k] = rec->linearized_bg[k];
            s.acc_0[k] = head->acc_0[k]; s.gyr_0[k] = head->gyr_0[k];
        }
        for (int k = 0; k < 4; k++) s.dq[k] = rec->delta_q[k];
        s.sum_dt = rec->sum_dt;
        memcpy(J, rec->jacobian, sizeof(J)); memcpy(C, rec->covariance, sizeof(C));
    }
    const int nav = it->op == ISV_PRE_PUSH && it->nav;
    if (nav) {
        memcpy(R, it->nav->R, sizeof(R)); memcpy(P, it->nav->P, sizeof(P)); memcpy(V, it->nav->V, sizeof(V));
    }
    for (int i = 0; i < n; i++) {
        double sm[PRE_SAMPLE];
        if (it->op == ISV_PRE_PUSH) {
            sm[0] = it->dt[i];
            for (int k = 0; k < 3; k++) { sm[1 + k] = it->acc[3 * i + k]; sm[4 + k] = it->gyr[3 * i + k]; }
        } else
            memcpy(sm, src + (size_t)i * PRE_SAMPLE, sizeof(sm));
        if (nav) nav_step(R, P, V, it->nav->Ba, it->nav->Bg, c->gravity, s.acc_0, s.gyr_0, sm[0], sm + 1, sm + 4);
        pre_step(&s, J, C, nd, sm[0], sm + 1, sm + 4);
        if (it->op != ISV_PRE_REPROPAGATE) memcpy(own + (size_t)(n0 + i) * PRE_SAMPLE, sm, sizeof(sm));
    }
    for (int k = 0; k < 3; k++) {
        rec->delta_p[k] = s.dp[k]; rec->delta_v[k] = s.dv[k]; rec->linearized_ba[k] = s.ba[k]; rec->linearized_bg[k] = s.bg[k];
        head->acc_0[k] = s.acc_0[k]; head->gyr_0[k] = s.gyr_0[k];
    }
    for (int k = 0; k < 4; k++) rec->delta_q[k] = s.dq[k];
    rec->sum_dt = s.sum_dt;
    memcpy(rec->jacobian, J, sizeof(J)); memcpy(rec->covariance, C, sizeof(C));
    head->constructed = 1;
    if (it->op != ISV_PRE_REPROPAGATE) head->n_buffered = n0 + n;
    res->status = ISV_PRE_OK; res->n_buffered = head->n_buffered;
    res->sum_dt = s.sum_dt;
    for (int k = 0; k < 3; k++) { res->delta_p[k] = s.dp[k]; res->delta_v[k] = s.dv[k]; res->P[k] = P[k]; res->V[k] = V[k]; }
    for (int k = 0; k < 4; k++) res->delta_q[k] = s.dq[k];
    for (int k = 0; k < 9; k++) res->R[k] = R[k];
    if (it->want_record) *it->record = *rec;
}

/* isv_pre_run_batch on the store: the same checks in the same order, the good items one after the other.  -1 as the entry point
 * refuses (a null argument, n out of range), else 0. */
int isvo_pre_run_batch(isvo_pre_t *o, int32_t n, const isv_pre_item_t *const *items, isv_pre_result_t *results) {
    if (!o || n < 0 || n > o->cfg.max_items || (n > 0 && (!items || !results))) return -1;
    for (int i = 0; i < n; i++)
        if (!items[i]) return -1;
    /* the checks all run before any item does: they read the counts of before the call */
    pre_named_all(&o->cfg, n, items, o->named, 1);
    for (int i = 0; i < n; i++) {
        memset(&results[i], 0, sizeof(results[i]));
        results[i].status = pre_check_item(&o->cfg, items[i], o->n_buf, o->named);
        if (items[i]->slot >= 0 && items[i]->slot < o->cfg.max_slots) o->named[items[i]->slot] |= PRE_NAMED_EARLIER;
    }
    pre_named_all(&o->cfg, n, items, o->named, 0);
    for (int i = 0; i < n; i++)
        if (results[i].status == ISV_PRE_OK) {
            const int after = pre_count_after(items[i], o->n_buf);
            run_item(o, items[i], &results[i]);
            o->n_buf[items[i]->slot] = after;
        }
    for (int i = 0; i < n; i++)
        if (results[i].status != ISV_PRE_OK) results[i].n_buffered = pre_count_of(&o->cfg, items[i]->slot, o->n_buf);
    return 0;
}
