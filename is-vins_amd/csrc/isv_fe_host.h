// isv_fe_host.h -- the host half of the whole-frame feature tracker (isv_frontend.hip; include/isvins_frontend.h has the contract),
// with no HIP in it, so that tests/native/fe_host_sanitize.cpp runs it stand-alone under the sanitizers: the per-item refusals of
// isv_fe_read_image_batch, the validation of a planted state (isv_fe_slot_set) and System::PubImageData's scalar gate.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/isvins_frontend.h"

#define FE_FINITE(v) ((v) - (v) == 0)   // neither an infinity nor a NaN

// what an item's checks need of its slot: the tracker's slot (its resident image) and the front end's (its sequence)
struct FeSlotView {
    int32_t img_valid, W, H;      // the tracker slot's resident image
    int32_t tag_ok;               // ... written by the bound equaliser, or raw when none is bound
    int32_t has_sequence;         // the front end's slot holds a sequence
    int32_t fresh;                // ... and the resident image is still the one the front end wrote (or took at slot_set)
};

// an item's own refusals, in their order; `have_msg`: its four message arrays are there
static inline int fe_check_item(int32_t max_slots, int32_t max_width, int32_t max_height, const isv_fe_item_t *it, int have_msg) {
    if (it->width < 1 || it->height < 1 || it->stride < it->width) return ISV_TRK_INPUT;
    if (it->slot < 0 || it->slot >= max_slots || !it->cur || !have_msg) return ISV_TRK_INPUT;
    if (!FE_FINITE(it->cur_time)) return ISV_TRK_INPUT;
    if (it->width > max_width || it->height > max_height) return ISV_TRK_CAPACITY;
    return ISV_TRK_OK;
}

// ... and those of its slot: a first frame takes any slot; a later frame needs the image the front end left there
static inline int fe_check_slot(const isv_fe_item_t *it, const FeSlotView &s) {
    if (!s.has_sequence) return ISV_TRK_OK;
    if (!s.img_valid || !s.tag_ok || !s.fresh || s.W != it->width || s.H != it->height) return ISV_TRK_INPUT;
    return ISV_TRK_OK;
}

// every good item of a slot that another good item names as well becomes INPUT, so that the order does not matter.  slot_of[i] is
// valid where status[i] is OK.
static inline void fe_refuse_duplicates(int n, const int32_t *slot_of, int32_t *status) {
    std::vector<std::pair<int32_t, int>> named;
    for (int i = 0; i < n; i++)
        if (status[i] == ISV_TRK_OK) named.push_back({slot_of[i], i});
    std::sort(named.begin(), named.end());
    for (size_t a = 0; a < named.size();) {
        size_t b = a + 1;
        while (b < named.size() && named[b].first == named[a].first) b++;
        if (b - a > 1)
            for (size_t k = a; k < b; k++) status[named[k].second] = ISV_TRK_INPUT;
        a = b;
    }
}

// cvRound of a float32, half to even, as the detector rounds a point to its pixel (isv_detect.h: det_round_coord)
static inline bool fe_round_coord(float f, int *out) {
    if (!(f >= -2147483648.0f && f < 2147483648.0f)) return false;
    *out = (int)rintf(f);
    return true;
}

// isv_fe_slot_set's validation of a state with a sequence: ISV_OK, ISV_ERR_CAPACITY or ISV_ERR_INVALID_ARG
static inline int fe_check_state(int32_t max_points, const FeSlotView &s, const isv_fe_state_t *st, const float *prev_pts, const int32_t *ids, const int32_t *track_cnt,
                                 const float *prev_un_pts, const uint8_t *in_map) {
    if (st->n_points < 0 || st->n_id < 0 || !FE_FINITE(st->prev_time)) return ISV_ERR_INVALID_ARG;
    if (st->n_points > max_points) return ISV_ERR_CAPACITY;
    if (!s.img_valid || !s.tag_ok) return ISV_ERR_INVALID_ARG;
    const int n = st->n_points;
    if (n > 0 && (!prev_pts || !ids || !track_cnt || !prev_un_pts || !in_map)) return ISV_ERR_INVALID_ARG;
    std::vector<int32_t> seen;
    for (int i = 0; i < n; i++) {
        int rx, ry;
        const float x = prev_pts[2 * i], y = prev_pts[2 * i + 1];
        if (!FE_FINITE(x) || !FE_FINITE(y) || !fe_round_coord(x, &rx) || !fe_round_coord(y, &ry) || rx < 0 || rx >= s.W || ry < 0 || ry >= s.H) return ISV_ERR_INVALID_ARG;
        if (!FE_FINITE(prev_un_pts[2 * i]) || !FE_FINITE(prev_un_pts[2 * i + 1])) return ISV_ERR_INVALID_ARG;
        if (ids[i] < -1 || ids[i] >= st->n_id) return ISV_ERR_INVALID_ARG;
        if (track_cnt[i] < 1 || track_cnt[i] > (1 << 30) || in_map[i] > 1) return ISV_ERR_INVALID_ARG;
        if (ids[i] >= 0) seen.push_back(ids[i]);
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return ISV_ERR_INVALID_ARG;
    return ISV_OK;
}

// ---- System::PubImageData's scalar logic (System.cpp:56-95, :102-104, :131-135; System.h:46-50, :67) ----
static inline int fe_gate_init(isv_fe_gate_t *g, int32_t freq) {
    if (!g || freq < 1) return ISV_ERR_INVALID_ARG;
    memset(g, 0, sizeof(*g));
    g->pub_count = 1; g->first_image_flag = 1; g->freq = freq;
    return ISV_OK;
}

static inline int fe_gate_step(isv_fe_gate_t *g, double t, isv_fe_gate_out_t *out) {
    if (!g || !out || g->freq < 1) return ISV_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    out->skip = 1;
    if (!g->init_feature) {                       // :56-61
        g->init_feature = 1;
        return ISV_OK;
    }
    if (g->first_image_flag) {                    // :63-70
        g->first_image_flag = 0;
        g->first_image_time = t; g->last_image_time = t;
        return ISV_OK;
    }
    if (t - g->last_image_time > 1.0 || t < g->last_image_time) {      // :72-79: "reset the feature tracker", but no tracker is reset
        g->first_image_flag = 1;
        g->last_image_time = 0;
        g->pub_count = 1;
        return ISV_OK;
    }
    g->last_image_time = t;
    out->skip = 0;
    const double rate = 1.0 * g->pub_count / (t - g->first_image_time);  // (a stamp equal to first_image_time: IEEE, no frame published)
    if (round(rate) <= g->freq) {                 // :82-91
        out->pub_this_frame = 1;
        if (fabs(rate - g->freq) < 0.01 * g->freq) {
            g->first_image_time = t;
            g->pub_count = 0;
        }
    }
    if (out->pub_this_frame) {                    // :102-104, :131-135 (readImage runs in between)
        if (g->pub_count < INT32_MAX) g->pub_count++;
        if (!g->init_pub) g->init_pub = 1;
        else out->deliver = 1;
    }
    return ISV_OK;
}
