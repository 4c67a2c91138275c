// isv_tracker.h -- internal to the feature tracking (isv_tracker.hip), outside include/: the debug read-back of a slot's pyramids,
// so that the tests report a wrong pyramid as a wrong pyramid rather than as wrong tracks; and the tracker handle itself with its
// slots, which the feature detection (isv_detect.hip) reads: a detector works on level 0 of a slot's resident pyramid; and the one
// body of the tracking call, which the CLAHE (isv_equalize.hip) runs with its kernels in place of the level-0 copy.
#pragma once
#include "../../include/isvins_tracker.h"

#ifdef __cplusplus
extern "C" {
#endif

// One level of a pyramid of `slot`: which = 0 the resident one (the cur image of the slot's last successful item), which = 1 the other
// buffer (the prev image of that item).  width / height receive the level's size (either may be NULL); out: NULL or [height][width]
// packed.  ISV_ERR_INVALID_ARG for an empty slot or a level the pyramid does not have.  Synchronous.
int isv_internal_trk_read_level(isv_trk_t *h, int32_t slot, int32_t which, int32_t level, uint8_t *out, int32_t *width, int32_t *height);

#ifdef __cplusplus
}
#endif

#ifdef __HIPCC__
#include <functional>
#include "isv_stage_launch.h"
#include "isv_pinhole.h"

constexpr int kTrkLevels = ISV_TRK_MAX_LEVEL + 1;

struct TrkShape {                 // a pyramid's levels: sizes and packed offsets
    int32_t lw[kTrkLevels], lh[kTrkLevels];
    uint32_t lo[kTrkLevels];
    int32_t nlev, pad;
};

struct TrkJob {                   // one pyramid to build: an uploaded image -> a slot buffer
    uint64_t src_off, dst_off;    // into the upload block's images; into the store
    TrkShape s;
};

struct TrkItem {                  // one item that passed every check
    uint64_t prev_off, cur_off;   // the two pyramids, into the store
    TrkShape s;
    int32_t np, pt_off, pad[2];
};

// par: which of the slot's two buffers is resident; tag: who wrote it, 0 a raw image (isv_trk_track_batch), else an equaliser's id
struct TrkSlot { int32_t W = 0, H = 0, par = 0, valid = 0, tag = 0; };

struct isv_trk : StageHandle {
    isv_trk_config_t cfg;
    PinholeCam cam;
    double pack_ms = 0;           // the host's packing of the last successful call
    uint8_t *d_store = nullptr;   // [max_slots][2][slot_bytes]: the slots' pyramids
    size_t slot_bytes = 0;        // a pyramid of max_width x max_height, rounded up to 256
    std::vector<TrkSlot> slots;
    std::vector<int32_t> named;   // [max_slots]: how many good items of the call name the slot (valid where stamp is the call's serial)
    std::vector<int64_t> stamp;
    std::vector<int64_t> gen;     // [max_slots]: bumped whenever a slot's resident image is replaced or dropped (isv_frontend.hip compares it)
    int64_t serial = 0;
    int32_t eq_ids = 0;           // equalisers created on this handle so far: the next one's id is eq_ids + 1
    std::vector<char> up;         // the upload block's host image (grow-only: an image batch is large)
    // the store offset of a slot's buffer; level 0 of a pyramid is at its start
    size_t store_off(int slot_i, int buf) const { return ((size_t)slot_i * 2 + buf) * slot_bytes; }
};

struct isv_eq;
// isv_trk_track_batch's body (`entry` names the caller).  eq == nullptr: the raw images become level 0, on the handle's own stage
// slot.  Otherwise the equaliser's kernels write level 0 (isv_equalize.h), and the call's block, times and error text are the equaliser's.
int trk_track_batch(isv_trk *h, isv_eq *eq, const char *entry, int32_t n, const isv_trk_item_t *const *items, isv_trk_result_t *results,
                    float *const *cur_pts, uint8_t *const *flags, float *const *err, float *const *cur_un_pts);

// The launch sequence of that body, on device-resident records, for isv_frontend.hip as well: the level-0 kernels (the CLAHE's with eq,
// which then calls mark() behind them) and k_trk_pyrdown per level on `nj` jobs; then k_trk_track on `m` items, a grid of max_np points
// per item (a lane beyond an item's np returns at once).  Everything goes on the handle's stream.
TrkShape trk_make_shape(int W, int H);
void trk_enqueue_pyramids(isv_trk *h, isv_eq *eq, const TrkJob *d_jobs, int nj, const uint8_t *d_img, uint8_t *d_lut, int maxLev, const int *maxLW, const int *maxLH,
                          const std::function<void()> &mark);
void trk_enqueue_track(isv_trk *h, const TrkItem *d_items, int m, int max_np, const float *d_pts, float *d_cur, float *d_un, float *d_err, uint8_t *d_flags);
#endif
