// isv_detect.h -- internal to the feature detection (isv_detect.hip), outside include/: the debug read-back of an item's planes from
// the last call, so that the tests report a wrong response or mask plane as a wrong plane rather than as wrong corners.
#pragma once
#include "../../include/isvins_detect.h"

#ifdef __cplusplus
extern "C" {
#endif

// A plane of items[item] of the last successful isv_det_detect_batch call: which = 0 the response (float32, written when the item's
// max_new > 0), which = 1 the mask (uint8).  width / height receive the plane's size, n_candidates the item's candidate count (any
// may be NULL); out: NULL or [height][width] packed, 4 or 1 bytes per pixel.  ISV_ERR_INVALID_ARG for an item the last call did not
// have or refused, and for the response plane of an item with max_new = 0.  Synchronous.
int isv_internal_det_read_plane(isv_det_t *h, int32_t item, int32_t which, void *out, int32_t *width, int32_t *height, int32_t *n_candidates);

#ifdef __cplusplus
}
#endif

#ifdef __HIPCC__
#include <functional>
#include "isv_tracker.h"

constexpr int kDetMaxR = 255;

struct DetItem {                  // one item that passed every check
    uint64_t img_off;             // level 0 of the slot's resident pyramid, into the tracker's store
    uint64_t mask_off, eig_off, key_off;      // the item's planes, into the call's block
    int32_t W, H, np, pt_off;     // its ordered points: at pt_off of the points section (and of the kept section)
    int32_t max_new, out_off;     // its corners: at out_off of the corner sections
    int32_t pad[2];
};
struct DetPoint { int32_t x, y, idx, pad; };                  // the rounded pixel and the input index
struct DetCount { uint32_t max_key, n_cand; int32_t n_kept, n_new; };     // zeroed before the kernels

struct DetLast { int32_t W = 0, H = 0, valid = 0, has_eig = 0, n_cand = 0; size_t mask_off = 0, eig_off = 0; };

struct isv_det {
    isv_det_config_t cfg;
    isv_trk *trk = nullptr;
    std::string err;
    StageSlot slot;               // the call's device block (grow-only), events and times
    StageCtx ctx() { return StageCtx{trk->device, trk->stream, &slot, &err}; }   // (the device and the stream are the tracker's)
    uint8_t hw[kDetMaxR + 1];     // the disc of radius min_dist: the half-width per |dy|
    std::vector<char> up;
    std::vector<DetLast> last;    // the last call's items, for the debug read-back
    std::vector<int32_t> named;   // as the tracker's
    std::vector<int64_t> stamp;
    int64_t serial = 0;
};

// cvRound of a float32, half to even (the default rounding mode); outside int's range it does not exist.  Host and device: the
// rounded pixel of a DetPoint is formed by this text wherever it is formed (rintf and lrintf round alike in the default mode).
__host__ __device__ inline bool det_round_coord(float f, int *out) {
    if (!(f >= -2147483648.0f && f < 2147483648.0f)) return false;
    *out = (int)rintf(f);
    return true;
}

// The four kernels on `m` device-resident records, on the tracker's stream (isv_det_detect_batch's launch, and isv_frontend.hip's).
// `d` is the block the records' plane offsets refer to; the counts are zero and the mask planes 255 before it.  any_new: whether
// k_det_eig, k_det_cand and k_det_select are launched at all; maxW x maxH and maxPix bound the records' images.  mark() is called
// behind k_det_mask and behind k_det_eig.
void det_enqueue(isv_det *h, const DetItem *d_items, int m, const DetPoint *d_pts, const uint8_t *d_hw, char *d, DetCount *d_counts, int32_t *d_kept, float *d_new,
                 float *d_un, int any_new, int maxW, int maxH, size_t maxPix, const std::function<void()> &mark);
#endif
