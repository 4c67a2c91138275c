// isv_equalize.h -- internal to the CLAHE (isv_equalize.hip), outside include/: the debug read-back of the tiles' LUTs, so that the
// tests report a wrong LUT as a wrong LUT rather than as a wrong image; and the equaliser handle itself with the launch of its
// kernels, which the tracker's call (isv_tracker.hip) runs in place of its level-0 copy.
#pragma once
#include "../../include/isvins_equalize.h"

#ifdef __cplusplus
extern "C" {
#endif

// The LUTs of items[item] of the last successful call: after isv_eq_apply_batch of the item's image (which = 0), after
// isv_eq_track_batch of its cur image (which = 0) or of its uploaded prev (which = 1).  tiles_x / tiles_y receive the grid (either may
// be NULL); out: NULL or [tiles_y][tiles_x][256].  ISV_ERR_INVALID_ARG for an item the last call did not have or refused, and for the
// prev of an item that brought none.  Synchronous.
int isv_internal_eq_read_luts(isv_eq_t *h, int32_t item, int32_t which, uint8_t *out, int32_t *tiles_x, int32_t *tiles_y);

#ifdef __cplusplus
}
#endif

#ifdef __HIPCC__
#include "isv_tracker.h"

struct EqLast { int64_t lut_off[2] = {-1, -1}; };      // into the block: the cur (or only) image's LUTs, the uploaded prev's

struct isv_eq {
    isv_eq_config_t cfg;
    isv_trk *trk = nullptr;
    int32_t id = 0;               // the tag of the slots this equaliser writes: unique on its tracker, never 0
    std::string err;
    StageSlot slot;               // the call's device block (grow-only), events and times
    double pack_ms = 0;
    StageCtx ctx() { return StageCtx{trk->device, trk->stream, &slot, &err}; }   // (the device and the stream are the tracker's)
    std::vector<char> up;         // isv_eq_apply_batch's upload block
    std::vector<EqLast> last;     // the last call's items, for the debug read-back
    size_t lut_bytes() const { return (size_t)cfg.tiles_x * cfg.tiles_y * 256; }  // per image
};

// k_eq_lut and k_eq_interp on `nj` jobs: the image at img + src_off, of the job's level-0 size, equalised into dst + dst_off, its LUTs
// into lut + j * lut_bytes().  maxW x maxH bounds the jobs' sizes.
void eq_launch(const isv_eq &e, hipStream_t stream, const TrkJob *jobs, int nj, const uint8_t *img, uint8_t *dst, uint8_t *lut, int maxW, int maxH);
#endif
