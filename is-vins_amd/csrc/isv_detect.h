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
