// isv_tracker.h -- internal to the feature tracking (isv_tracker.hip), outside include/: the debug read-back of a slot's pyramids,
// so that the tests report a wrong pyramid as a wrong pyramid rather than as wrong tracks.
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
