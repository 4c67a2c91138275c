// isv_keyframe.h -- internal to the keyframe extraction (isv_keyframe.hip), outside include/: the debug read-back of the two
// intermediate images of the handle's last successful call, so that the tests report a wrong blur as a wrong blur and a wrong corner
// score as a wrong score rather than as wrong descriptors.
#pragma once
#include "../../include/isvins_keyframe.h"

#ifdef __cplusplus
extern "C" {
#endif

// item `index` of the last successful isv_kf_extract_batch on h: its blurred image and its FAST score map (0: no corner; before the
// non-maximum suppression), each [height][width] packed, either may be NULL.  ISV_ERR_INVALID_ARG when there was no such call or item
// or the item was refused by the host checks.  Synchronous.
int isv_internal_kf_read_back(isv_kf_t *h, int32_t index, uint8_t *blurred, uint8_t *score_map);

#ifdef __cplusplus
}
#endif
