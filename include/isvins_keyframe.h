/*
 * isvins_keyframe.h -- C ABI of the batched KEYFRAME EXTRACTION: what the KeyFrame constructor computes from the image,
 *   KeyFrame::computeWindowBRIEFPoint     src/pose_graph/keyframe.cpp:43-53     BRIEF at the tracked window points
 *   KeyFrame::computeBRIEFPoint           :55-69                                cv::FAST(image, keypoints, 20, true), BRIEF at the
 *                                                                               corners, liftProjective of every corner
 * for many 8-bit grey images in one call (MI355X).  Its outputs are what isvins_bow.h and isvins_loop.h take: brief goes into
 * isv_bow_item_t.brief and isv_loop_pair_t.brief, keypoints_norm and window_brief into the isv_loop_pair_t members of the same
 * names, without conversion.  A 256-bit descriptor is four uint64_t words: bit 64 w + b of the descriptor is bit b of word w.
 *
 * Not here: the 80 x 60 thumbnail (cv::resize, read only under DEBUG_IMAGE), colour input, addKeyFrame's bookkeeping.
 *
 * The arithmetic is RESTATED from OpenCV 3.2.0 as published (features2d: fast.cpp, fast_score.cpp; imgproc: smooth.cpp, filter.cpp),
 * from thirdparty/DVision/BRIEF.cpp:39-106 and from PinholeCamera.cc:461-521, :657-673.  OpenCV is not available to this project, so
 * the restatement cannot be checked against it.  The CPU restatement tests/native/isv_kf_oracle.c pins the GPU, not OpenCV;
 * tests/test_kf_oracle.py pins the restatement against independent numpy statements of the definitions.  Everything is integer
 * arithmetic or a short fixed sequence of IEEE double operations (contraction off): GPU and restatement agree bit for bit.
 *
 *   the blur    BRIEF::compute's cv::GaussianBlur(9 x 9, sigma 2) on 8-bit: getGaussianKernel(9, 2, CV_32F) (exp in double, rounded to
 *               float32, normalised by the double sum of the float32 values), both separable kernels scaled by 256 and rounded to
 *               integers: {7, 17, 32, 46, 52, 46, 32, 17, 7}, sum 256 (every product is at least 0.03 away from a rounding tie).  The
 *               row pass in integers (at most 255 * 256: 16 bits), the column pass in integers (32 bits), (v + 32768) >> 16, border
 *               BORDER_REFLECT_101 (... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...; an axis of length 1 repeats its pixel).
 *   FAST 9-16   on the UNBLURRED image, threshold t: candidates are the pixels with 3 <= x < W - 3, 3 <= y < H - 3; the circle is the
 *               16 Bresenham offsets of radius 3 in OpenCV's order (x, y) = (0,3) (1,3) (2,2) (3,1) (3,0) (3,-1) (2,-2) (1,-3) (0,-3)
 *               (-1,-3) (-2,-2) (-3,-1) (-3,0) (-3,1) (-2,2) (-1,3); a pixel v is a corner iff 9 contiguous circle pixels are all
 *               < v - t or all > v + t (strict).  The score (cornerScore<16>): with d_k = v - p_k, the maximum over the 16 arcs of 9 of
 *               min d_k, the same for -d_k, the larger of the two and of t, minus 1, in a byte.  Non-maximum suppression: a corner is
 *               kept iff its score is STRICTLY greater than the score of each of its 8 neighbours, 0 where the neighbour is no
 *               corner.  Output in row-major order (y, then x), pt = ((float)x, (float)y).
 *   BRIEF       on the blurred image, for corners and window points alike: test i reads x1 = (int)(pt.x + x1[i]), a float32 addition
 *               and C truncation toward zero, the same for y1, x2, y2; bit i is set iff all four coordinates are inside the image and
 *               im(y1, x1) < im(y2, x2), otherwise it is 0.
 *   the lift    PinholeCamera::liftProjective in doubles, in the reference's operation order: mx_d = (1 / fx) u + (-cx / fx), the same
 *               in y; no distortion when k1 = k2 = p1 = p2 = 0, otherwise the recursive model (one distortion() at the distorted point,
 *               then 7 more at the running estimate); keypoints_norm = ((float)(mx_u / 1.0), (float)(my_u / 1.0)).
 *
 * Reference quirks that are KEPT (marked K1.. in the kernels and the restatement):
 *   K1  truncation toward zero makes a coordinate in (-1, 0) read pixel 0: window points are sub-pixel and may sit at the border.
 *   K2  two adjacent corners of equal score suppress each other: both vanish.
 *   K3  the score is the threshold's (the largest t at which the pixel is still a corner), not a contrast measure.
 *   K4  FAST reads the raw image, BRIEF the blurred one.
 *   K5  a test with an end outside the image is bit 0, not skipped.
 *   K6  the extractor blurs the image once per call of compute, so twice per keyframe.  Here it is blurred once; the results are the
 *       same.
 * Deviation (documented, not a quirk): (int) of a float32 outside the range of int is undefined in C; here such a coordinate counts
 * as outside the image (what x86's cvttss2si yields, INT_MIN, is outside as well).
 */
#ifndef ISVINS_KEYFRAME_H
#define ISVINS_KEYFRAME_H

#include <stddef.h>
#include <stdint.h>
#include "isvins_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISV_KF_PATTERN_BITS 256
#define ISV_KF_PATTERN_RADIUS 24

typedef enum isv_kf_status {
    ISV_KF_OK = 0,
    ISV_KF_CAPACITY = 1,          /* width > max_width, height > max_height, n_points > max_points, or more corners than max_keypoints */
    ISV_KF_INPUT = 2              /* negative sizes or counts, stride < width, a null array with a non-zero size, a non-finite window point */
} isv_kf_status_t;

typedef struct isv_kf_config {
    int32_t max_items;            /* images per call, at most 65535                                               */
    int32_t max_width, max_height;/* at most 8192 each                                                            */
    int32_t max_keypoints;        /* corners per image (isv_bow's ISV_BOW_MAX_FEATURES is 8192)                   */
    int32_t max_points;           /* window points per image                                                      */
    int32_t fast_threshold;       /* 20 (keyframe.cpp:58), within [1, 254]                                        */
    int8_t  x1[ISV_KF_PATTERN_BITS], y1[ISV_KF_PATTERN_BITS], x2[ISV_KF_PATTERN_BITS], y2[ISV_KF_PATTERN_BITS];
                                  /* the test pairs of config/brief_pattern.yml, each within [-24, 24]            */
    double  fx, fy, cx, cy;       /* the pinhole model's projection_parameters                                    */
    double  k1, k2, p1, p2;       /* its distortion_parameters                                                    */
} isv_kf_config_t;

typedef struct isv_kf_item {
    int32_t width, height, stride;/* stride in bytes between rows, at least width                                 */
    int32_t n_points;             /* window points                                                                */
    const uint8_t *image;         /* [height][stride], 8-bit grey                                                 */
    const float   *point_2d_uv;   /* [n_points][2]      point_2d_uv                                               */
} isv_kf_item_t;

typedef struct isv_kf_result {
    int32_t status;               /* isv_kf_status_t                                                              */
    int32_t n_keypoints;          /* keypoints.size() after cv::FAST, also when it exceeds max_keypoints (0 where FAST did not run) */
    int32_t n_points;             /* the item's                                                                   */
    int32_t _pad;
} isv_kf_result_t;

typedef struct isv_kf isv_kf_t;

/* Fails with ISV_ERR_DEVICE without a GPU: there is no CPU path.  ISV_ERR_INVALID_ARG for a pattern value outside [-24, 24], a
 * non-positive size, count or focal length, a threshold outside [1, 254], non-finite intrinsics. */
int  isv_kf_create(const isv_kf_config_t *cfg, isv_kf_t **out);
void isv_kf_destroy(isv_kf_t *h);
const char *isv_kf_last_error(const isv_kf_t *h);

/* items[0..n): one packed upload (the images are the bulk), k_kf_blur, k_kf_fast, k_kf_select, k_kf_brief, one download,
 * synchronous on the handle's own stream.  results [n].  The output arrays are [n] pointers each, caller-owned; with c = min(max_keypoints,
 * the item's candidate pixels) an item's are
 *   brief           [c][4]         brief_descriptors               keypoints_uv  [c][2]   keypoints[i].pt
 *   keypoints_norm  [c][2]         keypoints_norm                  score         [c]      keypoints[i].response
 *   window_brief    [n_points][4]  window_brief_descriptors
 * and [n_keypoints] / [n_points] of them are written.  An item that cannot be extracted is refused by its status (ISV_KF_CAPACITY,
 * ISV_KF_INPUT), never truncated: a refused item changes nothing and leaves its arrays untouched; the call returns ISV_OK whenever it
 * ran.  An item's outputs do not depend, bit for bit, on the batch it is in. */
int  isv_kf_extract_batch(isv_kf_t *h, int32_t n, const isv_kf_item_t *const *items, isv_kf_result_t *results, uint64_t *const *brief,
                          float *const *keypoints_uv, float *const *keypoints_norm, uint8_t *const *score, uint64_t *const *window_brief);
/* milliseconds of the last successful call: the whole call (host clock), k_kf_blur, k_kf_fast, k_kf_select, k_kf_brief, the upload of
 * the packed block (HIP events), the packing of that block on the host (host clock) */
int  isv_kf_last_ms(isv_kf_t *h, double out_ms[7]);

#ifdef __cplusplus
}
#endif
#endif /* ISVINS_KEYFRAME_H */
