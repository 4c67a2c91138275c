/*
 * isvins_frontend.h -- C ABI of the WHOLE-FRAME FEATURE TRACKER: one call per frame does, for many sequences,
 *   FeatureTracker::readImage             src/feature_tracker/feature_tracker_simple.cpp:81-151
 * and the message-building half of
 *   System::PubImageData                  src/System.cpp:102-129
 * on the MI355X.  A front end is bound to a tracker handle (isvins_tracker.h) and to the stages on it: a rejector (isvins_reject.h), a
 * detector (isvins_detect.h) and, for EQUALIZE = 1, an equaliser (isvins_equalize.h).  A sequence's whole FeatureTracker state lives
 * in its SLOT on the device: the image pyramid in the tracker's slot, and here prev_pts, ids, track_cnt, the previous un-distorted
 * point and its in-map flag per point, n_id and prev_time.  The stages' kernels run unchanged, back to back on the tracker's stream,
 * on per-item records that small glue kernels write on the device; the host sees no count between the upload (the images) and the
 * download (the message and the end-of-frame lists), and nothing synchronises in between.
 *
 * readImage, restated line by line (N = max_cnt is MAX_CNT; "the list" is cur_pts / ids / track_cnt, in order):
 *   first frame  the slot has no sequence yet (:94): the image becomes the slot's; setMask on no points; goodFeaturesToTrack(N) and
 *                addPoints (id -1, count 1) run WHATEVER pub_this_frame says (:94-107).  No flow.
 *   later frame  1. the flow on the slot's prev_pts (:114) and inBorder (:116-118);
 *                2. reduceVector of prev_pts, cur_pts, ids, track_cnt by both flag bits (:119-122);
 *                3. track_cnt++ (:124-125);
 *                4. only if pub_this_frame (:126-143): rejectWithF (fewer than 8 points: all are kept) and reduceVector by its
 *                   status; setMask's stable descending order by track_cnt and its kept list; max_new = N - n with n the count
 *                   after rejectWithF (see F3); no detection when max_new <= 0, but setMask has run and may have dropped points;
 *                   addPoints.
 *   always       UndistortPixelMotion: the lift of every point and the velocities (:197-244); updateID from the SLOT'S OWN n_id (the
 *                reference has one static counter for its one tracker: a slot starts at 0); prev_* = cur_*, prev_time = cur_time.
 *   velocity     (float)((double)(cur_un.x - prev_un.x) / (cur_time - prev_time)): the subtraction in float32, the division in double
 *                (:225-227); likewise y.  dt == 0 follows IEEE (an infinity, or NaN for 0 / 0).
 *   the message  only if pub_this_frame: the rows of the list with track_cnt > 1, in list order (System.cpp:114-128, NUM_OF_CAM = 1):
 *                feature_id = id, point = ((double)cur_un.x, (double)cur_un.y, 1.0), uv = cur_pts, velocity.  feature_id and point
 *                are the arguments of isv_estimator_push_image (isvins_estimator.h).
 *
 * Reference quirks that are KEPT:
 *   F1  UndistortPixelMotion runs before updateID: a newborn point enters cur_un_pts_map under the key -1 (only the first newborn
 *       does, std::map::insert keeps the first), so on its next frame its real id is not found and the first published observation
 *       of every feature (track_cnt == 2) carries velocity 0; real velocities start at track_cnt == 3.  The -1 entry is never looked
 *       up (:219); its only effect is that the map is non-empty whenever the previous frame ended with any point.  Here a point
 *       carries a flag "was in the map under its own id" and its previous un-distorted point through every compaction: ids are
 *       unique, so this is the map without the search.
 *   F2  the else branch (:237-242) appends zeros to pts_velocity without clearing it.  It is reached only when prev_un_pts_map is
 *       empty, that is when the previous frame ended with no point (F1) or there was none.  Then the previous pts_velocity was built
 *       for an empty list: either by the cleared loop (:216-236) over no points, or by this branch appending nothing to a vector that
 *       by induction held only zeros.  Every stale entry is therefore zero, and every index the message reads is below the count of
 *       the current list, which is the number of zeros appended.  The values read are zero: zeros are returned.
 * Deviation (documented, not a quirk):
 *   F3  the reference computes n_max_cnt from cur_pts.size() after setMask (:129-130); the detector stage takes max_new with the
 *       points, before its setMask has run, and its callers have always passed MAX_CNT - n with n the count after rejectWithF.  The
 *       front end keeps that: it differs from the reference only on a frame on which setMask drops a point, where the reference
 *       would refill the dropped points in the same frame and this refills them in the next published one.
 * The reset branch of PubImageData (System.cpp:72-79) resets no tracker although its message says so: isv_fe_gate_step restates it
 * as it is.
 */
#ifndef ISVINS_FRONTEND_H
#define ISVINS_FRONTEND_H

#include <stddef.h>
#include <stdint.h>
#include "isvins_tracker.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the bound stages, by their struct tags (isvins_equalize.h, isvins_reject.h, isvins_detect.h name the same types) */
struct isv_eq;
struct isv_rej;
struct isv_det;

typedef struct isv_fe_config {
    int32_t max_items;            /* items per call, 1 .. 65535, at most every bound stage's max_items                    */
    int32_t max_cnt;              /* MAX_CNT, 1 .. the detector's max_corners                                             */
    int32_t max_points;           /* state capacity per slot: max_cnt .. the tracker's, the rejector's and the detector's  */
    int32_t _pad;
} isv_fe_config_t;

typedef struct isv_fe_item {
    int32_t slot;                 /* the sequence's slot on the tracker                                                   */
    int32_t width, height, stride;/* of cur; stride in bytes between rows, at least width                                 */
    const uint8_t *cur;           /* [height][stride], 8-bit grey: _img                                                   */
    double  cur_time;             /* _cur_time, finite                                                                    */
    int32_t pub_this_frame;       /* PUB_THIS_FRAME (isv_fe_gate_step gives it)                                           */
    int32_t _pad;
} isv_fe_item_t;

typedef struct isv_fe_result {
    int32_t status;               /* isv_trk_status_t                                                                     */
    int32_t n_tracked;            /* after the flow and inBorder (0 on a first frame)                                     */
    int32_t n_after_reject;       /* after rejectWithF (n_tracked on an unpublished frame)                                */
    int32_t n_kept;               /* after setMask (n_tracked on an unpublished frame)                                    */
    int32_t n_new;                /* corners born                                                                         */
    int32_t n_points;             /* the list at the end of the frame: n_kept + n_new                                     */
    int32_t n_msg;                /* rows of the message (0 on an unpublished frame)                                      */
    int32_t method, iters;        /* the rejector's (ISV_REJ_NONE, 0 when it did not run)                                 */
    int32_t _pad;
} isv_fe_result_t;

/* a slot's feature state but for its arrays (isv_fe_slot_get / isv_fe_slot_set) */
typedef struct isv_fe_state {
    int32_t has_sequence;         /* 0: the next frame is a first frame, and nothing else here means anything             */
    int32_t n_points;
    int32_t n_id;                 /* the slot's next feature id                                                           */
    int32_t _pad;
    double  prev_time;
} isv_fe_state_t;

/* the scalar state of System::PubImageData (System.h:46-50, :67) */
typedef struct isv_fe_gate {
    int32_t init_feature, first_image_flag, init_pub, pub_count;
    double  first_image_time, last_image_time;
    int32_t freq;                 /* FREQ                                                                                 */
    int32_t _pad;
} isv_fe_gate_t;

typedef struct isv_fe_gate_out {
    int32_t skip;                 /* PubImageData returned before readImage: the frame is not given to the front end      */
    int32_t pub_this_frame;       /* PUB_THIS_FRAME for the frame's item                                                  */
    int32_t deliver;              /* the frame's message goes to the estimator (init_pub drops the first one)             */
    int32_t _pad;
} isv_fe_gate_out_t;

typedef struct isv_fe isv_fe_t;

/* A front end on a tracker handle and the stages bound to it; eq == NULL is EQUALIZE = 0.  ISV_ERR_INVALID_ARG for a null trk, rej,
 * det, cfg or out, a count outside its range above, a stage that is bound to another tracker, a capacity a bound stage cannot take.
 * ISV_ERR_DEVICE when the state cannot be allocated.  All slots start without a sequence.  Destroy it before its stages. */
int  isv_fe_create(isv_trk_t *trk, struct isv_eq *eq, struct isv_rej *rej, struct isv_det *det, const isv_fe_config_t *cfg, isv_fe_t **out);
void isv_fe_destroy(isv_fe_t *h);
const char *isv_fe_last_error(const isv_fe_t *h);

/* items[0..n), n at most max_items (ISV_ERR_CAPACITY beyond, before anything is enqueued): one upload (the images), every stage's
 * kernels and the glue kernels back to back on the tracker's stream, one download, synchronous.  results [n].  Every output is [n]
 * pointers to caller-owned arrays of max_points rows each; item i writes its first n_msg (the message) or n_points (the lists) rows:
 *   feature_id [.] int32, point [.][3] double, uv [.][2] float, velocity [.][2] float         the message; required
 *   cur_pts [.][2] float, cur_un_pts [.][2] float, ids [.] int32, track_cnt [.] int32, pts_velocity [.][2] float
 *                                                       the end-of-frame lists; each of the five may be NULL, and so may any entry
 * An item is refused by its status, never truncated: ISV_TRK_CAPACITY for a width or height beyond the tracker's; ISV_TRK_INPUT for
 * sizes below 1, stride < width, a slot outside the tracker's, a null cur or a null message array, a non-finite cur_time; on a slot
 * with a sequence also for another image size, and for a resident image that something else (isv_trk_track_batch, an equaliser's
 * tracking call, isv_trk_slot_reset) has replaced or dropped since the front end last wrote it; and for a slot that another item of
 * the call names as well (both are refused).  A refused item changes nothing: neither its slot nor its arrays.  An item's outputs do not
 * depend, bit for bit, on the batch it is in.  If the call itself fails on the device, the slots of its items have no sequence
 * afterwards.  The call returns ISV_OK whenever it ran. */
int  isv_fe_read_image_batch(isv_fe_t *h, int32_t n, const isv_fe_item_t *const *items, isv_fe_result_t *results, int32_t *const *feature_id,
                             double *const *point, float *const *uv, float *const *velocity, float *const *cur_pts, float *const *cur_un_pts,
                             int32_t *const *ids, int32_t *const *track_cnt, float *const *pts_velocity);

/* milliseconds of the last successful call: the whole call (host clock); then HIP events: the level-0 (or CLAHE) and pyramid kernels;
 * the flow and its compaction; rejectWithF and setMask's order; setMask, goodFeaturesToTrack and the end of the frame; the upload */
int  isv_fe_last_ms(isv_fe_t *h, double out_ms[6]);

/* Checkpoint and restore of a slot's feature state; the arrays hold max_points rows (get) or n_points rows (set); any array of get may
 * be NULL.  prev_pts [.][2] float, ids [.] int32, track_cnt [.] int32, prev_un_pts [.][2] float, in_map [.] uint8 (F1).  Synchronous.
 * set validates what the kernels rely on later: ISV_ERR_CAPACITY for n_points beyond max_points; ISV_ERR_INVALID_ARG for a negative
 * count or n_id, a non-finite prev_time, a null array with n_points > 0, a slot whose tracker slot has no resident image (or one an
 * equaliser other than the bound one wrote), a non-finite point or one whose rounded pixel is outside that image, an id that is
 * neither -1 nor in [0, n_id) or that occurs twice, a track_cnt outside [1, 2^30], an in_map other than 0 / 1.  With has_sequence = 0
 * it is isv_fe_slot_reset.  After set the front end takes the tracker slot's resident image for the sequence's prev_img.
 * reset leaves the slot without a sequence (its next frame is a first frame, its n_id 0); the tracker's slot is not touched. */
int  isv_fe_slot_get(isv_fe_t *h, int32_t slot, isv_fe_state_t *state, float *prev_pts, int32_t *ids, int32_t *track_cnt, float *prev_un_pts, uint8_t *in_map);
int  isv_fe_slot_set(isv_fe_t *h, int32_t slot, const isv_fe_state_t *state, const float *prev_pts, const int32_t *ids, const int32_t *track_cnt,
                     const float *prev_un_pts, const uint8_t *in_map);
int  isv_fe_slot_reset(isv_fe_t *h, int32_t slot);

/* The scalar logic of System::PubImageData around readImage (System.cpp:56-95, :102-104, :131-135), host only.  init sets the
 * reference's initial values (pub_count 1, first_image_flag set) and FREQ; ISV_ERR_INVALID_ARG for a null gate or freq < 1.
 * step takes a frame's stamp: init_feature and first_image_flag skip a frame each; a stamp more than 1 s after the last one, or before
 * it, skips the frame, sets first_image_flag, last_image_time = 0 and pub_count = 1 -- and resets no tracker; otherwise
 * pub_this_frame = round(pub_count / (t - first_image_time)) <= FREQ, with the window restarted when the rate is within 0.01 FREQ of
 * FREQ; a published frame counts, and the first one is not delivered (init_pub). */
int  isv_fe_gate_init(isv_fe_gate_t *gate, int32_t freq);
int  isv_fe_gate_step(isv_fe_gate_t *gate, double stamp, isv_fe_gate_out_t *out);

#ifdef __cplusplus
}
#endif
#endif /* ISVINS_FRONTEND_H */
