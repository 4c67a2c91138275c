/*
 * isvins_preint.h -- C ABI of the batched IMU PRE-INTEGRATION:
 *   IntegrationBase::IntegrationBase, push_back, propagate, midPointIntegration, repropagate
 *                                          include/factor/integration_base.h:13-158
 *   Estimator::processIMU                  src/estimator.cpp:91-124 (with its propagation of the newest frame's Rs / Ps / Vs)
 *   slideWindow's MARGIN_SECOND_NEW merge  src/estimator.cpp:1660-1675
 * for many IntegrationBase objects in one call (MI355X).  A pre-integrator is a handle of its own, with its own stream.
 *
 * A SLOT is one IntegrationBase object on the device: its isv_imu_t record (delta_p / q / v, the linearised biases, sum_dt, the 15 x 15
 * jacobian and covariance), acc_0 / gyr_0, linearized_acc / linearized_gyr, a constructed flag and its sample buffer (dt_buf, acc_buf,
 * gyr_buf).  The records of all slots are ONE device array of isv_imu_t indexed by slot, the buffers one array of
 * [max_slots][max_samples][7] doubles (dt, acc, gyr per sample).  A caller maps (sequence, frame) to slots itself: slideWindow's
 * std::swap of two pre-integrations is a swap of two integers on the caller's side and needs no call.
 *
 * An item is one of three operations on its `slot`:
 *   ISV_PRE_PUSH         with `reset` the slot is first constructed from the item's acc_0, gyr_0, ba, bg (new IntegrationBase: deltas
 *                        zero, delta_q identity, jacobian identity, covariance zero, sum_dt 0, an empty buffer, linearized_acc / gyr =
 *                        acc_0 / gyr_0); then push_back(dt[i], acc[i], gyr[i]) for i = 0 .. n_samples - 1, each sample appended to the
 *                        slot's buffer.  n_samples = 0 with reset is a bare constructor call, without reset a no-op that reads the
 *                        slot.  With `nav` the propagation of processIMU (estimator.cpp:109-122) runs beside every sample, from
 *                        nav's R, P, V with its Ba, Bg and the handle's gravity, reading acc_0 / gyr_0 as they stand before the
 *                        sample; the result returns R, P, V.
 *   ISV_PRE_REPROPAGATE  repropagate(ba, bg): the record is re-zeroed as the constructor leaves it, acc_0 / gyr_0 =
 *                        linearized_acc / gyr, the linearised biases become ba, bg, and push_back runs again over the slot's own
 *                        buffer, which is unchanged.
 *   ISV_PRE_MERGE        push_back on `slot` of every buffered sample of `src_slot`, in order, each appended to `slot`'s buffer
 *                        (pre_integrations[frame_count - 1]->push_back(tmp_dt, tmp_linear_acceleration, tmp_angular_velocity) over
 *                        dt_buf[frame_count]); src_slot is only read.
 * The arithmetic is the window manager's host code (PreIntegration::push_back and processIMU's propagation in
 * is-vins_amd/csrc/isv_estimator.cpp), operation for operation, stated once in is-vins_amd/csrc/isv_preint.h for the kernel and for
 * the CPU restatement tests/native/isv_pre_oracle.c; contraction is off on both sides and FP64 division and sqrt are correctly rounded
 * on both, so the kernel, the restatement and the host code give the same bits.
 *
 * Deviations (documented, not quirks):
 *   the buffer cap: the reference's dt_buf / acc_buf / gyr_buf are unbounded; a slot holds max_samples samples, and an item that would
 *   exceed them is refused (ISV_PRE_CAPACITY), never truncated.
 *   the statuses: the reference has no checks; an item is refused by its result's status as below.
 */
#ifndef ISVINS_PREINT_H
#define ISVINS_PREINT_H

#include <stddef.h>
#include <stdint.h>
#include "isvins_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISV_PRE_MAX_SLOTS 1048576
#define ISV_PRE_MAX_SAMPLES 4096
#define ISV_PRE_MAX_ITEMS 65536

#define ISV_PRE_PUSH 0
#define ISV_PRE_REPROPAGATE 1
#define ISV_PRE_MERGE 2

typedef enum isv_pre_status {
    ISV_PRE_OK = 0,
    ISV_PRE_CAPACITY = 1,         /* n_samples > max_samples (the call's staging holds max_samples per item), or the slot's buffer
                                     would exceed max_samples                                                                       */
    ISV_PRE_INPUT = 2,            /* an unknown op; a slot outside [0, max_slots); n_samples < 0; a slot named as `slot` by an earlier
                                     item of the same call (a refused one too); a MERGE whose src_slot is outside [0, max_slots), equals
                                     its slot, or is the `slot` of any other item of the same call; null dt / acc / gyr with
                                     n_samples > 0; want_record without a record; a non-finite number                               */
    ISV_PRE_UNSET = 3             /* the slot was never constructed: PUSH without reset, REPROPAGATE, MERGE (slot or src_slot)      */
} isv_pre_status_t;

typedef struct isv_pre_config {
    int32_t max_slots;            /* IntegrationBase objects resident at once, 1 .. ISV_PRE_MAX_SLOTS                              */
    int32_t max_samples;          /* samples a slot's buffer holds, 1 .. ISV_PRE_MAX_SAMPLES                                       */
    int32_t max_items;            /* items per call, 1 .. ISV_PRE_MAX_ITEMS                                                        */
    int32_t pad;
    double  acc_n, gyr_n, acc_w, gyr_w;   /* ACC_N, GYR_N, ACC_W, GYR_W: finite, not negative                                      */
    double  gravity[3];           /* G, subtracted in the nav propagation                                                          */
} isv_pre_config_t;

typedef struct isv_pre_nav {      /* the newest frame's state before the item's first sample                                       */
    double R[9];                  /* Rs[frame_count], row-major */
    double P[3], V[3], Ba[3], Bg[3];
} isv_pre_nav_t;

typedef struct isv_pre_item {
    int32_t op;                   /* ISV_PRE_PUSH / ISV_PRE_REPROPAGATE / ISV_PRE_MERGE                                            */
    int32_t slot;
    int32_t src_slot;             /* MERGE                                                                                         */
    int32_t reset;                /* PUSH: construct the slot first                                                                */
    int32_t n_samples;            /* PUSH                                                                                          */
    int32_t want_record;          /* copy the slot's record, as the item leaves it, into *record                                   */
    const double *dt;             /* PUSH: [n_samples]                                                                             */
    const double *acc;            /* PUSH: [n_samples][3]                                                                          */
    const double *gyr;            /* PUSH: [n_samples][3]                                                                          */
    double  acc_0[3], gyr_0[3];   /* PUSH with reset                                                                               */
    double  ba[3], bg[3];         /* PUSH with reset, REPROPAGATE                                                                  */
    const isv_pre_nav_t *nav;     /* PUSH, optional                                                                                */
    isv_imu_t *record;            /* out, with want_record; untouched by a refused item                                            */
} isv_pre_item_t;

typedef struct isv_pre_result {
    int32_t status;               /* isv_pre_status_t                                                                              */
    int32_t n_buffered;           /* the slot's buffered samples after the call (unchanged by a refused item); -1: no such slot, or
                                     the slot is not constructed                                                                   */
    double  sum_dt;
    double  delta_p[3];
    double  delta_q[4];           /* x y z w, as isv_imu_t                                                                         */
    double  delta_v[3];
    double  R[9], P[3], V[3];     /* the nav state after the item's last sample; zero without nav                                  */
} isv_pre_result_t;

typedef struct isv_pre isv_pre_t;

/* A pre-integrator on the current device, no slot constructed.  ISV_ERR_INVALID_ARG for a null argument or a value outside its range
 * above (before the device is touched); ISV_ERR_DEVICE without a GPU, or when the slots' store (max_slots * (3840 + 56 * max_samples)
 * bytes) cannot be allocated: there is no CPU path. */
int  isv_pre_create(const isv_pre_config_t *cfg, isv_pre_t **out);
void isv_pre_destroy(isv_pre_t *h);
const char *isv_pre_last_error(const isv_pre_t *h);

/* milliseconds of the last successful isv_pre_run_batch that launched: the whole call (host clock), k_pre_integrate and the upload
 * (HIP events) */
int  isv_pre_last_ms(isv_pre_t *h, double out_ms[3]);

/* items[0..n), results [n]; ISV_ERR_INVALID_ARG for n > max_items.  One packed upload (the item headers and the PUSH items' samples),
 * k_pre_integrate (one wavefront per good item; REPROPAGATE and MERGE read the slots' buffers in device memory), one download of the
 * result records and of the records asked for by want_record, synchronous on the handle's stream.  Every check that can refuse an item
 * runs on the host before anything is launched.  An item is refused by its result's status, never truncated; a refused item leaves
 * every slot it names untouched, its result zero apart from status and n_buffered, and does not stop the batch.  A call without a good
 * item launches nothing.  A result, and the slot behind it, does not depend, bit for bit, on the batch it ran in.  The call returns
 * ISV_OK whenever it ran. */
int  isv_pre_run_batch(isv_pre_t *h, int32_t n, const isv_pre_item_t *const *items, isv_pre_result_t *results);

#ifdef __cplusplus
}
#endif
#endif /* ISVINS_PREINT_H */
