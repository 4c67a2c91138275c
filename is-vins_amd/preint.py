"""Host-side mirror of include/isvins_preint.h: the batched IMU pre-integration, IntegrationBase's constructor, push_back and
repropagate (reference include/factor/integration_base.h:13-158), processIMU's propagation of the newest frame (src/estimator.cpp:91-124)
and slideWindow's MARGIN_SECOND_NEW merge (:1660-1675) for many IntegrationBase objects in one call.  `PreIntegrator(...)` raises when
the HIP extension is missing or there is no GPU: no CPU path.  An IntegrationBase object (its record, acc_0 / gyr_0, its sample buffer)
stays on the device in a slot; the caller maps (sequence, frame) to slots.  `push`, `repropagate` and `merge` make the items."""
import ctypes as C

import numpy as np

from . import _stage, abi

ISV_PRE_OK, ISV_PRE_CAPACITY, ISV_PRE_INPUT, ISV_PRE_UNSET = range(4)
PUSH, REPROPAGATE, MERGE = range(3)
MAX_SLOTS, MAX_SAMPLES, MAX_ITEMS = 1048576, 4096, 65536

_f64p = C.POINTER(C.c_double)
isv_imu_t = abi.isv_imu_t


class isv_pre_config_t(C.Structure):
    _fields_ = [("max_slots", C.c_int32), ("max_samples", C.c_int32), ("max_items", C.c_int32), ("pad", C.c_int32),
                ("acc_n", C.c_double), ("gyr_n", C.c_double), ("acc_w", C.c_double), ("gyr_w", C.c_double), ("gravity", C.c_double * 3)]


class isv_pre_nav_t(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("P", C.c_double * 3), ("V", C.c_double * 3), ("Ba", C.c_double * 3), ("Bg", C.c_double * 3)]


class isv_pre_item_t(C.Structure):
    _fields_ = [("op", C.c_int32), ("slot", C.c_int32), ("src_slot", C.c_int32), ("reset", C.c_int32), ("n_samples", C.c_int32), ("want_record", C.c_int32),
                ("dt", _f64p), ("acc", _f64p), ("gyr", _f64p), ("acc_0", C.c_double * 3), ("gyr_0", C.c_double * 3), ("ba", C.c_double * 3), ("bg", C.c_double * 3),
                ("nav", C.POINTER(isv_pre_nav_t)), ("record", C.POINTER(isv_imu_t))]


class isv_pre_result_t(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_buffered", C.c_int32), ("sum_dt", C.c_double), ("delta_p", C.c_double * 3), ("delta_q", C.c_double * 4),
                ("delta_v", C.c_double * 3), ("R", C.c_double * 9), ("P", C.c_double * 3), ("V", C.c_double * 3)]


EXPORTS = ["isv_pre_create", "isv_pre_destroy", "isv_pre_last_error", "isv_pre_last_ms", "isv_pre_run_batch"]


def make_config(max_slots=1, max_samples=64, max_items=256, acc_n=0.08, gyr_n=0.004, acc_w=0.00004, gyr_w=2.0e-6, gravity=(0.0, 0.0, 9.81)):
    c = isv_pre_config_t()
    c.max_slots, c.max_samples, c.max_items = max_slots, max_samples, max_items
    c.acc_n, c.gyr_n, c.acc_w, c.gyr_w = acc_n, gyr_n, acc_w, gyr_w
    c.gravity[:] = [float(v) for v in gravity]
    return c


class PreItem:
    """one operation on a slot: the arrays it points to are kept alive here behind an isv_pre_item_t (`.c`); `.record` is the
    isv_imu_t a good item with want_record fills, else None"""

    def __init__(self, op, slot, want_record=False):
        c = self.c = isv_pre_item_t()
        c.op, c.slot, c.src_slot, c.want_record = op, slot, -1, 1 if want_record else 0
        self.record = isv_imu_t() if want_record else None
        if want_record:
            c.record = C.pointer(self.record)


def _v3(dst, v):
    dst[:] = [float(x) for x in np.asarray(v, float).reshape(3)]


def push(slot, dt=(), acc=(), gyr=(), reset=False, acc_0=(0, 0, 0), gyr_0=(0, 0, 0), ba=(0, 0, 0), bg=(0, 0, 0), nav=None, want_record=False):
    """push_back of the samples dt [n], acc [n][3], gyr [n][3] on `slot`; with `reset` the slot is first constructed from acc_0,
    gyr_0, ba, bg.  nav = (R [3][3], P, V, Ba, Bg): processIMU's propagation runs beside every sample."""
    it = PreItem(PUSH, slot, want_record)
    it.dt = np.ascontiguousarray(dt, np.float64).reshape(-1)
    it.acc = np.ascontiguousarray(acc, np.float64).reshape(-1, 3)
    it.gyr = np.ascontiguousarray(gyr, np.float64).reshape(-1, 3)
    assert len(it.dt) == len(it.acc) == len(it.gyr)
    c = it.c
    c.reset, c.n_samples = 1 if reset else 0, len(it.dt)
    if len(it.dt):
        c.dt, c.acc, c.gyr = it.dt.ctypes.data_as(_f64p), it.acc.ctypes.data_as(_f64p), it.gyr.ctypes.data_as(_f64p)
    _v3(c.acc_0, acc_0); _v3(c.gyr_0, gyr_0); _v3(c.ba, ba); _v3(c.bg, bg)
    if nav is not None:
        R, P, V, Ba, Bg = nav
        it.nav = isv_pre_nav_t()
        it.nav.R[:] = [float(x) for x in np.asarray(R, float).reshape(9)]
        _v3(it.nav.P, P); _v3(it.nav.V, V); _v3(it.nav.Ba, Ba); _v3(it.nav.Bg, Bg)
        c.nav = C.pointer(it.nav)
    return it


def repropagate(slot, ba, bg, want_record=False):
    """IntegrationBase::repropagate(ba, bg) on `slot`"""
    it = PreItem(REPROPAGATE, slot, want_record)
    _v3(it.c.ba, ba); _v3(it.c.bg, bg)
    return it


def merge(slot, src_slot, want_record=False):
    """push_back on `slot` of every buffered sample of `src_slot` (slideWindow, MARGIN_SECOND_NEW)"""
    it = PreItem(MERGE, slot, want_record)
    it.c.src_slot = src_slot
    return it


@_stage.bind_once("pre")
def _bind(lib):
    vp = C.c_void_p
    lib.isv_pre_create.argtypes = [C.POINTER(isv_pre_config_t), C.POINTER(vp)]
    lib.isv_pre_destroy.argtypes = [vp]; lib.isv_pre_destroy.restype = None
    lib.isv_pre_last_error.argtypes = [vp]; lib.isv_pre_last_error.restype = C.c_char_p
    lib.isv_pre_last_ms.argtypes = [vp, _f64p]
    lib.isv_pre_run_batch.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(isv_pre_item_t)), C.POINTER(isv_pre_result_t)]


def run_on(call, handle, items):
    """`call`(handle, n, items, results) of the entry point's signature on PreItem list -> (results, records): records[i] is the
    isv_imu_t of a good item with want_record, else None"""
    n = len(items)
    res = (isv_pre_result_t * max(n, 1))()
    ptrs = (C.POINTER(isv_pre_item_t) * max(n, 1))(*[C.pointer(it.c) for it in items])
    rc = call(handle, n, ptrs, res)
    res = list(res)[:n]
    return rc, res, [it.record if r.status == ISV_PRE_OK else None for it, r in zip(items, res)]


class PreIntegrator(_stage.StageHandle):
    """IMU pre-integration on the MI355X: many IntegrationBase objects per call, each in a slot"""
    PREFIX, N_MS = "isv_pre", 3

    def __init__(self, max_slots, **kw):
        self.cfg = make_config(max_slots, **kw)
        self._create(_bind, C.byref(self.cfg), why=" (a MI355X and the HIP extension are required; there is no CPU path)")

    def run_batch(self, items):
        """items: PreItem list -> (isv_pre_result_t list, records)"""
        rc, res, recs = run_on(self.lib.isv_pre_run_batch, self.h, items)
        self._check(rc, "isv_pre_run_batch", with_last_error=True)
        return res, recs

    def last_ms(self):
        """(whole call, k_pre_integrate, upload) milliseconds of the last successful call that launched"""
        return super().last_ms()
