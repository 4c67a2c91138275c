"""Host-side mirror of include/isvins_exrot.h: the batched camera-IMU rotation calibration, InitialEXRotation::CalibrationExRotation
(reference src/initial/initial_ex_rotation.cpp, called from Estimator::processImage, src/estimator.cpp:139-153, with
estimate_extrinsic: 2) for many sequences in one call.  `Calibrator(...)` raises when the HIP extension is missing or there is no GPU:
no CPU path.  A sequence's state (frame_count, ric, the recorded Rc / Rimu / Rc_g) stays on the device in a slot.  One item per frame
per sequence until a result says `calibrated`; the solve handle is then created with estimate_extrinsic = 1 and the result's ric."""
import ctypes as C

import numpy as np

from . import _stage

ISV_EXR_OK, ISV_EXR_CAPACITY, ISV_EXR_INPUT, ISV_EXR_NO_MODEL = range(4)
MIN_CORRES, RANSAC_MIN, MAX_CORRES, MAX_FRAMES, VO_SIZE = 9, 15, 4096, 1024, 8
NONE, LMEDS, RANSAC = range(3)
HIST = 27                                  # doubles per recorded frame: Rc, Rimu, Rc_g

_f64p, _i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)


class isv_exr_config_t(C.Structure):
    _fields_ = [("max_slots", C.c_int32), ("max_frames", C.c_int32), ("max_corres", C.c_int32), ("vo_size", C.c_int32)]


class isv_exr_item_t(C.Structure):
    _fields_ = [("slot", C.c_int32), ("n_corres", C.c_int32), ("corres", _f64p), ("delta_q", C.c_double * 4)]


class isv_exr_result_t(C.Structure):
    _fields_ = [("status", C.c_int32), ("frame_count", C.c_int32), ("method", C.c_int32), ("iters", C.c_int32), ("best_inliers", C.c_int32),
                ("negated", C.c_int32), ("front", C.c_int32 * 4), ("choice", C.c_int32), ("calibrated", C.c_int32), ("Rc", C.c_double * 9),
                ("angle_deg", C.c_double), ("huber", C.c_double), ("singular", C.c_double * 4), ("ric", C.c_double * 9)]


EXPORTS = ["isv_exr_create", "isv_exr_destroy", "isv_exr_last_error", "isv_exr_last_ms", "isv_exr_reset", "isv_exr_calibrate_batch", "isv_exr_read_slot"]


def make_config(max_slots=1, max_frames=32, max_corres=256, vo_size=VO_SIZE):
    c = isv_exr_config_t()
    c.max_slots, c.max_frames, c.max_corres, c.vo_size = max_slots, max_frames, max_corres, vo_size
    return c


class ExrItem:
    """one sequence's frame: `corres` [n][4] doubles (first.x, first.y, second.x, second.y of getCorresponding(frame_count - 1,
    frame_count)) and `delta_q` (w, x, y, z), kept alive here behind an isv_exr_item_t (`.c`)"""

    def __init__(self, slot, corres, delta_q):
        self.corres = np.ascontiguousarray(corres, dtype=np.float64).reshape(-1, 4)
        c = self.c = isv_exr_item_t()
        c.slot, c.n_corres = slot, len(self.corres)
        c.corres = self.corres.ctypes.data_as(_f64p)
        c.delta_q[:] = [float(v) for v in delta_q]


@_stage.bind_once("exr")
def _bind(lib):
    vp = C.c_void_p
    lib.isv_exr_create.argtypes = [C.POINTER(isv_exr_config_t), C.POINTER(vp)]
    lib.isv_exr_destroy.argtypes = [vp]; lib.isv_exr_destroy.restype = None
    lib.isv_exr_last_error.argtypes = [vp]; lib.isv_exr_last_error.restype = C.c_char_p
    lib.isv_exr_last_ms.argtypes = [vp, _f64p]
    lib.isv_exr_reset.argtypes = [vp, C.c_int32, _i32p]
    lib.isv_exr_calibrate_batch.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(isv_exr_item_t)), C.POINTER(isv_exr_result_t)]
    lib.isv_exr_read_slot.argtypes = [vp, C.c_int32, _i32p, _f64p, _f64p]


class Calibrator(_stage.StageHandle):
    """CalibrationExRotation on the MI355X: many sequences per call, each in a slot"""
    PREFIX, N_MS = "isv_exr", 2

    def __init__(self, max_slots, **kw):
        self.cfg = make_config(max_slots, **kw)
        self._create(_bind, C.byref(self.cfg), why=" (a MI355X and the HIP extension are required; there is no CPU path)")

    def reset(self, slots):
        """frame_count = 0, ric = I in each slot"""
        a = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        self._check(self.lib.isv_exr_reset(self.h, len(a), a.ctypes.data_as(_i32p)), "isv_exr_reset", with_last_error=True)

    def calibrate_batch(self, items):
        """items: ExrItem list -> isv_exr_result_t list"""
        n = len(items)
        res = (isv_exr_result_t * max(n, 1))()
        ptrs = (C.POINTER(isv_exr_item_t) * max(n, 1))(*[C.pointer(it.c) for it in items])
        self._check(self.lib.isv_exr_calibrate_batch(self.h, n, ptrs, res), "isv_exr_calibrate_batch", with_last_error=True)
        return list(res)[:n]

    def read_slot(self, slot):
        """(frame_count, ric [3][3], history [frame_count][3][3][3] = Rc, Rimu, Rc_g of the frames 1 .. frame_count)"""
        fc = C.c_int32()
        ric = np.zeros(9)
        hist = np.zeros((self.cfg.max_frames, HIST))
        rc = self.lib.isv_exr_read_slot(self.h, slot, C.byref(fc), ric.ctypes.data_as(_f64p), hist.ctypes.data_as(_f64p))
        self._check(rc, "isv_exr_read_slot", with_last_error=True)
        return fc.value, ric.reshape(3, 3), hist[:fc.value].reshape(-1, 3, 3, 3).copy()

    def last_ms(self):
        """(whole call, k_exr_calibrate) milliseconds of the last successful call that launched"""
        return super().last_ms()
