"""Host-side mirror of include/isvins_reject.h: the batched outlier rejection, FeatureTracker::rejectWithF (reference
src/feature_tracker/feature_tracker_simple.cpp:153-180: the lift of prev_pts and cur_pts to the virtual pinhole of FOCAL_LENGTH and
cv::findFundamentalMat(un_prev_pts, un_cur_pts, cv::FM_RANSAC, F_THRESHOLD, 0.99, status)) for many sequences in one call.  A
`Rejector` is bound to a `tracker.Tracker` for its device, stream and camera; it touches no slot.  The order of a published frame is
track -> reduce_vector -> reject -> reduce_vector -> detect."""
import ctypes as C

import numpy as np

from . import _stage
from ._stage import filled, untouched
from .tracker import ISV_TRK_OK

MIN_POINTS, RANSAC_MIN, MAX_POINTS = 8, 15, 4096
NONE, LMEDS, RANSAC = range(3)
FOCAL_LENGTH, F_THRESHOLD = 460.0, 1.0               # parameters.h; config/euroc_config.yaml

_u8p, _f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_float)


class isv_rej_config_t(C.Structure):
    _fields_ = [("max_items", C.c_int32), ("max_points", C.c_int32), ("focal_length", C.c_double), ("f_threshold", C.c_double)]


class isv_rej_item_t(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("n_points", C.c_int32), ("_pad", C.c_int32), ("prev_pts", _f32p), ("cur_pts", _f32p)]


class isv_rej_result_t(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_points", C.c_int32), ("n_kept", C.c_int32), ("method", C.c_int32), ("iters", C.c_int32),
                ("best_inliers", C.c_int32), ("min_median", C.c_double)]


EXPORTS = ["isv_rej_create", "isv_rej_destroy", "isv_rej_last_error", "isv_rej_reject_batch", "isv_rej_last_ms"]


def make_config(max_items=1, max_points=256, focal_length=FOCAL_LENGTH, f_threshold=F_THRESHOLD):
    """the reference's constants as defaults"""
    c = isv_rej_config_t()
    c.max_items, c.max_points, c.focal_length, c.f_threshold = max_items, max_points, focal_length, f_threshold
    return c


class RejItem:
    """one sequence's rejection: numpy arrays (kept alive here) behind an isv_rej_item_t (`.c`).  `prev_pts`, `cur_pts` [n][2] float32
    are the tracker's arrays after the caller's reduce_vector; `width`, `height` are COL, ROW."""

    def __init__(self, width, height, prev_pts, cur_pts):
        self.prev_pts = np.ascontiguousarray(prev_pts, dtype=np.float32).reshape(-1, 2)
        self.cur_pts = np.ascontiguousarray(cur_pts, dtype=np.float32).reshape(-1, 2)
        assert len(self.prev_pts) == len(self.cur_pts)
        c = self.c = isv_rej_item_t()
        c.width, c.height, c.n_points = width, height, len(self.prev_pts)
        c.prev_pts = self.prev_pts.ctypes.data_as(_f32p)
        c.cur_pts = self.cur_pts.ctypes.data_as(_f32p)


def reduce_vector(status, *arrays):
    """the reference's reduceVector (feature_tracker_simple.cpp:14-30) on every array: the entries whose status is non-zero, in order"""
    keep = np.asarray(status).astype(bool)
    out = tuple(np.ascontiguousarray(np.asarray(a)[keep]) for a in arrays)
    return out[0] if len(out) == 1 else out


@_stage.bind_once("rej")
def _bind(lib):
    vp = C.c_void_p
    lib.isv_rej_create.argtypes = [vp, C.POINTER(isv_rej_config_t), C.POINTER(vp)]
    lib.isv_rej_destroy.argtypes = [vp]; lib.isv_rej_destroy.restype = None
    lib.isv_rej_last_error.argtypes = [vp]; lib.isv_rej_last_error.restype = C.c_char_p
    lib.isv_rej_reject_batch.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(isv_rej_item_t)), C.POINTER(isv_rej_result_t), C.POINTER(_u8p)]
    lib.isv_rej_last_ms.argtypes = [vp, C.POINTER(C.c_double)]


class Rejector(_stage.StageHandle):
    """rejectWithF on the MI355X, with the camera of a tracker.Tracker: many sequences per call.  Close it before its tracker."""
    PREFIX, N_MS = "isv_rej", 4

    def __init__(self, tracker, max_items=None, max_points=None, **kw):
        self.tracker = tracker                     # kept alive: the rejector uses its stream and camera
        self.cfg = make_config(tracker.cfg.max_items if max_items is None else max_items,
                               min(MAX_POINTS, tracker.cfg.max_points) if max_points is None else max_points, **kw)
        self._create(_bind, tracker.h, C.byref(self.cfg))

    def reject_batch(self, items):
        """items: RejItem list -> (isv_rej_result_t list, status list): [n_points] uint8 of 1 / 0 per good item, empty for a refused
        one.  The arrays are pre-filled with FILL bytes; what lies beyond an item's points, and all of a refused item's array, is
        checked to be untouched."""
        n = len(items)
        res = (isv_rej_result_t * max(n, 1))()
        ptrs = (C.POINTER(isv_rej_item_t) * max(n, 1))(*[C.pointer(it.c) for it in items])
        st = [filled(it.c.n_points, 1, np.uint8).reshape(-1) for it in items]
        rc = self.lib.isv_rej_reject_batch(self.h, n, ptrs, res, (_u8p * max(n, 1))(*[a.ctypes.data_as(_u8p) for a in st]))
        self._check(rc, "isv_rej_reject_batch", with_last_error=True)
        out = list(res)[:n]
        status = []
        for r, a in zip(out, st):
            p = r.n_points if r.status == ISV_TRK_OK else 0
            assert untouched(a, p), "written past an item's points, or into a refused item's array"
            status.append(a[:p])
        return out, status

    def last_ms(self):
        """(whole call, k_rej_f, the upload, the host's packing) milliseconds of the last successful call"""
        return super().last_ms()
