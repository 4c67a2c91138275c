"""Host-side mirror of include/isvins_detect.h: the batched feature detection, the part of FeatureTracker::readImage that gives
birth to tracks (reference src/feature_tracker/feature_tracker_simple.cpp:37-69, :126-143: setMask and cv::goodFeaturesToTrack with
MAX_CNT, 0.01 and MIN_DIST, and the lift of every new corner) for many sequences in one call.  A `Detector` is bound to a
`tracker.Tracker`: the image it works on is a slot's resident image, so nothing but the surviving points is uploaded.  The first
frame of a sequence: seed the slot with `TrkItem(slot, img, img)`, then detect with no points."""
import ctypes as C

import numpy as np

from . import _stage
from ._stage import filled, untouched

ISV_DET_OK, ISV_DET_CAPACITY, ISV_DET_INPUT = range(3)
BLOCK_SIZE, APERTURE, USE_HARRIS = 3, 3, 0
MAX_CNT, MIN_DIST, QUALITY = 150, 30, 0.01           # config/euroc_config.yaml; feature_tracker_simple.cpp:134

_f32p, _i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)


class isv_det_config_t(C.Structure):
    _fields_ = [("max_items", C.c_int32), ("max_points", C.c_int32), ("max_corners", C.c_int32), ("min_dist", C.c_int32), ("quality_level", C.c_double)]


class isv_det_item_t(C.Structure):
    _fields_ = [("slot", C.c_int32), ("n_points", C.c_int32), ("max_new", C.c_int32), ("_pad", C.c_int32), ("cur_pts", _f32p), ("track_cnt", _i32p)]


class isv_det_result_t(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_points", C.c_int32), ("n_kept", C.c_int32), ("n_new", C.c_int32), ("n_candidates", C.c_int32),
                ("max_val", C.c_float)]


EXPORTS = ["isv_det_create", "isv_det_destroy", "isv_det_last_error", "isv_det_detect_batch", "isv_det_last_ms"]


def make_config(max_items=1, max_points=256, max_corners=MAX_CNT, min_dist=MIN_DIST, quality_level=QUALITY):
    """the reference's constants as defaults"""
    c = isv_det_config_t()
    c.max_items, c.max_points, c.max_corners, c.min_dist, c.quality_level = max_items, max_points, max_corners, min_dist, quality_level
    return c


class DetItem:
    """one sequence's detection: numpy arrays (kept alive here) behind an isv_det_item_t (`.c`).  `points` [n][2] float32 are cur_pts
    after the caller's reduceVector, `track_cnt` [n] int32 theirs; `max_new` is MAX_CNT - n as the reference computes it."""

    def __init__(self, slot, points=None, track_cnt=None, max_new=0):
        self.points = np.ascontiguousarray(np.zeros((0, 2)) if points is None else points, dtype=np.float32).reshape(-1, 2)
        n = len(self.points)
        self.track_cnt = np.ascontiguousarray(np.ones(n) if track_cnt is None else track_cnt, dtype=np.int32).reshape(-1)
        assert len(self.track_cnt) == n
        c = self.c = isv_det_item_t()
        c.slot, c.n_points, c.max_new = slot, n, max_new
        c.cur_pts = self.points.ctypes.data_as(_f32p)
        c.track_cnt = self.track_cnt.ctypes.data_as(_i32p)

    def on_slot(self, slot):
        """the same detection on another slot"""
        it = DetItem(slot, self.points, self.track_cnt, self.c.max_new)
        it.c.n_points = self.c.n_points
        return it


class DetArrays:
    """an item's output arrays: kept_index [n_kept] int32 (input indices in setMask's order), new_pts [n_new][2] float32, new_un_pts
    [n_new][2] float32 (all empty for a refused item)"""

    def __init__(self, kept_index, new_pts, new_un_pts):
        self.kept_index, self.new_pts, self.new_un_pts = kept_index, new_pts, new_un_pts


@_stage.bind_once("det")
def _bind(lib):
    vp = C.c_void_p
    lib.isv_det_create.argtypes = [vp, C.POINTER(isv_det_config_t), C.POINTER(vp)]
    lib.isv_det_destroy.argtypes = [vp]; lib.isv_det_destroy.restype = None
    lib.isv_det_last_error.argtypes = [vp]; lib.isv_det_last_error.restype = C.c_char_p
    lib.isv_det_detect_batch.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(isv_det_item_t)), C.POINTER(isv_det_result_t), C.POINTER(_i32p),
                                         C.POINTER(_f32p), C.POINTER(_f32p)]
    lib.isv_det_last_ms.argtypes = [vp, C.POINTER(C.c_double)]
    lib.isv_internal_det_read_plane.argtypes = [vp, C.c_int32, C.c_int32, vp, _i32p, _i32p, _i32p]


class Detector(_stage.StageHandle):
    """setMask + goodFeaturesToTrack on the MI355X, on the slots of a tracker.Tracker: many sequences per call.  Close it before
    its tracker."""
    PREFIX, N_MS = "isv_det", 5

    def __init__(self, tracker, max_items=None, **kw):
        self.tracker = tracker                     # kept alive: the detector uses its slots, stream and camera
        self.cfg = make_config(tracker.cfg.max_items if max_items is None else max_items, **kw)
        self._create(_bind, tracker.h, C.byref(self.cfg))

    def detect_batch(self, items):
        """items: DetItem list -> (isv_det_result_t list, DetArrays list).  The arrays are pre-filled with FILL bytes; what lies
        beyond an item's counts, and all of a refused item's arrays, is checked to be untouched."""
        n = len(items)
        res = (isv_det_result_t * max(n, 1))()
        ptrs = (C.POINTER(isv_det_item_t) * max(n, 1))(*[C.pointer(it.c) for it in items])
        cap = self.cfg.max_corners
        ki = [filled(it.c.n_points, 1, np.int32).reshape(-1) for it in items]
        nw = [filled(min(max(it.c.max_new, 0), cap), 2, np.float32) for it in items]
        un = [filled(min(max(it.c.max_new, 0), cap), 2, np.float32) for it in items]
        arr = lambda t, xs: (t * max(n, 1))(*[a.ctypes.data_as(t) for a in xs])
        rc = self.lib.isv_det_detect_batch(self.h, n, ptrs, res, arr(_i32p, ki), arr(_f32p, nw), arr(_f32p, un))
        self._check(rc, "isv_det_detect_batch", with_last_error=True)
        out = list(res)[:n]
        arrays = []
        for i, r in enumerate(out):
            ok = r.status == ISV_DET_OK
            k, m = (r.n_kept, r.n_new) if ok else (0, 0)
            assert untouched(ki[i], k) and untouched(nw[i], m) and untouched(un[i], m), "written past an item's counts, or into a refused item's arrays"
            arrays.append(DetArrays(ki[i][:k], nw[i][:m], un[i][:m]))
        return out, arrays

    def read_plane(self, item, which):
        """a plane of item `item` of the last call (debug entry, csrc/isv_detect.h): which = 0 the response (float32), 1 the mask
        (uint8) -> (plane [height][width], n_candidates)"""
        w, h, nc = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.lib.isv_internal_det_read_plane(self.h, item, which, None, C.byref(w), C.byref(h), C.byref(nc)), "isv_internal_det_read_plane")
        out = np.zeros((h.value, w.value), np.float32 if which == 0 else np.uint8)
        self._check(self.lib.isv_internal_det_read_plane(self.h, item, which, out.ctypes.data_as(C.c_void_p), None, None, None), "isv_internal_det_read_plane")
        return out, nc.value

    def last_ms(self):
        """(whole call, k_det_eig, k_det_mask, k_det_cand + k_det_select, upload + download) milliseconds of the last successful call"""
        return super().last_ms()
