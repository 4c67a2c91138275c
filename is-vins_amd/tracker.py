"""Host-side mirror of include/isvins_tracker.h: the batched feature tracking, the per-image part of FeatureTracker::readImage
(reference src/feature_tracker/feature_tracker_simple.cpp:114-118, :197-208: cv::calcOpticalFlowPyrLK with a 21 x 21 window and 3
levels down, inBorder, liftProjective of every tracked point) for many sequences in one call.  `Tracker(...)` raises when the HIP
extension is missing or there is no GPU: no CPU path.  A sequence's state, the pyramid of its last image, stays on the device in a
slot; `kept` does the reference's reduceVector.

`analytic_image` samples a smooth analytic texture at shifted coordinates, for the tests and scripts/trk_bench.py."""
import ctypes as C

import numpy as np

from . import _stage
from ._stage import FILL, filled, untouched
from .keyframe import EUROC

ISV_TRK_OK, ISV_TRK_CAPACITY, ISV_TRK_INPUT = range(3)
WIN, MAX_LEVEL, MAX_ITER = 21, 3, 30
FLAG_STATUS, FLAG_BORDER = 1, 2

_u8p, _f32p, _i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32)


class isv_trk_config_t(C.Structure):
    _fields_ = [("max_slots", C.c_int32), ("max_items", C.c_int32), ("max_width", C.c_int32), ("max_height", C.c_int32), ("max_points", C.c_int32),
                ("win", C.c_int32), ("max_level", C.c_int32), ("_pad", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double)]


class isv_trk_item_t(C.Structure):
    _fields_ = [("slot", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("n_points", C.c_int32), ("_pad", C.c_int32),
                ("cur", _u8p), ("prev", _u8p), ("prev_pts", _f32p)]


class isv_trk_result_t(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_points", C.c_int32), ("n_kept", C.c_int32), ("n_levels", C.c_int32)]


EXPORTS = ["isv_trk_create", "isv_trk_destroy", "isv_trk_last_error", "isv_trk_track_batch", "isv_trk_last_ms", "isv_trk_slot_reset"]


def make_config(max_slots=1, max_items=1, max_width=752, max_height=480, max_points=256, win=WIN, max_level=MAX_LEVEL,
                fx=EUROC["fx"], fy=EUROC["fy"], cx=EUROC["cx"], cy=EUROC["cy"], k1=EUROC["k1"], k2=EUROC["k2"], p1=EUROC["p1"], p2=EUROC["p2"]):
    """the reference's constants as defaults (feature_tracker_simple.cpp:114, config/euroc_config.yaml)"""
    c = isv_trk_config_t()
    c.max_slots, c.max_items, c.max_width, c.max_height, c.max_points, c.win, c.max_level = max_slots, max_items, max_width, max_height, max_points, win, max_level
    c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2 = fx, fy, cx, cy, k1, k2, p1, p2
    return c


def levels(width, height):
    """the sizes [(w, h)] of the pyramid levels of a width x height image"""
    out = [(width, height)]
    while len(out) <= MAX_LEVEL:
        w, h = (out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2
        if w <= WIN or h <= WIN:
            break
        out.append((w, h))
    return out


class TrkItem:
    """one sequence's frame: numpy arrays (kept alive here) behind an isv_trk_item_t (`.c`).  `cur` and `prev` are [height][stride]
    uint8 (`prev` None: the slot's resident image); `width` defaults to the arrays'; `points` [n][2] float32 in prev."""

    def __init__(self, slot, cur, prev=None, points=None, width=None):
        self.cur = np.ascontiguousarray(cur, dtype=np.uint8)
        self.prev = None if prev is None else np.ascontiguousarray(prev, dtype=np.uint8)
        assert self.cur.ndim == 2 and (self.prev is None or self.prev.shape == self.cur.shape)
        self.points = np.ascontiguousarray(np.zeros((0, 2)) if points is None else points, dtype=np.float32).reshape(-1, 2)
        c = self.c = isv_trk_item_t()
        c.slot = slot
        c.height, c.stride = self.cur.shape
        c.width = c.stride if width is None else width
        c.n_points = len(self.points)
        c.cur = self.cur.ctypes.data_as(_u8p)
        c.prev = None if self.prev is None else self.prev.ctypes.data_as(_u8p)
        c.prev_pts = self.points.ctypes.data_as(_f32p)

    def with_prev(self, prev, slot=None):
        """the same frame with another prev (None: resident) and, optionally, another slot"""
        it = TrkItem(self.c.slot if slot is None else slot, self.cur, prev, self.points, self.c.width)
        it.c.stride, it.c.height, it.c.n_points = self.c.stride, self.c.height, self.c.n_points
        return it


class TrkArrays:
    """an item's output arrays: cur_pts [n][2] float32, flags [n] uint8, err [n] float32, cur_un_pts [n][2] float32 (empty for a
    refused item)"""

    def __init__(self, cur_pts, flags, err, cur_un_pts):
        self.cur_pts, self.flags, self.err, self.cur_un_pts = cur_pts, flags, err, cur_un_pts

    def kept(self, *others):
        """reduceVector: (cur_pts, cur_un_pts, *others) cut to the points the reference keeps (both flag bits set); `others` are
        per-point arrays of the caller (prev_pts, ids, track_cnt)"""
        m = self.flags == (FLAG_STATUS | FLAG_BORDER)
        return (self.cur_pts[m], self.cur_un_pts[m]) + tuple(np.asarray(o)[m] for o in others)


@_stage.bind_once("trk")
def _bind(lib):
    vp = C.c_void_p
    lib.isv_trk_create.argtypes = [C.POINTER(isv_trk_config_t), C.POINTER(vp)]
    lib.isv_trk_destroy.argtypes = [vp]; lib.isv_trk_destroy.restype = None
    lib.isv_trk_last_error.argtypes = [vp]; lib.isv_trk_last_error.restype = C.c_char_p
    lib.isv_trk_track_batch.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(isv_trk_item_t)), C.POINTER(isv_trk_result_t), C.POINTER(_f32p),
                                        C.POINTER(_u8p), C.POINTER(_f32p), C.POINTER(_f32p)]
    lib.isv_trk_last_ms.argtypes = [vp, C.POINTER(C.c_double)]
    lib.isv_trk_slot_reset.argtypes = [vp, C.c_int32]
    lib.isv_internal_trk_read_level.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, _u8p, _i32p, _i32p]


class Tracker(_stage.StageHandle):
    """FeatureTracker::readImage's optical flow on the MI355X: many sequences per call, one slot per sequence"""
    PREFIX, N_MS = "isv_trk", 5

    def __init__(self, max_slots=1, max_items=None, max_width=752, max_height=480, **kw):
        self.cfg = make_config(max_slots, max_slots if max_items is None else max_items, max_width, max_height, **kw)
        self._create(_bind, C.byref(self.cfg), why=" (a MI355X and the HIP extension are required; there is no CPU path)")

    def track_batch(self, items):
        """items: TrkItem list -> (isv_trk_result_t list, TrkArrays list).  The arrays are pre-filled with FILL bytes; a refused item's
        are checked to be untouched and come back empty."""
        n = len(items)
        res = (isv_trk_result_t * max(n, 1))()
        ptrs = (C.POINTER(isv_trk_item_t) * max(n, 1))(*[C.pointer(it.c) for it in items])
        nps = [it.c.n_points for it in items]
        cp = [filled(c, 2, np.float32) for c in nps]
        un = [filled(c, 2, np.float32) for c in nps]
        er = [filled(c, 1, np.float32).reshape(-1) for c in nps]
        fl = [filled(c, 1, np.uint8).reshape(-1) for c in nps]
        arr = lambda t, xs: (t * max(n, 1))(*[a.ctypes.data_as(t) for a in xs])
        rc = self.lib.isv_trk_track_batch(self.h, n, ptrs, res, arr(_f32p, cp), arr(_u8p, fl), arr(_f32p, er), arr(_f32p, un))
        self._check(rc, "isv_trk_track_batch", with_last_error=True)
        out = list(res)[:n]
        arrays = []
        for i, r in enumerate(out):
            p = r.n_points if r.status == ISV_TRK_OK else 0
            for a in (cp[i], un[i], er[i], fl[i]):
                assert untouched(a, p), "written past an item's points, or into a refused item's arrays"
            arrays.append(TrkArrays(cp[i][:p], fl[i][:p], er[i][:p], un[i][:p]))
        return out, arrays

    def slot_reset(self, slot):
        self._check(self.lib.isv_trk_slot_reset(self.h, slot), "isv_trk_slot_reset")

    def read_level(self, slot, level, which=0):
        """one pyramid level of a slot (debug entry, csrc/isv_tracker.h): which = 0 the resident pyramid (the last cur image's),
        1 the last prev image's"""
        w, h = C.c_int32(), C.c_int32()
        self._check(self.lib.isv_internal_trk_read_level(self.h, slot, which, level, None, C.byref(w), C.byref(h)), "isv_internal_trk_read_level")
        out = np.zeros((h.value, w.value), np.uint8)
        self._check(self.lib.isv_internal_trk_read_level(self.h, slot, which, level, out.ctypes.data_as(_u8p), None, None), "isv_internal_trk_read_level")
        return out

    def last_ms(self):
        """(whole call, the pyramid kernels, k_trk_track, the upload, the host's packing) milliseconds of the last successful call"""
        return super().last_ms()


# ---------------------------------------------------------------------------------------------------------------------
def analytic_image(width, height, shift=(0.0, 0.0), seed=0, waves=12, contrast=100.0):
    """A smooth analytic texture sampled on the pixel grid shifted by `shift`: pixel (x, y) shows the texture at (x - sx, y - sy), so a
    point of the texture at p in the image with shift 0 is at p + shift here.  A sum of `waves` plane waves with wavelengths of 9 to
    60 pixels and fixed pseudo-random directions and phases, in doubles, rounded to uint8."""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    lam = rng.uniform(9.0, 60.0, waves)
    ang = rng.uniform(0.0, 2.0 * np.pi, waves)
    ph = rng.uniform(0.0, 2.0 * np.pi, waves)
    amp = rng.uniform(0.5, 1.0, waves)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    xx, yy = xx - shift[0], yy - shift[1]
    v = sum(a * np.sin(2.0 * np.pi / l * (np.cos(t) * xx + np.sin(t) * yy) + p) for a, l, t, p in zip(amp, lam, ang, ph))
    return np.clip(np.rint(128.0 + contrast * v / amp.sum()), 0, 255).astype(np.uint8)
