"""Host-side mirror of include/isvins_equalize.h: the batched CLAHE, the first line of FeatureTracker::readImage with EQUALIZE set
(reference src/feature_tracker/feature_tracker_simple.cpp:86-92: cv::createCLAHE(3.0, cv::Size(8, 8))->apply) for many sequences
in one call.  An `Equalizer` is bound to a `tracker.Tracker`: `track_batch` is the tracker's call with every uploaded image equalised
on the device before it becomes level 0 of its slot's pyramid, `apply_batch` returns equalised images and touches no slot."""
import ctypes as C

import numpy as np

from . import _stage
from ._stage import filled, untouched
from .tracker import ISV_TRK_OK, TrkArrays, isv_trk_item_t, isv_trk_result_t

CLIP, TILES, MAX_TILES = 3.0, 8, 32                  # feature_tracker_simple.cpp:88

_u8p, _f32p, _i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32)


class isv_eq_config_t(C.Structure):
    _fields_ = [("clip_limit", C.c_double), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32), ("max_items", C.c_int32), ("_pad", C.c_int32)]


class isv_eq_image_t(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("_pad", C.c_int32), ("data", _u8p)]


EXPORTS = ["isv_eq_create", "isv_eq_destroy", "isv_eq_last_error", "isv_eq_track_batch", "isv_eq_apply_batch", "isv_eq_last_ms"]


def make_config(clip_limit=CLIP, tiles_x=TILES, tiles_y=TILES, max_items=1):
    """the reference's constants as defaults"""
    c = isv_eq_config_t()
    c.clip_limit, c.tiles_x, c.tiles_y, c.max_items = clip_limit, tiles_x, tiles_y, max_items
    return c


class EqImage:
    """one image for apply_batch: a numpy array [height][stride] uint8 (kept alive here) behind an isv_eq_image_t (`.c`); `width`
    defaults to the array's"""

    def __init__(self, image, width=None):
        self.image = np.ascontiguousarray(image, dtype=np.uint8)
        assert self.image.ndim == 2
        c = self.c = isv_eq_image_t()
        c.height, c.stride = self.image.shape
        c.width = c.stride if width is None else width
        c.data = self.image.ctypes.data_as(_u8p)


@_stage.bind_once("eq")
def _bind(lib):
    vp = C.c_void_p
    lib.isv_eq_create.argtypes = [vp, C.POINTER(isv_eq_config_t), C.POINTER(vp)]
    lib.isv_eq_destroy.argtypes = [vp]; lib.isv_eq_destroy.restype = None
    lib.isv_eq_last_error.argtypes = [vp]; lib.isv_eq_last_error.restype = C.c_char_p
    lib.isv_eq_track_batch.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(isv_trk_item_t)), C.POINTER(isv_trk_result_t), C.POINTER(_f32p),
                                       C.POINTER(_u8p), C.POINTER(_f32p), C.POINTER(_f32p)]
    lib.isv_eq_apply_batch.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(isv_eq_image_t)), _i32p, C.POINTER(_u8p)]
    lib.isv_eq_last_ms.argtypes = [vp, C.POINTER(C.c_double)]
    lib.isv_internal_eq_read_luts.argtypes = [vp, C.c_int32, C.c_int32, _u8p, _i32p, _i32p]


class Equalizer(_stage.StageHandle):
    """CLAHE on the MI355X, on the slots of a tracker.Tracker: many sequences per call.  Close it before its tracker."""
    PREFIX, N_MS = "isv_eq", 6

    def __init__(self, tracker, max_items=None, **kw):
        self.tracker = tracker                     # kept alive: the equaliser uses its slots, stream and limits
        self.cfg = make_config(max_items=tracker.cfg.max_items if max_items is None else max_items, **kw)
        self._create(_bind, tracker.h, C.byref(self.cfg))

    def track_batch(self, items):
        """tracker.Tracker.track_batch on the equalised images: TrkItem list -> (isv_trk_result_t list, TrkArrays list)"""
        n = len(items)
        res = (isv_trk_result_t * max(n, 1))()
        ptrs = (C.POINTER(isv_trk_item_t) * max(n, 1))(*[C.pointer(it.c) for it in items])
        nps = [it.c.n_points for it in items]
        cp = [filled(c, 2, np.float32) for c in nps]
        un = [filled(c, 2, np.float32) for c in nps]
        er = [filled(c, 1, np.float32).reshape(-1) for c in nps]
        fl = [filled(c, 1, np.uint8).reshape(-1) for c in nps]
        arr = lambda t, xs: (t * max(n, 1))(*[a.ctypes.data_as(t) for a in xs])
        rc = self.lib.isv_eq_track_batch(self.h, n, ptrs, res, arr(_f32p, cp), arr(_u8p, fl), arr(_f32p, er), arr(_f32p, un))
        self._check(rc, "isv_eq_track_batch", with_last_error=True)
        out = list(res)[:n]
        arrays = []
        for i, r in enumerate(out):
            p = r.n_points if r.status == ISV_TRK_OK else 0
            for a in (cp[i], un[i], er[i], fl[i]):
                assert untouched(a, p), "written past an item's points, or into a refused item's arrays"
            arrays.append(TrkArrays(cp[i][:p], fl[i][:p], er[i][:p], un[i][:p]))
        return out, arrays

    def apply_batch(self, items):
        """items: EqImage list -> (status list, image list): [height][width] uint8 per good item, None for a refused one, whose
        pre-filled array is checked to be untouched"""
        n = len(items)
        status = (C.c_int32 * max(n, 1))()
        ptrs = (C.POINTER(isv_eq_image_t) * max(n, 1))(*[C.pointer(it.c) for it in items])
        outs = [filled(max(it.c.height, 0), max(it.c.width, 1), np.uint8) for it in items]
        rc = self.lib.isv_eq_apply_batch(self.h, n, ptrs, status, (_u8p * max(n, 1))(*[a.ctypes.data_as(_u8p) for a in outs]))
        self._check(rc, "isv_eq_apply_batch", with_last_error=True)
        st, images = list(status)[:n], []
        for s, a, it in zip(st, outs, items):
            if s == ISV_TRK_OK:
                images.append(a[:it.c.height])
            else:
                assert untouched(a, 0), "written into a refused item's array"
                images.append(None)
        return st, images

    def read_luts(self, item, which=0):
        """the tiles' LUTs of item `item` of the last call (debug entry, csrc/isv_equalize.h) -> [tiles_y][tiles_x][256] uint8; after
        track_batch which = 0 is the item's cur image, 1 its uploaded prev"""
        tx, ty = C.c_int32(), C.c_int32()
        self._check(self.lib.isv_internal_eq_read_luts(self.h, item, which, None, C.byref(tx), C.byref(ty)), "isv_internal_eq_read_luts")
        out = np.zeros((ty.value, tx.value, 256), np.uint8)
        self._check(self.lib.isv_internal_eq_read_luts(self.h, item, which, out.ctypes.data_as(_u8p), None, None), "isv_internal_eq_read_luts")
        return out

    def last_ms(self):
        """(whole call, the CLAHE kernels, the pyramid kernels, k_trk_track, the upload, the host's packing) milliseconds of the last
        successful call"""
        return super().last_ms()
