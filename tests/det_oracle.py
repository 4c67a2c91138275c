"""Builds and loads tests/native/isv_det_oracle.c, the serial CPU restatement of include/isvins_detect.h, into a temporary directory
(gcc -O2 -ffp-contract=off -shared: the same flags as oracle/Makefile), and the Python side of it: `detect` runs one item on one
image, `reference` runs the scenario list once per (min_dist, camera) per process and is shared, unchanged, by the tests that need it."""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from isvins_amd import detect as det, tracker as trk

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "isv_det_oracle.c")
_u8p, _f32p, _i32p, _i64p = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
COUNTERS = ("dropped", "clipped", "candidates", "rejected", "cap_reached", "tie_pairs", "plateau", "masked")


def build(tmpdir, opt="-O2"):
    out = os.path.join(str(tmpdir), f"libisv_det_oracle{opt}.so")
    subprocess.check_call(["gcc", opt, "-ffp-contract=off", "-std=gnu11", "-Wall", "-Wno-unused-function", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "include"), "-o", out, SRC, "-lm"])
    lib = C.CDLL(out)
    lib.isvo_det_sizeof.argtypes = [C.c_int]
    lib.isvo_det_disc.argtypes = [_u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.isvo_det_sums.argtypes = [_u8p, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p]; lib.isvo_det_sums.restype = None
    lib.isvo_det_response.argtypes = [_u8p, C.c_int, C.c_int, C.c_int, _f32p]; lib.isvo_det_response.restype = None
    lib.isvo_det_lift.argtypes = [C.POINTER(trk.isv_trk_config_t), C.c_float, C.c_float, _f32p]; lib.isvo_det_lift.restype = None
    lib.isvo_det_detect.argtypes = [C.POINTER(det.isv_det_config_t), C.POINTER(trk.isv_trk_config_t), _u8p, C.c_int, C.c_int, C.c_int,
                                    C.POINTER(det.isv_det_item_t), C.POINTER(det.isv_det_result_t), _i32p, _f32p, _f32p, _f32p, _u8p, _i64p]
    lib.isvo_det_detect.restype = None
    for i, s in enumerate((det.isv_det_config_t, det.isv_det_item_t, det.isv_det_result_t)):
        assert lib.isvo_det_sizeof(i) == C.sizeof(s), s
    return lib


@functools.lru_cache(maxsize=1)
def load():
    """the restatement, built once per process (its directory goes when the process ends)"""
    d = tempfile.mkdtemp(prefix="isv_det_oracle_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return build(d)


def disc(lib, w, h, cx, cy, r):
    """(mask [h][w] with the disc set to 0 on 255, clipped)"""
    m = np.full((h, w), 255, np.uint8)
    clipped = lib.isvo_det_disc(m.ctypes.data_as(_u8p), w, h, cx, cy, r)
    return m, bool(clipped)


def sums(lib, img, width=None):
    """(Dx, Dy, Sxx, Sxy, Syy), int32 [h][width] each"""
    img = np.ascontiguousarray(img, np.uint8)
    h, stride = img.shape
    w = stride if width is None else width
    out = [np.zeros((h, w), np.int32) for _ in range(5)]
    lib.isvo_det_sums(img.ctypes.data_as(_u8p), w, h, stride, *[o.ctypes.data_as(_i32p) for o in out])
    return out


def response(lib, img, width=None):
    img = np.ascontiguousarray(img, np.uint8)
    h, stride = img.shape
    w = stride if width is None else width
    out = np.zeros((h, w), np.float32)
    lib.isvo_det_response(img.ctypes.data_as(_u8p), w, h, stride, out.ctypes.data_as(_f32p))
    return out


class Detected:
    """what the restatement gives for one item: the result record, DetArrays, the response plane (None when max_new is 0 or the item
    is refused), the mask plane (None for a refused item), the counters by name"""

    def __init__(self, r, arrays, eig, mask, counters):
        self.r, self.arrays, self.eig, self.mask, self.counters = r, arrays, eig, mask, counters


def detect(lib, cfg, cam, image, item, width=None):
    """the restatement on one item; image [h][stride] uint8, or None (an empty slot)"""
    r = det.isv_det_result_t()
    if image is None:
        img, h, stride, w = None, 0, 0, 0
    else:
        img = np.ascontiguousarray(image, np.uint8)
        h, stride = img.shape
        w = stride if width is None else width
    cap = min(max(item.c.max_new, 0), cfg.max_corners)
    ki = det.filled(item.c.n_points, 1, np.int32).reshape(-1)
    nw, un = det.filled(cap, 2, np.float32), det.filled(cap, 2, np.float32)
    eig, mask = np.zeros((max(h, 1), max(w, 1)), np.float32), np.zeros((max(h, 1), max(w, 1)), np.uint8)
    cnt = np.zeros(8, np.int64)
    lib.isvo_det_detect(C.byref(cfg), C.byref(cam), None if img is None else img.ctypes.data_as(_u8p), w, h, stride, C.byref(item.c), C.byref(r),
                        ki.ctypes.data_as(_i32p), nw.ctypes.data_as(_f32p), un.ctypes.data_as(_f32p), eig.ctypes.data_as(_f32p), mask.ctypes.data_as(_u8p),
                        cnt.ctypes.data_as(_i64p))
    ok = r.status == det.ISV_DET_OK
    k, m = (r.n_kept, r.n_new) if ok else (0, 0)
    assert det.untouched(ki, k) and det.untouched(nw, m) and det.untouched(un, m)
    return Detected(r, det.DetArrays(ki[:k], nw[:m], un[:m]), eig if ok and item.c.max_new > 0 else None, mask if ok else None,
                    dict(zip(COUNTERS, cnt.tolist())))


def uncapped(lib, cfg, cam, image, item, width=None):
    """the item with no cap on the corners"""
    big = det.make_config(cfg.max_items, cfg.max_points, 65535, cfg.min_dist, cfg.quality_level)
    it = det.DetItem(item.c.slot, item.points, item.track_cnt, 65535)
    return detect(lib, big, cam, image, it, width)


@functools.lru_cache(maxsize=8)
def reference(min_dist=30, distorted=True):
    """the restatement over det_cases.scenarios(), computed once and shared: (det cfg, trk cfg, scenarios, items, [Detected]).  An
    item whose max_new is EXACT gets the uncapped count of its image at this min_dist (1 if that is 0)."""
    import det_cases
    lib = load()
    cfg, cam, scen = det_cases.det_config(min_dist), det_cases.trk_config(distorted), det_cases.scenarios()
    items, out = [], []
    for s in scen:
        it = s["item"]
        if s["max_new"] == det_cases.EXACT:
            it = det.DetItem(it.c.slot, it.points, it.track_cnt, max(uncapped(lib, cfg, cam, s["image"], it, s["width"]).r.n_new, 1))
        items.append(it)
        out.append(detect(lib, cfg, cam, s["image"], it, s["width"]))
    return cfg, cam, scen, items, out


def describe(r):
    return dict(status=r.status, n_points=r.n_points, n_kept=r.n_kept, n_new=r.n_new, n_candidates=r.n_candidates, max_val=r.max_val)
