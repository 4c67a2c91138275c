"""Host-side mirror of include/isvins_frontend.h: the whole-frame feature tracker, FeatureTracker::readImage (reference
src/feature_tracker/feature_tracker_simple.cpp:81-151) and the message of System::PubImageData (src/System.cpp:102-129) for many
sequences in one call.  A `FrontEnd` is bound to a `tracker.Tracker`, a `reject.Rejector`, a `detect.Detector` and, optionally, an
`equalize.Equalizer` on it; a sequence's whole state lives in its slot on the device.  `gate_step` is PubImageData's scalar logic
(which frames publish) and needs no GPU."""
import ctypes as C

import numpy as np

from . import _stage, backend
from ._stage import FILL
from .tracker import ISV_TRK_OK

_u8p, _f32p, _i32p, _f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
FREQ = 10                                            # config/euroc_config.yaml


class isv_fe_config_t(C.Structure):
    _fields_ = [("max_items", C.c_int32), ("max_cnt", C.c_int32), ("max_points", C.c_int32), ("_pad", C.c_int32)]


class isv_fe_item_t(C.Structure):
    _fields_ = [("slot", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("cur", _u8p), ("cur_time", C.c_double),
                ("pub_this_frame", C.c_int32), ("_pad", C.c_int32)]


class isv_fe_result_t(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_tracked", C.c_int32), ("n_after_reject", C.c_int32), ("n_kept", C.c_int32), ("n_new", C.c_int32),
                ("n_points", C.c_int32), ("n_msg", C.c_int32), ("method", C.c_int32), ("iters", C.c_int32), ("_pad", C.c_int32)]


class isv_fe_state_t(C.Structure):
    _fields_ = [("has_sequence", C.c_int32), ("n_points", C.c_int32), ("n_id", C.c_int32), ("_pad", C.c_int32), ("prev_time", C.c_double)]


class isv_fe_gate_t(C.Structure):
    _fields_ = [("init_feature", C.c_int32), ("first_image_flag", C.c_int32), ("init_pub", C.c_int32), ("pub_count", C.c_int32),
                ("first_image_time", C.c_double), ("last_image_time", C.c_double), ("freq", C.c_int32), ("_pad", C.c_int32)]


class isv_fe_gate_out_t(C.Structure):
    _fields_ = [("skip", C.c_int32), ("pub_this_frame", C.c_int32), ("deliver", C.c_int32), ("_pad", C.c_int32)]


EXPORTS = ["isv_fe_create", "isv_fe_destroy", "isv_fe_last_error", "isv_fe_read_image_batch", "isv_fe_last_ms", "isv_fe_slot_get", "isv_fe_slot_set",
           "isv_fe_slot_reset", "isv_fe_gate_init", "isv_fe_gate_step"]
RESULT_FIELDS = ("status", "n_tracked", "n_after_reject", "n_kept", "n_new", "n_points", "n_msg", "method", "iters")


def make_config(max_items=1, max_cnt=150, max_points=256):
    c = isv_fe_config_t()
    c.max_items, c.max_cnt, c.max_points = max_items, max_cnt, max_points
    return c


class FeItem:
    """one sequence's frame: a numpy image [height][stride] uint8 (kept alive here) behind an isv_fe_item_t (`.c`)"""

    def __init__(self, slot, cur, cur_time, pub_this_frame=1, width=None):
        self.cur = np.ascontiguousarray(cur, dtype=np.uint8)
        assert self.cur.ndim == 2
        c = self.c = isv_fe_item_t()
        c.slot = slot
        c.height, c.stride = self.cur.shape
        c.width = c.stride if width is None else width
        c.cur = self.cur.ctypes.data_as(_u8p)
        c.cur_time, c.pub_this_frame = cur_time, int(pub_this_frame)

    def on_slot(self, slot):
        it = FeItem(slot, self.cur, self.c.cur_time, self.c.pub_this_frame, self.c.width)
        it.c.stride, it.c.height = self.c.stride, self.c.height
        return it


class Frame:
    """an item's outputs.  The message: feature_id [n_msg] int32, point [n_msg][3] float64, uv [n_msg][2], velocity [n_msg][2] float32;
    the end-of-frame lists: cur_pts, cur_un_pts [n][2] float32, ids, track_cnt [n] int32, pts_velocity [n][2] float32 (all empty for a
    refused item)"""
    ARRAYS = ("feature_id", "point", "uv", "velocity", "cur_pts", "cur_un_pts", "ids", "track_cnt", "pts_velocity")

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def message(self):
        """(feature_id, point): what estimator push_image takes"""
        return self.feature_id, self.point


class State:
    """a slot's feature state (isv_fe_slot_get / isv_fe_slot_set): has_sequence, n_id, prev_time and prev_pts [n][2] float32, ids [n],
    track_cnt [n] int32, prev_un_pts [n][2] float32, in_map [n] uint8"""
    ARRAYS = ("prev_pts", "ids", "track_cnt", "prev_un_pts", "in_map")

    def __init__(self, prev_pts=None, ids=None, track_cnt=None, prev_un_pts=None, in_map=None, n_id=0, prev_time=0.0, has_sequence=1):
        self.prev_pts = np.ascontiguousarray(np.zeros((0, 2)) if prev_pts is None else prev_pts, dtype=np.float32).reshape(-1, 2)
        n = len(self.prev_pts)
        self.ids = np.ascontiguousarray(np.full(n, -1) if ids is None else ids, dtype=np.int32).reshape(-1)
        self.track_cnt = np.ascontiguousarray(np.ones(n) if track_cnt is None else track_cnt, dtype=np.int32).reshape(-1)
        self.prev_un_pts = np.ascontiguousarray(np.zeros((n, 2)) if prev_un_pts is None else prev_un_pts, dtype=np.float32).reshape(-1, 2)
        self.in_map = np.ascontiguousarray(np.zeros(n) if in_map is None else in_map, dtype=np.uint8).reshape(-1)
        self.n_id, self.prev_time, self.has_sequence = int(n_id), float(prev_time), int(has_sequence)

    def key(self):
        """everything, as bytes, for bitwise comparisons"""
        return (self.has_sequence, self.n_id, np.float64(self.prev_time).tobytes()) + tuple(getattr(self, a).tobytes() for a in self.ARRAYS)


@_stage.bind_once("fe")
def _bind(lib):
    vp = C.c_void_p
    pp = lambda t: C.POINTER(t)
    lib.isv_fe_create.argtypes = [vp, vp, vp, vp, C.POINTER(isv_fe_config_t), C.POINTER(vp)]
    lib.isv_fe_destroy.argtypes = [vp]; lib.isv_fe_destroy.restype = None
    lib.isv_fe_last_error.argtypes = [vp]; lib.isv_fe_last_error.restype = C.c_char_p
    lib.isv_fe_read_image_batch.argtypes = [vp, C.c_int32, pp(pp(isv_fe_item_t)), pp(isv_fe_result_t), pp(_i32p), pp(_f64p), pp(_f32p), pp(_f32p), pp(_f32p),
                                            pp(_f32p), pp(_i32p), pp(_i32p), pp(_f32p)]
    lib.isv_fe_last_ms.argtypes = [vp, C.POINTER(C.c_double)]
    lib.isv_fe_slot_get.argtypes = [vp, C.c_int32, pp(isv_fe_state_t), _f32p, _i32p, _i32p, _f32p, _u8p]
    lib.isv_fe_slot_set.argtypes = [vp, C.c_int32, pp(isv_fe_state_t), _f32p, _i32p, _i32p, _f32p, _u8p]
    lib.isv_fe_slot_reset.argtypes = [vp, C.c_int32]
    lib.isv_fe_gate_init.argtypes = [pp(isv_fe_gate_t), C.c_int32]
    lib.isv_fe_gate_step.argtypes = [pp(isv_fe_gate_t), C.c_double, pp(isv_fe_gate_out_t)]


class Gate:
    """System::PubImageData's scalar state: `step(stamp)` -> (skip, pub_this_frame, deliver).  No GPU."""

    def __init__(self, freq=FREQ):
        self.lib = backend.load_library()
        _bind(self.lib)
        self.g = isv_fe_gate_t()
        if self.lib.isv_fe_gate_init(C.byref(self.g), freq) != 0:
            raise backend.BackendError("isv_fe_gate_init: ISV_ERR_INVALID_ARG")

    def step(self, stamp):
        out = isv_fe_gate_out_t()
        if self.lib.isv_fe_gate_step(C.byref(self.g), stamp, C.byref(out)) != 0:
            raise backend.BackendError("isv_fe_gate_step: ISV_ERR_INVALID_ARG")
        return bool(out.skip), bool(out.pub_this_frame), bool(out.deliver)


def gate_step(gate, stamp):
    return gate.step(stamp)


class FrontEnd(_stage.StageHandle):
    """readImage on the MI355X: many sequences per call, one slot per sequence, the state on the device.  Close it before its stages."""
    PREFIX, N_MS = "isv_fe", 6
    _SHAPES = dict(feature_id=(1, np.int32, _i32p), point=(3, np.float64, _f64p), uv=(2, np.float32, _f32p), velocity=(2, np.float32, _f32p),
                   cur_pts=(2, np.float32, _f32p), cur_un_pts=(2, np.float32, _f32p), ids=(1, np.int32, _i32p), track_cnt=(1, np.int32, _i32p),
                   pts_velocity=(2, np.float32, _f32p))

    def __init__(self, tracker, rejector, detector, equalizer=None, max_items=None, max_cnt=None, max_points=None):
        self.tracker, self.rejector, self.detector, self.equalizer = tracker, rejector, detector, equalizer      # kept alive
        stages = [tracker, rejector, detector] + ([equalizer] if equalizer is not None else [])
        self.cfg = make_config(min(s.cfg.max_items for s in stages) if max_items is None else max_items,
                               detector.cfg.max_corners if max_cnt is None else max_cnt,
                               min(tracker.cfg.max_points, rejector.cfg.max_points, detector.cfg.max_points) if max_points is None else max_points)
        self._create(_bind, tracker.h, equalizer.h if equalizer is not None else None, rejector.h, detector.h, C.byref(self.cfg))

    def read_image_batch(self, items, lists=True):
        """items: FeItem list -> (isv_fe_result_t list, Frame list).  The arrays are pre-filled with FILL bytes; what lies beyond an
        item's counts, and all of a refused item's arrays, is checked to be untouched."""
        n, P = len(items), self.cfg.max_points
        res = (isv_fe_result_t * max(n, 1))()
        ptrs = (C.POINTER(isv_fe_item_t) * max(n, 1))(*[C.pointer(it.c) for it in items])
        # one pre-filled block [n][max_points] per output, and the items' pointers into it
        bufs, args, keep = {}, [], []
        for name in Frame.ARRAYS:
            cols, dtype, pt = self._SHAPES[name]
            if not lists and name in Frame.ARRAYS[4:]:
                bufs[name] = None; args.append(None)
                continue
            row = cols * np.dtype(dtype).itemsize
            bufs[name] = np.full((max(n, 1), P, row), FILL, np.uint8)
            addr = np.ascontiguousarray(np.uint64(bufs[name].ctypes.data) + np.arange(max(n, 1), dtype=np.uint64) * np.uint64(P * row))
            keep.append(addr)
            args.append(C.cast((C.c_uint64 * max(n, 1)).from_buffer(addr), C.POINTER(pt)))
        rc = self.lib.isv_fe_read_image_batch(self.h, n, ptrs, res, *args)
        self._check(rc, "isv_fe_read_image_batch", with_last_error=True)
        out = list(res)[:n]
        used = np.array([[r.n_msg, r.n_points] if r.status == ISV_TRK_OK else [0, 0] for r in out], np.int64).reshape(-1, 2)
        beyond = [np.arange(P)[None, :] >= used[:, k, None] for k in (0, 1)]
        frames = [dict() for _ in out]
        for j, name in enumerate(Frame.ARRAYS):
            cols, dtype, _ = self._SHAPES[name]
            if bufs[name] is None:
                for kw in frames:
                    kw[name] = None
                continue
            assert n == 0 or (bufs[name][:n][beyond[int(j >= 4)]] == FILL).all(), "written past an item's counts, or into a refused item's arrays"
            typed = bufs[name].view(dtype)
            for i, kw in enumerate(frames):
                a = typed[i, :int(used[i, int(j >= 4)])]
                kw[name] = a.reshape(-1) if cols == 1 else a
        return out, [Frame(**kw) for kw in frames]

    def slot_get(self, slot):
        P = self.cfg.max_points
        st = isv_fe_state_t()
        a = State(np.zeros((P, 2)), np.zeros(P), np.zeros(P), np.zeros((P, 2)), np.zeros(P))
        rc = self.lib.isv_fe_slot_get(self.h, slot, C.byref(st), a.prev_pts.ctypes.data_as(_f32p), a.ids.ctypes.data_as(_i32p), a.track_cnt.ctypes.data_as(_i32p),
                                      a.prev_un_pts.ctypes.data_as(_f32p), a.in_map.ctypes.data_as(_u8p))
        self._check(rc, "isv_fe_slot_get", with_last_error=True)
        n = st.n_points
        return State(a.prev_pts[:n], a.ids[:n], a.track_cnt[:n], a.prev_un_pts[:n], a.in_map[:n], st.n_id, st.prev_time, st.has_sequence)

    def slot_set(self, slot, state):
        st = isv_fe_state_t()
        st.has_sequence, st.n_points, st.n_id, st.prev_time = state.has_sequence, len(state.prev_pts), state.n_id, state.prev_time
        rc = self.lib.isv_fe_slot_set(self.h, slot, C.byref(st), state.prev_pts.ctypes.data_as(_f32p), state.ids.ctypes.data_as(_i32p),
                                      state.track_cnt.ctypes.data_as(_i32p), state.prev_un_pts.ctypes.data_as(_f32p), state.in_map.ctypes.data_as(_u8p))
        self._check(rc, "isv_fe_slot_set", with_last_error=True)

    def slot_reset(self, slot):
        self._check(self.lib.isv_fe_slot_reset(self.h, slot), "isv_fe_slot_reset")

    def last_ms(self):
        """(whole call, the level-0 / CLAHE and pyramid kernels, the flow and its compaction, rejectWithF and setMask's order, the
        detection and the end of the frame, the upload) milliseconds of the last successful call"""
        return super().last_ms()
