"""Builds and loads tests/native/isv_exr_oracle.c, the serial CPU restatement of include/isvins_exrot.h, into a temporary directory
(gcc -O2 -ffp-contract=off -shared: the same flags as oracle/Makefile), and the Python side of it: `Slots` is a host-side slot store
on which `calibrate_batch` runs one whole call; `last` gives what the last good item left (the kept F and its subset, the
decomposition, the A it built); `quirks_off` switches single quirks off for the CPU controls."""
import atexit
import contextlib
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from isvins_amd import exrot as exr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "isv_exr_oracle.c")
_u8p, _f64p, _i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(C.c_int32)
STRUCTS = (exr.isv_exr_config_t, exr.isv_exr_item_t, exr.isv_exr_result_t)
DOUBLE_POINTS, DOUBLE_TRIANGULATION = 1, 2                     # isvo_exr_set_quirks_off's bits: X1, X4
INT_FIELDS = ("status", "frame_count", "method", "iters", "best_inliers", "negated", "choice", "calibrated")
DOUBLE_FIELDS = ("Rc", "angle_deg", "huber", "singular", "ric")


def _p(a):
    return a.ctypes.data_as(_f64p)


def build(tmpdir, opt="-O2"):
    out = os.path.join(str(tmpdir), f"libisv_exr_oracle{opt}.so")
    subprocess.check_call(["gcc", opt, "-ffp-contract=off", "-std=gnu11", "-Wall", "-Wno-unused-function", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "include"), "-o", out, SRC, "-lm"])
    lib = C.CDLL(out)
    cfgp, itemp = C.POINTER(exr.isv_exr_config_t), C.POINTER(exr.isv_exr_item_t)
    lib.isvo_exr_set_quirks_off.argtypes = [C.c_int]; lib.isvo_exr_set_quirks_off.restype = None
    lib.isvo_exr_sizeof.argtypes = [C.c_int]
    lib.isvo_exr_check_config.argtypes = [cfgp]
    lib.isvo_exr_check.argtypes = [cfgp, itemp, _i32p, _u8p]
    lib.isvo_exr_method.argtypes = [C.c_int]
    lib.isvo_exr_uniform.argtypes = [C.POINTER(C.c_uint64), C.c_uint32]; lib.isvo_exr_uniform.restype = C.c_uint32
    lib.isvo_exr_subsets.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int, _i32p]; lib.isvo_exr_subsets.restype = None
    for name, nargs in (("q_from_R", 2), ("q_to_R", 2), ("inv3", 2), ("imu_rows", 4), ("row", 6)):
        f = getattr(lib, "isvo_exr_" + name); f.argtypes = [_f64p] * nargs; f.restype = None
    lib.isvo_exr_calibrated.argtypes = [C.c_int, C.c_int, _f64p]
    lib.isvo_exr_decompose.argtypes = [_f64p] * 4
    lib.isvo_exr_choose.argtypes = [_i32p, C.c_int]
    lib.isvo_exr_front_count.argtypes = [_f64p, _f64p, C.c_double, C.c_int, _f64p]
    lib.isvo_exr_solve.argtypes = [C.c_int, _f64p, _f64p, _f64p]; lib.isvo_exr_solve.restype = None
    lib.isvo_exr_calibrate_batch.argtypes = [cfgp, C.c_int, C.POINTER(itemp), C.POINTER(exr.isv_exr_result_t), _i32p, _f64p, _f64p, _u8p]
    lib.isvo_exr_calibrate_batch.restype = None
    lib.isvo_exr_last.argtypes = [_i32p, _i32p, _i32p] + [_f64p] * 5
    lib.isvo_exr_last_A.argtypes = [_f64p]; lib.isvo_exr_last_A.restype = None
    lib.isvo_exr_free.argtypes = []; lib.isvo_exr_free.restype = None
    for i, s in enumerate(STRUCTS):
        assert lib.isvo_exr_sizeof(i) == C.sizeof(s), s
    return lib


@functools.lru_cache(maxsize=1)
def load():
    """the restatement, built once per process (its directory goes when the process ends)"""
    d = tempfile.mkdtemp(prefix="isv_exr_oracle_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return build(d)


@contextlib.contextmanager
def quirks_off(lib, mask):
    lib.isvo_exr_set_quirks_off(mask)
    try:
        yield
    finally:
        lib.isvo_exr_set_quirks_off(0)


class Slots:
    """a host-side slot store for the restatement: what a Calibrator of the same configuration holds on the device"""

    def __init__(self, cfg):
        self.cfg = cfg
        self.frame_counts = np.zeros(cfg.max_slots, np.int32)
        self.rics = np.tile(np.eye(3).reshape(9), (cfg.max_slots, 1))
        self.hists = np.zeros((cfg.max_slots, cfg.max_frames, exr.HIST))
        self.named = np.zeros(cfg.max_slots, np.uint8)

    def reset(self, slots):
        for s in slots:
            self.frame_counts[s] = 0
            self.rics[s] = np.eye(3).reshape(9)

    def load_slot(self, slot, state):
        """sets a slot to what a read_slot returned"""
        fc, ric, hist = state
        self.frame_counts[slot] = fc
        self.rics[slot] = np.asarray(ric).reshape(9)
        self.hists[slot, :fc] = np.asarray(hist).reshape(fc, exr.HIST)

    def read_slot(self, slot):
        """as Calibrator.read_slot"""
        fc = int(self.frame_counts[slot])
        return fc, self.rics[slot].reshape(3, 3).copy(), self.hists[slot, :fc].reshape(-1, 3, 3, 3).copy()

    def state_bytes(self, slot):
        fc, ric, hist = self.read_slot(slot)
        return fc, ric.tobytes(), hist.tobytes()


def calibrate_batch(lib, slots, items):
    """the restatement's isv_exr_calibrate_batch on a Slots store: ExrItem list -> isv_exr_result_t list"""
    n = len(items)
    res = (exr.isv_exr_result_t * max(n, 1))()
    ptrs = (C.POINTER(exr.isv_exr_item_t) * max(n, 1))(*[C.pointer(it.c) for it in items])
    lib.isvo_exr_calibrate_batch(C.byref(slots.cfg), n, ptrs, res, slots.frame_counts.ctypes.data_as(_i32p), _p(slots.rics), _p(slots.hists),
                                 slots.named.ctypes.data_as(_u8p))
    assert not slots.named.any()
    return list(res)[:n]


class Last:
    """what the last good item of the last call left (valid for an item of >= 9 correspondences that kept a model)"""


def last(lib):
    o = Last()
    ki, nk, sub = C.c_int32(), C.c_int32(), np.zeros(7, np.int32)
    o.F, o.R1, o.R2, o.t, det = np.zeros(9), np.zeros(9), np.zeros(9), np.zeros(3), C.c_double()
    rows = lib.isvo_exr_last(C.byref(ki), C.byref(nk), sub.ctypes.data_as(_i32p), _p(o.F), _p(o.R1), _p(o.R2), _p(o.t), C.byref(det))
    o.keep_iter, o.n_keeps, o.subset, o.det_first = ki.value, nk.value, sub, det.value
    o.F, o.R1, o.R2 = o.F.reshape(3, 3), o.R1.reshape(3, 3), o.R2.reshape(3, 3)
    o.A = np.zeros((rows, 4))
    lib.isvo_exr_last_A(_p(o.A))
    return o


def key_of(r):
    """everything a result is compared on exactly: the integer fields, front[], and the doubles' bits"""
    return (tuple(getattr(r, f) for f in INT_FIELDS) + tuple(r.front) +
            tuple(np.array(getattr(r, f), np.float64).tobytes() for f in DOUBLE_FIELDS))


def doubles_of(r):
    return np.concatenate([np.atleast_1d(np.array(getattr(r, f), np.float64)).reshape(-1) for f in DOUBLE_FIELDS])


# ---- the pieces ----
def q_from_R(lib, R):
    q = np.zeros(4); lib.isvo_exr_q_from_R(_p(np.ascontiguousarray(R, np.float64)), _p(q)); return q


def q_to_R(lib, q):
    R = np.zeros(9); lib.isvo_exr_q_to_R(_p(np.ascontiguousarray(q, np.float64)), _p(R)); return R.reshape(3, 3)


def inv3(lib, M):
    o = np.zeros(9); lib.isvo_exr_inv3(_p(np.ascontiguousarray(M, np.float64)), _p(o)); return o.reshape(3, 3)


def imu_rows(lib, ric, dq):
    a, b = np.zeros(9), np.zeros(9)
    lib.isvo_exr_imu_rows(_p(np.ascontiguousarray(ric, np.float64)), _p(np.ascontiguousarray(dq, np.float64)), _p(a), _p(b))
    return a.reshape(3, 3), b.reshape(3, 3)


def row(lib, Rc, Rimu, Rc_g):
    """(angle in degrees, huber, the 4 x 4 block)"""
    ang, hub, blk = C.c_double(), C.c_double(), np.zeros(16)
    lib.isvo_exr_row(_p(np.ascontiguousarray(Rc, np.float64)), _p(np.ascontiguousarray(Rimu, np.float64)), _p(np.ascontiguousarray(Rc_g, np.float64)),
                     C.cast(C.byref(ang), _f64p), C.cast(C.byref(hub), _f64p), _p(blk))
    return ang.value, hub.value, blk.reshape(4, 4)


def solve(lib, A):
    """(singular [4], ric [3][3]) of A [rows][4]"""
    a = np.array(A, np.float64).reshape(-1, 4).copy()
    s, ric = np.zeros(4), np.zeros(9)
    lib.isvo_exr_solve(len(a), _p(a), _p(s), _p(ric))
    return s, ric.reshape(3, 3)


def build_A(lib, hist):
    """the A the code builds from a slot's history [F][3][3][3]"""
    return np.concatenate([row(lib, h[0], h[1], h[2])[2] for h in hist]) if len(hist) else np.zeros((0, 4))


def subsets(lib, count, n_sub, state=(1 << 64) - 1):
    s = C.c_uint64(state)
    out = np.zeros((n_sub, 7), np.int32)
    lib.isvo_exr_subsets(C.byref(s), count, n_sub, out.ctypes.data_as(_i32p))
    return out, s.value
