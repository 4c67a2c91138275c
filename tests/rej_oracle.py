"""Builds and loads tests/native/isv_rej_oracle.c, the serial CPU restatement of include/isvins_reject.h, into a temporary directory
(gcc -O2 -ffp-contract=off -shared: the same flags as oracle/Makefile), and the Python side of it: `reject` runs rejectWithF on one
item and returns the result record, the status array and the iterations at which a model was kept; `quirks_off` switches single
quirks off for the CPU controls."""
import atexit
import contextlib
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from isvins_amd import reject as rej, tracker as trk

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "isv_rej_oracle.c")
_u8p, _f32p, _i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32)
STRUCTS = (rej.isv_rej_config_t, rej.isv_rej_item_t, rej.isv_rej_result_t)
DOUBLE_POINTS, DOUBLE_ERROR, RANSAC_BELOW_15, FLOAT_SORT = 1, 2, 4, 8          # isvo_rej_set_quirks_off's bits: J1, J2, J3, J4
FIELDS = ("status", "n_points", "n_kept", "method", "iters", "best_inliers")


def build(tmpdir, opt="-O2"):
    out = os.path.join(str(tmpdir), f"libisv_rej_oracle{opt}.so")
    subprocess.check_call(["gcc", opt, "-ffp-contract=off", "-std=gnu11", "-Wall", "-Wno-unused-function", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "include"), "-o", out, SRC, "-lm"])
    lib = C.CDLL(out)
    cfgp, tcfgp, itemp = C.POINTER(rej.isv_rej_config_t), C.POINTER(trk.isv_trk_config_t), C.POINTER(rej.isv_rej_item_t)
    lib.isvo_rej_set_quirks_off.argtypes = [C.c_int]; lib.isvo_rej_set_quirks_off.restype = None
    lib.isvo_rej_sizeof.argtypes = [C.c_int]
    lib.isvo_rej_check_config.argtypes = [cfgp, C.c_int]
    lib.isvo_rej_check.argtypes = [cfgp, itemp, C.c_int]
    lib.isvo_rej_lift.argtypes = [tcfgp, cfgp, C.c_int, C.c_int, C.c_int, _f32p, _f32p]; lib.isvo_rej_lift.restype = None
    lib.isvo_rej_lmeds_niters.argtypes = []
    lib.isvo_rej_sigma.argtypes = [C.c_int, C.c_double]; lib.isvo_rej_sigma.restype = C.c_double
    lib.isvo_rej_uniform.argtypes = [C.POINTER(C.c_uint64), C.c_uint32]; lib.isvo_rej_uniform.restype = C.c_uint32
    lib.isvo_rej_subsets.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int, _i32p]; lib.isvo_rej_subsets.restype = None
    lib.isvo_rej_median.argtypes = [_f32p, C.c_int]; lib.isvo_rej_median.restype = C.c_double
    lib.isvo_rej_reject.argtypes = [tcfgp, cfgp, itemp, C.POINTER(rej.isv_rej_result_t), _u8p]
    lib.isvo_rej_last_keeps.argtypes = [_i32p, C.c_int]
    for i, s in enumerate(STRUCTS):
        assert lib.isvo_rej_sizeof(i) == C.sizeof(s), s
    return lib


@functools.lru_cache(maxsize=1)
def load():
    """the restatement, built once per process (its directory goes when the process ends)"""
    d = tempfile.mkdtemp(prefix="isv_rej_oracle_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return build(d)


@contextlib.contextmanager
def quirks_off(lib, mask):
    lib.isvo_rej_set_quirks_off(mask)
    try:
        yield
    finally:
        lib.isvo_rej_set_quirks_off(0)


class Rejected:
    """what the restatement gives for one item: res (isv_rej_result_t), status [n_points] uint8 (empty for a refused item), keeps (the
    iterations at which a model was kept, in order)"""

    def __init__(self, res, status, keeps):
        self.res, self.status, self.keeps = res, status, keeps

    def key(self):
        """everything the GPU is compared on: the integer fields, min_median's bits, the status bytes"""
        return tuple(getattr(self.res, f) for f in FIELDS) + (np.float64(self.res.min_median).tobytes(), self.status.tobytes())


def key_of(res, status):
    return tuple(getattr(res, f) for f in FIELDS) + (np.float64(res.min_median).tobytes(), np.asarray(status, np.uint8).tobytes())


def reject(lib, tcfg, cfg, item):
    """the restatement on one RejItem"""
    res = rej.isv_rej_result_t()
    st = np.zeros(max(item.c.n_points, 1), np.uint8)
    lib.isvo_rej_reject(C.byref(tcfg), C.byref(cfg), C.byref(item.c), C.byref(res), st.ctypes.data_as(_u8p))
    keeps = (C.c_int32 * 64)()
    nk = lib.isvo_rej_last_keeps(keeps, 64) if res.status == 0 and res.method != rej.NONE else 0
    return Rejected(res, st[:item.c.n_points if res.status == 0 else 0], list(keeps)[:min(nk, 64)])


def lift(lib, tcfg, cfg, width, height, pts):
    """the restatement's lift of pixels [n][2] -> [n][2] float32"""
    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    out = np.zeros_like(p)
    lib.isvo_rej_lift(C.byref(tcfg), C.byref(cfg), width, height, len(p), p.ctypes.data_as(_f32p), out.ctypes.data_as(_f32p))
    return out


def median(lib, errors):
    e = np.array(errors, np.float32)
    return lib.isvo_rej_median(e.ctypes.data_as(_f32p), len(e))


def subsets(lib, count, n_sub, state=(1 << 64) - 1):
    s = C.c_uint64(state)
    out = np.zeros((n_sub, 7), np.int32)
    lib.isvo_rej_subsets(C.byref(s), count, n_sub, out.ctypes.data_as(_i32p))
    return out, s.value
