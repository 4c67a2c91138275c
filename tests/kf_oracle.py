"""Builds and loads tests/native/isv_kf_oracle.c, the serial CPU restatement of include/isvins_keyframe.h, into a temporary
directory (gcc -O2 -ffp-contract=off -shared: the same flags as oracle/Makefile), and the Python side of it: `extract` runs one
item, `reference` runs the scenario list once per process and is shared, unchanged, by the tests that need it."""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from isvins_amd import keyframe as kf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "isv_kf_oracle.c")
_u8p, _u64p, _f32p, _i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_int32)
K1, K2, K4 = 1, 2, 4                  # isvo_kf_set_quirks_off bits


def build(tmpdir, opt="-O2"):
    out = os.path.join(str(tmpdir), f"libisv_kf_oracle{opt}.so")
    subprocess.check_call(["gcc", opt, "-ffp-contract=off", "-std=gnu11", "-Wall", "-Wno-unused-function", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "include"), "-o", out, SRC, "-lm"])
    lib = C.CDLL(out)
    lib.isvo_kf_set_quirks_off.argtypes = [C.c_int]; lib.isvo_kf_set_quirks_off.restype = None
    lib.isvo_kf_sizeof.argtypes = [C.c_int]
    lib.isvo_kf_kernel.argtypes = [_i32p]
    lib.isvo_kf_lift.argtypes = [C.POINTER(kf.isv_kf_config_t), C.c_float, C.c_float, _f32p]; lib.isvo_kf_lift.restype = None
    lib.isvo_kf_extract.argtypes = [C.POINTER(kf.isv_kf_config_t), C.POINTER(kf.isv_kf_item_t), C.POINTER(kf.isv_kf_result_t), _u64p, _f32p,
                                    _f32p, _u8p, _u64p, _u8p, _u8p]
    lib.isvo_kf_extract.restype = None
    for i, s in enumerate((kf.isv_kf_config_t, kf.isv_kf_item_t, kf.isv_kf_result_t)):
        assert lib.isvo_kf_sizeof(i) == C.sizeof(s), s
    return lib


@functools.lru_cache(maxsize=1)
def load():
    """the restatement, built once per process (its directory goes when the process ends)"""
    d = tempfile.mkdtemp(prefix="isv_kf_oracle_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return build(d)


def extract(lib, cfg, item, quirks_off=0):
    """the restatement on one item -> (result, KfArrays, blurred, score_map); the two images are None for an item refused by the
    input checks"""
    r = kf.isv_kf_result_t()
    c, p = max(kf.keypoint_capacity(cfg, item), 1), max(item.c.n_points, 1)
    br, uv, nm = np.zeros((c, 4), np.uint64), np.zeros((c, 2), np.float32), np.zeros((c, 2), np.float32)
    sc, wb = np.zeros(c, np.uint8), np.zeros((p, 4), np.uint64)
    w, h = max(item.c.width, 0), max(item.c.height, 0)
    blur, smap = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    lib.isvo_kf_set_quirks_off(quirks_off)
    try:
        lib.isvo_kf_extract(C.byref(cfg), C.byref(item.c), C.byref(r), br.ctypes.data_as(_u64p), uv.ctypes.data_as(_f32p), nm.ctypes.data_as(_f32p),
                            sc.ctypes.data_as(_u8p), wb.ctypes.data_as(_u64p), blur.ctypes.data_as(_u8p), smap.ctypes.data_as(_u8p))
    finally:
        lib.isvo_kf_set_quirks_off(0)
    k, n = (r.n_keypoints, r.n_points) if r.status == kf.ISV_KF_OK else (0, 0)
    ran = r.status == kf.ISV_KF_OK or r.n_keypoints > 0
    return r, kf.KfArrays(br[:k], uv[:k], nm[:k], sc[:k], wb[:n]), blur if ran else None, smap if ran else None


def lift(lib, cfg, uv):
    out = np.zeros((len(uv), 2), np.float32)
    for i, (u, v) in enumerate(np.asarray(uv, np.float32)):
        lib.isvo_kf_lift(C.byref(cfg), float(u), float(v), out[i].ctypes.data_as(_f32p))
    return out


@functools.lru_cache(maxsize=4)
def reference(distorted=True):
    """the restatement over kf_cases.scenarios(), computed once and shared: (cfg, scenarios, [extract(...) per scenario])"""
    import kf_cases
    cfg = kf_cases.config(distorted)
    scen = kf_cases.scenarios()
    return cfg, scen, [extract(load(), cfg, s["item"]) for s in scen]


def describe(r):
    return dict(status=r.status, n_keypoints=r.n_keypoints, n_points=r.n_points)
