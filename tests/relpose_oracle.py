"""Builds and loads tests/native/isv_relpose_oracle.c, the CPU restatement of is-vins_amd/csrc/isv_relpose.h, into a temporary
directory (gcc -O2 -ffp-contract=off -shared: the same flags as oracle/Makefile)."""
import ctypes as C
import os
import subprocess

import numpy as np

from isvins_amd import initial

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "isv_relpose_oracle.c")
_dp = C.POINTER(C.c_double)


def build(tmpdir):
    out = os.path.join(str(tmpdir), "libisv_relpose_oracle.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-std=gnu11", "-Wall", "-Wno-unused-function", "-shared", "-fPIC",
                           "-o", out, SRC, "-lm"])
    lib = C.CDLL(out)
    lib.isvo_relpose.argtypes = [C.POINTER(initial.isv_sfm_problem_t), C.POINTER(initial.isv_relpose_result_t), C.POINTER(C.c_int32)]
    lib.isvo_relpose.restype = C.c_int
    lib.isvo_relpose_sizeof.argtypes = [C.c_int]
    lib.isvo_relpose_sizeof.restype = C.c_int
    lib.isvo_relpose_set_quirks_off.argtypes = [C.c_int]
    lib.isvo_relpose_set_quirks_off.restype = None
    lib.isvo_rp_solve_cubic.argtypes = [_dp, _dp]
    lib.isvo_rp_solve_cubic.restype = C.c_int
    lib.isvo_rp_run7point.argtypes = [_dp, _dp]
    lib.isvo_rp_run7point.restype = C.c_int
    lib.isvo_rp_update_num_iters.argtypes = [C.c_double, C.c_double, C.c_int, C.c_int]
    lib.isvo_rp_update_num_iters.restype = C.c_int
    lib.isvo_rp_is_inlier.argtypes = [_dp, _dp]
    lib.isvo_rp_is_inlier.restype = C.c_int
    return lib


def solve(lib, p, quirks_off=0):
    """the restatement on problem p; returns (result, per-track mask [n_tracks])"""
    r = initial.isv_relpose_result_t()
    m = np.full(max(p.c.n_tracks, 1), -1, dtype=np.int32)
    lib.isvo_relpose_set_quirks_off(quirks_off)
    try:
        lib.isvo_relpose(C.byref(p.c), C.byref(r), m.ctypes.data_as(C.POINTER(C.c_int32)))
    finally:
        lib.isvo_relpose_set_quirks_off(0)
    return r, m[:max(p.c.n_tracks, 0)]


def with_quirks_off(lib, mask, fn, *args):
    lib.isvo_relpose_set_quirks_off(mask)
    try:
        return fn(*args)
    finally:
        lib.isvo_relpose_set_quirks_off(0)


def solve_cubic(lib, c):
    r = np.zeros(3)
    n = lib.isvo_rp_solve_cubic(np.ascontiguousarray(c, dtype=np.float64).ctypes.data_as(_dp), r.ctypes.data_as(_dp))
    return n, r


def run7point(lib, pts):
    """pts [7][4] (x0 y0 x1 y1) -> (n, F [n][3][3])"""
    F = np.zeros(27)
    n = lib.isvo_rp_run7point(np.ascontiguousarray(pts, dtype=np.float64).ctypes.data_as(_dp), F.ctypes.data_as(_dp))
    return n, F.reshape(3, 3, 3)[:max(n, 0)]
