"""Builds and loads tests/native/isv_sfm_oracle.c, the CPU restatement of is-vins_amd/csrc/isv_sfm.h, into a temporary
directory (gcc -O2 -ffp-contract=off -shared: the same flags as oracle/Makefile)."""
import ctypes as C
import os
import subprocess

import numpy as np

from isvins_amd import initial

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "isv_sfm_oracle.c")


def build(tmpdir):
    out = os.path.join(str(tmpdir), "libisv_sfm_oracle.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-std=gnu11", "-Wall", "-Wno-unused-function", "-shared", "-fPIC",
                           "-o", out, SRC, "-lm"])
    lib = C.CDLL(out)
    lib.isvo_sfm.argtypes = [C.POINTER(initial.isv_sfm_problem_t), C.POINTER(initial.isv_sfm_result_t)]
    lib.isvo_sfm.restype = C.c_int
    lib.isvo_sfm_sizeof.argtypes = [C.c_int]
    lib.isvo_sfm_sizeof.restype = C.c_int
    lib.isvo_sfm_set_quirks_off.argtypes = [C.c_int]
    lib.isvo_sfm_set_quirks_off.restype = None
    return lib


def solve(lib, p, quirks_off=0):
    """the restatement on problem p; returns (result, positions copy, states copy)"""
    r = initial.isv_sfm_result_t()
    lib.isvo_sfm_set_quirks_off(quirks_off)
    try:
        lib.isvo_sfm(C.byref(p.c), C.byref(r))
    finally:
        lib.isvo_sfm_set_quirks_off(0)
    return r, p.position.copy(), p.state.copy()


def solve_all(lib, ps):
    return [solve(lib, p) for p in ps]


def positions_equal(a, b):
    return np.array_equal(a, b)
