"""Builds and loads tests/native/isv_init_oracle.c, the CPU restatement of is-vins_amd/csrc/isv_initial.h, into a temporary
directory (gcc -O2 -ffp-contract=off -shared: the same flags as oracle/Makefile)."""
import ctypes as C
import os
import subprocess

from isvins_amd import initial

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "isv_init_oracle.c")


def build(tmpdir):
    out = os.path.join(str(tmpdir), "libisv_init_oracle.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-std=gnu11", "-Wall", "-Wno-unused-function", "-shared", "-fPIC",
                           "-o", out, SRC, "-lm"])
    lib = C.CDLL(out)
    lib.isvo_visual_imu_align.argtypes = [C.POINTER(initial.isv_align_problem_t), C.POINTER(initial.isv_align_result_t)]
    lib.isvo_visual_imu_align.restype = C.c_int
    return lib


def solve(lib, p):
    r = initial.isv_align_result_t()
    lib.isvo_visual_imu_align(C.byref(p.c), C.byref(r))
    return r
