"""Builds and loads tests/native/isv_loop_oracle.c, the CPU restatement of include/isvins_loop.h, into a temporary directory
(gcc -O2 -ffp-contract=off -shared: the same flags as oracle/Makefile; `opt` selects another optimisation level for the
knife-edge check)."""
import ctypes as C
import os
import subprocess

import numpy as np

from isvins_amd import loop

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "isv_loop_oracle.c")
_dp, _fp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
L1, L3, L5, L6 = 1, 4, 16, 32        # isvo_loop_set_quirks_off bits


class lp_match_t(C.Structure):
    _fields_ = [("X", C.c_float * 3), ("uv", C.c_float * 2), ("src", C.c_int32)]


def build(tmpdir, opt="-O2"):
    out = os.path.join(str(tmpdir), f"libisv_loop_oracle{opt}.so")
    subprocess.check_call(["gcc", opt, "-ffp-contract=off", "-std=gnu11", "-Wall", "-Wno-unused-function", "-shared", "-fPIC",
                           "-o", out, SRC, "-lm"])
    lib = C.CDLL(out)
    cfgp, pairp, resp = C.POINTER(loop.isv_loop_config_t), C.POINTER(loop.isv_loop_pair_t), C.POINTER(loop.isv_loop_result_t)
    lib.isvo_loop_set_quirks_off.argtypes = [C.c_int]; lib.isvo_loop_set_quirks_off.restype = None
    lib.isvo_loop_sizeof.argtypes = [C.c_int]
    lib.isvo_loop_match.argtypes = [cfgp, pairp, _ip, _ip, C.POINTER(lp_match_t)]
    lib.isvo_loop_verify.argtypes = [cfgp, pairp, resp, _ip, _ip, _ip]
    lib.isvo_lp_iterative.argtypes = [C.c_int, _dp, _dp, _dp, _ip]
    lib.isvo_lp_epnp.argtypes = [C.c_int, _dp, _dp, _dp, _dp]; lib.isvo_lp_epnp.restype = None
    lib.isvo_lp_epnp_basis.argtypes = [C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]; lib.isvo_lp_epnp_basis.restype = None
    lib.isvo_eig_jacobi_sym.argtypes = [C.c_int, _dp, _dp, _dp]; lib.isvo_eig_jacobi_sym.restype = None
    lib.isvo_rodrigues_v2m.argtypes = [_dp, _dp]; lib.isvo_rodrigues_v2m.restype = None
    lib.isvo_lp_point_error.argtypes = [_dp, _dp, _fp, _fp]; lib.isvo_lp_point_error.restype = C.c_double
    assert lib.isvo_loop_sizeof(0) == C.sizeof(loop.isv_loop_config_t) and lib.isvo_loop_sizeof(1) == C.sizeof(loop.isv_loop_pair_t)
    assert lib.isvo_loop_sizeof(2) == C.sizeof(loop.isv_loop_result_t) and lib.isvo_loop_sizeof(3) == C.sizeof(lp_match_t)
    return lib


def _d(a):
    return a.ctypes.data_as(_dp)


def verify(lib, cfg, pair, quirks_off=0):
    """the restatement on one pair -> (result, match_index, match_dist, inlier)"""
    r = loop.isv_loop_result_t()
    n = max(pair.c.n_points, 0)
    mi, md, inl = (np.full(max(n, 1), -2, dtype=np.int32) for _ in range(3))
    lib.isvo_loop_set_quirks_off(quirks_off)
    try:
        lib.isvo_loop_verify(C.byref(cfg), C.byref(pair.c), C.byref(r), mi.ctypes.data_as(_ip), md.ctypes.data_as(_ip), inl.ctypes.data_as(_ip))
    finally:
        lib.isvo_loop_set_quirks_off(0)
    return r, mi[:n], md[:n], inl[:n]


def match(lib, cfg, pair, quirks_off=0):
    """searchByBRIEFDes alone -> (match_index, match_dist, matched source points in list order)"""
    n = pair.c.n_points
    mi, md = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    lst = (lp_match_t * max(n, 1))()
    lib.isvo_loop_set_quirks_off(quirks_off)
    try:
        k = lib.isvo_loop_match(C.byref(cfg), C.byref(pair.c), mi.ctypes.data_as(_ip), md.ctypes.data_as(_ip), lst)
    finally:
        lib.isvo_loop_set_quirks_off(0)
    return mi[:n], md[:n], np.array([lst[i].src for i in range(k)], dtype=np.int64)


def epnp(lib, X, uv):
    X = np.ascontiguousarray(X, dtype=np.float64); uv = np.ascontiguousarray(uv, dtype=np.float64)
    R, t = np.zeros(9), np.zeros(3)
    lib.isvo_lp_epnp(len(X), _d(X), _d(uv), _d(R), _d(t))
    return R.reshape(3, 3), t


def epnp_basis(lib, X, uv):
    """lp_epnp and the basis it used -> (R, t, control points [4][3], eigenvectors [4][12], smallest eigenvalue first)"""
    X = np.ascontiguousarray(X, dtype=np.float64); uv = np.ascontiguousarray(uv, dtype=np.float64)
    R, t, cws, vv = np.zeros(9), np.zeros(3), np.zeros((4, 3)), np.zeros((4, 12))
    lib.isvo_lp_epnp_basis(len(X), _d(X), _d(uv), _d(R), _d(t), _d(cws), _d(vv))
    return R.reshape(3, 3), t, cws, vv


def iterative(lib, X, uv):
    """the DLT + LM final solve -> (planar, R, t, iterations)"""
    pts = np.ascontiguousarray(np.hstack([X, uv]), dtype=np.float64)
    rv, tv, R, it = np.zeros(3), np.zeros(3), np.zeros(9), C.c_int32(0)
    planar = lib.isvo_lp_iterative(len(pts), _d(pts), _d(rv), _d(tv), C.byref(it))
    lib.isvo_rodrigues_v2m(_d(rv), _d(R))
    return planar, R.reshape(3, 3), tv, it.value


def eig_sym(lib, A):
    n = len(A)
    a = np.ascontiguousarray(A, dtype=np.float64).copy(); w = np.zeros(n); V = np.zeros((n, n))
    lib.isvo_eig_jacobi_sym(n, _d(a), _d(w), _d(V))
    return w, V


def point_error(lib, rvec, tvec, X, uv, quirks_off=0):
    rvec = np.ascontiguousarray(rvec, dtype=np.float64); tvec = np.ascontiguousarray(tvec, dtype=np.float64)
    X = np.ascontiguousarray(X, dtype=np.float32); uv = np.ascontiguousarray(uv, dtype=np.float32)
    lib.isvo_loop_set_quirks_off(quirks_off)
    try:
        return lib.isvo_lp_point_error(_d(rvec), _d(tvec), X.ctypes.data_as(_fp), uv.ctypes.data_as(_fp))
    finally:
        lib.isvo_loop_set_quirks_off(0)
