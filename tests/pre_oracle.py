"""Builds and loads tests/native/isv_pre_oracle.c, the serial CPU restatement of include/isvins_preint.h, into a temporary directory
(gcc -O2 -ffp-contract=off -shared: the same flags as oracle/Makefile), and the Python side of it: `Store` is a host-side slot store
with the handle's run_batch, whose arrays (records, heads, buffers) the tests read as bytes; `key_of` is everything a result and its
record are compared on."""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from isvins_amd import preint as pre

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "isv_pre_oracle.c")
STRUCTS = (pre.isv_pre_config_t, pre.isv_pre_nav_t, pre.isv_pre_item_t, pre.isv_pre_result_t, pre.isv_imu_t)
HEAD_BYTES = 104                           # PreSlotHead: acc_0, gyr_0, linearized_acc, linearized_gyr, constructed, n_buffered
SAMPLE = 7                                 # doubles per buffered sample: dt, acc, gyr
# make_config arguments that isv_pre_create and the restatement refuse
BAD_CONFIGS = (dict(max_slots=0), dict(max_slots=-1), dict(max_slots=pre.MAX_SLOTS + 1), dict(max_samples=0), dict(max_samples=-5),
               dict(max_samples=pre.MAX_SAMPLES + 1), dict(max_items=0), dict(max_items=pre.MAX_ITEMS + 1), dict(acc_n=-0.1), dict(gyr_n=float("nan")),
               dict(acc_w=float("inf")), dict(gyr_w=-1e-9), dict(gravity=(0.0, float("nan"), 9.81)))


def build(tmpdir, opt="-O2"):
    out = os.path.join(str(tmpdir), f"libisv_pre_oracle{opt}.so")
    subprocess.check_call(["gcc", opt, "-ffp-contract=off", "-std=gnu11", "-Wall", "-Wno-unused-function", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "include"), "-o", out, SRC, "-lm"])
    lib = C.CDLL(out)
    cfgp = C.POINTER(pre.isv_pre_config_t)
    lib.isvo_pre_sizeof.argtypes = [C.c_int]
    lib.isvo_pre_check_config.argtypes = [cfgp]
    lib.isvo_pre_new.argtypes = [cfgp]; lib.isvo_pre_new.restype = C.c_void_p
    lib.isvo_pre_free.argtypes = [C.c_void_p]; lib.isvo_pre_free.restype = None
    lib.isvo_pre_array.argtypes = [C.c_void_p, C.c_int]; lib.isvo_pre_array.restype = C.c_void_p
    lib.isvo_pre_run_batch.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.POINTER(pre.isv_pre_item_t)), C.POINTER(pre.isv_pre_result_t)]
    for i, s in enumerate(STRUCTS):
        assert lib.isvo_pre_sizeof(i) == C.sizeof(s), s
    assert lib.isvo_pre_sizeof(5) == HEAD_BYTES
    return lib


@functools.lru_cache(maxsize=1)
def load():
    """the restatement, built once per process (its directory goes when the process ends)"""
    d = tempfile.mkdtemp(prefix="isv_pre_oracle_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return build(d)


class Store:
    """the restatement's slot store for a configuration"""

    def __init__(self, lib, cfg):
        self.lib, self.cfg = lib, cfg
        self.h = lib.isvo_pre_new(C.byref(cfg))
        assert self.h, "the restatement refused the configuration"

    def close(self):
        if self.h:
            self.lib.isvo_pre_free(self.h); self.h = None

    def __del__(self):
        self.close()

    def run_batch(self, items):
        """(results, records) as PreIntegrator.run_batch gives them"""
        rc, res, recs = pre.run_on(self.lib.isvo_pre_run_batch, self.h, items)
        assert rc == 0, rc
        return res, recs

    def raw(self):
        """every byte of the store: the records, the heads, the buffers"""
        S = self.cfg.max_slots
        sizes = (S * C.sizeof(pre.isv_imu_t), S * HEAD_BYTES, S * self.cfg.max_samples * SAMPLE * 8)
        return b"".join(C.string_at(self.lib.isvo_pre_array(self.h, k), n) for k, n in enumerate(sizes))

    def head(self, slot):
        """(acc_0, gyr_0, linearized_acc, linearized_gyr, constructed, n_buffered) of a slot"""
        b = C.string_at(self.lib.isvo_pre_array(self.h, 1) + slot * HEAD_BYTES, HEAD_BYTES)
        d = np.frombuffer(b[:96], np.float64).reshape(4, 3)
        c, n = np.frombuffer(b[96:], np.int32)
        return d[0], d[1], d[2], d[3], int(c), int(n)

    def buffer(self, slot):
        """the slot's buffered samples [n_buffered][7]"""
        n = max(self.head(slot)[5], 0)
        b = C.string_at(self.lib.isvo_pre_array(self.h, 2) + slot * self.cfg.max_samples * SAMPLE * 8, n * SAMPLE * 8)
        return np.frombuffer(b, np.float64).reshape(n, SAMPLE)


def record_bytes(rec):
    return None if rec is None else C.string_at(C.addressof(rec), C.sizeof(rec))


def key_of(res, rec=None):
    """a result, with the record where there is one, as bytes: status, n_buffered and every double"""
    return C.string_at(C.addressof(res), C.sizeof(res)), record_bytes(rec)
