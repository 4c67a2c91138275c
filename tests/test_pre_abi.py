"""CPU checks of include/isvins_preint.h: the library exports every isv_pre_* it declares, the header declares nothing else and
spells no other stage's prefix, the other headers declare no isv_pre_*, the ABI version is still 2, the ctypes mirror has the header's
struct sizes, field offsets and constants (a small compiled probe prints them; the restatement's sizes too), isv_pre_create refuses
each bad configuration before it touches a device and gives ISV_ERR_DEVICE without a GPU, and the entry points refuse a null handle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pre_oracle as po
from isvins_amd import backend, preint as pre
from test_abi import ROOT, declared_functions

HEADER = os.path.join(ROOT, "include", "isvins_preint.h")
OTHER_PREFIXES = ("isv_exr_", "isv_rej_", "isv_det_", "isv_eq_", "isv_fe_", "isv_trk_", "isv_kf_", "isv_bow_", "isv_loop_", "isv_pgo_", "isv_estimator_",
                  "isv_batch_", "isv_internal_")
STRUCTS = ["isv_pre_config_t", "isv_pre_nav_t", "isv_pre_item_t", "isv_pre_result_t", "isv_imu_t"]
CONSTANTS = ["ISV_PRE_MAX_SLOTS", "ISV_PRE_MAX_SAMPLES", "ISV_PRE_MAX_ITEMS", "ISV_PRE_PUSH", "ISV_PRE_REPROPAGATE", "ISV_PRE_MERGE", "ISV_PRE_OK",
             "ISV_PRE_CAPACITY", "ISV_PRE_INPUT", "ISV_PRE_UNSET"]


@pytest.fixture(scope="module")
def lib():
    backend.build()
    lib = backend.load_library()
    pre._bind(lib)
    return lib


def test_every_pre_symbol_is_exported(lib):
    names = declared_functions(HEADER)
    assert set(names) == set(pre.EXPORTS) and len(names) == 5 and all(n.startswith("isv_pre_") for n in names)
    for n in names:
        assert hasattr(lib, n), f"{n} declared but not exported"
    text = open(HEADER).read()
    for p in OTHER_PREFIXES:
        assert p not in text, p
    for other in sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith((".h", ".hpp")) and f != "isvins_preint.h"):
        assert "isv_pre_" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert lib.isv_abi_version() == 2


def test_struct_sizes_and_offsets_match_header(tmp_path):
    fields = [(s, f) for s in STRUCTS[:4] for f, _ in getattr(pre, s)._fields_]
    src = tmp_path / "szp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "isvins_preint.h"\nint main(){' +
                   "".join(f'printf("%zu\\n", sizeof({n}));' for n in STRUCTS) +
                   "".join(f'printf("%zu\\n", offsetof({s}, {f}));' for s, f in fields) +
                   "".join(f'printf("%d\\n", (int){c});' for c in CONSTANTS) + "return 0;}")
    exe = tmp_path / "szp"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    o = po.load()                          # asserts isvo_pre_sizeof against the same mirrors
    for i, (n, s) in enumerate(zip(STRUCTS, out)):
        mirror = pre.isv_imu_t if n == "isv_imu_t" else getattr(pre, n)
        assert C.sizeof(mirror) == s == o.isvo_pre_sizeof(i), n
    assert out[:5] == [72, 168, 160, 216, 3736]
    for (s, f), off in zip(fields, out[5:5 + len(fields)]):
        assert getattr(getattr(pre, s), f).offset == off, (s, f)
    consts = out[5 + len(fields):]
    assert consts == [pre.MAX_SLOTS, pre.MAX_SAMPLES, pre.MAX_ITEMS, pre.PUSH, pre.REPROPAGATE, pre.MERGE, pre.ISV_PRE_OK, pre.ISV_PRE_CAPACITY,
                      pre.ISV_PRE_INPUT, pre.ISV_PRE_UNSET]
    assert consts == [1048576, 4096, 65536, 0, 1, 2, 0, 1, 2, 3]


def test_create_refusals_and_null_handles(lib):
    h = C.c_void_p()
    good = pre.make_config()
    assert lib.isv_pre_create(None, C.byref(h)) == -1 and not h.value
    assert lib.isv_pre_create(C.byref(good), None) == -1
    o = po.load()
    for bad in po.BAD_CONFIGS:
        c = pre.make_config(**bad)
        assert lib.isv_pre_create(C.byref(c), C.byref(h)) == -1, bad       # before any device call: the same answer without a GPU
        assert not h.value and o.isvo_pre_check_config(C.byref(c)) == 0
    assert o.isvo_pre_check_config(C.byref(good)) == 1
    assert lib.isv_pre_last_error(None) == b"null handle"
    assert lib.isv_pre_last_ms(None, (C.c_double * 3)()) == -1
    assert lib.isv_pre_run_batch(None, 0, None, None) == -1
    lib.isv_pre_destroy(None)


def test_pre_integrator_needs_a_gpu(lib):
    import torch
    if not torch.cuda.is_available():
        h = C.c_void_p()
        assert backend.STATUS[lib.isv_pre_create(C.byref(pre.make_config()), C.byref(h))] == "ISV_ERR_DEVICE" and not h.value
        with pytest.raises(backend.BackendError):
            pre.PreIntegrator(2)           # there is no CPU path
        return
    p = pre.PreIntegrator(2, max_samples=4, max_items=2)
    assert p.h and p.last_ms() == (0.0, 0.0, 0.0) and p.run_batch([]) == ([], [])
    p.close()


def test_host_helpers():
    c = pre.make_config()
    assert (c.max_slots, c.max_samples, c.max_items, list(c.gravity)) == (1, 64, 256, [0.0, 0.0, 9.81])
    it = pre.push(3, [0.005, 0.01], np.arange(6).reshape(2, 3), np.ones((2, 3), np.float32), reset=True, acc_0=(1, 2, 3), bg=(4, 5, 6),
                  nav=(np.eye(3), (1, 1, 1), (2, 2, 2), (3, 3, 3), (4, 4, 4)), want_record=True)
    assert (it.c.op, it.c.slot, it.c.reset, it.c.n_samples, it.c.want_record) == (pre.PUSH, 3, 1, 2, 1)
    assert it.acc.dtype == np.float64 and it.c.acc[5] == 5.0 and it.c.gyr[0] == 1.0 and list(it.c.acc_0) == [1, 2, 3] and list(it.c.bg) == [4, 5, 6]
    assert list(it.c.nav.contents.R) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(it.c.nav.contents.Bg) == [4, 4, 4] and it.record is not None
    e = pre.push(0)
    assert (e.c.n_samples, e.c.reset, e.c.want_record) == (0, 0, 0) and not e.c.dt and not e.c.nav and not e.c.record and e.record is None
    r = pre.repropagate(2, (1, 2, 3), (4, 5, 6))
    assert (r.c.op, r.c.slot) == (pre.REPROPAGATE, 2) and list(r.c.ba) == [1, 2, 3] and list(r.c.bg) == [4, 5, 6]
    m = pre.merge(1, 7, want_record=True)
    assert (m.c.op, m.c.slot, m.c.src_slot, m.c.want_record) == (pre.MERGE, 1, 7, 1)
