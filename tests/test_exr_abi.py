"""CPU checks of include/isvins_exrot.h: the library exports every isv_exr_* it declares, the header declares nothing else and
spells no other stage's prefix (not even in a comment: the other stages' ABI tests read every header), the other headers declare no
isv_exr_*, the tracker's header still declares its six functions and the ABI version is still 2, the ctypes mirror has the header's
struct sizes and constants (and the restatement's), isv_exr_create refuses each bad configuration before it touches a device, and the
entry points refuse a null handle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import exr_oracle
from isvins_amd import backend, exrot as exr
from test_abi import ROOT, declared_functions

HEADER = os.path.join(ROOT, "include", "isvins_exrot.h")
OTHER_PREFIXES = ("isv_rej_", "isv_det_", "isv_eq_", "isv_fe_", "isv_trk_", "isv_kf_", "isv_bow_", "isv_loop_", "isv_pgo_", "isv_estimator_", "isv_batch_", "isv_internal_")


@pytest.fixture(scope="module")
def lib():
    backend.build()
    lib = backend.load_library()
    exr._bind(lib)
    return lib


def test_every_exr_symbol_is_exported(lib):
    names = declared_functions(HEADER)
    assert set(names) == set(exr.EXPORTS) and len(names) == 7 and all(n.startswith("isv_exr_") for n in names)
    for n in names:
        assert hasattr(lib, n), f"{n} declared but not exported"
    text = open(HEADER).read()
    for p in OTHER_PREFIXES:
        assert p not in text, p
    for other in sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith((".h", ".hpp")) and f != "isvins_exrot.h"):
        assert "isv_exr_" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert len(declared_functions(os.path.join(ROOT, "include", "isvins_tracker.h"))) == 6
    assert lib.isv_abi_version() == 2


def test_struct_sizes_match_header(tmp_path):
    structs = ["isv_exr_config_t", "isv_exr_item_t", "isv_exr_result_t"]
    src = tmp_path / "szx.c"
    src.write_text('#include <stdio.h>\n#include "isvins_exrot.h"\nint main(){' + "".join(f'printf("%zu\\n", sizeof({n}));' for n in structs) +
                   'printf("%d %d %d %d %d %d %d %d %d %d %d %d\\n", ISV_EXR_MIN_CORRES, ISV_EXR_RANSAC_MIN, ISV_EXR_MAX_CORRES, ISV_EXR_MAX_FRAMES, ISV_EXR_VO_SIZE,'
                   ' ISV_EXR_NONE, ISV_EXR_LMEDS, ISV_EXR_RANSAC, ISV_EXR_OK, ISV_EXR_CAPACITY, ISV_EXR_INPUT, ISV_EXR_NO_MODEL); return 0;}')
    exe = tmp_path / "szx"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    o = exr_oracle.load()                 # asserts isvo_exr_sizeof against the same mirrors
    for i, (n, s) in enumerate(zip(structs, out)):
        assert C.sizeof(getattr(exr, n)) == s == o.isvo_exr_sizeof(i), n
    assert out[:3] == [16, 48, 240]
    assert out[3:] == [exr.MIN_CORRES, exr.RANSAC_MIN, exr.MAX_CORRES, exr.MAX_FRAMES, exr.VO_SIZE, exr.NONE, exr.LMEDS, exr.RANSAC,
                       exr.ISV_EXR_OK, exr.ISV_EXR_CAPACITY, exr.ISV_EXR_INPUT, exr.ISV_EXR_NO_MODEL]
    assert out[3:] == [9, 15, 4096, 1024, 8, 0, 1, 2, 0, 1, 2, 3]


def test_create_refusals_and_null_handles(lib):
    h = C.c_void_p()
    good = exr.make_config()
    assert lib.isv_exr_create(None, C.byref(h)) == -1 and not h.value
    assert lib.isv_exr_create(C.byref(good), None) == -1
    o = exr_oracle.load()
    for bad in (dict(max_slots=0), dict(max_slots=-1), dict(max_slots=65536), dict(max_frames=7), dict(max_frames=0), dict(max_frames=1025),
                dict(max_corres=8), dict(max_corres=-9), dict(max_corres=4097), dict(vo_size=1), dict(vo_size=0), dict(vo_size=-8)):
        c = exr.make_config(**bad)
        assert lib.isv_exr_create(C.byref(c), C.byref(h)) == -1, bad      # before any device call: the same answer without a GPU
        assert not h.value and o.isvo_exr_check_config(C.byref(c)) == 0
    assert o.isvo_exr_check_config(C.byref(good)) == 1
    assert lib.isv_exr_last_error(None) == b"null handle"
    assert lib.isv_exr_last_ms(None, (C.c_double * 2)()) == -1
    assert lib.isv_exr_reset(None, 0, None) == -1
    assert lib.isv_exr_calibrate_batch(None, 0, None, None) == -1
    assert lib.isv_exr_read_slot(None, 0, None, None, None) == -1
    lib.isv_exr_destroy(None)


def test_calibrator_needs_a_gpu(lib):
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(backend.BackendError):
            exr.Calibrator(2)             # there is no CPU path
        return
    c = exr.Calibrator(2, max_frames=8, max_corres=9, vo_size=2)
    assert c.h and c.last_ms() == (0.0, 0.0) and c.read_slot(1)[0] == 0
    c.close()


def test_host_helpers():
    c = exr.make_config()
    assert (c.max_slots, c.max_frames, c.max_corres, c.vo_size) == (1, 32, 256, 8)
    it = exr.ExrItem(3, np.arange(8, dtype=np.float32).reshape(2, 4), (1, 0, 0, 0))
    assert (it.c.slot, it.c.n_corres) == (3, 2) and it.corres.dtype == np.float64 and list(it.c.delta_q) == [1.0, 0.0, 0.0, 0.0]
    assert it.c.corres[7] == 7.0
