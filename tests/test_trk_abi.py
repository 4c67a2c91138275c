"""CPU checks of include/isvins_tracker.h: the library exports every isv_trk_* it declares (and the internal debug read-back), the
ctypes mirror has the header's struct sizes and constants, the handle fails loudly without a GPU and refuses each bad
configuration, and the entry points refuse a null handle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import trk_oracle
from isvins_amd import backend, tracker as trk
from test_abi import ROOT, declared_functions

HEADER = os.path.join(ROOT, "include", "isvins_tracker.h")


@pytest.fixture(scope="module")
def lib():
    backend.build()
    lib = backend.load_library()
    trk._bind(lib)
    return lib


def test_every_trk_symbol_is_exported(lib):
    names = declared_functions(HEADER)
    assert set(names) == set(trk.EXPORTS) and len(names) == 6
    for n in names + ["isv_internal_trk_read_level"]:
        assert hasattr(lib, n), f"{n} declared but not exported"
    for other in ("isvins_backend.h", "isvins_posegraph.h", "isvins_loop.h", "isvins_bow.h", "isvins_keyframe.h"):
        assert not [n for n in declared_functions(os.path.join(ROOT, "include", other)) if n.startswith("isv_trk_")]
    assert lib.isv_abi_version() == 2


def test_struct_sizes_match_header(tmp_path):
    structs = ["isv_trk_config_t", "isv_trk_item_t", "isv_trk_result_t"]
    src = tmp_path / "szt.c"
    src.write_text('#include <stdio.h>\n#include "isvins_tracker.h"\nint main(){' + "".join(f'printf("%zu\\n", sizeof({n}));' for n in structs) +
                   'printf("%d %d %d %d %d %d %d\\n", (int)ISV_TRK_CAPACITY, (int)ISV_TRK_INPUT, ISV_TRK_WIN, ISV_TRK_MAX_LEVEL, ISV_TRK_MAX_ITER, '
                   'ISV_TRK_FLAG_STATUS, ISV_TRK_FLAG_BORDER); return 0;}')
    exe = tmp_path / "szt"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    o = trk_oracle.load()                 # asserts isvo_trk_sizeof against the same mirrors
    for i, (n, s) in enumerate(zip(structs, out)):
        assert C.sizeof(getattr(trk, n)) == s == o.isvo_trk_sizeof(i), n
    assert out[3:] == [trk.ISV_TRK_CAPACITY, trk.ISV_TRK_INPUT, trk.WIN, trk.MAX_LEVEL, trk.MAX_ITER, trk.FLAG_STATUS, trk.FLAG_BORDER] == [1, 2, 21, 3, 30, 1, 2]


def test_create_fails_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(backend.BackendError):
        trk.Tracker(4)
    cfg, h = trk.make_config(4, 4), C.c_void_p()
    assert lib.isv_trk_create(C.byref(cfg), C.byref(h)) == -4 and not h.value


def test_create_rejects_bad_config(lib):
    h = C.c_void_p()
    assert lib.isv_trk_create(None, C.byref(h)) == -1
    assert lib.isv_trk_create(C.byref(trk.make_config()), None) == -1
    nan, inf = float("nan"), float("inf")
    for bad in (dict(max_slots=0), dict(max_slots=65537), dict(max_items=0), dict(max_items=65536), dict(max_width=0), dict(max_height=-1),
                dict(max_width=8193), dict(max_height=8193), dict(max_points=0), dict(max_points=65536), dict(win=15), dict(win=0), dict(win=23),
                dict(max_level=0), dict(max_level=2), dict(max_level=4), dict(fx=0.0), dict(fy=-1.0), dict(fx=nan), dict(cx=inf), dict(cy=nan),
                dict(k1=nan), dict(k2=inf), dict(p1=nan), dict(p2=-inf)):
        assert lib.isv_trk_create(C.byref(trk.make_config(**bad)), C.byref(h)) == -1, bad
        assert not h.value
    assert lib.isv_trk_last_error(None) == b"null handle"
    assert lib.isv_trk_last_ms(None, (C.c_double * 5)()) == -1
    assert lib.isv_trk_slot_reset(None, 0) == -1
    assert lib.isv_trk_track_batch(None, 0, None, None, None, None, None, None) == -1
    assert lib.isv_internal_trk_read_level(None, 0, 0, 0, None, None, None) == -1


def test_host_helpers():
    assert trk.levels(752, 480) == [(752, 480), (376, 240), (188, 120), (94, 60)]
    assert trk.levels(181, 179)[-1] == (23, 23) and trk.levels(24, 23) == [(24, 23)]
    a = trk.TrkArrays(np.arange(8, dtype=np.float32).reshape(4, 2), np.array([3, 1, 3, 0], np.uint8), np.zeros(4, np.float32),
                      np.arange(8, dtype=np.float32).reshape(4, 2) * 2)
    cp, un, ids = a.kept([10, 11, 12, 13])
    assert cp.tolist() == [[0, 1], [4, 5]] and un.tolist() == [[0, 2], [8, 10]] and ids.tolist() == [10, 12]
    img = trk.analytic_image(40, 30, (0.5, 0.25), 3)
    assert img.shape == (30, 40) and img.dtype == np.uint8 and img.std() > 5
    assert np.array_equal(trk.analytic_image(40, 30, (4.0, 0.0), 3)[:, 4:], trk.analytic_image(40, 30, (0, 0), 3)[:, :36])
