"""CPU checks of include/isvins_equalize.h: the library exports every isv_eq_* it declares (and the internal debug read-back), the header
declares nothing else and does not spell the detector's prefix, the tracker's header still declares its six functions, the ctypes
mirror has the header's struct sizes and constants (and the restatement's), isv_eq_create refuses each bad argument, and the entry
points refuse a null handle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import eq_oracle
from isvins_amd import backend, equalize as eq, tracker as trk
from test_abi import ROOT, declared_functions

HEADER = os.path.join(ROOT, "include", "isvins_equalize.h")


@pytest.fixture(scope="module")
def lib():
    backend.build()
    lib = backend.load_library()
    eq._bind(lib)
    return lib


def test_every_eq_symbol_is_exported(lib):
    names = declared_functions(HEADER)
    assert set(names) == set(eq.EXPORTS) and len(names) == 6 and all(n.startswith("isv_eq_") for n in names)
    for n in names + ["isv_internal_eq_read_luts"]:
        assert hasattr(lib, n), f"{n} declared but not exported"
    text = open(HEADER).read()
    assert "isv_det_" not in text                       # not even in a comment (tests/test_det_abi.py reads every other header for it)
    for other in sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith((".h", ".hpp")) and f != "isvins_equalize.h"):
        assert not [n for n in declared_functions(os.path.join(ROOT, "include", other)) if n.startswith("isv_eq_")], other
    assert len(declared_functions(os.path.join(ROOT, "include", "isvins_tracker.h"))) == 6
    assert lib.isv_abi_version() == 2


def test_struct_sizes_match_header(tmp_path):
    structs = ["isv_eq_config_t", "isv_eq_image_t"]
    src = tmp_path / "sze.c"
    src.write_text('#include <stdio.h>\n#include "isvins_equalize.h"\nint main(){' + "".join(f'printf("%zu\\n", sizeof({n}));' for n in structs) +
                   'printf("%d %d %d\\n", (int)(ISV_EQ_CLIP * 1000), ISV_EQ_TILES, ISV_EQ_MAX_TILES); return 0;}')
    exe = tmp_path / "sze"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    o = eq_oracle.load()                  # asserts isvo_eq_sizeof against the same mirrors
    for i, (n, s) in enumerate(zip(structs, out)):
        assert C.sizeof(getattr(eq, n)) == s == o.isvo_eq_sizeof(i), n
    assert out[:2] == [24, 24]
    assert out[2:] == [int(eq.CLIP * 1000), eq.TILES, eq.MAX_TILES] == [3000, 8, 32]


def test_create_refusals_and_null_handles(lib):
    h = C.c_void_p()
    fake = C.c_void_p(1)                  # never dereferenced: every refusal below comes first
    good = eq.make_config()
    assert lib.isv_eq_create(None, C.byref(good), C.byref(h)) == -1 and not h.value           # no tracker handle: no GPU, or none given
    assert lib.isv_eq_create(fake, None, C.byref(h)) == -1
    assert lib.isv_eq_create(fake, C.byref(good), None) == -1
    nan, inf = float("nan"), float("inf")
    for bad in (dict(clip_limit=-0.5), dict(clip_limit=nan), dict(clip_limit=inf), dict(clip_limit=-inf), dict(tiles_x=0), dict(tiles_x=-8), dict(tiles_x=33),
                dict(tiles_y=0), dict(tiles_y=33), dict(max_items=0), dict(max_items=-1), dict(max_items=65536)):
        assert lib.isv_eq_create(fake, C.byref(eq.make_config(**bad)), C.byref(h)) == -1, bad
        assert not h.value
    assert lib.isv_eq_last_error(None) == b"null handle"
    assert lib.isv_eq_last_ms(None, (C.c_double * 6)()) == -1
    assert lib.isv_eq_track_batch(None, 0, None, None, None, None, None, None) == -1
    assert lib.isv_eq_apply_batch(None, 0, None, None, None) == -1
    assert lib.isv_internal_eq_read_luts(None, 0, 0, None, None, None) == -1
    lib.isv_eq_destroy(None)


def test_equalizer_needs_a_tracker_and_so_a_gpu(lib):
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(backend.BackendError):
            eq.Equalizer(trk.Tracker(2))  # the tracker itself cannot exist: there is no CPU path
        return
    tr = trk.Tracker(2)
    e = eq.Equalizer(tr)
    assert e.h and e.cfg.max_items == 2 and (e.cfg.clip_limit, e.cfg.tiles_x, e.cfg.tiles_y) == (3.0, 8, 8) and e.last_ms() == (0.0,) * 6
    e.close(); tr.close()


def test_host_helpers():
    c = eq.make_config()
    assert (c.clip_limit, c.tiles_x, c.tiles_y, c.max_items) == (3.0, 8, 8, 1)
    it = eq.EqImage(np.zeros((61, 104), np.uint8), 97)
    assert (it.c.width, it.c.height, it.c.stride) == (97, 61, 104) and eq.EqImage(np.zeros((5, 7))).c.width == 7
