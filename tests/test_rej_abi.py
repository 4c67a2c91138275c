"""CPU checks of include/isvins_reject.h: the library exports every isv_rej_* it declares, the header declares nothing else, spells
neither the detector's prefix nor an equaliser's function, the other headers declare no isv_rej_* and the tracker's header still
declares its six functions, the ctypes mirror has the header's struct sizes and constants (and the restatement's), isv_rej_create
refuses each bad argument, and the entry points refuse a null handle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rej_oracle
from isvins_amd import backend, reject as rej, tracker as trk
from test_abi import ROOT, declared_functions

HEADER = os.path.join(ROOT, "include", "isvins_reject.h")


@pytest.fixture(scope="module")
def lib():
    backend.build()
    lib = backend.load_library()
    rej._bind(lib)
    return lib


def test_every_rej_symbol_is_exported(lib):
    names = declared_functions(HEADER)
    assert set(names) == set(rej.EXPORTS) and len(names) == 5 and all(n.startswith("isv_rej_") for n in names)
    for n in names:
        assert hasattr(lib, n), f"{n} declared but not exported"
    text = open(HEADER).read()
    assert "isv_det_" not in text and "isv_eq_" not in text   # not even in a comment (tests/test_det_abi.py, tests/test_eq_abi.py read this header)
    for other in sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith((".h", ".hpp")) and f != "isvins_reject.h"):
        assert not [n for n in declared_functions(os.path.join(ROOT, "include", other)) if n.startswith("isv_rej_")], other
    assert len(declared_functions(os.path.join(ROOT, "include", "isvins_tracker.h"))) == 6
    assert lib.isv_abi_version() == 2


def test_struct_sizes_match_header(tmp_path):
    structs = ["isv_rej_config_t", "isv_rej_item_t", "isv_rej_result_t"]
    src = tmp_path / "szr.c"
    src.write_text('#include <stdio.h>\n#include "isvins_reject.h"\nint main(){' + "".join(f'printf("%zu\\n", sizeof({n}));' for n in structs) +
                   'printf("%d %d %d %d %d %d %d %d\\n", ISV_REJ_MIN_POINTS, ISV_REJ_RANSAC_MIN, ISV_REJ_MAX_POINTS, ISV_REJ_NONE, ISV_REJ_LMEDS, ISV_REJ_RANSAC,'
                   ' (int)(ISV_REJ_FOCAL_LENGTH * 10), (int)(ISV_REJ_F_THRESHOLD * 10)); return 0;}')
    exe = tmp_path / "szr"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    o = rej_oracle.load()                 # asserts isvo_rej_sizeof against the same mirrors
    for i, (n, s) in enumerate(zip(structs, out)):
        assert C.sizeof(getattr(rej, n)) == s == o.isvo_rej_sizeof(i), n
    assert out[:3] == [24, 32, 32]
    assert out[3:] == [rej.MIN_POINTS, rej.RANSAC_MIN, rej.MAX_POINTS, rej.NONE, rej.LMEDS, rej.RANSAC, int(rej.FOCAL_LENGTH * 10), int(rej.F_THRESHOLD * 10)]
    assert out[3:] == [8, 15, 4096, 0, 1, 2, 4600, 10]


def test_create_refusals_and_null_handles(lib):
    h = C.c_void_p()
    fake = C.c_void_p(1)                  # never dereferenced: every refusal below comes first
    good = rej.make_config()
    assert lib.isv_rej_create(None, C.byref(good), C.byref(h)) == -1 and not h.value          # no tracker handle: no GPU, or none given
    assert lib.isv_rej_create(fake, None, C.byref(h)) == -1
    assert lib.isv_rej_create(fake, C.byref(good), None) == -1
    nan, inf = float("nan"), float("inf")
    for bad in (dict(max_items=0), dict(max_items=-1), dict(max_items=65536), dict(max_points=0), dict(max_points=-4), dict(max_points=4097),
                dict(focal_length=0.0), dict(focal_length=-460.0), dict(focal_length=nan), dict(focal_length=inf), dict(f_threshold=0.0),
                dict(f_threshold=-1.0), dict(f_threshold=nan), dict(f_threshold=inf), dict(f_threshold=-inf)):
        assert lib.isv_rej_create(fake, C.byref(rej.make_config(**bad)), C.byref(h)) == -1, bad
        assert not h.value
    assert lib.isv_rej_last_error(None) == b"null handle"
    assert lib.isv_rej_last_ms(None, (C.c_double * 4)()) == -1
    assert lib.isv_rej_reject_batch(None, 0, None, None, None) == -1
    lib.isv_rej_destroy(None)


def test_rejector_needs_a_tracker_and_so_a_gpu(lib):
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(backend.BackendError):
            rej.Rejector(trk.Tracker(2))  # the tracker itself cannot exist: there is no CPU path
        return
    tr = trk.Tracker(2, max_points=300)
    r = rej.Rejector(tr)
    assert r.h and (r.cfg.max_items, r.cfg.max_points, r.cfg.focal_length, r.cfg.f_threshold) == (2, 300, 460.0, 1.0) and r.last_ms() == (0.0,) * 4
    with pytest.raises(backend.BackendError):
        rej.Rejector(tr, max_points=301)  # beyond the tracker's
    r.close(); tr.close()


def test_host_helpers():
    c = rej.make_config()
    assert (c.max_items, c.max_points, c.focal_length, c.f_threshold) == (1, 256, 460.0, 1.0)
    it = rej.RejItem(752, 480, np.zeros((5, 2)), np.ones((5, 2), np.float64))
    assert (it.c.width, it.c.height, it.c.n_points) == (752, 480, 5) and it.cur_pts.dtype == np.float32
    ids, cnt, pts = np.arange(5), np.arange(5) * 2, np.arange(10.0).reshape(5, 2)
    a, b, p = rej.reduce_vector([1, 0, 1, 1, 0], ids, cnt, pts)
    assert a.tolist() == [0, 2, 3] and b.tolist() == [0, 4, 6] and p.tolist() == [[0.0, 1.0], [4.0, 5.0], [6.0, 7.0]]
    assert rej.reduce_vector(np.array([0, 3], np.uint8), ids[:2]).tolist() == [1]
