"""CPU checks of include/isvins_detect.h: the library exports every isv_det_* it declares (and the internal debug read-back), no other
public header declares one, the ctypes mirror has the header's struct sizes and constants (and the restatement's), isv_det_create
refuses each bad argument, and the entry points refuse a null handle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import det_oracle
from isvins_amd import backend, detect as det
from test_abi import ROOT, declared_functions

HEADER = os.path.join(ROOT, "include", "isvins_detect.h")


@pytest.fixture(scope="module")
def lib():
    backend.build()
    lib = backend.load_library()
    det._bind(lib)
    return lib


def test_every_det_symbol_is_exported(lib):
    names = [n for n in declared_functions(HEADER) if n.startswith("isv_det_")]
    assert set(names) == set(det.EXPORTS) and len(names) == 5
    for n in names + ["isv_internal_det_read_plane"]:
        assert hasattr(lib, n), f"{n} declared but not exported"
    others = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith((".h", ".hpp")) and f != "isvins_detect.h")
    assert "isvins_tracker.h" in others and len(others) >= 7
    for other in others:
        assert "isv_det_" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert lib.isv_abi_version() == 2


def test_struct_sizes_match_header(tmp_path):
    structs = ["isv_det_config_t", "isv_det_item_t", "isv_det_result_t"]
    src = tmp_path / "szd.c"
    src.write_text('#include <stdio.h>\n#include "isvins_detect.h"\nint main(){' + "".join(f'printf("%zu\\n", sizeof({n}));' for n in structs) +
                   'printf("%d %d %d %d %d\\n", (int)ISV_DET_CAPACITY, (int)ISV_DET_INPUT, ISV_DET_BLOCK_SIZE, ISV_DET_APERTURE, ISV_DET_USE_HARRIS); return 0;}')
    exe = tmp_path / "szd"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    o = det_oracle.load()                 # asserts isvo_det_sizeof against the same mirrors
    for i, (n, s) in enumerate(zip(structs, out)):
        assert C.sizeof(getattr(det, n)) == s == o.isvo_det_sizeof(i), n
    assert out[:3] == [24, 32, 24]
    assert out[3:] == [det.ISV_DET_CAPACITY, det.ISV_DET_INPUT, det.BLOCK_SIZE, det.APERTURE, det.USE_HARRIS] == [1, 2, 3, 3, 0]


def test_create_refusals_and_null_handles(lib):
    h = C.c_void_p()
    fake = C.c_void_p(1)                  # never dereferenced: every refusal below comes first
    good = det.make_config()
    assert lib.isv_det_create(None, C.byref(good), C.byref(h)) == -1 and not h.value          # no tracker handle: no GPU, or none given
    assert lib.isv_det_create(fake, None, C.byref(h)) == -1
    assert lib.isv_det_create(fake, C.byref(good), None) == -1
    nan, inf = float("nan"), float("inf")
    for bad in (dict(max_items=0), dict(max_items=65536), dict(max_points=0), dict(max_points=65536), dict(max_corners=0), dict(max_corners=65536),
                dict(min_dist=0), dict(min_dist=-3), dict(min_dist=256), dict(quality_level=0.0), dict(quality_level=-0.01), dict(quality_level=1.5),
                dict(quality_level=nan), dict(quality_level=inf)):
        assert lib.isv_det_create(fake, C.byref(det.make_config(**bad)), C.byref(h)) == -1, bad
        assert not h.value
    assert lib.isv_det_last_error(None) == b"null handle"
    assert lib.isv_det_last_ms(None, (C.c_double * 5)()) == -1
    assert lib.isv_det_detect_batch(None, 0, None, None, None, None, None) == -1
    assert lib.isv_internal_det_read_plane(None, 0, 0, None, None, None, None) == -1
    lib.isv_det_destroy(None)


def test_detector_needs_a_tracker_and_so_a_gpu(lib):
    import torch
    from isvins_amd import tracker as trk
    if not torch.cuda.is_available():
        with pytest.raises(backend.BackendError):
            det.Detector(trk.Tracker(2))  # the tracker itself cannot exist: there is no CPU path
        return
    tr = trk.Tracker(2)
    dt = det.Detector(tr)
    assert dt.h and dt.cfg.max_items == 2 and dt.last_ms() == (0.0,) * 5
    dt.close(); tr.close()


def test_host_helpers():
    c = det.make_config()
    assert (c.max_corners, c.min_dist, c.quality_level) == (150, 30, 0.01)
    it = det.DetItem(3, [[1.5, 2.5], [3, 4]], [2, 5], 7)
    assert (it.c.slot, it.c.n_points, it.c.max_new) == (3, 2, 7) and it.points.dtype == np.float32 and it.track_cnt.dtype == np.int32
    other = it.on_slot(9)
    assert other.c.slot == 9 and np.array_equal(other.points, it.points) and det.DetItem(0).c.n_points == 0
    a = det.filled(3, 2, np.float32)
    assert a.shape == (3, 2) and det.untouched(a, 0)
    a[1, 0] = 0.0
    assert det.untouched(a, 2) and not det.untouched(a, 1)
