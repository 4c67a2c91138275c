"""CPU checks of include/isvins_frontend.h: the library exports every isv_fe_* it declares and the header declares nothing else, the
other headers declare no isv_fe_*, the ctypes mirror has the header's struct sizes, isv_fe_create refuses each bad argument before it
looks into a handle, the entry points refuse a null handle, and a front end needs a tracker and so a GPU."""
import ctypes as C
import os
import subprocess

import pytest

from isvins_amd import backend, detect as det, frontend as fe, reject as rej, tracker as trk
from test_abi import ROOT, declared_functions

HEADER = os.path.join(ROOT, "include", "isvins_frontend.h")


@pytest.fixture(scope="module")
def lib():
    backend.build()
    lib = backend.load_library()
    fe._bind(lib)
    return lib


def test_every_fe_symbol_is_exported(lib):
    names = declared_functions(HEADER)
    assert set(names) == set(fe.EXPORTS) and len(names) == 10 and all(n.startswith("isv_fe_") for n in names)
    for n in names:
        assert hasattr(lib, n), f"{n} declared but not exported"
    for other in sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith((".h", ".hpp")) and f != "isvins_frontend.h"):
        assert not [n for n in declared_functions(os.path.join(ROOT, "include", other)) if n.startswith("isv_fe_")], other
    assert lib.isv_abi_version() == 2


def test_struct_sizes_match_header(tmp_path):
    structs = ["isv_fe_config_t", "isv_fe_item_t", "isv_fe_result_t", "isv_fe_state_t", "isv_fe_gate_t", "isv_fe_gate_out_t"]
    src = tmp_path / "szf.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "isvins_frontend.h"\nint main(){' + "".join(f'printf("%zu\\n", sizeof({n}));' for n in structs) +
                   'printf("%zu %zu %zu\\n", offsetof(isv_fe_item_t, cur_time), offsetof(isv_fe_state_t, prev_time), offsetof(isv_fe_gate_t, freq)); return 0;}')
    exe = tmp_path / "szf"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    for n, s in zip(structs, out):
        assert C.sizeof(getattr(fe, n)) == s, n
    assert out[:6] == [16, 40, 40, 24, 40, 16]
    assert out[6:] == [fe.isv_fe_item_t.cur_time.offset, fe.isv_fe_state_t.prev_time.offset, fe.isv_fe_gate_t.freq.offset] == [24, 16, 32]


def test_create_refusals_and_null_handles(lib):
    h = C.c_void_p()
    fake = C.c_void_p(1)                  # never dereferenced: every refusal below comes first
    good = fe.make_config()
    for args in ((None, None, fake, fake), (fake, None, None, fake), (fake, None, fake, None)):           # no tracker, no rejector, no detector
        assert lib.isv_fe_create(*args, C.byref(good), C.byref(h)) == -1 and not h.value
    assert lib.isv_fe_create(fake, None, fake, fake, None, C.byref(h)) == -1
    assert lib.isv_fe_create(fake, None, fake, fake, C.byref(good), None) == -1
    for bad in (dict(max_items=0), dict(max_items=-1), dict(max_items=65536), dict(max_cnt=0), dict(max_cnt=-150), dict(max_points=149),
                dict(max_points=0), dict(max_points=65536), dict(max_cnt=70000, max_points=70000)):
        assert lib.isv_fe_create(fake, fake, fake, fake, C.byref(fe.make_config(**bad)), C.byref(h)) == -1, bad
        assert not h.value
    assert lib.isv_fe_last_error(None) == b"null handle"
    assert lib.isv_fe_last_ms(None, (C.c_double * 6)()) == -1
    assert lib.isv_fe_read_image_batch(None, 0, *[None] * 11) == -1
    assert lib.isv_fe_slot_reset(None, 0) == -1
    st = fe.isv_fe_state_t()
    assert lib.isv_fe_slot_get(None, 0, C.byref(st), None, None, None, None, None) == -1
    assert lib.isv_fe_slot_set(None, 0, C.byref(st), None, None, None, None, None) == -1
    lib.isv_fe_destroy(None)


def test_front_end_needs_a_tracker_and_so_a_gpu(lib):
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(backend.BackendError):
            fe.FrontEnd(trk.Tracker(2), None, None)               # the tracker itself cannot exist: there is no CPU path
        return
    tr, tr2 = trk.Tracker(2, max_points=64), trk.Tracker(1, max_points=64)
    rj, dt, other = rej.Rejector(tr), det.Detector(tr, max_points=64, max_corners=40), rej.Rejector(tr2)
    f = fe.FrontEnd(tr, rj, dt)
    assert f.h and (f.cfg.max_items, f.cfg.max_cnt, f.cfg.max_points) == (2, 40, 64) and f.last_ms() == (0.0,) * 6
    for kw, stages in ((dict(max_points=65), (tr, rj, dt)), (dict(max_cnt=41), (tr, rj, dt)), (dict(max_items=3), (tr, rj, dt)), (dict(max_points=39), (tr, rj, dt)),
                       (dict(), (tr, other, dt))):            # beyond a stage's capacity; below max_cnt; a rejector on another tracker
        with pytest.raises(backend.BackendError):
            fe.FrontEnd(*stages, **kw)
    st = f.slot_get(1)
    assert (st.has_sequence, len(st.prev_pts), st.n_id) == (0, 0, 0)
    with pytest.raises(backend.BackendError):
        f.slot_get(2)
    f.close(); other.close(); dt.close(); rj.close(); tr2.close(); tr.close()


def test_host_helpers():
    c = fe.make_config()
    assert (c.max_items, c.max_cnt, c.max_points) == (1, 150, 256)
    s = fe.State([[1, 2], [3, 4]], n_id=5)
    assert s.ids.tolist() == [-1, -1] and s.track_cnt.tolist() == [1, 1] and s.in_map.dtype.name == "uint8" and s.prev_un_pts.shape == (2, 2)
    assert s.key() == fe.State([[1, 2], [3, 4]], n_id=5).key() != fe.State([[1, 2], [3, 4]], n_id=6).key()
