"""CPU checks of include/isvins_loop.h: the library exports every isv_loop_* it declares, the ctypes mirror has the header's
struct sizes, the handle fails loudly without a GPU and refuses bad configurations, and isv_loop_apply (host only) writes exactly
the keyframe members findConnection / PnPRANSAC write."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from isvins_amd import backend, loop, posegraph
from test_abi import ROOT, declared_functions

HEADER = os.path.join(ROOT, "include", "isvins_loop.h")


@pytest.fixture(scope="module")
def lib():
    backend.build()
    lib = backend.load_library()
    loop._bind(lib)
    return lib


def test_every_loop_symbol_is_exported(lib):
    names = [n for n in declared_functions(HEADER) if n.startswith("isv_loop_")]
    assert set(names) == set(loop.EXPORTS) and len(names) == 6
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/isvins_loop.h but not exported"
    # the new header adds nothing to the two whose export sets tests/test_abi.py pins
    for other in ("isvins_backend.h", "isvins_posegraph.h"):
        assert not [n for n in declared_functions(os.path.join(ROOT, "include", other)) if n.startswith("isv_loop_")]


def test_struct_sizes_match_header(tmp_path):
    structs = ["isv_loop_config_t", "isv_loop_pair_t", "isv_loop_result_t"]
    src = tmp_path / "szl.c"
    src.write_text('#include <stdio.h>\n#include "isvins_loop.h"\nint main(){' + "".join(f'printf("%zu\\n", sizeof({n}));' for n in structs) +
                   'printf("%d\\n", (int)ISV_LOOP_INPUT); return 0;}')
    exe = tmp_path / "szl"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    for n, s in zip(structs, out):
        assert C.sizeof(getattr(loop, n)) == s, n
    assert out[3] == loop.ISV_LOOP_INPUT == 7


def test_create_fails_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(backend.BackendError):
        loop.LoopVerifier(4)
    cfg, h = loop.make_config(4), C.c_void_p()
    assert lib.isv_loop_create(C.byref(cfg), C.byref(h)) == -4 and not h.value


def test_create_rejects_bad_config(lib):
    h = C.c_void_p()
    assert lib.isv_loop_create(None, C.byref(h)) == -1
    assert lib.isv_loop_create(C.byref(loop.make_config(1)), None) == -1
    for bad in (dict(max_pairs=0), dict(max_points=0), dict(max_keypoints=0), dict(max_keypoints=(1 << 20) + 1), dict(min_loop_num=8),
                dict(ransac_iterations=0), dict(match_accept_dist=0), dict(match_accept_dist=129), dict(match_max_dist=257),
                dict(focal_length=0.0), dict(ransac_threshold=-1.0), dict(ransac_confidence=1.0), dict(ransac_confidence=float("nan")),
                dict(max_yaw_deg=0.0), dict(max_distance=float("nan")), dict(tic=[0.0, float("inf"), 0.0]), dict(ric=np.full((3, 3), np.nan))):
        assert lib.isv_loop_create(C.byref(loop.make_config(**bad)), C.byref(h)) == -1, bad
        assert not h.value
    assert lib.isv_loop_last_error(None) == b"null handle"
    assert lib.isv_loop_last_ms(None, (C.c_double * 3)()) == -1
    assert lib.isv_loop_verify_batch(None, 0, None, None, None, None, None) == -1


def _keyframe():
    kf = posegraph.isv_pg_keyframe_t()
    raw = (C.c_ubyte * C.sizeof(kf)).from_buffer(kf)
    for i in range(len(raw)):
        raw[i] = (37 * i + 11) & 0xFF
    return kf


def _changed(before, after):
    """names of the keyframe members whose bytes differ"""
    out = []
    for name, _ in posegraph.isv_pg_keyframe_t._fields_:
        f = getattr(posegraph.isv_pg_keyframe_t, name)
        if bytes(before)[f.offset:f.offset + f.size] != bytes(after)[f.offset:f.offset + f.size]:
            out.append(name)
    return out


def test_apply_writes_the_reference_fields(lib):
    r = loop.isv_loop_result_t()
    r.status, r.has_loop, r.loop_index, r.loop_weight = loop.ISV_LOOP_OK, 1, 42, 123.5
    r.loop_info[:] = [0.1, 0.2, 0.3, 0.9, 0.01, 0.02, 0.03, 12.5]
    kf = _keyframe(); before = bytes(kf)
    loop.apply(r, kf, lib)
    assert sorted(_changed(before, kf)) == ["has_loop", "loop_index", "loop_info", "loop_weight"]
    assert (kf.has_loop, kf.loop_index, kf.loop_weight) == (1, 42, 123.5) and list(kf.loop_info) == list(r.loop_info)
    for st in range(1, 8):
        r.status, r.loop_weight = st, 7.25 + st
        kf = _keyframe(); before = bytes(kf)
        loop.apply(r, kf, lib)
        assert _changed(before, kf) == ["loop_weight"] and kf.loop_weight == 7.25 + st, st
    assert lib.isv_loop_apply(None, C.byref(kf)) == -1 and lib.isv_loop_apply(C.byref(r), None) == -1
