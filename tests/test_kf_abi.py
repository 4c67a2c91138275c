"""CPU checks of include/isvins_keyframe.h: the library exports every isv_kf_* it declares (and the internal debug read-back),
the ctypes mirror has the header's struct sizes, the handle fails loudly without a GPU and refuses each bad configuration, the
pattern-file loader refuses what it must, and the fixture tests/golden/brief_pattern.npz holds four lists of 256 int8 values
within [-24, 24]."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kf_oracle
from isvins_amd import backend, keyframe as kf
from test_abi import ROOT, declared_functions

HEADER = os.path.join(ROOT, "include", "isvins_keyframe.h")


@pytest.fixture(scope="module")
def lib():
    backend.build()
    lib = backend.load_library()
    kf._bind(lib)
    return lib


def test_every_kf_symbol_is_exported(lib):
    names = declared_functions(HEADER)
    assert set(names) == set(kf.EXPORTS) and len(names) == 5
    for n in names + ["isv_internal_kf_read_back"]:
        assert hasattr(lib, n), f"{n} declared but not exported"
    for other in ("isvins_backend.h", "isvins_posegraph.h", "isvins_loop.h", "isvins_bow.h"):
        assert not [n for n in declared_functions(os.path.join(ROOT, "include", other)) if n.startswith("isv_kf_")]
    assert lib.isv_abi_version() == 2


def test_struct_sizes_match_header(tmp_path):
    structs = ["isv_kf_config_t", "isv_kf_item_t", "isv_kf_result_t"]
    src = tmp_path / "szk.c"
    src.write_text('#include <stdio.h>\n#include "isvins_keyframe.h"\nint main(){' + "".join(f'printf("%zu\\n", sizeof({n}));' for n in structs) +
                   'printf("%d %d %d %d\\n", (int)ISV_KF_CAPACITY, (int)ISV_KF_INPUT, ISV_KF_PATTERN_BITS, ISV_KF_PATTERN_RADIUS); return 0;}')
    exe = tmp_path / "szk"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    for n, s in zip(structs, out):
        assert C.sizeof(getattr(kf, n)) == s, n
    assert out[3:] == [kf.ISV_KF_CAPACITY, kf.ISV_KF_INPUT, kf.PATTERN_BITS, kf.PATTERN_RADIUS] == [1, 2, 256, 24]
    kf_oracle.load()                      # asserts isvo_kf_sizeof against the same mirrors


def test_create_fails_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(backend.BackendError):
        kf.KeyframeExtractor(4)
    cfg, h = kf.make_config(4), C.c_void_p()
    assert lib.isv_kf_create(C.byref(cfg), C.byref(h)) == -4 and not h.value


def test_create_rejects_bad_config(lib):
    h = C.c_void_p()
    assert lib.isv_kf_create(None, C.byref(h)) == -1
    assert lib.isv_kf_create(C.byref(kf.make_config()), None) == -1
    nan, inf = float("nan"), float("inf")
    for bad in (dict(max_items=0), dict(max_width=0), dict(max_height=-1), dict(max_width=8193), dict(max_keypoints=0), dict(max_points=0),
                dict(fast_threshold=0), dict(fast_threshold=255), dict(fx=0.0), dict(fy=-1.0), dict(fx=nan), dict(cx=inf), dict(cy=nan),
                dict(k1=nan), dict(k2=inf), dict(p1=nan), dict(p2=-inf)):
        assert lib.isv_kf_create(C.byref(kf.make_config(**bad)), C.byref(h)) == -1, bad
        assert not h.value
    for key in ("x1", "y1", "x2", "y2"):
        for v in (25, -25, 127, -128):
            pat = kf.default_pattern()
            pat[key][100] = v
            assert lib.isv_kf_create(C.byref(kf.make_config(pattern=pat)), C.byref(h)) == -1, (key, v)
            assert not h.value
    assert lib.isv_kf_last_error(None) == b"null handle"
    assert lib.isv_kf_last_ms(None, (C.c_double * 7)()) == -1
    assert lib.isv_kf_extract_batch(None, 0, None, None, None, None, None, None, None) == -1
    assert lib.isv_internal_kf_read_back(None, 0, None, None) == -1


def _yaml(lists, head="%YAML:1.0"):
    return head + "\n" + "".join(f"{k}:\n" + "".join(f"  - {v}\n" for v in vs) for k, vs in lists.items())


def test_pattern_loader(tmp_path):
    rng = np.random.Generator(np.random.PCG64(5))
    good = {k: rng.integers(-24, 25, 256).tolist() for k in ("x1", "y1", "x2", "y2")}
    good["x1"][0], good["y2"][255] = -24, 24
    path = tmp_path / "pattern.yml"
    path.write_text(_yaml(good))
    got = kf.load_brief_pattern(str(path))
    assert sorted(got) == ["x1", "x2", "y1", "y2"]
    for k in good:
        assert got[k].dtype == np.int8 and got[k].tolist() == good[k]
    cfg = kf.make_config(pattern=got)
    assert list(cfg.y2) == good["y2"]

    def refused(text):
        path.write_text(text)
        with pytest.raises(ValueError):
            kf.load_brief_pattern(str(path))

    refused(_yaml(good, head="%YAML:1.1"))
    refused(_yaml({**good, "x2": good["x2"][:255]}))
    refused(_yaml({**good, "y1": good["y1"] + [0]}))
    refused(_yaml({**good, "x1": [25] + good["x1"][1:]}))
    refused(_yaml({**good, "y2": good["y2"][:-1] + [-25]}))
    refused(_yaml({k: good[k] for k in ("x1", "y1", "x2")}))
    refused(_yaml({**good, "z9": good["x1"]}))
    refused(_yaml(good).replace("  - ", "  - a", 1))
    refused("%YAML:1.0\n  - 3\n" + _yaml(good).split("\n", 1)[1])
    refused(_yaml(good) + "x1:\n  - 1\n")
    refused("")


def test_fixture_pattern():
    path = os.path.join(ROOT, "tests", "golden", "brief_pattern.npz")
    assert os.path.getsize(path) < 4096
    with np.load(path) as z:
        assert sorted(z.files) == ["x1", "x2", "y1", "y2"]
        for k in z.files:
            assert z[k].dtype == np.int8 and z[k].shape == (256,) and -24 <= z[k].min() and z[k].max() <= 24
    pat = kf.default_pattern()
    assert len(set(zip(pat["x1"].tolist(), pat["y1"].tolist(), pat["x2"].tolist(), pat["y2"].tolist()))) > 200
