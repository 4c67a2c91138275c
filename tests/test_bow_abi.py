"""CPU checks of include/isvins_bow.h: the library exports every isv_bow_* it declares, the ctypes mirror has the header's struct
sizes, the handle fails loudly without a GPU and refuses bad configurations and bad vocabularies, and isv_bow_vocab_check (host
only) accepts what make_vocabulary writes and refuses every malformed file of tests/bow_cases.py: one file per case."""
import ctypes as C
import os
import subprocess

import pytest

import bow_cases
from isvins_amd import backend, bow, loop
from test_abi import ROOT, declared_functions

HEADER = os.path.join(ROOT, "include", "isvins_bow.h")


@pytest.fixture(scope="module")
def lib():
    backend.build()
    lib = backend.load_library()
    bow._bind(lib)
    return lib


def test_every_bow_symbol_is_exported(lib):
    names = [n for n in declared_functions(HEADER) if n.startswith("isv_bow_")]
    assert set(names) == set(bow.EXPORTS) and len(names) == 9 and len(names) == len(declared_functions(HEADER))
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/isvins_bow.h but not exported"
    # the new header adds nothing to the three whose export sets other tests pin, and loop.EXPORTS is as it was
    for other in ("isvins_backend.h", "isvins_posegraph.h", "isvins_loop.h"):
        assert not [n for n in declared_functions(os.path.join(ROOT, "include", other)) if n.startswith("isv_bow_")]
    assert len(loop.EXPORTS) == 6


def test_struct_sizes_match_header(tmp_path):
    structs = ["isv_bow_config_t", "isv_bow_item_t", "isv_bow_result_t", "isv_bow_vocab_info_t"]
    src = tmp_path / "szb.c"
    src.write_text('#include <stdio.h>\n#include "isvins_bow.h"\nint main(){' + "".join(f'printf("%zu\\n", sizeof({n}));' for n in structs) +
                   'printf("%d %d %d %d %d\\n", (int)ISV_BOW_DUPLICATE, (int)ISV_BOW_QUERY, ISV_ERR_INPUT, ISV_BOW_MAX_RESULTS, ISV_BOW_MAX_FEATURES); return 0;}')
    exe = tmp_path / "szb"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    for n, s in zip(structs, out):
        assert C.sizeof(getattr(bow, n)) == s, n
    assert out[4:] == [bow.ISV_BOW_DUPLICATE, bow.ISV_BOW_QUERY, bow.ISV_ERR_INPUT, bow.ISV_BOW_MAX_RESULTS, bow.ISV_BOW_MAX_FEATURES] == [3, 2, -6, 8, 8192]


def test_create_fails_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    vb = bow.make_vocabulary(1, 2, 1)
    with pytest.raises(backend.BackendError):
        bow.LoopDetector(vb, 4, 4)
    cfg, h = bow.make_config(4, 4), C.c_void_p()
    assert lib.isv_bow_create(C.byref(cfg), vb, len(vb), C.byref(h)) == -4 and not h.value


def test_create_rejects_bad_config_and_vocabulary(lib):
    h = C.c_void_p()
    vb = bow.make_vocabulary(1, 2, 1)
    assert lib.isv_bow_create(None, vb, len(vb), C.byref(h)) == -1
    assert lib.isv_bow_create(C.byref(bow.make_config()), vb, len(vb), None) == -1
    assert lib.isv_bow_create(C.byref(bow.make_config()), None, 0, C.byref(h)) == -1
    for bad in (dict(max_items=0), dict(n_databases=0), dict(max_features=0), dict(max_features=8193), dict(max_results=0), dict(max_results=9),
                dict(min_gap=-1), dict(initial_entry_capacity=0), dict(neighbour_score=float("nan")), dict(loop_score=float("inf"))):
        assert lib.isv_bow_create(C.byref(bow.make_config(**bad)), vb, len(vb), C.byref(h)) == -1, bad
        assert not h.value
    # a bad vocabulary is refused by its own status, before any device is looked for
    for name, (data, status) in bow_cases.malformed().items():
        if status != 0:
            assert lib.isv_bow_create(C.byref(bow.make_config()), data, len(data), C.byref(h)) == status, name
            assert not h.value
    assert lib.isv_bow_last_error(None) == b"null handle"
    assert lib.isv_bow_last_ms(None, (C.c_double * 5)()) == -1
    assert lib.isv_bow_detect_batch(None, 0, None, None, None, None) == -1
    assert lib.isv_bow_reset(None, 0) == -1 and lib.isv_bow_entries(None, 0) == -1


def test_vocab_check_accepts_make_vocabulary(lib):
    for name, vb in bow_cases.vocabularies().items():
        rc, info = bow.vocab_check(vb, lib)
        k, L, _, _, nodes, words = bow.unpack_vocabulary(vb)
        assert rc == 0, name
        assert (info.k, info.L, info.n_nodes, info.n_words, info.n_leaves) == (k, L, len(nodes), len(words), len(words)), name
        assert info.max_depth == L and info.n_stop_words == int((nodes["weight"][[list(nodes["id"]).index(n) for n in words["node"]]] == 0).sum()), name
    assert bow.vocab_check(bow_cases.vocabularies()["all_stop"], lib)[1].n_stop_words == 9
    info = bow.vocab_check(bow_cases.vocabularies()["leaf_above"], lib)[1]
    assert (info.n_nodes, info.n_words, info.max_depth) == (27, 19, 3)     # one level-1 leaf, two full depth-3 branches
    assert lib.isv_bow_vocab_check(None, 0, None) == -1 and lib.isv_bow_vocab_check_file(None, None) == -1


@pytest.mark.parametrize("name", sorted(bow_cases.malformed()))
def test_vocab_check_refuses_malformed_file(lib, tmp_path, name):
    data, status = bow_cases.malformed()[name]
    path = tmp_path / f"{name}.bin"
    path.write_bytes(data)
    info = bow.isv_bow_vocab_info_t()
    info.n_nodes = -77
    assert lib.isv_bow_vocab_check_file(str(path).encode(), C.byref(info)) == status
    assert lib.isv_bow_vocab_check(data, len(data), C.byref(info)) == status
    assert (info.n_nodes == -77) == (status != 0)        # info is written on ISV_OK only
    assert lib.isv_bow_vocab_check(data, len(data), None) == status


def test_vocab_check_file_missing(lib, tmp_path):
    assert lib.isv_bow_vocab_check_file(str(tmp_path / "absent.bin").encode(), None) == -1
