"""The stage mirrors bind a library's entry points once per library object (is-vins_amd/_stage.py), not once per process: binding
one library must not make another look bound."""
import types

import pytest

from isvins_amd import _stage, bow, detect, keyframe, loop, tracker


class FakeLib:
    """a stand-in library: every public name is an entry point whose argtypes / restype can be set"""

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        f = types.SimpleNamespace(argtypes=None)
        setattr(self, name, f)
        return f


def test_bind_once_is_per_library():
    calls = []
    bind = _stage.bind_once("probe")(calls.append)
    a, b = FakeLib(), FakeLib()
    bind(a); bind(a)
    assert calls == [a]
    bind(b); bind(b); bind(a)
    assert calls == [a, b]


@pytest.mark.parametrize("mod", [loop, bow, keyframe, tracker, detect], ids=lambda m: m.__name__.split(".")[-1])
def test_each_mirror_binds_a_second_library(mod):
    a, b = FakeLib(), FakeLib()
    mod._bind(a)
    assert all(getattr(a, n).argtypes is not None for n in mod.EXPORTS if n in vars(a))
    assert vars(a) and not vars(b)                          # binding the first left the second alone
    mod._bind(b)
    assert {k for k in vars(a)} == {k for k in vars(b)}
    for n, f in vars(b).items():
        if not n.startswith("_"):
            assert f.argtypes == getattr(a, n).argtypes, n
