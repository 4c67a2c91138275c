"""What the mirrors of the batched stages on their own handles share (loop.py, bow.py, keyframe.py, tracker.py, detect.py, equalize.py, reject.py, frontend.py, exrot.py, preint.py): binding
a library's entry points once, the handle object's life and error texts, and the pre-filled output arrays."""
import ctypes as C

import numpy as np

from . import backend

FILL = 0xA5                                # the pattern the output arrays are pre-filled with


def filled(rows, cols, dtype):
    """an output array [max(rows, 1)][cols] pre-filled with FILL bytes"""
    return np.full((max(rows, 1), cols * np.dtype(dtype).itemsize), FILL, dtype=np.uint8).view(dtype)


def untouched(a, used):
    """nothing is written past `used` rows"""
    return bool((a.view(np.uint8).reshape(len(a), -1)[used:] == FILL).all())


def bind_once(key):
    """decorates a module's _bind(lib), which sets its entry points' argument types: it runs once per library object"""
    def wrap(declare):
        def _bind(lib):
            if not getattr(lib, "_bound_" + key, False):
                declare(lib)
                setattr(lib, "_bound_" + key, True)
        return _bind
    return wrap


class StageHandle:
    """a handle of the C ABI behind a Python object.  PREFIX names its entry points (<PREFIX>_create, _destroy, _last_error,
    _last_ms); N_MS is the length of its last_ms tuple."""
    PREFIX, N_MS = None, 0

    def _create(self, bind, *args, why=""):
        """<PREFIX>_create(*args, &handle) on the loaded library; `why` ends the message of a failure"""
        self.lib = backend.load_library()
        bind(self.lib)
        self.h = C.c_void_p()
        rc = getattr(self.lib, self.PREFIX + "_create")(*args, C.byref(self.h))
        if rc != 0:
            self.h = None
            raise backend.BackendError(f"{self.PREFIX}_create: {backend.STATUS.get(rc, rc)}{why}")

    def close(self):
        if getattr(self, "h", None):
            getattr(self.lib, self.PREFIX + "_destroy")(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, entry, with_last_error=False):
        """raises for a failed call of `entry`: "<entry>: <STATUS>", with the handle's last error after it on request"""
        if rc == 0:
            return
        text = f"{entry}: {backend.STATUS.get(rc, rc)}"
        if with_last_error:
            msg = getattr(self.lib, self.PREFIX + "_last_error")(self.h)
            text += f" {msg.decode() if msg else ''}"
        raise backend.BackendError(text)

    def last_ms(self):
        ms = (C.c_double * self.N_MS)()
        self._check(getattr(self.lib, self.PREFIX + "_last_ms")(self.h, ms), self.PREFIX + "_last_ms")
        return tuple(ms)
