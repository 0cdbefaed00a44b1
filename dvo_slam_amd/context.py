"""The device context: one GPU, one HIP stream and its scratch (dvo_hip_context); every other module of the binding starts here."""
import ctypes as C

from . import _lib
from ._lib import DvoHipError


class Context:
    """One device + one HIP stream + scratch (dvo_hip_context).  One per host thread."""

    def __init__(self, device=0):
        self._lib = _lib.lib()
        self.ptr = C.c_void_p()
        rc = self._lib.dvo_hip_context_create(device, C.byref(self.ptr))
        if rc != _lib.OK:
            raise DvoHipError(rc, self._lib.dvo_hip_last_error(None).decode())
        self.device = device

    def check(self, rc):
        if rc != _lib.OK:
            raise DvoHipError(rc, self._lib.dvo_hip_last_error(self.ptr).decode())

    def set_option(self, key, value):
        self.check(self._lib.dvo_hip_set_option(self.ptr, key.encode(), int(value)))

    def counter(self, key):
        """An event counter of the context ("resident_launches", "resident_timeouts")."""
        v = C.c_longlong(0)
        self.check(self._lib.dvo_hip_get_counter(self.ptr, key.encode(), C.byref(v)))
        return v.value

    @property
    def stream(self):
        return self._lib.dvo_hip_context_stream(self.ptr)

    def close(self):
        if getattr(self, "ptr", None):
            self._lib.dvo_hip_context_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_context = None


def default_context():
    global _default_context
    if _default_context is None:
        _default_context = Context(0)
    return _default_context
