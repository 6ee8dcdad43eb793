"""ctypes binding of libddp_cm.so (include/ddp_cm_mi355x.h): the confusion matrix accumulated on the device.

Like ``_lib`` and ``_eval_lib``: NO fallback.  A missing or stale library raises; build it with ``python -m ddp_amd.build``.
"""
import ctypes as C
import os

from . import build as _build

ABI_VERSION = 1
MAX_ITEMS = 64
TALLY = 4
E_BADCFG, E_ALIGN, E_LAUNCH, E_NULL = -1, -2, -3, -4

_fp = C.c_void_p


class Item(C.Structure):
    _fields_ = [('d_pred', _fp), ('d_label', _fp), ('h', C.c_int32), ('w', C.c_int32)]


EXPORTS = ['ddp_cm_last_error', 'ddp_cm_abi_version', 'ddp_cm_workspace', 'ddp_cm_seg']

_libs = {}


class DdpCmError(RuntimeError):
    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def load(path=None):
    """Load (once per path) and return libddp_cm.so; raises when it is missing or was built from other sources."""
    path = os.path.abspath(path or _build.CM_LIB_PATH)
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise DdpCmError(f'{path} not found: build it with `python -m ddp_amd.build` (hipcc --offload-arch=gfx950); '
                         'ddp_amd.confusion has no non-HIP fallback')
    if path == os.path.abspath(_build.CM_LIB_PATH) and _build.cm_built_hash() != _build.cm_hash():
        raise DdpCmError(f'{path} is stale: built from sources {_build.cm_built_hash() or "<no stamp>"}, the tree holds '
                         f'{_build.cm_hash()}; rebuild with `python -m ddp_amd.build`')
    lib = C.CDLL(path)
    lib.ddp_cm_last_error.restype = C.c_char_p
    lib.ddp_cm_last_error.argtypes = []
    lib.ddp_cm_abi_version.restype = C.c_int
    lib.ddp_cm_abi_version.argtypes = []
    lib.ddp_cm_workspace.restype = C.c_int
    lib.ddp_cm_workspace.argtypes = [C.c_int, C.POINTER(C.c_size_t)]
    lib.ddp_cm_seg.restype = C.c_int
    lib.ddp_cm_seg.argtypes = [C.POINTER(Item), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp]
    if lib.ddp_cm_abi_version() != ABI_VERSION:
        raise DdpCmError(f'ABI mismatch: library {lib.ddp_cm_abi_version()} vs binding {ABI_VERSION}')
    _libs[path] = lib
    return lib


def check(rc, lib=None):
    if rc != 0:
        raise DdpCmError(f'libddp_cm error {rc}: {(lib or load()).ddp_cm_last_error().decode()}', rc)
