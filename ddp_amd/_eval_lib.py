"""ctypes binding of libddp_eval.so (include/ddp_eval_mi355x.h): the pre_eval statistics reduced on the device.

Like ``_lib``: NO fallback.  A missing or stale library raises; build it with ``python -m ddp_amd.build``.
"""
import ctypes as C
import os

from . import build as _build

ABI_VERSION = 1
MAX_ITEMS = 64
SEG_BINS = 256
DEPTH_COLS = 16
MAX_THRESHOLDS = 16
E_BADCFG, E_ALIGN, E_LAUNCH, E_NULL = -1, -2, -3, -4

_fp = C.c_void_p


class SegItem(C.Structure):
    _fields_ = [('d_pred', _fp), ('d_label', _fp), ('h', C.c_int32), ('w', C.c_int32)]


class DepthItem(C.Structure):
    _fields_ = [('d_pred', _fp), ('d_gt', _fp), ('h', C.c_int32), ('w', C.c_int32),
                ('y0', C.c_int32), ('y1', C.c_int32), ('x0', C.c_int32), ('x1', C.c_int32)]


class BevItem(C.Structure):
    _fields_ = [('d_prob', _fp), ('d_gt', _fp)]


EXPORTS = ['ddp_eval_last_error', 'ddp_eval_abi_version', 'ddp_eval_seg', 'ddp_eval_depth_workspace', 'ddp_eval_depth',
           'ddp_eval_bev']

_libs = {}


class DdpEvalError(RuntimeError):
    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def load(path=None):
    """Load (once per path) and return libddp_eval.so; raises when it is missing or was built from other sources."""
    path = os.path.abspath(path or _build.EVAL_LIB_PATH)
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise DdpEvalError(f'{path} not found: build it with `python -m ddp_amd.build` (hipcc --offload-arch=gfx950); '
                           'ddp_amd.evaluation has no non-HIP fallback')
    if path == os.path.abspath(_build.EVAL_LIB_PATH) and _build.eval_built_hash() != _build.eval_hash():
        raise DdpEvalError(f'{path} is stale: built from sources {_build.eval_built_hash() or "<no stamp>"}, the tree holds '
                           f'{_build.eval_hash()}; rebuild with `python -m ddp_amd.build`')
    lib = C.CDLL(path)
    lib.ddp_eval_last_error.restype = C.c_char_p
    lib.ddp_eval_last_error.argtypes = []
    lib.ddp_eval_abi_version.restype = C.c_int
    lib.ddp_eval_abi_version.argtypes = []
    lib.ddp_eval_seg.argtypes = [C.POINTER(SegItem), C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp]
    lib.ddp_eval_depth_workspace.argtypes = [C.POINTER(DepthItem), C.c_int, C.POINTER(C.c_size_t)]
    lib.ddp_eval_depth.argtypes = [C.POINTER(DepthItem), C.c_int, C.c_float, C.c_float, _fp, _fp, _fp]
    lib.ddp_eval_bev.argtypes = [C.POINTER(BevItem), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, _fp, _fp]
    for n in ('ddp_eval_seg', 'ddp_eval_depth_workspace', 'ddp_eval_depth', 'ddp_eval_bev'):
        getattr(lib, n).restype = C.c_int
    if lib.ddp_eval_abi_version() != ABI_VERSION:
        raise DdpEvalError(f'ABI mismatch: library {lib.ddp_eval_abi_version()} vs binding {ABI_VERSION}')
    _libs[path] = lib
    return lib


def check(rc, lib=None):
    if rc != 0:
        raise DdpEvalError(f'libddp_eval error {rc}: {(lib or load()).ddp_eval_last_error().decode()}', rc)
