"""ctypes binding of libddp_lss.so (include/ddp_lss_mi355x.h): the LSSTransform lift and pool on the device.

Like ``_lib``, ``_eval_lib`` and ``_cm_lib``: NO fallback.  A missing or stale library raises; build it with
``python -m ddp_amd.build``.
"""
import ctypes as C
import os

from . import build as _build

ABI_VERSION = 1
MAX_CHANNELS = 256
MAX_DEPTH_BINS = 512
WS_ALIGN = 256
E_BADCFG, E_ALIGN, E_LAUNCH, E_NULL = -1, -2, -3, -4

_fp = C.c_void_p


class Cfg(C.Structure):
    _fields_ = [('batch', C.c_int32), ('cams', C.c_int32), ('depth_bins', C.c_int32), ('feat_h', C.c_int32), ('feat_w', C.c_int32),
                ('channels', C.c_int32), ('image_h', C.c_int32), ('image_w', C.c_int32),
                ('dbound', C.c_double * 3), ('xbound', C.c_double * 3), ('ybound', C.c_double * 3), ('zbound', C.c_double * 3),
                ('nx', C.c_int32 * 3)]


EXPORTS = ['ddp_lss_last_error', 'ddp_lss_abi_version', 'ddp_lss_workspace', 'ddp_lss_plan', 'ddp_lss_plan_from_ranks',
           'ddp_lss_ranks', 'ddp_lss_pool']

_libs = {}


class DdpLssError(RuntimeError):
    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def load(path=None):
    """Load (once per path) and return libddp_lss.so; raises when it is missing or was built from other sources."""
    path = os.path.abspath(path or _build.LSS_LIB_PATH)
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise DdpLssError(f'{path} not found: build it with `python -m ddp_amd.build` (hipcc --offload-arch=gfx950); '
                          'ddp_amd.lss has no non-HIP fallback')
    if path == os.path.abspath(_build.LSS_LIB_PATH) and _build.lss_built_hash() != _build.lss_hash():
        raise DdpLssError(f'{path} is stale: built from sources {_build.lss_built_hash() or "<no stamp>"}, the tree holds '
                          f'{_build.lss_hash()}; rebuild with `python -m ddp_amd.build`')
    lib = C.CDLL(path)
    cfg = C.POINTER(Cfg)
    lib.ddp_lss_last_error.restype = C.c_char_p
    lib.ddp_lss_last_error.argtypes = []
    lib.ddp_lss_abi_version.restype = C.c_int
    lib.ddp_lss_abi_version.argtypes = []
    lib.ddp_lss_workspace.restype = C.c_int
    lib.ddp_lss_workspace.argtypes = [cfg, C.POINTER(C.c_size_t)]
    lib.ddp_lss_plan.restype = C.c_int
    lib.ddp_lss_plan.argtypes = [cfg, _fp, _fp, _fp, _fp]
    lib.ddp_lss_plan_from_ranks.restype = C.c_int
    lib.ddp_lss_plan_from_ranks.argtypes = [cfg, _fp, _fp, _fp]
    lib.ddp_lss_ranks.restype = C.c_int
    lib.ddp_lss_ranks.argtypes = [cfg, _fp, C.POINTER(_fp)]
    lib.ddp_lss_pool.restype = C.c_int
    lib.ddp_lss_pool.argtypes = [cfg, _fp, _fp, _fp, _fp]
    if lib.ddp_lss_abi_version() != ABI_VERSION:
        raise DdpLssError(f'ABI mismatch: library {lib.ddp_lss_abi_version()} vs binding {ABI_VERSION}')
    _libs[path] = lib
    return lib


def check(rc, lib=None):
    if rc != 0:
        msg = (lib or load()).ddp_lss_last_error().decode()
        if rc == E_BADCFG:
            raise ValueError(f'libddp_lss refused the configuration: {msg}')
        raise DdpLssError(f'libddp_lss error {rc}: {msg}', rc)
