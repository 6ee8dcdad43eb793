"""ctypes binding of libddp_dlss.so (include/ddp_dlss_mi355x.h): the front of DepthLSSTransform on the device - lidar projection,
deterministic depth scatter, dtransform stem.

Like ``_lib``, ``_eval_lib``, ``_cm_lib`` and ``_lss_lib``: NO fallback.  A missing or stale library raises; build it with
``python -m ddp_amd.build``.
"""
import ctypes as C
import os

from . import build as _build

ABI_VERSION = 1
WS_ALIGN = 256
STEM_MID, STEM_OUT, STEM_FOLDED = 8, 32, 6448
E_BADCFG, E_ALIGN, E_LAUNCH, E_NULL = -1, -2, -3, -4

_fp = C.c_void_p


class Cfg(C.Structure):
    _fields_ = [('batch', C.c_int32), ('cams', C.c_int32), ('image_h', C.c_int32), ('image_w', C.c_int32), ('pmax', C.c_int32)]


STEM_POINTERS = ['d_conv1_weight', 'd_conv1_bias', 'd_bn1_weight', 'd_bn1_bias', 'd_bn1_mean', 'd_bn1_var',
                 'd_conv2_weight', 'd_conv2_bias', 'd_bn2_weight', 'd_bn2_bias', 'd_bn2_mean', 'd_bn2_var']


class StemParams(C.Structure):
    _fields_ = [(n, _fp) for n in STEM_POINTERS] + [('bn1_eps', C.c_double), ('bn2_eps', C.c_double)]


EXPORTS = ['ddp_dlss_last_error', 'ddp_dlss_abi_version', 'ddp_dlss_workspace', 'ddp_dlss_project', 'ddp_dlss_pixels',
           'ddp_dlss_scatter', 'ddp_dlss_scatter_from_tables', 'ddp_dlss_stem']

_libs = {}


class DdpDlssError(RuntimeError):
    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def load(path=None):
    """Load (once per path) and return libddp_dlss.so; raises when it is missing or was built from other sources."""
    path = os.path.abspath(path or _build.DLSS_LIB_PATH)
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise DdpDlssError(f'{path} not found: build it with `python -m ddp_amd.build` (hipcc --offload-arch=gfx950); '
                           'ddp_amd.dlss has no non-HIP fallback')
    if path == os.path.abspath(_build.DLSS_LIB_PATH) and _build.dlss_built_hash() != _build.dlss_hash():
        raise DdpDlssError(f'{path} is stale: built from sources {_build.dlss_built_hash() or "<no stamp>"}, the tree holds '
                           f'{_build.dlss_hash()}; rebuild with `python -m ddp_amd.build`')
    lib = C.CDLL(path)
    cfg = C.POINTER(Cfg)
    lib.ddp_dlss_last_error.restype = C.c_char_p
    lib.ddp_dlss_last_error.argtypes = []
    lib.ddp_dlss_abi_version.restype = C.c_int
    lib.ddp_dlss_abi_version.argtypes = []
    lib.ddp_dlss_workspace.restype = C.c_int
    lib.ddp_dlss_workspace.argtypes = [cfg, C.POINTER(C.c_size_t)]
    lib.ddp_dlss_project.restype = C.c_int
    lib.ddp_dlss_project.argtypes = [cfg, C.POINTER(_fp), C.POINTER(C.c_int32), C.c_int32, _fp, _fp, _fp, _fp]
    lib.ddp_dlss_pixels.restype = C.c_int
    lib.ddp_dlss_pixels.argtypes = [cfg, _fp, C.POINTER(_fp), C.POINTER(_fp)]
    lib.ddp_dlss_scatter.restype = C.c_int
    lib.ddp_dlss_scatter.argtypes = [cfg, _fp, _fp, _fp]
    lib.ddp_dlss_scatter_from_tables.restype = C.c_int
    lib.ddp_dlss_scatter_from_tables.argtypes = [cfg, _fp, _fp, _fp, _fp, _fp]
    lib.ddp_dlss_stem.restype = C.c_int
    lib.ddp_dlss_stem.argtypes = [cfg, _fp, C.POINTER(StemParams), _fp, _fp, _fp]
    if lib.ddp_dlss_abi_version() != ABI_VERSION:
        raise DdpDlssError(f'ABI mismatch: library {lib.ddp_dlss_abi_version()} vs binding {ABI_VERSION}')
    _libs[path] = lib
    return lib


def check(rc, lib=None):
    if rc != 0:
        msg = (lib or load()).ddp_dlss_last_error().decode()
        if rc == E_BADCFG:
            raise ValueError(f'libddp_dlss refused the configuration: {msg}')
        raise DdpDlssError(f'libddp_dlss error {rc}: {msg}', rc)
