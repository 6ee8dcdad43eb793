"""ctypes binding of libddp_dlss.so (include/ddp_dlss_mi355x.h): the front of DepthLSSTransform on the device - lidar projection,
deterministic depth scatter, dtransform stem.

NO fallback: ``_sidelib`` raises on a missing or stale library; build it with ``python -m ddp_amd.build``.
"""
import ctypes as C

from . import build as _build
from ._sidelib import Binding, SideLibError

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


_cfg = C.POINTER(Cfg)
ARGTYPES = {
    'ddp_dlss_workspace': [_cfg, C.POINTER(C.c_size_t)],
    'ddp_dlss_project': [_cfg, C.POINTER(_fp), C.POINTER(C.c_int32), C.c_int32, _fp, _fp, _fp, _fp],
    'ddp_dlss_pixels': [_cfg, _fp, C.POINTER(_fp), C.POINTER(_fp)],
    'ddp_dlss_scatter': [_cfg, _fp, _fp, _fp],
    'ddp_dlss_scatter_from_tables': [_cfg, _fp, _fp, _fp, _fp, _fp],
    'ddp_dlss_stem': [_cfg, _fp, C.POINTER(StemParams), _fp, _fp, _fp],
}
EXPORTS = ['ddp_dlss_last_error', 'ddp_dlss_abi_version', *ARGTYPES]


class DdpDlssError(SideLibError):
    pass


# a refused configuration is the caller's ValueError, anything else a DdpDlssError
_binding = Binding(_build.SIDE['dlss'], ABI_VERSION, ARGTYPES, 'ddp_amd.dlss', DdpDlssError, badcfg=E_BADCFG)
load, check = _binding.load, _binding.check
