"""ctypes binding of libddp_lss.so (include/ddp_lss_mi355x.h): the LSSTransform lift and pool on the device.

NO fallback: ``_sidelib`` raises on a missing or stale library; build it with ``python -m ddp_amd.build``.
"""
import ctypes as C

from . import build as _build
from ._sidelib import Binding, SideLibError

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


_cfg = C.POINTER(Cfg)
ARGTYPES = {
    'ddp_lss_workspace': [_cfg, C.POINTER(C.c_size_t)],
    'ddp_lss_plan': [_cfg, _fp, _fp, _fp, _fp],
    'ddp_lss_plan_from_ranks': [_cfg, _fp, _fp, _fp],
    'ddp_lss_ranks': [_cfg, _fp, C.POINTER(_fp)],
    'ddp_lss_pool': [_cfg, _fp, _fp, _fp, _fp],
}
EXPORTS = ['ddp_lss_last_error', 'ddp_lss_abi_version', *ARGTYPES]


class DdpLssError(SideLibError):
    pass


# a refused configuration is the caller's ValueError, anything else a DdpLssError
_binding = Binding(_build.SIDE['lss'], ABI_VERSION, ARGTYPES, 'ddp_amd.lss', DdpLssError, badcfg=E_BADCFG)
load, check = _binding.load, _binding.check
