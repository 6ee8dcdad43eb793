"""ctypes binding of libddp_cm.so (include/ddp_cm_mi355x.h): the confusion matrix accumulated on the device.

NO fallback: ``_sidelib`` raises on a missing or stale library; build it with ``python -m ddp_amd.build``.
"""
import ctypes as C

from . import build as _build
from ._sidelib import Binding, SideLibError

ABI_VERSION = 1
MAX_ITEMS = 64
TALLY = 4
E_BADCFG, E_ALIGN, E_LAUNCH, E_NULL = -1, -2, -3, -4

_fp = C.c_void_p


class Item(C.Structure):
    _fields_ = [('d_pred', _fp), ('d_label', _fp), ('h', C.c_int32), ('w', C.c_int32)]


ARGTYPES = {
    'ddp_cm_workspace': [C.c_int, C.POINTER(C.c_size_t)],
    'ddp_cm_seg': [C.POINTER(Item), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp],
}
EXPORTS = ['ddp_cm_last_error', 'ddp_cm_abi_version', *ARGTYPES]


class DdpCmError(SideLibError):
    pass


_binding = Binding(_build.SIDE['cm'], ABI_VERSION, ARGTYPES, 'ddp_amd.confusion', DdpCmError)
load, check = _binding.load, _binding.check
