"""ctypes binding of libddp_eval.so (include/ddp_eval_mi355x.h): the pre_eval statistics reduced on the device.

NO fallback: ``_sidelib`` raises on a missing or stale library; build it with ``python -m ddp_amd.build``.
"""
import ctypes as C

from . import build as _build
from ._sidelib import Binding, SideLibError

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


ARGTYPES = {
    'ddp_eval_seg': [C.POINTER(SegItem), C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp],
    'ddp_eval_depth_workspace': [C.POINTER(DepthItem), C.c_int, C.POINTER(C.c_size_t)],
    'ddp_eval_depth': [C.POINTER(DepthItem), C.c_int, C.c_float, C.c_float, _fp, _fp, _fp],
    'ddp_eval_bev': [C.POINTER(BevItem), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, _fp, _fp],
}
EXPORTS = ['ddp_eval_last_error', 'ddp_eval_abi_version', *ARGTYPES]


class DdpEvalError(SideLibError):
    pass


_binding = Binding(_build.SIDE['eval'], ABI_VERSION, ARGTYPES, 'ddp_amd.evaluation', DdpEvalError)
load, check = _binding.load, _binding.check
