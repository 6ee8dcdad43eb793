"""ctypes binding of libddp_vox.so (include/ddp_vox_mi355x.h): hard voxelisation of lidar points with the reference's sequential
result - cell ids, voxel assignment, the per-sample outputs and the batched ones of ``BEVFusion.voxelize``.

NO fallback: ``_sidelib`` raises on a missing or stale library; build it with ``python -m ddp_amd.build``.
"""
import ctypes as C

from . import build as _build
from ._sidelib import Binding, SideLibError

ABI_VERSION = 1
WS_ALIGN = 256
MAX_FEATS, MAX_POINTS, SCAN_TILE, HASH_MULT = 16, 256, 1024, 2654435761
E_BADCFG, E_ALIGN, E_LAUNCH, E_NULL = -1, -2, -3, -4

_fp = C.c_void_p


class Cfg(C.Structure):
    _fields_ = [('batch', C.c_int32), ('pmax', C.c_int32), ('max_voxels', C.c_int32), ('max_points', C.c_int32), ('feats', C.c_int32),
                ('grid', C.c_int32 * 3), ('lo', C.c_float * 3), ('vs', C.c_float * 3)]


_cfg = C.POINTER(Cfg)
_points = [C.POINTER(_fp), C.POINTER(C.c_int32), C.c_int32]     # h_points, h_counts, stride
ARGTYPES = {
    'ddp_vox_workspace': [_cfg, C.POINTER(C.c_size_t)],
    'ddp_vox_cells': [_cfg, *_points, _fp, _fp],
    'ddp_vox_assign': [_cfg, _fp, _fp],
    'ddp_vox_assign_from_cells': [_cfg, _fp, _fp, _fp],
    'ddp_vox_tables': [_cfg, _fp] + [C.POINTER(_fp)] * 5,
    'ddp_vox_gather': [_cfg, *_points, _fp, _fp, _fp, _fp, _fp],
    'ddp_vox_pack': [_cfg, *_points, C.c_int32, _fp, _fp, _fp, _fp, _fp],
}
EXPORTS = ['ddp_vox_last_error', 'ddp_vox_abi_version', *ARGTYPES]


def hash_capacity(pmax):
    """H of the header: the smallest power of two >= 2 * pmax (at least 2)"""
    h = 2
    while h < 2 * pmax:
        h *= 2
    return h


def home_slot(cell, pmax):
    """the documented hash: the slot a cell id tries first in a sample's table of ``hash_capacity(pmax)`` slots"""
    h = hash_capacity(pmax)
    return ((int(cell) & 0xFFFFFFFF) * HASH_MULT & 0xFFFFFFFF) >> (32 - (h.bit_length() - 1))


class DdpVoxError(SideLibError):
    pass


# a refused configuration is the caller's ValueError, anything else a DdpVoxError
_binding = Binding(_build.LATER['vox'], ABI_VERSION, ARGTYPES, 'ddp_amd.vox', DdpVoxError, badcfg=E_BADCFG)
load, check = _binding.load, _binding.check
