"""DDP_FLAG_SEEDED_NOISE: a NumPy restatement of the generator of csrc/ddp_noise.hip and the cases the two test files share.

Philox4x32-10 (Salmon et al., SC'11) in uint64 arithmetic, Box-Muller in fp64 on the same exact uniforms the kernels use:
  key = (seed_lo, seed_hi), counter = (e >> 2, image, stream, call), the element's value = output lane e & 3
  u = ((x >> 9) + 0.5) * 2^-23;  lanes (0, 1) = sqrt(-2 ln u0) * (cos, sin)(2 pi u1) from words (0, 1), lanes (2, 3) from words (2, 3)
"""
import numpy as np

import config_space_cases as S
from support import round256

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
SH = np.uint64(32)

# Seed of the GPU tests.  Chosen on the CPU (scan 2024, 2025, ...: the first whose first 10^5 values of image 0 pass the moment
# conditions of tests/test_seeded_noise_host.py with room to spare); a condition on the seed, not a measurement
SEED = 2024
SEED_B = 0x1234567800000007      # a second seed that uses the high key word


def philox4x32_10(counter, key):
    """counter (..., 4), key (2,) or (..., 2) uint32-valued -> (..., 4) uint32 words as uint64"""
    c = [np.asarray(counter[..., i], dtype=np.uint64) for i in range(4)]
    key = np.asarray(key, dtype=np.uint64)
    k0, k1 = key[..., 0], key[..., 1]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                  # < 2^64: both factors are below 2^32
        c = [(p1 >> SH) ^ c[1] ^ k0, p1 & MASK, (p0 >> SH) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, axis=-1)


def key_of(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)


def normals(seed, image, stream, call, n):
    """the first n values of (seed, image, stream, call) -> (values fp64 (n,), rad fp64 (n,): the Box-Muller radius of each value's pair)"""
    groups = (n + 3) // 4
    ctr = np.zeros((groups, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(groups, dtype=np.uint64)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = np.uint64(image & 0xFFFFFFFF), np.uint64(stream & 0xFFFFFFFF), np.uint64(call & 0xFFFFFFFF)
    x = philox4x32_10(ctr, key_of(seed))
    u = ((x >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    rad = np.sqrt(-2.0 * np.log(u[:, 0::2]))           # (groups, 2): words 0 and 2
    ang = 2.0 * np.pi * u[:, 1::2]                     # words 1 and 3
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1).reshape(groups, 4)
    return z.reshape(-1)[:n], np.repeat(rad, 2, axis=1).reshape(-1)[:n]


def noise_ref(seed, image_base, stream, call, B, per_image):
    """(B, per_image) fp64 values and radii of a call: image b is (seed, image_base + b, stream, call)"""
    zs, rs = zip(*[normals(seed, image_base + b, stream, call, per_image) for b in range(B)])
    return np.stack(zs), np.stack(rs)


BOUND_UNIT = 8 * 2.0 ** -23      # |gpu - ref| <= BOUND_UNIT * max(1, rad): ~1 ulp logf, ~2 ulp sincospif, correctly rounded sqrtf and
                                 # products, |z| <= 5.77 (the issue's derivation)

# ---- the cases of tests/test_seeded_noise_gpu.py (shapes of tests/test_step_record_gpu.py, on tests/config_space_cases.py) ------------
_SEG = dict(S.CASES['seg_L12'], L=2, h=7, w=13, K=3, seed=900)          # 7 x 13: w % 4 != 0, counter groups straddle rows
_DEPTH = dict(S.CASES['depth_K1'], L=2, K=4)
_BEV = dict(S.CASES['bev_kc5_th0.3'], L=2, K=3, h=5, w=9, threshold=0.5, Kc=6)
CASES = {
    # name: (case, engine flags); every task at r in {1, 2} and B in {1, 3}
    'seg_fused': (dict(_SEG, B=3), {}),                                   # head7 reads the generated NCHW buffer itself
    'seg_unfused_tail': (dict(_SEG, B=1), dict(fused_tail=False)),
    'seg_r2_cx96': (dict(_SEG, r=2, Cx=96), {}),                          # prologue path: launch_nchw_to_sb
    'seg_f32': (dict(_SEG, B=1, r=2), dict(gemm='f32')),                  # launch_nchw_to_tok
    'seg_ddpm': (dict(_SEG, sampler='ddpm', r=2, B=3), {}),
    'seg_ddpm_f32': (dict(_SEG, sampler='ddpm', r=1, B=1), dict(gemm='f32')),
    'depth_chain': (dict(_DEPTH, h=5, w=9, B=1), {}),                     # Cm = 1: 45 values per image, the last counter in part
    'depth_chain_1x37': (dict(_DEPTH, h=1, w=37, B=3), {}),
    'depth_unfused': (dict(_DEPTH, h=5, w=9, B=3), dict(fused_tail=False)),
    'depth_r2': (dict(_DEPTH, h=5, w=9, r=2), {}),                        # 90 values per image
    'depth_f32': (dict(_DEPTH, h=1, w=37, r=2, B=3), dict(gemm='f32')),
    'bev_chain': (dict(_BEV, B=3), {}),
    'bev_chain_r2': (dict(_BEV, r=2, B=1), {}),
    'bev_unfused_tail': (dict(_BEV, B=1), dict(fused_tail=False)),
    'bev_f32': (dict(_BEV, r=2, B=3), dict(gemm='f32')),
}
for _n, (_c, _f) in CASES.items():
    _c['name'] = 'seeded_noise_' + _n
PATHS = {'seg_fused': 'seg_head7', 'seg_r2_cx96': 'seg_prologue', 'seg_unfused_tail': 'seg_unfused_tail_head7',
         'depth_chain': 'depth_chain', 'depth_r2': 'depth_lt', 'depth_unfused': 'depth_unfused_tail', 'bev_chain': 'bev_chain',
         'bev_unfused_tail': 'bev_separate'}
# the FCN loop (ddp_sample_fcn): 7 x 13, K = 3
FCN_CASES = {'fcn_ddim': dict(h=7, w=13, K=3, r=1, B=3, sampler='ddim', Kc=19, num_convs=1),
             'fcn_ddim_r2': dict(h=7, w=13, K=3, r=2, B=1, sampler='ddim', Kc=19, num_convs=2),
             'fcn_ddpm': dict(h=7, w=13, K=3, r=2, B=1, sampler='ddpm', Kc=19, num_convs=1)}


def cm_of(c):
    return 1 if c.get('task') == 'depth' else 256


def per_image(c):
    return c['r'] * cm_of(c) * c['h'] * c['w']


def noise_bytes(c):
    return round256(c['B'] * per_image(c) * 4)


def fcn_cfg(c, flags=0):
    from ddp_amd import _lib
    cfg = _lib.DdpCfg()
    cfg.abi_version = _lib.ABI_VERSION
    cfg.task = _lib.TASK_SEG
    cfg.sampler = _lib.SAMPLER_DDPM if c['sampler'] == 'ddpm' else _lib.SAMPLER_DDIM
    cfg.batch, cfg.randsteps, cfg.timesteps, cfg.num_layers = c['B'], c['r'], c['K'], 0
    cfg.num_classes, cfg.feat_channels = c['Kc'], 256
    cfg.h = cfg.head_h = c['h']
    cfg.w = cfg.head_w = c['w']
    cfg.gemm_mode, cfg.flags = _lib.GEMM_BF16X3, flags
    cfg.accumulation, cfg.bit_scale = 1, 0.01
    return cfg
