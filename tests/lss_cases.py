"""Cases of the device-side LSS lift and pool (include/ddp_lss_mi355x.h, ddp_amd/lss.py) and the restatements they are checked
against.  Device-free: numpy and CPU torch only.

  ``CASES`` / ``case(name)``   geometry + a nuScenes-like rig (six yaws, focal ~1266, post_rot 0.48 I, post_trans (-32, -176, 0)) + inputs
  ``SYNTH`` / ``synth(name)``  chosen rank tables for ``plan_from_ranks`` (exact list lengths, 1025 scan tiles) + inputs; no geometry
  ``geometry_f32``             the fp32 chain of the reference's ``get_geometry`` as torch CPU ops -> (B, N, D, fH, fW, 3)
  ``cells_f64``                the same chain in float64 -> the cell coordinate q per axis, before truncation
  ``ranks_of``                 q -> int32 ranks with truncation toward zero (``mode='trunc'``, what ``.long()`` does) or ``floor``
  ``pool_f64``                 the pooled sum in float64 over a given rank table, with the terms of the error bound
"""
import itertools
import math

import numpy as np
import torch

DELTA = 1e-3               # a fp64 cell coordinate this close to an integer excuses the point's rank (either side)
EXCUSED_SHARE = 0.01       # at most this share of a case's points may be excused

# name -> geometry.  bounds are (lo, hi, step); feature (fH, fW); image (iH, iW).  `pitch`: degrees per camera (up positive).
CASES = {
    'tiny': dict(B=1, yaws=[0.0], pitch=[0.0], feature=(1, 1), image=(256, 704), C=1, in_channels=2, dbound=(2.0, 6.0, 2.0),
                 xbound=(2.5, 6.5, 2.0), ybound=(0.0, 2.0, 1.0), zbound=(-10.0, 10.0, 20.0), cam_radius=0.0, faces=['y+'], longest=1),
    'odd': dict(B=2, yaws=[0.0, 120.0, 240.0], pitch=[15.0, -25.0, 0.0], feature=(5, 7), image=(256, 704), C=8, in_channels=5,
                dbound=(1.0, 40.0, 3.0), xbound=(-16.0, 16.0, 2.0), ybound=(-16.0, 16.0, 2.0), zbound=(-4.0, 4.0, 4.0), longest=2),
    'c3': dict(B=1, yaws=[30.0, 210.0], pitch=[20.0, -30.0], feature=(3, 4), image=(256, 704), C=3, in_channels=4,
               dbound=(1.0, 31.0, 6.0), xbound=(-8.0, 8.0, 2.0), ybound=(-8.0, 8.0, 2.0), zbound=(-3.0, 3.0, 6.0), longest=1),
    'cfg': dict(B=1, yaws=[0.0, 55.0, -55.0, 180.0, 110.0, -110.0], pitch=[0.0, 45.0, 0.0, -28.0, 0.0, 0.0], feature=(4, 11),
                image=(256, 704), C=80, in_channels=8, dbound=(1.0, 60.0, 0.5), xbound=(-51.2, 51.2, 3.2), ybound=(-51.2, 51.2, 3.2),
                zbound=(-10.0, 10.0, 20.0), longest=65),
    'long': dict(same_points_as='cfg', xbound=(0.0, 40.0, 20.0), ybound=(0.0, 60.0, 30.0), longest=1000),
    'runs': dict(B=1, yaws=[0.0, 90.0, 180.0, 270.0], pitch=[10.0, -25.0, 18.0, -20.0], feature=(3, 5), image=(256, 704), C=8,
                 in_channels=3, dbound=(1.5, 46.5, 5.0), xbound=(-12.0, 12.0, 3.0), ybound=(-20.0, 20.0, 1.0), zbound=(-4.0, 4.0, 8.0),
                 longest=1),
    'empty': dict(B=1, yaws=[0.0, 180.0], pitch=[0.0, 0.0], feature=(2, 3), image=(256, 704), C=4, in_channels=3,
                  dbound=(1.0, 21.0, 4.0), xbound=(500.0, 532.0, 2.0), ybound=(500.0, 532.0, 2.0), zbound=(-10.0, 10.0, 20.0), longest=0),
    # past the first tile of each tiling of ddp_lss.hip: K = 4230 cells (five scan tiles of 1024, K % 4 = 2), 135 pixels (three
    # pre-pass tiles of 64, the last of 7)
    'tiles': dict(B=2, yaws=[0.0, 120.0, 240.0], pitch=[5.0, -15.0, 0.0], feature=(9, 15), image=(256, 704), C=5, in_channels=4,
                  dbound=(1.0, 61.0, 6.0), xbound=(-22.5, 22.5, 1.0), ybound=(-23.5, 23.5, 1.0), zbound=(-10.0, 10.0, 20.0), longest=100),
    # three and four channel groups of 64 in the pool; nz = 2, so that the fixtures stay small (no downsample = 2 variant)
    'c129': dict(B=1, yaws=[45.0, 225.0], pitch=[10.0, -20.0], feature=(5, 13), image=(256, 704), C=129, in_channels=3,
                 dbound=(1.0, 31.0, 5.0), xbound=(-8.0, 8.0, 4.0), ybound=(-9.0, 9.0, 2.0), zbound=(-4.0, 4.0, 4.0), longest=65),
    'c256': dict(B=1, yaws=[25.0, -155.0], pitch=[14.0, -16.0], feature=(8, 9), image=(256, 704), C=256, in_channels=3,
                 dbound=(1.2, 49.2, 8.0), xbound=(-9.0, 9.0, 6.0), ybound=(-17.5, 17.5, 1.0), zbound=(-4.0, 4.0, 4.0), longest=48),
}
NAMES = list(CASES)             # a case's seeds follow its place here: new cases are appended
ALL_FACES = ['x-', 'x+', 'y-', 'y+', 'z-', 'z+']
LSS_RUN = 32               # the pooling block's run of iy cells (ddp_lss.hip)


def spec(name):
    s = dict(CASES[name])
    if 'same_points_as' in s:
        s = dict(CASES[s.pop('same_points_as')], **s)
    s.setdefault('faces', ALL_FACES)
    s.setdefault('cam_radius', 1.5)
    return s


def _rot_z(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _camera2lidar(yaw, pitch, radius, height):
    """camera axes (x right, y down, z forward) in a lidar frame (x forward, y left, z up), looking along ``yaw`` raised by ``pitch``"""
    cy, sy = math.cos(math.radians(yaw)), math.sin(math.radians(yaw))
    cp, sp = math.cos(math.radians(pitch)), math.sin(math.radians(pitch))
    fwd = np.array([cy * cp, sy * cp, sp])
    right = np.array([sy, -cy, 0.0])
    down = np.cross(fwd, right)
    m = np.eye(4)
    m[:3, :3] = np.stack([right, down, fwd], axis=1)
    m[:3, 3] = [radius * cy, radius * sy, height]
    return m


_cache = {}


def case(name):
    """-> dict: the constructor kwargs (``kwargs``), the forward inputs as CPU fp32 tensors (``img`` (B, N, Cin, fH, fW) and the 4 x 4
    matrices), B, N, D, C, nx.  Built once per name and never modified."""
    if name in _cache:
        return _cache[name]
    s = spec(name)
    src = CASES[name].get('same_points_as', name)
    rng = np.random.default_rng(1000 + NAMES.index(src))
    B, N = s['B'], len(s['yaws'])
    fH, fW = s['feature']
    c2l = np.zeros((B, N, 4, 4))
    intr = np.zeros((B, N, 4, 4))
    aug = np.zeros((B, N, 4, 4))
    laug = np.zeros((B, 4, 4))
    for b in range(B):
        for n, (yaw, pitch) in enumerate(zip(s['yaws'], s['pitch'])):
            c2l[b, n] = _camera2lidar(yaw + 0.7 * b, pitch, s['cam_radius'], 1.5 if s['cam_radius'] else 0.0)
            intr[b, n] = np.eye(4)
            intr[b, n, 0, 0] = 1266.4 + 3.0 * n
            intr[b, n, 1, 1] = 1266.4 + 3.0 * n
            intr[b, n, 0, 2], intr[b, n, 1, 2] = 816.3 - 5.0 * n, 491.5 + 2.0 * b
            aug[b, n] = np.eye(4)
            aug[b, n, 0, 0] = aug[b, n, 1, 1] = 0.48
            aug[b, n, :3, 3] = [-32.0, -176.0, 0.0]
        laug[b] = np.eye(4)
        if s['cam_radius']:
            laug[b, :3, :3] = _rot_z(3.0 + 2.0 * b) * (1.0 + 0.02 * b)
            laug[b, :3, 3] = [0.3, -0.2 - 0.1 * b, 0.1]
    f32 = lambda a: torch.from_numpy(a.astype(np.float32))
    img = torch.from_numpy(rng.uniform(-1.0, 1.0, (B, N, s['in_channels'], fH, fW)).astype(np.float32))
    kwargs = dict(in_channels=s['in_channels'], out_channels=s['C'], image_size=s['image'], feature_size=s['feature'],
                  xbound=list(s['xbound']), ybound=list(s['ybound']), zbound=list(s['zbound']), dbound=list(s['dbound']))
    nx = [int(v) for v in torch.LongTensor([(r[1] - r[0]) / r[2] for r in (s['xbound'], s['ybound'], s['zbound'])])]
    D = int(torch.arange(*s['dbound'], dtype=torch.float).shape[0])
    c = dict(name=name, spec=s, kwargs=kwargs, img=img, camera2lidar=f32(c2l), camera_intrinsics=f32(intr), img_aug_matrix=f32(aug),
             lidar_aug_matrix=f32(laug), B=B, N=N, D=D, C=s['C'], nx=nx, fH=fH, fW=fW, P=B * N * D * fH * fW, K=B * nx[2] * nx[0] * nx[1])
    _cache[name] = c
    return c


# ---- synthetic cases: a chosen rank table for ``plan_from_ranks``, no geometry, no fixture, no plugin run; not in NAMES ----------------
# list length by cell on a 3 x 37 x 1 grid (K = 111, K % 4 = 3): 1..5 around the four rows the pool keeps in flight, 63 / 64 / 65 and
# 127 / 128 / 129 around the 64 entries a wave takes at a time; 36 and 37 are the last cell of row ix = 0 and the first of row ix = 1;
# 108, 109 and 110 are the three counts of the scan's scalar tail
LENS = {0: 1, 1: 2, 2: 3, 3: 4, 4: 5, 31: 7, 32: 8, 36: 63, 37: 64, 73: 65, 74: 127, 107: 128, 108: 129, 109: 1, 110: 3}
# 1025 scan tiles of 1024 cells, the last of 3: the one-block scan of the tile sums takes two values per thread.  The named cells sit
# on either side of the first tile boundary and of the last, and in the last tile's scalar tail.
SCAN_NX1 = 1024 * 1024 + 3
SCAN_CELLS = {0: 2, 1023: 1, 1024: 3, SCAN_NX1 - 4: 1, SCAN_NX1 - 3: 2, SCAN_NX1 - 2: 1, SCAN_NX1 - 1: 5}
SCAN_SINGLES = 600         # further cells, drawn by the seed, of one point each
_lens = lambda C: dict(C=C, D=16, feature=(8, 9), nx=[3, 37, 1], lens=LENS, singles=0, table_seed=2000)
SYNTH = {
    'lens_c64': _lens(64), 'lens_c65': _lens(65), 'lens_c128': _lens(128), 'lens_c192': _lens(192), 'lens_c193': _lens(193),
    'scan': dict(C=1, D=4, feature=(32, 32), nx=[1, SCAN_NX1, 1], lens=SCAN_CELLS, singles=SCAN_SINGLES, table_seed=2001),
}
SYNTH_NAMES = list(SYNTH)


def synth(name):
    """-> dict with the keys ``pool_f64``, ``pool_bound`` and ``workspace_bytes`` read (and ``spec``, whose bounds make ``LssPool``
    derive the stated nx and D), plus ``ranks`` (P,) int32 and the pool's input ``x`` (B * N, D + C, fH, fW) fp32 in [-2, 2): a
    logit range of at most 4.  B = N = 1.  The points are dealt to the cells through a seeded permutation of the point ids, so no
    list is a run of consecutive ids; every other point is dropped (-1).  Built once per name and never modified."""
    if name in _cache:
        return _cache[name]
    s = SYNTH[name]
    fH, fW = s['feature']
    D, C = s['D'], s['C']
    bounds = dict(xbound=(0.0, float(s['nx'][0]), 1.0), ybound=(0.0, float(s['nx'][1]), 1.0), zbound=(0.0, float(s['nx'][2]), 1.0),
                  dbound=(1.0, 1.0 + D, 1.0))
    nx = [int(v) for v in torch.LongTensor([(r[1] - r[0]) / r[2] for r in (bounds['xbound'], bounds['ybound'], bounds['zbound'])])]
    assert nx == s['nx'] and int(torch.arange(*bounds['dbound'], dtype=torch.float).shape[0]) == D
    P, K = D * fH * fW, nx[2] * nx[0] * nx[1]
    rng = np.random.default_rng(s['table_seed'])
    lens = dict(s['lens'])
    free = np.setdiff1d(np.arange(K), np.fromiter(lens, dtype=np.int64))
    lens.update((int(cell), 1) for cell in rng.choice(free, s['singles'], replace=False))
    order = rng.permutation(P)
    ranks = np.full(P, -1, dtype=np.int32)
    at = 0
    for cell, n in lens.items():
        ranks[order[at:at + n]] = cell
        at += n
    assert at <= P
    x = np.random.default_rng(3000 + SYNTH_NAMES.index(name)).uniform(-2.0, 2.0, (1, D + C, fH, fW)).astype(np.float32)
    c = dict(name=name, spec=dict(bounds, image=(256, 704), feature=(fH, fW), lens=lens), B=1, N=1, D=D, C=C, nx=nx, fH=fH, fW=fW, P=P, K=K,
             ranks=ranks, x=torch.from_numpy(x))
    _cache[name] = c
    return c


def forward_args(c, dev=None):
    """the positional arguments of ``LSSTransform.forward``; ``camera2ego`` and ``lidar2ego`` are sliced by the reference but
    never used: identities; the others it ignores are None"""
    mv = (lambda t: t.to(dev)) if dev is not None else (lambda t: t)
    eye = torch.eye(4)
    return (mv(c['img']), None, mv(eye.expand(c['B'], c['N'], 4, 4)), mv(eye.expand(c['B'], 4, 4)), None, None, mv(c['camera_intrinsics']),
            mv(c['camera2lidar']), mv(c['img_aug_matrix']), mv(c['lidar_aug_matrix']), None)


def frustum_f32(c):
    """(D, fH, fW, 3) fp32 of (xs[w], ys[h], ds[d]), the reference's ``create_frustum`` expressions"""
    s = c['spec']
    iH, iW = s['image']
    ds = torch.arange(*s['dbound'], dtype=torch.float).view(-1, 1, 1).expand(-1, c['fH'], c['fW'])
    xs = torch.linspace(0, iW - 1, c['fW'], dtype=torch.float).view(1, 1, -1).expand(c['D'], c['fH'], c['fW'])
    ys = torch.linspace(0, iH - 1, c['fH'], dtype=torch.float).view(1, -1, 1).expand(c['D'], c['fH'], c['fW'])
    return torch.stack((xs, ys, ds), -1)


def _parts(c, dtype):
    t = lambda m: m.to(dtype)
    c2l, intr, aug, laug = t(c['camera2lidar']), t(c['camera_intrinsics']), t(c['img_aug_matrix']), t(c['lidar_aug_matrix'])
    return (c2l[..., :3, :3], c2l[..., :3, 3], intr[..., :3, :3], aug[..., :3, :3], aug[..., :3, 3], laug[..., :3, :3], laug[..., :3, 3])


def _chain(c, dtype):
    """steps 1-7 of ``get_geometry`` in ``dtype`` on the fp32 frustum and fp32 matrices -> (B, N, D, fH, fW, 3)"""
    rots, trans, intr, post_rots, post_trans, extra_rots, extra_trans = _parts(c, dtype)
    B, N = c['B'], c['N']
    pts = frustum_f32(c).to(dtype) - post_trans.view(B, N, 1, 1, 1, 3)
    pts = torch.inverse(post_rots).view(B, N, 1, 1, 1, 3, 3).matmul(pts.unsqueeze(-1))
    pts = torch.cat((pts[..., :2, :] * pts[..., 2:3, :], pts[..., 2:3, :]), -2)
    pts = rots.matmul(torch.inverse(intr)).view(B, N, 1, 1, 1, 3, 3).matmul(pts).squeeze(-1)
    pts = pts + trans.view(B, N, 1, 1, 1, 3)
    pts = extra_rots.view(B, 1, 1, 1, 1, 3, 3).matmul(pts.unsqueeze(-1)).squeeze(-1)
    return pts + extra_trans.view(B, 1, 1, 1, 1, 3)


def geometry_f32(c):
    return _chain(c, torch.float32)


def grid_f32(c):
    s = c['spec']
    rows = [s['xbound'], s['ybound'], s['zbound']]
    dx = torch.Tensor([r[2] for r in rows])
    bx = torch.Tensor([r[0] + r[2] / 2.0 for r in rows])
    return dx, bx


def cells_f32(c, geom=None):
    """the fp32 cell coordinate before ``.long()``: (P, 3) fp32"""
    dx, bx = grid_f32(c)
    g = geometry_f32(c) if geom is None else geom
    return ((g - (bx - dx / 2.0)) / dx).reshape(-1, 3).numpy()


def cells_f64(c):
    """the cell coordinate in float64: the chain in float64, the fp32 grid parameters widened: (P, 3) float64"""
    dx, bx = grid_f32(c)
    lo = (bx - dx / 2.0).double()
    return ((_chain(c, torch.float64) - lo) / dx.double()).reshape(-1, 3).numpy()


def ranks_of(c, q, mode='trunc'):
    """q (P, 3) cell coordinates -> (ranks int32 (P,), kept bool (P,)); ``trunc`` is ``.long()``, ``floor`` the mutation"""
    q = np.asarray(q, dtype=np.float64)
    finite = np.isfinite(q).all(1)
    qs = np.where(np.isfinite(q), q, -5.0)
    i = (np.trunc(qs) if mode == 'trunc' else np.floor(qs)).clip(-2 ** 40, 2 ** 40).astype(np.int64)
    nx = np.array(c['nx'], dtype=np.int64)
    kept = finite & (i >= 0).all(1) & (i < nx).all(1)
    b = np.arange(c['P'], dtype=np.int64) // (c['P'] // c['B'])
    r = ((b * nx[2] + i[:, 2]) * nx[0] + i[:, 0]) * nx[1] + i[:, 1]
    return np.where(kept, r, -1).astype(np.int32), kept


def near_boundary(q64):
    """points whose fp64 cell coordinate lies within DELTA of an integer on some axis"""
    return (np.abs(q64 - np.rint(q64)) <= DELTA).any(1)


def admissible(c, q64, got):
    """True per point where ``got`` is the fp64 rank, or - for a point within DELTA of a cell boundary - the rank on either side of
    that boundary (the grid's edge included)"""
    got = np.asarray(got).reshape(-1)
    k = np.rint(q64)
    near = np.abs(q64 - k) <= DELTA
    ok = np.zeros(got.shape, dtype=bool)
    for combo in itertools.product((-0.5, 0.5), repeat=3):
        ok |= ranks_of(c, np.where(near, k + np.array(combo), q64))[0] == got
    return ok


def depthnet_out(c, weight, bias):
    """the 1 x 1 convolution in fp32 on the CPU: (B * N, D + C, fH, fW)"""
    x = c['img'].view(c['B'] * c['N'], -1, c['fH'], c['fW'])
    return torch.nn.functional.conv2d(x, torch.as_tensor(weight), torch.as_tensor(bias))


def pool_f64(c, x, ranks):
    """x (B * N, D + C, fH, fW) fp32, ranks (P,) -> out (B, nz * C, nx0, nx1) float64, absum (the same shape: sum |p64 * f|), and
    L (K,) list lengths.  Point p = (((b N + n) D + d) fH + h) fW + w."""
    D, C = c['D'], c['C']
    x = np.asarray(x, dtype=np.float64)
    logit = x[:, :D]
    e = np.exp(logit - logit.max(1, keepdims=True))
    prob = (e / e.sum(1, keepdims=True)).reshape(-1)                       # (BN, D, fH, fW) flat = point order
    feat = x[:, D:]                                                         # (BN, C, fH, fW)
    ranks = np.asarray(ranks).reshape(-1)
    kept = ranks >= 0
    nx = c['nx']
    K = c['K']
    L = np.bincount(ranks[kept], minlength=K)
    out = np.zeros((K, C))
    absum = np.zeros((K, C))
    r = ranks[kept]
    pk = prob[kept]
    for ch in range(C):
        f = np.broadcast_to(feat[:, ch][:, None], (x.shape[0], D, c['fH'], c['fW'])).reshape(-1)[kept]
        out[:, ch] = np.bincount(r, weights=pk * f, minlength=K)
        absum[:, ch] = np.bincount(r, weights=np.abs(pk * f), minlength=K)
    shape = lambda a: a.reshape(c['B'], nx[2], nx[0], nx[1], C).transpose(0, 1, 4, 2, 3).reshape(c['B'], nx[2] * C, nx[0], nx[1])
    return shape(out), shape(absum), L


def pool_bound(c, absum, L):
    """per output element: (L + D + 32) * 2^-24 * sum |p64 * f| - L - 1 additions, one product, the softmax's D - 1 additions, a
    division, expf, and the argument's rounding at |logit - max| <= 16"""
    nx = c['nx']
    Lc = np.broadcast_to(L.reshape(c['B'], nx[2], 1, nx[0], nx[1]), (c['B'], nx[2], c['C'], nx[0], nx[1])).reshape(absum.shape)
    return (Lc + c['D'] + 32) * 2.0 ** -24 * absum


def workspace_bytes(c, B=None, N=None):
    """the formula of include/ddp_lss_mi355x.h"""
    B, N = B or c['B'], N or c['N']
    r = lambda n: (n + 255) // 256 * 256
    P = B * N * c['D'] * c['fH'] * c['fW']
    K = B * c['nx'][2] * c['nx'][0] * c['nx'][1]
    X = B * N * c['fH'] * c['fW']
    return r(4 * P) + r(4 * (K + 1)) + r(4 * K) + r(4 * ((K + 1023) // 1024)) + 3 * r(4 * P) + r(4 * X * c['C'])


def load_fixture(name, golden_dir):
    """-> (main, ds2): the npz of the case and of its downsample = 2 variant (None where nz > 1: the reference's downsample stack
    takes C channels and cannot follow the z collapse of more than one slab)"""
    import os
    ds2 = os.path.join(golden_dir, f'lss_{name}_ds2.npz')
    return np.load(os.path.join(golden_dir, f'lss_{name}.npz')), np.load(ds2) if case(name)['nx'][2] == 1 else None


def state_dict_of(fix):
    return {k[3:]: torch.from_numpy(fix[k]) for k in fix.files if k.startswith('sd/')}
