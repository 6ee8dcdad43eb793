"""Cases of the device-side front of ``DepthLSSTransform`` (include/ddp_dlss_mi355x.h, ddp_amd/dlss.py) and the restatements they are
checked against.  Device-free: numpy and CPU torch only.  The rig builders are those of tests/lss_cases.py.

  ``CASES`` / ``case(name)``   a rig + lidar points per sample + camera features; also every key ``lss_cases`` needs for the lift and pool
  ``project``                  the chain of the reference's ``BaseDepthTransform.forward`` (base.py:243-275) as elementwise torch CPU ops in
                               fp32 or float64, on a copy of the points -> per sample (row/col (N, P, 2), clamped z (N, P))
  ``tables_of``                -> the (B, N, Pmax) pixel (int32, -1 off the image) and depth tables
  ``winner_scatter``           tables -> the depth image, the LARGEST point index of a pixel wins
  ``stem_f64`` / ``stem_bound``  ``dtransform[0:6]`` in float64 with eval-mode BatchNorm, and the per-element error bound of a fp32 evaluation
  ``depth_terms``              S of the depth-table bound: the absolute terms that form z
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import lss_cases as LC

DELTA = 1e-3               # a fp64 row or column this close to an integer (0, iH and iW are integers) excuses the pair's pixel
EXCUSED_SHARE = 0.01       # at most this share of a case's on-image pairs may be excused
DEPTH_ULPS = 16            # |dev - f64| <= 16 * 2^-24 * S on the depth table (``depth_terms``)
STEM_ULPS = 216            # (K + 16) * 2^-24 with K = 200 products (``stem_bound``)
Z_LO, Z_HI = 1e-5, 1e5

NUSC = dict(f=1266.4, cx=816.3, cy=491.5, scale=0.48, trans=(-32.0, -176.0), width=704)

# name -> geometry.  image (iH, iW); feature = the size dtransform leaves: two times (n - 1) // s + 1 with s = 4, 2.
CASES = {
    'one': dict(B=1, yaws=[0.0], pitch=[0.0], image=(5, 9), feature=(1, 2), counts=[7], stride=3, aimed=[7], cloud=[0], C=2, in_channels=3,
                dbound=(1.0, 31.0, 6.0), xbound=(-16.0, 16.0, 4.0), ybound=(-16.0, 16.0, 4.0), zbound=(-10.0, 10.0, 20.0), exact=True),
    'odd': dict(B=2, yaws=[0.0, 120.0, 240.0], pitch=[0.0, -8.0, 5.0], image=(23, 50), feature=(3, 7), counts=[300, 0], stride=5,
                aimed=[60, 0], cloud=[240, 0], C=4, in_channels=5, dbound=(1.0, 40.0, 3.0), xbound=(-16.0, 16.0, 2.0),
                ybound=(-16.0, 16.0, 2.0), zbound=(-4.0, 4.0, 4.0), laug='turn'),
    'dups': dict(B=1, yaws=[0.0, 180.0], pitch=[0.0, 0.0], image=(8, 12), feature=(1, 2), counts=[3000], stride=4, aimed=[3000], cloud=[0],
                 C=3, in_channels=4, dbound=(1.0, 31.0, 6.0), xbound=(-32.0, 32.0, 8.0), ybound=(-32.0, 32.0, 8.0),
                 zbound=(-10.0, 10.0, 20.0), crowd=100, exact=True),
    'behind': dict(B=1, yaws=[0.0, 180.0], pitch=[0.0, 0.0], image=(16, 24), feature=(2, 3), counts=[40], stride=5, aimed=[32], cloud=[0],
                   C=3, in_channels=4, dbound=(1.0, 31.0, 6.0), xbound=(-32.0, 32.0, 8.0), ybound=(-32.0, 32.0, 8.0),
                   zbound=(-10.0, 10.0, 20.0), axis=8, exact=True),
    'rig': dict(B=1, yaws=[0.0, 55.0, -55.0, 180.0, 110.0, -110.0], pitch=[0.0, 0.0, 0.0, 0.0, 0.0, 0.0], image=(32, 88), feature=(4, 11),
                counts=[6000], stride=5, aimed=[0], cloud=[6000], C=8, in_channels=8, dbound=(1.0, 60.0, 4.0),
                xbound=(-51.2, 51.2, 3.2), ybound=(-51.2, 51.2, 3.2), zbound=(-10.0, 10.0, 20.0), laug='full'),
    'wide': dict(B=2, yaws=[20.0, 200.0], pitch=[0.0, 0.0], image=(64, 176), feature=(8, 22), counts=[20000, 19000], stride=5,
                 aimed=[4000, 4000], cloud=[15994, 15000], C=4, in_channels=4, dbound=(1.0, 60.0, 4.0), xbound=(-51.2, 51.2, 3.2),
                 ybound=(-51.2, 51.2, 3.2), zbound=(-10.0, 10.0, 20.0), laug='turn', extras=True),
}
# ``wide``, sample 0, also holds six points no lidar gives: two farther than the upper clamp end from the camera that looks their way
# (z > 1e5: the table holds exactly 1e5; for the camera at their back exactly 1e-5), three non-finite ones, and one whose division by
# the clamped z overflows fp32 (a finite coordinate, +-inf after x / 1e-5).  The last four are dropped: pixel -1 in every camera.
EXTRAS = np.array([[2.0e5, 1.0e3, 0.0], [3.0e5, -2.0e3, 10.0], [np.nan, 1.0, 1.0], [np.inf, 0.0, 0.0], [1.0, -np.inf, 2.0], [0.0, 1.0e33, 0.0]])
EXTRAS_ABOVE, EXTRAS_DROPPED = 3, 4        # entries beyond the upper end (the two far points, and the last one in the camera it faces)
NAMES = list(CASES)
FIXTURES = [n for n in NAMES if n != 'wide']       # ``wide`` has no fixture: its expectations are computed in the test


def stem_size(image):
    return (image[0] - 1) // 4 + 1, (image[1] - 1) // 4 + 1


def _rig(s, seed):
    """float64 matrices of the case: camera2lidar, intrinsics, img_aug (B, N, 4, 4) and lidar_aug (B, 4, 4)"""
    B, N = s['B'], len(s['yaws'])
    iH, iW = s['image']
    c2l, intr, aug, laug = np.zeros((B, N, 4, 4)), np.zeros((B, N, 4, 4)), np.zeros((B, N, 4, 4)), np.zeros((B, 4, 4))
    r = iW / NUSC['width']
    for b in range(B):
        for n, (yaw, pitch) in enumerate(zip(s['yaws'], s['pitch'])):
            intr[b, n] = np.eye(4)
            aug[b, n] = np.eye(4)
            if 'axis' in s:
                # ``behind``: axis-aligned cameras at the origin, no principal point, the centring in img_aug: a point ON the optical axis
                # behind a camera has x = y = 0 exactly, so (x / 1e-5, y / 1e-5) = (0, 0) lands on the image whatever the clamp
                c2l[b, n] = np.round(LC._camera2lidar(yaw, pitch, 0.0, 0.0), 9)
                intr[b, n, 0, 0] = intr[b, n, 1, 1] = 20.0
                aug[b, n, :3, 3] = [iW / 2 + 0.5, iH / 2 + 0.5, 0.0]
            else:
                c2l[b, n] = LC._camera2lidar(yaw + 0.7 * b, pitch, 1.5, 1.5)
                intr[b, n, 0, 0] = intr[b, n, 1, 1] = NUSC['f'] + 3.0 * n
                intr[b, n, 0, 2], intr[b, n, 1, 2] = NUSC['cx'] - 5.0 * n, NUSC['cy'] + 2.0 * b
                aug[b, n, 0, 0] = aug[b, n, 1, 1] = NUSC['scale'] * r
                aug[b, n, :3, 3] = [NUSC['trans'][0] * r, NUSC['trans'][1] * r, 0.0]
        laug[b] = np.eye(4)
        if s.get('laug') == 'turn':
            laug[b, :3, :3] = LC._rot_z(3.0 + 2.0 * b)
            laug[b, :3, 3] = [0.3, -0.2 - 0.1 * b, 0.1]
        elif s.get('laug') == 'full':          # rotation, scale and shift
            laug[b, :3, :3] = LC._rot_z(-11.0) * 1.05
            laug[b, :3, 3] = [1.3, -0.7, 0.2]
    return c2l, intr, aug, laug


def _aim(rng, k, c2l, intr, aug, laug, image, pixel=None):
    """k lidar points (float64, in the augmented lidar frame) that fall on the image of one camera at depth 2 .. 40, a quarter of a
    pixel or more from every pixel boundary; ``pixel``: all of them on that (row, col)"""
    iH, iW = image
    row = (rng.integers(0, iH, k) if pixel is None else np.full(k, pixel[0])) + rng.uniform(0.25, 0.75, k)
    col = (rng.integers(0, iW, k) if pixel is None else np.full(k, pixel[1])) + rng.uniform(0.25, 0.75, k)
    depth = rng.uniform(2.0, 40.0, k)
    u = (col - aug[0, 3]) / aug[0, 0]
    v = (row - aug[1, 3]) / aug[1, 1]
    camp = np.stack([(u - intr[0, 2]) / intr[0, 0] * depth, (v - intr[1, 2]) / intr[1, 1] * depth, depth, np.ones(k)], 0)
    p = (c2l @ camp)[:3]
    return (laug[:3, :3] @ p + laug[:3, 3:4]).T


def _build(name, seed):
    s = dict(CASES[name])
    rng = np.random.default_rng(seed)
    B, N = s['B'], len(s['yaws'])
    iH, iW = s['image']
    c2l, intr, aug, laug = _rig(s, seed)
    f32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.float32))
    points = []
    for b in range(B):
        parts = []
        per = s['aimed'][b] - s.get('crowd', 0) if s['aimed'][b] else 0
        for n in range(N):
            k = per // N + (1 if n < per % N else 0)
            if k:
                parts.append(_aim(rng, k, c2l[b, n], intr[b, n], aug[b, n], laug[b], s['image']))
        if s.get('crowd') and s['aimed'][b]:
            parts.append(_aim(rng, s['crowd'], c2l[b, 0], intr[b, 0], aug[b, 0], laug[b], s['image'], pixel=(iH // 2, iW // 3)))
        if 'axis' in s:
            # behind camera 0 (which looks along +x): x = -d, and y, z so small that (f y / 1e-5, f z / 1e-5) is a few pixels
            d = rng.uniform(2.0, 30.0, s['axis'])
            off = np.array([[0.0, 0.0], [3.0, -2.0], [-5.25, 4.0], [7.25, 1.25], [-2.0, -6.25], [0.25, 0.25], [10.0, 5.0], [-11.0, -7.0]])[:s['axis']]
            parts.append(np.stack([-d, -off[:, 0] * 1e-5 / 20.0, -off[:, 1] * 1e-5 / 20.0], 1))
        k = s['cloud'][b]
        if k:
            rad, ang = rng.uniform(3.0, 45.0, k), rng.uniform(0.0, 2 * math.pi, k)
            p = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-2.0, 3.0, k)], 0)
            parts.append((laug[b, :3, :3] @ p + laug[b, :3, 3:4]).T)
        if s.get('extras') and b == 0:
            parts.append(EXTRAS)
        xyz = np.concatenate(parts, 0) if parts else np.zeros((0, 3))
        xyz = xyz[rng.permutation(xyz.shape[0])]
        assert xyz.shape[0] == s['counts'][b], (name, b, xyz.shape)
        rest = rng.uniform(0.0, 1.0, (xyz.shape[0], s['stride'] - 3))
        points.append(f32(np.concatenate([xyz, rest], 1)))
    k4 = intr
    l2i = k4 @ np.linalg.inv(c2l)
    fH, fW = s['feature']
    assert (fH, fW) == tuple((v - 1) // 2 + 1 for v in stem_size(s['image']))
    img = f32(rng.uniform(-1.0, 1.0, (B, N, s['in_channels'], fH, fW)))
    spec = dict(s, image=s['image'], feature=s['feature'])
    kwargs = dict(in_channels=s['in_channels'], out_channels=s['C'], image_size=list(s['image']), feature_size=list(s['feature']),
                  xbound=list(s['xbound']), ybound=list(s['ybound']), zbound=list(s['zbound']), dbound=list(s['dbound']))
    nx = [int(v) for v in torch.LongTensor([(r[1] - r[0]) / r[2] for r in (s['xbound'], s['ybound'], s['zbound'])])]
    D = int(torch.arange(*s['dbound'], dtype=torch.float).shape[0])
    return dict(name=name, seed=seed, spec=spec, kwargs=kwargs, points=points, img=img, camera2lidar=f32(c2l), camera_intrinsics=f32(k4),
                lidar2image=f32(l2i), img_aug_matrix=f32(aug), lidar_aug_matrix=f32(laug), B=B, N=N, iH=iH, iW=iW, counts=list(s['counts']),
                pmax=max(s['counts']), stride=s['stride'], D=D, C=s['C'], nx=nx, fH=fH, fW=fW, P=B * N * D * fH * fW,
                K=B * nx[2] * nx[0] * nx[1])


_cache = {}


def case(name):
    """Built once per name and never modified.  The seed is the first of 1000 * index + 0, 1, ... whose share of on-image pairs near a
    pixel or image boundary (float64) is at most EXCUSED_SHARE - none at all for the cases marked ``exact``."""
    if name in _cache:
        return _cache[name]
    for seed in range(1000 * NAMES.index(name), 1000 * NAMES.index(name) + 64):
        c = _build(name, seed)
        rc64 = [rc for rc, z in project(c, torch.float64)]
        on, near = on_image(c, rc64), near_boundary(c, rc64)
        share = float((near & on).sum()) / max(int(on.sum()), 1)
        if share <= (0.0 if c['spec'].get('exact') else EXCUSED_SHARE):
            _cache[name] = c
            return c
    raise AssertionError(f'no seed of {name} meets the near-boundary share')


def forward_args(c, dev=None):
    """the positional arguments of ``DepthLSSTransform.forward``: fresh copies of the points (the reference writes into them);
    ``sensor2ego`` and ``lidar2ego`` are sliced by the reference but never used: identities; ``lidar2camera`` and ``metas`` None"""
    mv = (lambda t: t.to(dev)) if dev is not None else (lambda t: t)
    eye = torch.eye(4)
    return (mv(c['img']), [mv(p.clone()) for p in c['points']], mv(eye.expand(c['B'], c['N'], 4, 4)), mv(eye.expand(c['B'], 4, 4)), None,
            mv(c['lidar2image']), mv(c['camera_intrinsics']), mv(c['camera2lidar']), mv(c['img_aug_matrix']), mv(c['lidar_aug_matrix']), None)


# ---- the chain -------------------------------------------------------------------------------------------------------------------------
def _mat3(m, x):
    """(..., 3, 3) times (..., 3, P) with one rounding per operation, summed left to right: (m0 x0 + m1 x1) + m2 x2.  What the reference's
    ``matmul`` gives when its BLAS runs in the reproducible mode the fixtures were recorded under (tests/golden/gen_dlss_golden.py), on
    every CPU; and the convention of the device kernel."""
    col = lambda j: m[..., :, j:j + 1]
    row = lambda j: x[..., j:j + 1, :]
    return (col(0) * row(0) + col(1) * row(1)) + col(2) * row(2)


def project(c, dtype=torch.float32, b=None, inverse=None):
    """base.py:243-268 step for step, in ``dtype``, on a COPY of the points -> per sample (rowcol (N, P, 2), z (N, P)); z is the clamped
    depth the reference reads back through its ``dist`` view.  The three ``matmul`` calls are written out (``_mat3``).  ``inverse``: the
    (B, 3, 3) fp32 ``torch.inverse(lidar_aug[:3, :3])`` a fixture recorded - LAPACK's last bit is the machine's; without it, this one's."""
    out = []
    for i in (range(c['B']) if b is None else [b]):
        cur = c['points'][i][:, :3].to(dtype).clone()
        aug, laug, l2i = c['img_aug_matrix'][i].to(dtype), c['lidar_aug_matrix'][i].to(dtype), c['lidar2image'][i].to(dtype)
        inv = torch.inverse(laug[:3, :3]) if inverse is None else torch.as_tensor(np.asarray(inverse[i])).to(dtype)
        cur -= laug[:3, 3]
        cur = _mat3(inv, cur.transpose(1, 0))
        cur = _mat3(l2i[:, :3, :3], cur.unsqueeze(0))
        cur += l2i[:, :3, 3].reshape(-1, 3, 1)
        dist = cur[:, 2, :]
        cur[:, 2, :] = torch.clamp(cur[:, 2, :], Z_LO, Z_HI)
        cur[:, :2, :] /= cur[:, 2:3, :]
        cur = _mat3(aug[:, :3, :3], cur)
        cur += aug[:, :3, 3].reshape(-1, 3, 1)
        out.append((cur[:, :2, :].transpose(1, 2)[..., [1, 0]].contiguous(), dist.clone()))
    return out


def counted_mask(c):
    """(B, 1, Pmax) bool: True for the rows a sample holds, False in the padding"""
    return (np.arange(c['pmax'])[None, :] < np.array(c['counts'])[:, None])[:, None, :]


def finite_mask(c):
    """(B, 1, Pmax) bool: rows whose x, y, z are all finite"""
    out = np.zeros((c['B'], 1, c['pmax']), dtype=bool)
    for b, p in enumerate(c['points']):
        out[b, 0, :p.shape[0]] = np.isfinite(p[:, :3].numpy()).all(1)
    return out


def raw_z(c):
    """the z BEFORE the clamp, float64: (B, N, Pmax), NaN in the padding (and for a non-finite point)"""
    out = np.full((c['B'], c['N'], c['pmax']), np.nan)
    for b in range(c['B']):
        p = c['points'][b][:, :3].double()
        laug, l2i = c['lidar_aug_matrix'][b].double(), c['lidar2image'][b].double()
        q = _mat3(torch.inverse(laug[:3, :3]), (p - laug[:3, 3]).T)
        out[b, :, :p.shape[0]] = (_mat3(l2i[:, :3, :3], q.unsqueeze(0))[:, 2, :] + l2i[:, 2, 3:4]).numpy()
    return out


def _padded(c, per_sample, fill, dtype):
    out = np.full((len(per_sample), c['N'], c['pmax']), fill, dtype=dtype)
    for b, a in enumerate(per_sample):
        out[b, :, :a.shape[1]] = a
    return out


def rowcol_table(c, rc):
    """(B, N, Pmax, 2) float64 of the row / column, NaN in the padding"""
    out = np.full((len(rc), c['N'], c['pmax'], 2), np.nan)
    for b, a in enumerate(rc):
        out[b, :, :a.shape[1]] = a.double().numpy()
    return out


def pixels_of(c, rowcol):
    """(…, 2) row / column -> int32 pixel ``trunc(row) * iW + trunc(col)`` where 0 <= row < iH and 0 <= col < iW, else -1 (NaN: -1)"""
    rc = np.asarray(rowcol, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        on = (rc[..., 0] >= 0) & (rc[..., 0] < c['iH']) & (rc[..., 1] >= 0) & (rc[..., 1] < c['iW'])
    t = np.trunc(np.where(on[..., None], rc, 0.0)).astype(np.int64)
    return np.where(on, t[..., 0] * c['iW'] + t[..., 1], -1).astype(np.int32)


def tables_of(c, chain):
    """``project`` output -> pix (B, N, Pmax) int32, dep (B, N, Pmax) in the chain's precision; the padding is -1 / 0"""
    pix = pixels_of(c, rowcol_table(c, [rc for rc, z in chain]))
    dep = _padded(c, [z.numpy() for rc, z in chain], 0.0, chain[0][1].numpy().dtype)
    return pix, dep


def on_image(c, rc):
    return pixels_of(c, rowcol_table(c, rc)) >= 0


def near_boundary(c, rc):
    """pairs whose float64 row or column lies within DELTA of an integer - a pixel boundary, or the image's edge 0 / iH / iW - and within
    DELTA of the image (a pair far outside has one answer)"""
    t = rowcol_table(c, rc) if isinstance(rc, list) else np.asarray(rc)
    with np.errstate(invalid='ignore'):
        close = np.abs(t - np.rint(t)) <= DELTA
        inside = ((t[..., 0] >= -DELTA) & (t[..., 0] <= c['iH'] + DELTA) & (t[..., 1] >= -DELTA) & (t[..., 1] <= c['iW'] + DELTA))
    return close.any(-1) & inside


def admissible(c, rc64, got):
    """True per (b, n, p) where ``got`` is the float64 pixel or - for a pair within DELTA of a boundary - the pixel on either side of it,
    "off the image" included"""
    t = rowcol_table(c, rc64) if isinstance(rc64, list) else np.asarray(rc64)
    k = np.rint(t)
    with np.errstate(invalid='ignore'):
        near = np.abs(t - k) <= DELTA
    ok = np.zeros(np.asarray(got).shape, dtype=bool)
    for dr in (-0.5, 0.5):
        for dc in (-0.5, 0.5):
            ok |= pixels_of(c, np.where(near, k + np.array([dr, dc]), t)) == got
    return ok


def winner_scatter(c, pix, dep):
    """tables -> (B, N, 1, iH, iW) of dep's dtype: among the entries of one (b, n) that name a pixel the LARGEST p wins; +0.0 elsewhere.
    An entry outside [0, iH * iW) counts as -1."""
    B, N, _ = pix.shape
    HW = c['iH'] * c['iW']
    img = np.zeros((B, N, HW), dtype=dep.dtype)
    for b in range(B):
        for n in range(N):
            keep = np.flatnonzero((pix[b, n] >= 0) & (pix[b, n] < HW))          # ascending p
            win = np.full(HW, -1, dtype=np.int64)
            np.maximum.at(win, pix[b, n, keep], keep)
            img[b, n, win >= 0] = dep[b, n, win[win >= 0]]
    return img.reshape(B, N, 1, c['iH'], c['iW'])


def depth_terms(c):
    """S (B, N, Pmax) float64: the sum of the absolute terms of the two 3 x 3 products and the two shifts that form z,
    z = sum_j L[2, j] (sum_k M[j, k] (p_k - t_k)) + l_2 with M = inverse(lidar_aug_rot): S = sum_j |L2j| sum_k |Mjk| (|p_k| + |t_k|) + |l_2|.
    Each term passes one subtraction, a product and two additions twice over, and the last shift: 8 roundings; the device takes M as the
    fp32 ``torch.inverse`` gives it (a few more ulps of every term): DEPTH_ULPS = 16."""
    out = np.zeros((c['B'], c['N'], c['pmax']))
    for b in range(c['B']):
        p = c['points'][b][:, :3].double().numpy()
        laug, l2i = c['lidar_aug_matrix'][b].double().numpy(), c['lidar2image'][b].double().numpy()
        M = np.abs(np.linalg.inv(laug[:3, :3]))
        with np.errstate(invalid='ignore'):                                        # a non-finite point has no bound: NaN or inf
            inner = (np.abs(p) + np.abs(laug[:3, 3])) @ M.T                       # (P, 3): sum_k |Mjk| (|p_k| + |t_k|)
            out[b, :, :p.shape[0]] = np.abs(l2i[:, 2, :3]) @ inner.T + np.abs(l2i[:, 2, 3])[:, None]
    return out


# ---- the stem ----------------------------------------------------------------------------------------------------------------------------
def _fold64(sd, conv, bn):
    t = lambda k: torch.as_tensor(np.asarray(sd[k])).double()
    g = t(f'dtransform.{bn}.weight') / torch.sqrt(t(f'dtransform.{bn}.running_var') + 1e-5)
    return t(f'dtransform.{conv}.weight'), t(f'dtransform.{conv}.bias'), g, t(f'dtransform.{bn}.running_mean'), t(f'dtransform.{bn}.bias')


def stem_f64(depth, sd):
    """``dtransform[0:6]`` in float64, eval-mode BatchNorm (eps 1e-5): depth (BN, 1, iH, iW) -> (out (BN, 32, oH, oW), terms) where
    ``terms`` is what ``stem_bound`` multiplies: the absolute terms of every output element"""
    d = torch.as_tensor(np.asarray(depth)).double().reshape(-1, 1, *np.asarray(depth).shape[-2:])
    w1, b1, g1, m1, be1 = _fold64(sd, 0, 1)
    w2, b2, g2, m2, be2 = _fold64(sd, 3, 4)
    s1 = (w1.view(-1) * g1).view(1, -1, 1, 1)
    a = torch.relu(s1 * d + ((b1 - m1) * g1 + be1).view(1, -1, 1, 1))
    a_abs = s1.abs() * d.abs() + ((b1 - m1).abs() * g1.abs() + be1.abs()).view(1, -1, 1, 1)       # >= a; zero padding pads both
    w2f = w2 * g2.view(-1, 1, 1, 1)
    out = torch.relu(F.conv2d(a, w2f, (b2 - m2) * g2 + be2, stride=4, padding=2))
    terms = F.conv2d(a_abs, w2f.abs(), (b2 - m2).abs() * g2.abs() + be2.abs(), stride=4, padding=2)
    return out.numpy(), terms.numpy()


def stem_bound(terms):
    """per element (K + 16) * 2^-24 * terms, K = 200 products: a product w2' a carries the folded weight's 4 roundings (add, sqrt, division,
    product), the activation's 8 relative to its absolute terms (folded scale 4, folded shift 3 of them, the fma 1) and at most 200
    additions of the sum; the folded bias 6 and the last addition 1; ReLU is 1-Lipschitz.  4 + 8 + 200 < 216."""
    return STEM_ULPS * 2.0 ** -24 * terms


# ---- the whole module in float64 ---------------------------------------------------------------------------------------------------------
def forward_f64(c, module, depth, ranks):
    """a ``DepthLSSTransform`` (its torch modules cast to double on a copy) on a given depth image and rank table -> the output in float64;
    the pooled sum is ``lss_cases.pool_f64``"""
    import copy
    m = copy.deepcopy(module).cpu().double().eval()
    with torch.no_grad():
        d = m.dtransform(torch.as_tensor(np.asarray(depth)).double().view(c['B'] * c['N'], 1, c['iH'], c['iW']))
        x = m.depthnet(torch.cat([d, c['img'].double().view(c['B'] * c['N'], -1, c['fH'], c['fW'])], 1)).numpy()
        pooled = LC.pool_f64(c, x, ranks)[0]
        return m.downsample(torch.from_numpy(pooled)).numpy()


def workspace_bytes(c, B=None, N=None, pmax=None):
    """the formula of include/ddp_dlss_mi355x.h"""
    B, N, pmax = B or c['B'], N or c['N'], c['pmax'] if pmax is None else pmax
    r = lambda n: (n + 255) // 256 * 256
    return 2 * r(4 * B * N * pmax) + r(4 * B * N * c['iH'] * c['iW']) + r(4 * 6448)


def load_fixture(name, golden_dir):
    import os
    return np.load(os.path.join(golden_dir, f'dlss_{name}.npz'))


def state_dict_of(fix, prefix='sd/'):
    return {k[len(prefix):]: torch.from_numpy(fix[k]) for k in fix.files if k.startswith(prefix)}
