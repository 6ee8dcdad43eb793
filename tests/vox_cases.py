"""The cases of the device-side hard voxelisation (include/ddp_vox_mi355x.h, ddp_amd/vox.py) and their restatement, shared by
tests/test_vox_host.py, tests/test_zz_vox_gpu.py and tests/golden/gen_vox_golden.py.

  ``hard_voxelize_ref``  the reference's sequential loop (bev/mmdet3d/ops/voxel/src/voxelization_cpu.cpp:45-101) in NumPy: fp32
                         ``floor((p - lo) / vs)``, a dict from cell to voxel, the two caps
  ``batch_ref``          ``BEVFusion.voxelize`` of the hard branch: concatenation, the batch column, the left-to-right fp32 mean
  ``mean_f64``           the float64 mean and the bound the device's and the fixture's fp32 means are held to

Which case has which source.  ``FIXTURES`` were run through the reference's own ``hard_voxelize_cpu`` and ``BEVFusion.voxelize``
(tests/golden/gen_vox_golden.py): their grids have grid_x == grid_z, the only grids on which the reference's CPU function is memory-safe
(its cell-to-voxel table is allocated {grid_z, grid_y, grid_x} and indexed [x][y][z], voxelization_cpu.cpp:75,129-130).  Every other
case - ``flat`` with its 40 x 40 x 8 grid among them - has the restatement alone.
"""
import json
import os

import numpy as np

F32 = np.float32


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def grid_of(voxel_size, point_cloud_range):
    """round((hi - lo) / vs) in fp32, half to even: what ``Voxelization.__init__`` computes with torch"""
    r, v = np.asarray(point_cloud_range, F32), np.asarray(voxel_size, F32)
    return [int(g) for g in np.rint((r[3:] - r[:3]) / v)]


def cells_ref(points, c):
    """(P,) int32: (x * gy + y) * gz + z or -1, from fp32 floor((p - lo) / vs) compared as floats"""
    lo, vs, grid = np.asarray(c['range'][:3], F32), np.asarray(c['voxel_size'], F32), np.asarray(c['grid'])
    p = np.ascontiguousarray(points[:, :3], dtype=F32)
    with np.errstate(all='ignore'):
        q = np.floor((p - lo) / vs)
        ok = ((q >= 0) & (q < grid.astype(F32))).all(1)
    qi = np.where(ok[:, None], q, 0).astype(np.int64)
    ids = (qi[:, 0] * grid[1] + qi[:, 1]) * grid[2] + qi[:, 2]
    return np.where(ok, ids, -1).astype(np.int32)


def assign_ref(cells, T, max_voxels):
    """the sequential loop over one sample's cell ids -> point_voxel (P,), voxel_points (M, T) (-1 = empty), voxel_cells (M,)"""
    voxel_of, rows, vcells = {}, [], []
    pvox = np.full(len(cells), -1, np.int32)
    for i, cid in enumerate(cells.tolist()):
        if cid < 0:
            continue
        v = voxel_of.get(cid)
        if v is None:
            if len(rows) >= max_voxels:
                continue
            v = voxel_of[cid] = len(rows)
            rows.append([])
            vcells.append(cid)
        pvox[i] = v
        if len(rows[v]) < T:
            rows[v].append(i)
    table = np.full((len(rows), T), -1, np.int32)
    for v, r in enumerate(rows):
        table[v, :len(r)] = r
    return pvox, table, np.asarray(vcells, np.int32).reshape(-1)


def hard_voxelize_ref(points, c, max_voxels=None):
    """one sample -> voxels (M, T, F) fp32 with +0.0 in unused slots, coors (M, 3) int32 x y z, num_points (M) int32"""
    T, F, grid = c['T'], c['F'], c['grid']
    pvox, table, vcells = assign_ref(cells_ref(points, c), T, c['max_voxels'] if max_voxels is None else max_voxels)
    M = len(table)
    voxels = np.zeros((M, T, F), F32)
    for v in range(M):
        n = int((table[v] >= 0).sum())
        voxels[v, :n] = points[table[v, :n], :F]
    vc = vcells.astype(np.int64)
    coors = np.stack([vc // (grid[1] * grid[2]), vc // grid[2] % grid[1], vc % grid[2]], 1).astype(np.int32).reshape(M, 3)
    return voxels, coors, (table >= 0).sum(1).astype(np.int32)


def batch_ref(c, reduce=True):
    """the samples of a case -> feats, coords (sum M, 4), sizes (sum M); feats (sum M, F): ((x_0 + x_1) + ...) / float(n) in fp32"""
    per = [hard_voxelize_ref(p, c) for p in c['points']]
    feats = np.concatenate([v for v, _, _ in per], 0)
    coords = np.concatenate([np.concatenate([np.full((len(co), 1), b, np.int32), co], 1) for b, (_, co, _) in enumerate(per)], 0)
    sizes = np.concatenate([n for _, _, n in per], 0)
    if reduce:
        total = feats[:, 0].copy()
        for s in range(1, c['T']):
            total = (total + feats[:, s]).astype(F32)          # adding the +0.0 of an unused slot changes no value
        feats = (total / sizes.astype(F32)[:, None]).astype(F32)
    return feats, coords, sizes


def mean_f64(voxels, sizes):
    """-> the float64 mean (M, F) of the kept rows and the bound (n + 1) 2^-24 sum|x_s| / n per element: n - 1 additions and one
    division, each within 2^-24 relative of its exact result, (1 + u)^n - 1 < (n + 1) u for the n <= 256 of the library"""
    v64 = voxels.astype(np.float64)
    n = sizes.astype(np.float64)[:, None]
    return v64.sum(1) / n, (n + 1) * 2.0 ** -24 * np.abs(v64).sum(1) / n


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _geometry(lo, vs, grid):
    hi = [float(F32(l) + F32(g) * F32(v)) for l, v, g in zip(lo, vs, grid)]
    rng = [float(v) for v in lo] + hi
    assert grid_of(vs, rng) == list(grid), (grid_of(vs, rng), grid)
    return dict(voxel_size=[float(v) for v in vs], range=rng, grid=list(grid))


G16 = _geometry((-0.8, -0.8, -0.8), (0.1, 0.1, 0.1), (16, 16, 16))
G_EDGES = _geometry((0.0, -1.2, -0.6), (0.075, 0.1, 0.075), (16, 24, 16))
G32 = _geometry((-1.6, -2.7, -1.6), (0.1, 0.15, 0.1), (32, 36, 32))
G_FLAT = _geometry((-2.0, -2.0, -1.0), (0.1, 0.1, 0.25), (40, 40, 8))          # the recipe's 1024 x 1024 x 40 shape, scaled down
G_RECIPE = dict(voxel_size=[0.1, 0.1, 0.2], range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], grid=[1024, 1024, 40])
assert grid_of(G_RECIPE['voxel_size'], G_RECIPE['range']) == G_RECIPE['grid']


def _cloud(rng, n, g, stride, spread=1.15, lattice=0.25):
    """n rows: xyz uniform over the range widened by ``spread`` (some fall outside), a share ``lattice`` of them moved onto
    lo + k * vs in fp32 with k in 0 .. grid (k = 0 and k = grid included); further columns uniform in [-1, 1)"""
    lo, vs, grid = np.asarray(g['range'][:3], F32), np.asarray(g['voxel_size'], F32), np.asarray(g['grid'])
    mid, half = lo + vs * grid / 2, vs * grid / 2
    p = rng.uniform(-1, 1, (n, stride)).astype(F32)
    p[:, :3] = (mid + half * spread * p[:, :3]).astype(F32)
    on = rng.uniform(size=n) < lattice
    k = rng.integers(0, grid + 1, (n, 3))
    k[::7] = np.where(rng.uniform(size=k[::7].shape) < 0.5, 0, grid)
    p[on, :3] = (lo + k[on].astype(F32) * vs).astype(F32)
    return p


def _in_cells(rng, cells, g, stride):
    """one row per entry of ``cells`` (cell ids), placed strictly inside its cell"""
    lo, vs, grid = np.asarray(g['range'][:3], np.float64), np.asarray(g['voxel_size'], np.float64), g['grid']
    cells = np.asarray(cells, np.int64)
    q = np.stack([cells // (grid[1] * grid[2]), cells // grid[2] % grid[1], cells % grid[2]], 1)
    p = rng.uniform(-1, 1, (len(cells), stride)).astype(F32)
    p[:, :3] = (lo + (q + rng.uniform(0.2, 0.8, (len(cells), 3))) * vs).astype(F32)
    return p


def _case(name, g, points, T, max_voxels, F=None, seed=0):
    points = [np.ascontiguousarray(p, dtype=F32) for p in points]
    c = dict(g, name=name, points=points, T=T, max_voxels=max_voxels, stride=points[0].shape[1], seed=seed)
    c['F'] = c['stride'] if F is None else F
    c['counts'] = [len(p) for p in points]
    c['B'] = len(points)
    return c


def _one(rng):
    return _case('one', G16, [_in_cells(rng, [1234], G16, 5)], 3, 5)


def _empty(rng):
    return _case('empty', G16, [np.zeros((0, 5), F32)], 3, 5)


def _all_out(rng):
    p = _in_cells(rng, [5] * 7, G16, 5)
    p[:, 0] += np.asarray([2, -2, 0, 0, 0, 0, 4], F32)
    p[:, 1] += np.asarray([0, 0, 2, -3, 0, 0, 4], F32)
    p[:, 2] += np.asarray([0, 0, 0, 0, 2, -2, 4], F32)
    return _case('all_out', G16, [p], 3, 5)


def _edges(rng):
    g = G_EDGES
    lo, vs, grid = np.asarray(g['range'][:3], F32), np.asarray(g['voxel_size'], F32), np.asarray(g['grid'])
    hi = np.asarray(g['range'][3:], F32)
    p = _cloud(rng, 200, g, 5, lattice=0.6)
    row = 0
    for j in range(3):                     # per axis: lo, hi, the neighbours of both, a lattice plane and its neighbours; -0.0 on x
        base = _in_cells(rng, [777] * 10, g, 5)
        k = F32(lo[j] + F32(5) * vs[j])
        # the neighbours of lo = 0.0 on x are +-2^-100, not the subnormal neighbours of zero: a mean of subnormals underflows, and the
        # bound of ``mean_f64`` is one of relative errors
        below, above = (F32(-2.0 ** -100), F32(2.0 ** -100)) if lo[j] == 0 else (np.nextafter(lo[j], F32(-np.inf)), np.nextafter(lo[j], F32(np.inf)))
        vals = [lo[j], below, above, hi[j], np.nextafter(hi[j], F32(-np.inf)),
                np.nextafter(hi[j], F32(np.inf)), k, np.nextafter(k, F32(-np.inf)), np.nextafter(k, F32(np.inf)), F32(-0.0) if j == 0 else lo[j]]
        base[:, j] = np.asarray(vals, F32)
        p[row:row + 10] = base
        row += 10
    return _case('edges', g, [p], 4, 4000)


def _nonfinite(rng):
    p = _in_cells(rng, rng.integers(0, 4096, 64), G16, 5)
    bad = [np.nan, np.inf, -np.inf, 1e30, -1e30]
    for j in range(3):
        for i, v in enumerate(bad):
            p[3 + 15 * j + 3 * i, j] = v       # every third row: both neighbours of a dropped row stay
    return _case('nonfinite', G16, [p], 3, 100)


def _dups(rng):
    cells = np.asarray([100, 2077, 4095, 0, 1500])
    deal = rng.permutation(np.repeat(cells, 60))
    return _case('dups', G16, [_in_cells(rng, deal, G16, 5)], 3, 50)


def _one_voxel(rng):
    return _case('one_voxel', G16, [_in_cells(rng, [2222] * 20000, G16, 5)], 10, 50)


def _cap(rng):
    cells = rng.choice(32 * 36 * 32, 400, replace=False)
    deal = np.concatenate([cells, rng.choice(cells, 600)])
    head = rng.permutation(700)                                            # all 400 cells appear among the first 700 rows or later
    deal = np.concatenate([deal[:700][head], deal[700:]])
    return _case('cap', G32, [_in_cells(rng, deal, G32, 5)], 5, 37)


def _cap_exact(rng, delta):
    cells = rng.choice(4096, 40, replace=False)
    deal = rng.permutation(np.concatenate([cells, rng.choice(cells, 80)]))
    return _case(f'cap_exact{delta:+d}', G16, [_in_cells(rng, deal, G16, 4)], 2, 40 + delta)


def _tiles(rng, n):
    """the last row founds a voxel of its own: with n one past a tile it is that tile's only point"""
    p = _cloud(rng, n, G32, 4, spread=1.05)
    used = set(cells_ref(p[:-1], G32).tolist())
    p[-1:] = _in_cells(rng, [next(i for i in range(32 * 36 * 32) if i not in used)], G32, 4)
    return _case(f'tiles{n}', G32, [p], 3, 5000)


def _feat(rng, F, pad):
    """130 rows dealt into 30 cells (every mean sums several rows, some voxels pass the point cap) and 20 of a cloud"""
    crowded = rng.choice(4096, 30, replace=False)
    p = np.concatenate([_in_cells(rng, rng.choice(crowded, 130), G16, F + pad), _cloud(rng, 20, G16, F + pad)])
    return _case(f'feat{F}+{pad}', G16, [rng.permutation(p)], 4, 60, F=F)


def _flat(rng):
    return _case('flat', G_FLAT, [_cloud(rng, 900, G_FLAT, 5)], 4, 500)


def _batch(rng):
    """two clouds with 40 crowded cells dealt into them (voxels of 1 .. T points and beyond the point cap), an empty sample between"""
    crowded = rng.choice(32 * 36 * 32, 40, replace=False)
    mix = lambda n, m: rng.permutation(np.concatenate([_cloud(rng, n, G32, 5), _in_cells(rng, rng.choice(crowded, m), G32, 5)]))
    return _case('batch', G32, [mix(400, 300), np.zeros((0, 5), F32), mix(800, 500)], 10, 350)


TILES = (1023, 1024, 1025, 4095, 4096, 4097)           # around one scan tile of 1024 points and around four
FEATS = ((3, 0), (3, 3), (4, 0), (4, 3), (5, 0), (5, 3), (16, 0), (16, 3))
BUILDERS = dict(one=_one, empty=_empty, all_out=_all_out, edges=_edges, nonfinite=_nonfinite, dups=_dups, one_voxel=_one_voxel, cap=_cap,
                **{f'cap_exact{d:+d}': (lambda rng, d=d: _cap_exact(rng, d)) for d in (-1, 0, 1)},
                **{f'tiles{n}': (lambda rng, n=n: _tiles(rng, n)) for n in TILES},
                **{f'feat{F}+{pad}': (lambda rng, F=F, pad=pad: _feat(rng, F, pad)) for F, pad in FEATS},
                flat=_flat, batch=_batch)
NAMES = list(BUILDERS)
# run through the reference's own code: grid_x == grid_z on every one of them
FIXTURES = ['one', 'all_out', 'edges', 'nonfinite', 'dups', 'cap', 'batch']
_made = {}


def case(name):
    """the case, made once per process from a seed of its own and left unchanged"""
    if name not in _made:
        seed = 1000 + NAMES.index(name)
        _made[name] = BUILDERS[name](np.random.default_rng(seed))
        _made[name]['seed'] = seed
    return _made[name]


def config_of(c):
    """what a fixture records beside its arrays: one JSON string"""
    return json.dumps({k: c[k] for k in ('name', 'voxel_size', 'range', 'grid', 'T', 'max_voxels', 'F', 'stride', 'counts', 'B', 'seed')}, sort_keys=True)


def load_fixture(name, golden):
    return np.load(os.path.join(golden, f'vox_{name}.npz'))


def workspace_bytes(B, pmax, max_voxels, T):
    """the formula of include/ddp_vox_mi355x.h"""
    r = lambda n: (n + 255) // 256 * 256
    H = 2
    while H < 2 * pmax:
        H *= 2
    P, V, nt = B * pmax, B * max_voxels, (pmax + 1023) // 1024
    return 3 * r(4 * P) + r(4 * V * T) + r(4 * V) + r(4 * B) + 3 * r(4 * B * H) + r(4 * B * nt) + r(4 * (B + 1))
