"""Edge cases of the device-side hard voxelisation (include/ddp_vox_mi355x.h) beyond tests/vox_cases.py - the integer half: the voxel
cap across scan tiles, more scan tiles than the one-block scan has threads, hash probing that wraps past the last slot, cell ids above
2^24 and 2^30, per-sample tables of a batch - and T = 1, T = 256, empty batches.  Shared by tests/test_vox_edges_host.py,
tests/test_zzz_vox_edges_gpu.py and tests/golden/gen_vox_golden.py.  The restatement is the one of tests/vox_cases.py, unchanged
(``cells_ref``, ``assign_ref``, ``hard_voxelize_ref``, ``batch_ref``, ``mean_f64``); nothing here appends to ``vox_cases.NAMES``.

  TABLE cases  a caller's (B, Pmax) int32 cell table for ``assign_from_cells``, a grid, T and the ``max_voxels`` values to run
  POINT cases  dicts of the ``vox_cases._case`` form, for the full path (cells, assign, gather, both forms of pack)

Beside the cases: the documented hash in NumPy (``homes``), a sequential model of the open-addressed table (``slots_ref``), and the
scan-form restatement ``assign_scan`` - founder flags, tile sums, tile starts, numbers, the cap - which equals ``assign_ref`` and can be
given one DEFECT at a time: what the host test uses in place of a mutated kernel.
"""
import numpy as np

import vox_cases as VC

F32 = np.float32
HASH_MULT, SCAN_TILE, THREADS = 2654435761, 1024, 256          # include/ddp_vox_mi355x.h; tests/test_vox_edges_host.py holds them to the binding
PER_THREAD = SCAN_TILE // THREADS
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
G128 = VC._geometry((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (128, 128, 128))            # the grid of the existing collision part
G_BIG = VC._geometry((0.0, 0.0, 0.0), (0.5, 0.5, 0.5), (2048, 1024, 1023))       # volume 2 145 386 496 < 2^31


def volume(g):
    return int(np.prod(np.asarray(g['grid'], np.int64)))


def capacity(pmax):
    """H: the smallest power of two >= 2 * pmax, at least 2"""
    h = 2
    while h < 2 * pmax:
        h *= 2
    return h


def homes(ids, pmax):
    """the documented hash, vectorised: (uint32(c) * 2654435761) >> (32 - log2 H)"""
    h = capacity(pmax)
    ids = np.asarray(ids, np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    return (((ids * np.uint64(HASH_MULT)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - (h.bit_length() - 1))).astype(np.int64)


def cell_id(g, x, y, z):
    return (int(x) * g['grid'][1] + int(y)) * g['grid'][2] + int(z)


# ---- models of the device's steps -----------------------------------------------------------------------------------------------------
def slots_ref(cells, pmax, order=None, wrap=True):
    """one sample's ids inserted one by one (``order``: the arrival order, default row order) -> {id: slot}; ``wrap=False`` is the
    defect "probing stops at slot H - 1": an id that runs off the end gets no slot (it is absent from the result)"""
    H = capacity(pmax)
    keys, slot_of = {}, {}
    rows = range(len(cells)) if order is None else order
    home = homes(np.where(np.asarray(cells) >= 0, cells, 0), pmax)
    for i in rows:
        c = int(cells[i])
        if c < 0 or c in slot_of:
            continue
        h = int(home[i])
        while h < H and h in keys:
            h = (h + 1) & (H - 1) if wrap else h + 1
        if h < H:
            keys[h] = c
            slot_of[c] = h
    return slot_of


DEFECTS = ('sums_past_256', 'cap_per_tile', 'cap_per_run', 'probe_stops', 'id_through_float', 'dropped_to_last')


def assign_scan(cells, T, max_voxels, defect=None):
    """``assign_ref`` in the form the device computes it: a founder is the first point of its cell; a founder's number is its tile's
    start (the exclusive scan of the tile sums) plus its rank inside the tile; a founder numbered >= max_voxels drops its cell.
    -> point_voxel, voxel_points, voxel_cells, count.  ``defect``: one of DEFECTS built in."""
    assert defect is None or defect in DEFECTS
    cells = np.asarray(cells, np.int64).copy()
    pmax = len(cells)
    if defect == 'id_through_float':
        as_float = cells.astype(F32).astype(np.int64)
        cells = np.where(cells >= 0, as_float, -1)
    if defect == 'probe_stops':
        placed = slots_ref(cells, pmax, wrap=False)
        cells = np.asarray([c if c in placed else -1 for c in cells.tolist()], np.int64)
    valid = cells >= 0
    uniq, first, inverse = np.unique(np.where(valid, cells, -1), return_index=True, return_inverse=True)
    founder = np.zeros(pmax, bool)
    founder[first[uniq >= 0]] = True
    nt = (pmax + SCAN_TILE - 1) // SCAN_TILE
    flags = np.zeros(nt * SCAN_TILE, np.int64)
    flags[:pmax] = founder
    sums = flags.reshape(nt, SCAN_TILE).sum(1)
    starts = np.concatenate([[0], np.cumsum(sums)[:-1]])
    total = int(sums.sum())
    if defect == 'sums_past_256':                                          # a scan of one entry per thread: the rest stays as it was
        starts[THREADS:] = sums[THREADS:]
        total = int(sums[:THREADS].sum())
    rank = (np.cumsum(flags.reshape(nt, SCAN_TILE), 1) - flags.reshape(nt, SCAN_TILE)).reshape(-1)
    number = (np.repeat(starts, SCAN_TILE) + rank)[:pmax]
    if defect == 'cap_per_tile':
        kept = rank[:pmax] < max_voxels
    elif defect == 'cap_per_run':                                          # the test made on the number the thread's run of 4 starts with
        at_start = (np.repeat(starts, SCAN_TILE) + rank).reshape(-1, PER_THREAD)[:, 0]
        kept = np.repeat(at_start < max_voxels, PER_THREAD)[:pmax]
    else:
        kept = number < max_voxels
    # the voxel of every point: its cell's founder's, or -1
    founder_row = np.full(len(uniq), -1, np.int64)
    founder_row[uniq >= 0] = first[uniq >= 0]
    mine = founder_row[inverse]
    safe = np.where(valid, mine, 0)
    pvox = np.where(valid & kept[safe], number[safe], -1)
    if defect == 'dropped_to_last':
        pvox = np.where(valid, np.minimum(number[safe], max_voxels - 1), -1)
    count = min(total, max_voxels)
    table = np.full((count, T), -1, np.int32)
    vcells = np.full(count, -1, np.int32)
    fill = np.zeros(count, np.int64)
    for i in np.flatnonzero((pvox >= 0) & (pvox < count)).tolist():
        v = int(pvox[i])
        if founder[i] and kept[i]:
            vcells[v] = cells[i]
        if fill[v] < T:
            table[v, fill[v]] = i
            fill[v] += 1
    return pvox.astype(np.int32), table, vcells, count


# ---- table cases ----------------------------------------------------------------------------------------------------------------------
def _table_case(name, g, table, T, caps):
    table = np.ascontiguousarray(np.asarray(table, np.int64).astype(np.int32))
    assert table.ndim == 2
    return dict(g, name=name, table=table, T=T, caps=list(caps), B=table.shape[0], pmax=table.shape[1], volume=volume(g))


def taken(tc):
    """what the library makes of a caller's table: an id outside [0, volume) counts as -1"""
    t = tc['table'].astype(np.int64)
    return np.where((t >= 0) & (t < tc['volume']), t, -1).astype(np.int32)


_refs = {}


def table_ref(tc, max_voxels):
    """per sample (point_voxel, voxel_points, voxel_cells) of ``assign_ref``, computed once per (case, cap) and left unchanged"""
    key = (tc['name'], max_voxels)
    if key not in _refs:
        _refs[key] = [VC.assign_ref(row, tc['T'], max_voxels) for row in taken(tc)]
    return _refs[key]


CAP_TILES_HEAD, CAP_TILES_NEW = 2052, 600            # founder number = row index over two tiles and one thread's run; later founders


def _cap_tiles(rng):
    pmax, g = 5 * SCAN_TILE + 3, VC.G_RECIPE
    ids = rng.choice(volume(g), CAP_TILES_HEAD + CAP_TILES_NEW, replace=False)
    head, new = ids[:CAP_TILES_HEAD], ids[CAP_TILES_HEAD:]
    a = rng.choice(head[:1000], 800)                                       # repeats of ids founded below row 1000
    a[:4] = head[0]                                                        # the one voxel of max_voxels = 1 gains points too
    b = np.repeat(np.concatenate([head[1020:1031], head[2040:2052]]), 4)   # of ids founded around the two tile borders
    c = np.repeat(new, rng.integers(1, 5, CAP_TILES_NEW))                  # 600 new ids, each 1 .. 4 times
    d = np.full(pmax - CAP_TILES_HEAD - len(a) - len(b) - len(c), -1)
    assert len(d) >= 100
    total = CAP_TILES_HEAD + CAP_TILES_NEW
    caps = (1, 1023, 1024, 1025, 1026, 1027, 2047, 2048, 2049, total, total + 1)
    return _table_case('cap_tiles', g, [np.concatenate([head, rng.permutation(np.concatenate([a, b, c, d]))])], 3, caps)


def _draw(rng, n, pool, vol):
    """n ids drawn with repeats from ``pool`` distinct ids, about 5 % of them -1; the last row is an id of its own"""
    ids = rng.choice(vol, pool + 1, replace=False)
    rows = ids[rng.integers(0, pool, n)]
    rows[rng.uniform(size=n) < 0.05] = -1
    rows[-1] = ids[-1]
    return rows


def _scan257(rng):
    pmax, vol = 256 * SCAN_TILE + 1, volume(VC.G_RECIPE)
    return _table_case('scan257', VC.G_RECIPE, [_draw(rng, pmax, 115000, vol), _draw(rng, pmax, pmax // 2, vol)], 2, (106000,))


def _scan600(rng):
    pmax, vol = 599 * SCAN_TILE + 1, volume(VC.G_RECIPE)
    return _table_case('scan600', VC.G_RECIPE, [_draw(rng, pmax, pmax // 2, vol)], 2, (250000,))


WRAP_PMAX = 400


def _wrap(rng):
    H = capacity(WRAP_PMAX)
    ids = np.arange(volume(G128))
    home = homes(ids, WRAP_PMAX)
    last = np.concatenate([rng.choice(ids[home == s], 32, replace=False) for s in (H - 3, H - 2, H - 1)])
    front = np.asarray([rng.choice(ids[home == s]) for s in (0, 1, 2, 3, 4, 5, 0, 3)])
    assert len(set(front.tolist())) == 8
    rows = rng.permutation(np.concatenate([np.repeat(last, 3), front, [-1, volume(G128), INT_MAX, INT_MIN]]))
    rows = np.concatenate([rows, np.full(WRAP_PMAX - len(rows), -1)])
    return _table_case('wrap', G128, [rows], 3, (120,))


def _wrap_small(rng, pmax):
    """every id has the LAST slot as its home: the second and third wrap to slot 0 and on.  Two samples, one with a repeat."""
    H = capacity(pmax)
    ids = np.arange(volume(G128))
    same = rng.choice(ids[homes(ids, pmax) == H - 1], pmax, replace=False)
    again = same[::-1].copy()
    again[-1] = again[0]
    return _table_case(f'wrap_small{pmax}', G128, [same, again], 2, (5,))


def _batch_tables(rng):
    """three samples over one pool of ids; the first id is in all three, at rows 3, 41 and 17"""
    pmax, vol = 70, volume(VC.G_RECIPE)
    pool = rng.choice(vol, 45, replace=False)
    rows = []
    for at in (3, 41, 17):
        r = rng.choice(pool[1:], pmax)
        r[rng.uniform(size=pmax) < 0.1] = -1
        r[at] = pool[0]
        rows.append(r)
    return _table_case('batch_tables', VC.G_RECIPE, rows, 3, (10, 45))


def _batch_hollow(rng):
    """the same with the middle sample all -1"""
    table = case('batch_tables')['table'].copy()
    table[1] = -1
    return _table_case('batch_hollow', VC.G_RECIPE, table, 3, (10, 45))


BIG_IDS = (0, 2 ** 24, 2 ** 24 + 1, 2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, volume(G_BIG) - 2, volume(G_BIG) - 1)


def _big_ids(rng):
    vol = volume(G_BIG)
    rows = rng.permutation(np.concatenate([np.repeat(np.asarray(BIG_IDS, np.int64), [1, 4, 2, 3, 1, 4, 2, 3]), [vol, vol, vol]]))
    rows = np.concatenate([rows, np.full(40 - len(rows), -1)])
    return _table_case('big_ids', G_BIG, [rows], 3, (5, 20))


TABLE_BUILDERS = dict(cap_tiles=_cap_tiles, scan257=_scan257, scan600=_scan600, wrap=_wrap, wrap_small2=lambda rng: _wrap_small(rng, 2),
                      wrap_small3=lambda rng: _wrap_small(rng, 3), batch_tables=_batch_tables, batch_hollow=_batch_hollow, big_ids=_big_ids)
TABLE_NAMES = list(TABLE_BUILDERS)


# ---- point cases ----------------------------------------------------------------------------------------------------------------------
CAP_BATCH_FOUNDERS, CAP_BATCH_PMAX = (900, 1100, 1700), 2500


def _cap_batch(rng):
    """three samples of 900, exactly 1100 and 1700 cells under a cap of 1100; each cell once and 50 repeats, dealt.  The coordinates
    are moved onto multiples of 1/64 (still strictly inside their cells: 0.16 of the narrowest cell) so that the reference-made fixture
    of 3850 points and 3100 voxels compresses below the size of ``vox_batch.npz``; what this case is for is the integer half"""
    def sample(founders):
        ids = rng.choice(volume(VC.G32), founders, replace=False)
        deal = rng.permutation(np.concatenate([ids, rng.choice(ids, 50)]))
        p = (np.round(VC._in_cells(rng, deal, VC.G32, 3) * F32(64)) / F32(64)).astype(F32)
        assert np.array_equal(VC.cells_ref(p, VC.G32), deal)
        return p
    return VC._case('cap_batch', VC.G32, [sample(n) for n in CAP_BATCH_FOUNDERS], 4, 1100)


def _corners(g):
    gx, gy, gz = g['grid']
    return [cell_id(g, x, y, z) for x in (0, gx - 1) for y in (0, gy - 1) for z in (0, gz - 1)]


def _big_points(rng):
    ids = _corners(G_BIG) + [cell_id(G_BIG, 1023, 511, 1022)]
    return VC._case('big_points', G_BIG, [VC._in_cells(rng, rng.permutation(np.repeat(ids, 2)), G_BIG, 5)], 3, 20)


def _recipe_corners(rng):
    ids = _corners(VC.G_RECIPE) + [cell_id(VC.G_RECIPE, 511, 1023, 20)]
    return VC._case('recipe_corners', VC.G_RECIPE, [VC._in_cells(rng, rng.permutation(np.repeat(ids, 2)), VC.G_RECIPE, 5)], 3, 20)


def _t1(rng):
    cells = rng.choice(4096, 40, replace=False)
    return VC._case('T1', VC.G16, [VC._in_cells(rng, rng.permutation(np.concatenate([cells, rng.choice(cells, 260)])), VC.G16, 5)], 1, 50)


T256_ROWS = (300, 256, 255, 2, 1, 257, 29)


def _t256(rng):
    cells = rng.choice(4096, len(T256_ROWS), replace=False)
    return VC._case('T256', VC.G16, [VC._in_cells(rng, rng.permutation(np.repeat(cells, T256_ROWS)), VC.G16, 19)], 256, 8, F=16)


def _all_empty(rng):
    return VC._case('all_empty', VC.G16, [np.zeros((0, 5), F32)] * 3, 3, 5)


def _ends_empty(rng):
    return VC._case('ends_empty', VC.G16, [np.zeros((0, 5), F32), VC._in_cells(rng, rng.integers(0, 4096, 60), VC.G16, 5), np.zeros((0, 5), F32)], 3, 100)


POINT_BUILDERS = dict(cap_batch=_cap_batch, big_points=_big_points, recipe_corners=_recipe_corners, T1=_t1, T256=_t256, all_empty=_all_empty,
                      ends_empty=_ends_empty)
POINT_NAMES = list(POINT_BUILDERS)
FIXTURES = ['cap_batch']       # run through the reference's own code (tests/golden/gen_vox_golden.py): grid_x == grid_z on G32
_made = {}


def case(name):
    """the case, made once per process from a seed of its own and left unchanged"""
    if name not in _made:
        builders, base = (TABLE_BUILDERS, 2000) if name in TABLE_BUILDERS else (POINT_BUILDERS, 3000)
        seed = base + list(builders).index(name)
        _made[name] = builders[name](np.random.default_rng(seed))
        _made[name]['seed'] = seed
    return _made[name]


_shared = {}


def reference(name):
    """a point case's restatement in the form ``test_zz_vox_gpu._check`` takes, computed once and left unchanged"""
    if name not in _shared:
        c = case(name)
        cells = [VC.cells_ref(p, c) for p in c['points']]
        assigned = [VC.assign_ref(ce, c['T'], c['max_voxels']) for ce in cells]
        per = [VC.hard_voxelize_ref(p, c) for p in c['points']]
        feats, coords, sizes = VC.batch_ref(c, reduce=True)
        raw = VC.batch_ref(c, reduce=False)[0]
        _shared[name] = dict(c=c, cells=cells, assigned=assigned, per=per, feats=feats, coords=coords, sizes=sizes, raw=raw,
                             mean64=VC.mean_f64(raw, sizes))
    return _shared[name]


def replan_calls():
    """the calls of the re-plan part on the points of ``tiles4097``: ('one', rows) for ``voxelize``, ('batch', [rows, ...]) for
    ``voxelize_batch`` - large, small, B = 3, large again, B = 3 in another order"""
    p = VC.case('tiles4097')['points'][0]
    slices = [p[:1500], p[1500:1507], p[1507:]]
    return [('one', p), ('one', p[:10]), ('batch', slices), ('one', p), ('batch', slices[::-1])]
