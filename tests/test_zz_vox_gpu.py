"""The device-side hard voxelisation on an MI355X (include/ddp_vox_mi355x.h, ddp_amd/vox.py, ddp_amd/bev/voxelize.py) on the cases of
tests/vox_cases.py.  The workspace and every output buffer are exactly sized, guarded and filled with ``support.PATTERN``; every
integer output and ``voxels`` are compared bit for bit with the sequential restatement (and, for ``vox_cases.FIXTURES``, with the
arrays recorded from the reference's own code); the means are held to ``vox_cases.mean_f64``'s bound around float64.  The
restatement of a case is computed once and left unchanged.  The parts run inside TWO tests, and the first part loops over the cases,
as tests/test_dlss_gpu.py does: the GPU suite had 5000 test ids before these two.  The file's name sorts behind every other test
file on purpose: a record of the GPU suite that keeps its first 5000 ids in collection order keeps all the earlier ones, and these two
come last.  Every part of a test runs and every failing part is reported, under its name and its case.  Reads only tests/golden/ and
tests/vox_cases.py."""
import os

import numpy as np
import pytest
import torch

import parity_report
import vox_cases as VC
from ddp_amd import _vox_lib as M
from ddp_amd import registry
from ddp_amd import vox as L
from ddp_amd.bev.voxelize import Voxelization
from support import PATTERN, Guarded, assert_guards, dev  # noqa: F401

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vox')
PAT = np.int32(PATTERN)
_shared = {}


def _reference(name):
    """per case, computed once: per sample the cell ids, the assignment and the reference triple; the batched outputs; the f64 means"""
    if name not in _shared:
        c = VC.case(name)
        cells = [VC.cells_ref(p, c) for p in c['points']]
        assigned = [VC.assign_ref(ce, c['T'], c['max_voxels']) for ce in cells]
        per = [VC.hard_voxelize_ref(p, c) for p in c['points']]
        feats, coords, sizes = VC.batch_ref(c, reduce=True)
        raw = VC.batch_ref(c, reduce=False)[0]
        _shared[name] = dict(c=c, cells=cells, assigned=assigned, per=per, feats=feats, coords=coords, sizes=sizes, raw=raw,
                             mean64=VC.mean_f64(raw, sizes))
    return _shared[name]


class Rig:
    """a case (or some samples of it) on the device: a HardVoxelizer in an exactly sized, guarded, PATTERN-filled workspace, and such
    output buffers for gather and both forms of pack"""

    def __init__(self, c, dev, samples=None, pmax=None):
        self.c, self.dev = c, dev
        self.samples = list(range(c['B'])) if samples is None else samples
        B, V, T, F = len(self.samples), c['max_voxels'], c['T'], c['F']
        self.B, self.pmax = B, max([c['counts'][b] for b in self.samples] + [1]) if pmax is None else pmax
        self.hv = L.HardVoxelizer(c['voxel_size'], c['range'], T, V)
        assert self.hv.grid == c['grid']
        need = self.hv.workspace_bytes(B, self.pmax, F)
        assert need == VC.workspace_bytes(B, self.pmax, V, T)
        self.ws = Guarded(need, dev)
        self.hv.use_workspace(self.ws.ws.view(torch.uint8))
        shapes = dict(voxels=(B, V, T, F), coors=(B, V, 3), num=(B, V), feats=(B * V, F), coords=(B * V, 4), sizes=(B * V,), raw=(B * V, T, F),
                      coords_raw=(B * V, 4), sizes_raw=(B * V,))
        self.g = {k: Guarded(4 * int(np.prod(s)), dev) for k, s in shapes.items()}
        self.out = {k: (self.g[k].ws if k in ('voxels', 'feats', 'raw') else self.g[k].ws.view(torch.int32)).view(shapes[k]) for k in shapes}
        self.points = [torch.from_numpy(c['points'][b]).to(dev) for b in self.samples]

    def enqueue(self):
        o = self.out
        self.hv.cells(self.points, pmax=self.pmax, feats=self.c['F']).assign()
        self.hv.gather(out=(o['voxels'], o['coors'], o['num']))
        self.hv.pack(True, out=(o['feats'], o['coords'], o['sizes']))
        self.hv.pack(False, out=(o['raw'], o['coords_raw'], o['sizes_raw']))

    def intact(self, what):
        torch.cuda.synchronize()
        for k, g in dict(self.g, workspace=self.ws).items():
            assert_guards(g, f'{self.c["name"]} {what}: {k}')

    def read(self):
        """-> the outputs and the tables as int32 / float32 arrays (bits: every buffer is compared as int32 where PATTERN matters)"""
        self.intact('run')
        got = {k: v.cpu().numpy().copy() for k, v in self.out.items()}
        got.update(zip(('cells', 'pvox', 'table', 'vcell', 'counts'), (t.cpu().numpy().copy() for t in self.hv.tables())))
        return got

    def run(self):
        self.enqueue()
        return self.read()

    def state(self, got):
        """the bytes of everything a caller can see"""
        return b''.join(got[k].tobytes() for k in sorted(got) if k != 'vcell') + b''.join(
            got['vcell'][b, :got['counts'][b]].tobytes() for b in range(self.B))       # voxel cells beyond M_b are not written


def _bits(a):
    return a.view(np.int32)


def _check(ref, got, samples=None):
    """every output of a run against the restatement -> the largest |mean - f64| / bound"""
    c = ref['c']
    samples = list(range(c['B'])) if samples is None else samples
    V, T, F = c['max_voxels'], c['T'], c['F']
    pmax = got['cells'].shape[1]
    row = 0
    for i, b in enumerate(samples):
        n = c['counts'][b]
        pvox, table, vcells = ref['assigned'][b]
        voxels, coors, num = ref['per'][b]
        m = len(table)
        assert got['counts'][i] == m == len(voxels), (b, got['counts'][i], m)
        assert np.array_equal(got['cells'][i, :n], ref['cells'][b]) and (got['cells'][i, n:] == -1).all(), b
        assert np.array_equal(got['pvox'][i, :n], pvox) and (got['pvox'][i, n:] == -1).all(), b
        assert np.array_equal(got['table'][i, :m], table) and (got['table'][i, m:] == -1).all(), b
        assert np.array_equal(got['vcell'][i, :m], vcells), b
        # the reference's triple, bit for bit: +0.0 in the unused slots; rows >= M as the caller left them
        assert got['voxels'][i, :m].tobytes() == voxels.tobytes(), b
        assert np.array_equal(got['coors'][i, :m], coors) and np.array_equal(got['num'][i, :m], num), b
        assert (_bits(got['voxels'][i, m:]) == PAT).all() and (got['coors'][i, m:] == PAT).all() and (got['num'][i, m:] == PAT).all(), b
        # the batched rows of this sample
        for key in ('coords', 'coords_raw'):
            assert (got[key][row:row + m, 0] == i).all() and np.array_equal(got[key][row:row + m, 1:], coors), (b, key)
        assert np.array_equal(got['sizes'][row:row + m], num) and np.array_equal(got['sizes_raw'][row:row + m], num), b
        assert got['raw'][row:row + m].tobytes() == voxels.tobytes(), b
        row += m
    for key in ('feats', 'raw'):
        assert (_bits(got[key][row:]) == PAT).all(), key
    for key in ('coords', 'coords_raw', 'sizes', 'sizes_raw'):
        assert (got[key][row:] == PAT).all(), key
    if row and samples[-1] == c['B'] - 1 and c['counts'][-1] and len(ref['per'][-1][0]):
        assert got['coords'][row - 1, 0] + 1 == len(samples)               # what ``extract_lidar_features`` takes as the batch size
    if samples != list(range(c['B'])):
        return 0.0
    # the means: inside the derived bound around float64, and the left-to-right fp32 sum of the header (by value: -0.0 == +0.0)
    want, bound = ref['mean64']
    assert row == len(want)
    err = np.abs(got['feats'][:row].astype(np.float64) - want)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f'{c["name"]}: largest |device mean - f64| / bound = {ratio:.4f} over {row} voxels')
    assert (err <= bound).all(), ratio
    assert np.array_equal(got['feats'][:row], ref['feats'])
    return ratio


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def _each(names, check, dev):
    for name in names:
        try:
            check(name, dev)
        except AssertionError as e:
            raise AssertionError(f'case {name}: {e}') from e


def _part_every_case_equals_the_sequential_result(dev):
    _each(VC.NAMES, _case_equals_the_sequential_result, dev)


def _case_equals_the_sequential_result(name, dev):
    ref = _reference(name)
    c = ref['c']
    got = Rig(c, dev).run()
    ratio = _check(ref, got)
    if name in ('one', 'empty', 'all_out'):
        assert got['counts'].tolist() == [1 if name == 'one' else 0]
    if name in VC.FIXTURES:                                                # the reference's own arrays
        fix = VC.load_fixture(name, GOLDEN)
        for b in range(c['B']):
            m = int(got['counts'][b])
            assert got['voxels'][b, :m].tobytes() == fix[f'voxels{b}'].tobytes() and np.array_equal(got['coors'][b, :m], fix[f'coors{b}'])
            assert np.array_equal(got['num'][b, :m], fix[f'num{b}'])
        rows = len(fix['sizes'])
        assert rows == got['counts'].sum() and np.array_equal(got['coords'][:rows], fix['coords']) and np.array_equal(got['sizes'][:rows], fix['sizes'])
        assert got['raw'][:rows].tobytes() == fix['feats_raw'].tobytes()
        want, bound = ref['mean64']
        assert (np.abs(fix['feats'].astype(np.float64) - want) <= bound).all()
    parity_report.record(f'vox {name}: exact on cells, voxels, coors, num_points, coords, sizes; largest |device mean - f64| / ((n + 1) 2^-24 '
                         f'sum|x| / n) = {ratio:.4f}; source: {"reference fixture + restatement" if name in VC.FIXTURES else "restatement"}')


def _part_colliding_and_out_of_range_ids_from_a_callers_table(dev):
    """``assign_from_cells``: 96 distinct ids with ONE home slot by the documented hash, dealt three times each through a permutation,
    between ids the library must count as -1 (-1, volume, INT_MAX, INT_MIN) and ids with other homes"""
    pmax, T, V = 400, 3, 120
    H = M.hash_capacity(pmax)
    # a grid of 128^3 cells: every home slot of the 1024 has about 2000 of them
    g = VC._geometry((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (128, 128, 128))
    volume = 128 ** 3
    ids = np.arange(volume, dtype=np.uint64)
    home = (((ids * np.uint64(M.HASH_MULT)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - (H.bit_length() - 1))).astype(np.int64)
    slot = int(np.bincount(home, minlength=H).argmax())
    same = ids[home == slot][:96].astype(np.int64)
    assert len(same) == 96 and all(M.home_slot(int(i), pmax) == slot for i in same)
    rng = np.random.default_rng(7)
    neighbours = ids[(home == (slot + 1) % H) | (home == (slot + 2) % H)][:8].astype(np.int64)     # their homes are taken by the probing
    table = np.concatenate([np.repeat(same, 3), neighbours, np.asarray([-1, volume, 2 ** 31 - 1, -2 ** 31, volume + 5, -7])])
    table = rng.permutation(table)
    assert len(table) <= pmax
    table = np.concatenate([table, np.full(pmax - len(table), -1)]).astype(np.int32).reshape(1, pmax)
    cells = np.where((table[0] >= 0) & (table[0] < volume), table[0], -1).astype(np.int32)
    pvox, want, vcells = VC.assign_ref(cells, T, V)
    assert len(want) == 96 + 8 and (want >= 0).sum() == 96 * 3 + 8
    hv = L.HardVoxelizer(g['voxel_size'], g['range'], T, V)
    ws = Guarded(hv.workspace_bytes(1, pmax), dev)
    hv.use_workspace(ws.ws.view(torch.uint8))
    first = None
    for order in range(3):
        ws.ws.view(torch.int32).fill_(PATTERN)
        hv.assign_from_cells(torch.from_numpy(table).to(dev))
        torch.cuda.synchronize()
        assert_guards(ws, 'collide')
        gc, gp, gt, gv, gm = (t.cpu().numpy() for t in hv.tables())
        assert gm.tolist() == [104] and np.array_equal(gc[0], cells) and np.array_equal(gp[0], pvox)
        assert np.array_equal(gt[0, :104], want) and (gt[0, 104:] == -1).all() and np.array_equal(gv[0, :104], vcells)
        state = (gc.tobytes(), gp.tobytes(), gt.tobytes(), gv[0, :104].tobytes())
        first = first or state
        assert state == first, order
    with pytest.raises(RuntimeError, match='made without points'):
        hv.gather()


def _part_reruns_and_the_workspace_content_do_not_show(dev):
    """three runs give identical bytes; so does a run whose workspace held zeros, not the NaN pattern, before the call"""
    for name in ('dups', 'cap', 'batch'):
        ref = _reference(name)
        rig = Rig(ref['c'], dev)
        states = []
        for fill in (PATTERN, PATTERN, PATTERN, 0):
            rig.ws.ws.view(torch.int32).fill_(fill)
            for g in rig.g.values():
                g.ws.view(torch.int32).fill_(PATTERN)
            got = rig.run()
            _check(ref, got)
            states.append(rig.state(got))
        assert states[0] == states[1] == states[2] == states[3], name


def _part_batch_equals_single_calls_and_smaller_buffers_suffice(dev):
    ref = _reference('batch')
    c = ref['c']
    both = Rig(c, dev).run()
    row = 0
    for b in range(c['B']):
        one = Rig(c, dev, samples=[b])
        got = one.run()
        _check(ref, got, samples=[b])
        m = int(got['counts'][0])
        assert m == both['counts'][b] and got['voxels'][0, :m].tobytes() == both['voxels'][b, :m].tobytes()
        assert np.array_equal(got['coords'][:m, 1:], both['coords'][row:row + m, 1:]) and (both['coords'][row:row + m, 0] == b).all()
        assert got['feats'][:m].tobytes() == both['feats'][row:row + m].tobytes() and got['raw'][:m].tobytes() == both['raw'][row:row + m].tobytes()
        row += m
    assert row == both['counts'].sum() and both['coords'][row - 1, 0] + 1 == c['B']
    # a larger pmax than any count changes nothing the caller sees
    wide = Rig(c, dev, pmax=max(c['counts']) + 777).run()
    _check(ref, wide)


def _part_replayed_graph_follows_rewritten_points(dev):
    ref = _reference('cap')
    c = ref['c']
    rig = Rig(c, dev)
    rig.run()                                                              # every buffer exists before the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                          # one stream, no branches
        rig.enqueue()
    # the same count, other points: the rows reversed and turned a quarter about z - another founder order and other cells
    old = c['points'][0]
    new = old[::-1].copy()
    new[:, 0], new[:, 1] = -old[::-1, 1] * np.float32(32 / 36 * 0.1 / 0.15), old[::-1, 0] * np.float32(36 / 32 * 0.15 / 0.1)
    c2 = dict(c, points=[new])
    want = Rig(c2, dev).run()
    assert want['table'].tobytes() != rig.read()['table'].tobytes()
    rig.points[0].copy_(torch.from_numpy(new))
    rig.ws.ws.view(torch.int32).fill_(PATTERN)
    for g in rig.g.values():
        g.ws.view(torch.int32).fill_(PATTERN)
    graph.replay()
    got = rig.read()
    assert rig.state(got) == rig.state(want)
    pvox, table, vcells = VC.assign_ref(VC.cells_ref(new, c), c['T'], c['max_voxels'])
    assert np.array_equal(got['table'][0, :len(table)], table) and got['counts'].tolist() == [len(table)]


class _Model:
    pass


def _part_plugin_and_patched_model_equal_the_engine(dev):
    ref = _reference('batch')
    c = ref['c']
    caps = (c['max_voxels'] + 50, c['max_voxels'])
    module = Voxelization(c['voxel_size'], c['range'], c['T'], caps, deterministic=False).eval()
    points = [torch.from_numpy(p).to(dev) for p in c['points']]
    before = [p.clone() for p in points]
    kept = []
    for b, p in enumerate(points):
        voxels, coors, num = module(p)
        kept.append((voxels, coors, num))
        want = ref['per'][b]
        assert voxels.dtype == torch.float32 and coors.dtype == num.dtype == torch.int32
        assert voxels.shape == want[0].shape and coors.shape == want[1].shape and num.shape == want[2].shape
    for (voxels, coors, num), want in zip(kept, ref['per']):               # tensors of their own: a later call left them alone
        assert voxels.cpu().numpy().tobytes() == want[0].tobytes() and np.array_equal(coors.cpu().numpy(), want[1]) and np.array_equal(num.cpu().numpy(), want[2])
    # training mode takes the other cap
    module.train()
    m_train = len(VC.hard_voxelize_ref(c['points'][2], c, max_voxels=caps[0])[0])
    assert module(points[2])[0].shape[0] == m_train > c['max_voxels']
    # the patched model: BEVFusion.voxelize for the whole batch in one call
    for reduce, key in ((True, 'feats'), (False, 'raw')):
        model = object.__new__(_Model)
        model.encoders = {'lidar': {'voxelize': Voxelization(c['voxel_size'], c['range'], c['T'], caps).eval()}}
        model.voxelize_reduce = reduce
        registry.use_device_voxelization(model)
        feats, coords, sizes = model.voxelize(points)
        again = model.voxelize(points[::-1])                               # a second call does not reach into the first one's tensors
        assert np.array_equal(feats.cpu().numpy(), ref[key]) and np.array_equal(coords.cpu().numpy(), ref['coords']) and np.array_equal(sizes.cpu().numpy(), ref['sizes'])
        assert int(coords[-1, 0]) + 1 == c['B'] and again[1][0, 0] == 0
    assert all(torch.equal(p, q) for p, q in zip(points, before))           # the caller's points are only read
    # a non-contiguous view and more columns than feats: read in place / copied, never written
    wide = torch.cat([points[0], torch.full((len(points[0]), 2), 9.0, device=dev)], 1)
    voxels, coors, num = module.eval().engine().voxelize(wide[:, :5])
    assert voxels.cpu().numpy().tobytes() == ref['per'][0][0].tobytes() and (wide[:, 5:] == 9.0).all()


# ---- the two tests ---------------------------------------------------------------------------------------------------------------------
def _parts(parts, dev):
    """every part runs, whatever the parts before it found (an AssertionError only: any other error ends the test at once, and nothing
    more is started on the card); the failures are reported together, each under its part's name"""
    failed = []
    for part in parts:
        try:
            part(dev)
        except AssertionError as e:
            failed.append(f'{part.__name__[6:]}: {e}')
    assert not failed, f'{len(failed)} of {len(parts)} parts failed:\n' + '\n'.join(failed)


def test_cases_and_injected_tables(dev):
    """every case of vox_cases.NAMES against the sequential restatement and the reference's fixtures; ``assign_from_cells`` on colliding
    and out-of-range ids"""
    _parts([_part_every_case_equals_the_sequential_result, _part_colliding_and_out_of_range_ids_from_a_callers_table], dev)


def test_reruns_batches_graph_and_plugin(dev):
    """three reruns and a zeroed workspace give the same bytes, a batch equals single calls, a replayed graph follows rewritten points,
    the plugin's ``forward`` and the patched ``model.voxelize`` equal the engine and leave the caller's points alone"""
    _parts([_part_reruns_and_the_workspace_content_do_not_show, _part_batch_equals_single_calls_and_smaller_buffers_suffice,
            _part_replayed_graph_follows_rewritten_points, _part_plugin_and_patched_model_equal_the_engine], dev)
