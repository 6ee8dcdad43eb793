"""The device-side LSS lift and pool on an MI355X (include/ddp_lss_mi355x.h, ddp_amd/lss.py, ddp_amd/bev/lss.py) on the cases of
tests/lss_cases.py.  Every buffer is exactly sized and guarded; the workspace and the output are pre-filled with 0xFF bytes (NaN as
floats, -1 as integers).

  1  the rank table of ``plan`` against the float64 restatement, every point (a point within DELTA of a cell boundary may take
     either side): the geometric cases (``NAMES``)
  2  ``pool`` on injected ranks against the float64 sum over the same table, inside the derived bound; empty cells exactly +0.0:
     the geometric cases and the synthetic rank tables (``SYNTH_NAMES``: chosen list lengths at 64 to 193 channels, 1025 scan tiles)
  3  pool(plan(matrices)) is bit-identical to pool(plan_from_ranks(ranks())): the geometric cases
  4  ten runs give the same bits (ranks, lists, output) and leave a plan whose segment lengths are the counts of its rank table,
     cell for cell (``odd``, ``cfg``, ``long``, ``tiles``, ``c256``; ``lens_c193`` and ``scan`` through ``plan_from_ranks``);
     B = 2 equals two B = 1 calls (``odd``, ``tiles``); a replayed graph follows new inputs
  5  the plugin on the fixtures' state dicts, ``downsample`` 1 and 2 (2 where nz = 1): the geometric cases
The parts loop over their cases inside one test each: the GPU suite stays below 5000 test ids.
Reads only tests/golden/ and tests/lss_cases.py."""
import os

import numpy as np
import pytest
import torch

import lss_cases as LC
import parity_report
from ddp_amd import lss as L
from ddp_amd.bev.lss import LSSTransform

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lss')
GUARD = 4096          # bytes on either side of every buffer the library writes


def _guarded_bytes(n):
    buf = torch.full((n + 2 * GUARD,), 0xFF, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 256 == 0
    return buf, buf[GUARD:GUARD + n]


def _intact(buf):
    return bool((buf[:GUARD] == 0xFF).all() and (buf[-GUARD:] == 0xFF).all())


class Rig:
    """one case on the device: an ``LssPool`` in an exactly sized, guarded, 0xFF-filled workspace, and such an output"""

    def __init__(self, c, B=None):
        s = c['spec']
        self.c, self.B, self.N = c, B or c['B'], c['N']
        self.pool = L.LssPool(s['image'], s['feature'], s['xbound'], s['ybound'], s['zbound'], s['dbound'], c['C'])
        need = self.pool.workspace_bytes(self.B, self.N)
        assert need == LC.workspace_bytes(c, self.B, self.N)
        self.wsbuf, self.ws = _guarded_bytes(need)
        self.pool.use_workspace(self.ws)
        self.shape = (self.B, c['nx'][2] * c['C'], c['nx'][0], c['nx'][1])
        self.outbuf, out = _guarded_bytes(4 * int(np.prod(self.shape)))
        self.out = out.view(torch.float32).view(self.shape)

    def refill(self):
        self.ws.fill_(0xFF)
        self.out.view(-1).view(torch.uint8).fill_(0xFF)

    def run_pool(self, x):
        got = self.pool.pool(x, out=self.out)
        assert got.data_ptr() == self.out.data_ptr()
        torch.cuda.synchronize()
        assert _intact(self.wsbuf) and _intact(self.outbuf)
        return self.out.cpu().numpy().copy()


def _regions(rig):
    """what a plan and a pool leave in the workspace, by the layout of include/ddp_lss_mi355x.h: rank table, offsets, the sorted
    lists, probabilities and context rows.  The unsorted lists between them are scratch: their order is the atomics' and k_lss_sort
    removes it."""
    c = rig.c
    P, K, X = rig.B * rig.N * c['D'] * c['fH'] * c['fW'], rig.B * c['K'] // c['B'], rig.B * rig.N * c['fH'] * c['fW']
    r = lambda n: (n + 255) // 256 * 256
    words = rig.ws.view(torch.int32).cpu().numpy()
    at = np.cumsum([0, r(4 * P), r(4 * (K + 1)), r(4 * K) + r(4 * ((K + 1023) // 1024)), r(4 * P), r(4 * P), r(4 * P)]) // 4
    ranks, offs = words[at[0]:][:P], words[at[1]:][:K + 1]
    kept = int((ranks >= 0).sum())
    return dict(ranks=ranks, offs=offs, lists=words[at[4]:][:kept], prob=words[at[5]:][:P], rows=words[at[6]:][:X * c['C']])


def _same_regions(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def _cameras(c, b=None):
    sl = slice(None) if b is None else slice(b, b + 1)
    m = lambda k: c[k][sl].cuda()
    c2l, intr, aug, laug = m('camera2lidar'), m('camera_intrinsics'), m('img_aug_matrix'), m('lidar_aug_matrix')
    return L.pack_cameras(c2l[..., :3, :3], c2l[..., :3, 3], intr[..., :3, :3], aug[..., :3, :3], aug[..., :3, 3], laug[..., :3, :3], laug[..., :3, 3])


_shared = {}


def _reference(name):
    """per case, computed once and left unchanged: the float64 cells, the fp32 restatement's ranks, the depthnet output of the
    fixture's weights, the float64 pool over the fp32 ranks; for a synthetic case its own rank table and input, and the float64 pool"""
    if name in LC.SYNTH and name not in _shared:
        c = LC.synth(name)
        want, absum, lists = LC.pool_f64(c, c['x'].numpy(), c['ranks'])
        _shared[name] = dict(c=c, r32=c['ranks'], x=c['x'], want=want, absum=absum, lists=lists, bound=LC.pool_bound(c, absum, lists))
    if name not in _shared:
        c = LC.case(name)
        fix = LC.load_fixture(name, GOLDEN)[0]
        q64 = LC.cells_f64(c)
        r32 = LC.ranks_of(c, LC.cells_f32(c))[0]
        x = LC.depthnet_out(c, fix['sd/depthnet.weight'], fix['sd/depthnet.bias']).contiguous()
        want, absum, lists = LC.pool_f64(c, x.numpy(), r32)
        _shared[name] = dict(c=c, fix=fix, q64=q64, r32=r32, x=x, want=want, absum=absum, lists=lists, bound=LC.pool_bound(c, absum, lists))
    return _shared[name]


def _check_pool(name, got, what):
    ref = _reference(name)
    err = np.abs(got.astype(np.float64) - ref['want'])
    assert np.isfinite(got).all(), what
    assert (err <= ref['bound']).all(), (what, float((err / np.maximum(ref['bound'], 1e-300)).max()))
    empty = ref['absum'] == 0
    assert (got[empty] == 0).all() and not np.signbit(got[empty]).any(), what          # exactly +0.0
    filled = ref['bound'] > 0
    return float((err[filled] / ref['bound'][filled]).max()) if filled.any() else 0.0


def _each(names, check):
    for name in names:
        try:
            check(name)
        except AssertionError as e:
            raise AssertionError(f'case {name}: {e}') from e


# ---- 1: ranks ------------------------------------------------------------------------------------------------------------------------
def test_rank_table_against_float64():
    """one test for all the cases (each is a few launches on small shapes, and the GPU suite stays below 5000 test ids); a failure
    names its case"""
    _each(LC.NAMES, _rank_table_against_float64)


def _rank_table_against_float64(name):
    ref = _reference(name)
    c = ref['c']
    rig = Rig(c)
    rig.pool.plan(*_cameras(c))
    ranks = rig.pool.ranks()
    assert ranks.shape == (c['B'], c['N'], c['D'], c['fH'], c['fW']) and ranks.dtype == torch.int32
    torch.cuda.synchronize()
    assert _intact(rig.wsbuf)
    got = ranks.cpu().numpy().reshape(-1)
    near = LC.near_boundary(ref['q64'])
    assert near.mean() <= LC.EXCUSED_SHARE
    ok = LC.admissible(c, ref['q64'], got)
    assert ok.all(), (name, np.flatnonzero(~ok)[:8], got[~ok][:8])
    r64 = LC.ranks_of(c, ref['q64'])[0]
    assert np.array_equal(got[~near], r64[~near])
    if name == 'empty':
        assert (got == -1).all()
    parity_report.record(f'lss {name}: {int((got != ref["r32"]).sum())} of {got.size} device ranks differ from the fp32 restatement, '
                         f'{int((got != r64).sum())} from float64; {int(near.sum())} points ({near.mean():.4%}) within {LC.DELTA} of a boundary')


# ---- 2: pool on injected ranks -------------------------------------------------------------------------------------------------------
def test_pool_on_injected_ranks_within_the_bound():
    """one test for all the cases (each is a few launches on small shapes, and the GPU suite stays below 5000 test ids); a failure
    names its case"""
    _each(LC.NAMES + LC.SYNTH_NAMES, _pool_on_injected_ranks_within_the_bound)


def _pool_on_injected_ranks_within_the_bound(name):
    ref = _reference(name)
    c = ref['c']
    rig = Rig(c)
    table = torch.from_numpy(ref['r32']).view(c['B'], c['N'], c['D'], c['fH'], c['fW']).cuda()
    rig.pool.plan_from_ranks(table)
    assert torch.equal(rig.pool.ranks(), table)
    got = rig.run_pool(ref['x'].cuda())
    ratio = _check_pool(name, got, name)
    if name == 'empty':
        assert not got.any() and not np.signbit(got).any()
    parity_report.record(f'lss {name}: pool on injected ranks, largest |dev - f64| / ((L + D + 32) 2^-24 sum|p f|) = {ratio:.4f} '
                         f'(longest list {int(ref["lists"].max())}, D {c["D"]})')


def test_out_of_range_injected_ranks_count_as_dropped():
    ref = _reference('c3')
    c = ref['c']
    rig = Rig(c)
    table = torch.from_numpy(ref['r32']).view(c['B'], c['N'], c['D'], c['fH'], c['fW']).cuda()
    bad = table.clone()
    dropped = bad < 0
    bad[dropped] = torch.tensor([c['K'], -7, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device='cuda').repeat(int(dropped.sum()) // 4 + 1)[:int(dropped.sum())]
    rig.pool.plan_from_ranks(bad)
    assert torch.equal(rig.pool.ranks(), table)
    _check_pool('c3', rig.run_pool(ref['x'].cuda()), 'c3 with out-of-range ranks')


# ---- 3: bit identity of the two plans ------------------------------------------------------------------------------------------------
def test_plan_from_matrices_equals_plan_from_its_ranks():
    """one test for all the cases (each is a few launches on small shapes, and the GPU suite stays below 5000 test ids); a failure
    names its case"""
    _each(LC.NAMES, _plan_from_matrices_equals_plan_from_its_ranks)


def _plan_from_matrices_equals_plan_from_its_ranks(name):
    ref = _reference(name)
    c = ref['c']
    x = ref['x'].cuda()
    a = Rig(c)
    a.pool.plan(*_cameras(c))
    out_a = a.run_pool(x)
    ranks = a.pool.ranks().clone()
    b = Rig(c)
    b.pool.plan_from_ranks(ranks)
    out_b = b.run_pool(x)
    assert out_a.tobytes() == out_b.tobytes()
    assert _same_regions(_regions(a), _regions(b))                        # ranks, offsets, lists, probabilities, rows


# ---- 4: determinism ------------------------------------------------------------------------------------------------------------------
def test_ten_runs_give_the_same_bits():
    """one test for all the cases (each is a few launches on small shapes, and the GPU suite stays below 5000 test ids); a failure
    names its case"""
    _each(['odd', 'cfg', 'long', 'tiles', 'c256', 'lens_c193', 'scan'], _ten_runs_give_the_same_bits)


def _ten_runs_give_the_same_bits(name):
    ref = _reference(name)
    c = ref['c']
    x = ref['x'].cuda()
    if name in LC.SYNTH:                                                  # no geometry: the plan is that of the injected table
        table = torch.from_numpy(ref['r32']).view(c['B'], c['N'], c['D'], c['fH'], c['fW']).cuda()
        plan = lambda: rig.pool.plan_from_ranks(table)
    else:
        cam, extra = _cameras(c)
        plan = lambda: rig.pool.plan(cam, extra)
    rig = Rig(c)
    first = None
    for i in range(10):
        rig.refill()
        plan()
        out = rig.run_pool(x)
        state = (_regions(rig), out.tobytes())                            # rank table, offsets, lists, probabilities, rows; output
        if first is None:
            first = state
        assert _same_regions(state[0], first[0]) and state[1] == first[1], i
    # no 0xFF word of the refill is left where the plan lives: ranks, offsets and every list entry were written
    ranks, offs, lists = first[0]['ranks'], first[0]['offs'], first[0]['lists']
    kept = lists.size
    assert np.array_equal(ranks, rig.pool.ranks().reshape(-1).cpu().numpy())
    assert offs[0] == 0 and offs[-1] == kept and (np.diff(offs) >= 0).all()
    if name in LC.SYNTH:
        assert np.array_equal(ranks, ref['r32'])
    # every segment is as long as its cell's count in the rank table, the empty cells too: a dropped tile start or a dropped count
    # of the scan's tail shows here even where the cells around it are empty
    assert offs.size == c['K'] + 1 and np.array_equal(np.diff(offs), np.bincount(ranks[ranks >= 0], minlength=c['K']))
    assert np.array_equal(np.sort(lists), np.flatnonzero(ranks >= 0))
    for cell in np.flatnonzero(np.diff(offs) > 0):
        seg = lists[offs[cell]:offs[cell + 1]]
        assert (ranks[seg] == cell).all() and (np.diff(seg) > 0).all(), cell       # ascending point order


def test_batch_of_two_equals_two_single_calls():
    """``odd``: two slabs per sample; ``tiles``: the second sample's cells start in the middle of a scan tile"""
    _each(['odd', 'tiles'], _batch_of_two_equals_two_single_calls)


def _batch_of_two_equals_two_single_calls(name):
    ref = _reference(name)
    c = ref['c']
    assert c['B'] == 2
    x = ref['x'].cuda()
    both = Rig(c)
    both.pool.plan(*_cameras(c))
    out = both.run_pool(x)
    ranks = both.pool.ranks().cpu().numpy()
    per = c['N']
    for b in range(2):
        one = Rig(c, B=1)
        one.pool.plan(*_cameras(c, b))
        got = one.run_pool(x[b * per:(b + 1) * per].contiguous())
        assert got.tobytes() == out[b:b + 1].tobytes(), b
        r1 = one.pool.ranks().cpu().numpy()
        assert np.array_equal(np.where(r1 >= 0, r1 + b * c['K'] // 2, -1), ranks[b:b + 1])


def test_replayed_graph_follows_new_matrices_and_features():
    ref = _reference('runs')
    c = ref['c']
    rig = Rig(c)
    cam, extra = _cameras(c)
    x = ref['x'].cuda().clone()

    def enqueue():
        rig.pool.plan(cam, extra)
        rig.pool.pool(x, out=rig.out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enqueue()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    # new matrices (the rig turned by 40 degrees and moved) and new features
    turn = torch.tensor([[0.766, -0.643, 0.0], [0.643, 0.766, 0.0], [0.0, 0.0, 1.0]], device='cuda')
    extra2 = torch.cat([(turn @ extra[:, :9].view(-1, 3, 3)).reshape(-1, 9), extra[:, 9:] + torch.tensor([1.0, -2.0, 0.5], device='cuda')], 1)
    x2 = torch.from_numpy(np.random.default_rng(9).uniform(-2, 2, tuple(x.shape)).astype(np.float32)).cuda()
    eager = Rig(c)
    eager.pool.plan(cam, extra2.contiguous())
    want = eager.run_pool(x2)
    want_ranks = eager.pool.ranks().clone()
    assert not torch.equal(want_ranks, rig.pool.ranks())
    extra.copy_(extra2)
    x.copy_(x2)
    rig.refill()
    graph.replay()
    torch.cuda.synchronize()
    assert _intact(rig.wsbuf) and _intact(rig.outbuf)
    assert torch.equal(rig.pool.ranks(), want_ranks) and rig.out.cpu().numpy().tobytes() == want.tobytes()


# ---- 5: plugin -----------------------------------------------------------------------------------------------------------------------
def test_plugin_on_the_fixtures():
    """one test for all the cases (each is a few launches on small shapes, and the GPU suite stays below 5000 test ids); a failure
    names its case"""
    _each(LC.NAMES, _plugin_on_the_fixtures)


def _plugin_on_the_fixtures(name):
    ref = _reference(name)
    c = ref['c']
    for ds, fix in zip((1, 2), LC.load_fixture(name, GOLDEN)):
        if fix is None:
            continue
        sd = LC.state_dict_of(fix)
        m = LSSTransform(downsample=ds, **c['kwargs'])
        m.load_state_dict(sd, strict=True)
        m = m.cuda().eval()
        seen = {}
        m.downsample.register_forward_pre_hook(lambda mod, inp: seen.setdefault('pooled', inp[0].detach().clone()))
        out = m(*LC.forward_args(c, 'cuda'))
        torch.cuda.synchronize()
        pooled = seen['pooled'].cpu().numpy()
        # before downsample: the float64 sum over the DEVICE's ranks (tests 1 and 3 cover those), inside the bound of test 2
        ranks = m.pooler.ranks().cpu().numpy().reshape(-1)
        assert LC.admissible(c, ref['q64'], ranks).all()
        # depthnet ran on the device, and the bound of test 2 is that of the pool alone: the sum is taken over the module's own
        # depthnet output
        x_dev = m.depthnet(c['img'].cuda().view(c['B'] * c['N'], -1, c['fH'], c['fW'])).detach().cpu().numpy()
        want, absum, lists = LC.pool_f64(c, x_dev, ranks)
        bound = LC.pool_bound(c, absum, lists)
        err = np.abs(pooled - want)
        assert (err <= bound).all(), (name, ds, float((err / np.maximum(bound, 1e-300)).max()))
        assert (pooled[absum == 0] == 0).all()
        # after downsample: within 4 x the distance of the fixture's own fp32 output from the float64 restatement
        gold = fix['out']
        assert out.shape == gold.shape
        m64 = LSSTransform(downsample=ds, **c['kwargs'])
        m64.load_state_dict(sd, strict=True)
        with torch.no_grad():
            x64 = m64.depthnet.double()(c['img'].double().view(c['B'] * c['N'], -1, c['fH'], c['fW'])).numpy()
            pooled64 = LC.pool_f64(c, x64, LC.load_fixture(name, GOLDEN)[0]['ranks'])[0]
            out64 = m64.downsample.double().eval()(torch.from_numpy(pooled64)).numpy()
        dist = float(np.abs(gold - out64).max())
        mine = float(np.abs(out.cpu().numpy() - out64).max())
        same_ranks = np.array_equal(ranks, LC.load_fixture(name, GOLDEN)[0]['ranks'])
        parity_report.record(f'lss {name} downsample={ds}: plugin {mine:.3e} from the float64 restatement, the fixture {dist:.3e}; '
                             f'device ranks equal the fixture\'s: {same_ranks}')
        assert mine <= 4 * dist, (name, ds, mine, dist)
