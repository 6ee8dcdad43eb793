"""The device-side front of ``DepthLSSTransform`` on an MI355X (include/ddp_dlss_mi355x.h, ddp_amd/dlss.py, ddp_amd/bev/depth_lss.py) on
the cases of tests/dlss_cases.py.  Every buffer the library writes is exactly sized and guarded; the workspace and the outputs are
pre-filled with 0xFF bytes (NaN as floats, -1 as integers).

  1  the tables of ``project`` against the float64 restatement, every (sample, camera, point)
  2  ``scatter_from_tables`` against ``winner_scatter``, bit for bit; out-of-range and -1 entries
  3  ``scatter()`` after ``project()`` equals ``scatter_from_tables(tables())``
  4  the stem inside ``stem_bound`` of ``stem_f64``; an all-zero image; an image wider than one tile
  5  ten runs give the same bytes; 6  B = 2 equals two B = 1 calls; 7  a replayed graph follows new inputs
  8  the plugin on the fixtures, ``downsample`` 1 and 2
The eight parts run inside TWO tests, and each part loops over its cases, as tests/test_lss_gpu.py does: the GPU suite stays below 5000
test ids (4997 before these two).  Every part of a test runs and every failing part is reported, under its name and its case.
Reads only tests/golden/, tests/dlss_cases.py and tests/lss_cases.py."""
import os

import numpy as np
import pytest
import torch

import dlss_cases as DC
import lss_cases as LC
import parity_report
from ddp_amd import dlss as L
from ddp_amd.bev.depth_lss import DepthLSSTransform

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dlss')
GUARD = 4096          # bytes on either side of every buffer the library writes


def _guarded_bytes(n):
    buf = torch.full((n + 2 * GUARD,), 0xFF, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 256 == 0
    return buf, buf[GUARD:GUARD + n]


def _intact(buf):
    return bool((buf[:GUARD] == 0xFF).all() and (buf[-GUARD:] == 0xFF).all())


class Rig:
    """one case on the device: a ``LidarDepth`` in an exactly sized, guarded, 0xFF-filled workspace, such an image and such a stem output"""

    def __init__(self, c, samples=None, pmax=None):
        self.c = c
        self.samples = list(range(c['B'])) if samples is None else samples
        self.B, self.N = len(self.samples), c['N']
        self.pmax = (max(c['counts'][b] for b in self.samples) if pmax is None else pmax)
        self.ld = L.LidarDepth(c['spec']['image'])
        need = self.ld.workspace_bytes(self.B, self.N, self.pmax)
        assert need == DC.workspace_bytes(c, self.B, self.N, self.pmax)
        self.wsbuf, self.ws = _guarded_bytes(need)
        self.ld.use_workspace(self.ws)
        self.shape = (self.B, self.N, 1, c['iH'], c['iW'])
        self.imgbuf, img = _guarded_bytes(4 * int(np.prod(self.shape)))
        self.image = img.view(torch.float32).view(self.shape)
        oH, oW = DC.stem_size(c['spec']['image'])
        self.stem_shape = (self.B * self.N, 32, oH, oW)
        self.stembuf, st = _guarded_bytes(4 * int(np.prod(self.stem_shape)))
        self.stem_out = st.view(torch.float32).view(self.stem_shape)
        sl = self.samples
        self.points = [c['points'][b].cuda() for b in sl]
        self.lidar, self.cam = L.pack_lidar(c['lidar2image'][sl].cuda(), c['img_aug_matrix'][sl].cuda(), c['lidar_aug_matrix'][sl].cuda())

    def refill(self):
        self.ws.fill_(0xFF)
        self.image.view(-1).view(torch.uint8).fill_(0xFF)
        self.stem_out.view(-1).view(torch.uint8).fill_(0xFF)

    def project(self):
        self.ld.project_packed(self.points, self.lidar, self.cam, pmax=self.pmax)
        return self

    def intact(self):
        torch.cuda.synchronize()
        return _intact(self.wsbuf) and _intact(self.imgbuf) and _intact(self.stembuf)

    def tables(self):
        pix, dep = self.ld.tables()
        return pix.cpu().numpy().copy(), dep.cpu().numpy().copy()

    def scatter(self):
        got = self.ld.scatter(out=self.image)
        assert got.data_ptr() == self.image.data_ptr() and self.intact()
        return self.image.cpu().numpy().copy()

    def scatter_from(self, pix, dep):
        self.ld.scatter_from_tables(torch.as_tensor(pix).cuda(), torch.as_tensor(dep).cuda(), out=self.image)
        assert self.intact()
        return self.image.cpu().numpy().copy()

    def stem(self, image, dtransform):
        self.ld.stem(image, dtransform, out=self.stem_out)
        assert self.intact()
        return self.stem_out.cpu().numpy().copy()


_shared = {}


def _reference(name):
    """per case, computed once and left unchanged: the float64 chain and its tables, the fp32 restatement's tables, the depth bound"""
    if name not in _shared:
        c = DC.case(name)
        ch64 = DC.project(c, torch.float64)
        rc64 = DC.rowcol_table(c, [rc for rc, z in ch64])
        pix64, dep64 = DC.tables_of(c, ch64)
        fix = DC.load_fixture(name, GOLDEN) if name in DC.FIXTURES else None
        pix32, dep32 = DC.tables_of(c, DC.project(c, torch.float32, inverse=None if fix is None else fix['lidar_aug_inverse']))
        _shared[name] = dict(c=c, rc64=rc64, pix64=pix64, dep64=dep64, pix32=pix32, dep32=dep32, terms=DC.depth_terms(c), fix=fix, raw=DC.raw_z(c),
                             counted=DC.counted_mask(c), finite=DC.finite_mask(c),
                             near=DC.near_boundary(c, rc64), image32=DC.winner_scatter(c, pix32, dep32))
    return _shared[name]


def _module(c, fix, ds=1):
    m = DepthLSSTransform(downsample=ds, **c['kwargs'])
    sd = DC.state_dict_of(fix)
    if ds == 2:
        sd.update(DC.state_dict_of(fix, 'sd2/'))
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def _each(names, check):
    for name in names:
        try:
            check(name)
        except AssertionError as e:
            raise AssertionError(f'case {name}: {e}') from e


def _check_tables(ref, pix, dep, b0=0, nb=None, clamped=None):
    """the device's tables of samples b0 .. b0 + nb against float64 -> (excused pairs, on-image pairs, largest depth ratio);
    ``clamped``: a [lower, upper] counter of the entries checked for the exact clamp ends"""
    clamped = [0, 0] if clamped is None else clamped
    c = ref['c']
    sl = slice(b0, b0 + (c['B'] if nb is None else nb))
    P = pix.shape[2]
    rc64, pix64, dep64, terms, near, raw, counted, finite = (ref[k][sl][:, :, :P] for k in ('rc64', 'pix64', 'dep64', 'terms', 'near', 'raw', 'counted', 'finite'))
    counted, finite = np.broadcast_to(counted, pix.shape), np.broadcast_to(finite, pix.shape)
    assert pix.dtype == np.int32 and dep.dtype == np.float32 and pix.shape == dep.shape == pix64.shape
    assert (pix[~counted] == -1).all() and (dep[~counted] == 0).all() and not np.signbit(dep[~counted]).any()      # the padding
    assert (pix[counted & ~finite] == -1).all()                            # a non-finite coordinate drops the point, in every camera
    ok = DC.admissible(c, rc64, pix)
    assert ok[counted].all(), (np.argwhere(~ok & counted)[:8], pix[~ok & counted][:8])
    assert np.array_equal(pix[counted & ~near], pix64[counted & ~near])
    on = pix64 >= 0
    excused = int((near & on).sum())
    assert excused <= DC.EXCUSED_SHARE * max(int(on.sum()), 1)
    # the depth table of the finite points: |dev - f64| <= 16 * 2^-24 * S (dlss_cases.depth_terms)
    bound = DC.DEPTH_ULPS * 2.0 ** -24 * terms
    lo, hi = np.float32(DC.Z_LO), np.float32(DC.Z_HI)
    err = np.abs(dep.astype(np.float64) - dep64)
    # a clamped entry too: float32(1e-5) lies 2.6e-13 from the float64 end, far inside the bound of the terms that formed the raw z
    assert (err[finite] <= bound[finite]).all(), float((err[finite] / bound[finite]).max())
    assert (dep[finite] >= lo).all() and (dep[finite] <= hi).all()
    # the clamp ends are exact: wherever the RAW float64 z lies a bound beyond an end, the table holds that end's fp32 value
    below, above = finite & (raw <= DC.Z_LO - bound), finite & (raw >= DC.Z_HI + bound)
    assert (dep[below] == lo).all() and (dep[above] == hi).all()
    clamped[0] += int(below.sum())
    clamped[1] += int(above.sum())
    free = finite & (raw > DC.Z_LO) & (raw < DC.Z_HI)
    ratio = float((err[free] / bound[free]).max()) if free.any() else 0.0
    return excused, int(on.sum()), ratio


# ---- 1: tables -------------------------------------------------------------------------------------------------------------------------
def _part_tables_against_float64():
    """Depth bound: z is formed by a subtraction, a 3 x 3 product (a product and two additions per term), a second one and a shift - 8
    roundings on the path of a term, (1 + u)^8 - 1 < 8.1 u - and the device multiplies by the fp32 ``torch.inverse`` of a similarity
    (condition 1: a few u per entry).  16 u S with S the sum of the absolute terms leaves a factor two; the largest observed ratio goes
    to the parity report.  One test for all the cases; a failure names its case."""
    _each(DC.NAMES, _tables_against_float64)


def _tables_against_float64(name):
    ref = _reference(name)
    c = ref['c']
    rig = Rig(c).project()
    assert rig.intact()
    pix, dep = rig.tables()
    assert pix.shape == (c['B'], c['N'], c['pmax'])
    clamped = [0, 0]
    excused, on, ratio = _check_tables(ref, pix, dep, clamped=clamped)
    assert clamped[0] > 0 or name == 'one'                                 # every case but the one-camera one has a camera at a point's back
    assert clamped[1] == (DC.EXTRAS_ABOVE if name == 'wide' else 0)        # the upper end: the far points of ``wide``
    if name == 'behind':
        assert ((dep[0, 0] == np.float32(1e-5)) & (pix[0, 0] >= 0)).sum() >= 1
    if name == 'wide':
        # the four points every camera drops (NaN, +-inf, inf after x / 1e-5): pixel -1, and the image is that of the other points
        gone = ~ref['finite'][0, 0] | (c['points'][0][:, 1].numpy() > 1e30)
        assert gone.sum() == DC.EXTRAS_DROPPED and (pix[0][:, gone] == -1).all()
        kept_pix, kept_dep = pix.copy(), dep.copy()
        kept_pix[0][:, gone], kept_dep[0][:, gone] = -1, 0.0
        assert rig.scatter().tobytes() == DC.winner_scatter(c, kept_pix, kept_dep).tobytes() and not np.isnan(rig.image.cpu().numpy()).any()
    parity_report.record(f'dlss {name}: {int((pix != ref["pix32"]).sum())} of {pix.size} device pixels differ from the fp32 restatement, '
                         f'{int((pix != ref["pix64"]).sum())} from float64; {excused} of {on} on-image pairs within {DC.DELTA} px of a boundary; '
                         f'depth table: largest |dev - f64| / (16 2^-24 S) = {ratio:.4f}, {int((dep.view(np.int32) != ref["dep32"].view(np.int32)).sum())} entries differ from fp32; '
                         f'{clamped[0]} + {clamped[1]} entries checked for the exact clamp ends')


# ---- 2: scatter on injected tables -----------------------------------------------------------------------------------------------------
def _part_scatter_on_injected_tables_is_exact():
    _each(DC.NAMES, _scatter_on_injected_tables_is_exact)


def _scatter_on_injected_tables_is_exact(name):
    ref = _reference(name)
    c = ref['c']
    rig = Rig(c)
    got = rig.scatter_from(ref['pix32'], ref['dep32'])
    assert got.tobytes() == ref['image32'].tobytes()
    empty = np.ones(got.shape, dtype=bool).reshape(c['B'], c['N'], -1)
    for b in range(c['B']):
        for n in range(c['N']):
            empty[b, n, ref['pix32'][b, n][ref['pix32'][b, n] >= 0]] = False
    assert (got.reshape(empty.shape)[empty] == 0).all() and not np.signbit(got.reshape(empty.shape)[empty]).any()       # +0.0
    if ref['fix'] is not None:
        assert got.tobytes() == ref['fix']['depth'].tobytes()              # the reference's own image, bit for bit


def _part_out_of_range_injected_pixels_count_as_off_the_image():
    ref = _reference('rig')
    c = ref['c']
    HW = c['iH'] * c['iW']
    bad = ref['pix32'].copy()
    off = np.flatnonzero(bad.reshape(-1) < 0)
    bad.reshape(-1)[off] = np.resize(np.array([HW, -7, 2 ** 31 - 1, -2 ** 31, HW + 5, -1], dtype=np.int64), off.size).astype(np.int32)
    dep = ref['dep32'].copy()
    dep.reshape(-1)[off] = 12345.0                                           # a depth no pixel may show
    assert off.size > 6
    got = Rig(c).scatter_from(bad, dep)
    assert got.tobytes() == ref['image32'].tobytes() and not (got == 12345.0).any()
    # a table without any entry (Pmax = 0) and one made of -1: all-zero images
    rig = Rig(c, pmax=0)
    z = rig.scatter_from(np.zeros((1, c['N'], 0), np.int32), np.zeros((1, c['N'], 0), np.float32))
    assert not z.any() and not np.signbit(z).any()
    z = Rig(c).scatter_from(np.full_like(bad, -1), dep)
    assert not z.any() and not np.signbit(z).any()


# ---- 3: scatter after project ----------------------------------------------------------------------------------------------------------
def _part_scatter_after_project_equals_scatter_from_its_tables():
    _each(DC.NAMES, _scatter_after_project_equals_scatter_from_its_tables)


def _scatter_after_project_equals_scatter_from_its_tables(name):
    ref = _reference(name)
    c = ref['c']
    a = Rig(c).project()
    pix, dep = a.tables()
    img_a = a.scatter()
    img_b = Rig(c).scatter_from(pix, dep)
    assert img_a.tobytes() == img_b.tobytes() == DC.winner_scatter(c, pix, dep).tobytes()
    if name == 'odd':
        assert not img_a[1].any() and not np.signbit(img_a[1]).any()       # the sample without a point


# ---- 4: stem ---------------------------------------------------------------------------------------------------------------------------
def _check_stem(got, image, sd, what):
    want, terms = DC.stem_f64(image, sd)
    bound = DC.stem_bound(terms)
    err = np.abs(got.astype(np.float64) - want)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    assert (err <= bound).all(), (what, float((err / bound).max()))
    return float((err / bound).max()), want


def _part_stem_inside_the_bound():
    """``stem_bound`` (dlss_cases): per element (200 + 16) 2^-24 times the absolute terms - K = 200 products and their additions, the
    folded affines of both stages.  On the fixtures' depth images, on an all-zero image (the constant-plus-padding pattern) and on an
    image wider than one tile of 64 output columns."""
    _each(DC.FIXTURES, _stem_inside_the_bound)
    # wider than a tile (oW = 75: two tiles along x, the second partial), rows no multiple of four, sparse like a depth image
    c = dict(DC.case('one'))
    c['spec'] = dict(c['spec'], image=(14, 298))
    c.update(iH=14, iW=298, B=1, N=2, counts=[0], pmax=0)
    fix = _reference('rig')['fix']
    m = _module(_reference('rig')['c'], fix)
    rng = np.random.default_rng(5)
    image = np.where(rng.uniform(size=(1, 2, 1, 14, 298)) < 0.05, rng.uniform(1.0, 60.0, (1, 2, 1, 14, 298)), 0.0).astype(np.float32)
    rig = Rig(c, samples=[0], pmax=0)
    got = rig.stem(torch.from_numpy(image).cuda(), m.dtransform)
    assert got.shape == (2, 32, 4, 75)
    ratio, _ = _check_stem(got, image, DC.state_dict_of(fix), 'wide image')
    parity_report.record(f'dlss stem 14 x 298 (two tiles along x): largest |dev - f64| / bound = {ratio:.4f}')


def _stem_inside_the_bound(name):
    ref = _reference(name)
    c, fix = ref['c'], ref['fix']
    m = _module(c, fix)
    sd = DC.state_dict_of(fix)
    rig = Rig(c)
    got = rig.stem(torch.from_numpy(fix['depth']).cuda(), m.dtransform)
    ratio, want = _check_stem(got, fix['depth'], sd, name)
    with torch.no_grad():
        eager = m.dtransform[0:6](torch.from_numpy(fix['depth']).cuda().flatten(0, 1)).cpu().numpy()
    rig.refill()
    zeros = rig.stem(torch.zeros(rig.shape, device='cuda'), m.dtransform)
    ratio0, want0 = _check_stem(zeros, np.zeros(rig.shape, np.float32), sd, name + ' zeros')
    # the pattern: one constant per channel wherever the whole window lies on the image, other values where taps lie in the padding
    oH, oW = want0.shape[2:]
    rows = [y for y in range(oH) if 4 * y - 2 >= 0 and 4 * y + 2 < c['iH']]
    cols = [x for x in range(oW) if 4 * x - 2 >= 0 and 4 * x + 2 < c['iW']]
    if rows and cols:
        inner = zeros[:, :, rows][:, :, :, cols]
        assert (inner == inner[:1, :, :1, :1]).all()
        assert (want0[0, :, 0, 0] != want0[0, :, rows[0], cols[0]]).any()                  # the corner window sees padding: another constant
    parity_report.record(f'dlss {name}: stem largest |dev - f64| / ((200 + 16) 2^-24 terms) = {ratio:.4f} (zeros {ratio0:.4f}); '
                         f'eager torch on the same card {float(np.abs(eager - want).max()):.3e} from f64, the kernel {float(np.abs(got - want).max()):.3e}')


# ---- 5: determinism --------------------------------------------------------------------------------------------------------------------
def _part_ten_runs_give_the_same_bytes():
    _each(['dups', 'wide'], _ten_runs_give_the_same_bytes)


def _ten_runs_give_the_same_bytes(name):
    ref = _reference(name)
    c = ref['c']
    fix = _reference('rig')['fix']
    m = _module(_reference('rig')['c'], fix)
    rig = Rig(c)
    first = None
    for i in range(10):
        rig.refill()
        rig.project()
        pix, dep = rig.tables()
        img = rig.scatter()
        st = rig.stem(rig.image, m.dtransform)
        state = (pix.tobytes(), dep.tobytes(), img.tobytes(), st.tobytes())
        if first is None:
            first = state
            fin = np.broadcast_to(ref['finite'], dep.shape)
            assert not np.isnan(img).any() and not np.isnan(st).any() and not np.isnan(dep[fin]).any()   # no 0xFF word of the refill is left
        assert state == first, i


# ---- 6: batch = singles ----------------------------------------------------------------------------------------------------------------
def _part_batch_of_two_equals_two_single_calls():
    _each(['odd', 'wide'], _batch_of_two_equals_two_single_calls)


def _batch_of_two_equals_two_single_calls(name):
    ref = _reference(name)
    c = ref['c']
    assert c['B'] == 2
    fix = _reference('rig')['fix']
    m = _module(_reference('rig')['c'], fix)
    both = Rig(c).project()
    pix, dep = both.tables()
    img = both.scatter()
    st = both.stem(both.image, m.dtransform)
    for b in range(2):
        one = Rig(c, samples=[b]).project()
        p1, d1 = one.tables()
        n = c['counts'][b]
        assert p1.shape[2] == n
        assert np.array_equal(p1, pix[b:b + 1, :, :n]) and d1.tobytes() == np.ascontiguousarray(dep[b:b + 1, :, :n]).tobytes()
        assert (pix[b, :, n:] == -1).all() and (dep[b, :, n:] == 0).all()
        i1 = one.scatter()
        assert i1.tobytes() == img[b:b + 1].tobytes(), b
        s1 = one.stem(one.image, m.dtransform)
        assert s1.tobytes() == st[b * c['N']:(b + 1) * c['N']].tobytes(), b
        _check_tables(ref, p1, d1, b0=b, nb=1)


# ---- 7: graph --------------------------------------------------------------------------------------------------------------------------
def _part_replayed_graph_follows_new_points_and_matrices():
    ref = _reference('wide')
    c = ref['c']
    fix = _reference('rig')['fix']
    m = _module(_reference('rig')['c'], fix)
    rig = Rig(c)

    def enqueue():
        rig.project()
        rig.ld.scatter(out=rig.image)
        rig.ld.stem(rig.image, m.dtransform, out=rig.stem_out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enqueue()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    old = rig.image.cpu().numpy().copy()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    # new points (the same counts: every point moved) and new matrices (the cloud turned by 40 degrees and shifted), in place
    turn = torch.tensor([[0.766, -0.643, 0.0], [0.643, 0.766, 0.0], [0.0, 0.0, 1.0]], device='cuda')
    lidar2 = torch.cat([(turn @ rig.lidar[:, :9].view(-1, 3, 3)).reshape(-1, 9), rig.lidar[:, 9:] + torch.tensor([1.0, -2.0, 0.5], device='cuda')], 1)
    points2 = [p.flip(0).contiguous() * torch.tensor([1.0, 0.9, 1.1, 1.0, 1.0], device='cuda') for p in rig.points]
    eager = Rig(c)
    eager.points, eager.lidar = points2, lidar2.contiguous()
    eager.project()
    want_pix, want_dep = eager.tables()
    want_img = eager.scatter()
    want_stem = eager.stem(eager.image, m.dtransform)
    assert want_img.tobytes() != old.tobytes()
    rig.lidar.copy_(lidar2)
    for p, q in zip(rig.points, points2):
        p.copy_(q)
    rig.refill()
    graph.replay()
    assert rig.intact()
    pix, dep = rig.tables()
    assert np.array_equal(pix, want_pix) and dep.tobytes() == want_dep.tobytes()
    assert rig.image.cpu().numpy().tobytes() == want_img.tobytes() and rig.stem_out.cpu().numpy().tobytes() == want_stem.tobytes()


# ---- 8: plugin -------------------------------------------------------------------------------------------------------------------------
def _part_plugin_on_the_fixtures():
    """the depth image: admissible under test 1 and, where no pair is excused, the fixture's bit for bit; the output: within 4 x the
    distance of the fixture's own fp32 output from the float64 restatement evaluated on the DEVICE's depth image (the rule of
    ``test_plugin_on_the_fixtures`` of tests/test_lss_gpu.py); ``points`` as they were."""
    _each(DC.FIXTURES, _plugin_on_the_fixtures)


def _plugin_on_the_fixtures(name):
    ref = _reference(name)
    c, fix = ref['c'], ref['fix']
    ranks32 = LC.ranks_of(c, LC.cells_f32(c))[0]
    for ds in (1, 2):
        if ds == 2 and c['nx'][2] != 1:
            continue
        m = _module(c, fix, ds)
        args = DC.forward_args(c, 'cuda')
        out = m(*args)
        torch.cuda.synchronize()
        assert all(torch.equal(p.cpu(), q) for p, q in zip(args[1], c['points']))              # the caller's points are only read
        pix, dep = (t.cpu().numpy() for t in m.lidar_depth.tables())
        excused, on, ratio = _check_tables(ref, pix, dep)
        depth = m.depth_image(args[1], args[5], args[8], args[9]).cpu().numpy()
        assert depth.tobytes() == DC.winner_scatter(c, pix, dep).tobytes()
        same = depth.tobytes() == fix['depth'].tobytes()
        if excused == 0:
            assert same
        ranks = m.pooler.ranks().cpu().numpy().reshape(-1)
        assert LC.admissible(c, LC.cells_f64(c), ranks).all()
        gold = fix['out'] if ds == 1 else fix['out2']
        assert out.shape == gold.shape
        out64 = DC.forward_f64(c, m, depth, ranks32)
        dist = float(np.abs(gold - out64).max())
        mine = float(np.abs(out.cpu().numpy() - out64).max())
        parity_report.record(f'dlss {name} downsample={ds}: plugin {mine:.3e} from the float64 restatement, the fixture {dist:.3e}; device depth '
                             f'image equals the fixture\'s: {same} ({excused} pairs excused); device ranks equal the fp32 restatement\'s: '
                             f'{np.array_equal(ranks, ranks32)}')
        assert mine <= 4 * dist, (name, ds, mine, dist)


# ---- the two tests ---------------------------------------------------------------------------------------------------------------------
def _parts(parts):
    """every part runs, whatever the parts before it found (an AssertionError only: any other error ends the test at once, and nothing
    more is started on the card); the failures are reported together, each under its part's name"""
    failed = []
    for part in parts:
        try:
            part()
        except AssertionError as e:
            failed.append(f'{part.__name__[6:]}: {e}')
    assert not failed, f'{len(failed)} of {len(parts)} parts failed:\n' + '\n'.join(failed)


def test_tables_scatter_and_stem():
    """parts 1 - 4: the tables against float64 (the depth bound's derivation: ``_part_tables_against_float64``), the scatter on injected
    tables bit for bit, out-of-range entries, ``scatter()`` after ``project()``, the stem inside its bound (``_part_stem_inside_the_bound``)"""
    _parts([_part_tables_against_float64, _part_scatter_on_injected_tables_is_exact, _part_out_of_range_injected_pixels_count_as_off_the_image,
            _part_scatter_after_project_equals_scatter_from_its_tables, _part_stem_inside_the_bound])


def test_reruns_batches_graph_and_plugin():
    """parts 5 - 8: ten runs give the same bytes, a batch of two equals two single calls, a replayed graph follows new points and
    matrices, the plugin on the fixtures (``_part_plugin_on_the_fixtures``)"""
    _parts([_part_ten_runs_give_the_same_bytes, _part_batch_of_two_equals_two_single_calls, _part_replayed_graph_follows_new_points_and_matrices,
            _part_plugin_on_the_fixtures])
