"""CPU side of the device-side front of ``DepthLSSTransform`` (tests/test_dlss_gpu.py runs the cases on an MI355X): the fixtures recorded
from the reference's own class equal the restatements of tests/dlss_cases.py (the depth image bit for bit); every case holds the witnesses
its name promises; the reference's fp32 pixel coordinates lie within DELTA / 4 of float64; the near-boundary share stays below 1 %; the
reference's own stem output lies inside the stem bound; the library is a library of its own (exports, hash, stamp, ABI); every refusal
happens before any launch; the workspace formula; no kernel touches scratch; the device-free plugin surface.  No GPU compute is invoked."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import dlss_cases as DC
import lss_cases as LC
from ddp_amd import _cm_lib, build, registry
from ddp_amd import _dlss_lib as M
from ddp_amd import dlss as L
from ddp_amd.bev.depth_lss import DepthLSSTransform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'dlss')

_shared = {}


def _chains(name):
    """per case, computed once and left unchanged: the fp32 chain (with the fp32 inverse the fixture recorded), the float64 one"""
    if name not in _shared:
        c = DC.case(name)
        inv = DC.load_fixture(name, GOLDEN)['lidar_aug_inverse'] if name in DC.FIXTURES else None
        ch32 = DC.project(c, torch.float32, inverse=inv)
        ch64 = DC.project(c, torch.float64)
        _shared[name] = (c, ch32, ch64)
    return _shared[name]


# ---- fixture = restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', DC.FIXTURES)
def test_fixture_depth_image_is_the_winner_scatter_of_the_fp32_tables(name):
    c, ch32, ch64 = _chains(name)
    fix = DC.load_fixture(name, GOLDEN)
    assert int(fix['seed']) == c['seed']
    for k in ('img', 'lidar2image', 'camera2lidar', 'camera_intrinsics', 'img_aug_matrix', 'lidar_aug_matrix'):
        assert np.array_equal(fix[k], c[k].numpy()), k
    for b, p in enumerate(c['points']):
        assert np.array_equal(fix[f'points{b}'], p.numpy()) and p.shape == (c['counts'][b], c['stride'])
    # the recorded fp32 inverse of lidar_aug: a few ulps from the float64 inverse of the same matrix
    inv64 = torch.inverse(c['lidar_aug_matrix'][:, :3, :3].double()).numpy()
    assert fix['lidar_aug_inverse'].dtype == np.float32 and np.abs(fix['lidar_aug_inverse'] - inv64).max() <= 4 * 2.0 ** -24 * np.abs(inv64).max()
    pix, dep = DC.tables_of(c, ch32)
    assert pix.dtype == np.int32 and dep.dtype == np.float32 and pix.shape == dep.shape == (c['B'], c['N'], c['pmax'])
    want = DC.winner_scatter(c, pix, dep)
    assert fix['depth'].shape == (c['B'], c['N'], 1, c['iH'], c['iW']) and fix['depth'].dtype == np.float32
    assert want.tobytes() == fix['depth'].tobytes()                         # bit for bit, +0.0 where no point falls
    assert not np.signbit(fix['depth'][fix['depth'] == 0]).any()
    oH, oW = DC.stem_size(c['spec']['image'])
    assert fix['stem'].shape == (c['B'] * c['N'], 32, oH, oW)
    assert fix['out'].shape == (c['B'], c['nx'][2] * c['C'], c['nx'][0], c['nx'][1])
    if c['nx'][2] == 1:
        assert fix['out2'].shape == (c['B'], c['C'], (c['nx'][0] + 1) // 2, (c['nx'][1] + 1) // 2)
    else:
        assert 'out2' not in fix.files and name == 'odd'


def test_last_wins_is_not_first_wins():
    """the rule is pinned: a scatter in which the SMALLEST index wins gives another image on the case made of duplicates"""
    c, ch32, ch64 = _chains('dups')
    pix, dep = DC.tables_of(c, ch32)
    first = DC.winner_scatter(c, pix[:, :, ::-1], dep[:, :, ::-1])
    assert not np.array_equal(first, DC.load_fixture('dups', GOLDEN)['depth'])


# ---- witnesses -----------------------------------------------------------------------------------------------------------------------
def test_each_name_keeps_its_promise():
    c, ch32, ch64 = _chains('one')
    assert (c['B'], c['N'], c['iH'], c['iW'], c['counts'], c['fH'], c['fW']) == (1, 1, 5, 9, [7], 1, 2)
    assert DC.stem_size((5, 9)) == (2, 3) and c['iH'] % 4 and c['iW'] % 4 and c['counts'][0] < 64
    c, ch32, ch64 = _chains('odd')
    assert (c['B'], c['N'], c['iH'], c['iW'], c['counts'], c['stride'], c['pmax']) == (2, 3, 23, 50, [300, 0], 5, 300)
    assert DC.stem_size((23, 50)) == (6, 13) and (c['fH'], c['fW']) == (3, 7)
    pix, dep = DC.tables_of(c, ch32)
    assert (pix[1] == -1).all() and (dep[1] == 0).all() and (pix[0] >= 0).any()              # the empty sample
    assert not DC.load_fixture('odd', GOLDEN)['depth'][1].any()
    c, ch32, ch64 = _chains('dups')
    pix, dep = DC.tables_of(c, ch32)
    assert (c['iH'], c['iW'], c['counts']) == (8, 12, [3000])
    per = [np.bincount(pix[0, n][pix[0, n] >= 0], minlength=96) for n in range(2)]
    assert all((p >= 2).all() for p in per) and max(p.max() for p in per) >= 64            # every pixel contested, one by >= 64
    c, ch32, ch64 = _chains('behind')
    assert (c['N'], c['iH'], c['iW']) == (2, 16, 24)
    pix, dep = DC.tables_of(c, ch32)
    raw = DC.raw_z(c)
    witness = (raw[0] < 0) & (pix[0] >= 0)
    assert witness.sum() >= 1 and (dep[0][witness] == np.float32(1e-5)).all()
    img = DC.load_fixture('behind', GOLDEN)['depth']
    assert (img == np.float32(1e-5)).sum() >= 1                                             # the clamped z is what the image stores
    c, ch32, ch64 = _chains('rig')
    assert (c['B'], c['N'], c['iH'], c['iW']) == (1, 6, 32, 88) and DC.stem_size((32, 88)) == (8, 22) and (c['fH'], c['fW']) == (4, 11)
    laug = c['lidar_aug_matrix'][0]
    assert abs(float(torch.det(laug[:3, :3])) - 1.05 ** 3) < 1e-4 and laug[0, 1] != 0 and laug[:3, 3].abs().min() > 0
    assert np.allclose(c['img_aug_matrix'][0, 0, 0, 0], 0.48 / 8) and 5000 < c['counts'][0] < 7000
    c, ch32, ch64 = _chains('wide')
    assert (c['B'], c['N'], c['iH'], c['iW']) == (2, 2, 64, 176) and c['counts'][0] != c['counts'][1]
    # its six points no lidar gives: two beyond the upper clamp end, four that every camera drops (non-finite, or inf after x / 1e-5)
    raw, (pix, dep) = DC.raw_z(c), DC.tables_of(c, ch32)
    assert ((raw[0] > 1e5) & (dep[0] == np.float32(1e5))).sum() == DC.EXTRAS_ABOVE == (dep[0] == np.float32(1e5)).sum() == (raw[0] > 1e5).sum()
    gone = ~DC.finite_mask(c)[0, 0, :c['counts'][0]] | (c['points'][0][:, 1].numpy() > 1e30)
    assert gone.sum() == DC.EXTRAS_DROPPED and (pix[0][:, :c['counts'][0]][:, gone] == -1).all() and DC.finite_mask(c)[1, 0, :c['counts'][1]].all()
    rc32 = DC.rowcol_table(c, [rc for rc, z in ch32])[0][:, :c['counts'][0]][:, c['points'][0][:, 1].numpy() > 1e30]
    assert not np.isfinite(rc32[1]).any() and np.isfinite(DC.rowcol_table(c, [rc for rc, z in ch64])[0][:, :c['counts'][0]][:, c['points'][0][:, 1].numpy() > 1e30]).all()
    oH, oW = DC.stem_size((64, 176))
    assert oH > 4 and c['B'] * c['N'] * ((oH + 3) // 4) > 1 and c['N'] * c['pmax'] > 256   # more tiles and more pairs than one block


# ---- the delta rule --------------------------------------------------------------------------------------------------------------------
def test_clamped_entries_are_the_clamp_ends_exactly():
    """selected by the RAW float64 z, a bound away from the end: the fp32 restatement holds float32(1e-5) / float32(1e5) there; every case
    with a camera at a point's back has lower-end entries, ``wide`` has the upper-end ones"""
    lo, hi = np.float32(DC.Z_LO), np.float32(DC.Z_HI)
    for name in DC.NAMES:
        c, ch32, ch64 = _chains(name)
        raw, dep = DC.raw_z(c), DC.tables_of(c, ch32)[1]
        with np.errstate(invalid='ignore'):
            bound = DC.DEPTH_ULPS * 2.0 ** -24 * DC.depth_terms(c)
            below, above = raw <= DC.Z_LO - bound, raw >= DC.Z_HI + bound
        assert (dep[below] == lo).all() and (dep[above] == hi).all()
        assert below.sum() > 0 or name == 'one'                          # ``one`` has one camera and every point in front of it
        assert (above.sum() == DC.EXTRAS_ABOVE) if name == 'wide' else not above.any()


def test_reference_fp32_pixel_coordinates_lie_within_a_quarter_of_delta_of_float64():
    assert DC.DELTA == 1e-3 == LC.DELTA
    worst = {}
    for name in DC.NAMES:
        c, ch32, ch64 = _chains(name)
        t32, t64 = DC.rowcol_table(c, [rc for rc, z in ch32]), DC.rowcol_table(c, [rc for rc, z in ch64])
        on = (DC.pixels_of(c, t64) >= 0) | (DC.pixels_of(c, t32) >= 0)
        worst[name] = float(np.abs(t32 - t64).max(-1)[on].max())
        # and the clamped depth
        z32, z64 = DC.tables_of(c, ch32)[1], DC.tables_of(c, ch64)[1]
        assert (np.abs(z32 - z64)[on] <= 4 * 2.0 ** -24 * np.abs(z64)[on] + DC.DEPTH_ULPS * 2.0 ** -24 * DC.depth_terms(c)[on]).all()
    print('largest |fp32 - float64| pixel distance per case:', worst)
    assert max(worst.values()) <= DC.DELTA / 4, worst


@pytest.mark.parametrize('name', DC.NAMES)
def test_near_boundary_share(name):
    c, ch32, ch64 = _chains(name)
    rc64 = [rc for rc, z in ch64]
    on, near = DC.on_image(c, rc64), DC.near_boundary(c, rc64)
    assert on.sum() > 0
    share = float((near & on).sum()) / float(on.sum())
    assert share <= DC.EXCUSED_SHARE
    if c['spec'].get('exact'):
        assert not near.any()
    # a pair away from every boundary has one admissible pixel, its own; the fp32 restatement is admissible everywhere
    p64 = DC.pixels_of(c, DC.rowcol_table(c, rc64))
    assert DC.admissible(c, rc64, p64).all()
    wrong = np.where(p64 >= 0, -1, 0).astype(np.int32)
    counted = np.broadcast_to(DC.counted_mask(c), p64.shape)
    assert not DC.admissible(c, rc64, wrong)[~near & counted].any()
    assert DC.admissible(c, rc64, DC.tables_of(c, ch32)[0]).all()


# ---- the stem bound holds for the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', DC.FIXTURES)
def test_reference_stem_output_lies_inside_the_bound(name):
    fix = DC.load_fixture(name, GOLDEN)
    want, terms = DC.stem_f64(fix['depth'], DC.state_dict_of(fix))
    err = np.abs(fix['stem'] - want)
    bound = DC.stem_bound(terms)
    assert (bound > 0).all() and (err <= bound).all(), float((err / bound).max())
    # the padding pads the stage-1 OUTPUT: with relu(bn(bias)) in the border instead of 0 the fixture is far outside the bound
    sd = DC.state_dict_of(fix)
    d = torch.from_numpy(fix['depth']).double().flatten(0, 1)
    w1, b1, g1, m1, be1 = DC._fold64(sd, 0, 1)
    w2, b2, g2, m2, be2 = DC._fold64(sd, 3, 4)
    a = torch.relu((w1.view(-1) * g1).view(1, -1, 1, 1) * torch.nn.functional.pad(d, (2, 2, 2, 2)) + ((b1 - m1) * g1 + be1).view(1, -1, 1, 1))
    mutant = torch.relu(torch.nn.functional.conv2d(a, w2 * g2.view(-1, 1, 1, 1), (b2 - m2) * g2 + be2, stride=4)).numpy()
    assert mutant.shape == want.shape and (np.abs(fix['stem'] - mutant) > bound).any()


# ---- the library's own (what every side library shares: tests/test_build_host.py) ------------------------------------------------------
def test_binding_matches_the_header():
    build.SIDE['dlss'].start(verbose=False)()
    header = open(os.path.join(ROOT, 'include', 'ddp_dlss_mi355x.h')).read()
    assert f'#define DDP_DLSS_STEM_FOLDED {M.STEM_FOLDED}' in header and M.STEM_FOLDED == 8 + 8 + 25 * 8 * 32 + 32
    assert (M.E_BADCFG, M.E_ALIGN, M.E_LAUNCH, M.E_NULL) == (_cm_lib.E_BADCFG, _cm_lib.E_ALIGN, _cm_lib.E_LAUNCH, _cm_lib.E_NULL)
    assert C.sizeof(M.Cfg) == 5 * 4 and C.sizeof(M.StemParams) == 12 * 8 + 2 * 8


def test_stale_or_missing_library_raises(tmp_path, monkeypatch):
    with pytest.raises(M.DdpDlssError, match='not found'):
        M.load(str(tmp_path / 'libddp_dlss.so'))
    monkeypatch.setattr(M._binding, 'libs', {})
    with monkeypatch.context() as m:
        m.setattr(build.SIDE['dlss'], 'built_hash', lambda: 'feedfeedfeedfeed')
        with pytest.raises(M.DdpDlssError, match='is stale'):
            M.load()
    monkeypatch.setattr(M._binding, 'abi_version', M.ABI_VERSION + 1)
    with pytest.raises(M.DdpDlssError, match='ABI mismatch: library 1 vs binding 2') as e:
        M.load()
    assert e.value.code is None and isinstance(e.value, RuntimeError) and not M._binding.libs


FAKE = 0x10000    # a non-NULL, 256-byte aligned "device pointer": every call below is refused before anything is enqueued


def _cfg(**over):
    cfg = M.Cfg(2, 3, 23, 50, 300)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def _stem_params(**over):
    p = M.StemParams(*([FAKE] * 12), 1e-5, 1e-5)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _calls(cfg, points=(FAKE, FAKE), counts=(300, 0), stride=5, lidar=FAKE, cam=FAKE, ws=FAKE, pix=FAKE, dep=FAKE, image=FAKE, out=FAKE,
           params=None, only=None):
    lib = M.load()
    n, p, q = C.c_size_t(0), C.c_void_p(0), C.c_void_p(0)
    B = max(cfg.batch, 1)
    ptrs = (C.c_void_p * B)(*(list(points) + [FAKE] * B)[:B]) if points is not None else None
    cnts = (C.c_int32 * B)(*(list(counts) + [0] * B)[:B]) if counts is not None else None
    params = params if params is not None else _stem_params()
    calls = dict(workspace=lambda: lib.ddp_dlss_workspace(C.byref(cfg), C.byref(n)),
                 project=lambda: lib.ddp_dlss_project(C.byref(cfg), ptrs, cnts, stride, lidar, cam, ws, None),
                 pixels=lambda: lib.ddp_dlss_pixels(C.byref(cfg), ws, C.byref(p), C.byref(q)),
                 scatter=lambda: lib.ddp_dlss_scatter(C.byref(cfg), ws, image, None),
                 scatter_from_tables=lambda: lib.ddp_dlss_scatter_from_tables(C.byref(cfg), pix, dep, ws, image, None),
                 stem=lambda: lib.ddp_dlss_stem(C.byref(cfg), image, C.byref(params), ws, out, None))
    return calls if only is None else calls[only]


def _refused(rc, code, words):
    msg = M.load().ddp_dlss_last_error().decode()
    assert rc == code and words in msg, (rc, msg, words)


def test_refusals_happen_before_any_launch():
    """no GPU is present where this runs: a call that got as far as a launch would fail with DDP_DLSS_E_LAUNCH, not with these"""
    bad = [(dict(batch=0), 'batch'), (dict(batch=-2), 'batch'), (dict(cams=0), 'cams'), (dict(image_h=0), 'image_h'), (dict(image_w=-3), 'image_w'),
           (dict(pmax=-1), 'pmax'), (dict(pmax=-2 ** 31), 'pmax'),                                     # what 2^31 looks like in an int32
           (dict(batch=1, cams=1, image_h=1 << 16, image_w=1 << 15), 'iH*iW'),                        # = 2^31
           (dict(batch=1, cams=1, image_h=46341, image_w=46341), 'iH*iW'),
           (dict(batch=2, cams=1, image_h=1 << 15, image_w=1 << 15), 'B*N*iH*iW'),
           (dict(batch=1 << 10, cams=1 << 10, image_h=1, image_w=1, pmax=1 << 11), 'B*N*pmax')]
    for over, words in bad:
        for name, call in _calls(_cfg(**over)).items():
            _refused(call(), M.E_BADCFG, words)
    # just below the limits: accepted
    n = C.c_size_t(0)
    assert M.load().ddp_dlss_workspace(C.byref(_cfg(batch=1, cams=1, image_h=1 << 15, image_w=(1 << 16) - 1, pmax=2 ** 31 - 1)), C.byref(n)) == 0
    assert n.value > 2 * 4 * (2 ** 31 - 1) + 4 * ((1 << 31) - (1 << 15))
    cfg = _cfg()
    _refused(_calls(cfg, stride=2, only='project')(), M.E_BADCFG, 'stride = 2')
    _refused(_calls(cfg, stride=0, only='project')(), M.E_BADCFG, 'stride = 0')
    _refused(_calls(cfg, counts=(300, -1), only='project')(), M.E_BADCFG, 'count[1] = -1')
    _refused(_calls(cfg, counts=(301, 0), only='project')(), M.E_BADCFG, 'exceeds pmax')
    _refused(_calls(cfg, params=_stem_params(bn2_eps=-1.0), only='stem')(), M.E_BADCFG, 'eps')
    _refused(_calls(cfg, params=_stem_params(bn1_eps=float('nan')), only='stem')(), M.E_BADCFG, 'eps')
    for kw, name, what in ((dict(points=None), 'project', 'h_points'), (dict(counts=None), 'project', 'h_counts'), (dict(points=(None, None)), 'project', 'h_points[b]'),
                           (dict(lidar=None), 'project', 'd_lidar'), (dict(cam=None), 'project', 'd_cam'), (dict(ws=None), 'project', 'd_workspace'),
                           (dict(ws=None), 'pixels', 'd_workspace'), (dict(ws=None), 'scatter', 'd_workspace'), (dict(image=None), 'scatter', 'd_image'),
                           (dict(pix=None), 'scatter_from_tables', 'd_pixels'), (dict(dep=None), 'scatter_from_tables', 'd_depths'),
                           (dict(ws=None), 'scatter_from_tables', 'd_workspace'), (dict(image=None), 'scatter_from_tables', 'd_image'),
                           (dict(image=None), 'stem', 'd_image'), (dict(ws=None), 'stem', 'd_workspace'), (dict(out=None), 'stem', 'd_out'),
                           (dict(params=_stem_params(d_bn2_var=None)), 'stem', 'd_bn2_var'), (dict(params=_stem_params(d_conv1_weight=None)), 'stem', 'd_conv1_weight')):
        _refused(_calls(cfg, only=name, **kw)(), M.E_NULL, what + ' is NULL')
    for kw, name, what in ((dict(points=(FAKE + 2, FAKE)), 'project', 'h_points[b]'), (dict(lidar=FAKE + 1), 'project', 'd_lidar'), (dict(cam=FAKE + 2), 'project', 'd_cam'),
                           (dict(ws=FAKE + 128), 'project', 'd_workspace'), (dict(ws=FAKE + 16), 'pixels', 'd_workspace'), (dict(ws=FAKE + 64), 'scatter', 'd_workspace'),
                           (dict(image=FAKE + 2), 'scatter', 'd_image'), (dict(pix=FAKE + 1), 'scatter_from_tables', 'd_pixels'),
                           (dict(dep=FAKE + 3), 'scatter_from_tables', 'd_depths'), (dict(image=FAKE + 3), 'stem', 'd_image'), (dict(out=FAKE + 2), 'stem', 'd_out'),
                           (dict(ws=FAKE + 32), 'stem', 'd_workspace'), (dict(params=_stem_params(d_conv2_weight=FAKE + 2)), 'stem', 'd_conv2_weight')):
        _refused(_calls(cfg, only=name, **kw)(), M.E_ALIGN, what + ' must be')
    # a sample without a point needs no pointer: the NULL of the second sample (count 0) is not what refuses this call
    _refused(_calls(cfg, points=(FAKE, None), ws=None, only='project')(), M.E_NULL, 'd_workspace is NULL')
    lib = M.load()
    _refused(lib.ddp_dlss_workspace(None, C.byref(C.c_size_t(0))), M.E_NULL, 'cfg is NULL')
    _refused(lib.ddp_dlss_workspace(C.byref(cfg), None), M.E_NULL, 'bytes is NULL')
    _refused(lib.ddp_dlss_pixels(C.byref(cfg), FAKE, None, C.byref(C.c_void_p(0))), M.E_NULL, 'd_pixels is NULL')
    _refused(lib.ddp_dlss_pixels(C.byref(cfg), FAKE, C.byref(C.c_void_p(0)), None), M.E_NULL, 'd_depths is NULL')
    _refused(lib.ddp_dlss_stem(C.byref(cfg), FAKE, None, FAKE, FAKE, None), M.E_NULL, 'params is NULL')
    # the binding turns a refused configuration into ValueError, anything else into DdpDlssError
    with pytest.raises(ValueError, match='image_h'):
        L.LidarDepth((0, 704))
    with pytest.raises(M.DdpDlssError, match='is NULL') as e:
        M.check(_calls(cfg, ws=None, only='scatter')(), lib)
    assert e.value.code == M.E_NULL


def test_workspace_formula_and_table_places():
    lib = M.load()
    r = lambda n: (n + 255) // 256 * 256
    for name in DC.NAMES:
        c = DC.case(name)
        ld = L.LidarDepth(c['spec']['image'])
        for B, N, pmax in ((c['B'], c['N'], c['pmax']), (3, 5, 1), (1, 1, 0)):
            assert ld.workspace_bytes(B, N, pmax) == DC.workspace_bytes(c, B, N, pmax)
            p, q = C.c_void_p(0), C.c_void_p(0)
            assert lib.ddp_dlss_pixels(C.byref(ld.cfg(B, N, pmax)), FAKE, C.byref(p), C.byref(q)) == 0
            assert p.value == FAKE and q.value == FAKE + r(4 * B * N * pmax)
    # the configuration's size: 6 cameras of 256 x 704, 250 000 points
    ld = L.LidarDepth((256, 704))
    assert ld.workspace_bytes(1, 6, 250000) == 2 * r(4 * 6 * 250000) + 4 * 6 * 256 * 704 + r(4 * 6448) == 16351488
    assert L.stem_size((256, 704)) == (64, 176) and L.stem_size((5, 9)) == (2, 3) and L.stem_size((23, 50)) == (6, 13)


# ---- kernel resources ----------------------------------------------------------------------------------------------------------------
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_no_kernel_touches_scratch(tmp_path):
    out = tmp_path / 'dlss.s'
    src = os.path.join(build.SIDE['dlss'].csrc, 'ddp_dlss.hip')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-x', 'hip', src,
                    '--cuda-device-only', '-S', '-o', str(out)], check=True, capture_output=True, timeout=600)
    figures = {}
    for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', out.read_text(), re.S):
        body = m.group(2)
        short = re.search(r'k_dlss_[a-z]+', m.group(1)).group(0)
        figures[short] = tuple(int(re.search(rf'\.amdhsa_{key} (\d+)', body).group(1))
                               for key in ('private_segment_fixed_size', 'next_free_vgpr', 'group_segment_fixed_size'))
    print('kernel: (scratch B, VGPRs, static LDS B)', figures)
    assert sorted(figures) == sorted(['k_dlss_project', 'k_dlss_clear', 'k_dlss_vote', 'k_dlss_resolve', 'k_dlss_fold', 'k_dlss_stem'])
    for name, (scratch, vgpr, lds) in figures.items():
        assert scratch == 0, f'{name}: {scratch} B of scratch'
        assert vgpr <= 64, f'{name}: {vgpr} registers (eight waves per SIMD need <= 64)'
    assert figures['k_dlss_stem'][2] == 17 * 257 * 4 and all(v[2] == 0 for k, v in figures.items() if k != 'k_dlss_stem')
    # the stem kernel's instruction mix DESIGN §8.4 quotes: the stage-2 weights arrive by scalar loads of 16 dwords (16 per tap: 8 x 32
    # floats), the 256 fma of a tap are 128 packed ones, and the one vector load from global memory is the patch fill
    code = re.search(r'^\S*k_dlss_stem\S*:[^\n]*\n(.*?)s_endpgm', out.read_text(), re.S | re.M).group(1)
    count = lambda pat: len(re.findall(pat, code))
    print('stem kernel:', {k: count(k) for k in ('s_load_dwordx16', 'v_pk_fma_f32', r'v_fma(c)?_f32', 'global_load_', 'ds_read|ds_load')})
    assert count('s_load_dwordx16') >= 16 and count('v_pk_fma_f32') == 128 and count('global_load_') == 1


# ---- plugin surface ------------------------------------------------------------------------------------------------------------------
def _reference_signatures():
    """the parameter names of the reference class: depth_lss.py:16-27 ``__init__``, base.py:211-225 ``BaseDepthTransform.forward``"""
    return (['in_channels', 'out_channels', 'image_size', 'feature_size', 'xbound', 'ybound', 'zbound', 'dbound', 'downsample'],
            ['img', 'points', 'sensor2ego', 'lidar2ego', 'lidar2camera', 'lidar2image', 'cam_intrinsic', 'camera2lidar', 'img_aug_matrix',
             'lidar_aug_matrix', 'metas'])


@pytest.mark.parametrize('name', ['one', 'odd', 'rig'])
def test_plugin_surface_is_the_reference_class(name):
    c = DC.case(name)
    fix = DC.load_fixture(name, GOLDEN)
    assert registry.VTRANSFORMS is registry.MODELS and registry.MODELS.get('DepthLSSTransform') is DepthLSSTransform
    import ddp_amd
    assert ddp_amd.DepthLSSTransform is DepthLSSTransform and 'DepthLSSTransform' in ddp_amd.__all__
    sd = DC.state_dict_of(fix)
    for ds in (1, 2):
        if ds == 2 and c['nx'][2] != 1:
            continue
        m = registry.VTRANSFORMS.build(dict(type='DepthLSSTransform', downsample=ds, **c['kwargs']))
        full = dict(sd, **DC.state_dict_of(fix, 'sd2/')) if ds == 2 else sd
        assert list(m.state_dict()) == list(full)                         # the reference's keys, in its order
        assert all(m.state_dict()[k].shape == v.shape and m.state_dict()[k].dtype == v.dtype for k, v in full.items())
        m.load_state_dict(full, strict=True)
        assert m.D == c['D'] and m.C == c['C'] and [int(v) for v in m.nx] == c['nx']
        assert torch.equal(m.frustum, LC.frustum_f32(c)) and not m.frustum.requires_grad
        keys = list(m.state_dict())
        assert keys[:4] == ['dx', 'bx', 'nx', 'frustum'] and 'dtransform.0.weight' in keys and 'dtransform.7.running_var' in keys
        assert 'depthnet.6.bias' in keys and ('downsample.0.weight' in keys) == (ds == 2)
        assert len(m.dtransform) == 9 and len(m.depthnet) == 7
        assert isinstance(m.downsample, torch.nn.Identity if ds == 1 else torch.nn.Sequential)
        assert not {'pooler', 'lidar_depth'} & set(dict(m.named_modules()))
    init, fwd = _reference_signatures()
    assert list(inspect.signature(DepthLSSTransform.__init__).parameters)[1:] == init
    assert list(inspect.signature(DepthLSSTransform.forward).parameters)[1:12] == fwd
    assert inspect.signature(DepthLSSTransform.forward).parameters['kwargs'].kind is inspect.Parameter.VAR_KEYWORD
    assert 'does NOT modify' in DepthLSSTransform.__doc__


def test_registration_is_a_call_of_its_own():
    assert registry.register_depth_vtransform_into_mmdet3d() == []        # no mmdet3d here: nothing touched, nothing raised
    src = inspect.getsource(registry.register_vtransform_into_mmdet3d)
    assert 'DepthLSSTransform' not in src and 'LSSTransform' in src
    assert "name='DepthLSSTransform'" in inspect.getsource(registry.register_depth_vtransform_into_mmdet3d)


def test_cpu_tensors_and_training_mode_raise_and_points_stay():
    c = DC.case('odd')
    ld = L.LidarDepth(c['spec']['image'])
    args = DC.forward_args(c)
    points = args[1]
    before = [p.clone() for p in points]
    with pytest.raises(ValueError, match='no CPU path'):
        ld.project(points, c['lidar2image'], c['img_aug_matrix'], c['lidar_aug_matrix'])
    with pytest.raises(ValueError, match='no CPU path'):
        ld.scatter_from_tables(torch.zeros(1, 1, 4, dtype=torch.int32), torch.zeros(1, 1, 4))
    with pytest.raises(ValueError, match='no CPU path'):
        ld.stem(torch.zeros(2, 3, 1, 23, 50), DepthLSSTransform(**c['kwargs']).eval().dtransform)
    with pytest.raises(RuntimeError, match='no tables'):
        ld.scatter()
    with pytest.raises(RuntimeError, match='no tables'):
        ld.tables()
    with pytest.raises(ValueError, match='non-empty list'):
        ld.project([], c['lidar2image'], c['img_aug_matrix'], c['lidar_aug_matrix'])
    m = DepthLSSTransform(**c['kwargs'])
    assert m.training
    with pytest.raises(RuntimeError, match='inference only'):
        m(*args)
    m.eval()
    with pytest.raises(ValueError, match='no CPU path'):
        m(*args)
    # the host part of the call path - the matrix tables - reads the points' batch size only; the points are what they were
    lidar, cam = L.pack_lidar(c['lidar2image'], c['img_aug_matrix'], c['lidar_aug_matrix'])
    assert lidar.shape == (2, 12) and cam.shape == (2, 3, 24) and lidar.dtype == cam.dtype == torch.float32
    assert torch.equal(lidar[1, :9].view(3, 3), torch.inverse(c['lidar_aug_matrix'][1, :3, :3])) and torch.equal(lidar[1, 9:], c['lidar_aug_matrix'][1, :3, 3])
    assert torch.equal(cam[0, 2, :9].view(3, 3), c['lidar2image'][0, 2, :3, :3]) and torch.equal(cam[0, 2, 9:12], c['lidar2image'][0, 2, :3, 3])
    assert torch.equal(cam[1, 1, 12:21].view(3, 3), c['img_aug_matrix'][1, 1, :3, :3]) and torch.equal(cam[1, 1, 21:], c['img_aug_matrix'][1, 1, :3, 3])
    assert all(torch.equal(p, q) for p, q in zip(points, before)) and all(torch.equal(p, q) for p, q in zip(points, c['points']))
