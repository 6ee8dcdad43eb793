"""The caller-visible tail of the sampler workspaces: ``ddp_amd.engine.caller_regions`` - the one host-side table - against the library's
own queries, over every case of tests/config_space_cases.py x both GEMM engines x every fused / unfused flag set of ``make_cfg`` x every
combination of the five tail flags (and DDP_FLAG_RECORD_X0 / DDP_FLAG_FORCE_X0) that ``validate`` accepts, and over the FCN loop.
Host only: the workspace queries and ddp_x0_trace run without a device.  (What the table must SAY is pinned by the independent
derivations of test_step_record_host.py, test_seeded_noise_host.py, test_x0_hints_host.py, test_prior_start_host.py and
test_class_prior_host.py; GPU companion: tests/test_workspace_regions_gpu.py.)"""
import ctypes as C
import itertools

import config_space_cases as S
from ddp_amd import _lib
from ddp_amd.engine import caller_regions, class_prior_places, prior_start_places, step_record_sizes
from support import lib, round256  # noqa: F401

TAIL = (_lib.FLAG_CLASS_PRIOR, _lib.FLAG_PRIOR_START, _lib.FLAG_X0_HINTS, _lib.FLAG_SEEDED_NOISE, _lib.FLAG_STEP_RECORD)
TAIL_MASK = sum(TAIL)
X0_BITS = _lib.FLAG_RECORD_X0 | _lib.FLAG_FORCE_X0
EXTRAS = [sum(f for f, on in zip(TAIL + (_lib.FLAG_RECORD_X0, _lib.FLAG_FORCE_X0), bits) if on)
          for bits in itertools.product((0, 1), repeat=7)]
# the buffers of each flag, in workspace order (include/ddp_mi355x.h, the list at ddp_query_workspace)
NAMES = {_lib.FLAG_CLASS_PRIOR: ('cprior_rows', 'cprior_table'), _lib.FLAG_PRIOR_START: ('prior_start', 'prior_map'),
         _lib.FLAG_X0_HINTS: ('hint_rows', 'hint_map'), _lib.FLAG_SEEDED_NOISE: ('seed_noise',),
         _lib.FLAG_STEP_RECORD: ('step_rec', 'step_map')}
FAKE_BASE = 1 << 40             # 256-aligned, never dereferenced: ddp_x0_trace only carves
FCN_HEADS = ((0, 1), (2, 1), (1, 2))            # (num_convs, dilation)


def expected_names(flags):
    names = [n for f in TAIL if flags & f for n in NAMES[f]]
    if flags & _lib.FLAG_SEEDED_NOISE and 'prior_start' in names:
        names.remove('prior_start')         # the seeded-noise buffer is the start map
    return names


def assert_tiles(regions, begin, end, what):
    """contiguous 256-aligned regions from ``begin`` to ``end``, each as long as its rounded size"""
    at = begin
    for name, (off, nbytes) in regions.items():
        assert off == at and off % 256 == 0 and nbytes > 0, (what, name, off, at)
        at = off + round256(nbytes)
    assert at == end, (what, at, end)


def _cfgs():
    """every cfg of the grid with its flags still at the fused / unfused set: (case name, case, cfg)"""
    for name, c in S.CASES.items():
        for gemm in ('bf16x3', 'f32'):
            for fl, fp, ft, nh in itertools.product((True, False), repeat=4):
                yield name, c, S.make_cfg(c, gemm, fl, fp, ft, nh)


def test_regions_tile_the_end_of_the_workspace_and_hold_the_record_where_the_library_says(lib):
    seen = refused = 0
    p = C.c_void_p()
    for name, c, cfg in _cfgs():
        base_flags = cfg.flags
        base_total = S.query(lib, cfg)[1]
        x0_total = {}                        # flag-clear totals with RECORD_X0 / FORCE_X0 set (seg)
        for extra in EXTRAS:
            cfg.flags = base_flags | extra
            rc, total, _ = S.query(lib, cfg)
            if rc != 0:
                refused += 1
                continue
            seen += 1
            what = (name, cfg.gemm_mode, hex(cfg.flags))
            regions = caller_regions(cfg, total)
            assert list(regions) == expected_names(extra), what
            # the first region begins where the workspace of the cfg without the five flags ends.  seg with DDP_FLAG_STEP_RECORD: the
            # x0 trace lies inside the record, so the bits that carve a trace of their own are cleared on that side
            # (tests/test_step_record_host.py::test_record_x0_and_step_record_share_one_buffer)
            x0 = extra & X0_BITS if not extra & _lib.FLAG_STEP_RECORD else 0
            if x0 not in x0_total:
                cfg.flags = base_flags | x0
                x0_total[x0] = S.query(lib, cfg)[1] if x0 else base_total
                cfg.flags = base_flags | extra
            assert_tiles(regions, x0_total[x0], total, what)
            if extra & _lib.FLAG_STEP_RECORD:
                assert lib.ddp_x0_trace(C.byref(cfg), FAKE_BASE, C.byref(p)) == 0, lib.ddp_last_error()
                assert regions['step_rec'][0] == p.value - FAKE_BASE, what
            # the functions the engines and the other host tests use are lookups into the table
            if extra & _lib.FLAG_PRIOR_START:
                start = 'seed_noise' if extra & _lib.FLAG_SEEDED_NOISE else 'prior_start'
                assert prior_start_places(cfg, total) == regions['prior_map'] + regions[start], what
            if extra & _lib.FLAG_CLASS_PRIOR:
                assert class_prior_places(cfg, total) == regions['cprior_table'] + regions['cprior_rows'], what
            if extra & _lib.FLAG_STEP_RECORD:
                assert step_record_sizes(cfg) == (regions['step_rec'][1], regions['step_map'][1]), what
    print(f'{seen} configurations checked, {refused} flag combinations refused by validate')
    assert seen > 60000 and refused > 0


def test_fcn_loop_ends_with_the_seeded_noise_and_step_record_groups(lib):
    """ddp_sample_fcn's workspace: the table on ITS byte count; the record at ddp_sample_fcn_workspace - round256(map) - round256(record)
    with the header's two formulas written out here"""
    n = C.c_size_t(0)

    def fcn_bytes(cfg, nc, dil):
        assert lib.ddp_sample_fcn_workspace(C.byref(cfg), nc, dil, C.byref(n)) == 0, lib.ddp_last_error()
        return n.value
    seen = 0
    for name, c in S.CASES.items():
        if c['task'] != 'seg':
            continue
        for nc, dil in FCN_HEADS:
            cfg = S.make_cfg(c)
            base = fcn_bytes(cfg, nc, dil)
            for extra in (_lib.FLAG_STEP_RECORD, _lib.FLAG_SEEDED_NOISE, _lib.FLAG_STEP_RECORD | _lib.FLAG_SEEDED_NOISE,
                          _lib.FLAG_STEP_RECORD | _lib.FLAG_FCN_PREPARED):
                cfg.flags = extra
                total = fcn_bytes(cfg, nc, dil)
                regions = caller_regions(cfg, total)
                assert list(regions) == expected_names(extra), (name, nc, extra)
                assert_tiles(regions, base, total, (name, nc, extra))
                if extra & _lib.FLAG_STEP_RECORD:
                    pixels = cfg.batch * cfg.head_h * cfg.head_w
                    rec, smap = cfg.timesteps * cfg.randsteps * pixels, pixels * 4
                    assert regions['step_rec'] == (total - round256(smap) - round256(rec), rec)
                    assert step_record_sizes(cfg) == (rec, smap)
                seen += 1
    assert seen >= 4 * len(FCN_HEADS) * 10


def test_a_flag_clear_cfg_has_no_regions(lib):
    cfg = S.make_cfg(S.CASES['seg_L12'])
    assert caller_regions(cfg, S.query(lib, cfg)[1]) == {}
