"""The elementwise __device__ functions of csrc/ on their own, against fp64 / exact integer references
(probe: tests/probe/device_math_probe.hip -> ddp_amd/lib/libddp_probe.so, references and grids: tests/device_math_util.py).

The sampler tests compare whole K-step calls with the oracle at 2e-4; an error of a few 1e-6 in the FFN activation or a wrong
piece of a bf16 split fits under that bar.  Here every function runs alone, one or two launches of at most 2.4 M elements per
test, and each test prints its worst figure on a line that starts with DEVICE-MATH.

Figures measured on an MI355X are quoted in the docstrings and in CHANGELOG.md."""
import numpy as np
import pytest
import torch

import device_math_util as U
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

GELU_ROUTES = ('fast', 'ops', 'sched', 'packed')
SPLIT_ROUTES = ('split8', 'split8_packed', 'split_ops')
ULP = 2.0 ** -23


@pytest.fixture(scope='module')
def probe():
    return U.load_probe()          # missing or stale: an error, never a skip


@pytest.fixture(scope='module')
def gelu_points():
    """dense + expo + special in one array, with the fp64 and the numpy-float32 reference computed once"""
    x = np.concatenate([U.dense(), U.expo(), U.special()])
    x.setflags(write=False)
    sl = {'dense': slice(0, U.dense().size), 'expo': slice(U.dense().size, U.dense().size + U.expo().size),
          'special': slice(U.dense().size + U.expo().size, x.size)}
    exact = U.gelu_exact(x)
    ref = U.gelu_as_ref_f32(x)
    return x, sl, exact, ref


def _gelu_run(probe, dev, route, x):
    """-> (g, pieces): g = the fp32 GELU value of the route (for the split routes fl(fl(p1 + p2) + p3)), pieces = three uint32
    arrays of the pieces' bit patterns (None for 'fast')"""
    if route == 'fast':
        return U.run_probe(probe, 'probe_gelu_fast', x, dev), None
    w = U.run_probe(probe, 'probe_gelu_' + route, x, dev)
    if route == 'packed':
        w = tuple(q.view(np.uint32) for q in U.pieces_to_f32(*w, n=x.size))
    return U.sum3_f32(*(q.view(np.float32) for q in w)), w


_GELU = {}


def _gelu(probe, dev, route, x):
    """_gelu_run on the module's shared points: one launch per route per module"""
    if route not in _GELU:
        _GELU[route] = _gelu_run(probe, dev, route, x)
    return _GELU[route]


@pytest.mark.parametrize('grid', ['dense', 'expo'])
@pytest.mark.parametrize('route', GELU_ROUTES)
def test_gelu_accuracy(probe, dev, gelu_points, route, grid):
    """|g - gelu_exact(x)| <= 2 E_ref |x| (+ 2^-126 below |x| = 2^-100), E_ref = the error per |x| of the SAME formula (A&S 7.1.26,
    unfolded constants of gemm_f32.h) in numpy float32 on the same points; factor 2: v_rcp_f32 and v_exp_f32 are 1-ulp
    approximations where numpy is correctly rounded.

    MI355X: every route 2.74e-7 on dense (at x = 0.066) and 2.32e-7 on expo - equal to E_ref itself, half the bar.  With the
    coefficient 0.27274550239055780 that layer_bf16x3.h held before, ops / sched / packed reach 3.15e-6 (dense, x = 0.628) and
    3.08e-6 (expo): 5.76 and 6.65 times the bar, while fast stays at 0.50."""
    x, sl, exact, ref = gelu_points
    g, _ = _gelu(probe, dev, route, x)
    xs, gs, ex, rf = x[sl[grid]], g[sl[grid]], exact[sl[grid]], ref[sl[grid]]
    e_ref = U.e_ref(xs, ex, rf)
    ax = np.abs(xs.astype(np.float64))
    nz = ax > 0
    err = np.abs(gs.astype(np.float64) - ex)
    bar = 2 * e_ref * ax + np.where(ax < U.TINY, U.ABS_FLOOR, 0.0)
    big = nz & (ax >= U.TINY)
    ratio = err[big] / ax[big]
    i = int(np.argmax(ratio))
    print(f'DEVICE-MATH gelu {route} {grid}: max |err|/|x| = {ratio[i]:.3e} at x = {xs[big][i]:.6g} (E_ref {e_ref:.3e}, bar {2 * e_ref:.3e}, '
          f'ratio to bar {ratio[i] / (2 * e_ref):.2f}); max |err| = {err[nz].max():.3e}; below 2^-100: max |err| = '
          f'{(err[nz & ~big].max() if np.any(nz & ~big) else 0.0):.3e}')
    assert np.all(np.isfinite(gs[nz]))
    assert np.all(err[nz] <= bar[nz])


def test_gelu_routes_agree(probe, dev, gelu_points):
    """ops and sched run the same instructions, only interleaved: bit-identical pieces.  packed is the same formula on the packed
    fp32 path: within 2 ulp of ops' by its arithmetic - and measured bit-identical to it on an MI355X (0.00 ulp over 2 430 730
    points), so that is what is asserted."""
    x, sl, _, _ = gelu_points
    g_ops, w_ops = _gelu(probe, dev, 'ops', x)
    g_sch, w_sch = _gelu(probe, dev, 'sched', x)
    g_pk, w_pk = _gelu(probe, dev, 'packed', x)
    for a, b in zip(w_ops, w_sch):
        assert np.array_equal(a, b)
    fin = np.isfinite(x) & (np.abs(x) >= U.TINY)
    d = np.abs(g_pk[fin].astype(np.float64) - g_ops[fin].astype(np.float64))
    # the fp32 ulp of the result in fp64 (np.spacing in fp32 overflows at FLT_MAX): 2^(e - 24) with |g| = m 2^e, 0.5 <= m < 1
    # (e = -125 at and below FLT_MIN, zero included: the subnormal spacing 2^-149)
    ag = np.abs(g_ops[fin]).astype(np.float64)
    ulp = np.ldexp(1.0, np.where(ag > 0, np.maximum(np.frexp(ag)[1], -125), -125) - 24)
    worst = float(np.max(d / ulp))
    same = all(np.array_equal(a[fin], b[fin]) for a, b in zip(w_ops, w_pk))
    print(f'DEVICE-MATH gelu packed vs ops: max difference {worst:.2f} ulp of the result over {int(fin.sum())} points; '
          f'pieces bit-identical: {same}; ops vs sched: bit-identical')
    assert worst <= 2.0 and same
    small = np.isfinite(x) & ~fin
    assert np.all(np.abs(g_pk[small].astype(np.float64) - g_ops[small].astype(np.float64)) <= U.ABS_FLOOR)


@pytest.mark.parametrize('route', GELU_ROUTES)
def test_gelu_specials(probe, dev, route):
    """+-0 -> a zero; +inf -> +inf; NaN -> NaN; -inf as torch.nn.functional.gelu (NaN-ness); |x| >= 13 -> exactly x on the
    positive side and a zero of either sign on the negative side"""
    big = np.concatenate([np.arange(13, 64, 0.25), 13 * 2.0 ** np.arange(0, 124, dtype=np.float64), [np.finfo(np.float32).max]])
    x = np.concatenate([[0.0, -0.0, np.inf, np.nan, -np.inf], big, -big]).astype(np.float32)
    g, w = _gelu_run(probe, dev, route, x)
    assert g[0] == 0 and g[1] == 0
    # the piece routes hand back the split of the value, and +inf splits into (+inf, NaN, NaN): its first piece is the witness
    # (a NaN value would give a NaN first piece)
    at_inf = g[2] if w is None else w[0].view(np.float32)[2]
    assert at_inf == np.inf and np.isnan(g[3])
    t = torch.nn.functional.gelu(torch.tensor([-np.inf], dtype=torch.float32))
    assert bool(np.isnan(g[4])) == bool(torch.isnan(t)[0]), (g[4], t)
    nb = big.size
    pos, neg = g[5:5 + nb], g[5 + nb:]
    print(f'DEVICE-MATH gelu {route} specials: gelu(-inf) = {g[4]}, {nb} points with |x| >= 13: '
          f'{int(np.sum(pos != x[5:5 + nb]))} positive results differ from x, {int(np.sum(neg != 0))} negative results are not zero')
    assert np.array_equal(pos, x[5:5 + nb])
    assert np.all(neg == 0)


@pytest.mark.parametrize('route', ['ops', 'sched', 'packed'])
def test_gelu_pieces(probe, dev, gelu_points, route):
    """the three pieces the FFN feeds to fc2: low 16 bits clear, their sum is an fp32 number g (p1 + p2 + p3 exact in fp64 ==
    fl(fl(p1 + p2) + p3)), and the CPU split of that g gives the same pieces bit for bit (finite |x| >= 2^-100: every piece is
    normal or zero there)."""
    x, sl, _, _ = gelu_points
    g, w = _gelu(probe, dev, route, x)
    ok = np.isfinite(x) & (np.abs(x) >= U.TINY)
    for p in w:
        assert not np.any(p[ok] & np.uint32(0xFFFF))
    pf = [p.view(np.float32)[ok] for p in w]
    assert np.array_equal(U.sum3_f64(*pf), g[ok].astype(np.float64))
    want = U.cpu_split(g[ok])
    # (a zero piece may carry either sign: g = -0 splits into -0, +0, +0 and sums back to +0)
    bad = sum(int(np.sum((a.view(np.uint32) != b.view(np.uint32)) & ~((a == 0) & (b == 0)))) for a, b in zip(want, pf))
    nz = [int(np.sum(p == 0)) for p in pf]
    print(f'DEVICE-MATH gelu {route} pieces: {int(ok.sum())} points, {bad} pieces differ from the CPU split of their own sum; '
          f'zero pieces p1/p2/p3: {nz[0]}/{nz[1]}/{nz[2]}')
    assert bad == 0


@pytest.fixture(scope='module')
def split_points():
    x = np.concatenate([U.bits(), U.special()])
    x.setflags(write=False)
    return x


def test_splits(probe, dev, split_points):
    """split8 (gemm_bf16x3.h), split8_packed and the 44-op split_op list handed out by SPLIT_HAND_LO (layer_bf16x3.h) on 2^20
    seeded bit patterns + the specials.  Finite |x| >= 2^-100: p1 + p2 + p3 == x exactly (fp64), and the three routes are
    bit-identical to each other and to the CPU split (x & 0xFFFF0000, subtract, repeat).  Smaller |x|: |x - sum| <= 2^-126
    (whether the device flushed is printed).  inf / NaN: the launch completes."""
    x = split_points
    fin = np.isfinite(x)
    ok = fin & (np.abs(x) >= U.TINY)
    small = fin & ~ok
    want = U.cpu_split(x)
    got = {}
    for r in SPLIT_ROUTES:
        w = U.run_probe(probe, 'probe_' + r, x, dev)
        got[r] = U.pieces_to_f32(*w, n=x.size)
    for r in SPLIT_ROUTES:
        p = got[r]
        s = U.sum3_f64(*(q[ok] for q in p))
        n_bad_sum = int(np.sum(s != x[ok].astype(np.float64)))
        n_bad_bits = sum(int(np.sum(a[ok].view(np.uint32) != b[ok].view(np.uint32))) for a, b in zip(want, p))
        d_small = np.abs(x[small].astype(np.float64) - U.sum3_f64(*(q[small] for q in p)))
        flushed = sum(int(np.sum(a[small].view(np.uint32) != b[small].view(np.uint32))) for a, b in zip(want, p))
        print(f'DEVICE-MATH {r}: {int(ok.sum())} points |x| >= 2^-100: {n_bad_sum} inexact sums, {n_bad_bits} pieces differ from the CPU '
              f'split; {int(small.sum())} smaller points: max |x - sum| = {d_small.max():.3e}, {flushed} pieces differ from the '
              f'unflushed CPU split ({"the device flushed" if flushed else "nothing flushed"})')
        assert n_bad_sum == 0 and n_bad_bits == 0
        assert np.all(d_small <= U.ABS_FLOOR)
    for r in SPLIT_ROUTES[1:]:
        for a, b in zip(got[SPLIT_ROUTES[0]], got[r]):
            assert np.array_equal(a[ok].view(np.uint32), b[ok].view(np.uint32))


def test_sigmoid(probe, dev):
    """sigmoidf_ (ddp_internal.h) vs fp64 on dense x 8 (+-96), expo and special.  Relative error <= 4 x 2^-23 (budget: expf <= 1 ulp,
    one rounded add, one correctly rounded divide = 2 ulp; the bar is twice the budget) wherever the fp64 result is a NORMAL fp32
    number (>= 2^-126, x >= -87.34).  Below that fp32 has no relative precision to offer (subnormal spacing 2^-149, and expf(-x)
    overflows from x = -88.73 on, so the function returns 0 for a true value of up to 2.9e-39): there the bar is the absolute
    2^-126 that the other tests of this file use for subnormal results.  Exact 0 / 1 at -inf / +inf, 0.5 at +-0, NaN at NaN, and
    monotone non-decreasing on the sorted dense grid (k_bev_update and the bev step record threshold this value)."""
    d8 = (U.dense().astype(np.float64) * 8).astype(np.float32)
    x = np.concatenate([d8, U.expo(), U.special()])
    s = U.run_probe(probe, 'probe_sigmoid', x, dev)
    fin = np.isfinite(x)
    ref = U.sigmoid_exact(x[fin])
    err = np.abs(s[fin].astype(np.float64) - ref)
    normal = ref >= U.ABS_FLOOR
    rel = err[normal] / ref[normal]
    i = int(np.argmax(rel))
    sub = err[~normal].max() if np.any(~normal) else 0.0
    steps_down = int(np.sum(np.diff(s[:d8.size]) < 0))
    print(f'DEVICE-MATH sigmoid: max relative error {rel[i] / ULP:.3f} x 2^-23 at x = {x[fin][normal][i]:.6g} over {int(normal.sum())} points '
          f'(bar 4 x 2^-23); results below 2^-126: max |err| = {sub:.3e} (bar 2^-126 = {U.ABS_FLOOR:.3e}); '
          f'{steps_down} decreasing steps on the sorted grid')
    assert np.all(rel <= 4 * ULP)
    assert sub <= U.ABS_FLOOR
    assert np.all((s[fin] >= 0) & (s[fin] <= 1))
    xs = x[~fin]
    for v, want in ((np.inf, 1.0), (-np.inf, 0.0)):
        assert np.all(s[~fin][xs == v] == want) and np.any(xs == v)
    assert np.all(np.isnan(s[~fin][np.isnan(xs)])) and np.any(np.isnan(xs))
    assert np.all(s[x == 0] == 0.5) and int(np.sum(x == 0)) >= 2
    assert steps_down == 0
