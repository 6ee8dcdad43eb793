"""CPU references, input grids and the ctypes binding of the probe library for the device-math tests
(tests/test_device_math_host.py, tests/test_device_math_gpu.py; probe source: tests/probe/device_math_probe.hip).

The references never call the code under test: gelu_exact is fp64 erf, gelu_as_ref_f32 restates Abramowitz-Stegun 7.1.26 with the
UNFOLDED constants of csrc/gemm_f32.h in numpy float32 (the yardstick for what an fp32 evaluation of that formula can reach),
cpu_split is the exact 3-way bf16 truncation split in integer / float32 numpy."""
import ctypes as C
import functools
import os

import numpy as np

F32 = np.float32
TINY = 2.0 ** -100          # below this the pieces of a split are subnormal: the bars get an absolute 2^-126 there
ABS_FLOOR = 2.0 ** -126


# ---------------------------------------------------------------------------------------------------------------- references
def gelu_exact(x):
    """0.5 x (1 + erf(x / sqrt 2)) in fp64 (x: any float array; NaN / inf propagate as IEEE arithmetic has it)"""
    import torch
    xd = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return 0.5 * xd * (1.0 + torch.erf(torch.from_numpy(xd / np.sqrt(2.0))).numpy())


def _fma32(a, b, c):
    """fl32(a b + c) with one rounding: the product of two fp32 is exact in fp64 (48 bits); the fp64 sum rounds at 53 bits before
    the fp32 rounding, a double rounding that moves the result in ~2^-29 of the cases by one fp32 ulp"""
    return (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(F32)


def gelu_as_ref_f32(x):
    """gelu_fast of csrc/gemm_f32.h op by op in numpy float32 (unfolded constants; exp2 and the reciprocal correctly rounded)"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        z = np.abs(x) * F32(0.70710678118654752440)
        t = F32(1.0) / _fma32(np.full_like(z, F32(0.3275911)), z, F32(1.0))
        p = _fma32(np.full_like(t, F32(1.061405429)), t, F32(-1.453152027))
        p = _fma32(p, t, F32(1.421413741))
        p = _fma32(p, t, F32(-0.284496736))
        p = _fma32(p, t, F32(0.254829592))
        p = p * t
        e = np.exp2(F32(-1.44269504088896340736) * z * z).astype(F32)
        erf_abs = (F32(1.0) - (p.astype(np.float64) * e.astype(np.float64))).astype(F32)      # fmaf(-p, e, 1)
        h = F32(0.5) * x
        s = np.copysign(erf_abs, x)
        return (s.astype(np.float64) * h.astype(np.float64) + h.astype(np.float64)).astype(F32)


def sigmoid_exact(x):
    xd = np.asarray(x, dtype=np.float64)
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-xd))


def cpu_split(x):
    """exact 3-way truncation split of fp32 into bf16-representable pieces: x & 0xFFFF0000, subtract, repeat.
    -> (p1, p2, p3) float32 (numpy keeps subnormals: nothing is flushed here)"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid='ignore', over='ignore'):
        h = (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)
        r = x - h
        m = (r.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)
        return h, m, r - m


def pieces_to_f32(p1, p2, p3, n=None):
    """unpack the 0x07060302 packing (word u = bf16 of element 2u in the low half, of element 2u + 1 in the high half) of
    three word arrays -> three fp32 arrays of n elements"""
    out = []
    for p in (p1, p2, p3):
        p = np.asarray(p, dtype=np.uint32)
        e = np.empty(2 * p.size, dtype=np.uint32)
        e[0::2] = p << np.uint32(16)
        e[1::2] = p & np.uint32(0xFFFF0000)
        out.append(e[:n].view(F32))
    return tuple(out)


def sum3_f32(p1, p2, p3):
    """fl(fl(p1 + p2) + p3) in float32"""
    with np.errstate(invalid='ignore', over='ignore'):
        return (p1 + p2) + p3


def sum3_f64(p1, p2, p3):
    with np.errstate(invalid='ignore', over='ignore'):
        return p1.astype(np.float64) + p2.astype(np.float64) + p3.astype(np.float64)


# --------------------------------------------------------------------------------------------------------------------- grids
@functools.lru_cache(maxsize=None)
def dense():
    """[-12, 12] in steps of 1e-5 (2 400 001 points, sorted)"""
    g = (np.arange(-1200000, 1200001, dtype=np.float64) * 1e-5).astype(F32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def expo():
    """+- m 2^e for e in [-126, 127], 64 seeded mantissas m in [1, 2) each"""
    rng = np.random.default_rng(20240607)
    e = np.repeat(np.arange(-126, 128), 64)
    m = 1.0 + rng.integers(0, 1 << 23, size=e.size).astype(np.float64) / (1 << 23)
    v = np.ldexp(m, e).astype(F32)
    g = np.concatenate([v, -v])
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def special():
    """+-0, +-inf, NaN, +-FLT_MAX, +-FLT_MIN, subnormals, every pattern in [0.5, 2) that ends in 16 zero bits and every pattern
    within 2^16 patterns of 1.0 that ends in 8 zero bits (pieces that come out zero), 1 - 2^-24, 1 + 2^-23 - each with both signs"""
    pos = [0x00000000, 0x7F800000, 0x7F7FFFFF, 0x00800000,                       # 0, inf, FLT_MAX, FLT_MIN
           0x00000001, 0x00000002, 0x000000FF, 0x00000100, 0x0000FFFF, 0x00010000, 0x00010001, 0x00400000, 0x007FFFFF,
           0x3F7FFFFF, 0x3F800001]                                               # 1 - 2^-24, 1 + 2^-23
    pos += list(range(0x3F000000, 0x40000000 + 1, 0x10000))
    pos += list(range(0x3F800000 - 0x10000, 0x3F800000 + 0x10000 + 1, 0x100))
    pos = np.array(pos, dtype=np.uint32)
    bits = np.concatenate([pos, pos | np.uint32(0x80000000), np.array([0x7FC00000], dtype=np.uint32)])
    g = bits.view(F32).copy()
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def bits():
    """2^20 seeded finite fp32 bit patterns (the exponent field 255 is redrawn as 254)"""
    rng = np.random.default_rng(977)
    b = rng.integers(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)
    nonfinite = (b & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
    b[nonfinite] &= np.uint32(0xFF7FFFFF)
    g = b.view(F32).copy()
    g.setflags(write=False)
    return g


def e_ref(x, exact=None, ref=None):
    """max |gelu_as_ref_f32 - gelu_exact| / |x| over the finite points with |x| >= 2^-100"""
    x = np.asarray(x, dtype=F32)
    ok = np.isfinite(x) & (np.abs(x) >= TINY)
    xs = x[ok]
    ex = gelu_exact(xs) if exact is None else exact[ok]
    rf = gelu_as_ref_f32(xs) if ref is None else ref[ok]
    return float(np.max(np.abs(rf.astype(np.float64) - ex) / np.abs(xs.astype(np.float64))))


# ----------------------------------------------------------------------------------------------------------- the probe library
PROBE_ONE_OUT = ('probe_gelu_fast', 'probe_sigmoid')
PROBE_THREE_OUT = ('probe_gelu_ops', 'probe_gelu_sched', 'probe_gelu_packed', 'probe_split8', 'probe_split8_packed', 'probe_split_ops')
PROBE_EXPORTS = PROBE_ONE_OUT + PROBE_THREE_OUT
PROBE_PACKED = ('probe_gelu_packed', 'probe_split8', 'probe_split8_packed', 'probe_split_ops')


def load_probe(path=None):
    """the probe library built by ddp_amd.build.build(); raises (a failure, not a skip) when it is missing or stale"""
    from ddp_amd import build
    if path is None:
        path = build.PROBE_LIB_PATH
        if not os.path.exists(path):
            raise RuntimeError(f'{path} not found: ddp_amd.build.build() makes it')
        if build.probe_built_hash() != build.probe_hash():
            raise RuntimeError(f'{path} is stale: built from {build.probe_built_hash() or "<no stamp>"}, the tree holds {build.probe_hash()}')
    lib = C.CDLL(path)
    for n in PROBE_ONE_OUT:
        getattr(lib, n).argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        getattr(lib, n).restype = C.c_int
    for n in PROBE_THREE_OUT:
        getattr(lib, n).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        getattr(lib, n).restype = C.c_int
    return lib


def run_probe(lib, name, x, dev):
    """one launch of probe ``name`` on the fp32 array x -> numpy outputs (one float32 array, or three uint32 arrays: per element
    for the ops / sched probes, per element PAIR for the packed ones).  Outputs are pre-filled with 0xCDCDCDCD and carry 64 guard
    words each, which must come back untouched."""
    import torch
    x = np.ascontiguousarray(x, dtype=F32)
    n = x.size
    d_in = torch.from_numpy(x.copy()).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    fn = getattr(lib, name)
    n_out = (n + 1) // 2 if name in PROBE_PACKED else n
    guard = 64
    fill = np.int32(np.uint32(0xCDCDCDCD).view(np.int32))
    outs = [torch.full((n_out + guard,), int(fill), dtype=torch.int32, device=dev) for _ in range(1 if name in PROBE_ONE_OUT else 3)]
    rc = fn(d_in.data_ptr(), *[o.data_ptr() for o in outs], n, stream)
    assert rc == 0, f'{name}: launch status {rc}'
    torch.cuda.synchronize(dev)
    res = []
    for o in outs:
        a = o.cpu().numpy().view(np.uint32)
        assert np.all(a[n_out:] == np.uint32(0xCDCDCDCD)), f'{name} wrote past its {n_out} output words'
        res.append(a[:n_out])
    if name in PROBE_ONE_OUT:
        return res[0].view(F32)
    return tuple(res)
