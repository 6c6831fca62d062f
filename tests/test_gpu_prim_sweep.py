"""The numeric primitives on the device over every float32 input (MI355X; DESIGN.md §Numerics, "The primitives over
every input"): rt_debug_math's sweep (op 16) generates the inputs on the device from (start pattern, odd multiplier,
mask), and prim_ref.compare evaluates the oracle at the same inputs, bit for bit (or both NaN), in chunks of at most
2^26 results.  One chunk's worth of host memory (256 MiB) is live at a time; a test that holds two ops' results side
by side takes them in half chunks.

The exponents of pow_nonneg (op 11) and pow_nonneg_wave (op 13) are the ones the shaders pass (prim_ref.EXPONENTS):
  np_expo = 0.68f + 0.1f   rt_runtime.cpp (consts_np_octaves) -> density_nomadplains' steep noise, rt_shader.h:383,
                           :419 and :578 (pow_nonneg_wave)
  1.5                      the lift of the nomadplains base, rt_shader.h:391, :423, :584 (pow_nonneg_wave), and the
                           Mie phase's denominator in the sky, rt_shader.h:984 (pow_nonneg)
  0.35, 0.15               density_factor (rt_runtime.cpp: 0.15 when recording), the march's step factor,
                           rt_shader.h:823 (pow_nonneg_wave)
  0.33                     the octave count np_octaves_exact, rt_shader.h:290, and the colour's detail level,
                           rt_shader.h:1035 (pow_nonneg)
  40                       the specular term, rt_shader.h:1075 and rt_kernels.hip shade_finish (pow_nonneg)
log2_nonneg (op 17) is the shading's mip level, rt_shader.h:1005.  The general pow (op 8) serves the host's constants
only (rt_runtime.cpp: pow(1.96f, n), pow(2.03f, n)); it, max and min take every ordered pair of prim_ref.edge_values().

Left out of a sweep over x >= 0: the 2^23 non-finite patterns 0x7f800000 .. 0x7fffffff, and nothing else (asserted).
Each test prints its wall time; DESIGN.md records them."""
import time

import numpy as np
import pytest

import oracle_lib as O
import prim_ref as P

pytestmark = pytest.mark.gpu

CHUNK = 1 << 26
HALF = CHUNK // 2
MIX = 0x9e3779b1
NONFINITE_NONNEG = 1 << 23


@pytest.fixture(scope="module")
def dev():
    import gpgpuraytrace_amd as G
    d = G.DeviceFactory.construct(G.DeviceAPI.HIP, 8, 8)
    assert d is not None, G.lib().rt_last_error()
    yield d
    d.destroy()


def device_sweep(dev, elem, start, n, mult=1, mask=P.FULL, y=0.0, out=None):
    """rt_debug_math op 16: the element op at the n inputs (start + i * mult) & mask, as uint32 bit patterns."""
    import gpgpuraytrace_amd as G
    assert isinstance(n, int) and 0 < n <= CHUNK
    words = np.array([start & P.FULL, mult & P.FULL, elem, mask], np.uint32)
    b = np.array([y], np.float32)
    out = np.empty(n, np.uint32) if out is None else out[:n]
    rc = G.lib().rt_debug_math(dev._h, P.SWEEP, words.ctypes.data, b.ctypes.data, out.ctypes.data, n)
    assert rc == 0, G.lib().rt_last_error()
    return out


def chunks(count, size):
    for off in range(0, count, size):
        yield off, min(size, count - off)


def sweep_vs_oracle(dev, elem, first, count, mult=1, mask=P.FULL, y=None, domain=P.ALL, census=False):
    """The element op against the oracle at `count` inputs from `first`: (inputs left out, special waves, ordinary
    waves); fails at the first chunk with a mismatch, naming the op, the inputs and both results."""
    buf = np.empty(min(count, CHUNK), np.uint32)
    left_out = special = ordinary = 0
    for off, n in chunks(count, CHUNK):
        start = (first + off * mult) & P.FULL
        got = device_sweep(dev, elem, start, n, mult, mask, y or 0.0, buf)
        r = P.compare(elem, got, start, mult, mask, y or 0.0, domain, census)
        assert r.mismatches == 0, "device " + P.describe(P.NAMES[elem], r, y)
        left_out += r.excluded
        special += r.waves_special
        ordinary += r.waves_ordinary
    return left_out, special, ordinary


def test_sweep_inputs_and_array_path_agree(dev):
    """The sweep makes the inputs it says: an element op through the sweep equals the same op through the array
    path at inputs made here, for a count that is no multiple of the block; an even multiplier and an element op
    outside 0-8, 11, 13, 17 are rejected."""
    import gpgpuraytrace_amd as G
    n, start = 4096 + 37, 0x3f7ffff0
    for mult, mask in ((1, P.FULL), (MIX, P.NONNEG), (4099, P.FULL)):
        x = ((start + np.arange(n, dtype=np.uint64) * mult) & mask).astype(np.uint32)
        for elem in (P.EXP2, P.RCP, P.LOG2_NONNEG):
            want = np.empty(n, np.uint32)
            assert G.lib().rt_debug_math(dev._h, elem, x.ctypes.data, None, want.ctypes.data, n) == 0
            got = device_sweep(dev, elem, start, n, mult, mask)
            both_nan = ((got & P.NONNEG) > P.INF_BITS) & ((want & P.NONNEG) > P.INF_BITS)
            assert np.all((got == want) | both_nan), (mult, elem)
    out = np.zeros(64, np.uint32)
    one = np.ones(1, np.float32)
    for words in ([0, 2, P.EXP2, P.FULL], [0, 1, 9, P.FULL], [0, 1, 12, P.FULL], [0, 1, 16, P.FULL], [0, 1, 18, P.FULL]):
        w = np.array(words, np.uint32)
        assert G.lib().rt_debug_math(dev._h, P.SWEEP, w.ctypes.data, one.ctypes.data, out.ctypes.data, 64) < 0
    dev.check()


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("op", range(8), ids=[P.NAMES[i] for i in range(8)])
def test_unary_every_pattern(dev, op, half):
    """Ops 0-7 at every one of the 2^32 patterns, NaNs and infinities included: no exclusions.  Two cases per op,
    the non-negative patterns and the negative ones."""
    t = time.perf_counter()
    left_out, _, _ = sweep_vs_oracle(dev, op, half << 31, 1 << 31)
    assert left_out == 0
    dev.check()
    print("%s half %d: %.2f s" % (P.NAMES[op], half, time.perf_counter() - t))


def test_log2_nonneg_every_finite_nonneg(dev):
    """Op 17 at every pattern 0 .. 0x7f7fffff (its domain: finite x >= 0) against the oracle, and equal to op 1."""
    t = time.perf_counter()
    a, b = np.empty(HALF, np.uint32), np.empty(HALF, np.uint32)
    for off, n in chunks(P.INF_BITS, HALF):
        got = device_sweep(dev, P.LOG2_NONNEG, off, n, out=a)
        r = P.compare(P.LOG2_NONNEG, got, off, domain=P.FINITE_NONNEG)
        assert r.mismatches == 0 and r.excluded == 0, "device " + P.describe("log2_nonneg", r)
        full = device_sweep(dev, P.LOG2, off, n, out=b)
        ne = np.flatnonzero(got != full)
        assert ne.size == 0, "log2_nonneg != log2 at x = 0x%08x: 0x%08x, 0x%08x" % (
            off + ne[0], got[ne[0]], full[ne[0]])
    dev.check()
    print("log2_nonneg: %.2f s" % (time.perf_counter() - t))


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("y", P.EXPONENTS, ids=["%g" % y for y in P.EXPONENTS])
def test_pow_nonneg_every_finite_nonneg(dev, y, half):
    """pow_nonneg (11) and pow_nonneg_wave (13) at every finite x >= 0 in consecutive order (uniform waves), each
    against the oracle, and 13 equal to 11.  Two cases per exponent, 2^30 patterns each; the second ends with the 2^23
    non-finite patterns, which are left out of the comparison (and of nothing else)."""
    t = time.perf_counter()
    a, b = np.empty(HALF, np.uint32), np.empty(HALF, np.uint32)
    left_out = 0
    for off, n in chunks(1 << 30, HALF):
        start = (half << 30) + off
        plain = device_sweep(dev, P.POW_NONNEG, start, n, 1, P.NONNEG, y, a)
        r = P.compare(P.POW_NONNEG, plain, start, 1, P.NONNEG, y, P.FINITE_NONNEG)
        assert r.mismatches == 0, "device " + P.describe("pow_nonneg", r, y)
        wave = device_sweep(dev, P.POW_WAVE, start, n, 1, P.NONNEG, y, b)
        r = P.compare(P.POW_WAVE, wave, start, 1, P.NONNEG, y, P.FINITE_NONNEG)
        assert r.mismatches == 0, "device " + P.describe("pow_nonneg_wave", r, y)
        left_out += r.excluded
        fin = max(0, min(n, P.INF_BITS - start))  # the finite x of this chunk come first
        ne = np.flatnonzero(plain[:fin] != wave[:fin])
        assert ne.size == 0, "pow_nonneg_wave != pow_nonneg (y = %r) at x = 0x%08x: 0x%08x, 0x%08x" % (
            y, start + ne[0], wave[ne[0]], plain[ne[0]])
    assert left_out == (NONFINITE_NONNEG if half else 0)
    dev.check()
    print("pow_nonneg, pow_nonneg_wave y = %g half %d: %.2f s" % (y, half, time.perf_counter() - t))


@pytest.mark.parametrize("y", P.EXPONENTS, ids=["%g" % y for y in P.EXPONENTS])
def test_pow_wave_mixed_order(dev, y):
    """pow_nonneg_wave with the multiplier 0x9e3779b1 over all 2^31 non-negative patterns: a wave mixes binades
    and holds zero, subnormal and non-finite lanes beside ordinary ones.  The finite-x lanes are compared (exactly
    2^23 left out); the non-finite lanes stay in their waves and make them take the clamped path.  For the exponents
    below 1 both kinds of wave, with and without a lane whose y * log2(x) is outside [-150, 128) or not finite, are at
    least 1 % of the waves (measured: 8,388,609 of 33,554,432, the 2^23 non-finite lanes one to a wave and the wave
    with x = 0); for 1.5 and 40 nearly every mixed wave is special, and the consecutive order above supplies the
    uniform ones."""
    t = time.perf_counter()
    left_out, special, ordinary = sweep_vs_oracle(dev, P.POW_WAVE, 0, 1 << 31, MIX, P.NONNEG, y, P.FINITE_NONNEG,
                                                  census=True)
    assert left_out == NONFINITE_NONNEG
    waves = (1 << 31) // 64
    assert special + ordinary == waves
    print("pow_nonneg_wave mixed y = %g: %d special, %d ordinary waves, %.2f s" % (
        y, special, ordinary, time.perf_counter() - t))
    if y < 1:
        assert special >= waves // 100 and ordinary >= waves // 100
    dev.check()


def _fmt(name, a, b, got, want, i):
    return "device %s(0x%08x, 0x%08x) = 0x%08x, oracle 0x%08x" % (name, a[i], b[i], got[i], want[i])


@pytest.mark.parametrize("gop,oop", [(P.POW, 0), (P.MAX, 1), (P.MIN, 2)], ids=["pow", "max", "min"])
def test_binary_edge_pairs(dev, gop, oop):
    """pow, max and min (the array path) at every ordered pair of the edge set against the oracle; for max and min
    also the sign of a zero result, and a NaN only when both inputs are NaN."""
    import gpgpuraytrace_amd as G
    t = time.perf_counter()
    a, b = P.edge_pairs()
    got = np.empty(a.size, np.uint32)
    assert G.lib().rt_debug_math(dev._h, gop, a.ctypes.data, b.ctypes.data, got.ctypes.data, a.size) == 0
    want = O.binary(oop, a.view(np.float32), b.view(np.float32)).view(np.uint32)
    nan = lambda u: (u & P.NONNEG) > P.INF_BITS  # noqa: E731
    ne = np.flatnonzero((got != want) & ~(nan(got) & nan(want)))
    assert ne.size == 0, "%d mismatches: %s" % (ne.size, _fmt(P.NAMES[gop], a, b, got, want, ne[0]))
    if gop != P.POW:
        bad = np.flatnonzero(nan(got) != (nan(a) & nan(b)))
        assert bad.size == 0, "NaN: " + _fmt(P.NAMES[gop], a, b, got, want, bad[0])
        zeros = ((a & P.NONNEG) == 0) & ((b & P.NONNEG) == 0)
        sign = (a & b) if gop == P.MAX else (a | b)  # max: -0 only from two -0; min: +0 only from two +0
        bad = np.flatnonzero(zeros & (got != sign))
        assert bad.size == 0, "zero sign: " + _fmt(P.NAMES[gop], a, b, got, want, bad[0])
        # any other zero result (beside a NaN, or against a value of the other side) is one of the inputs, sign included
        z = ((got & P.NONNEG) == 0) & ~zeros
        bad = np.flatnonzero(z & (got != a) & (got != b))
        assert bad.size == 0, "zero sign: " + _fmt(P.NAMES[gop], a, b, got, want, bad[0])
    dev.check()
    print("%s pairs: %d, %.2f s" % (P.NAMES[gop], a.size, time.perf_counter() - t))
