"""The trimmed march step (rt_math.h pow_nonneg_wave, rt_shader.h noise3d_z0, k_trace's per-lane
primary loop): each piece bit for bit against what it replaced and against the CPU oracle."""
import numpy as np
import pytest

import golden_index as GI
import oracle_lib as O
from test_gpu_parity import bits_equal, make

pytestmark = pytest.mark.gpu

NP_EXPO = np.float32(0.68) + np.float32(0.1)  # rt_runtime.cpp: nomadplains' density exponent
DENSITY_FACTOR = np.float32(0.35)             # the step factor's exponent (0.15 when recording)


def u2f(u):
    return np.array(u, np.uint32).view(np.float32)


def wave_pow_inputs():
    """4096 (base, exponent) pairs = 64 waves of 64 lanes.  Waves 0..31 hold ordinary lanes only
    (y*log2(x) inside [-150, 128), nonzero base): the straight-line path.  Waves 32..63 hold ordinary
    lanes and exactly ONE special lane, at a position that moves with the wave."""
    rng = np.random.default_rng(7)
    n = 4096
    x = np.exp(rng.uniform(np.log(1e-6), np.log(1e4), n)).astype(np.float32)
    y = np.array([NP_EXPO, 1.5, DENSITY_FACTOR, DENSITY_FACTOR - np.float32(0.2)], np.float32)[np.arange(n) % 4]
    # mantissas on both sides of log2's 0x3fb504f3 split (sqrt 2), at several exponents, in ordinary waves
    split = [((0x3FB504F3 + d) & 0x007FFFFF) | (e << 23) for e in (110, 126, 127, 128, 139) for d in (-2, -1, 0, 1, 2)]
    x[64:64 + len(split)] = u2f(split)
    special = [
        (0.0, NP_EXPO), (0.0, 1.5), (0.0, DENSITY_FACTOR),      # base +0
        (1e-40, NP_EXPO), (u2f(1), DENSITY_FACTOR),             # denormal bases, ordinary results
        (1e-40, 1.5), (1e-6, 8.0), (3e-3, 18.0),                # y*log2(x) below -150: +0
        (1e4, 10.0), (2.0, 128.0), (3.0e38, 1.5),               # at or above 128: +inf
    ]
    x[0:2], y[0:2] = [0.5, 2.0], [150.0, 127.99999]             # exactly -150 and just under 128: ordinary
    for w in range(32, 64):
        lane = (w * 7) % 64
        bx, by = special[(w - 32) % len(special)]
        x[w * 64 + lane], y[w * 64 + lane] = np.float32(bx), np.float32(by)
    return x, y


def test_wave_pow_bitexact():
    """rt_debug_math op 13 (pow_nonneg_wave) == op 11 (pow_nonneg) == the oracle's ro_pow, bit for bit."""
    import gpgpuraytrace_amd as G
    dev = G.DeviceFactory.construct(G.DeviceAPI.HIP, 8, 8)
    x, y = wave_pow_inputs()
    got, old = np.empty_like(x), np.empty_like(x)
    assert G.lib().rt_debug_math(dev._h, 13, x.ctypes.data, y.ctypes.data, got.ctypes.data, x.size) == 0
    assert G.lib().rt_debug_math(dev._h, 11, x.ctypes.data, y.ctypes.data, old.ctypes.data, x.size) == 0
    dev.destroy()
    ref = O.binary(0, x, y)
    assert np.isinf(ref).sum() >= 4 and (ref == 0).sum() >= 8
    assert np.array_equal(got.view(np.uint32), old.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def z0_points(limit, beyond):
    """4096 (x, y, 0): both signs, cell boundaries and their float neighbours, +-limit; with
    `beyond`, coordinates past 2^13 as well."""
    rng = np.random.default_rng(11)
    xy = rng.uniform(-300, 300, (4096, 2)).astype(np.float32)
    ints = rng.integers(-200, 200, (600, 2)).astype(np.float32)
    xy[0:600] = ints                                       # lattice points: the value is a zero
    xy[600:900, 0] = np.nextafter(ints[:300, 0], np.float32(np.inf))   # just inside the next cell
    xy[900:1200, 1] = np.nextafter(ints[:300, 1], np.float32(-np.inf))  # just inside the previous one
    xy[1200:1500] = rng.uniform(-limit, limit, (300, 2))
    edge = np.float32(limit)
    xy[1500:1508] = [[edge, edge], [-edge, -edge], [edge, -edge], [-edge, 0.5], [edge - 0.5, 0.25], [0.0, edge],
                     [-0.0, -edge], [np.nextafter(edge, np.float32(0)), 1.0]]
    if beyond:
        xy[1508:2000] = rng.uniform(-2e6, 2e6, (492, 2))
        xy[2000:2008] = [[8192, 8192], [-8193, 8193.5], [16384.25, -8192], [1e6, -1e6], [-8192.5, 3], [3, 70000.5],
                         [-123456.75, 8191], [2 ** 22 + 0.5, -(2 ** 22)]]
    return np.concatenate([xy, np.zeros((4096, 1), np.float32)], axis=1).astype(np.float32)


@pytest.mark.parametrize("mode,limit,beyond", [(2, 8191.0, True), (3, 8191.0, False)], ids=["general", "fast"])
def test_noise3d_z0_variants(mode, limit, beyond):
    """noise3d_z0 (rt_debug_noise mode 2) and its FAST variant (mode 3, |x|, |y| <= 2^13 - 1) equal the
    oracle's noise3d(x, y, 0): every nonzero value bit for bit, zeros up to their sign."""
    import gpgpuraytrace_amd as G
    dev, ter = make(GI.consts(64, 48, "reset"))
    p = z0_points(limit, beyond)
    assert np.abs(p).max() == limit or beyond
    out = np.empty(len(p), np.float32)
    assert G.lib().rt_debug_noise(ter.compute._h, p.ctypes.data, out.ctypes.data, len(p), mode) == 0
    dev.destroy()
    ref = O.noise3d(O.noise_tables(), p)
    assert np.array_equal(out, ref)  # +0 == -0
    assert bits_equal(out[ref != 0], ref[ref != 0])
    assert (ref == 0).sum() >= 600 and (ref != 0).sum() >= 3000


@pytest.fixture(scope="module")
def small_frame():
    """64x48 nomadplains, shadow + 1 AO ray, 64-step cap: the oracle's frame, rendered once."""
    consts = GI.consts(64, 48, "reset")
    return consts, O.render(O.noise_tables(), O.make_frame(consts, max_steps=64, ao=1))


@pytest.mark.parametrize("stats", [False, True], ids=["product", "stats"])
def test_small_frame_bitexact(small_frame, stats):
    consts, ref = small_frame
    dev, ter = make(consts, max_steps=64, ao=1, stats=stats)
    ter.render_device()
    dev.present()
    assert bits_equal(dev.readback_float(), ref["rgba32f"])
    assert np.array_equal(dev.readback(), ref["rgba8"])
    dev.check()
    if stats:
        st, rs = dev.stats(), ref["stats"]
        assert (st["primary_steps"], st["shadow_steps"], st["ao_steps"]) == \
            (rs["primary_steps"], rs["shadow_steps"], rs["ao_steps"])
        assert rs["primary_steps"] > 0 and rs["shadow_steps"] > 0 and rs["ao_steps"] > 0
    dev.destroy()


@pytest.mark.parametrize("stats", [False, True], ids=["product", "stats"])
def test_small_frame_batch_of_three(small_frame, stats):
    """Three such frames in one batch: the long-ray and segment loops run with rays of several frames."""
    from gpgpuraytrace_amd import engine as E
    consts, ref = small_frame
    frames = [make(consts, max_steps=64, ao=1, stats=stats) for _ in range(3)]
    E.render_batch([t for _, t in frames])
    for dev, _ in frames:
        assert bits_equal(dev.readback_float(), ref["rgba32f"])
        assert np.array_equal(dev.readback(), ref["rgba8"])
    if stats:
        st, rs = frames[0][0].stats(), ref["stats"]
        assert (st["primary_steps"], st["shadow_steps"], st["ao_steps"]) == \
            (3 * rs["primary_steps"], 3 * rs["shadow_steps"], 3 * rs["ao_steps"])
    for dev, _ in frames:
        dev.destroy()
