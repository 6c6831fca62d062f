"""k_trace's sky exit (rt_shader.h sky_exit, RT_SKY_EXIT): the product kernels end a primary ray that does not
descend once its next sample lies above the nomadplains ceiling (256).  The frames must stay the oracle's, bit
for bit, from poses that put rays on every side of the test; the predicate itself is pinned through
rt_debug_math op 14 against an exact host restatement."""
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_parity import bits_equal, make

pytestmark = pytest.mark.gpu

W = H = 64
CEIL = 256.0
YAW = -4.6
# (eye, euler): pitch -3.0 is the reset pose, -1.2 looks 69 degrees up, +1.2 as far down, 0 is level
POSES = {
    "reset": ((0.0, 100.0, 0.0), (-3.0, YAW, 0.0)),         # upward rays both hit mountains and miss
    "up": ((0.0, 100.0, 0.0), (-1.2, YAW, 0.0)),            # every ray has dir.y > 0
    "above_up": ((0.0, 300.0, 0.0), (-1.2, YAW, 0.0)),      # every ray exits before its first step
    "above_down": ((0.0, 300.0, 0.0), (1.2, YAW, 0.0)),     # rays cross the ceiling downward: full marches
    "level_below": ((0.0, 255.0, 0.0), (0.0, YAW, 0.0)),    # dir.y straddles 0, from just below the ceiling
    "level_above": ((0.0, 257.0, 0.0), (0.0, YAW, 0.0)),    # ... and from just above
}


def pose_consts(name):
    import gpgpuraytrace_amd as G
    eye, euler = POSES[name]
    return G.frame_constants(W, H, position=eye, euler=euler)


def ray_dir_y(c):
    """dir.y of every pixel ray (get_pixel_ray, tracing.hlsl:124-134), in float64."""
    M = np.asarray(c["view_inverse"], np.float64).reshape(4, 4)
    P = np.asarray(c["projection"], np.float64).reshape(4, 4)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    sx = ((px + 0.5) / W - 0.5) * 2.0 * P[1, 1]
    sy = ((py + 0.5) / H - 0.5) * 2.0 * P[0, 0]
    r = sx[..., None] * M[0, :3] + sy[..., None] * M[1, :3] + M[2, :3] + M[3, :3]
    d = r - np.asarray(c["eye"], np.float64)[:3]
    return d[..., 1] / np.linalg.norm(d, axis=-1)


def test_poses_are_what_they_claim():
    dy = {n: ray_dir_y(pose_consts(n)) for n in POSES}
    assert (dy["reset"] > 0.3).any() and (dy["reset"] < -0.3).any()
    assert dy["up"].min() > 0.2 and dy["above_up"].min() > 0.2
    assert dy["above_down"].max() < -0.2
    for n in ("level_below", "level_above"):
        assert (dy[n] > 0).any() and (dy[n] < 0).any() and abs(dy[n]).min() < 0.02
    assert POSES["level_below"][0][1] < CEIL < POSES["level_above"][0][1] and POSES["above_up"][0][1] > CEIL


_oracle = {}


def oracle_frame(pose, ms, ao, aa):
    key = (pose, ms, ao, aa)
    if key not in _oracle:
        r = O.render(O.noise_tables(), O.make_frame(pose_consts(pose), max_steps=ms, ao=ao, aa=aa))
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _oracle[key] = r
    return _oracle[key]


@pytest.mark.parametrize("aa", [1, 4])
@pytest.mark.parametrize("ao", [1, 0])
@pytest.mark.parametrize("ms", [512, 0])
@pytest.mark.parametrize("pose", list(POSES))
def test_frame_bitexact(pose, ms, ao, aa):
    """The product (non-STATS) kernels' frame, float32 and RGBA8, equals the oracle's."""
    ref = oracle_frame(pose, ms, ao, aa)
    dev, ter = make(pose_consts(pose), max_steps=ms, ao=ao, aa=aa)
    ter.render_device()
    dev.present()
    assert bits_equal(dev.readback_float(), ref["rgba32f"])
    assert np.array_equal(dev.readback(), ref["rgba8"])
    dev.check()
    dev.destroy()
    hits, rays = int(ref["stats"]["primary_hits"]), int(ref["stats"]["primary_rays"])
    assert rays == W * H * aa
    if pose == "above_up":
        assert hits == 0
    if pose in ("reset", "above_down"):
        assert 0 < hits and (pose == "above_down" or hits < rays)


def test_product_device_rgba8_bitexact():
    """The product's RGBA8-only device (hit pixels finished in k_trace) from the reset pose."""
    ref = oracle_frame("reset", 512, 1, 1)
    dev, ter = make(pose_consts("reset"), max_steps=512, ao=1, float_output=False)
    ter.render_device()
    dev.present()
    assert np.array_equal(dev.readback(), ref["rgba8"])
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("pose", list(POSES))
def test_gated_launch_bitexact(pose):
    """The gated launch's own k_trace instantiation (the prepass inside the trace kernel) takes the exit too."""
    ref = oracle_frame(pose, 512, 1, 1)
    dev, ter = make(pose_consts(pose), max_steps=512, ao=1, gated=True)
    ter.render_device()
    assert dev.launch_info() == (1, 0)
    assert bits_equal(dev.readback_float(), ref["rgba32f"])
    assert np.array_equal(dev.readback(), ref["rgba8"])
    dev.check()
    dev.destroy()


BATCH = ("reset", "above_up", "level_below")


def test_batch_of_three_cameras():
    """Three cameras in one launch: rays that exit, rays that march out and hits share the waves."""
    from gpgpuraytrace_amd import engine as E
    frames = [make(pose_consts(p), max_steps=512, ao=1) for p in BATCH]
    E.render_batch([t for _, t in frames])
    for (dev, _), p in zip(frames, BATCH):
        ref = oracle_frame(p, 512, 1, 1)
        assert bits_equal(dev.readback_float(), ref["rgba32f"]), p
        assert np.array_equal(dev.readback(), ref["rgba8"]), p
        dev.check()
    for dev, _ in frames:
        dev.destroy()


def test_sharded_packed_path():
    """The 2-way sharded launch that writes its shards straight into the packed buffer (the bench's path)."""
    import torch

    from gpgpuraytrace_amd import engine as E
    from gpgpuraytrace_amd import parallel as P
    world = 2
    plan = P.BatchPlan(W, H, len(BATCH), world)
    frames = [make(pose_consts(p), max_steps=512, ao=1, float_output=False) for p in BATCH]
    want = [oracle_frame(p, 512, 1, 1)["rgba8"].view(np.uint32).reshape(H, W) for p in BATCH]
    inside_of = {}
    seen = 0
    for rank in range(world):
        buf = torch.zeros(plan.packed_bytes(), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        E.render_batch_packed([t for _, t in frames], rank, world, buf.data_ptr(), plan.max_bytes)
        for d, _ in frames:
            d.synchronize()
            d.check()
        got = buf.cpu().numpy().view(np.uint32)
        for f, s, off in plan.packs(rank):
            exp = P.pack_host(want[f], s, world)
            if s not in inside_of:
                inside_of[s] = P.pack_host(np.ones((H, W), np.uint32), s, world) == 1
            part = got[off // 4:off // 4 + exp.size]
            assert np.array_equal(part[inside_of[s]], exp[inside_of[s]]), (rank, f, s)
            seen += int(inside_of[s].sum())
    assert seen == len(BATCH) * W * H  # every pixel of every frame was compared
    for d, _ in frames:
        d.destroy()


def f32(x):
    return np.float32(x)


def host_predicate(py, dy, dist):
    """sky_exit restated exactly: dir.y >= 0 and RN32(dir.y * dist + p.y) > 256.  The fused product-sum is
    evaluated in rationals; a float32 exceeds 256 after rounding iff the exact value exceeds 256 + 2^-16, the
    midpoint to the next float (the tie rounds to even, to 256)."""
    vals = (float(py), float(dy), float(dist))
    if any(np.isnan(v) for v in vals):
        return False
    if not dy >= 0:
        return False
    if any(np.isinf(v) for v in vals):
        with np.errstate(all="ignore"):
            return bool(np.float64(dy) * np.float64(dist) + np.float64(py) > CEIL)  # inf arithmetic is exact; nan > x is False
    v = Fraction(float(dy)) * Fraction(float(dist)) + Fraction(float(py))
    return v > Fraction(CEIL) + Fraction(1, 2 ** 16)


def predicate_inputs():
    up = np.nextafter(f32(CEIL), f32(np.inf))
    dn = np.nextafter(f32(CEIL), f32(0))
    den = np.array([1], np.uint32).view(np.float32)[0]  # the smallest denormal
    t = [
        # dir.y = +-0: y stays p.y, and -0 counts as not descending
        (up, 0.0, 10.0), (up, -0.0, 10.0), (CEIL, 0.0, 10.0), (CEIL, -0.0, 1e6), (dn, 0.0, 5000.0), (300.0, -0.0, 0.0),
        # denormal and negative dir.y
        (up, den, 1.0), (CEIL, den, 1e30), (CEIL, den, 3e38), (up, -den, 1.0), (300.0, -den, 0.0), (300.0, -1e-30, 0.0),
        (300.0, -0.5, 1.0), (1000.0, -1.0, 10.0), (100.0, -0.7, 4000.0),
        # y equal to the ceiling and one ulp either side, at dist = 0 and reached by the fma
        (CEIL, 0.5, 0.0), (up, 0.5, 0.0), (dn, 0.5, 0.0), (CEIL, 1.0, 0.0), (up, 1.0, 0.0),
        (0.0, 1.0, CEIL), (0.0, 1.0, up), (0.0, 1.0, dn), (128.0, 0.5, 256.0), (128.0, 0.5, np.nextafter(f32(256), f32(300))),
        # the product enters unrounded: 256 + 2^-16 is the tie (stays 256), a little more rounds up
        (CEIL, 2.0 ** -16, 1.0), (CEIL, 2.0 ** -16, np.nextafter(f32(1), f32(2))), (CEIL, 2.0 ** -17, 1.0),
        (CEIL, 2.0 ** -15, 1.0), (dn, 2.0 ** -16, 1.0), (dn, 3.0 * 2.0 ** -17, 1.0),
        # ordinary rays, far samples, specials
        (100.0, 0.14, 1114.0), (100.0, 0.14, 1115.0), (100.0, 0.3, 4999.0), (255.0, 1e-3, 999.0), (255.0, 1e-3, 1001.0),
        (np.nan, 0.5, 1.0), (300.0, np.nan, 1.0), (300.0, 0.5, np.nan), (np.inf, 0.5, 1.0), (-np.inf, 0.5, 1.0),
        (100.0, 0.5, np.inf), (100.0, 0.0, np.inf), (300.0, np.inf, 0.0),
    ]
    rng = np.random.default_rng(5)
    n = 4096
    rnd = np.stack([rng.uniform(0, 400, n), rng.uniform(-1, 1, n), rng.uniform(0, 5000, n)], axis=1)
    # samples that land within a few ulp of the ceiling
    k = 1024
    dy = rng.uniform(0.01, 1, k).astype(np.float32)
    dist = rng.uniform(1, 2000, k).astype(np.float32)
    py = (CEIL - dy.astype(np.float64) * dist.astype(np.float64)).astype(np.float32)
    near = np.stack([py, dy, dist], axis=1)
    return np.concatenate([np.array(t, np.float32), rnd.astype(np.float32), near]).astype(np.float32)


def test_predicate_op():
    import gpgpuraytrace_amd as G
    a = np.ascontiguousarray(predicate_inputs())
    n = len(a)
    out = np.full(n + 1, -1.0, np.float32)
    dev = G.DeviceFactory.construct(G.DeviceAPI.HIP, 8, 8)
    assert G.lib().rt_debug_math(dev._h, 14, a.ctypes.data, None, out.ctypes.data, n) == 0
    dev.destroy()
    want = np.array([host_predicate(*row) for row in a])
    assert set(np.unique(out[:n])) <= {0.0, 1.0}
    bad = np.nonzero((out[:n] == 1.0) != want)[0]
    assert bad.size == 0, [(a[i].tolist(), float(out[i])) for i in bad[:8]]
    assert want.sum() > 500 and (~want).sum() > 500
    # the ceiling the host computed for the product's octave constants stands below the kernel's literal
    assert 240.0 < out[n] <= CEIL
