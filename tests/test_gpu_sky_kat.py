"""GPU known-answer tests of the sky against tests/sky_ref.py, the float64 restatement of sky.hlsl, on the sets and
within the bounds of tests/test_sky_kat.py: rt_debug_sky over the sphere, the horizon band and the cones about the
sun for every eye and sun of the CPU test (bit-equal to the oracle, inside the restatement's bounds, the same
non-finite mask at Eye.y = 5000 and at the nadir, the same bits whatever the launch's size), then the product path,
which is another kernel: shaded rays that end in the sky, and whole frames with the sun's disc or the stars in view
(the float colours and the RGBA8 codes of the product kernels, of an RGBA8-only device and of a two-frame batch,
bit for bit the oracle's)."""
import numpy as np
import pytest

import hlsl_ref as H
import oracle_lib as O
import shade_ref as SH
import sky_ref as R
import test_sky_kat as K
from test_gpu_parity import bits_equal, make

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 256, 257)  # around k_debug_sky's block of 256 threads
HIGH = (0.0, 3000.0, 0.0)   # above every landscape's ceiling, and the eye of the shaded rays
RAY_SUNS = ("t=0.27", "t=0.05")  # the low sun, whose Mie peak is in the hundreds, and the night with its stars
DISC = 0.03                 # rad: the pixels this close to SunDirection are the disc (a 64x48 pixel spans 0.03)


def _sky_consts(eye, sun_vec):
    return {"width": 64, "height": 48, "eye": np.array(list(eye) + [1.0], np.float32),
            "view_inverse": np.eye(4, dtype=np.float32), "projection": np.eye(4, dtype=np.float32),
            "sun": np.asarray(sun_vec, np.float32)}


def _debug_sky(ter, dirs):
    import gpgpuraytrace_amd as G
    d = np.ascontiguousarray(dirs, np.float32)
    out = np.empty((len(d), 7), np.float32)
    assert G.lib().rt_debug_sky(ter.compute._h, d.ctypes.data, out.ctypes.data, len(d)) == 0
    return out


def _set_sun(ter, sun_vec):
    ter.set_time_of_day_vec(sun_vec)
    ter.update_shaders()


@pytest.mark.parametrize("eye", K.SPHERE_EYES + [K.NAN_EYE])
def test_sky_over_the_sphere_and_at_the_sun_device(eye):
    """One device per eye, every sun in turn.  At NAN_EYE the scattering is NaN on both sides and only the masks
    and the stars are compared; everywhere else the device must repeat the oracle's bits and so its error."""
    dev, ter = make(_sky_consts(eye, K.suns()["t=0.3"]))
    for name, sun_vec in K.suns().items():
        _set_sun(ter, sun_vec)
        d = K.sphere_directions(name)
        got = _debug_sky(ter, d)
        if eye == K.NAN_EYE:
            ref = O.sky(O.noise_tables(), K.sky_frame(eye, sun_vec), d)
            assert np.all(np.isnan(ref[:, 0:6]))
        else:
            ref = K.oracle_sky(eye, name)
            K.check_case(got, eye, name)
        assert np.array_equal(np.isfinite(got), np.isfinite(ref)), name
        assert bits_equal(got, ref), name
    dev.destroy()


def test_sky_block_tail_device():
    """k_debug_sky with 1, 255, 256 and 257 directions (its block is 256 threads) and with the whole set: equal at
    the indices they share."""
    name = "t=0.27"
    dev, ter = make(_sky_consts(K.EYES[1], K.suns()[name]))
    d = K.sphere_directions(name)
    whole = _debug_sky(ter, d)
    assert bits_equal(whole, K.oracle_sky(K.EYES[1], name))
    for n in SIZES:
        part = _debug_sky(ter, d[:n])
        assert part.shape == (n, 7) and bits_equal(part, whole[:n]), n
    dev.destroy()


def _sky_rays(name):
    """Rays from HIGH along the two cones of the sun and the horizon band."""
    d = np.concatenate([K.cones(K.suns()[name]), K.horizon_band().astype(np.float32)])
    return np.tile(np.array(HIGH, np.float32), (len(d), 1)), d


def composed_bound(mie, ray, denom, eye_cond):
    """traceSample's miss is mie + rayleigh + stars (tracescreen.hlsl:25-27, 37-38 with no fog): the three bounds of
    test_sky_kat summed per channel, and two float32 additions."""
    b_r, b_m, b_s = K.bounds(denom, eye_cond)
    total = np.abs(mie) + np.abs(ray)
    return b_m[:, None] * (np.abs(mie) + K.FLOOR) + b_r * (np.abs(ray) + K.FLOOR) + b_s + 2.0 * K.ULP * total


@pytest.mark.parametrize("land", ["nomadplains", "greenrocks"])
def test_shaded_rays_that_end_in_the_sky_device(land):
    """shade_rays (k_trace's shading, not k_debug_sky) for rays from above the terrain: the float colour is the
    oracle's trace_sample bit for bit; on nomadplains (no fog) the misses are also inside the composed bound of
    hlsl_ref.sample_color's miss branch."""
    c = _sky_consts(HIGH, K.suns()[RAY_SUNS[0]])
    dev, ter = make(c, land)
    for name in RAY_SUNS:
        sun_vec = K.suns()[name]
        _set_sun(ter, sun_vec)
        o, d = _sky_rays(name)
        res = ter.shade_rays(o, d, eye=np.array(HIGH, np.float32))
        dev.check()
        assert res is not None
        col, _ = SH.trace_sample(o, d, HIGH, land, sun=sun_vec)
        miss = ~(res[:, 7] > 0)
        assert miss.sum() >= len(K.cone(sun_vec)) + 64, (name, miss.sum())  # a whole cone and most of the band
        assert np.all(np.isfinite(col)) and bits_equal(res[:, :3], col), name
        if land != "nomadplains":
            continue
        m = np.flatnonzero(miss)
        pdn = d[m].astype(np.float64) / np.linalg.norm(d[m].astype(np.float64), axis=1, keepdims=True)
        fc = np.zeros((len(m), 4))  # nomadplains' getFog is 0
        ref, _ = H.sample_color(land, res[m][:, [4, 5, 6, 3]], res[m, 7], fc, pdn, HIGH, sun_vec, None, None, None)
        mie, ray, denom, eye_cond = R.rayleigh_mie(pdn, np.array(HIGH), sun_vec, conditioning=True)
        err = np.abs(res[m, :3].astype(np.float64) - ref)
        assert np.all(err <= composed_bound(mie, ray, denom, eye_cond)), (name, (err / composed_bound(mie, ray, denom, eye_cond)).max())
    dev.destroy()


# --- the sun and the stars in view -----------------------------------------------------------------
def sun_in_view():
    """64x48 at t = 0.27 from the reset position, the camera's front along +SunDirection: the low sun's disc at the
    frame's centre."""
    from gpgpuraytrace_amd import camera
    cam = camera.Camera(64, 48)
    cam.front = camera.sun_direction(0.27).astype(np.float64)
    cam.update()
    return camera.camera_constants(cam, 0.27)


def stars_in_view():
    """64x48 at night (t = 0.05), pitched up: every pixel is sky, with the stars on."""
    from gpgpuraytrace_amd import camera
    return camera.frame_constants(64, 48, euler=(-2.0, -4.6, 0.0), time_of_day=0.05)


def oracle_frame(consts):
    return O.render(O.noise_tables(), O.make_frame(consts))


def disc_pixels(consts):
    """(rows, columns, ray directions) of the pixels whose ray lies within DISC of SunDirection."""
    py, px = np.mgrid[0:consts["height"], 0:consts["width"]]
    _, d = H.pixel_ray(consts, px.ravel(), py.ravel())
    cos = (d @ np.asarray(consts["sun"], np.float64)) / np.linalg.norm(d, axis=1)
    near = np.flatnonzero(cos >= np.cos(DISC))
    return near // consts["width"], near % consts["width"], d[near].astype(np.float32)


def test_sun_and_stars_in_view_device():
    """The four pixels about the frame's centre look 0.021 rad past SunDirection, where the Mie term is 11 to 23
    (it reaches the hundreds only within 0.005 rad, between these pixels): their stored colour saturates and their
    codes are 255.  The night frame is all sky, 3 % of it stars (the rest of the field is negative and stored as 0).
    Both frames from the product kernels with and without the float target, alone and as a batch of two."""
    from gpgpuraytrace_amd import engine as E
    scenes = [sun_in_view(), stars_in_view()]
    refs = [oracle_frame(c) for c in scenes]
    rows, cols, disc = disc_pixels(scenes[0])
    assert len(rows) == 4
    assert O.sky(O.noise_tables(), O.make_frame(scenes[0]), disc)[:, 0:3].min() > 10.0
    assert np.all(refs[0]["rgba8"][rows, cols] == 255) and np.all(refs[0]["rgba32f"][rows, cols] == 1.0)
    assert refs[1]["stats"]["primary_hits"] == 0 and (refs[1]["rgba32f"][..., :3] > 0).mean() > 0.02  # stars
    for c, ref in zip(scenes, refs):
        assert np.all(np.isfinite(ref["rgba32f"]))
        dev, ter = make(c)
        ter.render_device()
        assert bits_equal(dev.readback_float(), ref["rgba32f"])
        assert np.array_equal(dev.readback(), ref["rgba8"])
        dev.destroy()
        dev, ter = make(c, float_output=False)
        ter.render_device()
        assert np.array_equal(dev.readback(), ref["rgba8"])
        dev.destroy()
    for float_output in (True, False):
        frames = [make(c, float_output=float_output) for c in scenes]
        E.render_batch([t for _, t in frames])
        for (d, _), ref in zip(frames, refs):
            px = d.readback()
            assert np.array_equal(px, ref["rgba8"])
            if float_output:
                assert bits_equal(d.readback_float(), ref["rgba32f"])
        assert np.all(frames[0][0].readback()[rows, cols] == 255)
        for d, _ in frames:
            d.destroy()
