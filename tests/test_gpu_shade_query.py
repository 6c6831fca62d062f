"""GPU tests of the shaded queries (rt_terrain_shade_rays / _device, ABI 9 additive): caller-supplied rays shaded
as tracescreen shades one sample of a pixel (tracescreen.hlsl:16-48, no AO).  Bar: the 8 result floats, the RGBA8
pixel and both step counts equal the checker's (tests/shade_ref.py: the oracle's own trace_ray, get_normal,
get_color and sky) bit for bit, at every size, grid and option; a query equals the frame at the frame's own pixel
rays; and a query between two renders changes nothing about the frame loop."""
import ctypes as C

import numpy as np
import pytest

import golden_index as GI
import ray_fixture as RF
import shade_ref as SH
from test_gpu_parity import FixedCamera, _device_cells, make

pytestmark = pytest.mark.gpu

RT_OK, RT_ERR_INVALID, RT_ERR_UNSUPPORTED, RT_ERR_STATE = 0, -1, -4, -5
DEFER = dict(deferred=True, debug_defer_small=True)
F_EYE = RF.eye("F0")


def _make(land="nomadplains", **kw):
    """A 64x48 device and its terrain: the golden reset pose (Eye = F's eye) under the shaded tests' sun."""
    consts = dict(GI.consts(64, 48, "reset"))
    consts["sun"] = SH.SUN
    return make(consts, land, float_output=False, **kw)


def _same(got, want, what=""):
    """got: (results, rgba8, steps) of shade_rays; want: the checker's tuple."""
    res, px, steps = got
    wres, wpx, wsteps = want[:3]
    assert res.shape == wres.shape and res.shape[1:] == (8,) and res.dtype == np.float32
    assert px.dtype == np.uint32 and steps.dtype == np.uint32 and steps.shape == wsteps.shape
    bad = np.flatnonzero((res.view(np.uint32) != wres.view(np.uint32)).any(axis=1))
    assert bad.size == 0, (what, bad.size, bad[:8], res[bad[:4]], wres[bad[:4]])
    assert np.array_equal(px, wpx), what
    bad = np.flatnonzero((steps != wsteps).any(axis=1))
    assert bad.size == 0, (what, bad.size, bad[:8], steps[bad[:4]], wsteps[bad[:4]])


def _pick(want, idx):
    return tuple(a[idx] for a in want[:3])


@pytest.mark.parametrize("land", RF.LANDSCAPES)
def test_parity_with_the_checker(land):
    """The F0-F3 query (n = 4096, one eye) and G (n = 1024, origin != eye): everything, then without the step
    counts, the results alone and the pixels alone."""
    import gpgpuraytrace_amd as G
    L = G.lib()
    dev, ter = _make(land)
    for names in (RF.F_SET, ("G",)):
        o, d = RF.query(names)
        eye = RF.eye(names[0])
        want = SH.query(names, land)
        got = ter.shade_rays(o, d, eye=eye, rgba8=True, steps=True)
        assert got is not None, L.rt_last_error()
        _same(got, want, names)
        res, px = ter.shade_rays(o, d, eye=eye, rgba8=True)  # the kernels without the step counts
        assert np.array_equal(res.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(px, want[1])
        res = ter.shade_rays(o, d, eye=eye)  # results only
        assert np.array_equal(res.view(np.uint32), want[0].view(np.uint32))
        px = np.zeros(len(o), np.uint32)  # rgba8 only
        opt = G.engine.surface_options(eye)
        assert L.rt_terrain_shade_rays(ter.compute._h, o.ctypes.data, d.ctypes.data, None, len(o), C.byref(opt), None,
                                       px.ctypes.data, None) == RT_OK
        assert np.array_equal(px, want[1])
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("max_blocks", [1, 2])
@pytest.mark.parametrize("land", ["nomadplains", "greenrocks"])
def test_refill_and_phase_mixing(land, max_blocks):
    """A grid of 1 or 2 blocks, n = 4096 + 37 under test_gpu_surface_query's seeded permutation: one block refills
    every lane several times, so lanes in their primary march, in their shadow march and at the shading coexist
    in a wave."""
    o, d = RF.query(RF.F_SET)
    perm = np.random.default_rng(4133).permutation(4096)
    idx = np.concatenate([perm, perm[:37]])
    dev, ter = _make(land)
    got = ter.shade_rays(o[idx], d[idx], eye=F_EYE, rgba8=True, steps=True, max_blocks=max_blocks)
    assert got is not None
    _same(got, _pick(SH.query(RF.F_SET, land), idx))
    dev.check()
    dev.destroy()


def test_sizes():
    """n = 1, 63, 64, 65 and 1025 from the head of the F0-F3 set, and n = 0, which launches nothing."""
    import gpgpuraytrace_amd as G
    L = G.lib()
    o, d = RF.query(RF.F_SET)
    want = SH.query(RF.F_SET, "nomadplains")
    dev, ter = _make()
    for n in (1, 63, 64, 65, 1025):
        got = ter.shade_rays(o[:n], d[:n], eye=F_EYE, rgba8=True, steps=True)
        assert got is not None, n
        _same(got, _pick(want, slice(0, n)), n)
    got = ter.shade_rays(o[:0], d[:0], eye=F_EYE, rgba8=True, steps=True)
    assert got is not None and got[0].shape == (0, 8) and got[1].shape == (0,) and got[2].shape == (0, 2)
    cs = ter.compute._h
    assert L.rt_terrain_shade_rays(cs, None, None, None, 0, None, None, None, None) == RT_OK
    assert L.rt_terrain_shade_rays_device(cs, None, 0, None, None, None, None) == RT_OK
    dev.check()
    dev.destroy()


def test_zero_directions_among_live_rays():
    """Zero directions give unspecified results but end (here: before their first step, so a refilled lane holds
    an ended march at once), and the rays around them are not disturbed.  A whole query of them ends too."""
    zo, zd = RF.query(("Z",))
    assert not zd.any()
    fo, fd = RF.query(("G",))
    mo, md = np.concatenate([zo[:100], fo[:200], zo[:30]]), np.concatenate([zd[:100], fd[:200], zd[:30]])
    dev, ter = _make()
    got = ter.shade_rays(mo, md, eye=RF.eye("G"), rgba8=True, steps=True, max_blocks=1)
    assert got is not None
    _same(tuple(a[100:300] for a in got), _pick(SH.query(("G",), "nomadplains"), slice(0, 200)))
    assert not got[2][:100].any() and not got[2][300:].any()  # no step of either march
    got = ter.shade_rays(zo, zd, eye=RF.eye("Z"), steps=True)
    assert got is not None and not got[1].any()
    dev.check()
    dev.destroy()


def test_options():
    """The seeded per-ray ranges, per-call params (t_min 0.5, t_max 100, stepmod 2), max_steps = 64, and the
    ranges together with max_steps."""
    o, d = RF.query(RF.F_SET)
    dev, ter = _make()
    rg = SH.SR.seeded_ranges()
    kw = dict(eye=F_EYE, rgba8=True, steps=True)
    _same(ter.shade_rays(o, d, ranges=rg, **kw), SH.query(RF.F_SET, "nomadplains", ranged=True), "ranges")
    res = ter.shade_rays(o, d, ranges=rg, eye=F_EYE)  # (the RANGE kernel without the step counts)
    assert np.array_equal(res.view(np.uint32), SH.query(RF.F_SET, "nomadplains", ranged=True)[0].view(np.uint32))
    _same(ter.shade_rays(o, d, t_min=0.5, t_max=100.0, stepmod=2.0, **kw),
          SH.query(RF.F_SET, "nomadplains", t_min=0.5, t_max=100.0, stepmod=2.0), "params")
    _same(ter.shade_rays(o, d, max_steps=64, **kw), SH.query(RF.F_SET, "nomadplains", max_steps=64), "max_steps")
    # the ranges override the per-call range, the other params hold beside them
    _same(ter.shade_rays(o, d, ranges=rg, t_min=7.0, t_max=8.0, max_steps=64, **kw),
          SH.query(RF.F_SET, "nomadplains", ranged=True, max_steps=64), "ranges + max_steps")
    dev.check()
    dev.destroy()


def test_options_on_another_landscape():
    o, d = RF.query(RF.F_SET)
    dev, ter = _make("greenrocks")
    _same(ter.shade_rays(o, d, ranges=SH.SR.seeded_ranges(), eye=F_EYE, stepmod=2.0, max_steps=64, rgba8=True, steps=True),
          SH.query(RF.F_SET, "greenrocks", ranged=True, stepmod=2.0, max_steps=64))
    dev.check()
    dev.destroy()


def test_eye():
    """The eye (the density's level of detail, getNormal's eps and the sky's camera): the option's, else the
    compute's Eye."""
    o, d = RF.query(("G",))
    want = SH.query(("G",), "nomadplains")
    want_f = SH.query(("G",), "nomadplains", eye="F0")
    assert not np.array_equal(want[0].view(np.uint32), want_f[0].view(np.uint32))
    dev, ter = _make()
    kw = dict(rgba8=True, steps=True)
    _same(ter.shade_rays(o, d, eye=RF.eye("G"), **kw), want)  # (the compute's Eye is F's)
    _same(ter.shade_rays(o, d, **kw), want_f)  # eye=None: the compute's, F's
    ter.set_camera(FixedCamera(RF.consts("G")))
    ter.update_terrain()  # writes the Eye variables
    _same(ter.shade_rays(o, d, **kw), want)
    dev.check()
    dev.destroy()


def test_frame_equivalence():
    """Camera F0 on a 256x256 float-output device with AA 1: at the fixture's pixels (px, py < 256), with ranges from
    the frame's own CellDistance, saturate(result.rgb) is readback_float's pixel and rgba8 the framebuffer's."""
    consts = dict(RF.consts("F0"))
    consts["sun"] = SH.SUN
    dev, ter = make(consts, "nomadplains", float_output=True)
    ter.render_device()
    dev.present()
    img, img8 = dev.readback_float(), dev.readback()
    keep, px, py, rg = SH.frame_pixels(_device_cells(ter))
    o, d = RF.rays("F0")
    res, pix = ter.shade_rays(o[keep], d[keep], ranges=rg, rgba8=True)
    hits = int((res[:, 7] > 0).sum())
    assert 64 <= hits <= len(keep) - 64
    sat = np.clip(res[:, :3], np.float32(0), np.float32(1))
    assert np.array_equal(sat.view(np.uint32), np.ascontiguousarray(img[py, px, :3]).view(np.uint32))
    assert np.array_equal(pix, np.ascontiguousarray(img8[py, px]).view(np.uint32).ravel())
    assert np.array_equal(dev.readback(), img8)  # the query left the frame alone
    dev.check()
    dev.destroy()


def test_device_form_equals_host_form():
    """torch-allocated rays and outputs; the rays are filled on torch's stream and handed over by event, the
    results handed back by event: no host synchronisation in between.  The output buffers start poisoned."""
    import torch
    import gpgpuraytrace_amd as G
    o, d = RF.query(("G",))
    n = len(o)
    rg = SH.SR.seeded_ranges(n)
    dev, ter = _make()
    host = ter.shade_rays(o, d, eye=RF.eye("G"), rgba8=True, steps=True)
    host_r = ter.shade_rays(o, d, ranges=rg, eye=RF.eye("G"), rgba8=True, steps=True)
    _same(host, SH.query(("G",), "nomadplains"))
    assert not np.array_equal(host[0].view(np.uint32), host_r[0].view(np.uint32))
    rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda:0")
    res = torch.full((n, 8), float("nan"), dtype=torch.float32, device="cuda:0")
    pix = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    steps = torch.full((n, 2), -1, dtype=torch.int32, device="cuda:0")
    pix2 = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    res3 = torch.full((n, 8), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rays.copy_(torch.from_numpy(G.pack_rays(o, d, rg)), non_blocking=False)
    filled = torch.cuda.Event()
    filled.record(torch.cuda.current_stream())
    dev.wait_event(filled.cuda_event)
    # without the flag the rays' spare words are ignored
    assert ter.shade_rays_device(rays.data_ptr(), n, res.data_ptr(), pix.data_ptr(), steps.data_ptr(), eye=RF.eye("G"))
    assert ter.shade_rays_device(rays.data_ptr(), n, 0, pix2.data_ptr(), eye=RF.eye("G"))  # the pixels alone
    assert ter.shade_rays_device(rays.data_ptr(), n, res3.data_ptr(), ray_range=True, eye=RF.eye("G"))
    done = torch.cuda.Event()
    done.record()  # torch creates its events on first record; the device then re-records it on its stream
    dev.record_event(done.cuda_event)
    torch.cuda.current_stream().wait_event(done)
    _same((res.cpu().numpy(), pix.cpu().numpy().view(np.uint32), steps.cpu().numpy().view(np.uint32)), host)
    assert np.array_equal(pix2.cpu().numpy().view(np.uint32), host[1])
    assert np.array_equal(res3.cpu().numpy().view(np.uint32), host_r[0].view(np.uint32))
    dev.check()
    dev.destroy()


def test_errors():
    import torch
    import gpgpuraytrace_amd as G
    from gpgpuraytrace_amd import _native
    L = G.lib()
    o, d = RF.query(("G",))
    res, px, st = np.zeros((1024, 8), np.float32), np.zeros(1024, np.uint32), np.zeros((1024, 2), np.uint32)
    dev, ter = _make()
    cs = ter.compute._h
    op, dp, rp, pp, sp = o.ctypes.data, d.ctypes.data, res.ctypes.data, px.ctypes.data, st.ctypes.data

    def host(n=8, opt=None, cs_=cs, o_=op, d_=dp, r_=rp, p_=pp):
        return L.rt_terrain_shade_rays(cs_, o_, d_, None, n, C.byref(opt) if opt is not None else None, r_, p_, sp)

    drays = torch.from_numpy(G.pack_rays(o[:8], d[:8])).to("cuda:0")
    dres = torch.zeros((8, 8), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    DR, DO = drays.data_ptr(), dres.data_ptr()

    def devf(n=8, opt=None, cs_=cs, rays=DR, r_=DO, p_=None):
        return L.rt_terrain_shade_rays_device(cs_, rays, n, C.byref(opt) if opt is not None else None, r_, p_, None)

    assert host() == RT_OK and devf() == RT_OK  # opt NULL
    dev.synchronize()
    assert np.array_equal(dres.cpu().numpy().view(np.uint32), res[:8].view(np.uint32))
    for f in (host, devf):
        # a camerarays compute has no SunDirection
        assert f(cs_=ter.camera_compute._h) == RT_ERR_INVALID and b"camerarays" in L.rt_last_error()
        # there is no segment shape
        assert f(opt=G.engine.surface_options(None, "segments", 0)) == RT_ERR_UNSUPPORTED and b"segment" in L.rt_last_error()
        assert f(opt=G.engine.surface_options(None, "lanes", 0)) == RT_OK
        # neither output
        assert f(r_=None, p_=None) == RT_ERR_INVALID and b"both null" in L.rt_last_error()
        # the option block and the count: as the surface queries
        assert f(n=-1) == RT_ERR_INVALID and b"2^26" in L.rt_last_error()
        assert f(n=(1 << 26) + 1) == RT_ERR_INVALID
        for size in (8, 24, 39):
            short = G.engine.surface_options()
            short.size = size
            assert f(opt=short) == RT_ERR_INVALID and b"size" in L.rt_last_error()
        both = G.engine.surface_options()
        both.flags = _native.RT_RAYS_FORCE_SEGMENTS | _native.RT_RAYS_FORCE_LANES
        assert f(opt=both) == RT_ERR_INVALID
        assert f(opt=G.engine.surface_options(stepmod=-1.0)) == RT_ERR_INVALID and b"stepmod" in L.rt_last_error()
        assert f(opt=G.engine.surface_options(t_min=10.0, t_max=9.0)) == RT_ERR_INVALID and b"t_max" in L.rt_last_error()
    assert host(o_=None) == RT_ERR_INVALID and host(d_=None) == RT_ERR_INVALID and devf(rays=None) == RT_ERR_INVALID
    # no texture bound: RT_ERR_STATE, as the other queries
    bare = dev.create_compute()
    assert bare.create("shaders", "tracescreen.hlsl", "CSMain", (16, 16, 1)) and bare.swap()
    assert host(cs_=bare._h) == RT_ERR_STATE and b"texPerm2D" in L.rt_last_error()
    assert devf(cs_=bare._h) == RT_ERR_STATE
    with pytest.raises(ValueError):
        ter.shade_rays(o, d[:5])
    with pytest.raises(ValueError):
        ter.shade_rays(o, d, ranges=np.zeros((5, 2), np.float32))
    dev.check()
    dev.destroy()


# --- the frame loop is undisturbed --------------------------------------------------------------
def _pose(ter, consts):
    ter.set_camera(FixedCamera(consts))
    ter.update_terrain()
    ter.set_time_of_day_vec(consts["sun"])


def _golden_pair():
    gold = GI.load()
    specs = [GI.FRAMES[0], GI.FRAMES[1]]
    land, _, w, h, aa, ms, ao = GI.unpack(specs[0])
    cams = [GI.consts(w, h, GI.unpack(s)[1]) for s in specs]
    return land, cams, [gold[GI.frame_key(*s) + "_rgba8"] for s in specs]


_want = {}


def _query(ter, sun, k):
    """G's rays with an explicit eye under the terrain's current sun (the pose's): the checker's bits."""
    o, d = RF.query(("G",))
    key = tuple(float(v) for v in np.asarray(sun, np.float32)[:3])
    if key not in _want:
        _want[key] = SH.shade(o, d, RF.eye("G"), "nomadplains", sun=key)
    got = ter.shade_rays(o, d, eye=RF.eye("G"), rgba8=True, steps=True)
    assert got is not None
    _same(got, _want[key], k)


def test_plain_serial_loop_is_undisturbed():
    """Six renders on a plain device, the camera alternating between two golden poses, a query after each: as
    many renders prepassed on the prepass stream as without queries, every frame golden."""
    land, cams, frames = _golden_pair()
    n = 6

    def loop(queries):
        dev, ter = make(cams[0], land, float_output=False)
        ring = dev.readback_ring("rgba8", depth=3)
        for k in range(n):
            _pose(ter, cams[k % 2])
            ter.render_device()
            t = ring.submit()
            if queries:
                _query(ter, cams[k % 2]["sun"], k)
            assert np.array_equal(ring.wait(t), frames[k % 2]), k
            ring.release(t)
        count = dev.prestream_renders()
        dev.check()
        ring.destroy()
        dev.destroy()
        return count

    assert loop(True) == loop(False) == n - 1


def test_deferred_loop_is_undisturbed():
    """A deferred device at one frame to a launch: a query between two renders launches no pending frame (the
    same deferred_fused and launch_info as without), and the frames are golden."""
    land, cams, frames = _golden_pair()
    n = 6

    def loop(queries):
        dev, ter = make(cams[0], land, float_output=False, **DEFER)
        dev.defer_batch(1)
        ring = dev.readback_ring("rgba8", depth=3)
        tickets = []
        for k in range(n):
            _pose(ter, cams[k % 2])
            ter.render_device()
            tickets.append(ring.submit())
            before = (dev.deferred_fused(), dev.launch_info())
            if queries:
                _query(ter, cams[k % 2]["sun"], k)
                assert (dev.deferred_fused(), dev.launch_info()) == before, k
            if k >= 2:
                assert np.array_equal(ring.wait(tickets[k - 2]), frames[k % 2]), k
                ring.release(tickets[k - 2])
        info = (dev.deferred_fused(), dev.launch_info())
        for k in (n - 2, n - 1):
            assert np.array_equal(ring.wait(tickets[k]), frames[k % 2]), k
            ring.release(tickets[k])
        dev.check()
        ring.destroy()
        dev.destroy()
        return info

    with_q, without = loop(True), loop(False)
    assert with_q == without and with_q[0] == n - 1


def test_graph_device_captures_nothing_again():
    land, cams, frames = _golden_pair()

    def loop(queries):
        dev, ter = make(cams[0], land, float_output=False, graph=True)
        for k in range(3):
            ter.render_device()
            if queries:
                _query(ter, cams[0]["sun"], k)
            assert np.array_equal(dev.readback(), frames[0]), k
        info = dev.graph_info()
        dev.check()
        dev.destroy()
        return info

    assert loop(True) == loop(False)
