"""GPU tests of the surface queries (rt_terrain_trace_surface / _device, ABI 9 additive): caller-supplied rays
marched as tracescreen marches its pixels' (traceRay with skiprefine off) with getNormal at each hit.  Bar: all 8
result floats and the step counts equal the checker's (tests/surface_ref.py: the oracle's own trace_ray and
get_normal) bit for bit, in both kernel shapes, at every size, grid and option, and a query between two renders
changes nothing about the frame loop."""
import ctypes as C

import numpy as np
import pytest

import golden_index as GI
import ray_fixture as RF
import surface_ref as SR
from test_gpu_parity import FixedCamera, make

pytestmark = pytest.mark.gpu

RT_OK, RT_ERR_INVALID, RT_ERR_UNSUPPORTED, RT_ERR_STATE = 0, -1, -4, -5
DEFER = dict(deferred=True, debug_defer_small=True)
F_EYE = RF.eye("F0")
SHAPES = ["lanes", "segments"]


def _make(land="nomadplains", consts=None, **kw):
    """A 64x48 device and its terrain (the camera is the golden reset pose: Eye = F's eye)."""
    return make(consts or GI.consts(64, 48, "reset"), land, float_output=False, **kw)


def _same(got, want, what=""):
    res, steps = got
    wres, wsteps = want
    assert res.shape == wres.shape and res.shape[1:] == (8,) and res.dtype == np.float32 and steps.dtype == np.uint32
    bad = np.flatnonzero((res.view(np.uint32) != wres.view(np.uint32)).any(axis=1))
    assert bad.size == 0, (what, bad.size, bad[:8], res[bad[:4]], wres[bad[:4]])
    assert np.array_equal(steps, wsteps), what


MODES = [(land, mode) for land in RF.LANDSCAPES for mode in ("auto", "lanes")] + [("nomadplains", "segments")]


@pytest.mark.parametrize("land,mode", MODES, ids=["%s-%s" % m for m in MODES])
def test_parity_with_the_checker(land, mode):
    """The F0-F3 query (n = 4096, one eye) and G (n = 1024, origin != eye) with the defaults."""
    import gpgpuraytrace_amd as G
    dev, ter = _make(land)
    for names in (RF.F_SET, ("G",)):
        o, d = RF.query(names)
        got = ter.trace_surface(o, d, eye=RF.eye(names[0]), steps=True, mode=mode)
        assert got is not None, G.lib().rt_last_error()
        _same(got, SR.query(names, land), names)
        res = ter.trace_surface(o, d, eye=RF.eye(names[0]), mode=mode)  # the kernels without the step counts
        assert np.array_equal(res.view(np.uint32), got[0].view(np.uint32))
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("max_blocks", [1, 2])
@pytest.mark.parametrize("land", ["nomadplains", "greenrocks"])
def test_refill(land, max_blocks):
    """Forced lanes on a grid of 1 or 2 blocks, n = 4096 + 37 under test_gpu_ray_query's seeded permutation: a
    one-block grid refills every lane about four times, and ended lanes compute normals while others march."""
    o, d = RF.query(RF.F_SET)
    perm = np.random.default_rng(4133).permutation(4096)
    idx = np.concatenate([perm, perm[:37]])
    dev, ter = _make(land)
    got = ter.trace_surface(o[idx], d[idx], eye=F_EYE, steps=True, mode="lanes", max_blocks=max_blocks)
    assert got is not None
    wres, wsteps = SR.query(RF.F_SET, land)
    _same(got, (wres[idx], wsteps[idx]))
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("mode", SHAPES)
def test_sizes(mode):
    """n = 1, 63, 64, 65 and 1025 from the head of the F0-F3 set, and n = 0, which launches nothing."""
    import gpgpuraytrace_amd as G
    o, d = RF.query(RF.F_SET)
    wres, wsteps = SR.query(RF.F_SET, "nomadplains")
    dev, ter = _make()
    for n in (1, 63, 64, 65, 1025):
        got = ter.trace_surface(o[:n], d[:n], eye=F_EYE, steps=True, mode=mode)
        assert got is not None, n
        _same(got, (wres[:n], wsteps[:n]), n)
    got = ter.trace_surface(o[:0], d[:0], eye=F_EYE, steps=True, mode=mode)
    assert got is not None and got[0].shape == (0, 8) and got[1].shape == (0,)
    opt = G.engine.surface_options(None, mode, 0)
    assert G.lib().rt_terrain_trace_surface(ter.camera_compute._h, None, None, None, 0, C.byref(opt), None, None) == RT_OK
    assert G.lib().rt_terrain_trace_surface_device(ter.camera_compute._h, None, 0, C.byref(opt), None, None) == RT_OK
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("mode", SHAPES)
def test_options(mode):
    """The seeded per-ray ranges, per-call params (t_min 0.5, t_max 100, stepmod 2) and max_steps = 64."""
    o, d = RF.query(RF.F_SET)
    dev, ter = _make()
    rg = SR.seeded_ranges()
    _same(ter.trace_surface(o, d, ranges=rg, eye=F_EYE, steps=True, mode=mode),
          SR.query(RF.F_SET, "nomadplains", ranged=True), "ranges")
    res = ter.trace_surface(o, d, ranges=rg, eye=F_EYE, mode=mode)  # (the RANGE kernels without the step counts)
    assert np.array_equal(res.view(np.uint32), SR.query(RF.F_SET, "nomadplains", ranged=True)[0].view(np.uint32))
    _same(ter.trace_surface(o, d, eye=F_EYE, t_min=0.5, t_max=100.0, stepmod=2.0, steps=True, mode=mode),
          SR.query(RF.F_SET, "nomadplains", t_min=0.5, t_max=100.0, stepmod=2.0), "params")
    _same(ter.trace_surface(o, d, eye=F_EYE, max_steps=64, steps=True, mode=mode),
          SR.query(RF.F_SET, "nomadplains", max_steps=64), "max_steps")
    # the ranges override the per-call range, the other params hold beside them
    _same(ter.trace_surface(o, d, ranges=rg, eye=F_EYE, t_min=7.0, t_max=8.0, max_steps=64, steps=True, mode=mode),
          SR.query(RF.F_SET, "nomadplains", ranged=True, max_steps=64), "ranges + max_steps")
    dev.check()
    dev.destroy()


def test_options_on_another_landscape():
    o, d = RF.query(RF.F_SET)
    dev, ter = _make("greenrocks")
    _same(ter.trace_surface(o, d, ranges=SR.seeded_ranges(), eye=F_EYE, stepmod=2.0, steps=True),
          SR.query(RF.F_SET, "greenrocks", ranged=True, stepmod=2.0))
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("mode", SHAPES)
def test_eye(mode):
    """The eye (the density's level of detail and getNormal's eps): the option's, else the compute's Eye."""
    o, d = RF.query(("G",))
    want = SR.query(("G",), "nomadplains")
    want_f = SR.query(("G",), "nomadplains", eye="F0")
    assert not np.array_equal(want[0].view(np.uint32), want_f[0].view(np.uint32))
    dev, ter = _make()
    _same(ter.trace_surface(o, d, eye=RF.eye("G"), steps=True, mode=mode), want)  # (the compute's Eye is F's)
    _same(ter.trace_surface(o, d, eye=F_EYE, steps=True, mode=mode), want_f)
    _same(ter.trace_surface(o, d, steps=True, mode=mode), want_f)  # eye=None: the compute's, F's
    ter.set_camera(FixedCamera(RF.consts("G")))
    ter.update_terrain()  # writes the Eye variables
    _same(ter.trace_surface(o, d, steps=True, mode=mode), want)
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("mode", SHAPES)
def test_recording_constants(mode):
    """A compute created with RECORDING: the march's step and density factors are the recording ones."""
    o, d = RF.query(("G",))
    want = SR.query(("G",), "nomadplains", recording=1)
    assert not np.array_equal(want[1], SR.query(("G",), "nomadplains")[1])
    dev, ter = _make(recording=True)
    _same(ter.trace_surface(o, d, eye=RF.eye("G"), steps=True, mode=mode), want)
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("land", RF.LANDSCAPES)
def test_zero_direction(land):
    o, d = RF.query(("Z",))
    assert not d.any()
    dev, ter = _make(land)
    zres, zsteps = SR.query(("Z",), land)
    assert not zsteps.any() and not zres[:, 7].any()
    for mode in SHAPES if land == "nomadplains" else ("auto",):
        _same(ter.trace_surface(o, d, eye=RF.eye("Z"), steps=True, mode=mode), (zres, zsteps), mode)
    # zero directions among live rays (a refilled lane whose ray ends before its first step)
    fo, fd = RF.query(("G",))
    mo, md = np.concatenate([o[:100], fo[:200], o[:30]]), np.concatenate([d[:100], fd[:200], d[:30]])
    wres, wsteps = SR.query(("G",), land)
    want = (np.concatenate([zres[:100], wres[:200], zres[:30]]), np.concatenate([zsteps[:100], wsteps[:200], zsteps[:30]]))
    _same(ter.trace_surface(mo, md, eye=RF.eye("G"), steps=True, mode="lanes", max_blocks=1), want)
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("mode", SHAPES)
def test_device_form_equals_host_form(mode):
    """torch-allocated rays, results and steps; the rays are filled on torch's stream and handed over by event,
    the results handed back by event: no host synchronisation in between.  The result buffers start poisoned."""
    import torch
    import gpgpuraytrace_amd as G
    o, d = RF.query(("G", "F2"))
    n = len(o)
    rg = SR.seeded_ranges(n)
    dev, ter = _make()
    host = ter.trace_surface(o, d, eye=RF.eye("G"), steps=True, mode=mode)
    host_r = ter.trace_surface(o, d, ranges=rg, eye=RF.eye("G"), steps=True, mode=mode)
    assert not np.array_equal(host[0].view(np.uint32), host_r[0].view(np.uint32))
    rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda:0")
    res = torch.full((n, 8), float("nan"), dtype=torch.float32, device="cuda:0")
    steps = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    res2 = torch.full((n, 8), float("nan"), dtype=torch.float32, device="cuda:0")
    res3 = torch.full((n, 8), float("nan"), dtype=torch.float32, device="cuda:0")
    steps3 = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    rays.copy_(torch.from_numpy(G.pack_rays(o, d, rg)), non_blocking=False)
    filled = torch.cuda.Event()
    filled.record(torch.cuda.current_stream())
    dev.wait_event(filled.cuda_event)
    # without the flag the rays' spare words are ignored
    assert ter.trace_surface_device(rays.data_ptr(), n, res.data_ptr(), steps.data_ptr(), eye=RF.eye("G"), mode=mode)
    assert ter.trace_surface_device(rays.data_ptr(), n, res2.data_ptr(), eye=RF.eye("G"), mode=mode)  # no steps
    assert ter.trace_surface_device(rays.data_ptr(), n, res3.data_ptr(), steps3.data_ptr(), ray_range=True,
                                    eye=RF.eye("G"), mode=mode)
    done = torch.cuda.Event()
    done.record()  # torch creates its events on first record; the device then re-records it on its stream
    dev.record_event(done.cuda_event)
    torch.cuda.current_stream().wait_event(done)
    _same((res.cpu().numpy(), steps.cpu().numpy().view(np.uint32)), host)
    assert np.array_equal(res2.cpu().numpy().view(np.uint32), host[0].view(np.uint32))
    _same((res3.cpu().numpy(), steps3.cpu().numpy().view(np.uint32)), host_r)
    _same((host[0][:1024], host[1][:1024]), SR.query(("G",), "nomadplains"))  # (F2's rays with G's eye: no checker run)
    dev.check()
    dev.destroy()


def test_arguments():
    import torch
    import gpgpuraytrace_amd as G
    from gpgpuraytrace_amd import _native
    L = G.lib()
    o, d = RF.query(("G",))
    res, st = np.zeros((1024, 8), np.float32), np.zeros(1024, np.uint32)
    dev, ter = _make()
    cs = ter.camera_compute._h
    op, dp, rp, sp = o.ctypes.data, d.ctypes.data, res.ctypes.data, st.ctypes.data

    def host(n=8, opt=None, o_=op, d_=dp, r_=rp):
        return L.rt_terrain_trace_surface(cs, o_, d_, None, n, C.byref(opt) if opt is not None else None, r_, sp)

    drays = torch.from_numpy(G.pack_rays(o[:8], d[:8])).to("cuda:0")
    dres = torch.zeros((8, 8), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    DR, DO = drays.data_ptr(), dres.data_ptr()

    def devf(n=8, opt=None, rays=DR, r_=DO):
        return L.rt_terrain_trace_surface_device(cs, rays, n, C.byref(opt) if opt is not None else None, r_, None)

    assert host() == RT_OK and devf() == RT_OK  # opt NULL
    dev.synchronize()
    assert np.array_equal(dres.cpu().numpy().view(np.uint32), res[:8].view(np.uint32))
    for f in (host, devf):
        assert f(n=-1) == RT_ERR_INVALID and b"2^26" in L.rt_last_error()
        assert f(n=(1 << 26) + 1) == RT_ERR_INVALID
        for size in (8, 24, 39):  # (24: an rt_ray_options is no rt_surface_options)
            short = G.engine.surface_options()
            short.size = size
            assert f(opt=short) == RT_ERR_INVALID and b"size" in L.rt_last_error()
        both = G.engine.surface_options()
        both.flags = _native.RT_RAYS_FORCE_SEGMENTS | _native.RT_RAYS_FORCE_LANES
        assert f(opt=both) == RT_ERR_INVALID
        for sm in (0.0, -1.0, float("inf"), float("nan")):
            assert f(opt=G.engine.surface_options(stepmod=sm)) == RT_ERR_INVALID and b"stepmod" in L.rt_last_error()
        assert f(opt=G.engine.surface_options(t_min=10.0, t_max=9.0)) == RT_ERR_INVALID and b"t_max" in L.rt_last_error()
        assert f(opt=G.engine.surface_options(t_min=10.0, t_max=10.0)) == RT_OK
        ignored = G.engine.surface_options(stepmod=-1.0, t_min=10.0, t_max=9.0)
        ignored.flags &= ~_native.RT_SURFACE_PARAMS  # the trailing fields are read with the flag only
        assert f(opt=ignored) == RT_OK
    assert host(o_=None) == RT_ERR_INVALID and host(d_=None) == RT_ERR_INVALID and host(r_=None) == RT_ERR_INVALID
    assert devf(rays=None) == RT_ERR_INVALID and devf(r_=None) == RT_ERR_INVALID
    later = (C.c_uint32 * 16)()  # a later, longer version of the options: its first fields mean the same
    later[0], later[1] = 64, _native.RT_RAYS_FORCE_LANES
    assert L.rt_terrain_trace_surface(cs, op, dp, None, 8, C.cast(later, C.POINTER(_native.RtSurfaceOptions)), rp, sp) == RT_OK
    # no texture bound: RT_ERR_STATE, as rt_terrain_trace_rays
    bare = dev.create_compute()
    assert bare.create("shaders", "camerarays.hlsl", "CSMain", (16, 16, 1)) and bare.swap()
    assert L.rt_terrain_trace_surface(bare._h, op, dp, None, 8, None, rp, sp) == RT_ERR_STATE and b"texPerm2D" in L.rt_last_error()
    assert L.rt_terrain_trace_surface_device(bare._h, DR, 8, None, DO, None) == RT_ERR_STATE
    dev.check()
    dev.destroy()
    # the segment shape exists for nomadplains only
    dev, ter = _make("testing")
    seg = G.engine.surface_options(None, "segments", 0)
    assert L.rt_terrain_trace_surface(ter.camera_compute._h, op, dp, None, 8, C.byref(seg), rp, sp) == RT_ERR_UNSUPPORTED
    assert L.rt_terrain_trace_surface_device(ter.camera_compute._h, DR, 8, C.byref(seg), DO, None) == RT_ERR_UNSUPPORTED
    assert ter.trace_surface(o, d, mode="segments") is None  # the mirror: None, no exception
    assert ter.trace_surface_device(DR, 8, DO, mode="segments") is False
    with pytest.raises(ValueError):
        ter.trace_surface(o, d[:5])
    with pytest.raises(ValueError):
        ter.trace_surface(o, d, ranges=np.zeros((5, 2), np.float32))
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


def _query(ter, k):
    """G's rays with an explicit eye, the shapes alternating: the checker's bits, and a ray query after it the
    oracle's prepass bits as without a surface query."""
    o, d = RF.query(("G",))
    got = ter.trace_surface(o, d, eye=RF.eye("G"), steps=True, mode=SHAPES[k % 2])
    _same(got, SR.query(("G",), "nomadplains"), k)
    res, steps = ter.trace_rays(o, d, eye=RF.eye("G"), steps=True, mode=SHAPES[(k + 1) % 2])
    wres, wsteps = RF.oracle("G", "nomadplains")
    assert np.array_equal(res.view(np.uint32), wres.view(np.uint32)) and np.array_equal(steps, wsteps), k


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
                _query(ter, k)
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
                _query(ter, k)
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
                _query(ter, k)
            assert np.array_equal(dev.readback(), frames[0]), k
        info = dev.graph_info()
        dev.check()
        dev.destroy()
        return info

    assert loop(True) == loop(False)
