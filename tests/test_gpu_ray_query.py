"""GPU tests of the ray queries (rt_terrain_trace_rays / _device, ABI 9 additive): caller-supplied rays marched as
camerarays.hlsl:12-21 marches its pixel rays.  Bar: results and step counts equal the oracle's prepass of the
exact fixture cameras (tests/ray_fixture.py) bit for bit, in both kernel shapes, at every size and grid, and a
query between two renders changes nothing about the frame loop."""
import ctypes as C

import numpy as np
import pytest

import golden_index as GI
import ray_fixture as RF
from test_gpu_parity import FixedCamera, make

pytestmark = pytest.mark.gpu

RT_OK, RT_ERR_INVALID, RT_ERR_UNSUPPORTED, RT_ERR_STATE = 0, -1, -4, -5
DEFER = dict(deferred=True, debug_defer_small=True)  # as test_gpu_deferred.py: the one-frame deferral on small frames
F_EYE = RF.eye("F0")


def _make(land="nomadplains", consts=None, **kw):
    """A 64x48 device and its terrain (the camera is the golden reset pose: Eye = F's eye)."""
    return make(consts or GI.consts(64, 48, "reset"), land, float_output=False, **kw)


def _same(got, want, what=""):
    res, steps = got
    wres, wsteps = want
    assert res.shape == wres.shape and res.dtype == np.float32 and steps.dtype == np.uint32
    bad = np.flatnonzero((res.view(np.uint32) != wres.view(np.uint32)).any(axis=1))
    assert bad.size == 0, (what, bad[:8], res[bad[:4]], wres[bad[:4]])
    assert np.array_equal(steps, wsteps), what


MODES = [(land, mode) for land in RF.LANDSCAPES for mode in ("auto", "lanes")] + [("nomadplains", "segments")]


@pytest.mark.parametrize("land,mode", MODES, ids=["%s-%s" % m for m in MODES])
def test_parity_with_the_oracle(land, mode):
    """The F0-F3 query (n = 4096, one eye) and G (n = 1024, origin != eye): results and steps equal the oracle's."""
    import gpgpuraytrace_amd as G
    dev, ter = _make(land)
    for names in (RF.F_SET, ("G",)):
        o, d = RF.query(names)
        got = ter.trace_rays(o, d, eye=RF.eye(names[0]), steps=True, mode=mode)
        assert got is not None, G.lib().rt_last_error()
        _same(got, RF.oracle_query(names, land), names)
        res = ter.trace_rays(o, d, eye=RF.eye(names[0]), mode=mode)  # the kernels without the step counts
        assert np.array_equal(res.view(np.uint32), got[0].view(np.uint32))
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("max_blocks", [1, 2])
@pytest.mark.parametrize("land", ["nomadplains", "greenrocks"])
def test_refill(land, max_blocks):
    """Forced lanes on a grid of 1 or 2 blocks, n = 4096 + 37: the F0-F3 rays under a seeded permutation (long
    and short rays interleave) and the first 37 again (a partial last wave).  One block has 1024 lanes, so every
    lane refills about four times; the bits are the oracle's after un-permuting."""
    o, d = RF.query(RF.F_SET)
    perm = np.random.default_rng(4133).permutation(4096)
    idx = np.concatenate([perm, perm[:37]])
    dev, ter = _make(land)
    got = ter.trace_rays(o[idx], d[idx], eye=F_EYE, steps=True, mode="lanes", max_blocks=max_blocks)
    assert got is not None
    wres, wsteps = RF.oracle_query(RF.F_SET, land)
    _same(got, (wres[idx], wsteps[idx]))
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("mode", ["lanes", "segments"])
def test_sizes(mode):
    """n = 1, 63, 64, 65 and 1025 from the head of the F0-F3 set (partial waves, one wave, one more ray, one more
    block), and n = 0, which launches nothing."""
    import gpgpuraytrace_amd as G
    o, d = RF.query(RF.F_SET)
    wres, wsteps = RF.oracle_query(RF.F_SET, "nomadplains")
    dev, ter = _make()
    for n in (1, 63, 64, 65, 1025):
        got = ter.trace_rays(o[:n], d[:n], eye=F_EYE, steps=True, mode=mode)
        assert got is not None, n
        _same(got, (wres[:n], wsteps[:n]), n)
    got = ter.trace_rays(o[:0], d[:0], eye=F_EYE, steps=True, mode=mode)
    assert got is not None and got[0].shape == (0, 4) and got[1].shape == (0,)
    opt = G.engine.ray_options(None, mode, 0)
    assert G.lib().rt_terrain_trace_rays(ter.camera_compute._h, None, None, 0, C.byref(opt), None, None) == RT_OK
    assert G.lib().rt_terrain_trace_rays_device(ter.camera_compute._h, None, 0, C.byref(opt), None, None) == RT_OK
    dev.destroy()


@pytest.mark.parametrize("mode", ["lanes", "segments"])
def test_eye(mode):
    """The LOD eye: the compute's Eye variable by default, the option's otherwise; live on nomadplains."""
    o, d = RF.query(("G",))
    want = RF.oracle("G", "nomadplains")
    dev, ter = _make()
    explicit = ter.trace_rays(o, d, eye=RF.eye("G"), steps=True, mode=mode)  # (the compute's Eye is F's)
    _same(explicit, want)
    other = ter.trace_rays(o, d, eye=F_EYE, steps=True, mode=mode)
    assert not np.array_equal(other[0].view(np.uint32), want[0].view(np.uint32))
    default_f = ter.trace_rays(o, d, steps=True, mode=mode)  # eye=None: the compute's, F's
    _same(default_f, other)
    ter.set_camera(FixedCamera(RF.consts("G")))
    ter.update_terrain()  # writes the Eye variables
    _same(ter.trace_rays(o, d, steps=True, mode=mode), want)
    # the tracescreen compute serves as well (the C-ABI accepts either kind)
    import gpgpuraytrace_amd as G
    res = np.empty((1024, 4), np.float32)
    st = np.empty(1024, np.uint32)
    opt = G.engine.ray_options(None, mode, 0)
    assert G.lib().rt_terrain_trace_rays(ter.compute._h, o.ctypes.data, d.ctypes.data, 1024, C.byref(opt),
                                         res.ctypes.data, st.ctypes.data) == RT_OK
    _same((res, st), want)
    dev.destroy()


@pytest.mark.parametrize("land", RF.LANDSCAPES)
def test_zero_direction(land):
    o, d = RF.query(("Z",))
    assert not d.any()
    dev, ter = _make(land)
    for mode in ("lanes", "segments") if land == "nomadplains" else ("auto",):
        _same(ter.trace_rays(o, d, eye=RF.eye("Z"), steps=True, mode=mode), RF.oracle("Z", land), mode)
    # zero directions among live rays (a refilled lane whose ray ends before its first step)
    fo, fd = RF.query(("G",))
    mo, md = np.concatenate([o[:100], fo[:200], o[:30]]), np.concatenate([d[:100], fd[:200], d[:30]])
    wres, wsteps = RF.oracle("G", land)
    zres, zsteps = RF.oracle("Z", land)
    want = (np.concatenate([zres[:100], wres[:200], zres[:30]]), np.concatenate([zsteps[:100], wsteps[:200], zsteps[:30]]))
    _same(ter.trace_rays(mo, md, eye=RF.eye("G"), steps=True, mode="lanes", max_blocks=1), want)
    dev.destroy()


@pytest.mark.parametrize("mode", ["lanes", "segments"])
def test_device_form_equals_host_form(mode):
    """torch-allocated rays, results and steps; the rays are filled on torch's stream and handed over by event,
    the results handed back by event: no host synchronisation in between.  The result buffers start poisoned."""
    import torch
    import gpgpuraytrace_amd as G
    o, d = RF.query(("G", "F2"))
    n = len(o)
    dev, ter = _make()
    host = ter.trace_rays(o, d, eye=RF.eye("G"), steps=True, mode=mode)
    rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda:0")
    res = torch.full((n, 4), float("nan"), dtype=torch.float32, device="cuda:0")
    steps = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    res2 = torch.full((n, 4), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rays.copy_(torch.from_numpy(G.pack_rays(o, d)), non_blocking=False)
    filled = torch.cuda.Event()
    filled.record(torch.cuda.current_stream())
    dev.wait_event(filled.cuda_event)
    assert ter.trace_rays_device(rays.data_ptr(), n, res.data_ptr(), steps.data_ptr(), eye=RF.eye("G"), mode=mode)
    assert ter.trace_rays_device(rays.data_ptr(), n, res2.data_ptr(), eye=RF.eye("G"), mode=mode)  # no steps
    done = torch.cuda.Event()
    done.record()  # torch creates its events on first record; the device then re-records it on its stream
    dev.record_event(done.cuda_event)
    torch.cuda.current_stream().wait_event(done)
    got = (res.cpu().numpy(), steps.cpu().numpy().view(np.uint32))
    _same(got, host)
    assert np.array_equal(res2.cpu().numpy().view(np.uint32), host[0].view(np.uint32))
    _same((host[0][:1024], host[1][:1024]), RF.oracle("G", "nomadplains"))  # (F2's rays with G's eye: no oracle)
    dev.check()
    dev.destroy()


def test_arguments():
    import gpgpuraytrace_amd as G
    from gpgpuraytrace_amd import _native
    L = G.lib()
    o, d = RF.query(("G",))
    res, st = np.zeros((1024, 4), np.float32), np.zeros(1024, np.uint32)
    dev, ter = _make()
    cs = ter.camera_compute._h
    op, dp, rp, sp = o.ctypes.data, d.ctypes.data, res.ctypes.data, st.ctypes.data

    def host(n=8, opt=None, o_=op, d_=dp, r_=rp):
        return L.rt_terrain_trace_rays(cs, o_, d_, n, C.byref(opt) if opt is not None else None, r_, sp)

    import torch
    drays = torch.from_numpy(G.pack_rays(o[:8], d[:8])).to("cuda:0")
    dres = torch.zeros((8, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    DR, DO = drays.data_ptr(), dres.data_ptr()

    def devf(n=8, opt=None, rays=DR, r_=DO):
        return L.rt_terrain_trace_rays_device(cs, rays, n, C.byref(opt) if opt is not None else None, r_, None)

    assert host() == RT_OK and devf() == RT_OK  # opt NULL
    dev.synchronize()
    assert np.array_equal(dres.cpu().numpy().view(np.uint32), res[:8].view(np.uint32))
    for f in (host, devf):
        assert f(n=-1) == RT_ERR_INVALID and b"2^26" in L.rt_last_error()
        assert f(n=(1 << 26) + 1) == RT_ERR_INVALID
        short = G.engine.ray_options()
        short.size = 8
        assert f(opt=short) == RT_ERR_INVALID and b"size" in L.rt_last_error()
        both = G.engine.ray_options()
        both.flags = _native.RT_RAYS_FORCE_SEGMENTS | _native.RT_RAYS_FORCE_LANES
        assert f(opt=both) == RT_ERR_INVALID
    assert host(o_=None) == RT_ERR_INVALID and host(d_=None) == RT_ERR_INVALID and host(r_=None) == RT_ERR_INVALID
    assert devf(rays=None) == RT_ERR_INVALID and devf(r_=None) == RT_ERR_INVALID
    later = (C.c_uint32 * 16)()  # a later, longer version of the options: its first fields mean the same
    later[0], later[1] = 64, _native.RT_RAYS_FORCE_LANES
    assert L.rt_terrain_trace_rays(cs, op, dp, 8, C.cast(later, C.POINTER(_native.RtRayOptions)), rp, sp) == RT_OK
    # no texture bound: RT_ERR_STATE, as rt_debug_noise
    bare = dev.create_compute()
    assert bare.create("shaders", "camerarays.hlsl", "CSMain", (16, 16, 1)) and bare.swap()
    assert L.rt_terrain_trace_rays(bare._h, op, dp, 8, None, rp, sp) == RT_ERR_STATE and b"texPerm2D" in L.rt_last_error()
    assert L.rt_terrain_trace_rays_device(bare._h, DR, 8, None, DO, None) == RT_ERR_STATE
    dev.destroy()
    # the segment shape exists for nomadplains only
    dev, ter = _make("testing")
    seg = G.engine.ray_options(None, "segments", 0)
    assert L.rt_terrain_trace_rays(ter.camera_compute._h, op, dp, 8, C.byref(seg), rp, sp) == RT_ERR_UNSUPPORTED
    assert L.rt_terrain_trace_rays_device(ter.camera_compute._h, DR, 8, C.byref(seg), DO, None) == RT_ERR_UNSUPPORTED
    assert ter.trace_rays(o, d, mode="segments") is None  # the mirror: None, no exception
    assert ter.trace_rays_device(DR, 8, DO, mode="segments") is False
    with pytest.raises(ValueError):
        ter.trace_rays(o, d[:5])
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
    """G's rays with an explicit eye, the shapes alternating; the oracle's bits."""
    o, d = RF.query(("G",))
    got = ter.trace_rays(o, d, eye=RF.eye("G"), steps=True, mode=("segments", "lanes")[k % 2])
    _same(got, RF.oracle("G", "nomadplains"), k)


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
                _query(ter, k)  # (blocks on the device stream; launches and reconfigures nothing of the loop)
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
        dev.destroy()
        return info

    assert loop(True) == loop(False)


@pytest.mark.parametrize("name", ["F0", "G"])
def test_query_reproduces_the_devices_own_prepass(name):
    """A 256x256 nomadplains frame of a fixture camera with the camera feed: the prepass is deterministic and its
    rays are known exactly, so a query of them reproduces its CameraResults (and the oracle's) in both shapes."""
    consts = RF.consts(name)
    dev, ter = make(consts, "nomadplains", float_output=False)
    ter.render_device(feed=True)
    feed = np.array(ter.camera_feed())
    assert np.array_equal(feed.view(np.uint32), RF.oracle(name, "nomadplains")[0].view(np.uint32))
    o, d = RF.rays(name)
    for mode in ("auto", "lanes", "segments"):
        res = ter.trace_rays(o, d, mode=mode)  # eye=None: the camera's
        assert np.array_equal(res.view(np.uint32), feed.view(np.uint32)), mode
    dev.check()
    dev.destroy()
