"""GPU tests of the asynchronous readback ring (rt_readback_*, ABI 9 additive) and the pipelined recorder
(rt_recorder_set_async): frames reach the host through a snapshot kernel, a copy stream and pinned slots, with no
host synchronisation per frame and, on an RT_DEVICE_DEFERRED device, without launching the pending frame.  Bar:
every captured frame equals the blocking readback / the golden frame bit for bit, and the counters of the
frames-in-flight paths (prestream_renders, deferred_fused, graph captures) equal those of the loop without a
ring."""
import ctypes as C

import numpy as np
import pytest

import golden_index as GI
import oracle_lib as O
from test_gpu_parity import FixedCamera, _consts_1080p_like, _hip, make

pytestmark = pytest.mark.gpu

DEFER = dict(deferred=True, debug_defer_small=True)  # as test_gpu_deferred.py: the one-frame deferral on small frames
RT_ERR_INVALID, RT_ERR_STATE = -1, -5


def _pose(ter, consts):
    ter.set_camera(FixedCamera(consts))
    ter.update_terrain()
    ter.set_time_of_day_vec(consts["sun"])


def _golden_pair():
    gold = GI.load()
    specs = [GI.FRAMES[0], GI.FRAMES[1]]
    land, _, w, h, aa, ms, ao = GI.unpack(specs[0])
    cams = [GI.consts(w, h, GI.unpack(s)[1]) for s in specs]
    frames = [gold[GI.frame_key(*s) + "_rgba8"] for s in specs]
    return land, w, h, cams, frames


def _device(kind):
    """(device, terrain) of one golden pair: "plain", "k1" (deferred, one frame to a launch), "k2", "k3"."""
    land, w, h, cams, _ = _golden_pair()
    if kind == "plain":
        return make(cams[0], land, float_output=False)
    dev, ter = make(cams[0], land, float_output=False, **DEFER)
    dev.defer_batch(int(kind[1:]))
    return dev, ter


def _submit_rc(ring):
    import gpgpuraytrace_amd as G
    t = C.c_ulonglong(12345)
    return G.lib().rt_readback_submit(ring._h, C.byref(t)), t.value


def _wait_rc(ring, ticket):
    import gpgpuraytrace_amd as G
    p = C.c_void_p(1)
    return G.lib().rt_readback_wait(ring._h, ticket, C.byref(p)), p.value


@pytest.mark.parametrize("size", [(64, 48), (50, 37), (1, 1)], ids=["64x48", "50x37-tail", "1x1"])
def test_snapshot_kernel_both_formats(size):
    """k_snapshot alone: the framebuffer filled with seeded random words, captured as RGBA8 (the blocking
    rt_device_readback's bytes) and as BGRX (RecorderWinAPI::write's conversion of them).  50x37 has 2 tail
    words behind its last 16-byte quad; 1x1 (the smallest device) is a tail only."""
    import gpgpuraytrace_amd as G
    w, h = size
    dev = G.DeviceFactory.construct(G.DeviceAPI.HIP, w, h)
    assert dev is not None, G.lib().rt_last_error()
    words = np.random.default_rng(w * 1000 + h).integers(0, 2 ** 32, w * h, dtype=np.uint64).astype(np.uint32)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(G.lib().rt_device_framebuffer(dev._h), words.ctypes.data, words.nbytes, 1) == 0
    want = dev.readback()
    assert np.array_equal(want.view(np.uint32).reshape(h, w), words.reshape(h, w))
    for fmt, ref in (("rgba8", want), ("bgrx", O.bgrx(want))):
        ring = dev.readback_ring(fmt, depth=2)
        for _ in range(3):  # (more captures than slots)
            t = ring.submit()
            got = ring.wait(t)
            assert got.shape == ref.shape and got.dtype == ref.dtype and not got.flags.writeable
            assert np.array_equal(got, ref), fmt
            ring.release(t)
        ring.destroy()
    dev.destroy()


def test_plain_serial_loop_keeps_frames_in_flight():
    """Seven frames on a plain device, the camera alternating between two golden poses, a submit after every
    render, ticket k-2 waited for and released inside the loop (depth 3).  Every ticket's frame is its pose's
    golden frame -- so a capture survives the next render overwriting the framebuffer -- and as many renders
    prepassed on the prepass stream as in the same loop without a ring."""
    land, w, h, cams, frames = _golden_pair()
    n = 7
    dev, ter = _device("plain")
    for k in range(n):
        _pose(ter, cams[k % 2])
        ter.render_device()
    control = dev.prestream_renders()
    dev.destroy()
    assert control == n - 1
    dev, ter = _device("plain")
    ring = dev.readback_ring("rgba8", depth=3)
    tickets, seen = [], 0

    def take(k):
        assert np.array_equal(ring.wait(tickets[k]), frames[k % 2]), k
        ring.release(tickets[k])

    for k in range(n):
        _pose(ter, cams[k % 2])
        ter.render_device()
        tickets.append(ring.submit())
        if k >= 2:
            take(k - 2)
            seen += 1
    assert tickets == list(range(n))
    assert dev.prestream_renders() == control
    for k in range(seen, n):
        take(k)
    dev.check()
    ring.destroy()
    dev.destroy()


def test_ring_semantics():
    """Full ring, release order, double wait, stale tickets, and a ready() that launches nothing."""
    import gpgpuraytrace_amd as G
    land, w, h, cams, frames = _golden_pair()
    dev, ter = _device("plain")
    ter.render_device()
    ring = dev.readback_ring("rgba8", depth=2)
    t0, t1 = ring.submit(), ring.submit()
    assert (t0, t1) == (0, 1)
    assert _submit_rc(ring) == (RT_ERR_STATE, 12345)  # full: no ticket, nothing queued
    assert _wait_rc(ring, t1)[0] == 0                 # out of order: the newer one first
    assert np.array_equal(ring.wait(t1), frames[0])   # waiting twice
    ring.release(t1)
    t2 = ring.submit()                                # one release: the next submit succeeds
    assert t2 == 2                                    # (the refused submit took no ticket)
    assert _submit_rc(ring)[0] == RT_ERR_STATE
    assert _wait_rc(ring, t1) == (RT_ERR_INVALID, None)  # released: stale
    assert G.lib().rt_readback_release(ring._h, t1) == RT_ERR_INVALID
    assert G.lib().rt_readback_ready(ring._h, t1) == RT_ERR_INVALID
    assert _wait_rc(ring, 99)[0] == RT_ERR_INVALID       # never issued
    assert G.lib().rt_readback_ready(ring._h, 99) == RT_ERR_INVALID
    for t in (t0, t2):
        assert np.array_equal(ring.wait(t), frames[0])
        ring.release(t)
    ring.destroy()
    dev.destroy()
    # ready() on a deferred device with a pending frame: 0, and no launch
    dev, ter = _device("k1")
    ring = dev.readback_ring("rgba8", depth=2)
    ter.render_device()
    t = ring.submit()
    before = (dev.deferred_fused(), dev.launch_info())
    for _ in range(3):
        assert ring.ready(t) is False
    assert G.lib().rt_readback_release(ring._h, t) == RT_ERR_STATE  # not the caller's yet: not releasable
    assert (dev.deferred_fused(), dev.launch_info()) == before
    _pose(ter, cams[1])
    ter.render_device()  # launches the pending frame with this one's prepass inside: still fused
    assert dev.deferred_fused() == before[0] + 1
    assert np.array_equal(ring.wait(t), frames[0])
    assert ring.ready(t) is True
    ring.release(t)
    ring.destroy()
    dev.destroy()


def test_deferred_k1_submit_does_not_end_the_deferral():
    """Seven frames on a deferred device at one frame to a launch, a submit after every render: the frames are
    golden, in order, and six of the seven prepasses ran fused.  The same loop with a blocking readback every
    frame -- the only per-frame consumer there was -- fuses none."""
    land, w, h, cams, frames = _golden_pair()
    n = 7
    dev, ter = _device("k1")
    ring = dev.readback_ring("rgba8", depth=3)
    tickets = []
    for k in range(n):
        _pose(ter, cams[k % 2])
        ter.render_device()
        tickets.append(ring.submit())
        if k >= 2:  # frame k-2's trace went out with render k-1: no launch here
            assert np.array_equal(ring.wait(tickets[k - 2]), frames[k % 2]), k
            ring.release(tickets[k - 2])
    assert dev.deferred_fused() == n - 1
    for k in (n - 2, n - 1):  # (the last one's wait launches the pending frame)
        assert np.array_equal(ring.wait(tickets[k]), frames[k % 2]), k
        ring.release(tickets[k])
    assert dev.deferred_fused() == n - 1 and dev.launch_info() == (0, 1)
    assert np.array_equal(dev.readback(), frames[(n - 1) % 2])
    dev.check()
    ring.destroy()
    dev.destroy()
    dev, ter = _device("k1")
    for k in range(n):
        _pose(ter, cams[k % 2])
        ter.render_device()
        assert np.array_equal(dev.readback(), frames[k % 2]), k
    assert dev.deferred_fused() == 0
    dev.destroy()


@pytest.mark.parametrize("every", [1, 2], ids=["every-frame", "every-other"])
@pytest.mark.parametrize("k", [2, 3])
def test_deferred_batch_captures_follow_their_frames(k, every):
    """k frames to a launch, seven frames, a capture of every (or every other) frame: each is attached to its
    frame's queue entry and queued behind the launch that traces it, from the frame slot or -- the flush's last
    frame -- the device's framebuffer.  Frames are golden; as many prepasses ran fused as without captures."""
    land, w, h, cams, frames = _golden_pair()
    n = 7
    dev, ter = _device("k%d" % k)
    for i in range(n):
        _pose(ter, cams[i % 2])
        ter.render_device()
    assert np.array_equal(dev.readback(), frames[(n - 1) % 2])
    control = dev.deferred_fused()
    dev.destroy()
    assert control == n - k
    dev, ter = _device("k%d" % k)
    ring = dev.readback_ring("rgba8", depth=8)
    tickets = {}
    for i in range(n):
        _pose(ter, cams[i % 2])
        ter.render_device()
        if i % every == 0:
            tickets[i] = ring.submit()
    for i, t in tickets.items():  # (the first wait on a frame still queued launches everything queued)
        assert np.array_equal(ring.wait(t), frames[i % 2]), i
        ring.release(t)
    assert dev.deferred_fused() == control
    assert np.array_equal(dev.readback(), frames[(n - 1) % 2])
    dev.check()
    ring.destroy()
    dev.destroy()


@pytest.mark.parametrize("kind", ["k1", "k2"])
def test_wait_launches_a_frame_not_yet_launched(kind):
    """Render, submit, wait at once: the capture's frame is still pending, so the wait launches it."""
    land, w, h, cams, frames = _golden_pair()
    dev, ter = _device(kind)
    ring = dev.readback_ring("bgrx", depth=1)
    for i in (1, 0):
        _pose(ter, cams[i])
        ter.render_device()
        t = ring.submit()
        assert np.array_equal(ring.wait(t), O.bgrx(frames[i])), i
        ring.release(t)
    ring.destroy()
    dev.destroy()


def test_real_deferral_size_matches_plain_readbacks():
    """1280x720 nomadplains, the smallest frame the product defers at one frame to a launch (no debug flag): four
    frames with a capture each equal the blocking readbacks of the same poses on a plain device."""
    w, h = 1280, 720
    cams = [_consts_1080p_like(w, h, p) for p in ("reset", "lookdown")]
    dev, ter = make(cams[0], max_steps=256, float_output=False)
    want = []
    for c in cams:
        _pose(ter, c)
        ter.render_device()
        want.append(dev.readback())
    dev.destroy()
    assert not np.array_equal(want[0], want[1])
    dev, ter = make(cams[0], max_steps=256, float_output=False, deferred=True)
    ring = dev.readback_ring("rgba8", depth=4)
    tickets = []
    for i in range(4):
        _pose(ter, cams[i % 2])
        ter.render_device()
        tickets.append(ring.submit())
    assert dev.deferred_fused() == 3
    for i, t in enumerate(tickets):
        assert np.array_equal(ring.wait(t), want[i % 2]), i
        ring.release(t)
    dev.check()
    ring.destroy()
    dev.destroy()


def test_graph_device_captures_nothing_again():
    """Three frames with a ring on an RT_DEVICE_GRAPH device: golden frames, and as many graph captures as the
    loop without a ring (the snapshot launches outside the captured graphs)."""
    land, w, h, cams, frames = _golden_pair()

    def loop(with_ring):
        dev, ter = make(cams[0], land, float_output=False, graph=True)
        ring = dev.readback_ring("rgba8", depth=3) if with_ring else None
        for _ in range(3):
            ter.render_device()
            if ring:
                ring.submit()
        if ring:
            for t in range(3):
                assert np.array_equal(ring.wait(t), frames[0]), t
                ring.release(t)
            ring.destroy()
        assert np.array_equal(dev.readback(), frames[0])
        info = dev.graph_info()
        dev.destroy()
        return info

    assert loop(True) == loop(False)


@pytest.mark.parametrize("fixed", [True, False], ids=["fixed-speed", "timer"])
@pytest.mark.parametrize("kind", ["plain", "k1", "k2"])
def test_async_recorder_writes_the_synchronous_files(tmp_path, kind, fixed):
    """Six recording presents through the pipelined recorder (depth 3) and through the synchronous one: the same
    bytes in the video and in its sample index, `frames` == 6 right after the loop, nothing written by presents
    before start or after stop.  On the deferred device at one frame to a launch five of the six prepasses ran
    fused (the synchronous recorder's present launches every frame: none)."""
    import gpgpuraytrace_amd as G
    land, w, h, cams, frames = _golden_pair()
    times = [0.04, 0.0333, 0.05, 0.016, 0.1, 0.02]
    dev, ter = _device(kind)

    def record(path, depth):
        rec = G.RecorderFactory.construct(dev, 25, fixed, path, async_depth=depth)
        assert rec is not None, G.lib().rt_last_error()
        dev.present()  # not recording: nothing is written
        rec.start()
        for i in range(6):
            _pose(ter, cams[i % 2])
            ter.render_device()
            rec.set_frame_time(times[i])
            dev.present()
        fused = dev.deferred_fused()
        assert rec.info()["frames"] == 6
        rec.stop()
        ter.render_device()
        dev.present()  # after stop: nothing is written
        rec.destroy()
        return fused

    pa, ps = str(tmp_path / "async.rgb32"), str(tmp_path / "sync.rgb32")
    fused = record(pa, 3)
    if kind == "k1":
        assert fused == 5
    record(ps, 0)
    video = open(pa, "rb").read()
    assert len(video) == 6 * w * h * 4
    assert video == open(ps, "rb").read()
    assert open(pa + ".txt", "rb").read() == open(ps + ".txt", "rb").read()
    vid, _ = G.read_recording(pa, w, h)
    for i in range(6):
        assert np.array_equal(vid[i], O.bgrx(frames[i % 2])), i
    dev.destroy()


def test_lifetimes():
    """A ring destroyed with one capture attached and one in flight; a device destroyed before its ring (every
    later ring call is RT_ERR_STATE); a fresh device then checks clean."""
    import gpgpuraytrace_amd as G
    land, w, h, cams, frames = _golden_pair()
    dev, ter = _device("k1")
    ring = dev.readback_ring("rgba8", depth=3)
    ter.render_device()
    ring.submit()        # attached to the pending frame ...
    _pose(ter, cams[1])
    ter.render_device()  # ... whose trace this render launches: in flight
    ring.submit()        # attached
    ring.destroy()
    assert np.array_equal(dev.readback(), frames[1])
    ring = dev.readback_ring("bgrx", depth=2)
    t = ring.submit()
    dev.destroy()
    L = G.lib()
    assert _submit_rc(ring)[0] == RT_ERR_STATE
    assert L.rt_readback_ready(ring._h, t) == RT_ERR_STATE
    assert _wait_rc(ring, t) == (RT_ERR_STATE, None)
    assert L.rt_readback_release(ring._h, t) == RT_ERR_STATE
    ring.destroy()
    dev, ter = _device("plain")
    ter.render_device()
    dev.check()
    assert np.array_equal(dev.readback(), frames[0])
    dev.destroy()
