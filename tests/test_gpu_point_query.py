"""GPU tests of point shading (rt_terrain_shade_points / _device, ABI 9 additive): getColor with its shadow ray and
the AO factor of K hemisphere rays at points and normals the caller holds, as a frame computes both for a pixel whose
primary ray ended there.  Bar: the 4 result floats, the RGBA8 word and both step counts equal the checker's
(tests/point_ref.py: the oracle's own get_color and ambient_occlusion) bit for bit, at every size, grid, K, seed and
option; the device form reads a mesh extraction's arrays as they are; and a query between two renders changes nothing
about the frame loop.  The point sets and their census are test_point_query_host.py's."""
import ctypes as C

import numpy as np
import pytest

import point_ref as PR
import ray_fixture as RF
from test_gpu_parity import make
from test_gpu_shade_query import DEFER, F_EYE, _golden_pair, _make, _pose

pytestmark = pytest.mark.gpu

RT_OK, RT_ERR_INVALID, RT_ERR_STATE = 0, -1, -5
SEEDS = (0, 3)
POISON = 0xdeadbeef


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what=""):
    """got: (results, rgba8, steps) of shade_points; want: the checker's tuple."""
    res, px, steps = got
    wres, wpx, wsteps = want[:3]
    assert res.shape == wres.shape and res.shape[1:] == (4,) and res.dtype == np.float32
    assert px.dtype == np.uint32 and steps.dtype == np.uint32 and steps.shape == wsteps.shape
    bad = np.flatnonzero((_bits(res) != _bits(wres)).any(axis=1))
    assert bad.size == 0, (what, bad.size, bad[:8], res[bad[:4]], wres[bad[:4]])
    bad = np.flatnonzero(px != wpx)
    assert bad.size == 0, (what, bad.size, bad[:8], px[bad[:4]], wpx[bad[:4]])
    bad = np.flatnonzero((steps != wsteps).any(axis=1))
    assert bad.size == 0, (what, bad.size, bad[:8], steps[bad[:4]], wsteps[bad[:4]])


@pytest.mark.parametrize("K", [0, 1, 4, 16])
@pytest.mark.parametrize("land", RF.LANDSCAPES)
def test_parity_with_the_checker(land, K):
    """PR.points(land) (at most 2,048 points, eye F0's) at both seeds: everything; at the first seed also without the
    step counts, the results alone and the pixels alone."""
    import gpgpuraytrace_amd as G
    L = G.lib()
    p, nrm = PR.points(land)
    dev, ter = _make(land)
    for seed in SEEDS:
        want = PR.query(land, K, seed)
        got = ter.shade_points(p, nrm, eye=F_EYE, ao_samples=K, seed=seed, rgba8=True, steps=True)
        assert got is not None, L.rt_last_error()
        _same(got, want, (land, K, seed))
        if K == 0:
            assert (got[0][:, 3] == 1).all() and not got[2][:, 1].any()
    seed = SEEDS[0]
    want = PR.query(land, K, seed)
    res, px = ter.shade_points(p, nrm, eye=F_EYE, ao_samples=K, seed=seed, rgba8=True)  # the kernels without the step counts
    assert np.array_equal(_bits(res), _bits(want[0])) and np.array_equal(px, want[1])
    res = ter.shade_points(p, nrm, eye=F_EYE, ao_samples=K, seed=seed)  # results only
    assert np.array_equal(_bits(res), _bits(want[0]))
    px = np.full(len(p), POISON, np.uint32)  # rgba8 only, with the step counts
    st = np.full((len(p), 2), POISON, np.uint32)
    opt = G.point_options(F_EYE, K, seed)
    assert L.rt_terrain_shade_points(ter.compute._h, p.ctypes.data, nrm.ctypes.data, len(p), C.byref(opt), None,
                                     px.ctypes.data, st.ctypes.data) == RT_OK
    assert np.array_equal(px, want[1]) and np.array_equal(st, want[2])
    dev.check()
    dev.destroy()


def _stretched(land, n):
    """n points: PR.points(land) over and over (a point's index enters its AO directions, so the checker runs on the
    very array)."""
    p, nrm = PR.points(land)
    reps = -(-n // len(p))
    return np.ascontiguousarray(np.tile(p, (reps, 1))[:n]), np.ascontiguousarray(np.tile(nrm, (reps, 1))[:n])


def test_sizes():
    """n = 1, 63, 64, 65 (a partial wave, a wave's boundary), 1023, 1025 and 2049 (a block's boundary, a third block),
    with K = 4, and n = 0, which launches nothing."""
    import gpgpuraytrace_amd as G
    L = G.lib()
    p, nrm = _stretched("nomadplains", 2049)
    want = PR.shade(p, nrm, F_EYE, "nomadplains", ao_samples=4, seed=3)  # (a prefix of the points is a prefix of the results)
    dev, ter = _make()
    for n in (1, 63, 64, 65, 1023, 1025, 2049):
        got = ter.shade_points(p[:n], nrm[:n], eye=F_EYE, ao_samples=4, seed=3, rgba8=True, steps=True)
        assert got is not None, n
        _same(got, tuple(a[:n] for a in want[:3]), n)
    got = ter.shade_points(p[:0], nrm[:0], eye=F_EYE, ao_samples=4, rgba8=True, steps=True)
    assert got is not None and got[0].shape == (0, 4) and got[1].shape == (0,) and got[2].shape == (0, 2)
    cs = ter.compute._h
    assert L.rt_terrain_shade_points(cs, None, None, 0, None, None, None, None) == RT_OK
    assert L.rt_terrain_shade_points_device(cs, None, None, 0, None, None, None, None) == RT_OK
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("max_blocks", [1, 2])
@pytest.mark.parametrize("land", ["nomadplains", "greenrocks"])
def test_refill_and_phase_mixing(land, max_blocks):
    """A grid of 1 or 2 blocks and 2,048 points in a seeded order, K = 4 and 16: a block refills every lane, so lanes
    in their shadow march, in any of their AO marches and at the colour coexist in a wave; two blocks share the
    counter."""
    p, nrm = _stretched(land, 2048)
    perm = np.random.default_rng(4133).permutation(2048)
    p, nrm = np.ascontiguousarray(p[perm]), np.ascontiguousarray(nrm[perm])
    dev, ter = _make(land)
    for K in (4, 16):
        got = ter.shade_points(p, nrm, eye=F_EYE, ao_samples=K, seed=3, rgba8=True, steps=True, max_blocks=max_blocks)
        assert got is not None
        _same(got, PR.shade(p, nrm, F_EYE, land, ao_samples=K, seed=3), (land, K))
    dev.check()
    dev.destroy()


def test_eye():
    """The eye (the density's level of detail and the viewpoint of dist and pdn): the option's, else the compute's
    Eye."""
    p, nrm = (a[:1024] for a in PR.points("nomadplains"))
    want_g = PR.shade(p, nrm, RF.eye("G"), "nomadplains", ao_samples=4, seed=3)
    want_f = PR.shade(p, nrm, F_EYE, "nomadplains", ao_samples=4, seed=3)
    assert not np.array_equal(_bits(want_g[0][:, :3]), _bits(want_f[0][:, :3]))
    dev, ter = _make()
    kw = dict(ao_samples=4, seed=3, rgba8=True, steps=True)
    _same(ter.shade_points(p, nrm, eye=RF.eye("G"), **kw), want_g)  # (the compute's Eye is F's)
    _same(ter.shade_points(p, nrm, **kw), want_f)  # eye=None: the compute's, F's
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("land", ["nomadplains", "simple"])
def test_recording_constants(land):
    """A compute created with RECORDING: the marches' step and density factors are the recording ones."""
    p, nrm = (a[:1024] for a in PR.points(land))
    want = PR.shade(p, nrm, F_EYE, land, ao_samples=4, seed=0, recording=1)
    plain = PR.query(land, 4, 0)
    assert not np.array_equal(want[2], plain[2][:1024])
    dev, ter = _make(land, recording=True)
    _same(ter.shade_points(p, nrm, eye=F_EYE, ao_samples=4, seed=0, rgba8=True, steps=True), want)
    dev.check()
    dev.destroy()


def test_device_form_equals_host_form():
    """torch-allocated points, normals and outputs; the inputs are filled on torch's stream and handed over by event,
    the results handed back by rt_device_record_event: no host synchronisation in between.  The spare words of the
    inputs are junk; the output buffers start poisoned."""
    import torch
    import gpgpuraytrace_amd as G
    p, nrm = (a[:1025] for a in PR.points("nomadplains"))
    n = len(p)
    dev, ter = _make()
    host = ter.shade_points(p, nrm, eye=F_EYE, ao_samples=4, seed=3, rgba8=True, steps=True)
    _same(host, tuple(a[:n] for a in PR.query("nomadplains", 4, 3)[:3]))
    pk, nk = G.pack_points(p), G.pack_points(nrm)
    pk[:, 3], nk[:, 3] = np.float32("nan"), np.float32(1e30)
    dp = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    dn = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    res = torch.full((n + 1, 4), float("nan"), dtype=torch.float32, device="cuda:0")
    pix = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda:0")
    steps = torch.full((n + 1, 2), -1, dtype=torch.int32, device="cuda:0")
    pix2 = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    dp.copy_(torch.from_numpy(pk), non_blocking=False)
    dn.copy_(torch.from_numpy(nk), non_blocking=False)
    filled = torch.cuda.Event()
    filled.record(torch.cuda.current_stream())
    dev.wait_event(filled.cuda_event)
    kw = dict(eye=F_EYE, ao_samples=4, seed=3)
    assert ter.shade_points_device(dp.data_ptr(), dn.data_ptr(), n, res.data_ptr(), pix.data_ptr(), steps.data_ptr(), **kw)
    assert ter.shade_points_device(dp.data_ptr(), dn.data_ptr(), n, 0, pix2.data_ptr(), **kw)  # the pixels alone
    done = torch.cuda.Event()
    done.record()  # torch creates its events on first record; the device then re-records it on its stream
    dev.record_event(done.cuda_event)
    torch.cuda.current_stream().wait_event(done)
    r, q, s, q2 = (x.cpu().numpy() for x in (res, pix, steps, pix2))
    _same((r[:n], q[:n].view(np.uint32), s[:n].view(np.uint32)), host)
    assert np.array_equal(q2[:n].view(np.uint32), host[1])
    # nothing beyond n
    assert np.isnan(r[n]).all() and q[n] == -1 and (s[n] == -1).all() and q2[n] == -1
    dev.check()
    dev.destroy()


def test_device_form_reads_a_mesh_extractions_arrays():
    """extract_mesh_device's vertices and normals of a 33^3 lattice go into shade_points_device as they are, the cell
    index and density words in place: the same bits as the host form on the downloaded arrays."""
    import torch
    import gpgpuraytrace_amd as G
    origin, spacing, dims = (-40.3, 0.0, -39.1), (2.5, 2.5, 2.5), (33, 33, 33)
    dev, ter = _make()
    need = G.engine.mesh_scratch_bytes(origin, spacing, dims)
    cap_v, cap_t = 32 * 32 * 32, 6 * 32 * 32 * 32
    scratch = torch.zeros(need, dtype=torch.uint8, device="cuda:0")
    v = torch.zeros((cap_v, 4), dtype=torch.float32, device="cuda:0")
    nr = torch.zeros((cap_v, 4), dtype=torch.float32, device="cuda:0")
    t = torch.zeros((cap_t, 3), dtype=torch.int32, device="cuda:0")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert ter.extract_mesh_device(origin, spacing, dims, scratch.data_ptr(), need, v.data_ptr(), nr.data_ptr(), cap_v,
                                   t.data_ptr(), cap_t, counts.data_ptr(), eye=F_EYE)
    dev.synchronize()
    nv = int(counts.cpu().numpy()[0])
    assert 256 <= nv <= cap_v
    res = torch.full((nv, 4), float("nan"), dtype=torch.float32, device="cuda:0")
    pix = torch.full((nv,), -1, dtype=torch.int32, device="cuda:0")
    steps = torch.full((nv, 2), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert ter.shade_points_device(v.data_ptr(), nr.data_ptr(), nv, res.data_ptr(), pix.data_ptr(), steps.data_ptr(),
                                   eye=F_EYE, ao_samples=4, seed=3)
    dev.synchronize()
    hv, hn = v.cpu().numpy()[:nv], nr.cpu().numpy()[:nv]
    assert hv[:, 3].view(np.uint32).max() > 0 and np.abs(hn[:, 3]).max() > 0  # the spare words are in place
    host = ter.shade_points(hv, hn, eye=F_EYE, ao_samples=4, seed=3, rgba8=True, steps=True)
    assert host is not None
    _same((res.cpu().numpy(), pix.cpu().numpy().view(np.uint32), steps.cpu().numpy().view(np.uint32)), host)
    # and the host form is the checker's on those arrays
    _same(host, PR.shade(hv, hn, F_EYE, "nomadplains", ao_samples=4, seed=3))
    dev.check()
    dev.destroy()


def test_extract_mesh_colours():
    """extract_mesh(colors=True, ao_samples=4): one more array, shade_points' pixels for the returned vertices at
    their normals; the default return value is unchanged."""
    origin, spacing, dims = (-40.3, 0.0, -39.1), (2.5, 2.5, 2.5), (17, 33, 17)
    dev, ter = _make()
    plain = ter.extract_mesh(origin, spacing, dims, eye=F_EYE)
    got = ter.extract_mesh(origin, spacing, dims, eye=F_EYE, colors=True, ao_samples=4, seed=3)
    assert plain is not None and got is not None and len(plain) == 4 and len(got) == 5
    for a, b in zip(plain, got[:4]):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    verts, nrm, _, _, colours = got
    assert len(verts) >= 64 and colours.shape == (len(verts),) and colours.dtype == np.uint32
    res, px = ter.shade_points(verts, nrm, eye=F_EYE, ao_samples=4, seed=3, rgba8=True)
    assert np.array_equal(colours, px) and (colours >> 24 == 255).all()
    assert np.array_equal(px, PR.shade(verts, nrm, F_EYE, "nomadplains", ao_samples=4, seed=3)[1])
    flat = ter.extract_mesh(origin, spacing, dims, eye=F_EYE, colors=True)  # K = 0
    assert np.array_equal(flat[4], ter.shade_points(verts, nrm, eye=F_EYE, rgba8=True)[1])
    with pytest.raises(ValueError):
        ter.extract_mesh(origin, spacing, dims, normals=False, colors=True)
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("land", ["nomadplains", "greenrocks"])
def test_consistent_with_shade_rays(land):
    """test_point_query_host's pin re-run with the device's numbers: p = rr.pd.xyz of shade_rays' hits for camera F0's
    rays and n from trace_surface.  shade_points at (p, n) is the checker's; and the oracle's get_color at the RAY's
    own (pdn, rr.pd.w), through trace_sample's two lerps with the oracle's fcolord and rayleigh term, is shade_rays'
    colour -- so the two queries differ by the definition's (pdn, dist) and the blends, nothing else."""
    o, d = RF.rays("F0")
    dev, ter = _make(land)
    shaded = ter.shade_rays(o, d, eye=F_EYE)
    surf = ter.trace_surface(o, d, eye=F_EYE)
    assert shaded is not None and surf is not None
    assert np.array_equal(_bits(shaded[:, 4:8]), _bits(np.concatenate([surf[:, :3], surf[:, 7:8]], axis=1)))
    hit = np.flatnonzero(shaded[:, 7] > 0)
    assert len(hit) >= 256
    p, nrm = np.ascontiguousarray(shaded[hit, 4:7]), np.ascontiguousarray(surf[hit, 4:7])
    got = ter.shade_points(p, nrm, eye=F_EYE, ao_samples=4, seed=3, rgba8=True, steps=True)
    want = PR.shade(p, nrm, F_EYE, land, ao_samples=4, seed=3)
    _same(got, want, land)
    _, _, fc, ray, pdn = PR.primary(o[hit], d[hit], F_EYE, land)
    col_ray, _ = PR.get_color(p, nrm, pdn, shaded[hit, 3], F_EYE, land)
    assert np.array_equal(_bits(PR.blend(col_ray, shaded[hit, 3], fc, ray)), _bits(shaded[hit, :3]))
    col_own, _ = PR.get_color(p, nrm, want[5][:, :3], want[5][:, 3], F_EYE, land)
    assert np.array_equal(_bits(got[0][:, :3]), _bits(col_own))
    dev.check()
    dev.destroy()


def test_errors():
    """Every argument error of the header, host and device form, with the output arrays poisoned and proved
    untouched."""
    import torch
    import gpgpuraytrace_amd as G
    from gpgpuraytrace_amd import _native
    L = G.lib()
    p, nrm = (np.ascontiguousarray(a[:8]) for a in PR.points("nomadplains"))
    res, px, st = np.zeros((8, 4), np.float32), np.zeros(8, np.uint32), np.zeros((8, 2), np.uint32)
    dev, ter = _make()
    cs = ter.compute._h
    pp, np_, rp, xp, sp = p.ctypes.data, nrm.ctypes.data, res.ctypes.data, px.ctypes.data, st.ctypes.data

    def ref(o):
        return C.byref(o) if o is not None else None

    def host(n=8, opt=None, cs_=cs, p_=pp, n_=np_, r_=rp, x_=xp):
        return L.rt_terrain_shade_points(cs_, p_, n_, n, ref(opt), r_, x_, sp)

    dpts = torch.from_numpy(G.pack_points(p)).to("cuda:0")
    dnrm = torch.from_numpy(G.pack_points(nrm)).to("cuda:0")
    dres = torch.zeros((8, 4), dtype=torch.float32, device="cuda:0")
    dpix = torch.zeros(8, dtype=torch.int32, device="cuda:0")
    dst = torch.zeros((8, 2), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    DP, DN, DR, DX, DS = (x.data_ptr() for x in (dpts, dnrm, dres, dpix, dst))

    def devf(n=8, opt=None, cs_=cs, p_=DP, n_=DN, r_=DR, x_=DX):
        return L.rt_terrain_shade_points_device(cs_, p_, n_, n, ref(opt), r_, x_, DS)

    good = G.point_options(F_EYE, 4, 3)
    assert host(opt=good) == RT_OK and devf(opt=good) == RT_OK
    dev.synchronize()
    _same((res, px, st), tuple(a[:8] for a in PR.query("nomadplains", 4, 3)[:3]))
    assert np.array_equal(_bits(dres.cpu().numpy()), _bits(res))
    assert host() == RT_OK and (res[:, 3] == 1).all()  # opt NULL: K = 0, seed 0, the compute's Eye
    # poison
    res.view(np.uint32)[:], px[:], st[:] = POISON, POISON, POISON
    for x in (dres, dpix, dst):
        x.view(torch.int32).fill_(-559038737)
    torch.cuda.synchronize()

    def opt_with(**kw):
        o = G.point_options(F_EYE, 4, 3)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    for f in (host, devf):
        # a camerarays compute has no SunDirection
        assert f(cs_=ter.camera_compute._h) == RT_ERR_INVALID and b"camerarays" in L.rt_last_error()
        # neither output
        assert f(r_=None, x_=None) == RT_ERR_INVALID and b"both null" in L.rt_last_error()
        # the inputs
        assert f(p_=None) == RT_ERR_INVALID and b"null points or normals" in L.rt_last_error()
        assert f(n_=None) == RT_ERR_INVALID
        # the count
        assert f(n=-1) == RT_ERR_INVALID and b"2^26" in L.rt_last_error()
        assert f(n=(1 << 26) + 1) == RT_ERR_INVALID
        # the option block
        for size in (0, 8, 24, 31):
            assert f(opt=opt_with(size=size)) == RT_ERR_INVALID and b"size" in L.rt_last_error()
        for flags in (2, 4, 8, 16, 32, 64, 1 << 31, _native.RT_RAYS_EYE | _native.RT_RAYS_FORCE_LANES):
            assert f(opt=opt_with(flags=flags)) == RT_ERR_INVALID and b"flags" in L.rt_last_error(), flags
        for k in (17, 64, 0xffffffff):
            assert f(opt=opt_with(ao_samples=k)) == RT_ERR_INVALID and b"ao_samples" in L.rt_last_error(), k
        assert f(cs_=None) == RT_ERR_INVALID
    # no texture bound: RT_ERR_STATE, as the other queries
    bare = dev.create_compute()
    assert bare.create("shaders", "tracescreen.hlsl", "CSMain", (16, 16, 1)) and bare.swap()
    assert host(cs_=bare._h) == RT_ERR_STATE and b"texPerm2D" in L.rt_last_error()
    assert devf(cs_=bare._h) == RT_ERR_STATE
    # the Python mirror: None or False, no exception; mismatched arrays raise
    assert ter.shade_points(p, nrm, ao_samples=17) is None
    assert not ter.shade_points_device(DP, DN, 8, DR, ao_samples=17)
    assert not ter.shade_points_device(DP, DN, 8)
    with pytest.raises(ValueError):
        ter.shade_points(p, nrm[:5])
    # nothing was written by any refused call
    dev.synchronize()
    assert (res.view(np.uint32) == POISON).all() and (px == POISON).all() and (st == POISON).all()
    for x in (dres, dpix, dst):
        assert (x.cpu().numpy().view(np.uint32) == POISON).all()
    # a larger size (a later version of the block) and ao_samples = 16 are fine
    assert host(opt=opt_with(size=64, ao_samples=16)) == RT_OK and devf(opt=opt_with(size=64, ao_samples=16)) == RT_OK
    dev.check()
    dev.destroy()


# --- the frame loop is undisturbed --------------------------------------------------------------
_want = {}


def _query(ter, sun, k):
    """256 points with an explicit eye under the terrain's current sun (the pose's), K = 4: the checker's bits."""
    p, nrm = (a[:256] for a in PR.points("nomadplains"))
    key = tuple(float(v) for v in np.asarray(sun, np.float32)[:3])
    if key not in _want:
        _want[key] = PR.shade(p, nrm, RF.eye("G"), "nomadplains", ao_samples=4, seed=3, sun=key)
    got = ter.shade_points(p, nrm, eye=RF.eye("G"), ao_samples=4, seed=3, rgba8=True, steps=True)
    assert got is not None
    _same(got, _want[key], k)


def test_plain_serial_loop_is_undisturbed():
    """Six renders on a plain device, the camera alternating between two golden poses, a query after each: as many
    renders prepassed on the prepass stream as without queries, every frame golden."""
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


@pytest.mark.parametrize("batch", [1, 2])
def test_deferred_loop_is_undisturbed(batch):
    """A deferred device at one and at two frames to a launch: a query between two renders launches no pending frame
    (the same deferred_fused and launch_info as without), and the frames are golden."""
    land, cams, frames = _golden_pair()
    n = 6

    def loop(queries):
        dev, ter = make(cams[0], land, float_output=False, **DEFER)
        dev.defer_batch(batch)
        infos = []
        for k in range(n):
            _pose(ter, cams[k % 2])
            ter.render_device()
            before = (dev.deferred_fused(), dev.launch_info())
            if queries:
                _query(ter, cams[k % 2]["sun"], k)
                assert (dev.deferred_fused(), dev.launch_info()) == before, k
            infos.append(before)
        assert np.array_equal(dev.readback(), frames[(n - 1) % 2])  # (launches what is pending)
        infos.append((dev.deferred_fused(), dev.launch_info()))
        dev.check()
        dev.destroy()
        return infos

    with_q, without = loop(True), loop(False)
    assert with_q == without and with_q[-1][0] == n - batch


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
