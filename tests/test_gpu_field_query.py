"""GPU tests of the field queries (rt_terrain_sample_field / _lattice and their device forms, ABI 9 additive): the
density getDensity gives and the normal getNormal gives at points of the caller's own and on a lattice the device
forms itself, with the lattice's occupancy bits.  Bar: every float and every occupancy word equals the checker's
(tests/field_ref.py: the oracle's ro_get_density_batch and get_normal) bit for bit, the lattice form equals the
point form over the same points, at every size, grid, eye and option, and a query between two renders changes
nothing about the frame loop."""
import ctypes as C

import numpy as np
import pytest

import field_ref as FR
import golden_index as GI
import ray_fixture as RF
from test_gpu_parity import FixedCamera, make

pytestmark = pytest.mark.gpu

RT_OK, RT_ERR_INVALID, RT_ERR_STATE = 0, -1, -5
DEFER = dict(deferred=True, debug_defer_small=True)
EYE = (0.3, 30.2, 0.4)  # inside the near lattice, 0.54 from its point (0, 30, 0): octave count 17 there
# the small shapes: partial waves, partial occupancy words, rows shorter than a wave; a spacing and an origin that
# are not dyadic (an unfused i * s + o differs from fmaf); the y origin puts each landscape's surface inside
SMALL = ((1, 1, 1), (33, 5, 3), (64, 4, 4), (70, 3, 2), (97, 1, 1))
SMALL_SPACING = (2.3, 4.1, 2.3)
SMALL_Y = {"nomadplains": 38.7, "testing": -8.3, "simple": -50.3, "greenrocks": -38.3}
# nomadplains (name -> origin, spacing, dims, eye)
NEAR = ((-60.0, 0.0, -50.0), (2.5, 2.5, 2.5), (48, 24, 40), EYE)
NOMAD = {
    "near": NEAR,                                                                   # counts 17..14, terraces, lift
    "coarse": ((-888.0, 0.0, -888.0), (37.0, 37.0, 37.0), (48, 4, 48), EYE),        # counts down to about 8
    "far": ((4600.0, 0.0, 100.0), (2.5, 12.5, 2.5), (33, 5, 3), EYE),               # the count clamps at 2
    "general": ((2960.0, 0.0, -2040.0), (2.5, 5.0, 2.5), (33, 12, 32), (3000.3, 30.2, -2000.4)),  # no fast cells
    "negative": ((60.0, 87.5, 50.0), (-2.5, -2.5, -2.5), (33, 24, 3), EYE),
    "zero": ((-40.0, 20.0, 7.5), (2.5, 2.5, 0.0), (33, 12, 3), EYE),
}


def _make(land="nomadplains", consts=None, **kw):
    """A 64x48 device and its terrain (the camera is the golden reset pose: Eye = (0, 100, 0))."""
    return make(consts or GI.consts(64, 48, "reset"), land, float_output=False, **kw)


def _bits(got, want, what=""):
    assert got is not None, what
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    g, w = np.ascontiguousarray(got).view(np.uint32).ravel(), np.ascontiguousarray(want).view(np.uint32).ravel()
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, bad.size, bad[:8], got.reshape(-1)[bad[:4]], want.reshape(-1)[bad[:4]])


def _octaves(points, eye):
    """nomadplains' octave count per point, in float64 (terrain.hlsl:16-22)."""
    dist = np.maximum(np.linalg.norm(points.astype(np.float64) - np.asarray(eye, np.float64), axis=1), 0.01)
    return np.floor(np.maximum(18.0 - dist ** 0.33, 2.0)).astype(int)


def _cloud(eye, n=1024, seed=11):
    """A seeded cloud around an eye: wide in x and z, y from 60 below to 60 above."""
    rng = np.random.default_rng(seed)
    p = np.asarray(eye, np.float64) + rng.normal(0.0, 1.0, (n, 3)) * np.array([80.0, 25.0, 80.0])
    return p.astype(np.float32)


def _points(land):
    """The point form's points: the fixture rays' last samples (4096, on and off the surface) and the cloud."""
    return np.ascontiguousarray(np.concatenate([RF.oracle_query(RF.F_SET, land)[0][:, :3], _cloud(RF.eye("F0"))]))


# --- the point form -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("land", RF.LANDSCAPES)
def test_points_parity_with_the_checker(land):
    import gpgpuraytrace_amd as G
    p = _points(land)
    eye = RF.eye("F0")
    want_d, want_n = FR.cached("points", p, eye, land), FR.cached("points", p, eye, land, normals=True)
    # conditions on the checker, not on the device: finite normals, both signs
    assert np.isfinite(want_n).all() and 0.1 < np.mean(want_d > 0) < 0.9
    _bits(want_n[:, 3].copy(), want_d)
    dev, ter = _make(land)
    _bits(ter.sample_field(p, eye=eye), want_d, G.lib().rt_last_error())
    _bits(ter.sample_field(p, eye=eye, normals=True), want_n)
    _bits(ter.sample_field(p), want_d)  # eye=None: the compute's Eye, the reset pose's (0, 100, 0)
    dev.check()
    dev.destroy()


def test_points_sizes_and_grids():
    """n = 1, 63, 64, 65, 255, 256, 257; 2049 on grids of one and two blocks (a block takes three tiles, the last
    partial); n = 0, which launches nothing."""
    import gpgpuraytrace_amd as G
    p = _points("nomadplains")
    eye = RF.eye("F0")
    want_d, want_n = FR.cached("points", p, eye, "nomadplains"), FR.cached("points", p, eye, "nomadplains", normals=True)
    dev, ter = _make()
    for n in (1, 63, 64, 65, 255, 256, 257):
        _bits(ter.sample_field(p[:n], eye=eye), want_d[:n], n)
        _bits(ter.sample_field(p[:n], eye=eye, normals=True), want_n[:n], n)
    for mb in (1, 2):
        _bits(ter.sample_field(p[:2049], eye=eye, max_blocks=mb), want_d[:2049], mb)
        _bits(ter.sample_field(p[:2049], eye=eye, normals=True, max_blocks=mb), want_n[:2049], mb)
    assert ter.sample_field(p[:0], eye=eye).shape == (0,) and ter.sample_field(p[:0], normals=True).shape == (0, 4)
    cs = ter.camera_compute._h
    assert G.lib().rt_terrain_sample_field(cs, None, 0, None, None) == RT_OK
    assert G.lib().rt_terrain_sample_field_device(cs, None, 0, None, None) == RT_OK
    dev.check()
    dev.destroy()


# --- the lattice form -----------------------------------------------------------------------------------------------
def _check_lattice(ter, key, origin, spacing, dims, eye, land, normals=True):
    """Densities, {normal, density}, occupancy (alone and beside the results) against the checker and the point form."""
    nx, ny, nz = dims
    p, want_d = FR.lattice(key, origin, spacing, dims, eye, land)
    occ = FR.occupancy_words(want_d, dims)
    got = ter.sample_lattice(origin, spacing, dims, eye=eye, occupancy=True)
    assert got is not None, key
    _bits(got[0], want_d, key)
    assert got[1].shape == occ.shape and np.array_equal(got[1], occ), key
    _bits(ter.sample_lattice(origin, spacing, dims, eye=eye), want_d, key)
    _bits(ter.sample_field(p, eye=eye).reshape(nz, ny, nx), want_d, key)
    # occupancy alone: results NULL (the buffer starts poisoned; padding bits are written 0)
    import gpgpuraytrace_amd as G
    alone = np.full(occ.shape, 0xdeadbeef, np.uint32)
    lat, opt = G.engine.lattice(origin, spacing, dims), G.engine.field_options(eye, normals)
    assert G.lib().rt_terrain_sample_lattice(ter.camera_compute._h, C.byref(lat), C.byref(opt), None, alone.ctypes.data) == RT_OK
    assert np.array_equal(alone, occ), key
    if normals:
        _, want_n = FR.lattice(key, origin, spacing, dims, eye, land, normals=True)
        assert np.isfinite(want_n).all(), key  # (a condition on the checker)
        got = ter.sample_lattice(origin, spacing, dims, eye=eye, normals=True, occupancy=True)
        _bits(got[0], want_n, key)
        assert np.array_equal(got[1], occ), key
        _bits(ter.sample_field(p, eye=eye, normals=True).reshape(nz, ny, nx, 4), want_n, key)
    return p, want_d


@pytest.mark.parametrize("land", RF.LANDSCAPES)
def test_small_lattices(land):
    origin = (0.7, SMALL_Y[land], 0.7)
    dev, ter = _make(land)
    for dims in SMALL:
        _, d = _check_lattice(ter, "small%dx%dx%d" % dims, origin, SMALL_SPACING, dims, EYE, land)
        if dims == (33, 5, 3):
            assert 0.1 < np.mean(d > 0) < 0.9, land  # the surface runs through it
    dev.check()
    dev.destroy()


def test_the_near_lattice_covers_the_density_s_paths():
    """48 x 24 x 40 of spacing 2.5 around the eye, y from 0 to 57.5: octave counts 17 down to 14, waves (rows of one
    y) with and without terraces (0.4 y > 13) and floor lift (0.4 y < 10), both signs, fast cells."""
    origin, spacing, dims, eye = NEAR
    p = FR.lattice_points(origin, spacing, dims)
    assert set(np.unique(_octaves(p, eye))) >= {14, 15, 16, 17}
    y = np.unique(p[:, 1])
    assert (0.4 * y > 13).any() and (0.4 * y <= 13).any() and (0.4 * y < 10).any() and (0.4 * y >= 10).any()
    dev, ter = _make()
    _, d = _check_lattice(ter, "near", origin, spacing, dims, eye, "nomadplains")
    assert 0.1 < np.mean(d > 0) < 0.9
    # a grid of one block walks every strip
    _bits(ter.sample_lattice(origin, spacing, dims, eye=eye, max_blocks=1), d)
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("name", ["coarse", "far", "general", "negative", "zero"])
def test_nomadplains_lattices(name):
    origin, spacing, dims, eye = NOMAD[name]
    p = FR.lattice_points(origin, spacing, dims)
    n_oct = _octaves(p, eye)
    q = np.abs(p.astype(np.float64) * 0.4 * 0.006).max(axis=1)
    scale = 1.96 ** n_oct.astype(np.float64)
    if name == "coarse":
        assert n_oct.min() <= 8 and n_oct.max() >= 14
    elif name == "far":
        assert np.linalg.norm(p.astype(np.float64) - np.asarray(eye), axis=1).min() > 4500 and (n_oct == 2).all()
    elif name == "general":
        # every lane's last octave lies outside the fast cells' range (rt_shader.h kFastCellRange = 2^13), with
        # a factor 1.96 to spare for a count one lower: every wave takes the general cell path
        assert (q * scale / 1.96 > 8192.0).all()
    else:
        assert (q * scale * 1.96 < 8192.0).mean() > 0.5  # (mostly fast cells)
    dev, ter = _make()
    _, d = _check_lattice(ter, name, origin, spacing, dims, eye, "nomadplains", normals=name != "coarse")
    if name in ("negative", "zero"):
        assert 0.1 < np.mean(d > 0) < 0.9
    if name == "zero":
        assert np.array_equal(d[0], d[1]) and np.array_equal(d[0], d[2])  # the same plane three times
    dev.check()
    dev.destroy()


def test_the_eye_is_the_option_s_or_the_compute_s():
    origin, spacing, dims = (-40.0, 20.0, -10.0), (2.5, 2.5, 2.5), (33, 12, 3)
    here, there = EYE, (13.0, 92.0, -9.5)
    _, d_here = FR.lattice("eye-here", origin, spacing, dims, here, "nomadplains", normals=True)
    p, d_there = FR.lattice("eye-there", origin, spacing, dims, there, "nomadplains", normals=True)
    assert (d_here.view(np.uint32) != d_there.view(np.uint32)).mean() > 0.5  # two eyes, two fields
    reset = RF.eye("F0")  # the compute's Eye after _make: the reset pose's
    _, d_reset = FR.lattice("eye-reset", origin, spacing, dims, reset, "nomadplains", normals=True)
    dev, ter = _make()
    _bits(ter.sample_lattice(origin, spacing, dims, eye=here, normals=True), d_here)
    _bits(ter.sample_lattice(origin, spacing, dims, eye=there, normals=True), d_there)
    _bits(ter.sample_lattice(origin, spacing, dims, normals=True), d_reset)  # eye=None
    _bits(ter.sample_field(p, normals=True).reshape(d_reset.shape), d_reset)
    consts = dict(RF.consts("G"))
    ter.set_camera(FixedCamera(consts))
    ter.update_terrain()  # writes the Eye variables: G's eye is `there`
    assert np.array_equal(RF.eye("G"), np.asarray(there, np.float32))
    _bits(ter.sample_lattice(origin, spacing, dims, normals=True), d_there)
    _bits(ter.sample_field(p, normals=True).reshape(d_there.shape), d_there)
    _bits(ter.sample_lattice(origin, spacing, dims, eye=here, normals=True), d_here)
    dev.check()
    dev.destroy()


def test_either_kind_of_compute():
    import gpgpuraytrace_amd as G
    origin, spacing, dims = (0.7, SMALL_Y["nomadplains"], 0.7), SMALL_SPACING, (33, 5, 3)
    _, want = FR.lattice("small33x5x3", origin, spacing, dims, EYE, "nomadplains")
    dev, ter = _make()
    got = np.empty(want.shape, np.float32)
    lat, opt = G.engine.lattice(origin, spacing, dims), G.engine.field_options(EYE)
    for cs in (ter.camera_compute._h, ter.compute._h):
        got[:] = np.nan
        assert G.lib().rt_terrain_sample_lattice(cs, C.byref(lat), C.byref(opt), got.ctypes.data, None) == RT_OK
        _bits(got, want)
    dev.check()
    dev.destroy()


# --- the device forms -----------------------------------------------------------------------------------------------
def test_device_forms_equal_the_host_forms():
    """torch-allocated points, results and occupancy on a caller's stream: the points are filled on torch's stream
    and handed over by event, the results handed back by event, no host synchronisation in between.  The outputs
    start poisoned."""
    import torch
    import gpgpuraytrace_amd as G
    origin, spacing, dims = (-40.0, 20.0, -10.0), (2.5, 2.5, 2.5), (70, 12, 3)
    nx, ny, nz = dims
    p = FR.lattice_points(origin, spacing, dims)
    n = len(p)
    dev, ter = _make()
    host_d, host_n = ter.sample_field(p, eye=EYE), ter.sample_field(p, eye=EYE, normals=True)
    host_l, host_occ = ter.sample_lattice(origin, spacing, dims, eye=EYE, occupancy=True)
    _bits(host_l.reshape(-1), host_d)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        pts = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
        res_d = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda:0")
        res_n = torch.full((n, 4), float("nan"), dtype=torch.float32, device="cuda:0")
        lat_d = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda:0")
        lat_n = torch.full((n, 4), float("nan"), dtype=torch.float32, device="cuda:0")
        occ = torch.full((nz, ny, (nx + 31) // 32), -1, dtype=torch.int32, device="cuda:0")
        occ2 = torch.full((nz, ny, (nx + 31) // 32), -1, dtype=torch.int32, device="cuda:0")
        pts.copy_(torch.from_numpy(G.pack_points(p)), non_blocking=False)
        filled = torch.cuda.Event()
        filled.record(side)
        dev.wait_event(filled.cuda_event)
        assert ter.sample_field_device(pts.data_ptr(), n, res_d.data_ptr(), eye=EYE)
        assert ter.sample_field_device(pts.data_ptr(), n, res_n.data_ptr(), eye=EYE, normals=True)
        assert ter.sample_lattice_device(origin, spacing, dims, lat_d.data_ptr(), occ.data_ptr(), eye=EYE)
        assert ter.sample_lattice_device(origin, spacing, dims, lat_n.data_ptr(), eye=EYE, normals=True)
        assert ter.sample_lattice_device(origin, spacing, dims, 0, occ2.data_ptr(), eye=EYE, normals=True)
        done = torch.cuda.Event()
        done.record(side)  # torch creates its events on first record; the device then re-records it on its stream
        dev.record_event(done.cuda_event)
        side.wait_event(done)
        out = [t.cpu().numpy() for t in (res_d, res_n, lat_d, lat_n, occ, occ2)]
    _bits(out[0], host_d)
    _bits(out[1], host_n)
    _bits(out[2], host_d)
    _bits(out[3], host_n)
    assert np.array_equal(out[4].view(np.uint32), host_occ) and np.array_equal(out[5].view(np.uint32), host_occ)
    _bits(host_n, FR.cached("device", p, EYE, "nomadplains", normals=True))
    dev.check()
    dev.destroy()


# --- arguments ------------------------------------------------------------------------------------------------------
def test_arguments():
    import torch
    import gpgpuraytrace_amd as G
    from gpgpuraytrace_amd import _native
    L = G.lib()
    p = _points("nomadplains")[:8].copy()
    # room for the largest host result below: the 16 points of `good` with their normals (256 bytes)
    res = np.zeros((16, 4), np.float32)
    dev, ter = _make()
    cs = ter.camera_compute._h
    pp, rp = p.ctypes.data, res.ctypes.data
    dpts = torch.from_numpy(G.pack_points(p)).to("cuda:0")
    dres = torch.zeros((64, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    DP, DO = dpts.data_ptr(), dres.data_ptr()

    def ref(o):
        return C.byref(o) if o is not None else None

    def host(n=8, opt=None, p_=pp, r_=rp):
        return L.rt_terrain_sample_field(cs, p_, n, ref(opt), r_)

    def devf(n=8, opt=None, p_=DP, r_=DO):
        return L.rt_terrain_sample_field_device(cs, p_, n, ref(opt), r_)

    good = G.engine.lattice((0, 30, 0), (1, 1, 1), (4, 2, 2))

    def lhost(lat=good, opt=None, r_=rp, o_=None):
        return L.rt_terrain_sample_lattice(cs, ref(lat), ref(opt), r_, o_)

    def ldev(lat=good, opt=None, r_=DO, o_=None):
        return L.rt_terrain_sample_lattice_device(cs, ref(lat), ref(opt), r_, o_)

    assert host() == RT_OK and devf() == RT_OK and lhost() == RT_OK and ldev() == RT_OK  # opt NULL
    dev.synchronize()
    for f in (host, devf):
        assert f(n=-1) == RT_ERR_INVALID and b"2^26" in L.rt_last_error()
        assert f(n=(1 << 26) + 1) == RT_ERR_INVALID
    assert host(p_=None) == RT_ERR_INVALID and host(r_=None) == RT_ERR_INVALID
    assert devf(p_=None) == RT_ERR_INVALID and devf(r_=None) == RT_ERR_INVALID
    for f in (host, devf, lhost, ldev):
        for size in (0, 8, 23):
            short = G.engine.field_options()
            short.size = size
            assert f(opt=short) == RT_ERR_INVALID and b"size" in L.rt_last_error()
        for flags in (2, 4, 8, 16, 64, 1 << 31, 32 | 4):
            bad = G.engine.field_options()
            bad.flags = flags
            assert f(opt=bad) == RT_ERR_INVALID and b"flags" in L.rt_last_error(), flags
        assert f(opt=G.engine.field_options(EYE, True)) == RT_OK
    later = (C.c_uint32 * 16)()  # a later, longer version of the options: its first fields mean the same
    later[0], later[1] = 64, _native.RT_FIELD_NORMAL
    assert L.rt_terrain_sample_field(cs, pp, 8, C.cast(later, C.POINTER(_native.RtFieldOptions)), rp) == RT_OK
    for f in (lhost, ldev):
        assert f(lat=None) == RT_ERR_INVALID
        assert f(r_=None, o_=None) == RT_ERR_INVALID and b"both null" in L.rt_last_error()
        for dims in ((4097, 1, 1), (1, 4097, 1), (1, 1, 4097), (0, 4097, 1)):
            assert f(lat=G.engine.lattice((0, 0, 0), (1, 1, 1), dims)) == RT_ERR_INVALID and b"4096" in L.rt_last_error()
        assert f(lat=G.engine.lattice((0, 0, 0), (1, 1, 1), (4096, 4096, 5))) == RT_ERR_INVALID and b"2^26" in L.rt_last_error()
        for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):  # nothing to do: RT_OK, nothing launched, nothing required
            assert f(lat=G.engine.lattice((0, 0, 0), (1, 1, 1), dims), r_=None, o_=None) == RT_OK
        for bad in (float("inf"), -float("inf"), float("nan")):
            for axis in range(3):
                o, s = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
                o[axis] = bad
                assert f(lat=G.engine.lattice(o, s, (2, 2, 2))) == RT_ERR_INVALID and b"finite" in L.rt_last_error()
                o[axis], s[axis] = 0.0, bad
                assert f(lat=G.engine.lattice(o, s, (2, 2, 2))) == RT_ERR_INVALID
    # the Python mirror: None / False, no exception
    assert ter.sample_lattice((0, 0, 0), (1, 1, 1), (4097, 1, 1)) is None
    assert ter.sample_lattice_device((0, 0, 0), (1, 1, 1), (2, 2, 2)) is False
    # no texture bound: RT_ERR_STATE, as the other queries
    bare = dev.create_compute()
    assert bare.create("shaders", "camerarays.hlsl", "CSMain", (16, 16, 1)) and bare.swap()
    assert L.rt_terrain_sample_field(bare._h, pp, 8, None, rp) == RT_ERR_STATE and b"texPerm2D" in L.rt_last_error()
    assert L.rt_terrain_sample_field_device(bare._h, DP, 8, None, DO) == RT_ERR_STATE
    assert L.rt_terrain_sample_lattice(bare._h, C.byref(good), None, rp, None) == RT_ERR_STATE
    assert L.rt_terrain_sample_lattice_device(bare._h, C.byref(good), None, DO, None) == RT_ERR_STATE
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
    """A lattice with an explicit eye (normals and occupancy on alternate calls) and the same points through the
    point form: the checker's bits."""
    origin, spacing, dims = (0.7, SMALL_Y["nomadplains"], 0.7), SMALL_SPACING, (33, 5, 3)
    p, want = FR.lattice("small33x5x3", origin, spacing, dims, EYE, "nomadplains", normals=bool(k % 2))
    got, occ = ter.sample_lattice(origin, spacing, dims, eye=EYE, normals=bool(k % 2), occupancy=True)
    _bits(got, want, k)
    assert np.array_equal(occ, FR.occupancy_words(want[..., 3] if k % 2 else want, dims)), k
    _bits(ter.sample_field(p, eye=EYE, normals=bool(k % 2)).reshape(want.shape), want, k)


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


@pytest.mark.parametrize("batch", [1, 2])
def test_deferred_loop_is_undisturbed(batch):
    """A deferred device at one and at two frames to a launch: a query between two renders launches no pending
    frame (the same deferred_fused and launch_info as without), and the frames are golden."""
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
                _query(ter, k)
                assert (dev.deferred_fused(), dev.launch_info()) == before, k
            infos.append(before)
        assert np.array_equal(dev.readback(), frames[(n - 1) % 2])  # (launches what is pending)
        infos.append((dev.deferred_fused(), dev.launch_info()))
        dev.check()
        dev.destroy()
        return infos

    with_q, without = loop(True), loop(False)
    assert with_q == without and with_q[-1][0] == n - batch  # all but the first `batch` frames prepass inside a trace


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
