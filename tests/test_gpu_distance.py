"""GPU tests of the distance fields (rt_terrain_distance_field and its device form, ABI 9 additive): the exact
squared lattice distance of every lattice point to the nearest point of the other occupancy state, and the signed
distance.  Bar: every d2 word and every distance float equals the checker's (tests/dist_ref.py: per-axis min-plus
over whole axes in numpy integers) bit for bit, for occupancy the caller gives and for the terrain's own, at every
shape, grid and option, and a call between two renders changes nothing about the frame loop."""
import ctypes as C

import numpy as np
import pytest

import dist_ref as DR
import golden_index as GI
import ray_fixture as RF
from test_gpu_field_query import DEFER, EYE, NEAR, SMALL, SMALL_SPACING, SMALL_Y, _golden_pair, _make, _pose
from test_gpu_parity import make

pytestmark = pytest.mark.gpu

RT_OK, RT_ERR_INVALID, RT_ERR_STATE = 0, -1, -5
FAR = DR.FAR
POISON = 0xdeadbeef
THERE = (13.0, 92.0, -9.5)  # a second eye: other octave counts, another field


def _call(ter, dims, words=None, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), eye=None, max_cells=0, max_blocks=0,
          d2=True, dist=True, cs=None):
    """The C entry point with both outputs poisoned: (rc, d2, distance)."""
    import gpgpuraytrace_amd as G
    nx, ny, nz = dims
    lat, opt = G.engine.lattice(origin, spacing, dims), G.engine.distance_options(eye, max_cells, max_blocks)
    out2 = np.full((nz, ny, nx), POISON, np.uint32)
    outd = np.full((nz, ny, nx), np.nan, np.float32)
    if words is not None:
        words = np.ascontiguousarray(words, np.uint32)
    rc = G.lib().rt_terrain_distance_field(cs or ter.camera_compute._h, C.byref(lat), C.byref(opt),
                                           words.ctypes.data if words is not None else None,
                                           out2.ctypes.data if d2 else None, outd.ctypes.data if dist else None)
    return rc, out2, outd


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = np.ascontiguousarray(got).view(np.uint32).ravel(), np.ascontiguousarray(want).view(np.uint32).ravel()
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, bad.size, bad[:8], got.reshape(-1)[bad[:4]], want.reshape(-1)[bad[:4]])


def _check(ter, dims, words, what, spacing=(1.0, 1.0, 1.0), checker_words=None, **kw):
    """Both outputs of one call against the checker, bit for bit.  checker_words: what the checker reads when the
    device forms the occupancy itself."""
    import gpgpuraytrace_amd as G
    ref = words if checker_words is None else checker_words
    mc = kw.get("max_cells", 0)
    rc, d2, dist = _call(ter, dims, words, spacing=spacing, **kw)
    assert rc == RT_OK, (what, G.lib().rt_last_error())
    _same(d2, DR.d2(ref, dims, mc), what)
    _same(dist, DR.distance(ref, dims, spacing, mc), what)
    return d2, dist


def _ball(dims, centre, radius):
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= radius * radius


# --- occupancy the caller gives: no terrain in the answer ------------------------------------------------------------
def test_given_shapes_with_known_answers():
    dev, ter = _make()
    # a single voxel in 33 x 5 x 3: d2 = dx^2 + dy^2 + dz^2, the voxel's own value 1
    dims = (33, 5, 3)
    inside = np.zeros((3, 5, 33), bool)
    inside[1, 3, 17] = True
    d2, dist = _check(ter, dims, DR.pack(inside, dims), "voxel", spacing=(2.5, 2.5, 2.5))
    z, y, x = np.meshgrid(np.arange(3), np.arange(5), np.arange(33), indexing="ij")
    want = ((x - 17) ** 2 + (y - 3) ** 2 + (z - 1) ** 2).astype(np.uint32)
    want[1, 3, 17] = 1
    assert np.array_equal(d2, want) and dist[1, 3, 17] == np.float32(-2.5) and (dist > 0).sum() == inside.size - 1
    # a sphere and a half space in 70 x 9 x 8
    dims = (70, 9, 8)
    _check(ter, dims, DR.pack(_ball(dims, (40, 4, 3), 3.3), dims), "sphere", spacing=(0.5, 0.5, 0.5))
    _check(ter, dims, DR.pack(~_ball(dims, (31.5, 4, 4), 3.7), dims), "hollow", spacing=(0.5, 0.5, 0.5))
    half = np.zeros((8, 9, 70), bool)
    half[:, :4, :] = True
    d2, dist = _check(ter, dims, DR.pack(half, dims), "half space")
    rows = np.where(np.arange(9) < 4, 4 - np.arange(9), np.arange(9) - 3)
    assert np.array_equal(d2, np.broadcast_to((rows * rows)[None, :, None], d2.shape))
    assert ((dist < 0) == half).all()
    half_x = np.zeros((8, 9, 70), bool)
    half_x[:, :, 37:] = True  # the boundary inside an occupancy word
    _check(ter, dims, DR.pack(half_x, dims), "half space in x")
    # all inside, all outside: far everywhere, the sign the state's
    for fill in (False, True):
        d2, dist = _check(ter, dims, DR.pack(np.full((8, 9, 70), fill), dims), "uniform")
        assert (d2 == FAR).all() and np.isinf(dist).all() and ((dist < 0) == fill).all()
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("nx", [33, 97])
def test_padding_bits_are_ignored(nx):
    """All-inside rows with the padding bits of a row's last word set to 1 and to 0: far everywhere both times.
    Then rows with points of both states: the padding must not pass for a point of either state."""
    dims = (nx, 3, 2)
    dev, ter = _make()
    full = np.ones((2, 3, nx), bool)
    results = []
    for padding in (1, 0):
        words = DR.pack(full, dims, padding)
        assert (words[..., -1] >> (nx % 32)).any() == bool(padding)  # (the padding is what it should be)
        d2, dist = _check(ter, dims, words, ("full", padding))
        assert (d2 == FAR).all() and (dist == -np.inf).all()
        results.append(d2)
    assert np.array_equal(results[0], results[1])
    rng = np.random.default_rng(nx)
    mixed = rng.random((2, 3, nx)) < 0.9
    mixed[0, 1, :] = True
    mixed[1, 2, :] = False
    a = _check(ter, dims, DR.pack(mixed, dims, 0), "mixed 0")
    b = _check(ter, dims, DR.pack(mixed, dims, 1), "mixed 1")
    garbage = DR.pack(mixed, dims, 0)
    garbage[..., -1] |= (rng.integers(0, 1 << 32, garbage[..., -1].shape, dtype=np.uint64).astype(np.uint32)
                         & np.uint32((0xffffffff << (nx % 32)) & 0xffffffff))
    c = _check(ter, dims, garbage, "mixed garbage")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0])
    _same(a[1], b[1])
    _same(a[1], c[1])
    dev.check()
    dev.destroy()


def test_rows_of_one_point_and_columns_longer_than_any_tile():
    dev, ter = _make()
    rng = np.random.default_rng(3)
    for dims in ((1, 7, 5), (1, 1, 1), (1, 1, 9), (5, 1, 1)):
        nx, ny, nz = dims
        inside = rng.random((nz, ny, nx)) < 0.4
        _check(ter, dims, DR.pack(inside, dims, 1), dims)
    for dims, axis in (((3, 300, 2), 1), ((2, 2, 300), 0)):
        nx, ny, nz = dims
        # a single voxel at the far end, a slab at the far end, and noise: scans of 1 to 299 cells
        one = np.zeros((nz, ny, nx), bool)
        one[(nz - 1, ny - 2, 1) if axis == 1 else (nz - 2, 1, 1)] = True
        d2, _ = _check(ter, dims, DR.pack(one, dims), (dims, "voxel"))
        assert d2.max() >= 297 * 297
        slab = np.zeros((nz, ny, nx), bool)
        slab[(slice(None), slice(290, None), slice(None)) if axis == 1 else (slice(290, None), slice(None), slice(None))] = True
        d2, _ = _check(ter, dims, DR.pack(slab, dims), (dims, "slab"))
        assert d2.max() == 290 * 290
        _check(ter, dims, DR.pack(rng.random((nz, ny, nx)) < 0.02, dims), (dims, "sparse"))
        _check(ter, dims, DR.pack(rng.random((nz, ny, nx)) < 0.5, dims), (dims, "dense"))
    dev.check()
    dev.destroy()


# --- the terrain's own occupancy ------------------------------------------------------------------------------------
@pytest.mark.parametrize("land", RF.LANDSCAPES)
def test_small_terrain_lattices(land):
    """test_gpu_field_query's small shapes and y origins.  Their spacing is anisotropic, so d2 is asked for alone
    and a second call on an isotropic spacing of the same x gives the distance."""
    origin = (0.7, SMALL_Y[land], 0.7)
    dev, ter = _make(land)
    for dims in SMALL:
        key = "small%dx%dx%d" % dims
        words = DR.terrain_words(key, origin, SMALL_SPACING, dims, EYE, land)
        if dims == (33, 5, 3):
            inside = DR.unpack(words, dims)
            assert inside.any() and not inside.all(), land  # (a condition on the checker)
        rc, d2, dist = _call(ter, dims, None, origin, SMALL_SPACING, eye=EYE, dist=False)
        assert rc == RT_OK, key
        _same(d2, DR.d2(words, dims), (land, key))
        assert np.isnan(dist).all()
        # the same occupancy handed back in gives the same field
        rc, again, _ = _call(ter, dims, words, origin, SMALL_SPACING, dist=False)
        assert rc == RT_OK and np.array_equal(again, d2)
    iso = (2.3, 2.3, 2.3)
    dims = (33, 5, 3)
    words = DR.terrain_words("small-iso", origin, iso, dims, EYE, land)
    _check(ter, dims, None, (land, "iso"), spacing=iso, checker_words=words, origin=origin, eye=EYE)
    dev.check()
    dev.destroy()


def test_the_near_lattice_with_two_eyes():
    origin, spacing, dims, eye = NEAR
    here = DR.terrain_words("near", origin, spacing, dims, eye, "nomadplains")
    there = DR.terrain_words("near-there", origin, spacing, dims, THERE, "nomadplains")
    # conditions on the checker: both states present, scans that cross more than a few cells, two eyes two fields
    for words in (here, there):
        inside = DR.unpack(words, dims)
        assert inside.any() and not inside.all()
        want = DR.d2(words, dims)
        print("largest finite d2 %d, inside %.3f" % (want[want != FAR].max(), inside.mean()))
        assert want[want != FAR].max() >= 16
    assert not np.array_equal(here, there)
    dev, ter = _make()
    _check(ter, dims, None, "near", spacing=spacing, checker_words=here, origin=origin, eye=eye)
    _check(ter, dims, None, "near there", spacing=spacing, checker_words=there, origin=origin, eye=THERE)
    # the Python mirror: the float field, the squared field, an occupancy array of the caller's
    dist = ter.distance_field(origin, spacing, dims, eye=eye)
    _same(dist, DR.distance(here, dims, spacing))
    _same(ter.distance_field(origin, spacing, dims, eye=eye, squared=True), DR.d2(here, dims))
    _same(ter.distance_field(origin, spacing, dims, occupancy=there, max_cells=2), DR.distance(there, dims, spacing, 2))
    # the README's use: the cells an agent of radius 3 may stand in
    free = dist >= 3.0
    assert free.any() and not (free & DR.unpack(here, dims)).any()
    # either kind of compute
    rc, d2, _ = _call(ter, dims, None, origin, spacing, eye=eye, cs=ter.compute._h)
    assert rc == RT_OK
    _same(d2, DR.d2(here, dims))
    dev.check()
    dev.destroy()


# --- options and grids ----------------------------------------------------------------------------------------------
def test_max_cells_grids_and_single_outputs():
    origin, spacing, dims, eye = NEAR
    words = DR.terrain_words("near", origin, spacing, dims, eye, "nomadplains")
    full = DR.d2(words, dims)
    dev, ter = _make()
    for mc in (1, 3, 5000):
        d2, _ = _check(ter, dims, words, ("max_cells", mc), spacing=spacing, max_cells=mc)
        assert ((d2 == FAR) == (full.astype(np.int64) > mc * mc)).all()
        _check(ter, dims, None, ("max_cells, own", mc), spacing=spacing, checker_words=words, origin=origin, eye=eye,
               max_cells=mc)
    # a sparse grid, where max_cells cuts long scans, on every grid
    rng = np.random.default_rng(8)
    sdims = (70, 40, 9)
    sparse = DR.pack(rng.random((9, 40, 70)) < 0.001, sdims, 1)
    for mb in (0, 1, 2):
        _check(ter, dims, words, ("max_blocks", mb), spacing=spacing, max_blocks=mb)
        _check(ter, dims, None, ("max_blocks, own", mb), spacing=spacing, checker_words=words, origin=origin, eye=eye,
               max_blocks=mb)
        for mc in (0, 1, 3, 5000):
            _check(ter, sdims, sparse, ("sparse", mb, mc), max_blocks=mb, max_cells=mc)
    # each output alone: the other array stays poisoned
    rc, d2, dist = _call(ter, dims, words, spacing=spacing, dist=False)
    assert rc == RT_OK and np.isnan(dist).all()
    _same(d2, full)
    rc, d2, dist = _call(ter, dims, words, spacing=spacing, d2=False)
    assert rc == RT_OK and (d2 == POISON).all()
    _same(dist, DR.distance(words, dims, spacing))
    dev.check()
    dev.destroy()


def test_negative_and_anisotropic_spacings():
    import gpgpuraytrace_amd as G
    dims = (33, 12, 5)
    dev, ter = _make()
    # a negative isotropic spacing: the lattice runs the other way, the distance is scaled by |spacing|
    origin, spacing = (40.0, 60.0, 5.0), (-2.5, -2.5, -2.5)
    words = DR.terrain_words("dist-negative", origin, spacing, dims, EYE, "nomadplains")
    inside = DR.unpack(words, dims)
    assert inside.any() and not inside.all()
    _, dist = _check(ter, dims, None, "negative", spacing=spacing, checker_words=words, origin=origin, eye=EYE)
    assert dist[~inside].min() == np.float32(2.5) and dist[inside].max() == np.float32(-2.5)
    _check(ter, dims, words, "mixed signs", spacing=(2.5, -2.5, 2.5))
    # anisotropic or zero: d2 is a lattice metric and fine, the distance is RT_ERR_INVALID and nothing is written
    for bad in ((2.5, 2.5, 5.0), (2.5, 5.0, 2.5), (5.0, 2.5, 2.5), (0.0, 0.0, 0.0), (2.5, 2.5, 0.0)):
        rc, d2, dist = _call(ter, dims, words, spacing=bad, dist=False)
        assert rc == RT_OK, bad
        _same(d2, DR.d2(words, dims), bad)
        for want_d2 in (True, False):
            rc, d2, dist = _call(ter, dims, words, spacing=bad, d2=want_d2)
            assert rc == RT_ERR_INVALID and b"isotropic" in G.lib().rt_last_error(), bad
            assert (d2 == POISON).all() and np.isnan(dist).all()
    assert ter.distance_field((0, 0, 0), (1, 1, 2), dims) is None
    assert ter.distance_field((0, 0, 0), (1, 1, 2), dims, occupancy=words, squared=True) is not None
    dev.check()
    dev.destroy()


# --- the device form ------------------------------------------------------------------------------------------------
def test_device_form_on_the_compute_s_stream():
    """torch-allocated occupancy, scratch and results, filled on torch's stream and handed over and back by event,
    no host synchronisation in between.  The outputs start poisoned; a scratch block one byte short is refused and
    nothing is written."""
    import torch
    import gpgpuraytrace_amd as G
    origin, spacing, dims, eye = NEAR
    nx, ny, nz = dims
    n = nx * ny * nz
    words = DR.terrain_words("near", origin, spacing, dims, eye, "nomadplains")
    rng = np.random.default_rng(4)
    given = DR.pack(rng.random((nz, ny, nx)) < 0.01, dims, 1)
    need = G.engine.distance_scratch_bytes(origin, spacing, dims)
    assert need > 12 * n
    dev, ter = _make()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        scratch = torch.zeros(need, dtype=torch.uint8, device="cuda:0")
        occ = torch.from_numpy(given.view(np.int32).copy()).to("cuda:0")
        outs = [torch.full((n,), -559038737, dtype=torch.int32, device="cuda:0") for _ in range(6)]
        filled = torch.cuda.Event()
        filled.record(side)
        dev.wait_event(filled.cuda_event)
        sp, p = scratch.data_ptr(), [t.data_ptr() for t in outs]
        assert ter.distance_field_device(origin, spacing, dims, sp, need, p[0], p[1], eye=eye)
        assert ter.distance_field_device(origin, spacing, dims, sp, need + 64, p[2], 0, occupancy_ptr=occ.data_ptr(), max_cells=9)
        assert ter.distance_field_device(origin, spacing, dims, sp, need, 0, p[3], occupancy_ptr=occ.data_ptr())
        # one byte short, a null block, no output: refused, nothing written
        assert not ter.distance_field_device(origin, spacing, dims, sp, need - 1, p[4], p[5], eye=eye)
        assert b"scratch" in G.lib().rt_last_error()
        assert not ter.distance_field_device(origin, spacing, dims, 0, need, p[4], p[5], eye=eye)
        assert not ter.distance_field_device(origin, spacing, dims, sp, need, 0, 0, eye=eye)
        done = torch.cuda.Event()
        done.record(side)  # torch creates its events on first record; the device then re-records it on its stream
        dev.record_event(done.cuda_event)
        side.wait_event(done)
        got = [t.cpu().numpy().view(np.uint32).reshape(nz, ny, nx) for t in outs]
    _same(got[0], DR.d2(words, dims))
    _same(got[1].view(np.float32), DR.distance(words, dims, spacing))
    _same(got[2], DR.d2(given, dims, 9))
    _same(got[3].view(np.float32), DR.distance(given, dims, spacing))
    assert (got[4] == POISON).all() and (got[5] == POISON).all()
    dev.check()
    dev.destroy()


# --- errors ---------------------------------------------------------------------------------------------------------
def test_every_argument_error_returns_its_code_and_writes_nothing():
    import torch
    import gpgpuraytrace_amd as G
    from gpgpuraytrace_amd import _native
    L = G.lib()
    dims = (33, 5, 3)
    n = 33 * 5 * 3
    words = DR.pack(_ball(dims, (16, 2, 1), 1.5), dims)
    dev, ter = _make()
    cs = ter.camera_compute._h
    d2 = np.full(n, POISON, np.uint32)
    dist = np.full(n, np.nan, np.float32)
    need = G.engine.distance_scratch_bytes((0, 0, 0), (1, 1, 1), dims)
    scratch = torch.zeros(need, dtype=torch.uint8, device="cuda:0")
    dout = torch.full((2, n), -559038737, dtype=torch.int32, device="cuda:0")
    docc = torch.from_numpy(words.view(np.int32).copy()).to("cuda:0")
    torch.cuda.synchronize()
    good = G.engine.lattice((0, 0, 0), (1, 1, 1), dims)

    def ref(o):
        return C.byref(o) if o is not None else None

    def host(lat=good, opt=None, occ=words.ctypes.data, a=d2.ctypes.data, b=dist.ctypes.data):
        return L.rt_terrain_distance_field(cs, ref(lat), ref(opt), occ, a, b)

    def devf(lat=good, opt=None, occ=docc.data_ptr(), a=dout[0].data_ptr(), b=dout[1].data_ptr(), sb=need):
        return L.rt_terrain_distance_field_device(cs, ref(lat), ref(opt), occ, scratch.data_ptr(), sb, a, b)

    for f in (host, devf):
        assert f(lat=None) == RT_ERR_INVALID
        for size in (0, 8, 24, 27):
            short = G.engine.distance_options()
            short.size = size
            assert f(opt=short) == RT_ERR_INVALID and b"size" in L.rt_last_error(), size
        for flags in (2, 4, 8, 16, 32, 64, 1 << 31, 1 | 32):
            bad = G.engine.distance_options()
            bad.flags = flags
            assert f(opt=bad) == RT_ERR_INVALID and b"flags" in L.rt_last_error(), flags
        assert f(a=None, b=None) == RT_ERR_INVALID and b"both null" in L.rt_last_error()
        for bad_dims in ((4097, 1, 1), (1, 4097, 1), (1, 1, 4097)):
            assert f(lat=G.engine.lattice((0, 0, 0), (1, 1, 1), bad_dims)) == RT_ERR_INVALID and b"4096" in L.rt_last_error()
        assert f(lat=G.engine.lattice((0, 0, 0), (1, 1, 1), (4096, 4096, 5))) == RT_ERR_INVALID and b"2^26" in L.rt_last_error()
        for bad in (float("inf"), float("nan")):
            assert f(lat=G.engine.lattice((0, bad, 0), (1, 1, 1), dims)) == RT_ERR_INVALID and b"finite" in L.rt_last_error()
            assert f(lat=G.engine.lattice((0, 0, 0), (1, 1, bad), dims)) == RT_ERR_INVALID
        for aniso in ((1, 1, 2), (0, 0, 0)):
            assert f(lat=G.engine.lattice((0, 0, 0), aniso, dims)) == RT_ERR_INVALID and b"isotropic" in L.rt_last_error()
        for zero in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):  # nothing to do: RT_OK, nothing launched, nothing required
            assert f(lat=G.engine.lattice((0, 0, 0), (1, 1, 1), zero), occ=None, a=None, b=None) == RT_OK
    assert devf(sb=need - 1) == RT_ERR_INVALID and devf(sb=0) == RT_ERR_INVALID
    assert L.rt_terrain_distance_field(None, ref(good), None, None, d2.ctypes.data, None) == RT_ERR_INVALID
    # no texture bound: RT_ERR_STATE, as the other queries
    bare = dev.create_compute()
    assert bare.create("shaders", "camerarays.hlsl", "CSMain", (16, 16, 1)) and bare.swap()
    assert L.rt_terrain_distance_field(bare._h, ref(good), None, words.ctypes.data, d2.ctypes.data, None) == RT_ERR_STATE
    assert b"texPerm2D" in L.rt_last_error()
    assert L.rt_terrain_distance_field_device(bare._h, ref(good), None, docc.data_ptr(), scratch.data_ptr(), need,
                                              dout[0].data_ptr(), None) == RT_ERR_STATE
    dev.synchronize()
    assert (d2 == POISON).all() and np.isnan(dist).all()
    assert (dout.cpu().numpy().view(np.uint32) == POISON).all()
    # and the calls the errors were variations of succeed; a later, longer option block means the same
    later = (C.c_uint32 * 16)()
    later[0], later[6] = 64, 1
    assert L.rt_terrain_distance_field(cs, ref(good), C.cast(later, C.POINTER(_native.RtDistanceOptions)),
                                       words.ctypes.data, d2.ctypes.data, dist.ctypes.data) == RT_OK
    _same(d2.reshape(3, 5, 33), DR.d2(words, dims, 1))
    assert host() == RT_OK and devf() == RT_OK
    dev.synchronize()
    _same(d2.reshape(3, 5, 33), DR.d2(words, dims))
    _same(dout[0].cpu().numpy().view(np.uint32).reshape(3, 5, 33), DR.d2(words, dims))
    _same(dout[1].cpu().numpy().view(np.float32).reshape(3, 5, 33), DR.distance(words, dims, (1, 1, 1)))
    dev.check()
    dev.destroy()


# --- the frame loop is undisturbed --------------------------------------------------------------
def _query(ter, k):
    """The terrain's own field with an explicit eye and a given occupancy on alternate calls: the checker's bits."""
    origin, spacing, dims = (0.7, SMALL_Y["nomadplains"], 0.7), (2.3, 2.3, 2.3), (33, 5, 3)
    words = DR.terrain_words("small-iso", origin, spacing, dims, EYE, "nomadplains")
    if k % 2:
        _same(ter.distance_field(origin, spacing, dims, eye=EYE), DR.distance(words, dims, spacing), k)
    else:
        _same(ter.distance_field(origin, spacing, dims, occupancy=words, squared=True, max_cells=3), DR.d2(words, dims, 3), k)


def test_plain_serial_loop_is_undisturbed():
    """Six renders on a plain device, the camera alternating between two golden poses, a distance field after each:
    as many renders prepassed on the prepass stream as without, every frame golden."""
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
    """A deferred device at two frames to a launch: a distance field between two renders launches no pending frame
    (the same deferred_fused and launch_info as without), and the frames are golden."""
    land, cams, frames = _golden_pair()
    n, batch = 6, 2

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
    assert with_q == without and with_q[-1][0] == n - batch
