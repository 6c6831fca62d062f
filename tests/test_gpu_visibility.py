"""GPU tests of the visibility fields (rt_terrain_visibility_field and its device form, ABI 9 additive): for every
point of a lattice the observers it has a free line of sight to over the occupancy bits.  Bar: every mask word and
every status word equal the checker's (tests/vis_ref.py: the header's definition in numpy int64, pinned on the CPU
by an exact interval test) bit for bit, for occupancy the caller gives and for the terrain's own, at every shape,
grid and option, and a call between two renders changes nothing about the frame loop."""
import ctypes as C

import numpy as np
import pytest

import dist_ref as DR
import ray_fixture as RF
import vis_ref as VR
from test_gpu_field_query import DEFER, EYE, NEAR, SMALL, SMALL_SPACING, SMALL_Y, _golden_pair, _make, _pose
from test_gpu_parity import make

pytestmark = pytest.mark.gpu

RT_OK, RT_ERR_INVALID, RT_ERR_STATE = 0, -1, -5
POISON = 0xdeadbeef
THERE = (13.0, 92.0, -9.5)  # a second eye: other octave counts, another field
_REF = {}  # the checker's results, computed once and shared (never written to)


def _want(words, dims, obs, max_range=0):
    key = (np.ascontiguousarray(words, np.uint32).tobytes(), tuple(dims), np.ascontiguousarray(obs, np.int32).tobytes(),
           int(max_range))
    if key not in _REF:
        mask, st = VR.field(words, dims, obs, max_range)
        mask.setflags(write=False)
        _REF[key] = (mask, st)
    return _REF[key]


def _call(ter, dims, words, obs, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), eye=None, max_range=0, max_blocks=0,
          status=True, cs=None):
    """The C entry point with every output poisoned: (rc, mask, status)."""
    import gpgpuraytrace_amd as G
    nx, ny, nz = dims
    lat = G.engine.lattice(origin, spacing, dims)
    opt = G.engine.visibility_options(eye, max_range, max_blocks)
    mask = np.full((nz, ny, nx), POISON, np.uint32)
    st = np.full(4, POISON, np.uint32)
    ob = np.ascontiguousarray(obs, np.int32).reshape(-1, 4)
    if words is not None:
        words = np.ascontiguousarray(words, np.uint32)
    rc = G.lib().rt_terrain_visibility_field(cs or ter.camera_compute._h, C.byref(lat), C.byref(opt),
                                             words.ctypes.data if words is not None else None, ob.ctypes.data, ob.shape[0],
                                             mask.ctypes.data, st.ctypes.data if status else None)
    return rc, mask, st


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = np.ascontiguousarray(got).ravel(), np.ascontiguousarray(want).ravel()
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, bad.size, bad[:8], g[bad[:4]], w[bad[:4]])


def _check(ter, dims, words, obs, what, checker_words=None, **kw):
    """The mask and the status of one host call against the checker, bit for bit."""
    import gpgpuraytrace_amd as G
    ref = words if checker_words is None else checker_words
    want = _want(ref, dims, obs, kw.get("max_range", 0))
    rc, mask, st = _call(ter, dims, words, obs, **kw)
    assert rc == RT_OK, (what, G.lib().rt_last_error())
    _same(mask, want[0], what)
    assert list(st) == want[1], (what, st, want[1])
    return mask, st


def _ball(dims, centre, radius):
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= radius * radius


# --- occupancy the caller gives: no terrain in the answer ------------------------------------------------------------
def test_given_shapes_with_known_answers():
    dev, ter = _make()
    dims = (33, 9, 8)
    n = 33 * 9 * 8
    wall = np.zeros((8, 9, 33), bool)
    wall[:, :, 16] = True
    mask, st = _check(ter, dims, DR.pack(wall, dims, 1), VR.observers([(3, 4, 4)]), "wall")
    assert list(st) == [1224, 1224, 1, 0] and (mask[:, :, :17] == 1).all() and not mask[:, :, 17:].any()
    wall[5, 2, 16] = False
    mask, st = _check(ter, dims, DR.pack(wall, dims, 1), VR.observers([(3, 4, 4)]), "wall with a hole")
    assert st[0] == 1259 and int(mask[:, :, 17:].sum()) == 35
    # the empty lattice: every bit; two observers at one point, one equal to the target, directions
    obs = VR.observers([(3, 4, 4), (3, 4, 4), (32, 8, 7)], [(0, 1, 0), (1, 1, 1), (-3, 2, 1)])
    mask, st = _check(ter, dims, DR.pack(np.zeros((8, 9, 33), bool), dims), obs, "empty")
    assert (mask == 63).all() and list(st) == [n, 6 * n, 6, 0]
    # all blocked: the observer (on a blocked point) and its 26 neighbours; a light reaches the last layer only
    mask, st = _check(ter, dims, DR.pack(np.ones((8, 9, 33), bool), dims), VR.observers([(3, 4, 4)], [(0, 1, 0)]), "all blocked")
    seen = np.argwhere(mask & 1)
    assert len(seen) == 27 and (np.abs(seen - np.array([4, 4, 3])).max(axis=1) <= 1).all() and mask[4, 4, 3] == 1
    assert list(st) == [27 + 33 * 8, 27 + 33 * 8, 2, 0]
    # a ball in 70 x 9 x 8: observers in the open, on the ball's surface and at its blocked centre, two at one point
    dims = (70, 9, 8)
    ball = DR.pack(_ball(dims, (40, 4, 3), 3.3), dims, 1)
    obs = VR.observers([(2, 4, 4), (40, 4, 3), (43, 4, 3), (2, 4, 4), (69, 8, 7)], [(0, 1, 0), (1, 1, 1), (-5, 1, 0)])
    mask, st = _check(ter, dims, ball, obs, "ball")
    assert np.array_equal(mask & 1, (mask >> 3) & 1) and mask[4, 4, 2] & 1 and mask[3, 4, 40] & 2
    assert 0 < int((mask & 1).sum()) < 70 * 9 * 8 and st[2] == 8
    for r in (3, 20):
        _check(ter, dims, ball, obs, ("ball", r), max_range=r)
    dev.check()
    dev.destroy()


def test_ties_touch_no_cell_and_enter_the_diagonal_cell():
    """17 x 17 x 17: the blocked set is the two cells beside each diagonal step of the x = y plane diagonals (and the
    six beside each space-diagonal step).  A line through a box edge or corner does not visit the cells it only
    touches, so the diagonals stay seen; a blocked diagonal cell occludes."""
    dev, ter = _make()
    dims = (17, 17, 17)
    corner, centre = (0, 0, 0), (8, 8, 8)
    obs = VR.observers([corner, centre], [(1, 1, 0), (1, -1, 1), (3, -2, 1), (0, 0, -1), (1, 1, 1), (-1, 1, 0)])
    beside = np.zeros((17, 17, 17), bool)
    for i in range(16):
        for dz, dy, dx in ((0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
            beside[i + dz, i + dy, i + dx] = True  # touched by the space diagonal's step from (i, i, i)
        beside[0, i, i + 1] = beside[0, i + 1, i] = True  # beside the in-plane 45 degree line in the z = 0 layer
    for i in range(17):
        beside[i, i, i] = False
        beside[0, i, i] = False
    mask, _ = _check(ter, dims, DR.pack(beside, dims), obs, "beside the diagonals")
    for i in range(17):
        assert mask[i, i, i] & 1 and mask[i, i, i] & 2 and mask[i, i, i] & (1 << 6), i  # corner, centre, (1, 1, 1)
        assert mask[0, i, i] & 1 and mask[0, i, i] & 4, i  # the in-plane diagonal from the corner; the light (1, 1, 0)
    on = beside.copy()
    on[5, 5, 5] = on[0, 11, 11] = True  # a diagonal cell itself
    mask, _ = _check(ter, dims, DR.pack(on, dims), obs, "a diagonal cell")
    assert not mask[6, 6, 6] & 1 and mask[5, 5, 5] & 1 and not mask[4, 4, 4] & 2 and mask[6, 6, 6] & 2
    assert not mask[4, 4, 4] & (1 << 6) and mask[5, 5, 5] & (1 << 6) and not mask[0, 12, 12] & 1 and not mask[0, 3, 3] & 4
    # random lattices under the same observers: every tie order
    rng = np.random.default_rng(17)
    for fill in (0.02, 0.1):
        _check(ter, dims, DR.pack(rng.random((17, 17, 17)) < fill, dims), obs, ("random", fill))
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("nx", [1, 31, 33, 64, 65])
def test_padding_bits_are_ignored(nx):
    dims = (nx, 3, 2)
    dev, ter = _make()
    rng = np.random.default_rng(nx)
    blocked = rng.random((2, 3, nx)) < 0.2
    obs = VR.observers([(0, 0, 0), (nx - 1, 2, 1)], [(1, 0, 0), (-1, 1, 0), (2, 1, 1)])
    out = []
    for padding in (0, 1):
        words = DR.pack(blocked, dims, padding)
        if nx % 32:
            assert (words[..., -1] >> (nx % 32)).any() == bool(padding)  # (the padding is what it should be)
        out.append(_check(ter, dims, words, obs, ("padding", padding)))
        full = DR.pack(np.zeros((2, 3, nx), bool), dims, padding)
        _, st = _check(ter, dims, full, obs, ("free, padding", padding))
        assert list(st) == [nx * 6, 5 * nx * 6, 5, 0]
    assert np.array_equal(out[0][0], out[1][0])
    dev.check()
    dev.destroy()


def test_rows_of_one_point():
    dev, ter = _make()
    rng = np.random.default_rng(3)
    for dims in ((1, 40, 3), (3, 1, 40), (1, 1, 1)):  # a wave spans many rows
        nx, ny, nz = dims
        blocked = rng.random((nz, ny, nx)) < 0.1
        obs = VR.observers([(0, 0, 0), (nx - 1, ny - 1, nz - 1)], [(0, 1, 0), (0, -1, 1), (1, 1, 1), (0, 0, -1)])
        _check(ter, dims, DR.pack(blocked, dims, 1), obs, dims)
    dev.check()
    dev.destroy()


_LONG = []


def _long_case():
    if not _LONG:
        dims = (4096, 3, 2)
        rng = np.random.default_rng(3)
        blocked = rng.random((2, 3, 4096)) < 0.02
        ends = ((0, 0, 0), (4095, 2, 1))
        sun = (4095, 1, 0)
        for x, y, z in VR.cells_between(*ends) + VR.direction_cells(ends[0], sun, dims) + VR.cells_between(ends[0], (4095, 0, 0)):
            blocked[z, y, x] = False
        _LONG.append((dims, ends, sun, DR.pack(blocked, dims)))
    return _LONG[0]


@pytest.mark.parametrize("case", ["ends", "sun", "range"])
def test_the_longest_walks(case):
    """4096 x 3 x 2: 128 words a row, walks of 4095 steps from both ends and along (4095, 1, 0).  About 2% blocked, so
    that most of the checker's walks are short, but for the cells of the long lines.  (A case an observer set: the
    checker takes a second or two for each walk of 4096 events.)"""
    dims, ends, sun, words = _long_case()
    dev, ter = _make()
    # (the assertions on the masks are conditions on the checker: the longest walks are walked to their ends)
    if case == "ends":
        mask, st = _check(ter, dims, words, VR.observers(ends), case)
        assert mask[1, 2, 4095] & 1 and mask[0, 0, 0] & 2 and mask[0, 0, 4095] & 1 and 4096 < st[1] < 2 * 4096 * 6
    elif case == "sun":
        mask, st = _check(ter, dims, words, VR.observers((), [sun]), case)
        assert mask[0, 0, 0] & 1 and 4096 < st[1] < 4096 * 6
    else:
        mask, _ = _check(ter, dims, words, VR.observers(ends[:1], [sun]), case, max_range=4000)
        assert not mask[1, 2, 4095] & 1 and mask[0, 0, 4000] & 1 and not mask[0, 0, 4001] & 1 and mask[0, 0, 0] & 2
    dev.check()
    dev.destroy()


RANDOM = (70, 24, 9)


def _random_case():
    """The random lattice, about 3% blocked, and 32 observers, points and directions mixed (bit 31 a direction)."""
    nx, ny, nz = RANDOM
    rng = np.random.default_rng(23)
    blocked = rng.random((nz, ny, nx)) < 0.03
    points = [(int(rng.integers(0, nx)), int(rng.integers(0, ny)), int(rng.integers(0, nz))) for _ in range(18)]
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (1, 1, 0), (-1, 1, 1), (3, -2, 1), (-7, 2, -1), (5, 3, 0), (255, -77, 13),
            (-4095, 4094, 1), (2, 1, 0), (-9, -4, 1), (1, 2, 0)]
    rows = []
    while points or dirs:  # alternating, so both kinds take low and high bits; the last four are points
        if points:
            rows.append(points.pop(0) + (VR.POINT,))
        if dirs:
            rows.append(dirs.pop(0) + (VR.DIRECTION,))
    obs = np.array(rows, np.int32)
    assert obs.shape == (32, 4)
    return DR.pack(blocked, RANDOM, 1), obs


def test_a_random_lattice_with_all_32_observers():
    words, obs = _random_case()
    n = RANDOM[0] * RANDOM[1] * RANDOM[2]
    want, st = _want(words, RANDOM, obs)
    assert st[2] == 32
    for k in range(32):  # (a condition on the checker: no bit is stuck either way)
        share = int(((want >> np.uint32(k)) & 1).sum()) / n
        assert 0.05 < share < 0.95, (k, obs[k], share)
    dev, ter = _make()
    for mb in (0, 1, 2):
        for r in (0, 5, 12):
            _check(ter, RANDOM, words, obs, ("random", mb, r), max_blocks=mb, max_range=r)
    assert not np.array_equal(_want(words, RANDOM, obs, 5)[0], want) and not np.array_equal(_want(words, RANDOM, obs, 12)[0], want)
    dev.check()
    dev.destroy()


# --- the terrain's own occupancy ------------------------------------------------------------------------------------
def _terrain_observers(words, dims, spacing):
    import gpgpuraytrace_amd as G
    nx, ny, nz = dims
    free = np.flatnonzero(~DR.unpack(words, dims).reshape(-1))
    first = int(free[0]) if free.size else 0
    sun = G.engine.lattice_direction(G.camera.sun_direction(0.3), spacing)
    return (first % nx, first // nx % ny, first // (nx * ny)), sun


@pytest.mark.parametrize("land", RF.LANDSCAPES)
def test_small_terrain_lattices(land):
    origin = (0.7, SMALL_Y[land], 0.7)
    dev, ter = _make(land)
    for dims in SMALL:
        key = "small%dx%dx%d" % dims
        words = DR.terrain_words(key, origin, SMALL_SPACING, dims, EYE, land)
        point, sun = _terrain_observers(words, dims, SMALL_SPACING)
        obs = VR.observers([point], [sun])
        mask, _ = _check(ter, dims, None, obs, (land, key), checker_words=words, origin=origin, spacing=SMALL_SPACING, eye=EYE)
        rc, again, _ = _call(ter, dims, words, obs, origin, SMALL_SPACING)
        assert rc == RT_OK and np.array_equal(again, mask)
    dev.check()
    dev.destroy()


def test_the_near_lattice_with_two_eyes():
    origin, spacing, dims, eye = NEAR
    here = DR.terrain_words("near", origin, spacing, dims, eye, "nomadplains")
    there = DR.terrain_words("near-there", origin, spacing, dims, THERE, "nomadplains")
    assert not np.array_equal(here, there)
    point, sun = _terrain_observers(here, dims, spacing)
    obs = VR.observers([point], [sun])
    want = _want(here, dims, obs)
    for b in (1, 2):  # (a condition on the checker: neither all set nor all clear)
        assert (want[0] & b).any() and not (want[0] & b).all()
    dev, ter = _make()
    _check(ter, dims, None, obs, "near", checker_words=here, origin=origin, spacing=spacing, eye=eye)
    _check(ter, dims, None, obs, "near there", checker_words=there, origin=origin, spacing=spacing, eye=THERE)
    for mb in (1, 2):
        _check(ter, dims, None, obs, ("near", mb), checker_words=here, origin=origin, spacing=spacing, eye=eye, max_blocks=mb,
               max_range=16)
    # the status optional: its block untouched
    rc, mask, st = _call(ter, dims, here, obs, status=False)
    assert rc == RT_OK and (st == POISON).all()
    _same(mask, want[0])
    # either kind of compute
    rc, mask, st = _call(ter, dims, None, obs, origin, spacing, eye=eye, cs=ter.compute._h)
    assert rc == RT_OK and list(st) == want[1]
    _same(mask, want[0])
    # the Python mirror: points and directions, the status, a given occupancy, a range
    status = []
    m = ter.visibility_field(origin, spacing, dims, observers=[point], directions=[sun], eye=eye, status=status)
    _same(m, want[0])
    assert status == want[1]
    m = ter.visibility_field(origin, spacing, dims, directions=[sun], occupancy=there, max_range=10, status=status)
    w = _want(there, dims, VR.observers((), [sun]), 10)
    _same(m, w[0])
    assert status == w[1]
    with pytest.raises(ValueError):
        ter.visibility_field(origin, spacing, dims, observers=[(dims[0], 0, 0)])
    dev.check()
    dev.destroy()


# --- the device form ------------------------------------------------------------------------------------------------
def test_device_form_on_the_compute_s_stream():
    """torch-allocated arrays, filled on torch's stream and handed over and back by event, no host synchronisation
    in between.  The outputs start poisoned; a scratch block of exactly scratch_bytes; a NULL status leaves its block
    alone; a scratch block one byte short is refused and nothing is written."""
    import torch
    import gpgpuraytrace_amd as G
    origin, spacing, dims, eye = NEAR
    nx, ny, nz = dims
    n = nx * ny * nz
    words = DR.terrain_words("near", origin, spacing, dims, eye, "nomadplains")
    point, sun = _terrain_observers(words, dims, spacing)
    obs = VR.observers([point], [sun])
    rng = np.random.default_rng(4)
    given = DR.pack(rng.random((nz, ny, nx)) < 0.03, dims, 1)
    # one invalid record among valid ones: its bit clear everywhere, status[2] counts the valid ones
    mixed = np.array([(5, 5, 5, 0), (nx, 0, 0, 0), (1, -2, 1, 1), (0, 0, 0, 1), (1, 1, 1, 7), (47, 23, 39, 0)], np.int32)
    need = G.engine.visibility_scratch_bytes(origin, spacing, dims)
    wants = (_want(words, dims, obs), _want(given, dims, mixed, 20), _want(words, dims, obs))
    assert wants[1][1][2] == 3 and not (wants[1][0] & 0b011010).any() and (wants[1][0] & 0b100101).any()
    host = []
    dev, ter = _make()
    for w, o, kw in ((None, obs, dict(origin=origin, spacing=spacing, eye=eye)), (given, VR.observers([(5, 5, 5)], [(1, -2, 1)]),
                                                                              dict(max_range=20))):
        rc, mask, st = _call(ter, dims, w, o, **kw)
        assert rc == RT_OK
        host.append(mask)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        scratch = torch.zeros(need, dtype=torch.uint8, device="cuda:0")
        occ = torch.from_numpy(given.view(np.int32).copy()).to("cuda:0")
        dobs = torch.from_numpy(np.concatenate([obs, mixed])).to("cuda:0")
        mask = torch.full((4, n), -559038737, dtype=torch.int32, device="cuda:0")
        st = torch.full((4, 4), -559038737, dtype=torch.int32, device="cuda:0")
        filled = torch.cuda.Event()
        filled.record(side)
        dev.wait_event(filled.cuda_event)
        sp = scratch.data_ptr()

        def run(k, obs_ptr, no, sb=need, status=True, **kw):
            return ter.visibility_field_device(origin, spacing, dims, obs_ptr, no, sp, sb, mask[k].data_ptr(),
                                               st[k].data_ptr() if status else 0, **kw)

        assert run(0, dobs.data_ptr(), 2, eye=eye), G.lib().rt_last_error()
        assert run(1, dobs.data_ptr() + 32, 6, occupancy_ptr=occ.data_ptr(), max_range=20)
        assert run(2, dobs.data_ptr(), 2, status=False, eye=eye)
        # one byte short, a null block: refused, nothing written
        assert not run(3, dobs.data_ptr(), 2, sb=need - 1, eye=eye)
        assert b"scratch" in G.lib().rt_last_error()
        assert not ter.visibility_field_device(origin, spacing, dims, dobs.data_ptr(), 2, 0, need, mask[3].data_ptr(), st[3].data_ptr())
        done = torch.cuda.Event()
        done.record(side)  # torch creates its events on first record; the device then re-records it on its stream
        dev.record_event(done.cuda_event)
        side.wait_event(done)
        got_m = mask.cpu().numpy().view(np.uint32).reshape(4, nz, ny, nx)
        got_s = st.cpu().numpy().view(np.uint32)
    for k, want in enumerate(wants):
        _same(got_m[k], want[0], k)
        if k < 2:
            assert list(got_s[k]) == want[1], (k, got_s[k])
    assert (got_s[2] == POISON).all()
    assert (got_m[3] == POISON).all() and (got_s[3] == POISON).all()
    # equal to the host form's (the mixed records' valid ones are the host call's observers at bits 0 and 2)
    _same(got_m[0], host[0])
    assert np.array_equal(got_m[1] & 1, host[1] & 1) and np.array_equal((got_m[1] >> 2) & 1, (host[1] >> 1) & 1)
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
    obs = VR.observers([(0, 0, 0), (32, 4, 2)], [(0, 1, 0)])
    dev, ter = _make()
    cs = ter.camera_compute._h
    mask = np.full(n, POISON, np.uint32)
    st = np.full(4, POISON, np.uint32)
    need = G.engine.visibility_scratch_bytes((0, 0, 0), (1, 1, 1), dims)
    scratch = torch.zeros(need, dtype=torch.uint8, device="cuda:0")
    dmask = torch.full((n,), -559038737, dtype=torch.int32, device="cuda:0")
    dst = torch.full((4,), -559038737, dtype=torch.int32, device="cuda:0")
    docc = torch.from_numpy(words.view(np.int32).copy()).to("cuda:0")
    dobs = torch.from_numpy(obs.copy()).to("cuda:0")
    torch.cuda.synchronize()
    good = G.engine.lattice((0, 0, 0), (1, 1, 1), dims)

    def ref(o):
        return C.byref(o) if o is not None else None

    def host(lat=good, opt=None, occ=words.ctypes.data, ob=obs.ctypes.data, no=3, m=mask.ctypes.data, s=st.ctypes.data):
        return L.rt_terrain_visibility_field(cs, ref(lat), ref(opt), occ, ob, no, m, s)

    def devf(lat=good, opt=None, occ=docc.data_ptr(), ob=dobs.data_ptr(), no=3, m=dmask.data_ptr(), s=dst.data_ptr(), sb=need,
             sp=scratch.data_ptr()):
        return L.rt_terrain_visibility_field_device(cs, ref(lat), ref(opt), occ, ob, no, sp, sb, m, s)

    for f in (host, devf):
        assert f(lat=None) == RT_ERR_INVALID
        for size in (0, 8, 24, 27):
            short = G.engine.visibility_options()
            short.size = size
            assert f(opt=short) == RT_ERR_INVALID and b"size" in L.rt_last_error(), size
        for flags in (2, 4, 8, 16, 32, 64, 1 << 31, 1 | 32):
            bad = G.engine.visibility_options()
            bad.flags = flags
            assert f(opt=bad) == RT_ERR_INVALID and b"flags" in L.rt_last_error(), flags
        for r in (8191, 1 << 16, 0xffffffff):  # a larger range would equal unbounded: rejected
            assert f(opt=G.engine.visibility_options(max_range=r)) == RT_ERR_INVALID and b"8190" in L.rt_last_error(), r
        for no in (0, 33, 0xffffffff):
            assert f(no=no) == RT_ERR_INVALID and b"n_observers" in L.rt_last_error(), no
        assert f(m=None) == RT_ERR_INVALID and b"null" in L.rt_last_error()
        assert f(ob=None) == RT_ERR_INVALID and b"null" in L.rt_last_error()
        for bad_dims in ((4097, 1, 1), (1, 4097, 1), (1, 1, 4097)):
            assert f(lat=G.engine.lattice((0, 0, 0), (1, 1, 1), bad_dims)) == RT_ERR_INVALID and b"4096" in L.rt_last_error()
        assert f(lat=G.engine.lattice((0, 0, 0), (1, 1, 1), (4096, 4096, 5))) == RT_ERR_INVALID and b"2^26" in L.rt_last_error()
        for bad in (float("inf"), float("nan")):
            assert f(lat=G.engine.lattice((0, bad, 0), (1, 1, 1), dims)) == RT_ERR_INVALID and b"finite" in L.rt_last_error()
        for zero in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):  # nothing to do: RT_OK, nothing launched
            assert f(lat=G.engine.lattice((0, 0, 0), (1, 1, 1), zero), occ=None) == RT_OK
    # the host form checks the observers; the device form its scratch block
    for row in ((33, 0, 0, 0), (0, 5, 0, 0), (0, 0, 3, 0), (-1, 0, 0, 0), (0, 0, 0, 1), (4096, 0, 0, 1), (0, -4096, 0, 1),
                (1, 1, 1, 2), (1, 1, 1, -1)):
        bad = np.array([(0, 0, 0, 0), row], np.int32)
        assert host(ob=bad.ctypes.data, no=2) == RT_ERR_INVALID and b"observer 1" in L.rt_last_error(), row
    assert devf(sb=need - 1) == RT_ERR_INVALID and b"scratch" in L.rt_last_error()
    assert devf(sb=0) == RT_ERR_INVALID and devf(sp=None) == RT_ERR_INVALID
    assert L.rt_terrain_visibility_field(None, ref(good), None, None, obs.ctypes.data, 3, mask.ctypes.data, None) == RT_ERR_INVALID
    # no texture bound: RT_ERR_STATE, as the other queries, with a given occupancy too
    bare = dev.create_compute()
    assert bare.create("shaders", "camerarays.hlsl", "CSMain", (16, 16, 1)) and bare.swap()
    assert L.rt_terrain_visibility_field(bare._h, ref(good), None, words.ctypes.data, obs.ctypes.data, 3, mask.ctypes.data,
                                         st.ctypes.data) == RT_ERR_STATE
    assert b"texPerm2D" in L.rt_last_error()
    dev.synchronize()
    assert (mask == POISON).all() and (st == POISON).all()
    assert (dmask.cpu().numpy().view(np.uint32) == POISON).all() and (dst.cpu().numpy().view(np.uint32) == POISON).all()
    # and the calls the errors were variations of succeed; a later, longer option block means the same
    want = _want(words, dims, obs)
    later = (C.c_uint32 * 16)()
    later[0], later[6] = 64, 4
    assert L.rt_terrain_visibility_field(cs, ref(good), C.cast(later, C.POINTER(_native.RtVisibilityOptions)), words.ctypes.data,
                                         obs.ctypes.data, 3, mask.ctypes.data, st.ctypes.data) == RT_OK
    _same(mask.reshape(3, 5, 33), _want(words, dims, obs, 4)[0])
    assert host(opt=G.engine.visibility_options(max_range=8190)) == RT_OK  # the largest range: the unbounded answer
    _same(mask.reshape(3, 5, 33), want[0])
    assert host() == RT_OK and devf() == RT_OK
    dev.synchronize()
    _same(mask.reshape(3, 5, 33), want[0])
    assert list(st) == want[1]
    _same(dmask.cpu().numpy().view(np.uint32).reshape(3, 5, 33), want[0])
    assert list(dst.cpu().numpy().view(np.uint32)) == want[1]
    dev.check()
    dev.destroy()


# --- the frame loop is undisturbed --------------------------------------------------------------
def _query(ter, k):
    """The terrain's own field with an explicit eye and a given occupancy on alternate calls: the checker's bits."""
    origin, spacing, dims = (0.7, SMALL_Y["nomadplains"], 0.7), (2.3, 2.3, 2.3), (33, 5, 3)
    words = DR.terrain_words("small-iso", origin, spacing, dims, EYE, "nomadplains")
    point, sun = _terrain_observers(words, dims, spacing)
    if k % 2:
        status = []
        m = ter.visibility_field(origin, spacing, dims, observers=[point], directions=[sun], eye=EYE, status=status)
        want = _want(words, dims, VR.observers([point], [sun]))
        _same(m, want[0], k)
        assert status == want[1]
    else:
        m = ter.visibility_field(origin, spacing, dims, directions=[sun], occupancy=words, max_range=3)
        _same(m, _want(words, dims, VR.observers((), [sun]), 3)[0], k)


def test_plain_serial_loop_is_undisturbed():
    """Six renders on a plain device, the camera alternating between two golden poses, a visibility field after
    each: as many renders prepassed on the prepass stream as without, every frame golden."""
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
    """A deferred device at two frames to a launch: a visibility field between two renders launches no pending frame
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
