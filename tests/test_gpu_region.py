"""GPU tests of the region fields (rt_terrain_region_field and its device form, ABI 9 additive): for every point of a
lattice the smallest point index of its connected region of free or of blocked points, the region's size and the
status.  Bar: every label word, size word and status word equals the checker's (tests/region_ref.py: a flood fill
over the definition) bit for bit, for occupancy the caller gives and for the terrain's own, at every shape, grid and
option; status[0] is 1 everywhere; and a call between two renders changes nothing about the frame loop."""
import ctypes as C

import numpy as np
import pytest

import dist_ref as DR
import path_ref as PR
import ray_fixture as RF
import region_ref as RR
from test_gpu_field_query import DEFER, EYE, NEAR, SMALL, SMALL_SPACING, SMALL_Y, _golden_pair, _make, _pose
from test_gpu_parity import make
from test_region_host import pin_lattices

pytestmark = pytest.mark.gpu

RT_OK, RT_ERR_INVALID, RT_ERR_STATE = 0, -1, -5
NONE = RR.NONE
POISON = 0xdeadbeef
THERE = (13.0, 92.0, -9.5)  # a second eye: other octave counts, another field
BIG, SMALLISH = (70, 9, 8), (33, 5, 3)
_WANT = {}


def _want(words, dims, clearance=0, connectivity=26, solid=False):
    """The checker's field, computed once for each input and left unchanged."""
    key = (np.ascontiguousarray(words, np.uint32).tobytes(), tuple(dims), clearance, connectivity, solid)
    if key not in _WANT:
        _WANT[key] = RR.field(words, dims, clearance, connectivity, solid)
        for a in _WANT[key][:2]:
            a.setflags(write=False)
    return _WANT[key]


def _call(ter, dims, words, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), eye=None, clearance=0, connectivity=26,
          solid=False, max_blocks=0, size=True, status=True, cs=None):
    """The C entry point with every output poisoned: (rc, label, size, status)."""
    import gpgpuraytrace_amd as G
    nx, ny, nz = dims
    lat = G.engine.lattice(origin, spacing, dims)
    opt = G.engine.region_options(eye, clearance, connectivity, solid, max_blocks)
    lab = np.full((nz, ny, nx), POISON, np.uint32)
    sz = np.full((nz, ny, nx), POISON, np.uint32)
    st = np.full(4, POISON, np.uint32)
    if words is not None:
        words = np.ascontiguousarray(words, np.uint32)
    rc = G.lib().rt_terrain_region_field(cs or ter.camera_compute._h, C.byref(lat), C.byref(opt),
                                         words.ctypes.data if words is not None else None, lab.ctypes.data,
                                         sz.ctypes.data if size else None, st.ctypes.data if status else None)
    return rc, lab, sz, st


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = np.ascontiguousarray(got).ravel(), np.ascontiguousarray(want).ravel()
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, bad.size, bad[:8], g[bad[:4]], w[bad[:4]])


def _check(ter, dims, words, what, checker_words=None, **kw):
    """Label, size and status of one host call against the checker, bit for bit."""
    import gpgpuraytrace_amd as G
    ref = words if checker_words is None else checker_words
    want = _want(ref, dims, kw.get("clearance", 0), kw.get("connectivity", 26), kw.get("solid", False))
    rc, lab, sz, st = _call(ter, dims, words, **kw)
    assert rc == RT_OK, (what, G.lib().rt_last_error())
    _same(lab, want[0], what)
    _same(sz, want[1], what)
    assert tuple(int(v) for v in st) == (1,) + want[2], (what, st, want[2])
    return lab, sz, st


def _both(ter, dims, blocked, what, padding=0):
    """Both states at both connectivities; the status words [1] of the four calls."""
    words = DR.pack(blocked, dims, padding)
    out = []
    for solid in (False, True):
        for conn in (6, 26):
            out.append(int(_check(ter, dims, words, (what, solid, conn), connectivity=conn, solid=solid)[2][1]))
    return out


def _ball(dims, centre, radius):
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= radius * radius


def _idx(dims, *p):
    return PR.index(dims, *p)


# --- occupancy the caller gives: no terrain in the answer ------------------------------------------------------------
@pytest.mark.parametrize("dims", [BIG, SMALLISH])
def test_given_shapes_with_known_answers(dims):
    nx, ny, nz = dims
    n = nx * ny * nz
    dev, ter = _make()
    empty = np.zeros((nz, ny, nx), bool)
    lab, sz, st = _check(ter, dims, DR.pack(empty, dims, 1), "all free")
    assert (lab == 0).all() and (sz == n).all() and list(st) == [1, 1, n, n]
    lab, sz, st = _check(ter, dims, DR.pack(empty, dims, 1), "all free, solid", solid=True)
    assert (lab == NONE).all() and (sz == 0).all() and list(st) == [1, 0, 0, 0]
    lab, sz, st = _check(ter, dims, DR.pack(~empty, dims), "all blocked")
    assert (lab == NONE).all() and (sz == 0).all() and list(st) == [1, 0, 0, 0]
    lab, _, st = _check(ter, dims, DR.pack(~empty, dims), "all blocked, solid", connectivity=6, solid=True)
    assert (lab == 0).all() and list(st) == [1, 1, n, n]
    ball = _ball(dims, (nx // 2 + 5, ny // 2, nz // 2), min(ny, nz) / 2 - 0.7)
    assert _both(ter, dims, ball, "ball") == [1, 1, 1, 1]
    # a wall without and with a hole
    wall = empty.copy()
    wall[:, :, nx // 2 + 2] = True
    assert _both(ter, dims, wall, "wall") == [2, 2, 1, 1]
    lab, _, _ = _check(ter, dims, DR.pack(wall, dims), "wall, labels")
    assert lab[0, 0, 0] == 0 and lab[nz - 1, ny - 1, nx - 1] == nx // 2 + 3  # the far side's first index: row 0
    wall[nz // 2, ny // 2, nx // 2 + 2] = False
    assert _both(ter, dims, wall, "wall with a hole") == [1, 1, 1, 1]
    # a sealed pocket: the inside gets its own label, the pocket's first index
    if dims == BIG:
        pocket = empty.copy()
        pocket[2:7, 2:7, 29:36] = True
        pocket[3:6, 3:6, 30:35] = False
        first = _idx(dims, 30, 3, 3)
        lab, sz, st = _check(ter, dims, DR.pack(pocket, dims), "sealed pocket")
        assert (lab[3:6, 3:6, 30:35] == first).all() and (sz[3:6, 3:6, 30:35] == 45).all() and lab[7, 8, 69] == 0
        assert list(st) == [1, 2, n - (5 * 5 * 7 - 45), n - 5 * 5 * 7]
        _check(ter, dims, DR.pack(pocket, dims), "sealed pocket, 6", connectivity=6)
    # the checkerboard: singletons at 6, one region at 26, either state
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    board = (x + y + z) % 2 == 1
    got = _both(ter, dims, board, "checkerboard", 1)
    assert got == [int((~board).sum()), 1, int(board.sum()), 1]
    dev.check()
    dev.destroy()


def test_contacts_across_tile_corners_edges_and_faces():
    """Two free points in a blocked lattice, one move apart, placed across the tile boundary at (32, 4, 4) on every
    axis along which the move steps: each of the 26 moves, so every face, edge and corner contact in every sense.
    What links them is the move between them alone."""
    dims = BIG
    dev, ter = _make()
    for dx, dy, dz, w in PR.MOVES:
        if not w:
            continue
        # along an axis the move steps on, the pair straddles the boundary; along the others it stays in the tile
        a = tuple(e - 1 if d >= 0 else e for e, d in zip((32, 4, 4), (dx, dy, dz)))
        b = (a[0] + dx, a[1] + dy, a[2] + dz)
        free = np.zeros((8, 9, 70), bool)
        free[a[2], a[1], a[0]] = free[b[2], b[1], b[0]] = True
        first = min(_idx(dims, *a), _idx(dims, *b))
        words = DR.pack(~free, dims)
        lab, sz, st = _check(ter, dims, words, ("contact", a, b))
        assert lab[a[2], a[1], a[0]] == lab[b[2], b[1], b[0]] == first and list(st) == [1, 1, 2, 2]
        _, _, st = _check(ter, dims, words, ("contact, 6", a, b), connectivity=6)
        assert st[1] == (1 if w == 3 else 2)
        _check(ter, dims, DR.pack(free, dims), ("contact, solid", a, b), solid=True, connectivity=26 if w > 3 else 6)
    # the case the definition names: (31, 3, 3) and (32, 4, 4)
    free = np.zeros((8, 9, 70), bool)
    free[3, 3, 31] = free[4, 4, 32] = True
    lab, _, st = _check(ter, dims, DR.pack(~free, dims), "corner")
    assert lab[4, 4, 32] == _idx(dims, 31, 3, 3) and st[1] == 1
    lab, _, st = _check(ter, dims, DR.pack(~free, dims), "corner, 6", connectivity=6)
    assert lab[4, 4, 32] == _idx(dims, 32, 4, 4) and st[1] == 2
    dev.check()
    dev.destroy()


def test_the_serpentine_maze():
    """A wall across every x = 3 mod 4 with one gap at alternating corners: one free region that re-enters tiles many
    times, the merge kernel's hard case; 17 solid regions."""
    dims = BIG
    maze = PR.serpentine(dims)
    dev, ter = _make()
    for conn in (6, 26):
        lab, sz, st = _check(ter, dims, DR.pack(maze, dims, 1), ("maze", conn), connectivity=conn)
        assert (lab[~maze] == 0).all() and st[1] == 1 and (sz[~maze] == (~maze).sum()).all()
        _, _, st = _check(ter, dims, DR.pack(maze, dims, 1), ("maze, solid", conn), connectivity=conn, solid=True)
        assert st[1] == 17
    dev.check()
    dev.destroy()


def test_long_chains():
    dev, ter = _make()
    # 128 tiles in a row
    dims = (4096, 3, 2)
    free = np.zeros((2, 3, 4096), bool)
    lab, sz, st = _check(ter, dims, DR.pack(free, dims), "4096 free")
    assert (lab == 0).all() and list(st) == [1, 1, 4096 * 6, 4096 * 6]
    # every x = 64 k + 63 blocked in one row only: still one region, through the other rows
    cut = free.copy()
    cut[0, 0, 63::64] = True
    lab, _, st = _check(ter, dims, DR.pack(cut, dims), "4096 cut in one row")
    assert st[1] == 1 and (lab[~cut] == 0).all()
    _check(ter, dims, DR.pack(cut, dims), "4096 cut, 6", connectivity=6)
    _, _, st = _check(ter, dims, DR.pack(cut, dims), "4096 cut, solid", solid=True)
    assert st[1] == 64
    # the row alone: 64 pieces of 63 points
    row = (4096, 1, 1)
    _, _, st = _check(ter, row, DR.pack(cut[:1, :1], row), "4096 row cut")
    assert st[1] == 64 and st[3] == 63
    # columns longer than any tile and rows of one point
    rng = np.random.default_rng(5)
    for dims in ((1, 300, 1), (1, 1, 300), (97, 1, 1)):
        nx, ny, nz = dims
        lab, _, st = _check(ter, dims, DR.pack(np.zeros((nz, ny, nx), bool), dims, 1), (dims, "free"), connectivity=6)
        assert (lab == 0).all() and st[1] == 1
        _both(ter, dims, rng.random((nz, ny, nx)) < 0.2, (dims, "noise"), 1)
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("k", range(8))
def test_random_lattices_at_every_grid(k):
    """The lattices the checker is pinned on (tests/test_region_host.py), both connectivities and both states, at
    max_blocks 0, 1 and 2: all equal to the checker, so to each other."""
    dims, fill, blocked = pin_lattices()[k]
    words = DR.pack(blocked, dims, 1)
    dev, ter = _make()
    for solid in (False, True):
        for conn in (6, 26):
            for mb in (0, 1, 2):
                _check(ter, dims, words, (dims, fill, solid, conn, mb), connectivity=conn, solid=solid, max_blocks=mb)
    dev.check()
    dev.destroy()


def _pocket_lattice():
    """test_gpu_path.py's recipe: a few balls and a slab in an open 70 x 24 x 9 lattice."""
    dims = (70, 24, 9)
    solid = _ball(dims, (20, 10, 4), 3.2) | _ball(dims, (45, 14, 3), 2.5)
    solid[:, :3, 50:] = True
    return dims, DR.pack(solid, dims)


def test_clearances_on_a_lattice_with_pockets():
    import gpgpuraytrace_amd as G
    dims, words = _pocket_lattice()
    dev, ter = _make()
    members = []
    for r in (0, 1, 2):
        for conn in (6, 26):
            for mb in (0, 1):
                _, _, st = _check(ter, dims, words, ("clearance", r, conn, mb), clearance=r, connectivity=conn, max_blocks=mb)
        members.append(int(st[2]))
    assert members[0] > members[1] > members[2] > 0
    # the random lattice of the same recipe, where a clearance splits the free space
    rng = np.random.default_rng(11)
    noise = DR.pack(rng.random((9, 24, 70)) < 0.85, dims, 1)
    for r in (0, 1):
        _check(ter, dims, noise, ("noise, clearance", r), clearance=r)
    # the solid state takes no clearance
    rc, lab, sz, st = _call(ter, dims, words, clearance=1, solid=True)
    assert rc == RT_ERR_INVALID and b"clearance" in G.lib().rt_last_error()
    assert (lab == POISON).all() and (sz == POISON).all() and (st == POISON).all()
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("nx", [33, 64, 70, 97])
def test_padding_bits_are_ignored(nx):
    dims = (nx, 5, 3)
    dev, ter = _make()
    rng = np.random.default_rng(nx)
    blocked = rng.random((3, 5, nx)) < 0.4
    out = []
    for padding in (0, 1):
        words = DR.pack(blocked, dims, padding)
        if nx % 32:
            assert (words[..., -1] >> (nx % 32)).any() == bool(padding)  # (the padding is what it should be)
        out.append([_check(ter, dims, words, ("padding", padding, solid), solid=solid) for solid in (False, True)])
        _, _, st = _check(ter, dims, DR.pack(np.zeros((3, 5, nx), bool), dims, padding), ("free, padding", padding), solid=True)
        assert st[2] == 0
        _, _, st = _check(ter, dims, DR.pack(np.ones((3, 5, nx), bool), dims, padding), ("blocked, padding", padding), solid=True)
        assert st[2] == nx * 15
    for s in (0, 1):
        assert np.array_equal(out[0][s][0], out[1][s][0]) and np.array_equal(out[0][s][1], out[1][s][1])
    dev.check()
    dev.destroy()


# --- the terrain's own occupancy ------------------------------------------------------------------------------------
@pytest.mark.parametrize("land", RF.LANDSCAPES)
def test_small_terrain_lattices(land):
    origin = (0.7, SMALL_Y[land], 0.7)
    dev, ter = _make(land)
    for dims in SMALL:
        key = "small%dx%dx%d" % dims
        words = DR.terrain_words(key, origin, SMALL_SPACING, dims, EYE, land)
        for solid in (False, True):
            lab, _, _ = _check(ter, dims, None, (land, key, solid), checker_words=words, origin=origin, spacing=SMALL_SPACING,
                               eye=EYE, solid=solid)
            rc, again, _, _ = _call(ter, dims, words, origin, SMALL_SPACING, solid=solid)
            assert rc == RT_OK and np.array_equal(again, lab)
    dev.check()
    dev.destroy()


def test_the_near_lattice_with_two_eyes():
    origin, spacing, dims, eye = NEAR
    here = DR.terrain_words("near", origin, spacing, dims, eye, "nomadplains")
    there = DR.terrain_words("near-there", origin, spacing, dims, THERE, "nomadplains")
    assert not np.array_equal(here, there)
    assert _want(here, dims, 0, 6)[2][0] != _want(here, dims, 0, 26)[2][0]  # (a condition on the checker: 3 against 2)
    dev, ter = _make()
    for conn in (6, 26):
        _check(ter, dims, None, ("near", conn), checker_words=here, origin=origin, spacing=spacing, eye=eye, connectivity=conn)
    _check(ter, dims, None, "near, solid", checker_words=here, origin=origin, spacing=spacing, eye=eye, solid=True)
    _check(ter, dims, None, "near there", checker_words=there, origin=origin, spacing=spacing, eye=THERE)
    # either kind of compute
    want = _want(here, dims)
    rc, lab, sz, st = _call(ter, dims, None, origin, spacing, eye=eye, cs=ter.compute._h)
    assert rc == RT_OK and list(st) == [1] + list(want[2])
    _same(lab, want[0])
    _same(sz, want[1])
    # the Python mirror
    status = []
    lab, sz = ter.region_field(origin, spacing, dims, eye=eye, sizes=True, status=status)
    _same(lab, want[0])
    _same(sz, want[1])
    assert status == [1] + list(want[2])
    _same(ter.region_field(origin, spacing, dims, occupancy=there, connectivity=6, solid=True), _want(there, dims, 0, 6, True)[0])
    dev.check()
    dev.destroy()


def test_agreement_with_the_path_field():
    """For the free state at connectivity 26 a region is a set of points with a finite path cost from one another:
    from one seed in each of up to 8 regions the path field is finite exactly where the label is the seed's."""
    origin, spacing, dims, eye = NEAR
    here = DR.terrain_words("near", origin, spacing, dims, eye, "nomadplains")
    pdims, pwords = _pocket_lattice()
    noise = DR.pack(np.random.default_rng(11).random((9, 24, 70)) < 0.85, pdims, 1)
    dev, ter = _make()
    for d, words in ((dims, here), (pdims, pwords), (pdims, noise)):
        for r in (0, 2):
            lab = ter.region_field((0, 0, 0), (1, 1, 1), d, occupancy=words, clearance=r)
            roots = np.flatnonzero(lab.reshape(-1) == np.arange(lab.size, dtype=np.uint32))
            for root in roots[:8]:
                members = np.flatnonzero(lab.reshape(-1) == root)
                seed = int(members[len(members) // 2])
                cost = ter.path_field((0, 0, 0), (1, 1, 1), d, [seed], occupancy=words, clearance=r)
                assert np.array_equal(cost != PR.FAR, lab == root), (d, r, root)
    dev.check()
    dev.destroy()


def test_each_output_alone():
    dims, fill, blocked = pin_lattices()[2]
    words = DR.pack(blocked, dims, 1)
    want = _want(words, dims)
    dev, ter = _make()
    # label only: nothing is counted, size and status untouched
    rc, lab, sz, st = _call(ter, dims, words, size=False, status=False)
    assert rc == RT_OK and (sz == POISON).all() and (st == POISON).all()
    _same(lab, want[0])
    # size without status, status without size
    rc, lab, sz, st = _call(ter, dims, words, status=False)
    assert rc == RT_OK and (st == POISON).all()
    _same(lab, want[0])
    _same(sz, want[1])
    rc, lab, sz, st = _call(ter, dims, words, size=False)
    assert rc == RT_OK and (sz == POISON).all() and list(st) == [1] + list(want[2])
    _same(lab, want[0])
    _same(ter.region_field((0, 0, 0), (1, 1, 1), dims, occupancy=words), want[0])
    dev.check()
    dev.destroy()


# --- the device form ------------------------------------------------------------------------------------------------
def test_device_form_on_the_compute_s_stream():
    """torch-allocated arrays, filled on torch's stream and handed over and back by event, no host synchronisation
    in between.  Two calls into two buffers with the scratch block filled with 0xA5 before each; a scratch block one
    byte short is refused and nothing is written."""
    import torch
    import gpgpuraytrace_amd as G
    origin, spacing, dims, eye = NEAR
    nx, ny, nz = dims
    n = nx * ny * nz
    words = DR.terrain_words("near", origin, spacing, dims, eye, "nomadplains")
    given = DR.pack(np.random.default_rng(4).random((nz, ny, nx)) < 0.6, dims, 1)
    need = G.engine.region_scratch_bytes(origin, spacing, dims, 2)
    assert need > G.engine.region_scratch_bytes(origin, spacing, dims) + 16 * n
    wants = (_want(words, dims, 2), _want(given, dims, 0, 6, True), _want(words, dims))
    dev, ter = _make()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        scratch = torch.zeros(need, dtype=torch.uint8, device="cuda:0")
        occ = torch.from_numpy(given.view(np.int32).copy()).to("cuda:0")
        lab = torch.full((4, n), -559038737, dtype=torch.int32, device="cuda:0")
        sz = torch.full((4, n), -559038737, dtype=torch.int32, device="cuda:0")
        st = torch.full((4, 4), -559038737, dtype=torch.int32, device="cuda:0")
        sp = scratch.data_ptr()

        def run(k, sb=need, size=True, status=True, **kw):
            scratch.fill_(0xA5)
            filled = torch.cuda.Event()
            filled.record(side)
            dev.wait_event(filled.cuda_event)
            ok = ter.region_field_device(origin, spacing, dims, sp, sb, lab[k].data_ptr(), sz[k].data_ptr() if size else 0,
                                         st[k].data_ptr() if status else 0, **kw)
            done = torch.cuda.Event()
            done.record(side)  # torch creates its events on first record; the device then re-records it on its stream
            dev.record_event(done.cuda_event)
            side.wait_event(done)
            return ok

        assert run(0, eye=eye, clearance=2)
        assert run(1, sb=need + 64, occupancy_ptr=occ.data_ptr(), connectivity=6, solid=True)
        assert run(2, size=False, status=False, eye=eye)
        # one byte short, a null block: refused, nothing written
        assert not run(3, sb=need - 1, eye=eye, clearance=2)
        assert b"scratch" in G.lib().rt_last_error()
        assert not ter.region_field_device(origin, spacing, dims, 0, need, lab[3].data_ptr(), sz[3].data_ptr(), st[3].data_ptr())
        got_l = lab.cpu().numpy().view(np.uint32).reshape(4, nz, ny, nx)
        got_z = sz.cpu().numpy().view(np.uint32).reshape(4, nz, ny, nx)
        got_s = st.cpu().numpy().view(np.uint32)
    for k, want in enumerate(wants):
        _same(got_l[k], want[0], k)
        if k < 2:
            _same(got_z[k], want[1], k)
            assert list(got_s[k]) == [1] + list(want[2]), (k, got_s[k])
    assert (got_z[2] == POISON).all() and (got_s[2] == POISON).all()
    assert (got_l[3] == POISON).all() and (got_z[3] == POISON).all() and (got_s[3] == POISON).all()
    dev.check()
    dev.destroy()


# --- errors ---------------------------------------------------------------------------------------------------------
def test_every_argument_error_returns_its_code_and_writes_nothing():
    import torch
    import gpgpuraytrace_amd as G
    from gpgpuraytrace_amd import _native
    L = G.lib()
    dims = SMALLISH
    n = 33 * 5 * 3
    words = DR.pack(_ball(dims, (16, 2, 1), 1.5), dims)
    dev, ter = _make()
    cs = ter.camera_compute._h
    lab = np.full(n, POISON, np.uint32)
    sz = np.full(n, POISON, np.uint32)
    st = np.full(4, POISON, np.uint32)
    need = G.engine.region_scratch_bytes((0, 0, 0), (1, 1, 1), dims, 2)
    scratch = torch.zeros(need, dtype=torch.uint8, device="cuda:0")
    dlab = torch.full((n,), -559038737, dtype=torch.int32, device="cuda:0")
    dsz = torch.full((n,), -559038737, dtype=torch.int32, device="cuda:0")
    dst = torch.full((4,), -559038737, dtype=torch.int32, device="cuda:0")
    docc = torch.from_numpy(words.view(np.int32).copy()).to("cuda:0")
    torch.cuda.synchronize()
    good = G.engine.lattice((0, 0, 0), (1, 1, 1), dims)

    def ref(o):
        return C.byref(o) if o is not None else None

    def host(lat=good, opt=None, occ=words.ctypes.data, a=lab.ctypes.data, b=sz.ctypes.data, s=st.ctypes.data):
        return L.rt_terrain_region_field(cs, ref(lat), ref(opt), occ, a, b, s)

    def devf(lat=good, opt=None, occ=docc.data_ptr(), a=dlab.data_ptr(), b=dsz.data_ptr(), s=dst.data_ptr(), sb=need):
        return L.rt_terrain_region_field_device(cs, ref(lat), ref(opt), occ, scratch.data_ptr(), sb, a, b, s)

    for f in (host, devf):
        assert f(lat=None) == RT_ERR_INVALID
        for size in (0, 8, 24, 28, 35):
            short = G.engine.region_options()
            short.size = size
            assert f(opt=short) == RT_ERR_INVALID and b"size" in L.rt_last_error(), size
        for flags in (2, 4, 8, 16, 32, 64, 1 << 31, 1 | 32):
            bad = G.engine.region_options()
            bad.flags = flags
            assert f(opt=bad) == RT_ERR_INVALID and b"flags" in L.rt_last_error(), flags
        assert f(opt=G.engine.region_options(clearance=4096)) == RT_ERR_INVALID and b"4095" in L.rt_last_error()
        for conn in (1, 4, 18, 27, 0xffffffff):
            assert f(opt=G.engine.region_options(connectivity=conn)) == RT_ERR_INVALID and b"connectivity" in L.rt_last_error()
        for state in (2, 3, 0xffffffff):
            bad = G.engine.region_options()
            bad.state = state
            assert f(opt=bad) == RT_ERR_INVALID and b"state" in L.rt_last_error(), state
        assert f(opt=G.engine.region_options(clearance=1, solid=True)) == RT_ERR_INVALID and b"clearance" in L.rt_last_error()
        assert f(a=None) == RT_ERR_INVALID and b"null" in L.rt_last_error()
        for bad_dims in ((4097, 1, 1), (1, 4097, 1), (1, 1, 4097)):
            assert f(lat=G.engine.lattice((0, 0, 0), (1, 1, 1), bad_dims)) == RT_ERR_INVALID and b"4096" in L.rt_last_error()
        assert f(lat=G.engine.lattice((0, 0, 0), (1, 1, 1), (4096, 4096, 5))) == RT_ERR_INVALID and b"2^26" in L.rt_last_error()
        for bad in (float("inf"), float("nan")):
            assert f(lat=G.engine.lattice((0, bad, 0), (1, 1, 1), dims)) == RT_ERR_INVALID and b"finite" in L.rt_last_error()
        for zero in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):  # nothing to do: RT_OK, nothing launched
            assert f(lat=G.engine.lattice((0, 0, 0), (1, 1, 1), zero), occ=None) == RT_OK
    # the device form checks its scratch block
    assert devf(sb=G.engine.region_scratch_bytes((0, 0, 0), (1, 1, 1), dims) - 1) == RT_ERR_INVALID and devf(sb=0) == RT_ERR_INVALID
    assert devf(opt=G.engine.region_options(clearance=2), sb=need - 1) == RT_ERR_INVALID and b"scratch" in L.rt_last_error()
    assert L.rt_terrain_region_field(None, ref(good), None, None, lab.ctypes.data, None, None) == RT_ERR_INVALID
    # no texture bound: RT_ERR_STATE, as the other queries
    bare = dev.create_compute()
    assert bare.create("shaders", "camerarays.hlsl", "CSMain", (16, 16, 1)) and bare.swap()
    assert L.rt_terrain_region_field(bare._h, ref(good), None, None, lab.ctypes.data, sz.ctypes.data, st.ctypes.data) == RT_ERR_STATE
    assert b"texPerm2D" in L.rt_last_error()
    dev.synchronize()
    assert (lab == POISON).all() and (sz == POISON).all() and (st == POISON).all()
    assert (dlab.cpu().numpy().view(np.uint32) == POISON).all() and (dsz.cpu().numpy().view(np.uint32) == POISON).all()
    assert (dst.cpu().numpy().view(np.uint32) == POISON).all()
    # and the calls the errors were variations of succeed; a later, longer option block means the same
    later = (C.c_uint32 * 16)()
    later[0], later[7] = 64, 6
    assert L.rt_terrain_region_field(cs, ref(good), C.cast(later, C.POINTER(_native.RtRegionOptions)), words.ctypes.data,
                                     lab.ctypes.data, sz.ctypes.data, st.ctypes.data) == RT_OK
    _same(lab.reshape(3, 5, 33), _want(words, dims, 0, 6)[0])
    want = _want(words, dims)
    assert host() == RT_OK and devf() == RT_OK
    dev.synchronize()
    _same(lab.reshape(3, 5, 33), want[0])
    _same(sz.reshape(3, 5, 33), want[1])
    assert list(st) == [1] + list(want[2])
    _same(dlab.cpu().numpy().view(np.uint32).reshape(3, 5, 33), want[0])
    _same(dsz.cpu().numpy().view(np.uint32).reshape(3, 5, 33), want[1])
    assert list(dst.cpu().numpy().view(np.uint32)) == [1] + list(want[2])
    dev.check()
    dev.destroy()


# --- the frame loop is undisturbed --------------------------------------------------------------
def _query(ter, k):
    """The terrain's own field with an explicit eye and a given occupancy on alternate calls: the checker's bits."""
    origin, spacing, dims = (0.7, SMALL_Y["nomadplains"], 0.7), (2.3, 2.3, 2.3), (33, 5, 3)
    words = DR.terrain_words("small-iso", origin, spacing, dims, EYE, "nomadplains")
    if k % 2:
        lab, sz = ter.region_field(origin, spacing, dims, eye=EYE, sizes=True)
        want = _want(words, dims)
        _same(lab, want[0], k)
        _same(sz, want[1], k)
    else:
        _same(ter.region_field(origin, spacing, dims, occupancy=words, clearance=1, connectivity=6), _want(words, dims, 1, 6)[0], k)


def test_plain_serial_loop_is_undisturbed():
    """Six renders on a plain device, the camera alternating between two golden poses, a region field after each: as
    many renders prepassed on the prepass stream as without, every frame golden."""
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
    """A deferred device at two frames to a launch: a region field between two renders launches no pending frame (the
    same deferred_fused and launch_info as without), and the frames are golden."""
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
