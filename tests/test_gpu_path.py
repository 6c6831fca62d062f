"""GPU tests of the path fields (rt_terrain_path_field and its device form, ABI 9 additive): the cost of the cheapest
3-4-5 chamfer path from seed points through the passable points of a lattice, and its first move.  Bar: every cost
word, every flow byte and status[2] equal the checker's (tests/path_ref.py: a heap Dijkstra over the definition)
bit for bit, for occupancy the caller gives and for the terrain's own, at every shape, grid and option, and a call
between two renders changes nothing about the frame loop."""
import ctypes as C

import numpy as np
import pytest

import dist_ref as DR
import path_ref as PR
import ray_fixture as RF
from test_gpu_field_query import DEFER, EYE, NEAR, SMALL, SMALL_SPACING, SMALL_Y, _golden_pair, _make, _pose
from test_gpu_parity import make

pytestmark = pytest.mark.gpu

RT_OK, RT_ERR_INVALID, RT_ERR_STATE = 0, -1, -5
FAR = PR.FAR
POISON = 0xdeadbeef
POISON8 = 0xa5
THERE = (13.0, 92.0, -9.5)  # a second eye: other octave counts, another field
MAZE = (70, 9, 8)
MAZE_SEED = (0, 8, 7)
MAZE_COST = 627  # the cheapest path to the maze's last point, the checker's figure


def _call(ter, dims, words, seeds, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), eye=None, clearance=0, max_cost=0,
          max_sweeps=0, max_blocks=0, flow=True, status=True, cs=None):
    """The C entry point with every output poisoned: (rc, cost, flow, status)."""
    import gpgpuraytrace_amd as G
    nx, ny, nz = dims
    lat = G.engine.lattice(origin, spacing, dims)
    opt = G.engine.path_options(eye, clearance, max_cost, max_sweeps, max_blocks)
    cost = np.full((nz, ny, nx), POISON, np.uint32)
    fl = np.full((nz, ny, nx), POISON8, np.uint8)
    st = np.full(4, POISON, np.uint32)
    sd = np.ascontiguousarray(seeds, np.uint32)
    if words is not None:
        words = np.ascontiguousarray(words, np.uint32)
    rc = G.lib().rt_terrain_path_field(cs or ter.camera_compute._h, C.byref(lat), C.byref(opt),
                                       words.ctypes.data if words is not None else None, sd.ctypes.data, sd.size,
                                       cost.ctypes.data, fl.ctypes.data if flow else None, st.ctypes.data if status else None)
    return rc, cost, fl, st


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = np.ascontiguousarray(got).ravel(), np.ascontiguousarray(want).ravel()
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, bad.size, bad[:8], g[bad[:4]], w[bad[:4]])


def _check(ter, dims, words, seeds, what, checker_words=None, **kw):
    """Cost, flow and status of one host call, run to convergence, against the checker, bit for bit."""
    import gpgpuraytrace_amd as G
    ref = words if checker_words is None else checker_words
    want = PR.field(ref, dims, seeds, kw.get("clearance", 0), kw.get("max_cost", 0))
    rc, cost, fl, st = _call(ter, dims, words, seeds, **kw)
    assert rc == RT_OK, (what, G.lib().rt_last_error())
    _same(cost, want[0], what)
    _same(fl, want[1], what)
    assert st[0] == 1 and st[2] == want[2] and st[3] == 0, (what, st, want[2])
    return cost, fl, st


def _ball(dims, centre, radius):
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= radius * radius


def _idx(dims, *p):
    return PR.index(dims, *p)


# --- occupancy the caller gives: no terrain in the answer ------------------------------------------------------------
def test_given_shapes_with_known_answers():
    dev, ter = _make()
    # open 33 x 5 x 3 from one seed: 3 a + b + c, a >= b >= c the sorted absolute offsets
    dims = (33, 5, 3)
    empty = DR.pack(np.zeros((3, 5, 33), bool), dims)
    cost, fl, st = _check(ter, dims, empty, [_idx(dims, 16, 2, 1)], "open")
    z, y, x = np.meshgrid(np.arange(3), np.arange(5), np.arange(33), indexing="ij")
    o = np.sort(np.stack([abs(x - 16), abs(y - 2), abs(z - 1)]), axis=0)
    assert np.array_equal(cost, (3 * o[2] + o[1] + o[0]).astype(np.uint32))
    assert fl[1, 2, 16] == 13 and fl[1, 2, 20] == 12 and fl[1, 2, 3] == 14 and st[2] == 33 * 5 * 3
    # 70 x 9 x 8 with a ball; a wall with a hole; a sealed pocket; all blocked; all free; two seeds; a duplicate
    # and a blocked seed
    dims = (70, 9, 8)
    ball = _ball(dims, (40, 4, 3), 3.3)
    _check(ter, dims, DR.pack(ball, dims), [_idx(dims, 2, 4, 4)], "ball")
    wall = np.zeros((8, 9, 70), bool)
    wall[:, :, 37] = True
    wall[5, 2, 37] = False
    cost, _, _ = _check(ter, dims, DR.pack(wall, dims), [_idx(dims, 36, 8, 0)], "wall with a hole")
    assert cost[5, 2, 37] != FAR and cost[0, 8, 38] > cost[5, 2, 37]
    pocket = np.zeros((8, 9, 70), bool)
    pocket[2:7, 2:7, 30:36] = True
    pocket[3:6, 3:6, 31:35] = False
    cost, fl, _ = _check(ter, dims, DR.pack(pocket, dims), [0], "sealed pocket")
    assert (cost[3:6, 3:6, 31:35] == FAR).all() and (fl[3:6, 3:6, 31:35] == 255).all() and cost[7, 8, 69] != FAR
    cost, fl, st = _check(ter, dims, DR.pack(np.ones((8, 9, 70), bool), dims), [0, 77], "all blocked")
    assert (cost == FAR).all() and (fl == 255).all() and st[2] == 0 and st[1] == 0
    free = DR.pack(np.zeros((8, 9, 70), bool), dims, 1)
    _, _, st = _check(ter, dims, free, [_idx(dims, 69, 8, 7)], "all free")
    assert st[2] == 70 * 9 * 8
    cost, _, _ = _check(ter, dims, free, [_idx(dims, 0, 0, 0), _idx(dims, 69, 8, 7)], "two seeds")
    assert cost[0, 0, 0] == 0 and cost[7, 8, 69] == 0
    s = _idx(dims, 2, 4, 4)
    a, _, _ = _check(ter, dims, DR.pack(ball, dims), [s, s, _idx(dims, 40, 4, 3), s], "duplicate and blocked seeds")
    b, _, _ = _check(ter, dims, DR.pack(ball, dims), [s], "ball")
    assert np.array_equal(a, b)
    dev.check()
    dev.destroy()


def test_the_serpentine_maze():
    """A wall across every x = 3 mod 4 with one gap at alternating corners: the cheapest path re-enters tiles many
    times.  The host form to convergence; the device form at the contract's sweep count; one sweep: unconverged,
    every cost an upper bound, the seed 0."""
    import torch
    import gpgpuraytrace_amd as G
    dims = MAZE
    nx, ny, nz = dims
    n = nx * ny * nz
    words = DR.pack(PR.serpentine(dims), dims, 1)
    seed = _idx(dims, *MAZE_SEED)
    want = PR.field(words, dims, [seed])
    assert want[0][want[0] != FAR].max() == MAZE_COST == want[0][nz - 1, ny - 1, nx - 1]  # (a condition on the checker)
    dev, ter = _make()
    _, _, st = _check(ter, dims, words, [seed], "maze, host")
    assert st[1] >= 3  # the maze is three tiles long
    need = G.engine.path_scratch_bytes((0, 0, 0), (1, 1, 1), dims)
    scratch = torch.zeros(need, dtype=torch.uint8, device="cuda:0")
    occ = torch.from_numpy(words.view(np.int32).copy()).to("cuda:0")
    sd = torch.tensor([seed], dtype=torch.int32, device="cuda:0")
    cost = torch.full((2, n), -559038737, dtype=torch.int32, device="cuda:0")
    fl = torch.full((2, n), POISON8, dtype=torch.uint8, device="cuda:0")
    st = torch.full((2, 4), -559038737, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for k, sweeps in enumerate((MAZE_COST // 3 + 2, 1)):
        assert ter.path_field_device((0, 0, 0), (1, 1, 1), dims, sd.data_ptr(), 1, scratch.data_ptr(), need,
                                     cost[k].data_ptr(), st[k].data_ptr(), flow_ptr=fl[k].data_ptr(),
                                     occupancy_ptr=occ.data_ptr(), max_sweeps=sweeps), G.lib().rt_last_error()
    dev.synchronize()
    got_c = cost.cpu().numpy().view(np.uint32).reshape(2, nz, ny, nx)
    got_f = fl.cpu().numpy().reshape(2, nz, ny, nx)
    got_s = st.cpu().numpy().view(np.uint32)
    _same(got_c[0], want[0], "maze, device")
    _same(got_f[0], want[1], "maze, device")
    assert list(got_s[0][[0, 2, 3]]) == [1, want[2], 0]
    print("maze: working sweeps", got_s[0][1], "one sweep reached", got_s[1][2], "of", want[2])
    assert got_s[1][0] == 0 and got_s[1][1] == 1 and got_s[1][3] == 0
    assert (got_c[1] >= want[0]).all() and got_c[1][MAZE_SEED[2], MAZE_SEED[1], MAZE_SEED[0]] == 0
    assert got_s[1][2] == (got_c[1] != FAR).sum() < want[2]
    # the host form stopped early: RT_OK, unconverged, upper bounds
    rc, c1, _, s1 = _call(ter, dims, words, [seed], max_sweeps=3)
    assert rc == RT_OK and s1[0] == 0 and 1 <= s1[1] <= 3 and (c1 >= want[0]).all() and c1.ravel()[seed] == 0
    # max_cost at a value that cuts the maze
    for mc in (300, 301, MAZE_COST - 1, MAZE_COST):
        c, _, s = _check(ter, dims, words, [seed], ("max_cost", mc), max_cost=mc)
        assert ((c == FAR) == ((want[0] == FAR) | (want[0] > mc))).all()
    assert s[2] == want[2]
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("nx", [33, 97])
def test_padding_bits_are_ignored(nx):
    dims = (nx, 3, 2)
    dev, ter = _make()
    rng = np.random.default_rng(nx)
    blocked = rng.random((2, 3, nx)) < 0.3
    blocked[0, 0, 0] = False
    out = []
    for padding in (0, 1):
        words = DR.pack(blocked, dims, padding)
        assert (words[..., -1] >> (nx % 32)).any() == bool(padding)  # (the padding is what it should be)
        out.append(_check(ter, dims, words, [0, _idx(dims, nx - 1, 2, 1)], ("padding", padding)))
        full = DR.pack(np.zeros((2, 3, nx), bool), dims, padding)
        _, _, st = _check(ter, dims, full, [_idx(dims, nx - 1, 1, 1)], ("free, padding", padding))
        assert st[2] == nx * 6
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    dev.check()
    dev.destroy()


def test_rows_of_one_point_and_columns_longer_than_any_tile():
    dev, ter = _make()
    rng = np.random.default_rng(3)
    for dims in ((1, 7, 5), (1, 1, 1), (1, 1, 9), (5, 1, 1)):
        nx, ny, nz = dims
        blocked = rng.random((nz, ny, nx)) < 0.2
        blocked.reshape(-1)[0] = False
        _check(ter, dims, DR.pack(blocked, dims, 1), [0], dims)
    for dims in ((3, 300, 2), (2, 2, 300)):
        nx, ny, nz = dims
        cost, _, _ = _check(ter, dims, DR.pack(np.zeros((nz, ny, nx), bool), dims), [0], (dims, "free"))
        assert cost.max() >= 3 * 299
        blocked = rng.random((nz, ny, nx)) < 0.25
        blocked.reshape(-1)[0] = False
        _check(ter, dims, DR.pack(blocked, dims), [0, nx * ny * nz - 1], (dims, "noise"))
    dev.check()
    dev.destroy()


def test_a_random_lattice_with_pockets_and_clearances():
    dims = (70, 24, 9)
    nx, ny, nz = dims
    rng = np.random.default_rng(11)
    blocked = rng.random((nz, ny, nx)) < 0.85
    blocked[4, 12, 35] = False
    words = DR.pack(blocked, dims, 1)
    seed = _idx(dims, 35, 12, 4)
    want = PR.field(words, dims, [seed])[0]
    free = ~blocked
    assert (want[free] != FAR).sum() > 100 and (want[free] == FAR).sum() > 10  # (the checker has both)
    dev, ter = _make()
    for mb in (0, 1, 2):
        _check(ter, dims, words, [seed], ("random", mb), max_blocks=mb)
    # clearance 1 and 2 against the checker's passable set: a few balls and a slab in an open lattice
    solid = _ball(dims, (20, 10, 4), 3.2) | _ball(dims, (45, 14, 3), 2.5)
    solid[:, :3, 50:] = True
    cwords = DR.pack(solid, dims)
    seeds = [_idx(dims, 1, 20, 7), _idx(dims, 20, 10, 4), _idx(dims, 20, 14, 4)]  # free, blocked, near the ball
    reached = []
    for r in (0, 1, 2):
        ok = PR.passable(cwords, dims, r)
        for mb in (0, 1):
            cost, _, st = _check(ter, dims, cwords, seeds, ("clearance", r, mb), clearance=r, max_blocks=mb)
            assert ((cost != FAR) <= ok).all()
        reached.append(int(st[2]))
    assert reached[0] > reached[1] > reached[2] > 0
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
        free = np.flatnonzero(~DR.unpack(words, dims).reshape(-1))
        seeds = [int(free[0]), int(free[-1])] if free.size else [0]
        cost, _, _ = _check(ter, dims, None, seeds, (land, key), checker_words=words, origin=origin, spacing=SMALL_SPACING,
                            eye=EYE)
        rc, again, _, _ = _call(ter, dims, words, seeds, origin, SMALL_SPACING)
        assert rc == RT_OK and np.array_equal(again, cost)
    dev.check()
    dev.destroy()


def test_the_near_lattice_with_two_eyes():
    import gpgpuraytrace_amd as G
    origin, spacing, dims, eye = NEAR
    nx, ny, nz = dims
    here = DR.terrain_words("near", origin, spacing, dims, eye, "nomadplains")
    there = DR.terrain_words("near-there", origin, spacing, dims, THERE, "nomadplains")
    assert not np.array_equal(here, there)
    seed = int(np.flatnonzero(PR.passable(here, dims, 2).reshape(-1))[0])  # passable at every clearance used here
    sx, sy, sz = seed % nx, seed // nx % ny, seed // (nx * ny)
    for words in (here, there):
        blocked = DR.unpack(words, dims)
        assert blocked.any() and not blocked.all() and PR.passable(words, dims, 2).reshape(-1)[seed]
    dev, ter = _make()
    _check(ter, dims, None, [seed], "near", checker_words=here, origin=origin, spacing=spacing, eye=eye)
    _check(ter, dims, None, [seed], "near there", checker_words=there, origin=origin, spacing=spacing, eye=THERE)
    for r in (1, 2):
        for mb in (0, 1, 2):
            _check(ter, dims, None, [seed], ("near, clearance", r, mb), checker_words=here, origin=origin, spacing=spacing,
                   eye=eye, clearance=r, max_blocks=mb)
    # flow=None: the cost alone, the flow array untouched, the status optional
    want = PR.field(here, dims, [seed])
    rc, cost, fl, st = _call(ter, dims, here, [seed], flow=False, status=False)
    assert rc == RT_OK and (fl == POISON8).all() and (st == POISON).all()
    _same(cost, want[0])
    # either kind of compute
    rc, cost, fl, _ = _call(ter, dims, None, [seed], origin, spacing, eye=eye, cs=ter.compute._h)
    assert rc == RT_OK
    _same(cost, want[0])
    _same(fl, want[1])
    # the Python mirror, (n, 3) seeds, and the route along the flow
    status = []
    c, f = ter.path_field(origin, spacing, dims, [(sx, sy, sz)], eye=eye, flow=True, status=status)
    _same(c, want[0])
    _same(f, want[1])
    assert status == [1, status[1], want[2], 0]
    _same(ter.path_field(origin, spacing, dims, [seed], occupancy=there, clearance=1), PR.field(there, dims, [seed], 1)[0])
    far_points = np.argwhere((c != FAR) & (c == c[c != FAR].max()))
    z, y, x = (int(v) for v in far_points[0])
    route = G.engine.follow_flow(f, (x, y, z))
    assert tuple(route[0]) == (x, y, z) and tuple(route[-1]) == (sx, sy, sz)
    assert G.engine.path_cost_along(route) == c[z, y, x]
    blocked = np.argwhere(DR.unpack(here, dims))[0]
    assert G.engine.follow_flow(f, (blocked[2], blocked[1], blocked[0])).shape == (0, 3)
    dev.check()
    dev.destroy()


# --- the device form ------------------------------------------------------------------------------------------------
def test_device_form_on_the_compute_s_stream():
    """torch-allocated arrays, filled on torch's stream and handed over and back by event, no host synchronisation
    in between.  The outputs start poisoned; a scratch block one byte short is refused and nothing is written."""
    import torch
    import gpgpuraytrace_amd as G
    origin, spacing, dims, eye = NEAR
    nx, ny, nz = dims
    n = nx * ny * nz
    words = DR.terrain_words("near", origin, spacing, dims, eye, "nomadplains")
    seed = int(np.flatnonzero(PR.passable(words, dims, 2).reshape(-1))[0])
    rng = np.random.default_rng(4)
    given = DR.pack(rng.random((nz, ny, nx)) < 0.3, dims, 1)
    given_seed = int(np.flatnonzero(~DR.unpack(given, dims).reshape(-1))[0])
    need = G.engine.path_scratch_bytes(origin, spacing, dims, 2)
    assert need > G.engine.path_scratch_bytes(origin, spacing, dims) + 16 * n
    wants = (PR.field(words, dims, [seed], 2), PR.field(given, dims, [given_seed]), PR.field(words, dims, [seed]))
    # the contract: H + 2 sweeps converge, H <= (largest finite cost) / 3
    sweeps = max(int(w[0][w[0] != FAR].max()) for w in wants) // 3 + 2
    dev, ter = _make()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        scratch = torch.zeros(need, dtype=torch.uint8, device="cuda:0")
        occ = torch.from_numpy(given.view(np.int32).copy()).to("cuda:0")
        sd = torch.tensor([seed, given_seed, -1, n], dtype=torch.int32, device="cuda:0")  # two past the lattice: skipped
        cost = torch.full((4, n), -559038737, dtype=torch.int32, device="cuda:0")
        fl = torch.full((4, n), POISON8, dtype=torch.uint8, device="cuda:0")
        st = torch.full((4, 4), -559038737, dtype=torch.int32, device="cuda:0")
        filled = torch.cuda.Event()
        filled.record(side)
        dev.wait_event(filled.cuda_event)
        sp = scratch.data_ptr()

        def run(k, seeds_ptr, ns, sb=need, **kw):
            return ter.path_field_device(origin, spacing, dims, seeds_ptr, ns, sp, sb, cost[k].data_ptr(), st[k].data_ptr(),
                                         max_sweeps=sweeps, **kw)

        assert run(0, sd.data_ptr(), 1, eye=eye, flow_ptr=fl[0].data_ptr(), clearance=2)
        assert run(1, sd.data_ptr() + 4, 3, sb=need + 64, occupancy_ptr=occ.data_ptr(), flow_ptr=fl[1].data_ptr())
        assert run(2, sd.data_ptr(), 1, eye=eye)
        # one byte short, a null block: refused, nothing written
        assert not run(3, sd.data_ptr(), 1, sb=need - 1, eye=eye, clearance=2, flow_ptr=fl[3].data_ptr())
        assert b"scratch" in G.lib().rt_last_error()
        assert not ter.path_field_device(origin, spacing, dims, sd.data_ptr(), 1, 0, need, cost[3].data_ptr(), st[3].data_ptr(),
                                         max_sweeps=sweeps)
        done = torch.cuda.Event()
        done.record(side)  # torch creates its events on first record; the device then re-records it on its stream
        dev.record_event(done.cuda_event)
        side.wait_event(done)
        got_c = cost.cpu().numpy().view(np.uint32).reshape(4, nz, ny, nx)
        got_f = fl.cpu().numpy().reshape(4, nz, ny, nx)
        got_s = st.cpu().numpy().view(np.uint32)
    for k, want in enumerate(wants):
        assert got_s[k][0] == 1 and got_s[k][2] == want[2] and got_s[k][3] == 0, (k, got_s[k])
        _same(got_c[k], want[0], k)
        if k < 2:
            _same(got_f[k], want[1], k)
    assert (got_f[2] == POISON8).all()
    assert (got_c[3] == POISON).all() and (got_f[3] == POISON8).all() and (got_s[3] == POISON).all()
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
    seeds = np.array([0, n - 1], np.uint32)
    dev, ter = _make()
    cs = ter.camera_compute._h
    cost = np.full(n, POISON, np.uint32)
    fl = np.full(n, POISON8, np.uint8)
    st = np.full(4, POISON, np.uint32)
    need = G.engine.path_scratch_bytes((0, 0, 0), (1, 1, 1), dims, 2)
    scratch = torch.zeros(need, dtype=torch.uint8, device="cuda:0")
    dcost = torch.full((n,), -559038737, dtype=torch.int32, device="cuda:0")
    dfl = torch.full((n,), POISON8, dtype=torch.uint8, device="cuda:0")
    dst = torch.full((4,), -559038737, dtype=torch.int32, device="cuda:0")
    docc = torch.from_numpy(words.view(np.int32).copy()).to("cuda:0")
    dseeds = torch.from_numpy(seeds.view(np.int32).copy()).to("cuda:0")
    torch.cuda.synchronize()
    good = G.engine.lattice((0, 0, 0), (1, 1, 1), dims)
    sweeps = G.engine.path_options(max_sweeps=64)

    def ref(o):
        return C.byref(o) if o is not None else None

    def host(lat=good, opt=None, occ=words.ctypes.data, sd=seeds.ctypes.data, ns=2, a=cost.ctypes.data, b=fl.ctypes.data,
             s=st.ctypes.data):
        return L.rt_terrain_path_field(cs, ref(lat), ref(opt), occ, sd, ns, a, b, s)

    def devf(lat=good, opt=sweeps, occ=docc.data_ptr(), sd=dseeds.data_ptr(), ns=2, a=dcost.data_ptr(), b=dfl.data_ptr(),
             s=dst.data_ptr(), sb=need):
        return L.rt_terrain_path_field_device(cs, ref(lat), ref(opt), occ, sd, ns, scratch.data_ptr(), sb, a, b, s)

    for f in (host, devf):
        assert f(lat=None) == RT_ERR_INVALID
        for size in (0, 8, 24, 28, 35):
            short = G.engine.path_options(max_sweeps=64)
            short.size = size
            assert f(opt=short) == RT_ERR_INVALID and b"size" in L.rt_last_error(), size
        for flags in (2, 4, 8, 16, 32, 64, 1 << 31, 1 | 32):
            bad = G.engine.path_options(max_sweeps=64)
            bad.flags = flags
            assert f(opt=bad) == RT_ERR_INVALID and b"flags" in L.rt_last_error(), flags
        assert f(opt=G.engine.path_options(clearance=4096, max_sweeps=64)) == RT_ERR_INVALID and b"4095" in L.rt_last_error()
        for ns in (0, (1 << 26) + 1, 0xffffffff):
            assert f(ns=ns) == RT_ERR_INVALID and b"n_seeds" in L.rt_last_error(), ns
        assert f(a=None) == RT_ERR_INVALID and b"null" in L.rt_last_error()
        assert f(sd=None) == RT_ERR_INVALID and b"null" in L.rt_last_error()
        for bad_dims in ((4097, 1, 1), (1, 4097, 1), (1, 1, 4097)):
            assert f(lat=G.engine.lattice((0, 0, 0), (1, 1, 1), bad_dims)) == RT_ERR_INVALID and b"4096" in L.rt_last_error()
        assert f(lat=G.engine.lattice((0, 0, 0), (1, 1, 1), (4096, 4096, 5))) == RT_ERR_INVALID and b"2^26" in L.rt_last_error()
        for bad in (float("inf"), float("nan")):
            assert f(lat=G.engine.lattice((0, bad, 0), (1, 1, 1), dims)) == RT_ERR_INVALID and b"finite" in L.rt_last_error()
        for zero in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):  # nothing to do: RT_OK, nothing launched
            assert f(lat=G.engine.lattice((0, 0, 0), (1, 1, 1), zero), occ=None) == RT_OK
    # the host form checks the seeds; the device form its status, its sweeps and its scratch block
    for bad_seed in (n, n + 1, 0xffffffff):
        assert host(sd=np.array([0, bad_seed], np.uint32).ctypes.data) == RT_ERR_INVALID and b"seed 1" in L.rt_last_error()
    assert devf(s=None) == RT_ERR_INVALID and b"null" in L.rt_last_error()
    for ms in (0, 4097):
        assert devf(opt=G.engine.path_options(max_sweeps=ms)) == RT_ERR_INVALID and b"max_sweeps" in L.rt_last_error()
    assert devf(opt=None) == RT_ERR_INVALID and b"max_sweeps" in L.rt_last_error()
    assert devf(sb=G.engine.path_scratch_bytes((0, 0, 0), (1, 1, 1), dims) - 1) == RT_ERR_INVALID and devf(sb=0) == RT_ERR_INVALID
    assert devf(opt=G.engine.path_options(clearance=2, max_sweeps=64), sb=need - 1) == RT_ERR_INVALID
    assert L.rt_terrain_path_field(None, ref(good), None, None, seeds.ctypes.data, 2, cost.ctypes.data, None, None) == RT_ERR_INVALID
    # no texture bound: RT_ERR_STATE, as the other queries
    bare = dev.create_compute()
    assert bare.create("shaders", "camerarays.hlsl", "CSMain", (16, 16, 1)) and bare.swap()
    assert L.rt_terrain_path_field(bare._h, ref(good), None, None, seeds.ctypes.data, 2, cost.ctypes.data, fl.ctypes.data,
                                   st.ctypes.data) == RT_ERR_STATE
    assert b"texPerm2D" in L.rt_last_error()
    dev.synchronize()
    assert (cost == POISON).all() and (fl == POISON8).all() and (st == POISON).all()
    assert (dcost.cpu().numpy().view(np.uint32) == POISON).all() and (dfl.cpu().numpy() == POISON8).all()
    assert (dst.cpu().numpy().view(np.uint32) == POISON).all()
    # and the calls the errors were variations of succeed; a later, longer option block means the same
    want = PR.field(words, dims, seeds)
    later = (C.c_uint32 * 16)()
    later[0], later[7] = 64, 20
    assert L.rt_terrain_path_field(cs, ref(good), C.cast(later, C.POINTER(_native.RtPathOptions)), words.ctypes.data,
                                   seeds.ctypes.data, 2, cost.ctypes.data, fl.ctypes.data, st.ctypes.data) == RT_OK
    _same(cost.reshape(3, 5, 33), PR.field(words, dims, seeds, 0, 20)[0])
    assert host() == RT_OK and devf() == RT_OK
    dev.synchronize()
    _same(cost.reshape(3, 5, 33), want[0])
    _same(fl.reshape(3, 5, 33), want[1])
    assert list(st[[0, 2, 3]]) == [1, want[2], 0]
    _same(dcost.cpu().numpy().view(np.uint32).reshape(3, 5, 33), want[0])
    _same(dfl.cpu().numpy().reshape(3, 5, 33), want[1])
    assert list(dst.cpu().numpy().view(np.uint32)[[0, 2, 3]]) == [1, want[2], 0]
    dev.check()
    dev.destroy()


# --- the frame loop is undisturbed --------------------------------------------------------------
def _query(ter, k):
    """The terrain's own field with an explicit eye and a given occupancy on alternate calls: the checker's bits."""
    origin, spacing, dims = (0.7, SMALL_Y["nomadplains"], 0.7), (2.3, 2.3, 2.3), (33, 5, 3)
    words = DR.terrain_words("small-iso", origin, spacing, dims, EYE, "nomadplains")
    seed = int(np.flatnonzero(~DR.unpack(words, dims).reshape(-1))[0])
    if k % 2:
        c, f = ter.path_field(origin, spacing, dims, [seed], eye=EYE, flow=True)
        want = PR.field(words, dims, [seed])
        _same(c, want[0], k)
        _same(f, want[1], k)
    else:
        _same(ter.path_field(origin, spacing, dims, [seed], occupancy=words, clearance=1), PR.field(words, dims, [seed], 1)[0], k)


def test_plain_serial_loop_is_undisturbed():
    """Six renders on a plain device, the camera alternating between two golden poses, a path field after each: as
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
    """A deferred device at two frames to a launch: a path field between two renders launches no pending frame (the
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
