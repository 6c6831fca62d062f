"""CPU tests of the path fields (rt_terrain_path_field, its _device form and rt_terrain_path_scratch_bytes,
include/frosttrace.h): the declared and exported entry points, the option struct, the scratch formula and the
argument errors that need no device, the host-only planning header under AddressSanitizer + UBSan (its own program),
engine.follow_flow, and the checker the GPU tests compare with (tests/path_ref.py) pinned by means that are not the
checker: scipy's Dijkstra on the explicit graph where scipy is installed, the closed form of the open lattice, and
hand-made cases."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dist_ref as DR
import path_ref as PR
from test_field_query_host import _struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = -1
NAMES = ("rt_terrain_path_scratch_bytes", "rt_terrain_path_field", "rt_terrain_path_field_device")
FAR = PR.FAR


# --- entry points ---------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    import gpgpuraytrace_amd as G
    from gpgpuraytrace_amd import _native
    txt = open(os.path.join(ROOT, "include", "frosttrace.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    nm = shutil.which("nm")
    assert nm
    out = subprocess.run([nm, "-D", "--defined-only", G.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", code), name
        assert name in exported and hasattr(G.lib(), name), name
        assert name in _native.SIGNATURES
    assert sorted(s for s in exported if s.startswith("rt_terrain_path_")) == sorted(NAMES)
    fields = _struct_fields(code, "rt_path_options")
    assert fields == [("size", 4), ("flags", 4), ("eye", 12), ("max_blocks", 4), ("clearance_cells", 4), ("max_cost", 4),
                      ("max_sweeps", 4)]
    struct = _native.RtPathOptions
    assert [f[0] for f in struct._fields_] == [f[0] for f in fields]
    off = 0
    for name, size in fields:
        d = getattr(struct, name)
        assert (d.offset, d.size) == (off, size), name
        off += size
    assert off == C.sizeof(struct) == 36
    m = re.search(r"#define\s+RT_PATH_FAR\s+0x([0-9A-Fa-f]+)u", code)
    assert m and int(m.group(1), 16) == _native.RT_PATH_FAR == FAR
    m = re.search(r"#define\s+RT_PATH_NONE\s+(\d+)u", code)
    assert m and int(m.group(1)) == _native.RT_PATH_NONE == PR.NONE == 255
    assert G.lib().rt_abi_version() == 9  # additive
    for meth in ("path_field", "path_field_device"):
        assert hasattr(G.Terrain, meth), meth
    for fn in ("path_options", "path_scratch_bytes", "follow_flow"):
        assert hasattr(G.engine, fn), fn
    # what the header states: the two facts about overflow, the chamfer's error, and what is out of scope
    for text in ("5 * 2^26", "far value is never", "-5.7%", "+10.6%", "(1, 1, 0)", "(1, 1/3, 1/3)", "padding bits",
                 "H + 2", "Continuing an unconverged field".lower(), "per-cell traversal weights", "diagonal moves",
                 "gravity", "any-angle", "an eye per"):
        assert text in txt, text


def _scratch(dims, clearance=0):
    nx, ny, nz = dims
    n = nx * ny * nz
    if n == 0:
        return 0
    up = lambda b: (b + 15) // 16 * 16  # noqa: E731
    occ = up((nx + 31) // 32 * ny * nz * 4)
    tiles = ((nx + 31) // 32) * ((ny + 3) // 4) * ((nz + 3) // 4)
    dist = up(occ + up(4 * n) + up(8 * n) + 4 * n) if clearance else 0
    return occ + dist + occ + up(8 * tiles) + 64


def test_scratch_bytes_and_the_argument_checks_that_need_no_device():
    import gpgpuraytrace_amd as G
    from gpgpuraytrace_amd import _native
    L = G.lib()
    for dims in ((1, 1, 1), (33, 5, 3), (70, 9, 8), (97, 1, 1), (3, 300, 2), (2, 2, 300), (256, 64, 256), (4096, 4096, 4)):
        for r in (0, 1, 2, 4095):
            assert G.engine.path_scratch_bytes((0, 0, 0), (1, 1, 1), dims, r) == _scratch(dims, r), (dims, r)
        # with a clearance: the distance field's own scratch block and a word a point on top
        assert (G.engine.path_scratch_bytes((0, 0, 0), (1, 1, 1), dims, 3) - G.engine.path_scratch_bytes((0, 0, 0), (1, 1, 1), dims)
                == (G.engine.distance_scratch_bytes((0, 0, 0), (1, 1, 1), dims) + 4 * dims[0] * dims[1] * dims[2] + 15) // 16 * 16)
    assert _scratch((256, 64, 256)) == 2 * (1 << 19) + 8 * 8192 + 64
    # nothing to do, invalid lattices and invalid options: 0
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (4097, 1, 1), (4096, 4096, 5)):
        assert G.engine.path_scratch_bytes((0, 0, 0), (1, 1, 1), dims) == 0, dims
    assert G.engine.path_scratch_bytes((0, float("nan"), 0), (1, 1, 1), (2, 2, 2)) == 0
    assert G.engine.path_scratch_bytes((0, 0, 0), (1, 1, 1), (2, 2, 2), 4096) == 0
    assert L.rt_terrain_path_scratch_bytes(None, None) == 0
    lat = G.engine.lattice((0, 0, 0), (1, 1, 1), (4, 2, 2))
    assert L.rt_terrain_path_scratch_bytes(C.byref(lat), None) == _scratch((4, 2, 2))
    opt = G.engine.path_options((1, 2, 3), 7, 900, 11, 5)
    assert (opt.size, opt.flags, list(opt.eye), opt.max_blocks, opt.clearance_cells, opt.max_cost, opt.max_sweeps) == \
        (36, _native.RT_RAYS_EYE, [1, 2, 3], 5, 7, 900, 11)
    none = G.engine.path_options()
    assert (none.size, none.flags, none.max_blocks, none.clearance_cells, none.max_cost, none.max_sweeps) == (36, 0, 0, 0, 0, 0)
    # a null compute, before anything else
    buf = np.zeros(16, np.uint32)
    p = buf.ctypes.data
    assert L.rt_terrain_path_field(None, C.byref(lat), None, None, p, 1, p, None, None) == RT_ERR_INVALID
    assert b"null" in L.rt_last_error()
    assert L.rt_terrain_path_field_device(None, C.byref(lat), None, None, p, 1, p, 1 << 20, p, None, p) == RT_ERR_INVALID
    assert not buf.any()
    # seeds as rows and as flat indices
    assert list(G.engine.seed_indices([(1, 2, 3), (0, 0, 0)], (5, 4, 6))) == [(3 * 4 + 2) * 5 + 1, 0]
    assert list(G.engine.seed_indices([7, 9], (5, 4, 6))) == [7, 9]
    with pytest.raises(ValueError):
        G.engine.seed_indices([(5, 0, 0)], (5, 4, 6))


def test_planning_header_under_sanitizers(tmp_path):
    """tests/tools/pathquery_check.cpp: rt_rayquery.h's path options, the scratch layout, the plan, the tiles' cover,
    the move tables and the flow rule.  Its own main, its own process: nothing of it is loaded into this
    interpreter."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/tools/pathquery_check.cpp"
    exe = str(tmp_path / "pathquery_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I",
                    os.path.join(ROOT, "gpgpuraytrace_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "pathquery_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("pathquery_check ok")


# --- the checker, pinned by means that are not the checker ------------------------------------------------------
def _scipy_cost(free, seeds):
    """The definition on the explicit graph: an edge a move between two passable points, scipy's Dijkstra."""
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import dijkstra
    nz, ny, nx = free.shape
    idx = np.arange(free.size).reshape(free.shape)
    rows, cols, vals = [], [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                k = abs(dx) + abs(dy) + abs(dz)
                if not k:
                    continue
                src = (slice(max(0, -dz), nz - max(0, dz)), slice(max(0, -dy), ny - max(0, dy)), slice(max(0, -dx), nx - max(0, dx)))
                dst = (slice(max(0, dz), nz - max(0, -dz)), slice(max(0, dy), ny - max(0, -dy)), slice(max(0, dx), nx - max(0, -dx)))
                ok = free[src] & free[dst]
                rows.append(idx[src][ok])
                cols.append(idx[dst][ok])
                vals.append(np.full(int(ok.sum()), 2 + k, np.float64))
    g = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(free.size, free.size))
    good = [s for s in seeds if free.reshape(-1)[s]]
    out = np.full(free.size, FAR, np.uint32)
    if good:
        d = dijkstra(g, directed=True, indices=good, min_only=True)
        out[np.isfinite(d)] = d[np.isfinite(d)].astype(np.uint32)
    return out.reshape(free.shape)


def test_checker_equals_scipy_s_dijkstra_on_the_explicit_graph():
    rng = np.random.default_rng(7)
    dims = (70, 9, 8)
    maze = PR.serpentine(dims)
    cases = [(~maze, [PR.index(dims, 0, 8, 7)]), (~maze, [PR.index(dims, 0, 0, 0), PR.index(dims, 69, 4, 4)])]
    for d, fill in (((33, 12, 9), 0.3), ((20, 20, 20), 0.85), ((9, 7, 5), 0.6)):
        free = rng.random(d[::-1]) >= fill
        seeds = [int(s) for s in rng.integers(0, free.size, 3)]
        cases.append((free, seeds))
    for free, seeds in cases:
        want = _scipy_cost(free, seeds)
        assert np.array_equal(PR.cost(free, seeds), want)
        for mc in (7, 100):
            assert np.array_equal(PR.cost(free, seeds, mc), np.where(want > mc, np.uint32(FAR), want))
    assert PR.cost(~maze, [PR.index(dims, 0, 8, 7)]).reshape(-1)[-1] == 627


def test_checker_on_the_open_lattice_in_closed_form():
    dims = (33, 5, 3)
    words = DR.pack(np.zeros((3, 5, 33), bool), dims, 1)
    z, y, x = np.meshgrid(np.arange(3), np.arange(5), np.arange(33), indexing="ij")
    for sx, sy, sz in ((16, 2, 1), (0, 0, 0), (32, 4, 2)):
        o = np.sort(np.stack([abs(x - sx), abs(y - sy), abs(z - sz)]), axis=0)
        cost, flow, reached = PR.field(words, dims, [PR.index(dims, sx, sy, sz)])
        assert cost.dtype == np.uint32 and flow.dtype == np.uint8
        assert np.array_equal(cost, (3 * o[2] + o[1] + o[0]).astype(np.uint32)) and reached == cost.size
        assert flow[sz, sy, sx] == 13 and (flow != 13).sum() == cost.size - 1 and (flow != PR.NONE).all()
    # along the x axis the flow is the face move back, code 12 (towards -x) and 14 (towards +x)
    cost, flow, _ = PR.field(words, dims, [PR.index(dims, 16, 2, 1)])
    assert (flow[1, 2, 17:] == 12).all() and (flow[1, 2, :16] == 14).all()
    # a tie takes the smallest code: (17, 3, 1) may step by (-1, -1, 0), code 9, only
    assert flow[1, 3, 17] == 9 and cost[1, 3, 17] == 4


def test_checker_on_hand_made_cases():
    dims = (9, 5, 1)
    # a wall with one hole
    blocked = np.zeros((1, 5, 9), bool)
    blocked[0, :, 4] = True
    blocked[0, 0, 4] = False
    cost, flow, reached = PR.field(DR.pack(blocked, dims), dims, [PR.index(dims, 3, 4, 0)])
    assert cost[0, 4, 3] == 0 and cost[0, 0, 4] == 3 * 3 + 4 and cost[0, 4, 5] == (3 * 3 + 4) + 4 + 3 * 3
    assert (cost[blocked] == FAR).all() and (flow[blocked] == PR.NONE).all() and reached == 45 - 4
    # a sealed pocket: far inside it
    dims = (7, 7, 1)
    blocked = np.zeros((1, 7, 7), bool)
    blocked[0, 2:5, 2:5] = True
    blocked[0, 3, 3] = False
    cost, flow, reached = PR.field(DR.pack(blocked, dims), dims, [0])
    assert cost[0, 3, 3] == FAR and flow[0, 3, 3] == PR.NONE and reached == 49 - 9
    assert cost[0, 6, 6] == 30  # three corner moves and six face moves round the block
    # seeded inside the pocket: the pocket alone
    cost, _, reached = PR.field(DR.pack(blocked, dims), dims, [PR.index(dims, 3, 3, 0)])
    assert reached == 1 and cost[0, 3, 3] == 0
    # two seeds: the nearer one wins; a duplicate changes nothing; a blocked or out-of-range seed contributes nothing
    dims = (11, 1, 1)
    free = DR.pack(np.zeros((1, 1, 11), bool), dims)
    cost, flow, _ = PR.field(free, dims, [0, 10])
    assert list(cost[0, 0]) == [0, 3, 6, 9, 12, 15, 12, 9, 6, 3, 0]
    assert list(flow[0, 0]) == [13, 12, 12, 12, 12, 12, 14, 14, 14, 14, 13]  # the tie at 5: the smallest code
    assert np.array_equal(PR.field(free, dims, [0, 10, 0, 10, 10])[0], cost)
    blocked = np.zeros((1, 1, 11), bool)
    blocked[0, 0, 10] = True
    cost, _, reached = PR.field(DR.pack(blocked, dims), dims, [0, 10, 11, 99])
    assert list(cost[0, 0]) == [0, 3, 6, 9, 12, 15, 18, 21, 24, 27, FAR] and reached == 10
    # max_cost: nothing above it, everything at or below it as without
    cost, flow, reached = PR.field(free, dims, [0], max_cost=14)
    assert list(cost[0, 0]) == [0, 3, 6, 9, 12] + [FAR] * 6 and reached == 5 and flow[0, 0, 5] == PR.NONE
    # a clearance: passable is more than R cells from every blocked point
    dims = (9, 9, 1)
    blocked = np.zeros((1, 9, 9), bool)
    blocked[0, 4, 4] = True
    ok1, ok2 = PR.passable(DR.pack(blocked, dims), dims, 1), PR.passable(DR.pack(blocked, dims), dims, 2)
    assert (~ok1).sum() == 5 and (~ok2).sum() == 13 and PR.passable(DR.pack(blocked, dims, 1), dims).sum() == 80
    # all blocked and the empty lattice
    cost, flow, reached = PR.field(DR.pack(np.ones((1, 9, 9), bool), dims), dims, [0, 5])
    assert (cost == FAR).all() and (flow == PR.NONE).all() and reached == 0
    assert PR.field(np.zeros((0,), np.uint32), (0, 3, 3), [0])[0].shape == (3, 3, 0)


def test_follow_flow_ends_on_a_seed_and_sums_to_the_cost():
    import gpgpuraytrace_amd as G
    dims = (70, 9, 8)
    words = DR.pack(PR.serpentine(dims), dims)
    seed = (0, 8, 7)
    cost, flow, _ = PR.field(words, dims, [PR.index(dims, *seed)])
    route = G.engine.follow_flow(flow, (69, 8, 7))
    assert route.shape[1] == 3 and tuple(route[0]) == (69, 8, 7) and tuple(route[-1]) == seed
    assert G.engine.path_cost_along(route) == cost[7, 8, 69] == 627
    assert (np.abs(np.diff(route, axis=0)).max(axis=1) == 1).all()  # every step a move
    assert not PR.serpentine(dims)[route[:, 2], route[:, 1], route[:, 0]].any()  # through free points only
    # costs fall along the route by each move's weight
    c = cost[route[:, 2], route[:, 1], route[:, 0]].astype(np.int64)
    assert (np.diff(c) < 0).all() and c[-1] == 0
    assert tuple(G.engine.follow_flow(flow, seed)[0]) == seed and len(G.engine.follow_flow(flow, seed)) == 1
    assert G.engine.follow_flow(flow, (3, 4, 4)).shape == (0, 3)  # inside a wall: no flow
    assert len(G.engine.follow_flow(flow, (69, 8, 7), max_len=5)) == 5
