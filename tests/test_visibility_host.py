"""CPU tests of the visibility fields (rt_terrain_visibility_field, its _device form and
rt_terrain_visibility_scratch_bytes, include/frosttrace.h): the declared and exported entry points, the option
struct, the scratch formula and the argument errors that need no device, engine.pack_observers and
engine.lattice_direction, the shared walker under AddressSanitizer + UBSan (its own program), and the checker the
GPU tests compare with (tests/vis_ref.py) pinned by means that are not the checker: an exact interval test per
candidate cell with fractions.Fraction, the directional walk against the point walk, and known answers."""
import ctypes as C
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import dist_ref as DR
import vis_ref as VR
from test_field_query_host import _struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = -1
NAMES = ("rt_terrain_visibility_scratch_bytes", "rt_terrain_visibility_field", "rt_terrain_visibility_field_device")


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
    assert sorted(s for s in exported if s.startswith("rt_terrain_visibility_")) == sorted(NAMES)
    fields = _struct_fields(code, "rt_visibility_options")
    assert fields == [("size", 4), ("flags", 4), ("eye", 12), ("max_blocks", 4), ("max_range", 4)]
    struct = _native.RtVisibilityOptions
    assert [f[0] for f in struct._fields_] == [f[0] for f in fields]
    off = 0
    for name, size in fields:
        d = getattr(struct, name)
        assert (d.offset, d.size) == (off, size), name
        off += size
    assert off == C.sizeof(struct) == 28
    assert G.lib().rt_abi_version() == 9  # additive
    for meth in ("visibility_field", "visibility_field_device"):
        assert hasattr(G.Terrain, meth), meth
    for fn in ("visibility_options", "visibility_scratch_bytes", "pack_observers", "lattice_direction"):
        assert hasattr(G.engine, fn), fn
    assert (_native.RT_VIS_POINT, _native.RT_VIS_DIRECTION) == (VR.POINT, VR.DIRECTION) == (0, 1)
    # what the header states: the tie rule, the integer bound, the range's bound, and what is out of scope
    for text in ("open unit box", "|x - c| < 1/2", "(2 k + 1) / (2 |d_i|)", "symmetric", "< 2^25", "padding bits",
                 "TOWARDS the light", "2 * 4095 = 8190", "seeing\n *   nothing", "sub-cell or density-refined",
                 "observers off the\n *   lattice", "more than 32 observers", "soft visibility", "count of occluders",
                 "hierarchical", "an eye per point"):
        assert text in txt, text


def _scratch(dims):
    nx, ny, nz = dims
    if nx * ny * nz == 0:
        return 0
    up = lambda b: (b + 15) // 16 * 16  # noqa: E731
    return up((nx + 31) // 32 * ny * nz * 4) + 64


def test_scratch_bytes_and_the_argument_checks_that_need_no_device():
    import gpgpuraytrace_amd as G
    from gpgpuraytrace_amd import _native
    L = G.lib()
    for dims in ((1, 1, 1), (33, 5, 3), (70, 9, 8), (97, 1, 1), (3, 300, 2), (2, 2, 300), (256, 64, 256), (4096, 3, 2),
                 (4096, 4096, 4)):
        assert G.engine.visibility_scratch_bytes((0, 0, 0), (1, 1, 1), dims) == _scratch(dims), dims
    assert _scratch((256, 64, 256)) == (1 << 19) + 64
    # nothing to do and invalid lattices: 0
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (4097, 1, 1), (4096, 4096, 5)):
        assert G.engine.visibility_scratch_bytes((0, 0, 0), (1, 1, 1), dims) == 0, dims
    assert G.engine.visibility_scratch_bytes((0, float("nan"), 0), (1, 1, 1), (2, 2, 2)) == 0
    assert L.rt_terrain_visibility_scratch_bytes(None) == 0
    opt = G.engine.visibility_options((1, 2, 3), 32, 5)
    assert (opt.size, opt.flags, list(opt.eye), opt.max_blocks, opt.max_range) == (28, _native.RT_RAYS_EYE, [1, 2, 3], 5, 32)
    none = G.engine.visibility_options()
    assert (none.size, none.flags, none.max_blocks, none.max_range) == (28, 0, 0, 0)
    # a null compute, before anything else
    lat = G.engine.lattice((0, 0, 0), (1, 1, 1), (4, 2, 2))
    buf = np.zeros(16, np.uint32)
    p = buf.ctypes.data
    assert L.rt_terrain_visibility_field(None, C.byref(lat), None, None, p, 1, p, p) == RT_ERR_INVALID
    assert b"null" in L.rt_last_error()
    assert L.rt_terrain_visibility_field_device(None, C.byref(lat), None, None, p, 1, p, 1 << 20, p, p) == RT_ERR_INVALID
    assert not buf.any()


def test_pack_observers_and_lattice_direction():
    import gpgpuraytrace_amd as G
    E = G.engine
    dims = (5, 4, 6)
    ob = E.pack_observers([(1, 2, 3), (0, 0, 0)], [(0, 1, 0), (-3, 2, 4095)], dims)
    assert ob.dtype == np.int32 and ob.flags.c_contiguous
    assert ob.tolist() == [[1, 2, 3, 0], [0, 0, 0, 0], [0, 1, 0, 1], [-3, 2, 4095, 1]]  # the points first
    assert np.array_equal(ob, VR.observers([(1, 2, 3), (0, 0, 0)], [(0, 1, 0), (-3, 2, 4095)]))
    assert E.pack_observers(None, [(1, 1, 1)], dims).tolist() == [[1, 1, 1, 1]]
    assert E.pack_observers([(4, 3, 5)], None, dims).tolist() == [[4, 3, 5, 0]]
    assert E.pack_observers((4, 3, 5), None, dims).tolist() == [[4, 3, 5, 0]]  # one bare triple
    assert E.pack_observers([(0, 0, 0)] * 20, [(1, 0, 0)] * 12, dims).shape == (32, 4)
    for o in ob:
        assert VR.observer_valid(o, dims)
    for points, dirs in ((None, None), ([], []), ([(5, 0, 0)], None), ([(0, 4, 0)], None), ([(0, 0, 6)], None),
                         ([(-1, 0, 0)], None), (None, [(0, 0, 0)]), (None, [(4096, 0, 0)]), (None, [(0, -4096, 1)]),
                         ([(0, 0, 0)] * 20, [(1, 0, 0)] * 13), ([(0, 0)], None), (None, [(0.5, 1, 0)])):
        with pytest.raises(ValueError):
            E.pack_observers(points, dirs, dims)
    # the nearest integer direction in lattice terms: round(max_abs * v / max|v|), v = world / spacing
    assert E.lattice_direction((0, 1, 0), (1, 1, 1)) == (0, 255, 0)
    assert E.lattice_direction((0, -2, 0), (1, 1, 1), 1) == (0, -1, 0)
    assert E.lattice_direction((1, 1, 1), (2, 2, 2), 7) == (7, 7, 7)
    assert E.lattice_direction((1, 1, 1), (1, 2, 4), 100) == (100, 50, 25)  # a coarser axis takes fewer cells
    assert E.lattice_direction((1, 1, 0), (1, -1, 1), 4095) == (4095, -4095, 0)  # a negative spacing flips the axis
    assert E.lattice_direction((0.3, -0.9, 0.1), (1.5, 1.5, 1.5), 9) == (3, -9, 1)
    sun = G.camera.sun_direction(0.3)
    d = E.lattice_direction(sun, (2.0, 2.0, 2.0))
    assert max(abs(c) for c in d) == 255 and VR.observer_valid(d + (1,), dims)
    v = np.asarray(sun, np.float64) / 2.0
    assert d == tuple(int(c) for c in np.rint(255 * v / np.abs(v).max()))
    for w, s, m in (((0, 0, 0), (1, 1, 1), 255), ((1, 0, 0), (0, 1, 1), 255), ((1, 0, 0), (1, 1, 1), 0),
                    ((1, 0, 0), (1, 1, 1), 4096)):
        with pytest.raises(ValueError):
            E.lattice_direction(w, s, m)


def test_shared_walker_under_sanitizers(tmp_path):
    """tests/tools/visquery_check.cpp: rt_rayquery.h's visibility options, the observer rule, the scratch layout, the
    plan, and the walker the kernel runs against a 64-bit rational walker.  Its own main, its own process: nothing
    of it is loaded into this interpreter."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/tools/visquery_check.cpp"
    exe = str(tmp_path / "visquery_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I",
                    os.path.join(ROOT, "gpgpuraytrace_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "visquery_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("visquery_check ok")


# --- the checker, pinned by means that are not the checker ------------------------------------------------------
def _meets(o, p, c):
    """The definition, exactly: is there a t in (0, 1) with |o + t (p - o) - c| < 1/2 on all three axes?  Each axis
    gives an open interval of t; the open intervals meet iff the largest lower end is below the smallest upper end."""
    lo, hi = Fraction(0), Fraction(1)
    for i in range(3):
        d = p[i] - o[i]
        if d == 0:
            if o[i] != c[i]:  # |o_i - c_i| < 1/2 between integers: equal
                return False
            continue
        a, b = Fraction(2 * (c[i] - o[i]) - 1, 2 * d), Fraction(2 * (c[i] - o[i]) + 1, 2 * d)
        lo, hi = max(lo, min(a, b)), min(hi, max(a, b))
    return lo < hi


def test_checker_s_cells_equal_the_exact_interval_test_both_ways_round():
    dims = (6, 5, 4)
    pts = [tuple(int(v) for v in q) for q in VR._points(dims)]
    assert len(pts) == 120
    pairs = 0
    for o in pts[::7]:
        for p in pts:
            want = {c for c in pts if c != o and c != p and _meets(o, p, c)}
            fwd, back = VR.cells_between(o, p), VR.cells_between(p, o)
            assert len(set(fwd)) == len(fwd) and set(fwd) == want, (o, p)
            assert back == fwd[::-1], (o, p)  # the same cells from the other end, in the other order
            pairs += 1
    assert pairs == 18 * 120


def test_checker_s_directional_walk_is_the_point_walk_cut_at_the_lattice():
    rng = np.random.default_rng(11)
    dims = (9, 7, 6)
    inside = lambda c: all(0 <= c[i] < dims[i] for i in range(3))  # noqa: E731
    for _ in range(300):
        p = tuple(int(rng.integers(0, dims[i])) for i in range(3))
        u = (0, 0, 0)
        while u == (0, 0, 0):
            u = tuple(int(v) for v in rng.integers(-4, 5, 3))
        end = tuple(p[i] + 40 * u[i] for i in range(3))
        line = VR.cells_between(p, end) + [end]
        cut = next(i for i, c in enumerate(line) if not inside(c))
        assert VR.direction_cells(p, u, dims) == line[:cut], (p, u)


def _field(blocked, dims, points=(), directions=(), max_range=0, padding=0):
    return VR.field(DR.pack(blocked, dims, padding), dims, VR.observers(points, directions), max_range)


def test_checker_reproduces_the_known_answers():
    dims = (33, 9, 8)
    wall = np.zeros((8, 9, 33), bool)
    wall[:, :, 16] = True
    mask, st = _field(wall, dims, [(3, 4, 4)])
    assert mask.dtype == np.uint32 and mask.shape == (8, 9, 33)
    assert st == [1224, 1224, 1, 0] and (mask[:, :, :16] == 1).all() and (mask[:, :, 16] == 1).all() and not mask[:, :, 17:].any()
    wall[5, 2, 16] = False
    mask, st = _field(wall, dims, [(3, 4, 4)])
    assert st[0] == 1259 and int(mask[:, :, 17:].sum()) == 35 and (mask[:, :, :17] == 1).all()
    # the empty lattice: every bit set, the observer's own point included
    n = 33 * 9 * 8
    mask, st = _field(np.zeros((8, 9, 33), bool), dims, [(3, 4, 4), (32, 8, 7)], [(0, 1, 0), (1, 1, 1), (-3, 2, 1)])
    assert (mask == 31).all() and st == [n, 5 * n, 5, 0]
    # all blocked: the observer and its 26 neighbours (the ends are not tested); a light reaches the last layer only
    mask, st = _field(np.ones((8, 9, 33), bool), dims, [(3, 4, 4)], [(0, 1, 0)])
    seen = np.argwhere(mask & 1)
    assert len(seen) == 27 and (np.abs(seen - np.array([4, 4, 3])).max(axis=1) <= 1).all()
    assert (mask[:, 8, :] & 2).all() and not (mask[:, :8, :] & 2).any() and st == [27 + 33 * 8, 27 + 33 * 8, 2, 0]
    # direction (0, 1, 0): no blocked point above me in my column
    rng = np.random.default_rng(5)
    blocked = rng.random((8, 9, 33)) < 0.1
    mask, _ = _field(blocked, dims, (), [(0, 1, 0), (0, 7, 0), (0, -1, 0)])
    above = np.zeros_like(blocked)
    for iy in range(9):
        above[:, iy, :] = blocked[:, iy + 1:, :].any(axis=1)
    assert np.array_equal((mask & 1) != 0, ~above) and np.array_equal((mask >> 1) & 1, mask & 1)
    below = np.zeros_like(blocked)
    for iy in range(9):
        below[:, iy, :] = blocked[:, :iy, :].any(axis=1)
    assert np.array_equal((mask & 4) != 0, ~below)
    # direction (1, 1, 1): the pure diagonal, no neighbour of it
    dims = (7, 7, 7)
    blocked = np.ones((7, 7, 7), bool)
    for i in range(7):
        blocked[i, i, i] = False
    mask, _ = _field(blocked, dims, (), [(1, 1, 1)])
    assert all(mask[i, i, i] == 1 for i in range(7))
    blocked[:] = False
    blocked[4, 4, 4] = True
    mask, _ = _field(blocked, dims, (), [(1, 1, 1)])
    assert [int(mask[i, i, i]) for i in range(7)] == [0, 0, 0, 0, 1, 1, 1] and int((mask == 0).sum()) == 4
    # the range: a point observer beyond it is not seen, a caster beyond it does not count
    dims = (11, 1, 1)
    blocked = np.zeros((1, 1, 11), bool)
    blocked[0, 0, 8] = True
    mask, _ = _field(blocked, dims, [(0, 0, 0)], [(1, 0, 0)], max_range=3)
    assert list(mask[0, 0] & 1) == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert list((mask[0, 0] >> 1) & 1) == [1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1]  # 5, 6, 7 are within 3 cells of the caster
    mask, _ = _field(blocked, dims, [(0, 0, 0)], [(1, 0, 0)])
    assert list(mask[0, 0] & 1) == [1] * 9 + [0, 0] and list((mask[0, 0] >> 1) & 1) == [0] * 8 + [1, 1, 1]
    # padding bits change nothing; an invalid record sees nothing and is not counted
    dims = (33, 2, 2)
    blocked = rng.random((2, 2, 33)) < 0.2
    a = _field(blocked, dims, [(0, 0, 0)], [(1, 0, 0)])
    b = _field(blocked, dims, [(0, 0, 0)], [(1, 0, 0)], padding=1)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    obs = np.array([(0, 0, 0, 0), (33, 0, 0, 0), (1, 0, 0, 1), (0, 0, 0, 1), (1, 0, 0, 2), (0, 4096, 0, 1)], np.int32)
    mask, st = VR.field(DR.pack(blocked, dims), dims, obs)
    assert not (mask & 0b111010).any() and st[2] == 2 and np.array_equal(mask & 1, a[0] & 1) and np.array_equal((mask >> 2) & 1, (a[0] >> 1) & 1)
    assert VR.field(np.zeros((0,), np.uint32), (0, 3, 3), obs)[0].shape == (3, 3, 0)
