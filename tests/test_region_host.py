"""CPU tests of the region fields (rt_terrain_region_field, its _device form and rt_terrain_region_scratch_bytes,
include/frosttrace.h): the declared and exported entry points, the option struct, the scratch formula and the
argument errors that need no device, the host-only planning header with the shared find / unite under
AddressSanitizer + UBSan (its own program), and the checker the GPU tests compare with (tests/region_ref.py) pinned
by means that are not the checker: scipy.ndimage.label with both structures, and hand-made cases."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dist_ref as DR
import path_ref as PR
import region_ref as RR
from test_field_query_host import _struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = -1
NAMES = ("rt_terrain_region_scratch_bytes", "rt_terrain_region_field", "rt_terrain_region_field_device")
NONE = RR.NONE
SEED = 20261021
PIN_DIMS = ((70, 9, 8), (97, 13, 11))
PIN_FILLS = (0.3, 0.5, 0.75)
PIN_EXTRA_FILLS = (0.1, 0.9)


def pin_lattices():
    """The random lattices the checker is pinned on and the GPU tests run: (dims, fill, blocked), each from a
    generator of its own with the same seed.  Two more at the end, PIN_EXTRA_FILLS on the smaller lattice: without
    them the solid regions at 26 never pass 10 (9 at most) and no lattice has one region at 6."""
    out = []
    for dims, fills in ((PIN_DIMS[0], PIN_FILLS), (PIN_DIMS[1], PIN_FILLS), (PIN_DIMS[0], PIN_EXTRA_FILLS)):
        nx, ny, nz = dims
        for fill in fills:
            out.append((dims, fill, np.random.default_rng(SEED).random((nz, ny, nx)) < fill))
    return out


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
    assert sorted(s for s in exported if s.startswith("rt_terrain_region_")) == sorted(NAMES)
    fields = _struct_fields(code, "rt_region_options")
    assert fields == [("size", 4), ("flags", 4), ("eye", 12), ("max_blocks", 4), ("clearance_cells", 4), ("connectivity", 4),
                      ("state", 4)]
    struct = _native.RtRegionOptions
    assert [f[0] for f in struct._fields_] == [f[0] for f in fields]
    off = 0
    for name, size in fields:
        d = getattr(struct, name)
        assert (d.offset, d.size) == (off, size), name
        off += size
    assert off == C.sizeof(struct) == 36
    m = re.search(r"#define\s+RT_REGION_NONE\s+0x([0-9A-Fa-f]+)u", code)
    assert m and int(m.group(1), 16) == _native.RT_REGION_NONE == NONE
    assert G.lib().rt_abi_version() == 9  # additive
    for meth in ("region_field", "region_field_device"):
        assert hasattr(G.Terrain, meth), meth
    for fn in ("region_options", "region_scratch_bytes"):
        assert hasattr(G.engine, fn), fn
    # what the header states: the definition's terms and what is out of scope
    for text in ("smallest linear point index", "label[p] == p", "padding bits", "state 1 (solid)", "0 means 26",
                 "fail-safe bound", "18-connectivity", "renumbered label set", "both states in one call",
                 "across two lattices", "incremental relabelling", "walkable-surface regions"):
        assert text in txt, text


def _scratch(dims, clearance=0):
    nx, ny, nz = dims
    n = nx * ny * nz
    if n == 0:
        return 0
    up = lambda b: (b + 15) // 16 * 16  # noqa: E731
    occ = up((nx + 31) // 32 * ny * nz * 4)
    dist = up(occ + up(4 * n) + up(8 * n) + 4 * n) if clearance else 0
    return occ + dist + occ + up(4 * n) + 64


def test_scratch_bytes_and_the_argument_checks_that_need_no_device():
    import gpgpuraytrace_amd as G
    from gpgpuraytrace_amd import _native
    L = G.lib()
    for dims in ((1, 1, 1), (33, 5, 3), (70, 9, 8), (97, 1, 1), (3, 300, 2), (2, 2, 300), (256, 64, 256), (4096, 4096, 4)):
        for r in (0, 1, 2, 4095):
            assert G.engine.region_scratch_bytes((0, 0, 0), (1, 1, 1), dims, r) == _scratch(dims, r), (dims, r)
        # with a clearance: the distance field's own scratch block and a word a point on top
        assert (G.engine.region_scratch_bytes((0, 0, 0), (1, 1, 1), dims, 3) - G.engine.region_scratch_bytes((0, 0, 0), (1, 1, 1), dims)
                == (G.engine.distance_scratch_bytes((0, 0, 0), (1, 1, 1), dims) + 4 * dims[0] * dims[1] * dims[2] + 15) // 16 * 16)
    assert _scratch((256, 64, 256)) == 2 * (1 << 19) + (1 << 24) + 64
    # nothing to do, invalid lattices and invalid options: 0
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (4097, 1, 1), (4096, 4096, 5)):
        assert G.engine.region_scratch_bytes((0, 0, 0), (1, 1, 1), dims) == 0, dims
    assert G.engine.region_scratch_bytes((0, float("nan"), 0), (1, 1, 1), (2, 2, 2)) == 0
    assert G.engine.region_scratch_bytes((0, 0, 0), (1, 1, 1), (2, 2, 2), 4096) == 0
    assert L.rt_terrain_region_scratch_bytes(None, None) == 0
    lat = G.engine.lattice((0, 0, 0), (1, 1, 1), (4, 2, 2))
    assert L.rt_terrain_region_scratch_bytes(C.byref(lat), None) == _scratch((4, 2, 2))
    for bad in (G.engine.region_options(connectivity=18), G.engine.region_options(clearance=1, solid=True)):
        assert L.rt_terrain_region_scratch_bytes(C.byref(lat), C.byref(bad)) == 0
    bad = G.engine.region_options()
    bad.state = 2
    assert L.rt_terrain_region_scratch_bytes(C.byref(lat), C.byref(bad)) == 0
    opt = G.engine.region_options((1, 2, 3), 7, 6, True, 5)
    assert (opt.size, opt.flags, list(opt.eye), opt.max_blocks, opt.clearance_cells, opt.connectivity, opt.state) == \
        (36, _native.RT_RAYS_EYE, [1, 2, 3], 5, 7, 6, 1)
    none = G.engine.region_options()
    assert (none.size, none.flags, none.max_blocks, none.clearance_cells, none.connectivity, none.state) == (36, 0, 0, 0, 26, 0)
    # a null compute, before anything else
    buf = np.zeros(16, np.uint32)
    p = buf.ctypes.data
    assert L.rt_terrain_region_field(None, C.byref(lat), None, None, p, p, p) == RT_ERR_INVALID
    assert b"null" in L.rt_last_error()
    assert L.rt_terrain_region_field_device(None, C.byref(lat), None, None, p, 1 << 20, p, p, p) == RT_ERR_INVALID
    assert not buf.any()


def test_planning_header_under_sanitizers(tmp_path):
    """tests/tools/regionquery_check.cpp: rt_rayquery.h's region options, the scratch layout, the plan, the
    backward-move tables and the shared find / unite against a flood fill.  Its own main, its own process: nothing
    of it is loaded into this interpreter."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/tools/regionquery_check.cpp"
    exe = str(tmp_path / "regionquery_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I",
                    os.path.join(ROOT, "gpgpuraytrace_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "regionquery_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("regionquery_check ok")


# --- the checker, pinned by means that are not the checker ------------------------------------------------------
def _scipy_field(member, connectivity):
    """scipy.ndimage.label: it numbers the regions by their first raster occurrence, which is the region's smallest
    index, so the label of region k is the first index at which k occurs."""
    ndi = pytest.importorskip("scipy.ndimage")
    structure = ndi.generate_binary_structure(3, 3 if connectivity == 26 else 1)
    numbered, count = ndi.label(member, structure=structure)
    flat = numbered.reshape(-1)
    first = np.full(count + 1, NONE, np.uint32)
    idx = np.flatnonzero(flat)
    first[flat[idx][::-1]] = idx[::-1].astype(np.uint32)  # the last write wins: the smallest index
    sizes = np.bincount(flat, minlength=count + 1).astype(np.uint32)
    sizes[0] = 0
    largest = int(sizes[1:].max()) if count else 0
    return first[numbered], sizes[numbered], (count, int(member.sum()), largest)


def test_checker_equals_scipy_s_label_with_both_structures():
    counts = {}
    for dims, fill, blocked in pin_lattices():
        words = DR.pack(blocked, dims, 1)
        for solid in (False, True):
            for conn in (6, 26):
                got = RR.field(words, dims, 0, conn, solid)
                want = _scipy_field(blocked if solid else ~blocked, conn)
                assert got[0].dtype == got[1].dtype == np.uint32
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (dims, fill, solid, conn)
                counts[(dims, fill, solid, conn)] = got[2][0]
    # the figures measured on these lattices, free 6 / free 26 / solid 6 / solid 26
    small = PIN_DIMS[0]
    table = {0.3: (9, 1, 372, 2), 0.5: (79, 1, 78, 1), 0.75: (467, 11, 8, 1)}
    for fill, row in table.items():
        assert tuple(counts[(small, fill, s, c)] for s, c in ((False, 6), (False, 26), (True, 6), (True, 26))) == row, fill
    assert (counts[(PIN_DIMS[1], 0.75, False, 6)], counts[(PIN_DIMS[1], 0.75, False, 26)]) == (1244, 18)
    assert tuple(counts[(small, 0.1, s, c)] for s, c in ((False, 6), (False, 26), (True, 6), (True, 26))) == (1, 1, 352, 111)
    assert tuple(counts[(small, 0.9, s, c)] for s, c in ((False, 6), (False, 26), (True, 6), (True, 26))) == (369, 133, 1, 1)
    # a condition on the inputs: every family used, a state at a connectivity, has a case with more than 10 regions
    # and one with exactly 1
    for solid in (False, True):
        for conn in (6, 26):
            family = [v for (d, f, s, c), v in counts.items() if s == solid and c == conn]
            assert max(family) > 10 and 1 in family, (solid, conn, family)


def test_checker_on_hand_made_cases():
    # two points that touch only across a corner: one region at 26, two at 6
    dims = (4, 4, 4)
    free = np.zeros((4, 4, 4), bool)
    free[1, 1, 1] = free[2, 2, 2] = True
    words = DR.pack(~free, dims)
    a, b = PR.index(dims, 1, 1, 1), PR.index(dims, 2, 2, 2)
    lab, size, st = RR.field(words, dims, 0, 26)
    assert lab[1, 1, 1] == lab[2, 2, 2] == a and st == (1, 2, 2) and size[2, 2, 2] == 2
    lab, size, st = RR.field(words, dims, 0, 6)
    assert lab[1, 1, 1] == a and lab[2, 2, 2] == b and st == (2, 2, 1) and size[2, 2, 2] == 1
    assert (lab[~free] == NONE).all() and (size[~free] == 0).all()
    # the same for the solid state, from the complement
    lab, _, st = RR.field(DR.pack(free, dims), dims, 0, 6, True)
    assert lab[2, 2, 2] == b and st == (2, 2, 1)
    # the 3-D checkerboard: singletons at 6, one region at 26
    dims = (70, 9, 8)
    z, y, x = np.meshgrid(np.arange(8), np.arange(9), np.arange(70), indexing="ij")
    board = (x + y + z) % 2 == 1  # blocked
    words = DR.pack(board, dims, 1)
    lab, size, st = RR.field(words, dims, 0, 6)
    assert st == (2520, 2520, 1) and (size[~board] == 1).all()
    assert np.array_equal(lab[~board], np.flatnonzero(~board.reshape(-1)).astype(np.uint32))
    lab, size, st = RR.field(words, dims, 0, 26)
    assert st == (1, 2520, 2520) and (lab[~board] == 0).all() and (size[~board] == 2520).all()
    assert RR.field(words, dims, 0, 6, True)[2] == (2520, 2520, 1) and RR.field(words, dims, 0, 26, True)[2] == (1, 2520, 2520)
    # the serpentine maze: one free region, 17 solid ones (the walls)
    maze = PR.serpentine(dims)
    words = DR.pack(maze, dims)
    for conn in (6, 26):
        lab, _, st = RR.field(words, dims, 0, conn)
        assert st[0] == 1 and (lab[~maze] == 0).all(), conn
        assert RR.field(words, dims, 0, conn, True)[2][0] == 17, conn
    # a clearance takes the members from the path field's passable set; the empty lattice
    assert np.array_equal(RR.members(words, dims, 1), PR.passable(words, dims, 1))
    assert RR.field(np.zeros((0,), np.uint32), (0, 3, 3))[0].shape == (3, 3, 0)
    assert RR.field(np.zeros((0,), np.uint32), (0, 3, 3))[2] == (0, 0, 0)
