"""CPU tests of the distance fields (rt_terrain_distance_field, its _device form and
rt_terrain_distance_scratch_bytes, include/frosttrace.h): the declared and exported entry points, the option
struct, the scratch formula and the argument errors that need no device, the host-only planning header and the x
pass's row arithmetic under AddressSanitizer + UBSan (its own program), and the checker the GPU tests compare with
(tests/dist_ref.py) pinned by means that are not the checker: a literal loop over every pair of points, shapes whose
answer is known in closed form, and scipy's Euclidean transform where scipy is installed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dist_ref as DR
from test_field_query_host import _struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = -1
NAMES = ("rt_terrain_distance_scratch_bytes", "rt_terrain_distance_field", "rt_terrain_distance_field_device")
FAR = DR.FAR


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
        assert not name.startswith(("rt_terrain_sample_", "rt_terrain_trace_"))
    assert sorted(s for s in exported if s.startswith("rt_terrain_distance_")) == sorted(NAMES)
    fields = _struct_fields(code, "rt_distance_options")
    assert fields == [("size", 4), ("flags", 4), ("eye", 12), ("max_blocks", 4), ("max_cells", 4)]
    struct = _native.RtDistanceOptions
    assert [f[0] for f in struct._fields_] == [f[0] for f in fields]
    off = 0
    for name, size in fields:
        d = getattr(struct, name)
        assert (d.offset, d.size) == (off, size), name
        off += size
    assert off == C.sizeof(struct) == 28
    m = re.search(r"#define\s+RT_DIST_FAR\s+0x([0-9A-Fa-f]+)u", code)
    assert m and int(m.group(1), 16) == _native.RT_DIST_FAR == FAR
    assert G.lib().rt_abi_version() == 9  # additive
    for meth in ("distance_field", "distance_field_device"):
        assert hasattr(G.Terrain, meth), meth
    # what the header states: the bound's direction and what is out of scope
    for text in ("UPPER bound", "one cell diagonal", "isotropic", "padding bits", "sub-cell refinement",
                 "anisotropic metric", "trilinear", "sphere-sweep", "an eye per point"):
        assert text in txt, text


def _scratch(dims):
    nx, ny, nz = dims
    n = nx * ny * nz
    if n == 0:
        return 0
    up = lambda b: (b + 15) // 16 * 16  # noqa: E731
    return up((nx + 31) // 32 * ny * nz * 4) + up(4 * n) + up(8 * n)


def test_scratch_bytes_and_the_argument_checks_that_need_no_device():
    import gpgpuraytrace_amd as G
    from gpgpuraytrace_amd import _native
    L = G.lib()
    for dims in ((1, 1, 1), (33, 5, 3), (70, 9, 8), (97, 1, 1), (3, 300, 2), (2, 2, 300), (256, 64, 256), (4096, 4096, 4)):
        assert G.engine.distance_scratch_bytes((0, 0, 0), (1, 1, 1), dims) == _scratch(dims), dims
    assert _scratch((256, 64, 256)) == (1 << 19) + 12 * (1 << 22)
    # nothing to do, and invalid lattices: 0
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (4097, 1, 1), (4096, 4096, 5)):
        assert G.engine.distance_scratch_bytes((0, 0, 0), (1, 1, 1), dims) == 0, dims
    assert G.engine.distance_scratch_bytes((0, float("nan"), 0), (1, 1, 1), (2, 2, 2)) == 0
    assert G.engine.distance_scratch_bytes((0, 0, 0), (1, float("inf"), 1), (2, 2, 2)) == 0
    assert L.rt_terrain_distance_scratch_bytes(None) == 0
    # the spacing does not enter the scratch: d2 is defined for any
    assert G.engine.distance_scratch_bytes((0, 0, 0), (0, -1, 2), (33, 5, 3)) == _scratch((33, 5, 3))
    opt = G.engine.distance_options((1, 2, 3), 7, 5)
    assert (opt.size, opt.flags, list(opt.eye), opt.max_blocks, opt.max_cells) == (28, _native.RT_RAYS_EYE, [1, 2, 3], 5, 7)
    none = G.engine.distance_options()
    assert (none.size, none.flags, none.max_blocks, none.max_cells) == (28, 0, 0, 0)
    # a null compute, before anything else
    lat = G.engine.lattice((0, 0, 0), (1, 1, 1), (4, 2, 2))
    buf = np.zeros(16, np.uint32)
    p = buf.ctypes.data
    assert L.rt_terrain_distance_field(None, C.byref(lat), None, None, p, None) == RT_ERR_INVALID
    assert b"null" in L.rt_last_error()
    assert L.rt_terrain_distance_field_device(None, C.byref(lat), None, None, p, 1 << 20, p, None) == RT_ERR_INVALID
    assert not buf.any()


def test_planning_header_under_sanitizers(tmp_path):
    """tests/tools/distquery_check.cpp: rt_rayquery.h's distance options, max_cells, the isotropy rule, the scratch
    layout, the plan and the x pass's row arithmetic against a bit-by-bit loop.  Its own main, its own process:
    nothing of it is loaded into this interpreter."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/tools/distquery_check.cpp"
    exe = str(tmp_path / "distquery_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I",
                    os.path.join(ROOT, "gpgpuraytrace_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "distquery_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("distquery_check ok")


# --- the checker, pinned by means that are not the checker ------------------------------------------------------
def _every_pair(inside):
    """The definition as a literal loop over every pair of points (Python integers)."""
    nz, ny, nx = inside.shape
    out = np.full(inside.shape, FAR, np.uint64)
    pts = [(x, y, z) for z in range(nz) for y in range(ny) for x in range(nx)]
    for (x, y, z) in pts:
        best = FAR
        for (u, v, w) in pts:
            if inside[w, v, u] != inside[z, y, x]:
                d = (u - x) ** 2 + (v - y) ** 2 + (w - z) ** 2
                if d < best:
                    best = d
        out[z, y, x] = best
    return out


def test_checker_equals_the_loop_over_every_pair():
    rng = np.random.default_rng(5)
    cases = [((9, 7, 5), 0.5), ((9, 7, 5), 0.97), ((9, 7, 5), 0.03), ((5, 1, 3), 0.5), ((1, 6, 1), 0.3), ((2, 2, 9), 0.9),
             ((7, 5, 4), 0.002), ((7, 5, 4), 0.998)]
    for dims, fill in cases:
        nx, ny, nz = dims
        inside = rng.random((nz, ny, nx)) < fill
        if fill in (0.002, 0.998):  # exactly one point of the rarer state
            inside[:] = fill > 0.5
            inside[rng.integers(nz), rng.integers(ny), rng.integers(nx)] ^= True
        assert inside.any() and not inside.all(), (dims, fill)
        pairs = _every_pair(inside)
        assert (pairs != FAR).all() and pairs.min() >= 1
        for padding in (0, 1):
            words = DR.pack(inside, dims, padding)
            assert np.array_equal(DR.unpack(words, dims), inside)
            for mc in (0, 1, 2, 3, 50):
                want = pairs if not mc else np.where(pairs > mc * mc, np.uint64(FAR), pairs)  # the definition's clause
                assert np.array_equal(DR.d2(words, dims, mc), want.astype(np.uint32)), (dims, fill, mc, padding)


def test_checker_on_a_single_voxel():
    dims = (33, 5, 3)
    nx, ny, nz = dims
    inside = np.zeros((nz, ny, nx), bool)
    inside[1, 3, 17] = True
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    want = ((x - 17) ** 2 + (y - 3) ** 2 + (z - 1) ** 2).astype(np.uint32)
    want[1, 3, 17] = 1  # the voxel's own value: its nearest outside point is a neighbour
    got = DR.d2(DR.pack(inside, dims), dims)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    dist = DR.distance(DR.pack(inside, dims), dims, (2.5, -2.5, 2.5))
    assert dist.dtype == np.float32 and dist[1, 3, 17] == np.float32(-2.5) and dist[1, 3, 18] == np.float32(2.5)
    assert dist[0, 0, 0] == np.float32(np.sqrt(np.float32(17 ** 2 + 3 ** 2 + 1))) * np.float32(2.5)
    assert (dist > 0).sum() == inside.size - 1


def test_checker_on_a_half_space_and_on_uniform_lattices():
    dims = (70, 9, 8)
    nx, ny, nz = dims
    inside = np.zeros((nz, ny, nx), bool)
    inside[:, :4, :] = True  # y < 4 is ground
    y = np.arange(ny)
    d = np.where(y < 4, 4 - y, y - 3)  # to the nearest row of the other state
    want = np.broadcast_to((d * d)[None, :, None], inside.shape).astype(np.uint32)
    assert np.array_equal(DR.d2(DR.pack(inside, dims, 1), dims), want)
    dist = DR.distance(DR.pack(inside, dims), dims, (0.5, 0.5, 0.5))
    assert np.array_equal(dist, np.broadcast_to(np.where(y < 4, -0.5 * d, 0.5 * d)[None, :, None], inside.shape).astype(np.float32))
    for fill in (False, True):
        for padding in (0, 1):
            words = DR.pack(np.full((nz, ny, nx), fill), dims, padding)
            assert (DR.d2(words, dims) == FAR).all() and (DR.d2(words, dims, 3) == FAR).all()
            dist = DR.distance(words, dims, (1, 1, 1))
            assert np.isinf(dist).all() and ((dist < 0) == fill).all()
    assert DR.d2(np.zeros((0,), np.uint32), (0, 3, 3)).shape == (3, 3, 0)


def test_checker_with_max_cells():
    dims = (33, 5, 3)
    nx, ny, nz = dims
    inside = np.zeros((nz, ny, nx), bool)
    inside[1, 2, 16] = True
    words = DR.pack(inside, dims)
    full = DR.d2(words, dims)
    for mc in (1, 2, 5000):
        got = DR.d2(words, dims, mc)
        keep = full.astype(np.int64) <= mc * mc
        assert np.array_equal(got[keep], full[keep]) and (got[~keep] == FAR).all()
        assert keep.sum() == {1: 7, 2: 31, 5000: inside.size}[mc]  # the points of a ball of that radius, clipped
        assert np.isinf(DR.distance(words, dims, (1, 1, 1), mc)[~keep]).all()
    with pytest.raises(AssertionError):
        DR.distance(words, dims, (1, 1, 2))
    with pytest.raises(AssertionError):
        DR.distance(words, dims, (0, 0, 0))


def test_checker_equals_scipy_s_euclidean_transform():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(9)
    for dims, fill in (((33, 12, 9), 0.5), ((70, 9, 8), 0.9), ((20, 20, 20), 0.05)):
        nx, ny, nz = dims
        inside = rng.random((nz, ny, nx)) < fill
        # distance_transform_edt: every non-zero point's distance to the nearest zero point
        to_out = ndi.distance_transform_edt(inside)
        to_in = ndi.distance_transform_edt(~inside)
        want = np.rint(np.where(inside, to_out, to_in) ** 2).astype(np.uint32)
        assert np.array_equal(DR.d2(DR.pack(inside, dims), dims), want), dims
