"""CPU tests of the field queries (rt_terrain_sample_field*, rt_terrain_sample_lattice*, include/frosttrace.h): the
declared and exported entry points, the two structs' sizes, the host-only planning header under AddressSanitizer +
UBSan (its own program), the checker's lattice and occupancy helpers, and known answers that pin the checker the
GPU tests compare with (tests/field_ref.py) on the `testing` landscape, whose field is analytic:
d = 10 sin(0.1 x) cos(0.1 z) - y."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import field_ref as FR
import ray_fixture as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = -1
NAMES = ("rt_terrain_sample_field", "rt_terrain_sample_field_device", "rt_terrain_sample_lattice",
         "rt_terrain_sample_lattice_device")


def _struct_fields(code, name):
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + name + r"\s*;", code)
    assert m, name
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        assert ctype in ("uint32_t", "float"), decl
        for nm in names.split(","):
            a = re.match(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*$", nm)
            fields.append((a.group(1), 4 * int(a.group(2) or 1)))
    return fields


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
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in exported and hasattr(G.lib(), name), name
        assert name in _native.SIGNATURES
    assert sorted(s for s in exported if s.startswith("rt_terrain_sample_")) == sorted(NAMES)
    # the header's fields in order: the binding's names, offsets and sizes
    for cname, struct, total in (("rt_field_options", _native.RtFieldOptions, 24), ("rt_lattice", _native.RtLattice, 36)):
        fields = _struct_fields(code, cname)
        assert [f[0] for f in struct._fields_] == [f[0] for f in fields]
        off = 0
        for name, size in fields:
            d = getattr(struct, name)
            assert (d.offset, d.size) == (off, size), (cname, name)
            off += size
        assert off == C.sizeof(struct) == total
    m = re.search(r"\bRT_FIELD_NORMAL\s*=\s*(\d+)", code)
    assert m and int(m.group(1)) == _native.RT_FIELD_NORMAL == 32
    assert _native.RT_RAYS_EYE == 1
    assert G.lib().rt_abi_version() == 9  # additive
    for meth in ("sample_field", "sample_field_device", "sample_lattice", "sample_lattice_device"):
        assert hasattr(G.Terrain, meth), meth
    # what the header states: the definition's sources and what is out of scope
    for text in ("tracing.hlsl:107-116", "tracescreen.hlsl:29", "mesh extraction", "getFog", "eye", "eps",
                 "finite differences between lattice neighbours"):
        assert text in txt, text


def test_argument_checks_that_need_no_device_and_the_option_helpers():
    import gpgpuraytrace_amd as G
    from gpgpuraytrace_amd import _native
    L = G.lib()
    buf = np.zeros(8, np.float32)
    p = buf.ctypes.data
    lat = G.engine.lattice((0.7, 1, 2), (2.3, -1, 0), (33, 5, 3))
    assert (list(lat.dims), lat.origin[0], lat.spacing[0]) == ([33, 5, 3], np.float32(0.7), np.float32(2.3))
    assert L.rt_terrain_sample_field(None, p, 1, None, p) == RT_ERR_INVALID and b"null" in L.rt_last_error()
    assert L.rt_terrain_sample_field_device(None, p, 1, None, p) == RT_ERR_INVALID
    assert L.rt_terrain_sample_field(None, p, 0, None, p) == RT_ERR_INVALID  # (a null compute, whatever n)
    assert L.rt_terrain_sample_lattice(None, C.byref(lat), None, p, None) == RT_ERR_INVALID
    assert L.rt_terrain_sample_lattice_device(None, C.byref(lat), None, p, None) == RT_ERR_INVALID
    opt = G.engine.field_options((1, 2, 3), True, 5)
    assert opt.size == 24 and opt.flags == 33 and list(opt.eye) == [1, 2, 3] and opt.max_blocks == 5
    assert G.engine.field_options().flags == 0 and G.engine.field_options(normals=True).flags == _native.RT_FIELD_NORMAL
    q = G.pack_points(np.arange(6, dtype=np.float64).reshape(2, 3))
    assert q.dtype == np.float32 and q.tolist() == [[0, 1, 2, 0], [3, 4, 5, 0]] and q.flags.c_contiguous


def test_planning_header_under_sanitizers(tmp_path):
    """tests/tools/fieldquery_check.cpp: rt_rayquery.h's field options, the lattice's validation, both plans and
    the strips' cover of a lattice.  Its own main, its own process: nothing of it is loaded into this interpreter."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/tools/fieldquery_check.cpp"
    exe = str(tmp_path / "fieldquery_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I",
                    os.path.join(ROOT, "gpgpuraytrace_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "fieldquery_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("fieldquery_check ok")


# --- the checker's own helpers -----------------------------------------------------------------------------------
def test_lattice_points_are_the_fused_coordinates():
    """Spacing 2.3 and origin 0.7 are not dyadic: i * s rounded to float32 and then added differs from the single
    rounding somewhere on the axis, so a device that does not fuse fails the lattice tests."""
    x = FR.lattice_axis(0.7, 2.3, 97)
    f32 = np.float32
    unfused = (np.arange(97, dtype=f32) * f32(2.3) + f32(0.7)).astype(f32)
    assert x.dtype == f32 and x[0] == f32(0.7) and (x != unfused).any()
    assert np.array_equal(x.astype(np.float64), (np.float64(f32(0.7)) + np.arange(97) * np.float64(f32(2.3))).astype(f32))
    p = FR.lattice_points((0.7, 1, 2), (2.3, -1, 0), (33, 5, 3))
    assert p.shape == (33 * 5 * 3, 3)
    i = (2 * 5 + 3) * 33 + 7  # (ix, iy, iz) = (7, 3, 2)
    assert p[i].tolist() == [x[7], -2.0, 2.0]
    with pytest.raises(AssertionError):
        FR.lattice_axis(2.0 ** 14, 1.0, 4)
    with pytest.raises(AssertionError):
        FR.lattice_axis(0.0, 2.0 ** -13, 4)
    with pytest.raises(AssertionError):
        FR.lattice_axis(0.0, 1.0, 4097)
    with pytest.raises(AssertionError):
        FR.lattice_axis(2.0 ** -60, 2.3, 64)  # inside the stated condition, yet not exact in float64: caught by value


def test_occupancy_words():
    d = -np.ones((2, 3, 70), np.float32)
    d[1, 2, 0] = d[1, 2, 31] = d[1, 2, 32] = d[1, 2, 69] = 1
    d[0, 0, 5] = 0.0  # the surface itself is outside (d > 0)
    w = FR.occupancy_words(d, (70, 3, 2))
    assert w.shape == (2, 3, 3) and w.dtype == np.uint32
    assert w[1, 2].tolist() == [0x80000001, 1, 1 << 5] and not w[0].any() and not w[1, :2].any()
    assert FR.occupancy_words(np.ones(97, np.float32), (97, 1, 1)).ravel().tolist() == [0xffffffff] * 3 + [1]


# --- known answers that pin the checker itself, on `testing` ---------------------------------------------------
def _analytic(p):
    p = p.astype(np.float64)
    d = 10 * np.sin(0.1 * p[:, 0]) * np.cos(0.1 * p[:, 2]) - p[:, 1]
    # getNormal is the backward difference of the density: n ~ -grad d
    g = np.stack([-np.cos(0.1 * p[:, 0]) * np.cos(0.1 * p[:, 2]), np.ones(len(p)),
                  np.sin(0.1 * p[:, 0]) * np.sin(0.1 * p[:, 2])], axis=1)
    return d, g / np.linalg.norm(g, axis=1)[:, None]


def test_density_and_normal_agree_with_the_analytic_field():
    """A lattice through the surface near the eye (|p - E| < 50, so eps < 0.25 against a wavelength of 63): the
    density within 1e-4 of the analytic one (float32 sin / cos of arguments below 10), its sign the analytic sign
    wherever |d| > 1e-4, both signs present; the normals unit vectors within 0.5 degrees... of -grad d (dot >= 0.999),
    for points inside and outside alike."""
    eye = (3.0, 4.0, -2.0)
    p, r = FR.lattice("analytic", (-20.0, -12.0, -24.5), (2.3, 1.5, 2.75), (17, 16, 17), eye, "testing", normals=True)
    want, g = _analytic(p)
    r = r.reshape(-1, 4).astype(np.float64)
    err = np.abs(r[:, 3] - want)
    print("max |d - analytic| %.2e" % err.max())
    assert err.max() <= 1e-4
    clear = np.abs(want) > 1e-4
    assert np.array_equal(r[clear, 3] > 0, want[clear] > 0)
    inside = float(np.mean(r[:, 3] > 0))
    assert 0.2 <= inside <= 0.8, inside
    assert np.isfinite(r).all()
    dots = (r[:, :3] * g).sum(axis=1)
    print("min dot %.5f (inside %.5f, outside %.5f)" % (dots.min(), dots[r[:, 3] > 0].min(), dots[r[:, 3] <= 0].min()))
    assert dots.min() >= 0.999
    assert np.abs(np.linalg.norm(r[:, :3], axis=1) - 1).max() <= 2e-7
    # the densities alone are the same bits
    assert np.array_equal(FR.field(p, eye, "testing").view(np.uint32), r[:, 3].astype(np.float32).view(np.uint32))


def test_the_eye_enters_nomadplains_only_through_the_level_of_detail():
    p = FR.lattice_points((-30.0, 0.0, -30.0), (5.0, 10.0, 5.0), (12, 12, 12))
    near, far = FR.field(p, (0, 30, 0), "nomadplains"), FR.field(p, (0, 30, 6000), "nomadplains")
    assert (near.view(np.uint32) != far.view(np.uint32)).mean() > 0.9
    assert 0.1 < np.mean(near > 0) < 0.9
    for land in ("testing", "simple", "greenrocks"):
        a, b = FR.field(p[:64], (0, 30, 0), land), FR.field(p[:64], (0, 30, 6000), land)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), land


def test_fixture_sample_positions_mix_inside_and_outside():
    """The points of the GPU tests' point form: the fixture rays' last samples (hits lie inside, misses outside)."""
    for land in RF.LANDSCAPES:
        pos = RF.oracle_query(RF.F_SET, land)[0][:, :3]
        d = FR.cached("F_SET", pos, RF.eye("F0"), land)
        inside = float(np.mean(d > 0))
        print(land, "inside %.3f" % inside)
        assert 0.2 <= inside <= 0.8, (land, inside)
