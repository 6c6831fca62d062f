"""CPU tests of the ray queries (rt_terrain_trace_rays*, include/frosttrace.h): the exact-camera fixture the GPU
tests rest on (tests/ray_fixture.py), pack_rays, the declared and exported entry points, the argument checks that
need no device, and the host-only planning header under AddressSanitizer + UBSan (its own program)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ray_fixture as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = -1


@pytest.mark.parametrize("name", sorted(RF.CAMERAS))
def test_fixture_cameras_are_exact(name):
    """rays() asserts that the float32 evaluation of getPixelRay and p - Eye rounds nowhere."""
    o, d = RF.rays(name)
    assert o.shape == d.shape == (1024, 3) and o.dtype == d.dtype == np.float32
    e = RF.eye(name)
    assert np.array_equal(d, o - e)
    if name == "Z":
        assert not d.any() and np.array_equal(o, np.tile(e, (1024, 1)))
    else:
        assert np.all(np.abs(d).sum(axis=1) > 0)
    if name in ("F2", "G"):
        t = np.array(RF.CAMERAS[name][1], np.float32)
        assert not np.array_equal(t, e)  # the origin is not the eye
    # the bench's shifted cameras are exact too
    if name == "F0":
        for k in (1, 7, 23):
            RF.rays("F0", shift=(8 * k, 0, 8 * k))


def test_fixture_screen_coordinates():
    sx, sy = RF.screen_coords()
    # 31 * float32(1/31) rounds to 1, so the last column is pixel 256 (as camerarays.hlsl computes it)
    assert sx[0] == np.float32(-1 + 1 / 256) and sx[31] == np.float32(1 + 1 / 256) and sx[32] == sx[0]
    assert sy[0] == sx[0] and sy[31] == sy[0] and sy[32] > sy[0] and sy[1023] == sx[31]
    assert np.all(np.diff(sx[:32]) > 0)
    assert len(np.unique(sx)) == 32 and len(np.unique(sy)) == 32


@pytest.mark.parametrize("land", RF.LANDSCAPES)
def test_f_set_mixes_hits_and_misses(land):
    """Between 25% and 75% of the F0-F3 query hits on every landscape, so neither outcome can hide."""
    res, steps = RF.oracle_query(RF.F_SET, land)
    assert res.shape == (4096, 4) and steps.shape == (4096,)
    hits = float(np.mean(res[:, 3] < RF.FAR))
    print(land, "hits %.3f" % hits, "steps %d..%d" % (steps.min(), steps.max()))
    assert 0.25 <= hits <= 0.75, hits
    assert steps.max() > 20 * max(int(steps.min()), 1)  # rays of very different lengths


@pytest.mark.parametrize("land", RF.LANDSCAPES)
def test_zero_direction_oracle(land):
    res, steps = RF.oracle("Z", land)
    assert np.array_equal(res, np.tile(np.array([0, 0, 0, 0.01], np.float32), (1024, 1))) and not steps.any()


def test_pack_rays_layout():
    import gpgpuraytrace_amd as G
    assert "pack_rays" in G.__all__
    o = np.arange(15, dtype=np.float64).reshape(5, 3)
    d = -np.arange(15, dtype=np.float32).reshape(5, 3) - 1
    p = G.pack_rays(o, d)
    assert p.shape == (5, 8) and p.dtype == np.float32 and p.flags.c_contiguous
    assert np.array_equal(p[:, 0:3], o.astype(np.float32)) and np.array_equal(p[:, 4:7], d)
    assert not p[:, 3].any() and not p[:, 7].any()
    assert G.pack_rays(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 8)
    assert G.pack_rays([1, 2, 3], [4, 5, 6]).tolist() == [[1, 2, 3, 0, 4, 5, 6, 0]]
    with pytest.raises(ValueError):
        G.pack_rays(np.zeros((2, 3)), np.zeros((3, 3)))


def test_header_declares_and_library_exports_the_entry_points():
    """Fails without the feature: the library exports both calls, the header declares them and the option
    block, and the binding's struct and flags match the header."""
    import gpgpuraytrace_amd as G
    from gpgpuraytrace_amd import _native
    txt = open(os.path.join(ROOT, "include", "frosttrace.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("rt_terrain_trace_rays", "rt_terrain_trace_rays_device"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(G.lib(), name), name
        assert name in _native.SIGNATURES
    assert re.search(r"\}\s*rt_ray_options\s*;", code)
    for flag in ("RT_RAYS_EYE", "RT_RAYS_FORCE_SEGMENTS", "RT_RAYS_FORCE_LANES"):
        m = re.search(r"\b" + flag + r"\s*=\s*(\d+)", code)
        assert m and int(m.group(1)) == getattr(_native, flag), flag
    assert C.sizeof(_native.RtRayOptions) == 24
    assert [f[0] for f in _native.RtRayOptions._fields_] == ["size", "flags", "eye", "max_blocks"]
    assert G.lib().rt_abi_version() == 9  # additive
    assert hasattr(G.Terrain, "trace_rays") and hasattr(G.Terrain, "trace_rays_device")
    assert "camerarays.hlsl:12-21" in txt and "tracing.hlsl:47-105" in txt


def test_argument_checks_that_need_no_device():
    import gpgpuraytrace_amd as G
    L = G.lib()
    buf = np.zeros(8, np.float32)
    p = buf.ctypes.data
    assert L.rt_terrain_trace_rays(None, p, p, 1, None, p, None) == RT_ERR_INVALID and b"null" in L.rt_last_error()
    assert L.rt_terrain_trace_rays_device(None, p, 1, None, p, None) == RT_ERR_INVALID
    assert L.rt_terrain_trace_rays(None, p, p, 0, None, p, None) == RT_ERR_INVALID  # (a null compute, whatever n)
    with pytest.raises(ValueError):
        G.engine.ray_options(None, "fastest", 0)
    opt = G.engine.ray_options((1, 2, 3), "lanes", 5)
    assert opt.size == 24 and opt.flags == 5 and list(opt.eye) == [1, 2, 3] and opt.max_blocks == 5
    assert G.engine.ray_options().flags == 0


def test_planning_header_under_sanitizers(tmp_path):
    """tests/tools/rayquery_check.cpp: rt_rayquery.h's option parsing (never past the caller's size), count
    limits, shape and lanes-per-ray ladder, grids and packing.  Its own main, its own process: nothing of it is
    loaded into this interpreter."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/tools/rayquery_check.cpp"
    exe = str(tmp_path / "rayquery_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I",
                    os.path.join(ROOT, "gpgpuraytrace_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "rayquery_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("rayquery_check ok")


def test_block_layout_and_option_prefix_under_sanitizers(tmp_path):
    """tests/tools/querylayout_check.cpp: what the query families share in rt_rayquery.h -- the layout of the host
    forms' device block (every part at a multiple of 16, in order, an absent part no space, size_t arithmetic at 2^26
    elements, the largest lattice) and the one option-prefix parser behind the three option parsers (never past the
    caller's size).  Its own main, its own process: nothing of it is loaded into this interpreter."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/tools/querylayout_check.cpp"
    exe = str(tmp_path / "querylayout_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I",
                    os.path.join(ROOT, "gpgpuraytrace_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "querylayout_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("querylayout_check ok")
