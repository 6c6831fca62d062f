"""CPU tests of the shaded queries (rt_terrain_shade_rays*, include/frosttrace.h): the declared and exported entry
points, the host-only plan under AddressSanitizer + UBSan (its own program), and what pins the checker the GPU
tests compare with (tests/shade_ref.py): it equals the oracle's own trace_sample with ao_samples = 0, it equals a
frame of ro_tracescreen2 at the fixture's pixels, and under the tests' sun its inputs hold every class of ray."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import ray_fixture as RF
import shade_ref as SH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = -1


def test_header_declares_and_library_exports_the_entry_points():
    import gpgpuraytrace_amd as G
    from gpgpuraytrace_amd import _native
    txt = open(os.path.join(ROOT, "include", "frosttrace.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("rt_terrain_shade_rays", "rt_terrain_shade_rays_device"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(G.lib(), name), name
        assert name in _native.SIGNATURES
    assert len(_native.SIGNATURES["rt_terrain_shade_rays"][1]) == 9
    assert len(_native.SIGNATURES["rt_terrain_shade_rays_device"][1]) == 7
    assert C.sizeof(_native.RtSurfaceOptions) == 40  # the option block is the surface queries', unchanged
    assert G.lib().rt_abi_version() == 9  # additive
    assert hasattr(G.Terrain, "shade_rays") and hasattr(G.Terrain, "shade_rays_device")
    # the header says what is out of scope
    doc = txt[txt.index("shaded queries"):txt.index("int rt_terrain_shade_rays(")]
    assert "tracescreen.hlsl:16-48" in doc and "NO ambient occlusion" in doc and "RT_ERR_UNSUPPORTED" in doc


def test_argument_checks_that_need_no_device():
    import gpgpuraytrace_amd as G
    L = G.lib()
    buf = np.zeros(8, np.float32)
    p = buf.ctypes.data
    assert L.rt_terrain_shade_rays(None, p, p, None, 1, None, p, None, None) == RT_ERR_INVALID and b"null" in L.rt_last_error()
    assert L.rt_terrain_shade_rays_device(None, p, 1, None, p, None, None) == RT_ERR_INVALID
    assert L.rt_terrain_shade_rays(None, p, p, None, 0, None, p, None, None) == RT_ERR_INVALID  # (a null compute, whatever n)


def test_planning_header_under_sanitizers(tmp_path):
    """tests/tools/shadequery_check.cpp: rt_rayquery.h's plan_shade -- always lanes, the grid's three bounds, forced
    segments refused -- behind the surface queries' option parser.  Its own main, its own process: nothing of it is
    loaded into this interpreter."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/tools/shadequery_check.cpp"
    exe = str(tmp_path / "shadequery_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I",
                    os.path.join(ROOT, "gpgpuraytrace_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "shadequery_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("shadequery_check ok")


# --- what pins the checker itself --------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("land", RF.LANDSCAPES)
def test_checker_equals_the_oracles_trace_sample(land):
    """With stepmod 1 (trace_sample's own) the checker's colour and both step counts are the oracle's trace_sample
    with ao_samples = 0, for the F0-F3 rays and G's (origin != eye), also with per-ray ranges and a step cap."""
    for names in (RF.F_SET, ("G",)):
        o, d = RF.query(names)
        res, px, steps, _, _ = SH.query(names, land)
        col, tsteps = SH.trace_sample(o, d, RF.eye(names[0]), land)
        assert np.array_equal(_bits(res[:, :3]), _bits(col)) and np.array_equal(steps, tsteps), names
        assert not steps[res[:, 7] <= 0, 1].any()  # a miss has no shadow ray
        assert steps[res[:, 7] > 0, 1].all()
        sat = np.clip(res[:, :3], 0, 1)
        want = np.rint(sat * np.float32(255)).astype(np.uint32)
        assert np.array_equal(px, want[:, 0] | want[:, 1] << 8 | want[:, 2] << 16 | np.uint32(0xff000000))
    o, d = RF.query(RF.F_SET)
    rg = SH.SR.seeded_ranges()
    res, _, steps, _, _ = SH.query(RF.F_SET, land, ranged=True, max_steps=64)
    col, tsteps = SH.trace_sample(o, d, RF.eye("F0"), land, ranges=rg, max_steps=64)
    assert np.array_equal(_bits(res[:, :3]), _bits(col)) and np.array_equal(steps, tsteps)
    assert steps[:, 0].max() <= 64


def test_checker_equals_a_frame_at_the_fixtures_pixels():
    """Camera F0 as a 256x256 frame with AA 1 under the tests' sun: at the fixture's pixel coordinates (px, py < 256)
    saturate(colour) is ro_tracescreen2's rgba32f, the pixel its rgba8, the step counts its primary_steps and
    secondary_steps, with ranges (CellDistance[cell].x, 5000)."""
    consts = dict(RF.consts("F0"))
    consts["sun"] = SH.SUN
    fr = O.make_frame(consts, landscape=O.NOMADPLAINS)
    prim = np.zeros((RF.SIZE, RF.SIZE), np.float32)
    sec = np.zeros((RF.SIZE, RF.SIZE), np.float32)
    rgba, rgba8, _, cd, _ = O.render_rows(O.noise_tables(), fr, steps=prim, secondary_steps=sec)
    keep, px, py, rg = SH.frame_pixels(cd)
    assert len(keep) == 31 * 31
    o, d = RF.rays("F0")
    res, pix, steps, cls, _ = SH.shade(o[keep], d[keep], RF.eye("F0"), "nomadplains", ranges=rg)
    assert min((cls == k).sum() for k in (SH.MISS, SH.LIT, SH.SHADOWED)) >= 16
    sat = np.clip(res[:, :3], np.float32(0), np.float32(1))
    assert np.array_equal(_bits(sat), _bits(rgba[py, px, :3]))
    assert np.array_equal(pix, np.ascontiguousarray(rgba8[py, px]).view(np.uint32).ravel())
    assert np.array_equal(steps[:, 0], prim[py, px].astype(np.uint32))
    assert np.array_equal(steps[:, 1], sec[py, px].astype(np.uint32))


@pytest.mark.parametrize("land", RF.LANDSCAPES)
def test_parity_inputs_hold_every_class(land):
    """Under SH.SUN = (0.75, 0.5, 0.4330127) -- 30 degrees up; the fixture's (0, -1, 0) shadows everything -- the
    F0-F3 rays hold at least 64 misses, 64 lit hits and 64 shadowed hits on every landscape, and on greenrocks at
    least 64 rays with primary fog (fcolord.w > 0).  Counted with the checker alone."""
    assert np.array_equal(SH.SUN, np.array([0.75, 0.5, 0.4330127], np.float32))
    res, _, _, cls, fog = SH.query(RF.F_SET, land)
    counts = [int((cls == k).sum()) for k in (SH.MISS, SH.LIT, SH.SHADOWED)]
    print(land, "miss, lit, shadowed:", counts, "fog w > 0:", int((fog > 0).sum()))
    assert sum(counts) == 4096 and min(counts) >= 64
    assert np.array_equal(cls == SH.MISS, res[:, 7] <= 0)
    if land == "greenrocks":
        assert (fog > 0).sum() >= 64
    else:
        assert not fog.any()
    # the down-pointing sun of the fixture would leave no lit hit
    if land == "testing":
        _, _, _, down, _ = SH.shade(*RF.query(("F0",)), RF.eye("F0"), land, sun=(0.0, -1.0, 0.0))
        assert not (down == SH.LIT).any()
