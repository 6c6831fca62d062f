"""CPU tests of point shading (rt_terrain_shade_points*, include/frosttrace.h): the declared and exported entry
points, the host-only option parser and plan under AddressSanitizer + UBSan (its own program), what pins the checker
the GPU tests compare with (tests/point_ref.py) on the oracle's own trace_sample, the census of the point sets those
tests use, and the Python side that needs no GPU: write_obj's vertex colours and extract_mesh's argument check."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import point_ref as PR
import ray_fixture as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID = -1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_header_declares_and_library_exports_the_entry_points():
    import gpgpuraytrace_amd as G
    from gpgpuraytrace_amd import _native, engine
    txt = open(os.path.join(ROOT, "include", "frosttrace.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("rt_terrain_shade_points", "rt_terrain_shade_points_device"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(G.lib(), name), name
        assert name in _native.SIGNATURES
    assert len(_native.SIGNATURES["rt_terrain_shade_points"][1]) == 8
    assert len(_native.SIGNATURES["rt_terrain_shade_points_device"][1]) == 8
    assert re.search(r"\}\s*rt_point_options\s*;", code)
    assert C.sizeof(_native.RtPointOptions) == 32
    assert [f[0] for f in _native.RtPointOptions._fields_] == ["size", "flags", "eye", "max_blocks", "ao_samples", "seed"]
    assert G.lib().rt_abi_version() == 9  # additive
    assert hasattr(G.Terrain, "shade_points") and hasattr(G.Terrain, "shade_points_device")
    # the header says what the definition is and what is out of scope
    doc = txt[txt.index("point shading"):txt.index("} rt_point_options;")]
    for words in ("getColor(p_i, n_i, pdn, dist)", "ao_dir(n_i, px = i, py = seed, a = 0, k)", "NOT multiplied by ao",
                  "unorm8(saturate(color.rgb) * ao)", "TRACESCREEN", "Out of scope", "a sun or an eye per point",
                  "A query reads no", "ao_samples above 16"):
        assert words in doc, words
    # the device layout of the points and of the normals is the field queries' packed point
    p = np.arange(15, dtype=np.float32).reshape(5, 3)
    packed = G.pack_points(p)
    assert packed.shape == (5, 4) and np.array_equal(packed[:, :3], p) and not packed[:, 3].any()
    # point_options
    o = G.point_options()
    assert (o.size, o.flags, o.max_blocks, o.ao_samples, o.seed) == (32, 0, 0, 0, 0)
    o = engine.point_options(eye=(1.5, -2, 3.25), ao_samples=4, seed=0xdeadbeef, max_blocks=7)
    assert (o.size, o.flags, o.max_blocks, o.ao_samples, o.seed) == (32, _native.RT_RAYS_EYE, 7, 4, 0xdeadbeef)
    assert list(o.eye) == [1.5, -2.0, 3.25]


def test_argument_checks_that_need_no_device():
    import gpgpuraytrace_amd as G
    L = G.lib()
    buf = np.zeros(8, np.float32)
    p = buf.ctypes.data
    assert L.rt_terrain_shade_points(None, p, p, 1, None, p, None, None) == RT_ERR_INVALID and b"null" in L.rt_last_error()
    assert L.rt_terrain_shade_points_device(None, p, p, 1, None, p, None, None) == RT_ERR_INVALID
    assert L.rt_terrain_shade_points(None, p, p, 0, None, p, None, None) == RT_ERR_INVALID  # (a null compute, whatever n)
    assert not buf.any()


def test_planning_header_under_sanitizers(tmp_path):
    """tests/tools/pointquery_check.cpp: rt_rayquery.h's parse_point_options -- every accept and reject -- and
    plan_points -- always lanes, the grid's three bounds --, the host form's block and the packing.  Its own main,
    its own process: nothing of it is loaded into this interpreter."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/tools/pointquery_check.cpp"
    exe = str(tmp_path / "pointquery_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I",
                    os.path.join(ROOT, "gpgpuraytrace_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "pointquery_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("pointquery_check ok")


# --- what pins the checker itself --------------------------------------------------------------------------------
@pytest.mark.parametrize("land", RF.LANDSCAPES)
def test_checker_is_pinned_on_the_oracles_trace_sample(land):
    """The fixture rays F0-F3 that hit, under shade_ref.SUN, eye F0's.  The oracle's own march gives rr and
    get_normal (PR.primary); the oracle's own trace_sample with ao_samples = K and (px, py, a) = (i, seed, 0) gives
    the sample and its ao (PR.trace_sample).
    Which case held: dist and pdn recomputed from p - E are NOT rr.pd.w and the ray's pdn for any hit, on any
    landscape -- rr.pd.w is the march's distance after its last refinement step, not the last sample's, and
    p = fma(dir, sd, origin) is rounded -- so the bit-for-bit identity with trace_sample's colour is asserted for
    the (few or no) rays where the pairs agree and the chain is pinned link by link for all:
      - get_color at the RAY's (pdn, rr.pd.w) through trace_sample's two lerps IS trace_sample's colour, and its
        shadow count trace_sample's (so PR.get_color and PR.blend are the oracle's);
      - the checker's recomputed (pdn, dist) ARE norm3(p - E), len3(p - E);
      - the checker's colour and shadow count ARE get_color's at the checker's own (pdn, dist);
      - ambient_occlusion at the RAY's rr.pd.w IS trace_sample's ao and AO step sum (so PR.ambient_occlusion is the
        oracle's), and the checker's ao and step sum ARE ambient_occlusion's at the checker's own dist;
      - directly: the checker's ao and AO step sum ARE trace_sample's wherever shadow_precision(dist), the only way
        dist enters ambient_occlusion, is shadow_precision(rr.pd.w): it is 8 below a distance of about 134, so for
        the near hits (about 1,200 on testing, none on greenrocks, whose hits are all farther)."""
    K, seed = 4, 3
    eye = RF.eye("F0")
    o, d = RF.query(RF.F_SET)
    pd, nd, fc, ray, pdn = PR.primary(o, d, eye, land)
    hit = np.flatnonzero(nd[:, 3] > 0)
    assert len(hit) >= 1024
    o, d, pd, nd, fc, ray, pdn = (np.ascontiguousarray(a[hit]) for a in (o, d, pd, nd, fc, ray, pdn))
    p, nrm = pd[:, :3], nd[:, :3]
    col_ts, ao_ts, steps_ts = PR.trace_sample(o, d, eye, land, K, seed)
    assert steps_ts[:, 1].all() and steps_ts[:, 2].all()  # every ray here is a hit: it has a shadow ray and AO rays
    # the links PR.get_color and PR.blend: trace_sample's own colour from its own rr
    col_ray, sh_ray = PR.get_color(p, nrm, pdn, pd[:, 3], eye, land)
    assert np.array_equal(_bits(PR.blend(col_ray, pd[:, 3], fc, ray)), _bits(col_ts))
    assert np.array_equal(sh_ray, steps_ts[:, 1])
    # the checker
    res, px, steps, cls, occ, view = PR.shade(p, nrm, eye, land, ao_samples=K, seed=seed)
    v = (p - eye[None, :]).astype(np.float32)  # one IEEE subtraction a component, as sub3
    assert np.array_equal(_bits(view), _bits(PR.norm_len(v)))
    col_own, sh_own = PR.get_color(p, nrm, view[:, :3], view[:, 3], eye, land)
    assert np.array_equal(_bits(res[:, :3]), _bits(col_own)) and np.array_equal(steps[:, 0], sh_own)
    same = (_bits(view[:, 3]) == _bits(pd[:, 3])) & (_bits(view[:, :3]) == _bits(pdn)).all(axis=1)
    print(land, "hits", len(hit), "recomputed (pdn, dist) equal the ray's for", int(same.sum()))
    assert np.array_equal(_bits(PR.blend(res[same, :3], pd[same, 3], fc[same], ray[same])), _bits(col_ts[same]))
    same_prec = _bits(PR.precision(view[:, 3])) == _bits(PR.precision(pd[:, 3]))
    print(land, "shadow_precision equal for", int(same_prec.sum()))
    ao_ray, aost_ray = PR.ambient_occlusion(p, nrm, pd[:, 3], eye, land, K, seed)
    assert np.array_equal(_bits(ao_ray), _bits(ao_ts)) and np.array_equal(aost_ray, steps_ts[:, 2])
    ao_own, aost_own = PR.ambient_occlusion(p, nrm, view[:, 3], eye, land, K, seed)
    assert np.array_equal(_bits(res[:, 3]), _bits(ao_own)) and np.array_equal(steps[:, 1], aost_own)
    assert np.array_equal(_bits(res[same_prec, 3]), _bits(ao_ts[same_prec]))
    assert np.array_equal(steps[same_prec, 1], steps_ts[same_prec, 2])
    # ao, occ and the pixel: the definition's last lines
    # (fma(-0.6f, occ / 4, 1): exact in float64, 24 + 3 bits and the 1, so rounded once)
    assert np.array_equal(_bits(res[:, 3]),
                          _bits((1.0 - np.float64(np.float32(0.6)) * (occ.astype(np.float64) * 0.25)).astype(np.float32)))
    sat = np.clip(res[:, :3], np.float32(0), np.float32(1)) * res[:, 3:4]
    want = np.rint(sat * np.float32(255)).astype(np.uint32)
    assert np.array_equal(px, want[:, 0] | want[:, 1] << 8 | want[:, 2] << 16 | np.uint32(0xff000000))
    # K = 0: ao is 1, no AO step, the same colour
    res0, px0, steps0, _, occ0, _ = PR.shade(p, nrm, eye, land)
    assert np.array_equal(_bits(res0[:, :3]), _bits(res[:, :3])) and (res0[:, 3] == 1).all()
    assert not steps0[:, 1].any() and not occ0.any() and np.array_equal(steps0[:, 0], steps[:, 0])


@pytest.mark.parametrize("land", RF.LANDSCAPES)
def test_parity_inputs_hold_every_class(land):
    """The census of PR.points(land) -- what the GPU tests shade -- with K = 4, counted with the checker alone, for
    both seeds of the GPU tests (0 and 3): at least 64 lit and 64 shadowed points, 32 with 0 < occ < K, 8 with
    occ == 0 and 8 with occ == K.  Found (lit, shadowed | occ = 0, 1, 2, 3, 4), seed 0 / seed 3:
      nomadplains  1408 points, the hits of F0-F3, every second:  835, 573 | 390 336 213 204 265 / 418 283 214 226 267
      greenrocks   1405 points, the same:                         982, 423 | 841 315 141 82 26 / 860 300 130 78 37
      testing and simple do not meet the last line with the cameras' hits (occ = 4 at seed 0: none of every second
      hit, 1392 and 1408 points), so theirs are fewer hits and the vertices of a small lattice's mesh
      (PR.POINT_LATTICES):
      testing      2048 points, 254 hits and 1794 vertices:       1596, 452 | 681 787 456 114 10 / 668 844 416 109 11
      simple       1802 points, 563 hits and 1239 vertices:       1621, 181 | 837 544 323 89 9 / 880 496 318 98 10"""
    p, nrm = PR.points(land)
    assert 1024 < len(p) <= PR.MAX_POINTS and p.shape == nrm.shape
    for seed in (0, 3):
        _, _, _, cls, occ, _ = PR.query(land, 4, seed)
        lit, shadowed = int((cls == PR.LIT).sum()), int((cls == PR.SHADOWED).sum())
        hist = np.bincount(occ, minlength=5)
        print(land, len(p), "seed", seed, "lit, shadowed:", lit, shadowed, "occ 0..4:", hist)
        assert lit + shadowed == len(p) and lit >= 64 and shadowed >= 64
        assert hist[1:4].sum() >= 32 and hist[0] >= 8 and hist[4] >= 8 and len(hist) == 5


# --- the Python side that needs no GPU ---------------------------------------------------------------------------
def _read_obj(path):
    v, vn, f = [], [], []
    for line in open(path):
        w = line.split()
        if not w or w[0] == "#":
            continue
        if w[0] == "v":
            v.append([np.float32(x) for x in w[1:]])
        elif w[0] == "vn":
            vn.append([np.float32(x) for x in w[1:]])
        elif w[0] == "f":
            f.append([int(x.split("/")[0]) - 1 for x in w[1:]])
    return np.array(v, np.float32), np.array(vn, np.float32), np.array(f, np.int64)


def test_write_obj_colours(tmp_path):
    from gpgpuraytrace_amd import output
    rng = np.random.default_rng(5)
    v = rng.normal(size=(7, 3)).astype(np.float32) * np.float32(100)
    nrm = rng.normal(size=(7, 4)).astype(np.float32)
    t = rng.integers(0, 7, size=(5, 3)).astype(np.uint32)
    words = rng.integers(0, 1 << 32, size=7, dtype=np.uint64).astype(np.uint32)
    words[0], words[1] = 0xff000000, 0xffffffff
    a = str(tmp_path / "a.obj")
    # RGBA8 words: channels byte / 255, R in the low byte, alpha dropped
    output.write_obj(a, v, t, nrm, colors=words)
    rv, rn, rf = _read_obj(a)
    assert rv.shape == (7, 6) and np.array_equal(_bits(rv[:, :3]), _bits(v)) and np.array_equal(_bits(rn), _bits(nrm[:, :3]))
    assert np.array_equal(rf, t.astype(np.int64))
    back = np.rint(rv[:, 3:] * np.float32(255)).astype(np.uint32)
    assert np.array_equal(back[:, 0] | back[:, 1] << 8 | back[:, 2] << 16, words & np.uint32(0xffffff))
    assert rv[:, 3:].min() >= 0 and rv[:, 3:].max() <= 1
    # (nv, 3) floats: written as they are
    cf = rng.random(size=(7, 3)).astype(np.float32)
    output.write_obj(a, v, t, colors=cf)
    rv, rn, rf = _read_obj(a)
    assert np.array_equal(_bits(rv[:, 3:]), _bits(cf)) and np.array_equal(_bits(rv[:, :3]), _bits(v)) and len(rn) == 0
    assert all(len(line.split()) == 4 for line in open(a) if line.startswith("f "))
    with pytest.raises(ValueError):
        output.write_obj(a, v, t, colors=cf[:6])
    with pytest.raises(ValueError):
        output.write_obj(a, v, t, colors=words[:6])
    # without colours: byte for byte the file as it always was
    for normals in (None, nrm):
        output.write_obj(a, v, t, normals)
        want = "# 7 vertices, 5 triangles\n" + "".join("v %.9g %.9g %.9g\n" % tuple(map(float, q)) for q in v)
        if normals is not None:
            want += "".join("vn %.9g %.9g %.9g\n" % tuple(map(float, q[:3])) for q in nrm)
            want += "".join("f %d//%d %d//%d %d//%d\n" % (i + 1, i + 1, j + 1, j + 1, k + 1, k + 1) for i, j, k in t.astype(int))
        else:
            want += "".join("f %d %d %d\n" % (i + 1, j + 1, k + 1) for i, j, k in t.astype(int))
        assert open(a, "rb").read() == want.encode()


def test_extract_mesh_colours_need_normals():
    """The arguments are checked before any native call: no Terrain, no device."""
    import gpgpuraytrace_amd as G
    with pytest.raises(ValueError):
        G.Terrain.extract_mesh(None, (0, 0, 0), (1, 1, 1), (2, 2, 2), normals=False, colors=True)
    with pytest.raises(ValueError):
        G.Terrain.shade_points(None, np.zeros((3, 3), np.float32), np.zeros((2, 3), np.float32))
