"""The checker of the shaded queries (TEST INFRASTRUCTURE): builds, binds and caches tests/tools/shade_ref.c,
which includes the oracle's source and evaluates the definition of rt_terrain_shade_rays (include/frosttrace.h)
from the oracle's own trace_ray, get_normal, get_color, get_rayleigh_mie and get_space_color for rays of the
caller's own.  Built with the oracle's own flags into tests/tools/_build/."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as O
import ray_fixture as RF
import surface_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "shade_ref.c")
SO = os.path.join(ROOT, "tests", "tools", "_build", "libshade_ref.so")
T_MIN, T_MAX = SR.T_MIN, SR.T_MAX
# The sun of the shaded tests.  The fixture's (0, -1, 0) points down: every shadow ray runs into the ground.  This
# one stands 30 degrees up (0.5 = sin 30), so that on each landscape the F0-F3 rays hold at least 64 misses, 64 lit
# and 64 shadowed hits (test_shade_query_host.py counts them with the checker alone).
SUN = np.array([0.75, 0.5, 0.4330127], np.float32)
MISS, LIT, SHADOWED = 0, 1, 2

_lib = None
_cache = {}


def lib():
    global _lib
    if _lib is None:
        deps = [SRC, os.path.join(ROOT, "oracle", "rt_oracle.c"), os.path.join(ROOT, "oracle", "rt_oracle.h")]
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in deps):
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            tmp = "%s.%d.tmp" % (SO, os.getpid())
            subprocess.run(["gcc"] + SR.CFLAGS + ["-shared", "-o", tmp, SRC, "-lm"], check=True)
            os.replace(tmp, SO)
        L = C.CDLL(SO)
        fp = C.POINTER(C.c_float)
        L.sr_shade_rays.argtypes = [C.POINTER(O.Noise), C.POINTER(O.Frame), fp, fp, fp, C.c_int64, C.c_float,
                                    C.c_float, C.c_float, C.c_int, fp, C.c_void_p, C.c_void_p, C.c_void_p, fp, fp]
        L.sr_shade_rays.restype = None
        L.sr_trace_sample.argtypes = [C.POINTER(O.Noise), C.POINTER(O.Frame), fp, fp, fp, C.c_int64, C.c_float,
                                      C.c_float, fp, C.c_void_p]
        L.sr_trace_sample.restype = None
        _lib = L
    return _lib


def frame(eye, landscape, sun=SUN, recording=0, max_steps=0):
    consts = dict(RF.consts("F0"))
    consts["eye"] = np.array([eye[0], eye[1], eye[2], 0], np.float32)
    consts["sun"] = np.asarray(sun, np.float32)
    return O.make_frame(consts, landscape=O.LANDSCAPES[landscape], recording=recording, max_steps=max_steps)


def _rays(origins, dirs, ranges):
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    rg = None
    if ranges is not None:
        rg = np.ascontiguousarray(ranges, np.float32).reshape(-1, 2)
        assert len(rg) == len(o)
    return o, d, rg


def shade(origins, dirs, eye, landscape, ranges=None, t_min=T_MIN, t_max=T_MAX, stepmod=1.0, max_steps=0, recording=0,
          sun=SUN, fog_rgb=False):
    """(results (n, 8) float32, rgba8 (n,) uint32, steps (n, 2) uint32, classes (n,) uint8: MISS, LIT, SHADOWED,
    fog_w (n,) float32: the primary march's fcolord.w) of the definition in include/frosttrace.h for these rays;
    with fog_rgb a sixth: (n, 3) float32, the primary march's fcolord.rgb."""
    o, d, rg = _rays(origins, dirs, ranges)
    n = len(o)
    fr = frame(eye, landscape, sun, recording)
    res = np.zeros((n, 8), np.float32)
    px = np.zeros(n, np.uint32)
    steps = np.zeros((n, 2), np.uint32)
    cls = np.zeros(n, np.uint8)
    fog = np.zeros(n, np.float32)
    frgb = np.zeros((n, 3), np.float32) if fog_rgb else None
    lib().sr_shade_rays(C.byref(O.noise_tables()), C.byref(fr), O._fp(o), O._fp(d), O._fp(rg) if rg is not None else None,
                        n, t_min, t_max, stepmod, max_steps, O._fp(res), px.ctypes.data, steps.ctypes.data, cls.ctypes.data,
                        O._fp(fog), O._fp(frgb) if fog_rgb else None)
    return (res, px, steps, cls, fog, frgb) if fog_rgb else (res, px, steps, cls, fog)


def trace_sample(origins, dirs, eye, landscape, ranges=None, t_min=T_MIN, t_max=T_MAX, max_steps=0, recording=0, sun=SUN):
    """(colours (n, 3) float32, steps (n, 2) uint32) of the oracle's own trace_sample with ao_samples = 0."""
    o, d, rg = _rays(origins, dirs, ranges)
    n = len(o)
    fr = frame(eye, landscape, sun, recording, max_steps)
    col = np.zeros((n, 3), np.float32)
    steps = np.zeros((n, 2), np.uint32)
    lib().sr_trace_sample(C.byref(O.noise_tables()), C.byref(fr), O._fp(o), O._fp(d), O._fp(rg) if rg is not None else None,
                          n, t_min, t_max, O._fp(col), steps.ctypes.data)
    return col, steps


def frame_pixels(cell_distance):
    """The fixture rays that are pixel rays of a 256x256 frame (px, py < 256; ray_fixture.screen_coords): their
    indices in the camera's 1024 rays, px, py and ranges (CellDistance[cell].x, 5000) with tracescreen.hlsl's
    cell of the pixel."""
    i = np.arange(1024)
    f32 = np.float32
    px, py = (((t.astype(f32) * (f32(1) / f32(31))) * f32(RF.SIZE)).astype(np.uint32) for t in (i % 32, i // 32))
    keep = np.flatnonzero((px < RF.SIZE) & (py < RF.SIZE))
    px, py = px[keep], py[keep]
    spx, spy = px.astype(f32) / f32(RF.SIZE), py.astype(f32) / f32(RF.SIZE)
    cell = (np.floor(spy * f32(32)) * f32(32) + np.floor(spx * f32(32))).astype(np.uint32)
    cd = np.asarray(cell_distance, np.float32).reshape(1024, 2)
    rg = np.stack([cd[cell, 0], np.full(len(keep), 5000, np.float32)], axis=1).astype(np.float32)
    return keep, px, py, rg


def query(names, landscape, eye=None, ranged=False, **kw):
    """The fixture cameras' rays (ray_fixture.query) through shade(); eye: a camera's name (default: the first's).
    Computed once per argument set, read-only."""
    names = tuple(names)
    key = (names, landscape, eye, ranged, tuple(sorted(kw.items())))
    if key not in _cache:
        o, d = RF.query(names)
        rg = SR.seeded_ranges(len(o)) if ranged else None
        out = shade(o, d, RF.eye(eye or names[0]), landscape, ranges=rg, **kw)
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]
