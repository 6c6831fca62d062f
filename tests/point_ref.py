"""The checker of point shading (TEST INFRASTRUCTURE): builds, binds and caches tests/tools/point_ref.c, which
includes the oracle's source and evaluates the definition of rt_terrain_shade_points (include/frosttrace.h) from
the oracle's own get_color and ambient_occlusion for points and normals of the caller's own.  Built with the
oracle's own flags into tests/tools/_build/."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as O
import ray_fixture as RF
import shade_ref as SH
import surface_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "point_ref.c")
SO = os.path.join(ROOT, "tests", "tools", "_build", "libpoint_ref.so")
SUN = SH.SUN
LIT, SHADOWED = 1, 2
T_MIN, T_MAX = SR.T_MIN, SR.T_MAX

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
        fp, vp, nzp, frp = C.POINTER(C.c_float), C.c_void_p, C.POINTER(O.Noise), C.POINTER(O.Frame)
        L.pr_shade_points.argtypes = [nzp, frp, fp, fp, C.c_int64, C.c_int, C.c_uint32, fp, vp, vp, vp, vp, fp]
        L.pr_primary.argtypes = [nzp, frp, fp, fp, C.c_int64, C.c_float, C.c_float, fp, fp, fp, fp, fp]
        L.pr_trace_sample.argtypes = [nzp, frp, fp, fp, C.c_int64, C.c_float, C.c_float, C.c_int, C.c_uint32, fp, fp, vp]
        L.pr_get_color.argtypes = [nzp, frp, fp, fp, fp, fp, C.c_int64, fp, vp]
        L.pr_ambient_occlusion.argtypes = [nzp, frp, fp, fp, fp, C.c_int64, C.c_int, C.c_uint32, fp, vp]
        L.pr_blend.argtypes = [fp, fp, fp, fp, C.c_int64, fp]
        L.pr_norm_len.argtypes = [fp, C.c_int64, fp]
        L.pr_precision.argtypes = [fp, C.c_int64, fp]
        for f in (L.pr_shade_points, L.pr_primary, L.pr_trace_sample, L.pr_get_color, L.pr_ambient_occlusion, L.pr_blend, L.pr_norm_len,
                  L.pr_precision):
            f.restype = None
        _lib = L
    return _lib


def _xyz(a):
    a = np.asarray(a, np.float32)
    if a.ndim == 2 and a.shape[1] == 4:
        a = a[:, :3]
    return np.ascontiguousarray(a).reshape(-1, 3)


def shade(points, normals, eye, landscape, ao_samples=0, seed=0, recording=0, sun=SUN):
    """(results (n, 4) float32, rgba8 (n,) uint32, steps (n, 2) uint32, classes (n,) uint8: LIT or SHADOWED,
    occ (n,) uint32: the occluded AO rays, view (n, 4) float32: pdn and dist as recomputed from p - E) of the
    definition in include/frosttrace.h for these points; (n, 4) inputs lose their spare word."""
    p, nr = _xyz(points), _xyz(normals)
    n = len(p)
    assert len(nr) == n
    fr = SH.frame(eye, landscape, sun, recording)
    res = np.zeros((n, 4), np.float32)
    px = np.zeros(n, np.uint32)
    steps = np.zeros((n, 2), np.uint32)
    cls = np.zeros(n, np.uint8)
    occ = np.zeros(n, np.uint32)
    view = np.zeros((n, 4), np.float32)
    lib().pr_shade_points(C.byref(O.noise_tables()), C.byref(fr), O._fp(p), O._fp(nr), n, int(ao_samples),
                          int(seed) & 0xffffffff, O._fp(res), px.ctypes.data, steps.ctypes.data, cls.ctypes.data,
                          occ.ctypes.data, O._fp(view))
    return res, px, steps, cls, occ, view


def primary(origins, dirs, eye, landscape, t_min=T_MIN, t_max=T_MAX, recording=0, sun=SUN):
    """The oracle's own primary march and get_normal for rays (trace_sample's first lines): pd (n, 4), normal and
    density (n, 4), fcolord (n, 4), scat.rayleigh (n, 3), pdn (n, 3)."""
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    n = len(o)
    fr = SH.frame(eye, landscape, sun, recording)
    pd, nd, fc = (np.zeros((n, 4), np.float32) for _ in range(3))
    ray, pdn = (np.zeros((n, 3), np.float32) for _ in range(2))
    lib().pr_primary(C.byref(O.noise_tables()), C.byref(fr), O._fp(o), O._fp(d), n, t_min, t_max, O._fp(pd), O._fp(nd),
                     O._fp(fc), O._fp(ray), O._fp(pdn))
    return pd, nd, fc, ray, pdn


def trace_sample(origins, dirs, eye, landscape, ao_samples, seed, t_min=T_MIN, t_max=T_MAX, recording=0, sun=SUN):
    """(colours (n, 3) float32, ao (n,) float32, steps (n, 3) uint32: primary, shadow, AO) of the oracle's own
    trace_sample with ao_samples and (px, py, a) = (i, seed, 0)."""
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    n = len(o)
    fr = SH.frame(eye, landscape, sun, recording)
    col = np.zeros((n, 3), np.float32)
    ao = np.zeros(n, np.float32)
    steps = np.zeros((n, 3), np.uint32)
    lib().pr_trace_sample(C.byref(O.noise_tables()), C.byref(fr), O._fp(o), O._fp(d), n, t_min, t_max, int(ao_samples),
                          int(seed) & 0xffffffff, O._fp(col), O._fp(ao), steps.ctypes.data)
    return col, ao, steps


def get_color(points, normals, pdn, dist, eye, landscape, recording=0, sun=SUN):
    """(colours (n, 3) float32, shadow iterations (n,) uint32) of the oracle's get_color at the given pdn and dist."""
    p, nr = _xyz(points), _xyz(normals)
    v = np.ascontiguousarray(pdn, np.float32).reshape(-1, 3)
    ds = np.ascontiguousarray(dist, np.float32).reshape(-1)
    n = len(p)
    assert len(nr) == n and len(v) == n and len(ds) == n
    fr = SH.frame(eye, landscape, sun, recording)
    col = np.zeros((n, 3), np.float32)
    steps = np.zeros(n, np.uint32)
    lib().pr_get_color(C.byref(O.noise_tables()), C.byref(fr), O._fp(p), O._fp(nr), O._fp(v), O._fp(ds), n, O._fp(col),
                       steps.ctypes.data)
    return col, steps


def ambient_occlusion(points, normals, dist, eye, landscape, ao_samples, seed, recording=0, sun=SUN):
    """(ao (n,) float32, the AO rays' iterations (n,) uint32) of the oracle's ambient_occlusion at the given dist,
    with (px, py, a) = (i, seed, 0)."""
    p, nr = _xyz(points), _xyz(normals)
    ds = np.ascontiguousarray(dist, np.float32).reshape(-1)
    n = len(p)
    assert len(nr) == n and len(ds) == n and ao_samples > 0
    fr = SH.frame(eye, landscape, sun, recording)
    ao = np.zeros(n, np.float32)
    steps = np.zeros(n, np.uint32)
    lib().pr_ambient_occlusion(C.byref(O.noise_tables()), C.byref(fr), O._fp(p), O._fp(nr), O._fp(ds), n, int(ao_samples),
                               int(seed) & 0xffffffff, O._fp(ao), steps.ctypes.data)
    return ao, steps


def blend(colors, pdw, fc, ray):
    """trace_sample's two lerps for a hit: lerp(lerp(colour, fcolord.rgb, fcolord.w), rayleigh, skyAmount(pd.w))."""
    c = np.ascontiguousarray(colors, np.float32).reshape(-1, 3)
    w = np.ascontiguousarray(pdw, np.float32).reshape(-1)
    f = np.ascontiguousarray(fc, np.float32).reshape(-1, 4)
    r = np.ascontiguousarray(ray, np.float32).reshape(-1, 3)
    out = np.zeros_like(c)
    lib().pr_blend(O._fp(c), O._fp(w), O._fp(f), O._fp(r), len(c), O._fp(out))
    return out


def norm_len(v):
    """(n, 4) float32: the oracle's norm3(v), len3(v)."""
    a = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    out = np.zeros((len(a), 4), np.float32)
    lib().pr_norm_len(O._fp(a), len(a), O._fp(out))
    return out


def precision(dist):
    """The oracle's shadow_precision(dist): the shadow and AO rays' stepmod."""
    d = np.ascontiguousarray(dist, np.float32).reshape(-1)
    out = np.zeros_like(d)
    lib().pr_precision(O._fp(d), len(d), O._fp(out))
    return out


# The point set of the parity tests, per landscape: the hits (pd.xyz, get_normal) of the oracle's own primary march
# for the fixture cameras' rays, one eye (F0's), as many cameras as the census of test_point_query_host.py takes;
# at most 2,048 points.
POINT_CAMERAS = {"nomadplains": ("F0", "F1", "F2", "F3"), "testing": ("F0", "F1", "F2", "F3"),
                 "simple": ("F0", "F1", "F2", "F3"), "greenrocks": ("F0", "F1", "F2", "F3")}
MAX_POINTS = 2048
# testing (smooth sine hills) and simple (gentle noise hills) hold no point with all four AO rays occluded among
# the cameras' hits, so their sets take the cameras' hits down to FIXTURE_POINTS and add mesh_ref's vertices (with
# field_ref's normals) of a small lattice where the terrain closes in: the bottom of a valley of testing's sines,
# and in simple the foot of the cliff where the floor of its terrace band (y about 9.3) meets the wall.
# landscape -> (origin, spacing, dims)
POINT_LATTICES = {"testing": ((14.2, -10.25, 29.9), (0.07, 0.07, 0.07), (44, 7, 44)),
                  "simple": ((-321.5, 8.5, 221.0), (0.25, 0.25, 0.25), (29, 7, 89))}
FIXTURE_POINTS = {"testing": 256, "simple": 564}


def hit_points(names, landscape):
    """(points (m, 3), normals (m, 3), ray indices (m,)) of the cameras' rays that hit; computed once, read-only."""
    key = ("hits", tuple(names), landscape)
    if key not in _cache:
        o, d = RF.query(names)
        pd, nd, _, _, _ = primary(o, d, RF.eye(names[0]), landscape)
        hit = np.flatnonzero(nd[:, 3] > 0)
        out = (np.ascontiguousarray(pd[hit, :3]), np.ascontiguousarray(nd[hit, :3]), hit)
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def points(landscape):
    """The landscape's point set (points, normals), at most MAX_POINTS: every (hits / MAX_POINTS)-th hit, so that
    all the cameras take part."""
    key = ("points", landscape)
    if key not in _cache:
        p, nr, _ = hit_points(POINT_CAMERAS[landscape], landscape)
        lat = POINT_LATTICES.get(landscape)
        stride = -(-len(p) // (FIXTURE_POINTS[landscape] if lat else MAX_POINTS))
        p, nr = p[::stride], nr[::stride]
        if lat:
            import mesh_ref as MR
            eye = RF.eye(POINT_CAMERAS[landscape][0])
            m = MR.lattice_mesh("point-census", lat[0], lat[1], lat[2], eye, landscape)
            mn = MR.normals("point-census-" + landscape, m.vertices, eye, landscape)
            room = MAX_POINTS - len(p)  # (the vertices are in cell order: a cut drops the lattice's last slabs)
            p = np.concatenate([p, m.vertices[:room]])
            nr = np.concatenate([nr, mn[:room, :3]])
        out = (np.ascontiguousarray(p, np.float32), np.ascontiguousarray(nr, np.float32))
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def query(landscape, ao_samples=0, seed=0, eye="F0", **kw):
    """points(landscape) through shade(); eye: a camera's name.  Computed once per argument set, read-only."""
    key = ("query", landscape, ao_samples, seed, eye, tuple(sorted(kw.items())))
    if key not in _cache:
        p, nr = points(landscape)
        out = shade(p, nr, RF.eye(eye), landscape, ao_samples=ao_samples, seed=seed, **kw)
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]
