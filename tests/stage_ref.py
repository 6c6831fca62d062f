"""The oracle's shading stages at inputs of the caller's own (TEST INFRASTRUCTURE): builds, binds and caches
tests/tools/stage_ref.c, which includes the oracle's source and exports its static get_normal, get_fog,
get_pixel_ray, get_color and trace_ray, its AA offset tables, and of the AO extension pcg_hash, ao_dir, the factor
and trace_sample.  Built with the oracle's own flags into tests/tools/_build/."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as O
import shade_ref as SH
import surface_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "stage_ref.c")
SO = os.path.join(ROOT, "tests", "tools", "_build", "libstage_ref.so")
LIT, SHADOWED = SH.LIT, SH.SHADOWED

_lib = None


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
        fp, nzp, frp = C.POINTER(C.c_float), C.POINTER(O.Noise), C.POINTER(O.Frame)
        L.st_normal.argtypes = [nzp, frp, fp, C.c_int64, fp]
        L.st_fog.argtypes = [nzp, frp, fp, fp, C.c_int64, fp]
        L.st_pixel_ray.argtypes = [nzp, frp, fp, C.c_int64, fp, fp]
        L.st_color.argtypes = [nzp, frp, fp, fp, fp, fp, C.c_int64, fp, C.c_void_p, fp]
        L.st_trace_ray.argtypes = [nzp, frp, fp, fp, fp, fp, fp, C.c_int64, C.c_int, C.c_int, C.c_int, fp, fp, fp,
                                   C.c_void_p]
        for f in (L.st_normal, L.st_fog, L.st_pixel_ray, L.st_color, L.st_trace_ray):
            f.restype = None
        L.st_shadow_precision.argtypes = [fp, C.c_int64, fp]
        L.st_shadow_precision.restype = None
        L.st_aa_offsets.argtypes = [C.c_int, fp]
        L.st_aa_offsets.restype = C.c_int
        L.st_pcg_hash.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.st_pcg_hash.restype = None
        L.st_ao_dir.argtypes = [fp, C.c_void_p, C.c_int64, fp]
        L.st_ao_dir.restype = None
        L.st_ao_factor.argtypes = [C.c_int, C.c_int]
        L.st_ao_factor.restype = C.c_float
        L.st_trace_samples.argtypes = [nzp, frp, fp, fp, fp, C.c_void_p, C.c_int64, fp, fp, fp, fp]
        L.st_trace_samples.restype = None
        _lib = L
    return _lib


def _a(x, width):
    return np.ascontiguousarray(x, np.float32).reshape(-1, width)


def normal(land, pos, w, eye):
    """get_normal(float4(pos, w)) with Eye = eye: (n, 3) float32."""
    pd = np.ascontiguousarray(np.concatenate([_a(pos, 3), _a(w, 1)], axis=1), np.float32)
    out = np.zeros((len(pd), 3), np.float32)
    fr = SH.frame(eye, land)
    lib().st_normal(C.byref(O.noise_tables()), C.byref(fr), O._fp(pd), len(pd), O._fp(out))
    return out


def fog(land, p, dist):
    """get_fog(p, dist): (n, 4) float32."""
    p, dist = _a(p, 3), _a(dist, 1)
    assert len(p) == len(dist)
    out = np.zeros((len(p), 4), np.float32)
    fr = SH.frame((0, 0, 0), land)
    lib().st_fog(C.byref(O.noise_tables()), C.byref(fr), O._fp(p), O._fp(dist), len(p), O._fp(out))
    return out


def pixel_ray(consts, px, py):
    """get_pixel_ray for the frame constants (oracle_lib.make_frame's dict): (p (n, 3), dir (n, 3)) float32."""
    pix = np.ascontiguousarray(np.stack([np.asarray(px, np.float32).ravel(), np.asarray(py, np.float32).ravel()], axis=1))
    p, d = np.zeros((len(pix), 3), np.float32), np.zeros((len(pix), 3), np.float32)
    fr = O.make_frame(consts)
    lib().st_pixel_ray(C.byref(O.noise_tables()), C.byref(fr), O._fp(pix), len(pix), O._fp(p), O._fp(d))
    return p, d


def color(land, p, n, d, dist, eye, sun=SH.SUN):
    """get_color(p, n, d, dist) with SunDirection = sun and Eye = eye (the shadow march's level of detail):
    (rgb (n, 3) float32, classes (n,) uint8: LIT or SHADOWED, the shadow ray's fcolord.w (n,) float32)."""
    p, n, d, dist = _a(p, 3), _a(n, 3), _a(d, 3), _a(dist, 1)
    assert len(p) == len(n) == len(d) == len(dist)
    rgb = np.zeros((len(p), 3), np.float32)
    cls = np.zeros(len(p), np.uint8)
    w = np.zeros(len(p), np.float32)
    fr = SH.frame(eye, land, sun)
    lib().st_color(C.byref(O.noise_tables()), C.byref(fr), O._fp(p), O._fp(n), O._fp(d), O._fp(dist), len(p), O._fp(rgb),
                   cls.ctypes.data, O._fp(w))
    return rgb, cls, w


def trace_ray(land, p, dist, enddist, stepmod, dir, eye, calcfog, skiprefine, max_steps=0, recording=0, sun=SH.SUN):
    """The oracle's trace_ray (tracing.hlsl:47-105) with every argument the caller's: p, dir (n, 3); dist, enddist,
    stepmod scalars or (n,); max_steps the build's cap (0: none).  (pd (n, 4), fcolord (n, 4), density (n,) float32,
    steps (n,) uint32)."""
    p, dir = _a(p, 3), _a(dir, 3)
    n = len(p)
    assert len(dir) == n
    dist, enddist, stepmod = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32).reshape(-1), (n,)))
                              for v in (dist, enddist, stepmod))
    pd, fc = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    dens, steps = np.zeros(n, np.float32), np.zeros(n, np.uint32)
    fr = SH.frame(eye, land, sun, recording)
    lib().st_trace_ray(C.byref(O.noise_tables()), C.byref(fr), O._fp(p), O._fp(dist), O._fp(enddist), O._fp(stepmod),
                       O._fp(dir), n, int(bool(calcfog)), int(bool(skiprefine)), int(max_steps), O._fp(pd), O._fp(fc),
                       O._fp(dens), steps.ctypes.data)
    return pd, fc, dens, steps


def aa_offsets(samples):
    """getSampleOffset(0 .. samples-1) as the oracle's tracescreen selects and scales them: (samples, 2) float32."""
    out = np.zeros((16, 2), np.float32)
    n = lib().st_aa_offsets(int(samples), O._fp(out))
    return out[:n].copy()


def pcg_hash(x):
    """The oracle's pcg_hash of uint32 words: uint32, the shape of x."""
    x = np.ascontiguousarray(x, np.uint32)
    out = np.zeros_like(x)
    lib().st_pcg_hash(x.ctypes.data, x.size, out.ctypes.data)
    return out


def ao_dir(normals, keys):
    """The oracle's ao_dir for normals (n, 3), used as given, and keys (n, 4) uint32 (px, py, a, k): (n, 3) float32."""
    nr = _a(normals, 3)
    keys = np.ascontiguousarray(keys, np.uint32).reshape(-1, 4)
    assert len(keys) == len(nr)
    out = np.zeros((len(nr), 3), np.float32)
    lib().st_ao_dir(O._fp(nr), keys.ctypes.data, len(nr), O._fp(out))
    return out


def ao_factor(occ, samples):
    """ambient_occlusion's factor for occ occluded rays of samples: a float32."""
    return np.float32(lib().st_ao_factor(int(occ), int(samples)))


def trace_samples(consts, land, p, dir, ranges, keys, aa=1, ao=0, max_steps=0):
    """The oracle's trace_sample for n rays as ro_tracescreen calls it for the frame of consts (oracle_lib.make_frame's
    dict) with these macros: p, dir (n, 3); ranges (n, 2) plane.x, plane.y; keys (n, 3) uint32 (px, py, a).
    (colour (n, 3), not saturated; ao (n,): 1 for a miss; the primary march's pd (n, 4) and density (n,)) float32."""
    p, dir, ranges = _a(p, 3), _a(dir, 3), _a(ranges, 2)
    keys = np.ascontiguousarray(keys, np.uint32).reshape(-1, 3)
    n = len(p)
    assert len(dir) == n and len(ranges) == n and len(keys) == n
    col, f, pd, dens = (np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros((n, 4), np.float32),
                        np.zeros(n, np.float32))
    fr = O.make_frame(consts, landscape=O.LANDSCAPES[land], aa=aa, ao=ao, max_steps=max_steps)
    lib().st_trace_samples(C.byref(O.noise_tables()), C.byref(fr), O._fp(p), O._fp(dir), O._fp(ranges), keys.ctypes.data,
                           n, O._fp(col), O._fp(f), O._fp(pd), O._fp(dens))
    return col, f, pd, dens


def shadow_precision(dist):
    """The stepmod get_color gives its shadow ray for a hit at dist (color.hlsl:47-50): (n,) float32."""
    dist = np.ascontiguousarray(dist, np.float32).reshape(-1)
    out = np.zeros(len(dist), np.float32)
    lib().st_shadow_precision(O._fp(dist), len(dist), O._fp(out))
    return out
