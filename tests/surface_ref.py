"""The checker of the surface queries (TEST INFRASTRUCTURE): builds, binds and caches tests/tools/surface_ref.c,
which includes the oracle's source and runs its refined march (trace_ray with skiprefine off) and get_normal for
rays of the caller's own.  Built with the oracle's own flags into tests/tools/_build/."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as O
import ray_fixture as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "surface_ref.c")
SO = os.path.join(ROOT, "tests", "tools", "_build", "libsurface_ref.so")
# oracle/Makefile's CFLAGS
CFLAGS = ["-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-Wall", "-Wno-unknown-pragmas"]
T_MIN, T_MAX = 0.01, 5000.0

_lib = None
_cache = {}


def lib():
    global _lib
    if _lib is None:
        deps = [SRC, os.path.join(ROOT, "oracle", "rt_oracle.c"), os.path.join(ROOT, "oracle", "rt_oracle.h")]
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in deps):
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            tmp = "%s.%d.tmp" % (SO, os.getpid())
            subprocess.run(["gcc"] + CFLAGS + ["-shared", "-o", tmp, SRC, "-lm"], check=True)
            os.replace(tmp, SO)
        L = C.CDLL(SO)
        fp = C.POINTER(C.c_float)
        L.sr_trace_surface.argtypes = [C.POINTER(O.Noise), C.POINTER(O.Frame), fp, fp, fp, C.c_int64, C.c_float,
                                       C.c_float, C.c_float, C.c_int, fp, C.c_void_p]
        L.sr_trace_surface.restype = None
        _lib = L
    return _lib


def trace(origins, dirs, eye, landscape, ranges=None, t_min=T_MIN, t_max=T_MAX, stepmod=1.0, max_steps=0,
          recording=0):
    """(results (n, 8) float32, steps (n,) uint32) of the definition in include/frosttrace.h for these rays."""
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    n = len(o)
    consts = dict(RF.consts("F0"))
    consts["eye"] = np.array([eye[0], eye[1], eye[2], 0], np.float32)
    fr = O.make_frame(consts, landscape=O.LANDSCAPES[landscape], recording=recording)
    res = np.zeros((n, 8), np.float32)
    steps = np.zeros(n, np.uint32)
    rg = None
    if ranges is not None:
        rg = np.ascontiguousarray(ranges, np.float32).reshape(-1, 2)
        assert len(rg) == n
    lib().sr_trace_surface(C.byref(O.noise_tables()), C.byref(fr), O._fp(o), O._fp(d), O._fp(rg) if rg is not None else None,
                           n, t_min, t_max, stepmod, max_steps, O._fp(res), steps.ctypes.data)
    return res, steps


def seeded_ranges(n=4096):
    """The per-ray ranges of the tests: default_rng(7), t_min from {0.01, 0.5, 3, 40}, t_max from {25, 100, 5000}."""
    rng = np.random.default_rng(7)
    t0 = rng.choice(np.array([0.01, 0.5, 3, 40], np.float32), n)
    t1 = rng.choice(np.array([25, 100, 5000], np.float32), n)
    return np.stack([t0, t1], axis=1).astype(np.float32)


def query(names, landscape, eye=None, ranged=False, **kw):
    """The fixture cameras' rays (ray_fixture.query) through trace(); eye: a camera's name (default: the first's).
    Computed once per argument set, read-only."""
    names = tuple(names)
    key = (names, landscape, eye, ranged, tuple(sorted(kw.items())))
    if key not in _cache:
        o, d = RF.query(names)
        rg = seeded_ranges(len(o)) if ranged else None
        res, steps = trace(o, d, RF.eye(eye or names[0]), landscape, ranges=rg, **kw)
        res.setflags(write=False)
        steps.setflags(write=False)
        _cache[key] = (res, steps)
    return _cache[key]
