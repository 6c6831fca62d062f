"""The checker of the numeric primitives' sweeps (TEST INFRASTRUCTURE): builds, binds and caches
tests/tools/prim_sweep.cpp, which links the oracle and includes rt_math.h as host C++.  Built with the oracle's own
flags (-ffp-contract=off, OpenMP) into tests/tools/_build/.

Inputs are a triple (start pattern, odd multiplier m, count n) and a mask: input i has the float32 bit pattern
(start + i * m mod 2^32) & mask.  Function ids are rt_debug_math's (include/frosttrace.h), and for the host forms
without a device op EXP2_FIN, EXP_FIN, SINCOS_S, SINCOS_C."""
import ctypes as C
import os
import subprocess
from collections import namedtuple

import numpy as np

import surface_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "prim_sweep.cpp")
BUILD = os.path.join(ROOT, "tests", "tools", "_build")
SO = os.path.join(BUILD, "libprim_sweep.so")
CSRC = os.path.join(ROOT, "gpgpuraytrace_amd", "csrc")
ORACLE = os.path.join(ROOT, "oracle")

EXP2, LOG2, EXP, SIN, COS, SQRT, RCP, RSQRT, POW, MAX, MIN, POW_NONNEG, POW_WAVE, SWEEP, LOG2_NONNEG = \
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 16, 17
EXP2_FIN, EXP_FIN, SINCOS_S, SINCOS_C = 18, 19, 20, 21
NAMES = {0: "exp2", 1: "log2", 2: "exp", 3: "sin", 4: "cos", 5: "sqrt", 6: "rcp", 7: "rsqrt", 8: "pow", 9: "max",
         10: "min", 11: "pow_nonneg", 13: "pow_nonneg_wave", 17: "log2_nonneg", 18: "exp2_fin", 19: "exp_fin",
         20: "sincos.s", 21: "sincos.c"}
# domains: every pattern; finite x >= 0 (patterns below 0x7f800000); no NaN; finite
ALL, FINITE_NONNEG, NO_NAN, FINITE = 0, 1, 2, 3
FULL, NONNEG = 0xffffffff, 0x7fffffff
INF_BITS = 0x7f800000
# The exponents the shaders pass to pow_nonneg / pow_nonneg_wave, as float32 arithmetic gives them:
# np_expo = 0.68f + 0.1f (rt_runtime.cpp), 1.5, density_factor 0.35 and 0.15, 0.33, 40 (tests/test_gpu_prim_sweep.py
# says where each comes from).
EXPONENTS = (float(np.float32(0.68) + np.float32(0.1)), 1.5, float(np.float32(0.35)), float(np.float32(0.15)),
             float(np.float32(0.33)), 40.0)

Result = namedtuple("Result", "mismatches excluded first waves_special waves_ordinary")
Accuracy = namedtuple("Accuracy", "ulp ulp_at abs abs_at counted early_overflow")

_lib = None


def fbits(v):
    """The bit pattern of the float32 nearest v."""
    return int(np.array([v], np.float32).view(np.uint32)[0])


def lib():
    global _lib
    if _lib is None:
        osrc = os.path.join(ORACLE, "rt_oracle.c")
        deps = [SRC, osrc, os.path.join(ORACLE, "rt_oracle.h"), os.path.join(CSRC, "rt_math.h")]
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in deps):
            os.makedirs(BUILD, exist_ok=True)
            tmp = "%s.%d.tmp" % (SO, os.getpid())
            obj = "%s.%d.oracle.o" % (SO, os.getpid())
            cxx = [f for f in SR.CFLAGS if not f.startswith("-std=")]
            try:
                subprocess.run(["gcc"] + SR.CFLAGS + ["-c", "-o", obj, osrc], check=True)
                subprocess.run(["g++", "-std=c++17"] + cxx + ["-I", CSRC, "-I", ORACLE, "-shared", "-o", tmp, SRC, obj,
                                                            "-lm"], check=True)
            finally:
                if os.path.exists(obj):
                    os.unlink(obj)
            os.replace(tmp, SO)
        L = C.CDLL(SO)
        u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
        L.ps_compare.argtypes = [C.c_int, u32, u32, u32, u32, u64, C.c_int, vp, C.c_int, vp, vp]
        L.ps_host_compare.argtypes = [C.c_int, u32, u32, u32, u32, u64, C.c_int, vp, vp]
        L.ps_accuracy.argtypes = [C.c_int, u32, u32, u32, u32, u64, C.c_float, C.c_float, C.c_double, vp, vp, vp]
        L.ps_pairs.argtypes = [C.c_int, vp, vp, u64, vp]
        L.ps_pairs.restype = C.c_int64
        _lib = L
    return _lib


def _result(k, counts, first):
    assert k >= 0, "bad arguments"
    return Result(int(counts[0]), int(counts[1]), [tuple(int(v) for v in first[i]) for i in range(k)], int(counts[2]),
                  int(counts[3]))


def compare(op, got, start, mult=1, mask=FULL, y=0.0, domain=ALL, census=False):
    """got (n results, float32 or uint32) against the oracle's op at the inputs of (start, mult, len(got)) under
    mask, y the second operand: Result(mismatches, inputs left out as outside the domain, the first 16 mismatches as
    (input bits, got, want), and with census the waves of 64 inputs with / without a lane whose y * log2(x) is
    outside [-150, 128) or not finite)."""
    g = np.ascontiguousarray(got).reshape(-1)
    assert g.dtype.itemsize == 4
    counts, first = np.zeros(4, np.uint64), np.zeros((16, 3), np.uint32)
    k = lib().ps_compare(op, fbits(y), start & FULL, mult & FULL, mask, g.size, domain, g.ctypes.data, int(census),
                         counts.ctypes.data, first.ctypes.data)
    return _result(k, counts, first)


def host_compare(fn, start, n, mult=1, mask=FULL, y=0.0, domain=ALL):
    """rt_math.h's host function fn against the oracle at the inputs of (start, mult, n) under mask."""
    counts, first = np.zeros(4, np.uint64), np.zeros((16, 3), np.uint32)
    k = lib().ps_host_compare(fn, fbits(y), start & FULL, mult & FULL, mask, int(n), domain, counts.ctypes.data,
                              first.ctypes.data)
    return _result(k, counts, first)


def accuracy(op, start, n, lo, hi, mult=1, mask=FULL, y=0.0, ulp_floor=0.0):
    """The oracle's op against double-precision libm at the inputs of (start, mult, n) with lo <= x <= hi:
    Accuracy(worst error in float32 ulps of the reference, its input bits, worst absolute error, its input bits,
    inputs counted, inputs left out because the oracle's result is infinite where the reference still fits float32).
    Inputs whose reference is beyond float32 are not looked at."""
    worst, where, counted = np.zeros(2, np.float64), np.zeros(2, np.uint32), np.zeros(2, np.uint64)
    rc = lib().ps_accuracy(op, fbits(y), start & FULL, mult & FULL, mask, int(n), lo, hi, ulp_floor, worst.ctypes.data,
                           where.ctypes.data, counted.ctypes.data)
    assert rc == 0, "bad arguments"
    return Accuracy(float(worst[0]), int(where[0]), float(worst[1]), int(where[1]), int(counted[0]), int(counted[1]))


def host_pairs(fn, a, b):
    """rt_math.h's host pow / max / min against the oracle for the pairs (a[i], b[i]) (uint32 bit patterns):
    (mismatches, the first 16 as (a, b, got, want))."""
    a, b = np.ascontiguousarray(a, np.uint32), np.ascontiguousarray(b, np.uint32)
    assert a.shape == b.shape
    first = np.zeros((16, 4), np.uint32)
    bad = lib().ps_pairs(fn, a.ctypes.data, b.ctypes.data, a.size, first.ctypes.data)
    assert bad >= 0, "bad arguments"
    return int(bad), [tuple(int(v) for v in first[i]) for i in range(min(bad, 16))]


def describe(name, r, y=None):
    """The message for a Result with mismatches: the op, the input pattern(s), the results on both sides."""
    head = "%s%s: %d mismatches" % (name, "" if y is None else " (y = %r, bits 0x%08x)" % (y, fbits(y)), r.mismatches)
    return head + "".join("\n  x = 0x%08x (%r): got 0x%08x (%r), oracle 0x%08x (%r)" % (
        x, _f(x), g, _f(g), w, _f(w)) for x, g, w in r.first)


def _f(u):
    return float(np.array([u], np.uint32).view(np.float32)[0])


_edges = None


def edge_values():
    """The edge set of the binary ops' pair tests, as uint32 bit patterns (read-only, about 1,500): both signs of
    zero, of the smallest and largest subnormals and normals and of 1 with their neighbours, of every power of two,
    of infinity, of quiet and signalling NaNs with several payloads, and 1,024 fixed-seed random patterns."""
    global _edges
    if _edges is None:
        pos = []
        for c in (0x00000000, 0x00000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0x3f800000):
            pos += [c + d for d in (-2, -1, 0, 1, 2) if 0 <= c + d < INF_BITS]
        pos += [e << 23 for e in range(1, 255)]              # the normal powers of two
        pos += [1 << k for k in range(23)]                   # the subnormal ones
        pos += [INF_BITS]
        pos += [0x7fc00000, 0x7fc00001, 0x7fd5aaaa, 0x7fffffff,   # quiet NaNs
                0x7f800001, 0x7f8abcde, 0x7fa00000, 0x7fbfffff]   # signalling NaNs
        pos = sorted(set(pos))
        both = pos + [p | 0x80000000 for p in pos]
        rnd = np.random.default_rng(20).integers(0, 1 << 32, 1024, dtype=np.uint64).astype(np.uint32)
        _edges = np.concatenate([np.array(both, np.uint32), rnd])
        _edges.setflags(write=False)
    return _edges


def edge_pairs():
    """Every ordered pair of edge_values(): (a, b) uint32 arrays."""
    e = edge_values()
    return np.repeat(e, e.size), np.tile(e, e.size)
