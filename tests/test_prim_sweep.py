"""The numeric primitives over every float32 input, on the CPU ("The primitives over every
input"): rt_math.h's host branches against the oracle bit for bit (prim_ref.host_compare), the oracle against
double-precision libm (prim_ref.accuracy), and the host branches once more under ASan + UBSan in a program of their
own (tests/tools/prim_check.cpp).  The exhaustive forms are marked slow; the quick forms take every 4,099th pattern
and the patterns within 2 of every binade boundary, of the log2 mantissa split 0x3fb504f3 in every binade and of
the exp2 thresholds -150 and 128.  Threads come from OMP_NUM_THREADS (8 without it).

Measured, exhaustively (the tests print these figures; the bounds asserted are rt_math.h's own claims):
  exp2 on [-150, 128)                  0.952 ulp at 0xbefdf4fb
  log2 on finite x > 0, floor 2^-24    1.086 ulp at 0x3f34e3f1
  sin, cos on |x| <= 1e5               7.43e-8 absolute each"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import prim_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE = 4099
STRIDED = (1 << 32) // STRIDE + 1
# (function, domain): every function of rt_math.h with a counterpart in the oracle and one float argument
UNARY = [(P.EXP2, P.ALL), (P.LOG2, P.ALL), (P.EXP, P.ALL), (P.SIN, P.ALL), (P.COS, P.ALL), (P.SQRT, P.ALL),
         (P.RCP, P.ALL), (P.RSQRT, P.ALL), (P.LOG2_NONNEG, P.FINITE_NONNEG), (P.EXP2_FIN, P.NO_NAN),
         (P.EXP_FIN, P.NO_NAN), (P.SINCOS_S, P.FINITE), (P.SINCOS_C, P.FINITE)]
# the patterns each domain leaves out of all 2^32: none; the negative and the non-finite; the NaNs; the non-finite
LEFT_OUT = {P.ALL: 0, P.FINITE_NONNEG: (1 << 32) - P.INF_BITS, P.NO_NAN: 2 * ((1 << 23) - 1), P.FINITE: 1 << 24}
POWS = [(fn, y) for y in P.EXPONENTS for fn in (P.POW, P.POW_NONNEG, P.POW_WAVE)]
NONFINITE_NONNEG = 1 << 23  # the patterns 0x7f800000 .. 0x7fffffff


UNARY_IDS = [P.NAMES[fn] for fn, _ in UNARY]
POW_IDS = ["%s-%g" % (P.NAMES[fn], y) for fn, y in POWS]


def centres(signs=(0, 0x80000000)):
    """The patterns the quick forms look around: every binade's boundary and log2 split, and the exp2 thresholds."""
    c = [s | (e << 23) | m for s in signs for e in range(256) for m in (0, 0x3504f3)]
    return c + [P.fbits(-150.0), P.fbits(128.0)]


def quick(fn, mask=P.FULL, y=0.0, domain=P.ALL, signs=(0, 0x80000000)):
    r = P.host_compare(fn, 0, STRIDED, mult=STRIDE, mask=mask, y=y, domain=domain)
    assert r.mismatches == 0, P.describe(P.NAMES[fn], r, y)
    assert r.excluded < STRIDED
    for c in centres(signs):
        r = P.host_compare(fn, c - 2, 5, mask=mask, y=y, domain=domain)
        assert r.mismatches == 0, P.describe(P.NAMES[fn], r, y)


@pytest.mark.parametrize("fn,domain", UNARY, ids=UNARY_IDS)
def test_host_unary_quick(fn, domain):
    quick(fn, domain=domain)


@pytest.mark.parametrize("fn,y", POWS, ids=POW_IDS)
def test_host_pow_quick(fn, y):
    quick(fn, mask=P.NONNEG, y=y, domain=P.FINITE_NONNEG, signs=(0,))


@pytest.mark.parametrize("fn", [P.POW, P.MAX, P.MIN], ids=["pow", "max", "min"])
def test_host_edge_pairs(fn):
    """Host pow, max and min against the oracle for every ordered pair of the edge set."""
    a, b = P.edge_pairs()
    bad, first = P.host_pairs(fn, a, b)
    assert bad == 0, "%s: %d mismatches, first (a, b, got, want) %s" % (
        P.NAMES[fn], bad, ["0x%08x 0x%08x 0x%08x 0x%08x" % f for f in first])


@pytest.mark.slow
@pytest.mark.parametrize("fn,domain", UNARY, ids=UNARY_IDS)
def test_host_unary_exhaustive(fn, domain):
    r = P.host_compare(fn, 0, 1 << 32, domain=domain)
    assert r.mismatches == 0, P.describe(P.NAMES[fn], r)
    assert r.excluded == LEFT_OUT[domain]


@pytest.mark.slow
@pytest.mark.parametrize("fn,y", POWS, ids=POW_IDS)
def test_host_pow_exhaustive(fn, y):
    """Every finite x >= 0: the 2^23 non-finite patterns from 0x7f800000 are left out, and nothing else."""
    r = P.host_compare(fn, 0, 1 << 31, mask=P.NONNEG, y=y, domain=P.FINITE_NONNEG)
    assert r.mismatches == 0, P.describe(P.NAMES[fn], r, y)
    assert r.excluded == NONFINITE_NONNEG


def test_helper_notices_a_wrong_bit():
    """compare() reports a flipped low bit, names the input, and treats NaNs of any payload as equal."""
    import oracle_lib as O
    start, mult, n = 0x3f000000, 0x9e3779b1, 4096
    x = (start + np.arange(n, dtype=np.uint64) * mult).astype(np.uint32)
    y = O.unary(P.LOG2, x.view(np.float32)).view(np.uint32).copy()
    assert P.compare(P.LOG2, y, start, mult).mismatches == 0
    nan = int(np.flatnonzero((y & 0x7fffffff) > P.INF_BITS)[0])
    y[nan] ^= 0x1234
    assert P.compare(P.LOG2, y, start, mult).mismatches == 0
    ok = int(np.flatnonzero((y & 0x7fffffff) < P.INF_BITS)[7])
    want = int(y[ok])
    y[ok] ^= 1
    r = P.compare(P.LOG2, y, start, mult)
    assert r.mismatches == 1 and r.first == [(int(x[ok]), want ^ 1, want)]
    r = P.compare(P.LOG2, y, start, mult, domain=P.FINITE_NONNEG)
    assert r.excluded == int(np.count_nonzero(x >= P.INF_BITS)) and r.mismatches == (1 if x[ok] < P.INF_BITS else 0)


def test_mixed_order_wave_census():
    """What the device test of pow_nonneg_wave in mixed order relies on, from the oracle's own y * log2(x): with the
    multiplier 0x9e3779b1 over the non-negative patterns, a wave of 64 holds a non-finite lane (the clamped path) in
    about a quarter of the waves for the exponents below 1, and nearly every wave has a lane out of range for 1.5
    and 40.  A 2^22-element slice; the device test counts the whole 2^31."""
    n = 1 << 22
    for y in P.EXPONENTS:
        r = P.compare(P.POW_WAVE, np.zeros(n, np.uint32), 0, 0x9e3779b1, P.NONNEG, y=y, domain=P.FINITE_NONNEG,
                      census=True)
        waves = r.waves_special + r.waves_ordinary
        assert waves == n // 64
        print("y = %g: %d special, %d ordinary waves" % (y, r.waves_special, r.waves_ordinary))
        if y < 1:
            assert r.waves_special >= waves // 100 and r.waves_ordinary >= waves // 100
        else:
            assert r.waves_special >= waves * 99 // 100


# --- the oracle against double-precision libm ---------------------------------------------------------------
BELOW_128 = float(np.nextafter(np.float32(128), np.float32(0)))
TINY, HUGE = float(np.float32(1e-45)), float(np.finfo(np.float32).max)
# (op, lo, hi, ulp floor, bound in ulps or None, absolute bound or None): rt_math.h's claims
CLAIMS = [(P.EXP2, -150.0, BELOW_128, 0.0, 2.0, None), (P.LOG2, TINY, HUGE, 2.0 ** -24, 2.0, None),
          (P.SIN, -1e5, 1e5, 0.0, None, 2e-7), (P.COS, -1e5, 1e5, 0.0, None, 2e-7)]


def claim(op, lo, hi, floor, ulps, absolute, n, mult):
    a = P.accuracy(op, 0, n, lo, hi, mult=mult, ulp_floor=floor)
    print("%s on [%g, %g]: %.4f ulp at 0x%08x, %.4g absolute at 0x%08x, %d inputs" % (
        P.NAMES[op], lo, hi, a.ulp, a.ulp_at, a.abs, a.abs_at, a.counted))
    assert a.counted > 0 and a.early_overflow == 0
    if ulps is not None:
        assert a.ulp <= ulps, "%s: %.4f ulp at 0x%08x" % (P.NAMES[op], a.ulp, a.ulp_at)
    if absolute is not None:
        assert a.abs <= absolute, "%s: %.4g at 0x%08x" % (P.NAMES[op], a.abs, a.abs_at)
    return a


@pytest.mark.parametrize("op,lo,hi,floor,ulps,absolute", CLAIMS, ids=["exp2", "log2", "sin", "cos"])
def test_accuracy_quick(op, lo, hi, floor, ulps, absolute):
    claim(op, lo, hi, floor, ulps, absolute, STRIDED, STRIDE)


@pytest.mark.slow
@pytest.mark.parametrize("op,lo,hi,floor,ulps,absolute", CLAIMS, ids=["exp2", "log2", "sin", "cos"])
def test_accuracy_exhaustive(op, lo, hi, floor, ulps, absolute):
    a = claim(op, lo, hi, floor, ulps, absolute, 1 << 32, 1)
    # every float of the domain was looked at
    if op == P.EXP2:
        assert a.counted == P.fbits(BELOW_128) + 1 + P.fbits(-150.0) - 0x80000000 + 1
    elif op == P.LOG2:
        assert a.counted == P.INF_BITS - 1
    else:
        assert a.counted == 2 * (P.fbits(1e5) + 1)


def record(n, mult):
    """exp and pow are exp2(y * log2 x): the rounding of the argument is scaled by |y log2 x|, so their error is a
    consequence of the definition, recorded and not bounded; the bit-exact comparisons guard them."""
    a = P.accuracy(P.EXP, 0, n, -88.0, 88.0, mult=mult)
    print("exp on |x| <= 88: %.2f ulp at 0x%08x" % (a.ulp, a.ulp_at))
    assert a.counted > 0
    for y in P.EXPONENTS:
        a = P.accuracy(P.POW, 0, n, 0.0, HUGE, mult=mult, mask=P.NONNEG, y=y)
        print("pow(x, %g) on finite x >= 0: %.2f ulp at 0x%08x, %d inputs, %d more infinite before the reference is" % (
            y, a.ulp, a.ulp_at, a.counted, a.early_overflow))
        assert a.counted > 0


def test_exp_pow_error_recorded_quick():
    record(STRIDED, STRIDE)


@pytest.mark.slow
def test_exp_pow_error_recorded_exhaustive():
    record(1 << 31, 1)


def test_prim_check_under_sanitizers(tmp_path):
    """tests/tools/prim_check.cpp: the quick host sweep and the edge pairs under ASan + UBSan with
    float-cast-overflow.  Its own main, its own process: nothing of it is loaded into this interpreter."""
    cc, cxx = shutil.which("gcc"), shutil.which("g++")
    assert cc and cxx, "gcc and g++ are needed to build tests/tools/prim_check.cpp"
    san = ["-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unknown-pragmas",
           "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined,float-cast-overflow"]
    obj, exe = str(tmp_path / "rt_oracle.o"), str(tmp_path / "prim_check")
    # (the oracle is not the code under test here: without OpenMP its thread counts are unused variables)
    subprocess.run([cc, "-std=c11", "-Wno-unused-variable"] + san + ["-c", "-o", obj, os.path.join(ROOT, "oracle", "rt_oracle.c")], check=True)
    subprocess.run([cxx, "-std=c++17"] + san + ["-static-libasan", "-static-libubsan", "-I",
                    os.path.join(ROOT, "gpgpuraytrace_amd", "csrc"), "-I", os.path.join(ROOT, "oracle"),
                    os.path.join(ROOT, "tests", "tools", "prim_check.cpp"), obj, "-lm", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("prim_check ok")
