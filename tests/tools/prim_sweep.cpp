// prim_sweep.cpp -- TEST INFRASTRUCTURE: sweeps of the numeric primitives over
// float32 bit patterns, bound by tests/prim_ref.py.  Links the oracle (oracle/rt_oracle.c, the definition) and
// includes rt_math.h compiled as host C++ (the branches the host constant builder runs).
//
// Inputs are a triple (start, odd multiplier m, count n) and a mask: input i has the bit pattern
// (start + i * m mod 2^32) & mask.  A wave is 64 consecutive i.
//   ps_compare       device results (or any buffer of n results) against the oracle
//   ps_host_compare  the rtm:: host function against the oracle
//   ps_accuracy      the oracle against double-precision libm
//   ps_pairs         the rtm:: host pow / max / min against the oracle for explicit operand pairs
// Function ids: 0 exp2, 1 log2, 2 exp, 3 sin, 4 cos, 5 sqrt, 6 rcp, 7 rcp(sqrt), 8 pow, 9 max, 10 min,
// 11 pow_nonneg, 13 pow_nonneg_wave, 17 log2_nonneg (rt_debug_math's numbers); host only: 18 exp2_fin, 19 exp_fin,
// 20 / 21 sincos' sine / cosine.  Domains: 0 every pattern, 1 finite x >= 0 (patterns below 0x7f800000), 2 no NaN,
// 3 finite.  An input outside the domain is not evaluated and is counted as left out.
// Threads: OMP_NUM_THREADS, 8 without it; never the CPU count.
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "rt_math.h"
#include "rt_oracle.h"

namespace {

enum { kAll = 0, kFiniteNonneg = 1, kNoNan = 2, kFinite = 3 };
enum { kFirst = 16 };

inline uint32_t f2u(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
inline float u2f(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}
inline uint32_t pattern(uint32_t start, uint32_t mult, uint32_t mask, uint64_t i) { return (start + (uint32_t)i * mult) & mask; }
inline bool in_domain(int dom, uint32_t p)
{
    const uint32_t mag = p & 0x7fffffffu;
    switch (dom) {
    case kFiniteNonneg: return p < 0x7f800000u;
    case kNoNan: return mag <= 0x7f800000u;
    case kFinite: return mag < 0x7f800000u;
    default: return true;
    }
}
// equal bit patterns, or both NaN (bits_equal of tests/test_gpu_parity.py)
inline bool same(uint32_t a, uint32_t b) { return a == b || ((a & 0x7fffffffu) > 0x7f800000u && (b & 0x7fffffffu) > 0x7f800000u); }

int threads()
{
    const char* s = getenv("OMP_NUM_THREADS");
    const int t = s ? atoi(s) : 8;
    return t < 1 ? 1 : (t > 256 ? 256 : t);
}

// the definition: the oracle's function for an id; < 0 for an id it has no counterpart of
bool oracle_has(int fn) { return (fn >= 0 && fn <= 11) || fn == 13 || (fn >= 17 && fn <= 21); }
float oracle_eval(int fn, float x, float y)
{
    float r;
    switch (fn) {
    case 0: case 18: return ro_exp2(x);
    case 1: case 17: return ro_log2(x);
    case 2: case 19: return ro_exp(x);
    case 3: case 20: return ro_sin(x);
    case 4: case 21: return ro_cos(x);
    case 5: case 6: case 7: ro_batch_unary(fn, &x, &r, 1); return r; // sqrt, rcp, rcp(sqrt) as the oracle states them
    case 9: return ro_max(x, y);
    case 10: return ro_min(x, y);
    default: return ro_pow(x, y); // 8, 11, 13
    }
}
float host_eval(int fn, float x, float y)
{
    float s, c;
    switch (fn) {
    case 0: return rtm::exp2(x);
    case 1: return rtm::log2(x);
    case 2: return rtm::exp(x);
    case 3: return rtm::sin(x);
    case 4: return rtm::cos(x);
    case 5: return rtm::sqrt(x);
    case 6: return rtm::rcp(x);
    case 7: return rtm::rcp(rtm::sqrt(x));
    case 8: return rtm::pow(x, y);
    case 9: return rtm::max(x, y);
    case 10: return rtm::min(x, y);
    case 11: return rtm::pow_nonneg(x, y);
    case 13: return rtm::pow_nonneg_wave(x, y);
    case 17: return rtm::log2_nonneg(x);
    case 18: return rtm::exp2_fin(x);
    case 19: return rtm::exp_fin(x);
    case 20: rtm::sincos(x, &s, &c); return s;
    default: rtm::sincos(x, &s, &c); return c;
    }
}

// got: n results, or null for the rtm:: host function.  counts: mismatches, inputs left out, and with census the
// waves that hold a lane whose y * log2(x) (the oracle's) is outside [-150, 128) or not finite, and the waves
// that hold none.  first: up to 16 (input bits, got, want) in order of i.  Returns how many of them it wrote.
int sweep(int fn, uint32_t ybits, uint32_t start, uint32_t mult, uint32_t mask, uint64_t n, int dom, const uint32_t* got,
          int census, uint64_t* counts, uint32_t* first)
{
    if (!oracle_has(fn) || !counts || !(mult & 1u)) return -1;
    const float y = u2f(ybits);
    const uint64_t waves = (n + 63) / 64;
    uint64_t bad = 0, out = 0, special = 0;
    const int nt = threads();
    (void)nt; // (unused in a build without OpenMP)
#pragma omp parallel for schedule(static) num_threads(nt) reduction(+ : bad, out, special) if (waves > 64)
    for (uint64_t w = 0; w < waves; ++w) {
        const uint64_t end = (w * 64 + 64 < n) ? w * 64 + 64 : n;
        bool sp = false;
        for (uint64_t i = w * 64; i < end; ++i) {
            const uint32_t p = pattern(start, mult, mask, i);
            const float x = u2f(p);
            if (census) {
                const float a = y * ro_log2(x);
                sp = sp || !(a >= -150.0f && a < 128.0f);
            }
            if (!in_domain(dom, p)) {
                ++out;
                continue;
            }
            const uint32_t want = f2u(oracle_eval(fn, x, y));
            const uint32_t have = got ? got[i] : f2u(host_eval(fn, x, y));
            bad += !same(have, want);
        }
        special += sp;
    }
    counts[0] = bad;
    counts[1] = out;
    counts[2] = census ? special : 0;
    counts[3] = census ? waves - special : 0;
    int k = 0;
    for (uint64_t i = 0; bad && first && i < n && k < kFirst; ++i) {
        const uint32_t p = pattern(start, mult, mask, i);
        if (!in_domain(dom, p)) continue;
        const float x = u2f(p);
        const uint32_t want = f2u(oracle_eval(fn, x, y));
        const uint32_t have = got ? got[i] : f2u(host_eval(fn, x, y));
        if (same(have, want)) continue;
        first[3 * k] = p;
        first[3 * k + 1] = have;
        first[3 * k + 2] = want;
        ++k;
    }
    return k;
}

// double-precision libm at the float's exact value
bool libm_has(int fn) { return (fn >= 0 && fn <= 4) || fn == 8; }
double libm_eval(int fn, double x, double y)
{
    switch (fn) {
    case 0: return ::exp2(x);
    case 1: return ::log2(x);
    case 2: return ::exp(x);
    case 3: return ::sin(x);
    case 4: return ::cos(x);
    default: return ::pow(x, y);
    }
}
// the spacing of float32 at the reference rounded to float32 (numpy's spacing(abs(float32(ref))))
double ulp32(double ref)
{
    const float r = fabsf((float)ref);
    const float up = nextafterf(r, INFINITY);
    return up < INFINITY ? (double)up - (double)r : ldexp(1.0, 104); // (the top binade's spacing at FLT_MAX)
}

struct Worst {
    double ulp, abs;
    uint32_t at_ulp, at_abs;
    uint64_t n, early;
};
inline void take(Worst& a, const Worst& b)
{
    // (ties go to the smaller pattern, so that the answer does not depend on the thread count)
    if (b.ulp > a.ulp || (b.ulp == a.ulp && b.n && b.at_ulp < a.at_ulp)) a.ulp = b.ulp, a.at_ulp = b.at_ulp;
    if (b.abs > a.abs || (b.abs == a.abs && b.n && b.at_abs < a.at_abs)) a.abs = b.abs, a.at_abs = b.at_abs;
    a.n += b.n;
    a.early += b.early;
}

} // namespace

extern "C" {

int ps_compare(int op, uint32_t ybits, uint32_t start, uint32_t mult, uint32_t mask, uint64_t n, int domain,
               const uint32_t* got, int census, uint64_t* counts, uint32_t* first)
{
    if (!got) return -1;
    return sweep(op, ybits, start, mult, mask, n, domain, got, census, counts, first);
}

int ps_host_compare(int fn, uint32_t ybits, uint32_t start, uint32_t mult, uint32_t mask, uint64_t n, int domain,
                    uint64_t* counts, uint32_t* first)
{
    return sweep(fn, ybits, start, mult, mask, n, domain, nullptr, 0, counts, first);
}

// The oracle's op against libm in double over the inputs with lo <= x <= hi (NaN never is).  worst: the largest
// error in float32 ulps of the reference (an ulp no smaller than ulp_floor) and the largest absolute error; where:
// the input bits of each; counted[0]: the inputs in [lo, hi] whose reference is finite in float32 and that went into
// worst; counted[1]: those among them left out of worst because the oracle's result is infinite all the same (pow's
// early overflow at the top of the range).  Returns 0, or -1 for an op libm has no counterpart of.
int ps_accuracy(int op, uint32_t ybits, uint32_t start, uint32_t mult, uint32_t mask, uint64_t n, float lo, float hi,
                double ulp_floor, double* worst, uint32_t* where, uint64_t* counted)
{
    if (!libm_has(op) || !worst || !where || !counted || !(mult & 1u)) return -1;
    const float y = u2f(ybits);
    const int nt = threads();
    (void)nt;
    const uint64_t blocks = (n + 4095) / 4096;
    Worst all = {-1.0, -1.0, 0xffffffffu, 0xffffffffu, 0, 0};
#pragma omp parallel num_threads(nt) if (blocks > 4)
    {
        Worst mine = {-1.0, -1.0, 0xffffffffu, 0xffffffffu, 0, 0};
#pragma omp for schedule(static) nowait
        for (uint64_t b = 0; b < blocks; ++b) {
            const uint64_t end = (b * 4096 + 4096 < n) ? b * 4096 + 4096 : n;
            for (uint64_t i = b * 4096; i < end; ++i) {
                const uint32_t p = pattern(start, mult, mask, i);
                const float x = u2f(p);
                if (!(x >= lo && x <= hi)) continue;
                const double ref = libm_eval(op, (double)x, (double)y);
                if (!(fabsf((float)ref) < INFINITY)) continue; // (a reference beyond float32 has no ulp)
                const double have = (double)oracle_eval(op, x, y);
                if (fabs(have) == INFINITY) {
                    ++mine.early;
                    continue;
                }
                const double err = fabs(have - ref);
                const double u = ulp32(ref);
                Worst one = {err / (u > ulp_floor ? u : ulp_floor), err, p, p, 1, 0};
                take(mine, one);
            }
        }
#pragma omp critical
        take(all, mine);
    }
    worst[0] = all.ulp;
    worst[1] = all.abs;
    where[0] = all.at_ulp;
    where[1] = all.at_abs;
    counted[0] = all.n;
    counted[1] = all.early;
    return 0;
}

// The rtm:: host pow (8), max (9) or min (10) against the oracle for n explicit pairs (bit patterns).  Returns the
// mismatch count (< 0: bad arguments); first: up to 16 (a, b, got, want).
int64_t ps_pairs(int fn, const uint32_t* a, const uint32_t* b, uint64_t n, uint32_t* first)
{
    if (fn < 8 || fn > 10 || !a || !b) return -1;
    int64_t bad = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const float x = u2f(a[i]), y = u2f(b[i]);
        const uint32_t want = f2u(oracle_eval(fn, x, y)), have = f2u(host_eval(fn, x, y));
        if (same(have, want)) continue;
        if (first && bad < kFirst) {
            uint32_t* f = first + 4 * bad;
            f[0] = a[i], f[1] = b[i], f[2] = have, f[3] = want;
        }
        ++bad;
    }
    return bad;
}

} // extern "C"
