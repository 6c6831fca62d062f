// prim_check.cpp -- TEST INFRASTRUCTURE: rt_math.h's host branches against the oracle under ASan + UBSan (with
// float-cast-overflow: the (int)n of exp2 and the quadrant cast of sincos convert floats to int), as a program of
// its own (tests/test_prim_sweep.py builds and runs it; nothing of it is loaded into an interpreter, nothing of it
// runs on a GPU).  The quick strided sweep of every host function (every 4,099th pattern and the patterns around
// every binade boundary, the log2 mantissa split and the exp2 thresholds) and every ordered pair of an edge set
// for pow, max and min.
#include <stdio.h>

#include <vector>

#include "prim_sweep.cpp"

namespace {

int failures = 0;

void report(const char* what, int fn, uint64_t bad, const uint32_t* first, int k)
{
    if (!bad) return;
    ++failures;
    printf("%s fn %d: %llu mismatches\n", what, fn, (unsigned long long)bad);
    for (int i = 0; i < k; ++i) printf("  x 0x%08x got 0x%08x want 0x%08x\n", first[3 * i], first[3 * i + 1], first[3 * i + 2]);
}

void host(int fn, float y, uint32_t start, uint32_t mult, uint32_t mask, uint64_t n, int dom)
{
    uint64_t counts[4];
    uint32_t first[3 * kFirst];
    const int k = ps_host_compare(fn, f2u(y), start, mult, mask, n, dom, counts, first);
    if (k < 0) {
        ++failures;
        printf("fn %d: bad arguments\n", fn);
        return;
    }
    report("sweep", fn, counts[0], first, k);
}

void quick(int fn, float y, uint32_t mask, int dom)
{
    host(fn, y, 0u, 4099u, mask, (1ull << 32) / 4099u + 1u, dom);
    for (uint32_t e = 0; e < 256; ++e)
        for (uint32_t sign = 0; sign < 2; ++sign) {
            const uint32_t s = sign << 31;
            host(fn, y, (s | (e << 23)) - 2u, 1u, mask, 5, dom);              // the binade's boundary
            host(fn, y, (s | (e << 23) | 0x3504f3u) - 2u, 1u, mask, 5, dom);  // its log2 mantissa split
        }
    host(fn, y, f2u(-150.0f) - 2u, 1u, mask, 5, dom);
    host(fn, y, f2u(128.0f) - 2u, 1u, mask, 5, dom);
}

std::vector<uint32_t> edges()
{
    std::vector<uint32_t> pos;
    const uint32_t centres[] = {0x00000000u, 0x00000001u, 0x007fffffu, 0x00800000u, 0x7f7fffffu, 0x3f800000u};
    for (uint32_t c : centres)
        for (int d = -2; d <= 2; ++d)
            if ((int64_t)c + d >= 0 && (int64_t)c + d < 0x7f800000) pos.push_back((uint32_t)((int64_t)c + d));
    for (uint32_t e = 1; e < 255; ++e) pos.push_back(e << 23);
    for (uint32_t k = 0; k < 23; ++k) pos.push_back(1u << k);
    pos.push_back(0x7f800000u);
    const uint32_t nans[] = {0x7fc00000u, 0x7fc00001u, 0x7fd5aaaau, 0x7fffffffu, 0x7f800001u, 0x7f8abcdeu, 0x7fa00000u, 0x7fbfffffu};
    for (uint32_t v : nans) pos.push_back(v);
    std::vector<uint32_t> all(pos);
    for (uint32_t p : pos) all.push_back(p | 0x80000000u);
    uint32_t s = 20u;
    for (int i = 0; i < 1024; ++i) {
        s = s * 1664525u + 1013904223u;
        all.push_back(s ^ (s >> 15));
    }
    return all;
}

} // namespace

int main()
{
    const float expo[] = {0.68f + 0.1f, 1.5f, 0.35f, 0.15f, 0.33f, 40.0f};
    const int every[] = {0, 1, 2, 3, 4, 5, 6, 7};
    for (int fn : every) quick(fn, 0.0f, 0xffffffffu, kAll);
    quick(17, 0.0f, 0xffffffffu, kFiniteNonneg);
    quick(18, 0.0f, 0xffffffffu, kNoNan);
    quick(19, 0.0f, 0xffffffffu, kNoNan);
    quick(20, 0.0f, 0xffffffffu, kFinite);
    quick(21, 0.0f, 0xffffffffu, kFinite);
    for (float y : expo) {
        quick(8, y, 0xffffffffu, kAll);
        quick(11, y, 0x7fffffffu, kFiniteNonneg);
        quick(13, y, 0x7fffffffu, kFiniteNonneg);
    }
    const std::vector<uint32_t> e = edges();
    std::vector<uint32_t> a, b;
    for (uint32_t x : e)
        for (uint32_t y : e) {
            a.push_back(x);
            b.push_back(y);
        }
    for (int fn = 8; fn <= 10; ++fn) {
        uint32_t first[4 * kFirst];
        const int64_t bad = ps_pairs(fn, a.data(), b.data(), a.size(), first);
        if (bad) {
            ++failures;
            printf("pairs fn %d: %lld mismatches, first a 0x%08x b 0x%08x got 0x%08x want 0x%08x\n", fn, (long long)bad,
                   first[0], first[1], first[2], first[3]);
        }
    }
    if (failures) return 1;
    printf("prim_check ok: %zu edge values, %zu pairs\n", e.size(), a.size());
    return 0;
}
