// Stand-alone check of the surface queries' part of gpgpuraytrace_amd/csrc/rt_rayquery.h (the host-only part of
// rt_terrain_trace_surface): the option block parsed through its size field, every validation case, both
// shapes' plans, the range packing.  Built with -fsanitize=address,undefined by
// tests/test_surface_query_host.py; its own main.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "rt_rayquery.h"

#define CHECK(x)                                                          \
    do {                                                                  \
        if (!(x)) {                                                       \
            std::printf("surfquery_check FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

struct SurfV1 {
    uint32_t size, flags;
    float eye[3];
    uint32_t max_blocks;
    float t_min, t_max, stepmod;
    uint32_t max_steps;
};

// the block on the heap at exactly `bytes` bytes, so that ASan faults any read past the caller's size
static int parse_exact(const SurfV1& v, size_t bytes, rtq::SurfOptions* o, const char** why)
{
    std::vector<unsigned char> buf(bytes, 0xee);
    std::memcpy(buf.data(), &v, bytes < sizeof v ? bytes : sizeof v);
    return rtq::parse_surface_options(buf.data(), o, why);
}

int main()
{
    using namespace rtq;
    const char* why = "";
    SurfOptions o;
    static_assert(sizeof(SurfV1) == kSurfOptSizeV1, "the first version of rt_surface_options");
    static_assert(kSurfParams == 8u && kSurfRayRange == 16u, "RT_SURFACE_*");
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

    // null: the defaults
    CHECK(parse_surface_options(nullptr, &o, &why) == OK && o.flags == 0 && o.max_blocks == 0);
    CHECK(o.t_min == 0.01f && o.t_max == 5000.0f && o.stepmod == 1.0f && o.max_steps == 0);

    // sizes: too short (only the size field exists), 39, 40, above 40
    {
        std::vector<unsigned char> tiny(4);
        for (uint32_t sz : {0u, 8u, 24u, 39u}) {
            std::memcpy(tiny.data(), &sz, 4);
            CHECK(parse_surface_options(tiny.data(), &o, &why) == INVALID);
        }
    }
    SurfV1 v = {sizeof(SurfV1), kEye | kForceLanes | kSurfParams | kSurfRayRange, {1.5f, -2.0f, 3.25f}, 7, 0.5f, 100.0f, 2.0f, 64};
    CHECK(parse_exact(v, 40, &o, &why) == OK);
    CHECK(o.flags == v.flags && o.eye[0] == 1.5f && o.eye[1] == -2.0f && o.eye[2] == 3.25f && o.max_blocks == 7);
    CHECK(o.t_min == 0.5f && o.t_max == 100.0f && o.stepmod == 2.0f && o.max_steps == 64);
    v.size = 39;
    CHECK(parse_exact(v, 39, &o, &why) == INVALID);
    v.size = 64; // a later version: its first fields mean the same
    CHECK(parse_exact(v, 64, &o, &why) == OK && o.max_steps == 64 && o.t_max == 100.0f);
    v.size = 40;

    // the trailing fields are read with RT_SURFACE_PARAMS only: garbage there is ignored without it
    {
        SurfV1 g = v;
        g.flags = kForceSegments;
        g.t_min = nan;
        g.t_max = -inf;
        g.stepmod = -1.0f;
        g.max_steps = 0xffffffffu;
        CHECK(parse_exact(g, 40, &o, &why) == OK && o.flags == kForceSegments);
        CHECK(o.t_min == 0.01f && o.t_max == 5000.0f && o.stepmod == 1.0f && o.max_steps == 0);
    }

    // validation
    {
        SurfV1 b = v;
        b.flags = kForceSegments | kForceLanes;
        CHECK(parse_exact(b, 40, &o, &why) == INVALID);
        for (float sm : {0.0f, -0.0f, -1.0f, inf, -inf, nan}) {
            b = v;
            b.stepmod = sm;
            CHECK(parse_exact(b, 40, &o, &why) == INVALID);
        }
        b = v;
        b.stepmod = 1e-30f;
        CHECK(parse_exact(b, 40, &o, &why) == OK);
        b = v;
        b.t_min = 10.0f;
        b.t_max = 9.0f;
        CHECK(parse_exact(b, 40, &o, &why) == INVALID);
        b.t_max = 10.0f; // an empty range is a range
        CHECK(parse_exact(b, 40, &o, &why) == OK);
        b.t_max = nan;
        CHECK(parse_exact(b, 40, &o, &why) == INVALID);
        b = v;
        b.t_min = nan;
        CHECK(parse_exact(b, 40, &o, &why) == INVALID);
        b = v;
        b.max_steps = 0xffffffffu;
        CHECK(parse_exact(b, 40, &o, &why) == OK && o.max_steps == 0xffffffffu);
    }
    CHECK(surface_max_steps(0) == 0 && surface_max_steps(64) == 64 && surface_max_steps(0x7fffffffu) == 0x7fffffff);
    CHECK(surface_max_steps(0x80000000u) == 0x7fffffff && surface_max_steps(0xffffffffu) == 0x7fffffff);

    // plans: both shapes
    Plan p;
    const int BS1 = 256, LPR1 = 16;
    CHECK(plan_surface(100, false, kForceSegments, 0, 256, BS1, LPR1, &p, &why) == UNSUPPORTED);
    CHECK(plan_surface(100, false, kSurfParams | kSurfRayRange | kEye, 0, 256, BS1, LPR1, &p, &why) == OK);
    CHECK(p.shape == LANES && p.blocks == 1 && p.bs == 1024 && p.lpr == 1);
    CHECK(plan_surface(1, true, 0, 0, 256, BS1, LPR1, &p, &why) == OK && p.shape == SEGMENTS);
    CHECK(p.bs == BS1 && p.lpr == LPR1 && p.blocks == 1); // one pick: one segment
    CHECK(plan_surface(kSurfAutoSegmentsMax, true, kSurfParams, 0, 256, BS1, LPR1, &p, &why) == OK && p.shape == SEGMENTS);
    CHECK(plan_surface(kSurfAutoSegmentsMax + 1, true, kSurfRayRange, 0, 256, BS1, LPR1, &p, &why) == OK && p.shape == LANES);
    CHECK(plan_surface(kSurfAutoSegmentsMax + 1, false, 0, 0, 256, BS1, LPR1, &p, &why) == OK && p.shape == LANES);
    const struct {
        int n, bs, lpr;
    } ladder[] = {{1, BS1, LPR1}, {2048, BS1, LPR1}, {2049, 512, 32}, {4096, 512, 32}, {4097, 512, 8},
                  {16384, 512, 8}, {16385, 512, 4}, {kMaxRays, 512, 4}};
    for (const auto& l : ladder) {
        CHECK(plan_surface(l.n, true, kForceSegments | kSurfParams, 0, 256, BS1, LPR1, &p, &why) == OK && p.shape == SEGMENTS);
        CHECK(p.bs == l.bs && p.lpr == l.lpr);
        const uint64_t per = (uint64_t)(p.bs / p.lpr);
        CHECK((uint64_t)p.blocks * per >= (uint64_t)l.n && ((uint64_t)p.blocks - 1) * per < (uint64_t)l.n);
    }
    for (int n : {1, 63, 64, 65, 1024, 1025, 4133, 1 << 20, kMaxRays}) {
        CHECK(plan_surface(n, true, kForceLanes, 0, 256, BS1, LPR1, &p, &why) == OK && p.shape == LANES);
        CHECK(p.bs == 1024 && p.lpr == 1 && p.blocks >= 1 && p.blocks <= 256);
        CHECK(p.blocks == 256 || (uint64_t)p.blocks * 1024 >= (uint64_t)n);
        CHECK(plan_surface(n, true, kForceLanes, 2, 256, BS1, LPR1, &p, &why) == OK && p.blocks <= 2 && p.blocks >= 1);
        CHECK(plan_surface(n, true, kForceLanes, 0, 0, BS1, LPR1, &p, &why) == OK && p.blocks == 1);
    }

    // packing: the ranges fill words 3 and 7 and nothing else
    {
        const int n = 3;
        std::vector<float> org(3 * n), dir(3 * n), rng(2 * n), out(8 * n, -1.0f);
        for (int i = 0; i < 3 * n; ++i) {
            org[i] = (float)i;
            dir[i] = 100.0f + (float)i;
        }
        for (int i = 0; i < 2 * n; ++i) rng[i] = 1000.0f + (float)i;
        pack(org.data(), dir.data(), n, out.data());
        pack_ranges(rng.data(), n, out.data());
        for (int i = 0; i < n; ++i) {
            for (int a = 0; a < 3; ++a) CHECK(out[8 * i + a] == org[3 * i + a] && out[8 * i + 4 + a] == dir[3 * i + a]);
            CHECK(out[8 * i + 3] == rng[2 * i] && out[8 * i + 7] == rng[2 * i + 1]);
        }
        pack_ranges(rng.data(), 0, nullptr); // nothing touched
    }
    std::printf("surfquery_check ok\n");
    return 0;
}
