// Stand-alone check of gpgpuraytrace_amd/csrc/rt_rayquery.h (the host-only part of rt_terrain_trace_rays):
// option parsing through the size field, the count limits, the shape / lanes-per-ray / grid plan, the ray
// packing.  Built with -fsanitize=address,undefined by tests/test_ray_query_host.py; its own main.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_rayquery.h"

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            std::printf("rayquery_check FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                    \
        }                                                                \
    } while (0)

struct OptV1 {
    uint32_t size, flags;
    float eye[3];
    uint32_t max_blocks;
};

int main()
{
    using namespace rtq;
    const char* why = "";
    Options o;
    static_assert(sizeof(OptV1) == kOptSizeV1, "the first version of rt_ray_options");

    // options: null, too short (read no further than the size field), exact, a later (longer) version
    CHECK(parse_options(nullptr, &o, &why) == OK && o.flags == 0 && o.max_blocks == 0);
    {
        std::vector<unsigned char> tiny(4); // only the size field exists: ASan faults a read past it
        uint32_t sz = 8;
        std::memcpy(tiny.data(), &sz, 4);
        CHECK(parse_options(tiny.data(), &o, &why) == INVALID);
        sz = 0;
        std::memcpy(tiny.data(), &sz, 4);
        CHECK(parse_options(tiny.data(), &o, &why) == INVALID);
        sz = kOptSizeV1 - 1;
        std::memcpy(tiny.data(), &sz, 4);
        CHECK(parse_options(tiny.data(), &o, &why) == INVALID);
    }
    {
        OptV1 v = {sizeof(OptV1), kEye | kForceLanes, {1.5f, -2.0f, 3.25f}, 7};
        std::vector<unsigned char> exact(sizeof v); // heap, exactly the struct: no read past its end
        std::memcpy(exact.data(), &v, sizeof v);
        CHECK(parse_options(exact.data(), &o, &why) == OK);
        CHECK(o.flags == (kEye | kForceLanes) && o.eye[0] == 1.5f && o.eye[1] == -2.0f && o.eye[2] == 3.25f);
        CHECK(o.max_blocks == 7);
        v.size = 64; // a later version: its first fields mean the same
        std::vector<unsigned char> later(64, 0xee);
        std::memcpy(later.data(), &v, sizeof v);
        CHECK(parse_options(later.data(), &o, &why) == OK && o.max_blocks == 7);
        v.size = sizeof(OptV1);
        v.flags = kForceSegments | kForceLanes;
        CHECK(parse_options(&v, &o, &why) == INVALID);
    }

    // counts
    CHECK(check_count(0, &why) == OK && check_count(1, &why) == OK && check_count(kMaxRays, &why) == OK);
    CHECK(check_count(-1, &why) == INVALID && check_count(kMaxRays + 1, &why) == INVALID);
    CHECK(check_count(-2147483647 - 1, &why) == INVALID && check_count(2147483647, &why) == INVALID);

    // plans
    Plan p;
    const int BS1 = 256, LPR1 = 16;
    CHECK(plan(100, false, kForceSegments, 0, 256, BS1, LPR1, &p, &why) == UNSUPPORTED);
    CHECK(plan(100, false, 0, 0, 256, BS1, LPR1, &p, &why) == OK && p.shape == LANES && p.blocks == 1);
    CHECK(plan(100, true, 0, 0, 256, BS1, LPR1, &p, &why) == OK && p.shape == SEGMENTS);
    CHECK(p.bs == BS1 && p.lpr == LPR1 && p.blocks == 7); // 16 rays a block
    CHECK(plan(kAutoSegmentsMax, true, 0, 0, 256, BS1, LPR1, &p, &why) == OK && p.shape == SEGMENTS);
    CHECK(plan(kAutoSegmentsMax + 1, true, 0, 0, 256, BS1, LPR1, &p, &why) == OK && p.shape == LANES);
    const struct {
        int n, bs, lpr;
    } ladder[] = {{1, BS1, LPR1}, {2048, BS1, LPR1}, {2049, 512, 32}, {4096, 512, 32}, {4097, 512, 8},
                  {16384, 512, 8}, {16385, 512, 4}, {kMaxRays, 512, 4}};
    for (const auto& l : ladder) {
        CHECK(plan(l.n, true, kForceSegments, 0, 256, BS1, LPR1, &p, &why) == OK && p.shape == SEGMENTS);
        CHECK(p.bs == l.bs && p.lpr == l.lpr);
        const uint64_t per = (uint64_t)(p.bs / p.lpr); // every ray has a segment, and no block is empty
        CHECK((uint64_t)p.blocks * per >= (uint64_t)l.n && ((uint64_t)p.blocks - 1) * per < (uint64_t)l.n);
    }
    for (int n : {1, 63, 64, 65, 1024, 1025, 4133, 1 << 20, kMaxRays}) {
        CHECK(plan(n, true, kForceLanes, 0, 256, BS1, LPR1, &p, &why) == OK && p.shape == LANES);
        CHECK(p.bs == 1024 && p.lpr == 1 && p.blocks >= 1 && p.blocks <= 256);
        CHECK(p.blocks == 256 || (uint64_t)p.blocks * 1024 >= (uint64_t)n); // fewer blocks only when they cover n
        CHECK(plan(n, true, kForceLanes, 2, 256, BS1, LPR1, &p, &why) == OK && p.blocks <= 2 && p.blocks >= 1);
        CHECK(plan(n, true, kForceLanes, 1000, 250, BS1, LPR1, &p, &why) == OK && p.blocks <= 250);
        CHECK(plan(n, true, kForceLanes, 0, 0, BS1, LPR1, &p, &why) == OK && p.blocks == 1); // every CU reserved
    }

    // packing
    {
        const int n = 3;
        std::vector<float> org(3 * n), dir(3 * n), out(8 * n, -1.0f);
        for (int i = 0; i < 3 * n; ++i) {
            org[i] = (float)i;
            dir[i] = 100.0f + (float)i;
        }
        pack(org.data(), dir.data(), n, out.data());
        for (int i = 0; i < n; ++i) {
            for (int a = 0; a < 3; ++a) CHECK(out[8 * i + a] == org[3 * i + a] && out[8 * i + 4 + a] == dir[3 * i + a]);
            CHECK(out[8 * i + 3] == 0.0f && out[8 * i + 7] == 0.0f);
        }
        pack(org.data(), dir.data(), 0, nullptr); // nothing touched
    }
    std::printf("rayquery_check ok\n");
    return 0;
}
