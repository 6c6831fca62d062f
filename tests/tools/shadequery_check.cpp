// Stand-alone check of the shaded queries' part of gpgpuraytrace_amd/csrc/rt_rayquery.h (the host-only part of
// rt_terrain_shade_rays): plan_shade -- always the lanes shape, its grid min(ceil(n / 1024), CUs, max_blocks),
// forced segments refused -- behind the surface queries' option parser, which the shaded queries reuse unchanged.
// Built with -fsanitize=address,undefined by tests/test_shade_query_host.py; its own main.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_rayquery.h"

#define CHECK(x)                                                           \
    do {                                                                   \
        if (!(x)) {                                                        \
            std::printf("shadequery_check FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

struct SurfV1 {
    uint32_t size, flags;
    float eye[3];
    uint32_t max_blocks;
    float t_min, t_max, stepmod;
    uint32_t max_steps;
};

int main()
{
    using namespace rtq;
    const char* why = "";
    Plan p;

    // the shape is the lanes' whatever the flags say, but forced segments
    for (uint32_t flags : {0u, kEye, kForceLanes, kSurfParams | kSurfRayRange | kEye, kForceLanes | kSurfParams}) {
        CHECK(plan_shade(100, flags, 0, 256, &p, &why) == OK);
        CHECK(p.shape == LANES && p.bs == 1024 && p.lpr == 1 && p.blocks == 1);
    }
    why = "";
    CHECK(plan_shade(100, kForceSegments, 0, 256, &p, &why) == UNSUPPORTED && why[0] != 0);
    CHECK(plan_shade(1 << 20, kForceSegments | kSurfParams, 4, 256, &p, &why) == UNSUPPORTED);

    // the grid: min(ceil(n / 1024), cus, max_blocks)
    const int cus = 248;
    for (int n : {1, 63, 64, 65, 1023, 1024, 1025, 4096, 4133, 65536, 1 << 20, 2073600, kMaxRays}) {
        const uint32_t need = (uint32_t)(((uint64_t)n + 1023u) / 1024u);
        CHECK(plan_shade(n, 0, 0, cus, &p, &why) == OK && p.shape == LANES && p.bs == 1024 && p.lpr == 1);
        CHECK(p.blocks == (need < (uint32_t)cus ? need : (uint32_t)cus) && p.blocks >= 1);
        for (uint32_t mb : {1u, 2u, 7u, 248u, 1000u}) {
            uint32_t want = need < (uint32_t)cus ? need : (uint32_t)cus;
            if (mb < want) want = mb;
            CHECK(plan_shade(n, kForceLanes, mb, cus, &p, &why) == OK && p.blocks == want);
        }
        // no CU left after the reserved ones: still one block
        CHECK(plan_shade(n, 0, 0, 0, &p, &why) == OK && p.blocks == 1);
        CHECK(plan_shade(n, 0, 0, -3, &p, &why) == OK && p.blocks == 1);
    }

    // the option block in front of it: the surface queries' parser, the block on the heap at its exact size
    {
        SurfV1 v = {sizeof(SurfV1), kEye | kSurfParams | kSurfRayRange, {1.5f, -2.0f, 3.25f}, 2, 0.5f, 100.0f, 2.0f, 64};
        std::vector<unsigned char> buf(sizeof v);
        std::memcpy(buf.data(), &v, sizeof v);
        SurfOptions o;
        CHECK(parse_surface_options(buf.data(), &o, &why) == OK);
        CHECK(plan_shade(4133, o.flags, o.max_blocks, cus, &p, &why) == OK && p.blocks == 2);
        CHECK(surface_max_steps(o.max_steps) == 64 && o.t_min == 0.5f && o.t_max == 100.0f && o.stepmod == 2.0f);
        v.flags |= kForceSegments;
        std::memcpy(buf.data(), &v, sizeof v);
        CHECK(parse_surface_options(buf.data(), &o, &why) == OK); // (the parser takes it: the plan refuses)
        CHECK(plan_shade(4133, o.flags, o.max_blocks, cus, &p, &why) == UNSUPPORTED);
    }
    std::printf("shadequery_check ok\n");
    return 0;
}
