// Stand-alone check of the field queries' part of gpgpuraytrace_amd/csrc/rt_rayquery.h (the host-only part of
// rt_terrain_sample_field / rt_terrain_sample_lattice): the option parser (never read past the caller's size,
// unknown flags refused), the lattice's validation, the two plans (grid, rows per strip, column reuse), the strip
// count, which must cover every lattice point exactly once, and the point packing.
// Built with -fsanitize=address,undefined by tests/test_field_query_host.py; its own main.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "rt_rayquery.h"

#define CHECK(x)                                                           \
    do {                                                                   \
        if (!(x)) {                                                        \
            std::printf("fieldquery_check FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

struct FieldV1 {
    uint32_t size, flags;
    float eye[3];
    uint32_t max_blocks;
};
struct LatticeV1 {
    float origin[3], spacing[3];
    uint32_t dims[3];
};
static_assert(sizeof(FieldV1) == 24 && sizeof(LatticeV1) == 36 && sizeof(rtq::Lattice) == 36, "the C-ABI's sizes");

int main()
{
    using namespace rtq;
    const char* why = "";
    FieldOptions o;

    // the option block, on the heap at its exact size
    CHECK(parse_field_options(nullptr, &o, &why) == OK && o.flags == 0 && o.max_blocks == 0);
    {
        FieldV1 v = {sizeof(FieldV1), kEye | kFieldNormal, {1.5f, -2.0f, 3.25f}, 7};
        std::vector<unsigned char> buf(sizeof v);
        std::memcpy(buf.data(), &v, sizeof v);
        CHECK(parse_field_options(buf.data(), &o, &why) == OK);
        CHECK(o.flags == (kEye | kFieldNormal) && o.eye[0] == 1.5f && o.eye[1] == -2.0f && o.eye[2] == 3.25f && o.max_blocks == 7);
        for (uint32_t size : {0u, 4u, 8u, 23u}) { // too short: only the size word is read
            std::vector<unsigned char> small(4);
            std::memcpy(small.data(), &size, 4);
            why = "";
            CHECK(parse_field_options(small.data(), &o, &why) == INVALID && why[0] != 0);
        }
        v.size = 64; // a later, longer version: the first fields mean the same (the buffer stays 24 bytes)
        std::memcpy(buf.data(), &v, sizeof v);
        CHECK(parse_field_options(buf.data(), &o, &why) == OK && o.max_blocks == 7);
        for (uint32_t bad : {2u, 4u, 8u, 16u, 64u, 0x80000000u, kForceLanes | kFieldNormal}) {
            v.flags = bad;
            std::memcpy(buf.data(), &v, sizeof v);
            why = "";
            CHECK(parse_field_options(buf.data(), &o, &why) == INVALID && why[0] != 0);
        }
        for (uint32_t good : {0u, kEye, kFieldNormal, kEye | kFieldNormal}) {
            v.flags = good;
            std::memcpy(buf.data(), &v, sizeof v);
            CHECK(parse_field_options(buf.data(), &o, &why) == OK && o.flags == good);
        }
    }

    // the lattice
    {
        Lattice l;
        uint32_t n = 99;
        CHECK(check_lattice(nullptr, &l, &n, &why) == INVALID);
        auto check = [&](LatticeV1 v, uint32_t* out_n) {
            std::vector<unsigned char> buf(sizeof v);
            std::memcpy(buf.data(), &v, sizeof v);
            return check_lattice(buf.data(), &l, out_n, &why);
        };
        CHECK(check({{0.7f, 1, 2}, {2.3f, -1.0f, 0.0f}, {33, 5, 3}}, &n) == OK && n == 33 * 5 * 3);
        CHECK(l.origin[0] == 0.7f && l.spacing[1] == -1.0f && l.dims[2] == 3);
        CHECK(check({{0, 0, 0}, {1, 1, 1}, {0, 5, 3}}, &n) == OK && n == 0);
        CHECK(check({{0, 0, 0}, {1, 1, 1}, {5, 5, 0}}, &n) == OK && n == 0);
        CHECK(check({{0, 0, 0}, {1, 1, 1}, {4096, 4096, 4}}, &n) == OK && n == (1u << 26));
        CHECK(check({{0, 0, 0}, {1, 1, 1}, {4096, 4096, 5}}, &n) == INVALID);
        CHECK(check({{0, 0, 0}, {1, 1, 1}, {4096, 4096, 4096}}, &n) == INVALID); // (2^36: no 32-bit product)
        CHECK(check({{0, 0, 0}, {1, 1, 1}, {4097, 1, 1}}, &n) == INVALID);
        CHECK(check({{0, 0, 0}, {1, 1, 1}, {1, 1, 0xffffffffu}}, &n) == INVALID);
        CHECK(check({{0, 0, 0}, {1, 1, 1}, {0, 4097, 1}}, &n) == INVALID); // a dim above the bound, whatever the product
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        for (float bad : {inf, -inf, nan})
            for (int i = 0; i < 6; ++i) {
                LatticeV1 v = {{0, 0, 0}, {1, 1, 1}, {2, 2, 2}};
                (i < 3 ? v.origin[i] : v.spacing[i - 3]) = bad;
                why = "";
                CHECK(check(v, &n) == INVALID && why[0] != 0);
            }
    }

    // the points plan: min(ceil(n / 1024), cus, max_blocks), at least one block
    const int cus = 248;
    for (uint32_t n : {1u, 63u, 64u, 65u, 1023u, 1024u, 1025u, 4133u, 65536u, 1u << 20, (uint32_t)kMaxRays}) {
        const uint32_t need = (n + 1023u) / 1024u;
        FieldPlan p = plan_field_points(n, 0, cus);
        CHECK(p.blocks == (need < (uint32_t)cus ? need : (uint32_t)cus) && p.blocks >= 1);
        for (uint32_t mb : {1u, 2u, 7u, 248u, 1000u}) {
            uint32_t want = need < (uint32_t)cus ? need : (uint32_t)cus;
            if (mb < want) want = mb;
            CHECK(plan_field_points(n, mb, cus).blocks == want);
        }
        CHECK(plan_field_points(n, 0, 0).blocks == 1 && plan_field_points(n, 0, -3).blocks == 1);
    }

    // the lattice plan: rows min(kFieldRows, ny), the column reuse on nomadplains with >= 2 rows, and the strips
    // walked the way the kernel walks them cover every point once
    const uint32_t shapes[][3] = {{1, 1, 1},  {33, 5, 3},   {64, 4, 4},    {70, 3, 2},    {97, 1, 1},     {48, 24, 40},
                                  {65, 9, 2}, {4096, 1, 1}, {1, 4096, 16}, {1, 1, 4096},  {256, 128, 256}, {4096, 4096, 4}};
    for (const auto& d : shapes)
        for (int nomad = 0; nomad < 2; ++nomad) {
            const FieldPlan p = plan_field_lattice(d, nomad != 0, 0, cus);
            CHECK(p.rows >= 1 && p.rows == (d[1] < kFieldRows ? d[1] : kFieldRows));
            CHECK(p.column == (nomad && p.rows > 1));
            const uint32_t strips = lattice_strips(d, p.rows);
            const uint32_t need = (strips + kFieldWaves - 1u) / kFieldWaves;
            CHECK(p.blocks >= 1 && p.blocks == (need < (uint32_t)cus ? need : (uint32_t)cus));
            CHECK(plan_field_lattice(d, nomad != 0, 1, cus).blocks == 1);
            CHECK(plan_field_lattice(d, nomad != 0, 0, 0).blocks == 1);
            const uint64_t total = (uint64_t)d[0] * d[1] * d[2];
            if (total > (1u << 22)) continue;
            std::vector<unsigned char> seen(total, 0);
            const uint32_t xc = (d[0] + 63u) / 64u, yc = (d[1] + p.rows - 1u) / p.rows;
            CHECK(strips == xc * yc * d[2]);
            for (uint32_t s = 0; s < strips; ++s) {
                const uint32_t cx = s % xc, r = s / xc, cy = r % yc, iz = r / yc;
                const uint32_t iy0 = cy * p.rows, iy1 = iy0 + p.rows < d[1] ? iy0 + p.rows : d[1];
                CHECK(iz < d[2]);
                for (uint32_t iy = iy0; iy < iy1; ++iy)
                    for (uint32_t lane = 0; lane < 64; ++lane) {
                        const uint32_t ix = cx * 64u + lane;
                        if (ix >= d[0]) continue;
                        const uint64_t i = ((uint64_t)iz * d[1] + iy) * d[0] + ix;
                        CHECK(i < total && !seen[i]);
                        seen[i] = 1;
                    }
            }
            for (unsigned char v : seen) CHECK(v == 1);
        }

    // the point packing: x y z 0, nothing read or written past the arrays
    {
        std::vector<float> pts = {1, 2, 3, 4, 5, 6, 7, 8, 9};
        std::vector<float> packed(12, -1.0f);
        pack_points(pts.data(), 3, packed.data());
        const float want[12] = {1, 2, 3, 0, 4, 5, 6, 0, 7, 8, 9, 0};
        for (int i = 0; i < 12; ++i) CHECK(packed[i] == want[i]);
        pack_points(pts.data(), 0, packed.data());
    }
    std::printf("fieldquery_check ok\n");
    return 0;
}
