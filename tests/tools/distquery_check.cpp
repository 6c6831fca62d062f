// Stand-alone check of the distance fields' part of gpgpuraytrace_amd/csrc/rt_rayquery.h (the host-only part of
// rt_terrain_distance_field): the option parser (never read past the caller's size, unknown flags refused), what
// max_cells becomes, the isotropy rule, the scratch layout, the grid plan, and the x pass's row arithmetic against a
// bit-by-bit loop over the row: random, all-set and all-clear rows, with garbage in the padding bits.
// Built with -fsanitize=address,undefined by tests/test_distance_host.py; its own main.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_rayquery.h"

#define CHECK(x)                                                           \
    do {                                                                   \
        if (!(x)) {                                                        \
            std::printf("distquery_check FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

struct DistanceV1 {
    uint32_t size, flags;
    float eye[3];
    uint32_t max_blocks, max_cells;
};
static_assert(sizeof(DistanceV1) == 28, "the C-ABI's size");

static uint32_t g_seed = 12345u;
static uint32_t rnd()
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return g_seed ^ (g_seed >> 15);
}

// the definition, bit by bit: the distance from ix to the nearest point of the row whose bit equals `want`
static uint32_t slow_row(const std::vector<uint32_t>& row, uint32_t nx, uint32_t ix, uint32_t want)
{
    uint32_t best = rtq::kDistRowFar;
    for (uint32_t k = 0; k < nx; ++k)
        if (((row[k / 32u] >> (k % 32u)) & 1u) == want) {
            const uint32_t d = k > ix ? k - ix : ix - k;
            if (d < best) best = d;
        }
    return best;
}

static int check_row(const std::vector<uint32_t>& row, uint32_t nx)
{
    const uint32_t words = (nx + 31u) / 32u;
    // the row on the heap at its exact size: a word read past it is the sanitizer's
    std::vector<uint32_t> exact(row.begin(), row.begin() + words);
    for (uint32_t w = 0; w < words; ++w) {
        uint16_t in[32], out[32];
        for (int b = 0; b < 32; ++b) in[b] = out[b] = 0x1234;
        rtq::dist_row(exact.data(), nx, w, in, out);
        const rtq::DistRowWord r = rtq::dist_row_word(exact.data(), nx, w);
        CHECK((r.bits[0] & r.bits[1]) == 0u && (r.bits[0] | r.bits[1]) == rtq::dist_valid_bits(nx, w));
        for (uint32_t b = 0; b < 32u; ++b) {
            const uint32_t ix = 32u * w + b;
            if (ix >= nx) {
                CHECK(in[b] == 0x1234 && out[b] == 0x1234); // beyond the row: left alone
                continue;
            }
            CHECK(in[b] == slow_row(exact, nx, ix, 1u));
            CHECK(out[b] == slow_row(exact, nx, ix, 0u));
            CHECK(rtq::dist_row_pack(r, b) == ((uint32_t)in[b] | ((uint32_t)out[b] << 16)));
            CHECK((in[b] == 0) != (out[b] == 0)); // the point is in exactly one set
        }
    }
    return 0;
}

int main()
{
    using namespace rtq;
    const char* why = "";
    DistanceOptions o;

    // the option block, on the heap at its exact size
    CHECK(parse_distance_options(nullptr, &o, &why) == OK && o.flags == 0 && o.max_blocks == 0 && o.max_cells == 0);
    {
        DistanceV1 v = {sizeof(DistanceV1), kEye, {1.5f, -2.0f, 3.25f}, 7, 9};
        std::vector<unsigned char> buf(sizeof v);
        std::memcpy(buf.data(), &v, sizeof v);
        CHECK(parse_distance_options(buf.data(), &o, &why) == OK);
        CHECK(o.flags == kEye && o.eye[0] == 1.5f && o.eye[1] == -2.0f && o.eye[2] == 3.25f && o.max_blocks == 7 &&
              o.max_cells == 9);
        for (uint32_t size : {0u, 4u, 8u, 24u, 27u}) { // too short: only the size word is read
            std::vector<unsigned char> small(4);
            std::memcpy(small.data(), &size, 4);
            why = "";
            CHECK(parse_distance_options(small.data(), &o, &why) == INVALID && why[0] != 0);
        }
        v.size = 64; // a later, longer version: the first fields mean the same (the buffer stays 28 bytes)
        std::memcpy(buf.data(), &v, sizeof v);
        CHECK(parse_distance_options(buf.data(), &o, &why) == OK && o.max_blocks == 7 && o.max_cells == 9);
        for (uint32_t bad : {2u, 4u, 8u, 16u, 32u, 64u, 0x80000000u, kEye | kFieldNormal}) {
            v.flags = bad;
            std::memcpy(buf.data(), &v, sizeof v);
            why = "";
            CHECK(parse_distance_options(buf.data(), &o, &why) == INVALID && why[0] != 0);
        }
        for (uint32_t good : {0u, kEye}) {
            v.flags = good;
            v.max_cells = 0xffffffffu;
            std::memcpy(buf.data(), &v, sizeof v);
            CHECK(parse_distance_options(buf.data(), &o, &why) == OK && o.flags == good && o.max_cells == 0xffffffffu);
        }
    }

    // max_cells: the reach of a scan and the largest finite d2; from 7093 on it bounds nothing (3 * 4095^2 < 7093^2)
    {
        const uint64_t largest = 3ull * 4095ull * 4095ull;
        CHECK(largest < (uint64_t)kDistMaxCells * kDistMaxCells && largest >= (uint64_t)(kDistMaxCells - 1u) * (kDistMaxCells - 1u));
        CHECK(largest < (1ull << 26));
        for (uint32_t r : {0u, kDistMaxCells, kDistMaxCells + 1u, 65536u, 0xffffffffu}) {
            const DistanceBound b = distance_bound(r);
            CHECK(b.reach >= kMaxLatticeDim - 1u && b.limit2 >= largest && b.limit2 < kDistFar);
        }
        for (uint32_t r : {1u, 2u, 3u, 8u, 4095u, 5000u, kDistMaxCells - 1u}) {
            const DistanceBound b = distance_bound(r);
            CHECK(b.reach == r && b.limit2 == r * r && (uint64_t)b.limit2 == (uint64_t)r * r);
        }
    }

    // distance wants |spacing| equal on the three axes and not 0
    {
        const float iso[][3] = {{1, 1, 1}, {2.5f, 2.5f, 2.5f}, {-2.5f, 2.5f, -2.5f}, {-0.1f, -0.1f, -0.1f}};
        for (const auto& s : iso) CHECK(distance_isotropic(s));
        const float not_iso[][3] = {{0, 0, 0}, {-0.0f, 0.0f, 0.0f}, {1, 1, 2}, {1, 2, 1}, {2, 1, 1}, {1, 1, 0}, {2.3f, 4.1f, 2.3f}};
        for (const auto& s : not_iso) CHECK(!distance_isotropic(s));
    }

    // the scratch layout: occupancy words, a word a point, two words a point, each part from a multiple of 16
    {
        const uint32_t shapes[][3] = {{1, 1, 1}, {33, 5, 3}, {70, 9, 8}, {97, 1, 1}, {3, 300, 2}, {256, 64, 256}, {4096, 4096, 4}};
        for (const auto& d : shapes) {
            const DistanceScratch s = distance_scratch(d);
            const size_t n = (size_t)d[0] * d[1] * d[2], occ = (size_t)((d[0] + 31) / 32) * d[1] * d[2] * 4;
            auto up = [](size_t b) { return (b + 15) / 16 * 16; };
            CHECK(s.points == n);
            CHECK(s.lay.offset[DIST_OCCUPANCY] == 0 && s.lay.offset[DIST_ROWS] == up(occ));
            CHECK(s.lay.offset[DIST_PLANES] == up(occ) + up(4 * n) && s.lay.total == up(occ) + up(4 * n) + up(8 * n));
        }
        const uint32_t empty[][3] = {{0, 2, 2}, {2, 0, 2}, {2, 2, 0}};
        for (const auto& d : empty) CHECK(distance_scratch(d).points == 0 && distance_scratch(d).lay.total == 0);
    }

    // the plan: min(ceil(points / 256), 8 cus, max_blocks), at least one block; the tiles a block strides over cover
    // every point once
    {
        const int cus = 248;
        for (uint32_t n : {1u, 255u, 256u, 257u, 495u, 1800u, 46080u, 1u << 22, (uint32_t)kMaxRays}) {
            const uint32_t need = (n + kDistThreads - 1u) / kDistThreads, cap = 8u * cus;
            CHECK(plan_distance(n, 0, cus).blocks == (need < cap ? need : cap));
            for (uint32_t mb : {1u, 2u, 7u, 5000u}) {
                uint32_t want = need < cap ? need : cap;
                if (mb < want) want = mb;
                CHECK(plan_distance(n, mb, cus).blocks == want && want >= 1u);
            }
            CHECK(plan_distance(n, 0, 0).blocks == (need < 8u ? need : 8u) && plan_distance(n, 0, -3).blocks >= 1u);
            if (n > (1u << 22)) continue;
            for (uint32_t mb : {1u, 2u, 0u}) {
                const uint32_t blocks = plan_distance(n, mb, cus).blocks;
                std::vector<unsigned char> seen(n, 0);
                for (uint32_t b = 0; b < blocks; ++b)
                    for (uint32_t t = 0; t < kDistThreads; ++t)
                        for (uint32_t i = b * kDistThreads + t; i < n; i += blocks * kDistThreads) {
                            CHECK(!seen[i]);
                            seen[i] = 1;
                        }
                for (unsigned char v : seen) CHECK(v == 1);
            }
        }
    }

    // the row arithmetic
    for (uint32_t nx : {1u, 31u, 32u, 33u, 63u, 64u, 65u, 97u, 130u}) {
        const uint32_t words = (nx + 31u) / 32u, pad = words * 32u - nx;
        const uint32_t pad_mask = pad ? ~(0xffffffffu >> pad) : 0u;
        std::vector<uint32_t> row(words);
        for (int fill = 0; fill < 2; ++fill)         // all clear, all set
            for (int garbage = 0; garbage < 3; ++garbage) { // padding 0, 1, random
                for (uint32_t& w : row) w = fill ? 0xffffffffu : 0u;
                row[words - 1u] = (row[words - 1u] & ~pad_mask) | ((garbage == 0 ? 0u : garbage == 1 ? 0xffffffffu : rnd()) & pad_mask);
                if (check_row(row, nx)) return 1;
            }
        for (int trial = 0; trial < 200; ++trial) {
            // dense, sparse, nearly full, and single points
            const int kind = trial % 4;
            for (uint32_t& w : row) {
                const uint32_t a = rnd(), b = rnd(), c = rnd();
                w = kind == 0 ? a : kind == 1 ? (a & b & c) : kind == 2 ? (a | b | c) : 0u;
            }
            if (kind == 3) row[(rnd() % nx) / 32u] |= 1u << (rnd() % 32u);
            row[words - 1u] = (row[words - 1u] & ~pad_mask) | (rnd() & pad_mask); // garbage in the padding
            if (check_row(row, nx)) return 1;
            // the padding never matters: the same row with the padding flipped gives the same words
            std::vector<uint32_t> flipped = row;
            flipped[words - 1u] ^= pad_mask;
            for (uint32_t w = 0; w < words; ++w) {
                const DistRowWord x = dist_row_word(row.data(), nx, w), y = dist_row_word(flipped.data(), nx, w);
                CHECK(std::memcmp(&x, &y, sizeof x) == 0);
            }
        }
    }
    std::printf("distquery_check ok\n");
    return 0;
}
