// Stand-alone check of the region fields' part of gpgpuraytrace_amd/csrc/rt_rayquery.h (the host-only part of
// rt_terrain_region_field): every accept and reject of the option parser (never read past the caller's size), the
// scratch layout, the plan, the backward-move tables against a literal triple loop (13 and 3 moves, which with their
// negations give all 26 and 6), and the shared region_find / region_unite -- the functions the kernels run -- single-
// threaded over random lattices in raster, reversed and shuffled link order against a flood fill, with
// label[p] <= p checked after every step (at every store, and over the whole forest on the smaller lattices).
// Built with -fsanitize=address,undefined by tests/test_region_host.py; its own main.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <tuple>
#include <utility>
#include <vector>

#include "rt_rayquery.h"

#define CHECK(x)                                                           \
    do {                                                                   \
        if (!(x)) {                                                        \
            std::printf("regionquery_check FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

struct RegionV1 {
    uint32_t size, flags;
    float eye[3];
    uint32_t max_blocks, clearance_cells, connectivity, state;
};
static_assert(sizeof(RegionV1) == 36, "the C-ABI's size");

// the definition: a flood fill from every member in raster order; the label is the fill's start
static std::vector<uint32_t> flood(const std::vector<unsigned char>& in, const uint32_t d[3], uint32_t conn)
{
    std::vector<uint32_t> lab(in.size(), rtq::kRegionNone), stack;
    for (uint32_t s = 0; s < in.size(); ++s) {
        if (!in[s] || lab[s] != rtq::kRegionNone) continue;
        lab[s] = s;
        stack.assign(1, s);
        while (!stack.empty()) {
            const uint32_t p = stack.back();
            stack.pop_back();
            const int x = (int)(p % d[0]), y = (int)(p / d[0] % d[1]), z = (int)(p / (d[0] * d[1]));
            for (int dz = -1; dz <= 1; ++dz)
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int k = std::abs(dx) + std::abs(dy) + std::abs(dz);
                        if (k == 0 || (conn == 6u && k != 1)) continue;
                        const int u = x + dx, v = y + dy, t = z + dz;
                        if (u < 0 || v < 0 || t < 0 || u >= (int)d[0] || v >= (int)d[1] || t >= (int)d[2]) continue;
                        const uint32_t q = ((uint32_t)t * d[1] + (uint32_t)v) * d[0] + (uint32_t)u;
                        if (in[q] && lab[q] == rtq::kRegionNone) {
                            lab[q] = s;
                            stack.push_back(q);
                        }
                    }
        }
    }
    return lab;
}

// the plain-array policy with every store checked: a word only falls, to a member's index that is not above its own
struct CheckedForest {
    uint32_t* w;
    const unsigned char* in;
    uint32_t faults = 0, bad = 0;
    uint32_t load(uint32_t i) { return w[i]; }
    uint32_t fall(uint32_t i, uint32_t v)
    {
        const uint32_t old = w[i];
        if (!in[i] || !in[v] || v > i || old > i) ++bad;
        if (v < old) w[i] = v;
        return old;
    }
    void fault() { ++faults; }
};

int main()
{
    using namespace rtq;
    const char* why = "";
    RegionOptions o;

    // the option block, on the heap at its exact size
    CHECK(parse_region_options(nullptr, &o, &why) == OK && o.flags == 0 && o.max_blocks == 0 && o.clearance_cells == 0 &&
          o.connectivity == 26u && o.state == 0u);
    {
        RegionV1 v = {sizeof(RegionV1), kEye, {1.5f, -2.0f, 3.25f}, 7, 9, 6, 0};
        std::vector<unsigned char> buf(sizeof v);
        auto parse = [&]() {
            std::memcpy(buf.data(), &v, sizeof v);
            why = "";
            return parse_region_options(buf.data(), &o, &why);
        };
        CHECK(parse() == OK);
        CHECK(o.flags == kEye && o.eye[0] == 1.5f && o.eye[1] == -2.0f && o.eye[2] == 3.25f && o.max_blocks == 7 &&
              o.clearance_cells == 9 && o.connectivity == 6u && o.state == 0u);
        for (uint32_t size : {0u, 4u, 8u, 24u, 28u, 35u}) { // too short: only the size word is read
            std::vector<unsigned char> small(4);
            std::memcpy(small.data(), &size, 4);
            why = "";
            CHECK(parse_region_options(small.data(), &o, &why) == INVALID && why[0] != 0);
        }
        v.size = 64; // a later, longer version: the first fields mean the same (the buffer stays 36 bytes)
        CHECK(parse() == OK && o.max_blocks == 7 && o.clearance_cells == 9 && o.connectivity == 6u);
        for (uint32_t bad : {2u, 4u, 8u, 16u, 32u, 64u, 0x80000000u, kEye | kFieldNormal}) {
            v.flags = bad;
            CHECK(parse() == INVALID && why[0] != 0);
        }
        for (uint32_t good : {0u, kEye}) {
            v.flags = good;
            v.clearance_cells = kPathMaxClearance;
            CHECK(parse() == OK && o.flags == good && o.clearance_cells == 4095u);
        }
        for (uint32_t r : {4096u, 7093u, 0xffffffffu}) {
            v.clearance_cells = r;
            CHECK(parse() == INVALID && why[0] != 0);
        }
        v.clearance_cells = 0;
        for (uint32_t conn : {0u, 6u, 26u}) { // 0 is read as 26
            v.connectivity = conn;
            CHECK(parse() == OK && o.connectivity == (conn ? conn : 26u));
        }
        for (uint32_t conn : {1u, 4u, 8u, 18u, 27u, 0xffffffffu}) {
            v.connectivity = conn;
            CHECK(parse() == INVALID && why[0] != 0);
        }
        v.connectivity = 26;
        for (uint32_t state : {0u, 1u}) {
            v.state = state;
            CHECK(parse() == OK && o.state == state);
        }
        for (uint32_t state : {2u, 3u, 0xffffffffu}) {
            v.state = state;
            CHECK(parse() == INVALID && why[0] != 0);
        }
        v.state = 1; // the solid state takes no clearance; the free state does
        v.clearance_cells = 1;
        CHECK(parse() == INVALID && why[0] != 0);
        v.state = 0;
        CHECK(parse() == OK && o.clearance_cells == 1u);
    }

    // the backward moves against a literal triple loop: the moves with a negative linear offset, 13 of the 26 and 3
    // of the 6, each once; with their negations all the moves
    for (uint32_t conn : {26u, 6u}) {
        std::set<std::tuple<int, int, int>> want, all, got;
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int k = std::abs(dx) + std::abs(dy) + std::abs(dz);
                    if (k == 0 || (conn == 6u && k != 1)) continue;
                    all.insert({dx, dy, dz});
                    if ((dz * 100 + dy) * 100 + dx < 0) want.insert({dx, dy, dz}); // the offset in a 100 x 100 x . lattice
                }
        CHECK(region_backward_count(conn) == (conn == 6u ? 3u : 13u) && want.size() == region_backward_count(conn));
        for (uint32_t k = 0; k < region_backward_count(conn); ++k) {
            int dx, dy, dz;
            region_backward_move(conn, k, &dx, &dy, &dz);
            CHECK(got.insert({dx, dy, dz}).second);
        }
        CHECK(got == want);
        for (const auto& m : want) got.insert({-std::get<0>(m), -std::get<1>(m), -std::get<2>(m)});
        CHECK(got == all && all.size() == (size_t)conn);
    }

    // the scratch layout: occupancy words; with a clearance the distance scratch and a word a point; the member
    // words; a word a point for the counts; the counters; each part from a multiple of 16
    {
        const uint32_t shapes[][3] = {{1, 1, 1}, {33, 5, 3}, {70, 9, 8}, {97, 1, 1}, {3, 300, 2}, {256, 64, 256}, {4096, 4096, 4}};
        auto up = [](size_t b) { return (b + 15) / 16 * 16; };
        for (const auto& d : shapes)
            for (uint32_t r : {0u, 1u, 4095u}) {
                const RegionScratch s = region_scratch(d, r);
                const size_t n = (size_t)d[0] * d[1] * d[2], occ = (size_t)((d[0] + 31) / 32) * d[1] * d[2] * 4;
                const size_t dist = r ? distance_scratch(d).lay.total + 4 * n : 0;
                CHECK(s.points == n && s.tiles.total == path_tiles(d).total);
                CHECK(s.d2_offset == (r ? up(occ) + up(4 * n) + up(8 * n) : 0));
                CHECK(s.lay.offset[REGION_OCCUPANCY] == 0 && s.lay.offset[REGION_DISTANCE] == up(occ));
                CHECK(s.lay.offset[REGION_MEMBER] == up(occ) + up(dist));
                CHECK(s.lay.offset[REGION_COUNTS] == up(occ) + up(dist) + up(occ));
                CHECK(s.lay.offset[REGION_COUNTERS] == up(occ) + up(dist) + up(occ) + up(4 * n));
                CHECK(s.lay.total == s.lay.offset[REGION_COUNTERS] + 64);
                CHECK(s.lay.total == region_scratch(d, r ? 7u : 0u).lay.total); // the clearance's value does not matter
            }
        const uint32_t empty[][3] = {{0, 2, 2}, {2, 0, 2}, {2, 2, 0}};
        for (const auto& d : empty) CHECK(region_scratch(d, 2).points == 0 && region_scratch(d, 2).lay.total == 0);
        CHECK(REGION_CNT_FAULT < REGION_CNT_STATUS && REGION_CNT_STATUS + 4 <= REGION_CNT_WORDS && REGION_CNT_WORDS * 4 == 64);
    }

    // the plan: the tile passes min(tiles, 4 cus, max_blocks), the point passes as the distance passes; a block at least
    {
        const int cus = 248;
        const uint32_t shapes[][3] = {{1, 1, 1}, {70, 9, 8}, {256, 64, 256}, {4096, 4096, 4}};
        for (const auto& d : shapes) {
            const RegionScratch s = region_scratch(d, 0);
            for (uint32_t mb : {0u, 1u, 2u, 7u, 5000u}) {
                uint32_t want = s.tiles.total < 4u * cus ? s.tiles.total : 4u * cus;
                if (mb && mb < want) want = mb;
                const RegionPlan p = plan_region(s, mb, cus);
                CHECK(p.tile_blocks == want && want >= 1u);
                CHECK(p.point_blocks == plan_distance(s.points, mb, cus).blocks && p.point_blocks >= 1u);
            }
            CHECK(plan_region(s, 0, 0).tile_blocks >= 1u && plan_region(s, 0, -3).tile_blocks <= 4u);
        }
    }

    // region_find and region_unite, the functions the kernels run, with the plain-array policy: every point its own
    // root, then every backward link united in raster, reversed and shuffled order; label[p] <= p after every step;
    // after a find of every point the forest is the flood fill's labels
    {
        std::mt19937 rng(20261021u);
        const uint32_t shapes[][3] = {{70, 9, 8}, {33, 5, 3}, {1, 1, 40}, {40, 1, 1}, {5, 6, 7}};
        for (const auto& d : shapes)
            for (double fill : {0.0, 0.3, 0.5, 0.75, 1.0})
                for (uint32_t conn : {26u, 6u}) {
                    const uint32_t n = d[0] * d[1] * d[2];
                    std::vector<unsigned char> in(n);
                    for (auto& b : in) b = std::uniform_real_distribution<double>(0.0, 1.0)(rng) >= fill;
                    const std::vector<uint32_t> want = flood(in, d, conn);
                    std::vector<std::pair<uint32_t, uint32_t>> links;
                    for (uint32_t p = 0; p < n; ++p) {
                        if (!in[p]) continue;
                        const uint32_t x = p % d[0], y = p / d[0] % d[1], z = p / (d[0] * d[1]);
                        for (uint32_t k = 0; k < region_backward_count(conn); ++k) {
                            int dx, dy, dz;
                            region_backward_move(conn, k, &dx, &dy, &dz);
                            const uint32_t u = x + (uint32_t)dx, v = y + (uint32_t)dy, t = z + (uint32_t)dz;
                            if (u >= d[0] || v >= d[1] || t >= d[2]) continue;
                            const uint32_t q = (t * d[1] + v) * d[0] + u;
                            CHECK(q < p);
                            if (in[q]) links.push_back({p, q});
                        }
                    }
                    for (int order = 0; order < 3; ++order) {
                        if (order == 1) std::reverse(links.begin(), links.end());
                        if (order == 2) std::shuffle(links.begin(), links.end(), rng);
                        std::vector<uint32_t> lab(n);
                        for (uint32_t p = 0; p < n; ++p) lab[p] = in[p] ? p : kRegionNone;
                        CheckedForest f{lab.data(), in.data()};
                        for (const auto& l : links) {
                            if (order == 2 && (l.first & 1u)) region_unite(f, l.second, l.first, n); // either end first
                            else region_unite(f, l.first, l.second, n);
                            CHECK(f.bad == 0u); // every store of the step kept the invariant
                            if (n <= 500u) // and the whole forest, where that is affordable
                                for (uint32_t p = 0; p < n; ++p) CHECK(in[p] ? lab[p] <= p : lab[p] == kRegionNone);
                            CHECK(region_find(f, l.first, n) == region_find(f, l.second, n));
                        }
                        for (uint32_t p = 0; p < n; ++p) {
                            if (!in[p]) continue;
                            const uint32_t r = region_find(f, p, n);
                            CHECK(r == want[p] && lab[r] == r);
                        }
                        CHECK(f.faults == 0u);
                    }
                }
    }

    // a word above its index is no forest: the loops end all the same, and a bound that is hit counts a fault
    {
        std::vector<uint32_t> lab = {0, 0, 1, 2, 3, 4};
        RegionHostForest f{lab.data()};
        CHECK(region_find(f, 5, 1) != 0u && f.faults == 1u); // a bound of one step on a chain of five
        std::vector<uint32_t> loop = {1, 0};                  // word 0 above its index: read as a root
        RegionHostForest g{loop.data()};
        CHECK(region_find(g, 1, 2) == 0u && g.faults == 0u);
    }
    std::printf("regionquery_check ok\n");
    return 0;
}
