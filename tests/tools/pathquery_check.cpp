// Stand-alone check of the path fields' part of gpgpuraytrace_amd/csrc/rt_rayquery.h (the host-only part of
// rt_terrain_path_field): the option parser (never read past the caller's size, unknown flags and a clearance above
// 4095 refused), the cost limit, the scratch layout, the plan, the tiles' exact cover of lattices whose dims are no
// multiples of the tile, the move tables against a literal triple loop, and the flow's smallest-code rule.
// Built with -fsanitize=address,undefined by tests/test_path_host.py; its own main.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_rayquery.h"

#define CHECK(x)                                                           \
    do {                                                                   \
        if (!(x)) {                                                        \
            std::printf("pathquery_check FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

struct PathV1 {
    uint32_t size, flags;
    float eye[3];
    uint32_t max_blocks, clearance_cells, max_cost, max_sweeps;
};
static_assert(sizeof(PathV1) == 36, "the C-ABI's size");

int main()
{
    using namespace rtq;
    const char* why = "";
    PathOptions o;

    // the option block, on the heap at its exact size
    CHECK(parse_path_options(nullptr, &o, &why) == OK && o.flags == 0 && o.max_blocks == 0 && o.clearance_cells == 0 &&
          o.max_cost == 0 && o.max_sweeps == 0);
    {
        PathV1 v = {sizeof(PathV1), kEye, {1.5f, -2.0f, 3.25f}, 7, 9, 1000, 33};
        std::vector<unsigned char> buf(sizeof v);
        std::memcpy(buf.data(), &v, sizeof v);
        CHECK(parse_path_options(buf.data(), &o, &why) == OK);
        CHECK(o.flags == kEye && o.eye[0] == 1.5f && o.eye[1] == -2.0f && o.eye[2] == 3.25f && o.max_blocks == 7 &&
              o.clearance_cells == 9 && o.max_cost == 1000 && o.max_sweeps == 33);
        for (uint32_t size : {0u, 4u, 8u, 24u, 28u, 35u}) { // too short: only the size word is read
            std::vector<unsigned char> small(4);
            std::memcpy(small.data(), &size, 4);
            why = "";
            CHECK(parse_path_options(small.data(), &o, &why) == INVALID && why[0] != 0);
        }
        v.size = 64; // a later, longer version: the first fields mean the same (the buffer stays 36 bytes)
        std::memcpy(buf.data(), &v, sizeof v);
        CHECK(parse_path_options(buf.data(), &o, &why) == OK && o.max_blocks == 7 && o.clearance_cells == 9 && o.max_sweeps == 33);
        for (uint32_t bad : {2u, 4u, 8u, 16u, 32u, 64u, 0x80000000u, kEye | kFieldNormal}) {
            v.flags = bad;
            std::memcpy(buf.data(), &v, sizeof v);
            why = "";
            CHECK(parse_path_options(buf.data(), &o, &why) == INVALID && why[0] != 0);
        }
        for (uint32_t good : {0u, kEye}) {
            v.flags = good;
            v.max_cost = 0xffffffffu;
            v.max_sweeps = 0xffffffffu; // (the entry points judge it: the two forms differ)
            v.clearance_cells = kPathMaxClearance;
            std::memcpy(buf.data(), &v, sizeof v);
            CHECK(parse_path_options(buf.data(), &o, &why) == OK && o.flags == good && o.max_cost == 0xffffffffu &&
                  o.max_sweeps == 0xffffffffu && o.clearance_cells == 4095u);
        }
        for (uint32_t r : {4096u, 7093u, 0xffffffffu}) {
            v.clearance_cells = r;
            std::memcpy(buf.data(), &v, sizeof v);
            why = "";
            CHECK(parse_path_options(buf.data(), &o, &why) == INVALID && why[0] != 0);
        }
    }

    // the limit: max_cost, or everything below the far value; a finite cost is below 5 * 2^26 and never overflows
    CHECK(path_limit(0) == kPathFar - 1u && path_limit(1) == 1u && path_limit(627) == 627u && path_limit(kPathFar) == kPathFar);
    CHECK(5ull * (1ull << 26) + 5ull < (uint64_t)kPathFar);
    // a clearance within the distance passes' own bound: max_cells = R leaves d2 far exactly when d2 > R * R
    CHECK(kPathMaxClearance < kDistMaxCells && distance_bound(kPathMaxClearance).limit2 == 4095u * 4095u);

    // the move tables against a literal triple loop
    {
        uint32_t c = 0, faces = 0, edges = 0, corners = 0;
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx, ++c) {
                    int x, y, z;
                    path_move(c, &x, &y, &z);
                    CHECK(x == dx && y == dy && z == dz);
                    CHECK(c == (uint32_t)((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)));
                    const int k = std::abs(dx) + std::abs(dy) + std::abs(dz);
                    const uint32_t want = k == 0 ? 0u : k == 1 ? 3u : k == 2 ? 4u : 5u;
                    CHECK(path_weight(dx, dy, dz) == want);
                    faces += k == 1, edges += k == 2, corners += k == 3;
                    CHECK((c == kPathStay) == (k == 0));
                }
        CHECK(c == 27u && faces == 6u && edges == 12u && corners == 8u);
    }

    // the flow: the smallest code whose neighbour explains the cost; far neighbours and the lattice's edge skipped
    {
        const uint32_t dims[3] = {3, 3, 3};
        std::vector<uint32_t> cost(27, kPathFar);
        auto at = [&](uint32_t i) { return cost.at(i); };
        cost[13] = 10;
        CHECK(path_flow(at, dims, 1, 1, 1, 10) == kPathNone);
        cost[26] = 5; // (+1, +1, +1): a corner
        CHECK(path_flow(at, dims, 1, 1, 1, 10) == 26u);
        cost[14] = 7; // (+1, 0, 0): a face
        CHECK(path_flow(at, dims, 1, 1, 1, 10) == 14u);
        cost[1] = 6; // (0, -1, -1): an edge, the smallest code of the three
        CHECK(path_flow(at, dims, 1, 1, 1, 10) == 1u);
        cost[0] = 6; // a corner at the wrong cost
        CHECK(path_flow(at, dims, 1, 1, 1, 10) == 1u);
        // at the lattice's corner only the seven neighbours that exist are read (vector::at would throw)
        std::vector<uint32_t> open(27);
        for (uint32_t i = 0; i < 27u; ++i) open[i] = 100u * i; // not a chamfer field: numbers that only one neighbour explains
        auto at2 = [&](uint32_t i) { return open.at(i); };
        CHECK(path_flow(at2, dims, 0, 0, 0, open[1] + 3u) == 14u);
        CHECK(path_flow(at2, dims, 2, 2, 2, open[25] + 3u) == 12u);
        const uint32_t line[3] = {1, 1, 4};
        std::vector<uint32_t> col = {0, 3, 6, 9};
        auto at3 = [&](uint32_t i) { return col.at(i); };
        CHECK(path_flow(at3, line, 0, 0, 3, 9) == 4u && path_flow(at3, line, 0, 0, 1, 3) == 4u);
    }

    // the tiles: every point in exactly one tile, tile_of agrees with the tile's box, the halo's size
    {
        CHECK(kPathTilePoints == 512u && kPathHaloPoints == 34u * 6u * 6u);
        const uint32_t shapes[][3] = {{1, 1, 1}, {33, 5, 3},  {70, 9, 8}, {97, 1, 1}, {3, 300, 2},
                                      {2, 2, 300}, {32, 4, 4}, {64, 8, 8}, {31, 3, 5}};
        for (const auto& d : shapes) {
            const PathTiles t = path_tiles(d);
            CHECK(t.n[0] == (d[0] + 31u) / 32u && t.n[1] == (d[1] + 3u) / 4u && t.n[2] == (d[2] + 3u) / 4u);
            CHECK(t.total == t.n[0] * t.n[1] * t.n[2] && t.total >= 1u);
            std::vector<unsigned char> seen((size_t)d[0] * d[1] * d[2], 0);
            for (uint32_t tile = 0; tile < t.total; ++tile) {
                const uint32_t tx = tile % t.n[0], ty = tile / t.n[0] % t.n[1], tz = tile / (t.n[0] * t.n[1]);
                for (uint32_t p = 0; p < kPathTilePoints; ++p) { // the sweep's thread p of this tile
                    const uint32_t ix = tx * kPathTileX + p % kPathTileX, iy = ty * kPathTileY + p / kPathTileX % kPathTileY,
                                   iz = tz * kPathTileZ + p / (kPathTileX * kPathTileY);
                    if (ix >= d[0] || iy >= d[1] || iz >= d[2]) continue;
                    CHECK(path_tile_of(t, ix, iy, iz) == tile);
                    unsigned char& s = seen.at(((size_t)iz * d[1] + iy) * d[0] + ix);
                    CHECK(!s);
                    s = 1;
                }
            }
            for (unsigned char v : seen) CHECK(v == 1);
        }
    }

    // the scratch layout: occupancy words; with a clearance the distance scratch and a word a point; the passable
    // words; two words a tile; the counters; each part from a multiple of 16
    {
        const uint32_t shapes[][3] = {{1, 1, 1}, {33, 5, 3}, {70, 9, 8}, {97, 1, 1}, {3, 300, 2}, {256, 64, 256}, {4096, 4096, 4}};
        auto up = [](size_t b) { return (b + 15) / 16 * 16; };
        for (const auto& d : shapes)
            for (uint32_t r : {0u, 1u, 4095u}) {
                const PathScratch s = path_scratch(d, r);
                const size_t n = (size_t)d[0] * d[1] * d[2], occ = (size_t)((d[0] + 31) / 32) * d[1] * d[2] * 4;
                const size_t tiles = (size_t)((d[0] + 31) / 32) * ((d[1] + 3) / 4) * ((d[2] + 3) / 4);
                const size_t dist = r ? distance_scratch(d).lay.total + 4 * n : 0;
                CHECK(s.points == n && s.tiles.total == tiles);
                CHECK(s.d2_offset == (r ? up(occ) + up(4 * n) + up(8 * n) : 0));
                CHECK(s.lay.offset[PATH_OCCUPANCY] == 0 && s.lay.offset[PATH_DISTANCE] == up(occ));
                CHECK(s.lay.offset[PATH_PASSABLE] == up(occ) + up(dist));
                CHECK(s.lay.offset[PATH_FLAGS] == up(occ) + up(dist) + up(occ));
                CHECK(s.lay.offset[PATH_COUNTERS] == up(occ) + up(dist) + up(occ) + up(8 * tiles));
                CHECK(s.lay.total == s.lay.offset[PATH_COUNTERS] + 64);
            }
        const uint32_t empty[][3] = {{0, 2, 2}, {2, 0, 2}, {2, 2, 0}};
        for (const auto& d : empty) CHECK(path_scratch(d, 2).points == 0 && path_scratch(d, 2).lay.total == 0);
        CHECK(PATH_CNT_ACTIVE + 3 <= PATH_CNT_WORKED && PATH_CNT_WORKED + 2 <= PATH_CNT_SWEEPS && PATH_CNT_VISITS < PATH_CNT_WORDS);
    }

    // the plan: the sweep min(tiles, 4 cus, max_blocks), the point passes as the distance passes; at least a block
    {
        const int cus = 248;
        const uint32_t shapes[][3] = {{1, 1, 1}, {70, 9, 8}, {256, 64, 256}, {4096, 4096, 4}};
        for (const auto& d : shapes) {
            const PathScratch s = path_scratch(d, 0);
            for (uint32_t mb : {0u, 1u, 2u, 7u, 5000u}) {
                uint32_t want = s.tiles.total < 4u * cus ? s.tiles.total : 4u * cus;
                if (mb && mb < want) want = mb;
                const PathPlan p = plan_path(s, mb, cus);
                CHECK(p.sweep_blocks == want && want >= 1u);
                CHECK(p.point_blocks == plan_distance(s.points, mb, cus).blocks && p.point_blocks >= 1u);
            }
            CHECK(plan_path(s, 0, 0).sweep_blocks >= 1u && plan_path(s, 0, -3).sweep_blocks <= 4u);
        }
    }
    std::printf("pathquery_check ok\n");
    return 0;
}
