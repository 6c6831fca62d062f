// Stand-alone check of the mesh extraction's part of gpgpuraytrace_amd/csrc/rt_rayquery.h (the host-only part of
// rt_terrain_extract_mesh): the scratch layout (parts in order, 16-byte aligned, inside the total, none without
// cells), the grids of the passes, and the mask arithmetic k_meshcount runs per mask word (mesh_masks), driven over
// random occupancy words on heap arrays of their exact size and compared with a bit-by-bit loop over the cells.
// Built with -fsanitize=address,undefined by tests/test_mesh_host.py; its own main.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_rayquery.h"

#define CHECK(x)                                                           \
    do {                                                                   \
        if (!(x)) {                                                        \
            std::printf("meshquery_check FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 32);
}

// fill: 0 random bits, 1 random runs (surfaces are runs of equal bits), 2 all inside, 3 all outside
static int check_masks(uint32_t nx, uint32_t ny, uint32_t nz, int fill)
{
    using namespace rtq;
    const uint32_t dims[3] = {nx, ny, nz};
    const uint32_t occ_words = (nx + 31u) / 32u;
    std::vector<unsigned char> in((size_t)nx * ny * nz);
    unsigned char run = 0;
    for (auto& b : in) {
        if (fill == 0) b = rnd() & 1u;
        else if (fill == 1) b = run = (rnd() % 9u == 0u) ? !run : run;
        else b = fill == 2;
    }
    std::vector<uint32_t> occ(occupancy_bytes(dims) / 4, 0u); // exact size: a read past a row's words is caught
    for (uint32_t z = 0; z < nz; ++z)
        for (uint32_t y = 0; y < ny; ++y)
            for (uint32_t x = 0; x < nx; ++x)
                if (in[((size_t)z * ny + y) * nx + x]) occ[((size_t)z * ny + y) * occ_words + x / 32u] |= 1u << (x % 32u);
    const MeshScratch s = mesh_scratch(dims);
    CHECK(s.row_words == (nx - 1u + 63u) / 64u && s.words == s.row_words * (ny - 1u) * (nz - 1u));
    auto at = [&](uint32_t x, uint32_t y, uint32_t z) { return in[((size_t)z * ny + y) * nx + x] != 0; };
    uint64_t vertices = 0, quads = 0;
    for (uint32_t w = 0; w < s.words; ++w) {
        // as k_meshcount decodes a word
        const uint32_t j = w % s.row_words, row = w / s.row_words, cy = row % (ny - 1u), cz = row / (ny - 1u);
        const uint32_t* r00 = occ.data() + ((size_t)cz * ny + cy) * occ_words;
        const uint32_t* r01 = r00 + (size_t)ny * occ_words;
        const MeshMasks m = mesh_masks(r00, r00 + occ_words, r01, r01 + occ_words, occ_words, j, nx, cy, cz);
        MeshMasks want = {0, 0, 0, 0};
        for (uint32_t b = 0; b < 64u; ++b) {
            const uint32_t cx = 64u * j + b;
            if (cx >= nx - 1u) break;
            uint32_t n_in = 0;
            for (uint32_t k = 0; k < 8u; ++k) n_in += at(cx + (k & 1u), cy + ((k >> 1) & 1u), cz + (k >> 2));
            const uint64_t bit = 1ull << b;
            if (n_in > 0 && n_in < 8) want.active |= bit;
            const bool c0 = at(cx, cy, cz);
            if (cy >= 1 && cz >= 1 && c0 != at(cx + 1, cy, cz)) want.ex |= bit;
            if (cz >= 1 && cx >= 1 && c0 != at(cx, cy + 1, cz)) want.ey |= bit;
            if (cx >= 1 && cy >= 1 && c0 != at(cx, cy, cz + 1)) want.ez |= bit;
        }
        CHECK(m.active == want.active && m.ex == want.ex && m.ey == want.ey && m.ez == want.ez);
        CHECK(((m.ex | m.ey | m.ez) & ~m.active) == 0); // a cell with a crossing edge is active
        CHECK(mesh_popc(m.active) == (uint32_t)__builtin_popcountll(want.active));
        vertices += mesh_popc(m.active);
        quads += mesh_popc(m.ex) + mesh_popc(m.ey) + mesh_popc(m.ez);
    }
    CHECK(vertices <= s.cells && quads <= 3ull * s.cells);
    if (fill >= 2) CHECK(vertices == 0 && quads == 0);
    return 0;
}

int main()
{
    using namespace rtq;

    // the scratch layout
    const uint32_t shapes[][3] = {{2, 2, 2},   {3, 3, 3},    {33, 5, 3},      {66, 4, 3},     {130, 6, 5}, {48, 24, 40},
                                  {65, 2, 2},  {64, 2, 2},   {129, 3, 2},     {256, 64, 256}, {4096, 2, 2}, {2, 4096, 2},
                                  {2, 2, 4096}, {4096, 4096, 4}};
    for (const auto& d : shapes) {
        const MeshScratch s = mesh_scratch(d);
        CHECK(s.points == d[0] * d[1] * d[2] && s.cells == (d[0] - 1u) * (d[1] - 1u) * (d[2] - 1u) && s.cells >= 1);
        CHECK(s.row_words * 64u >= d[0] - 1u && (s.row_words - 1u) * 64u < d[0] - 1u);
        CHECK(s.words == s.row_words * (d[1] - 1u) * (d[2] - 1u) && s.words <= s.cells);
        const size_t bytes[4] = {(size_t)s.points * 4, occupancy_bytes(d), (size_t)s.words * 32, (size_t)s.words * 8};
        size_t end = 0;
        for (int i = 0; i < 4; ++i) {
            CHECK(s.lay.offset[i] % 16 == 0 && s.lay.offset[i] >= end);
            end = s.lay.offset[i] + bytes[i];
        }
        CHECK(end <= s.lay.total && s.lay.total % 16 == 0 && s.lay.total < end + 16);
        // the grids: at least one block, never more than the work or the cap
        const uint32_t cus = 248;
        for (uint32_t cap : {0u, 1u, 7u, s.cells, 0xffffffffu}) {
            const MeshPlan p = plan_mesh(s, cap, 0, (int)cus);
            // (a word a thread, a word a wave, in blocks of kMeshThreads; eight such blocks a CU)
            CHECK(p.count_blocks >= 1 && p.count_blocks <= 8u * cus && p.count_blocks <= (s.words + 255u) / 256u);
            CHECK(p.emit_blocks >= 1 && p.emit_blocks <= 8u * cus && p.emit_blocks <= (s.words + 3u) / 4u);
            CHECK(p.count_blocks == 8u * cus || p.count_blocks * kMeshThreads >= s.words);
            CHECK(p.emit_blocks == 8u * cus || p.emit_blocks * kMeshWaves >= s.words);
            const uint32_t v = cap < s.cells ? cap : s.cells;
            CHECK(p.normal_blocks == ((v + 1023u) / 1024u < cus ? (v + 1023u) / 1024u : cus));
            const MeshPlan one = plan_mesh(s, cap, 1, (int)cus);
            CHECK(one.count_blocks == 1 && one.emit_blocks == 1 && one.normal_blocks <= 1);
        }
    }
    // no cells: nothing to lay out
    const uint32_t flat[][3] = {{97, 1, 4}, {1, 5, 5}, {5, 5, 1}, {0, 3, 3}, {1, 1, 1}};
    for (const auto& d : flat) {
        const MeshScratch s = mesh_scratch(d);
        CHECK(s.cells == 0 && s.words == 0 && s.row_words == 0 && s.lay.total == 0);
    }

    // the mask arithmetic: rows of 1, 2, 3 and 5 occupancy words, cell rows that end at bit 63, 0 and 1 of a word
    const uint32_t lattices[][3] = {{2, 2, 2},  {3, 3, 3},  {33, 5, 3},  {64, 3, 3}, {65, 3, 3}, {66, 4, 3},
                                    {97, 3, 4}, {129, 3, 3}, {130, 6, 5}, {160, 2, 3}};
    for (const auto& d : lattices)
        for (int fill = 0; fill < 4; ++fill)
            for (int rep = 0; rep < (fill < 2 ? 4 : 1); ++rep)
                if (check_masks(d[0], d[1], d[2], fill)) return 1;
    std::printf("meshquery_check ok\n");
    return 0;
}
