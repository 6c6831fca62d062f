// rt_rayquery.h -- host-only decisions of rt_terrain_trace_rays, rt_terrain_trace_surface,
// rt_terrain_shade_rays, rt_terrain_shade_points and the field queries rt_terrain_sample_field /
// rt_terrain_sample_lattice (include/frosttrace.h): the option blocks' validation, the choice of the kernel shape,
// its lanes per ray, its strips and its grid, the layout of the host forms' device block, and the scratch layout,
// grids and mask arithmetic of rt_terrain_extract_mesh.  No HIP in here (the mask arithmetic is marked
// __host__ __device__ under hipcc only, for k_meshcount): tests/tools/rayquery_check.cpp, surfquery_check.cpp,
// shadequery_check.cpp, pointquery_check.cpp, fieldquery_check.cpp, meshquery_check.cpp, distquery_check.cpp,
// pathquery_check.cpp, visquery_check.cpp, regionquery_check.cpp and querylayout_check.cpp
// drive it stand-alone under ASan + UBSan.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace rtq {

constexpr int kMaxRays = 1 << 26;
// rt_ray_options.flags (RT_RAYS_*)
constexpr uint32_t kEye = 1u, kForceSegments = 2u, kForceLanes = 4u;
// the first version of rt_ray_options: size, flags, eye[3], max_blocks
constexpr uint32_t kOptSizeV1 = 24u;
// error codes of the C-ABI (RT_OK, RT_ERR_INVALID, RT_ERR_UNSUPPORTED)
enum { OK = 0, INVALID = -1, UNSUPPORTED = -4 };
enum Shape { SEGMENTS = 0, LANES = 1 };

// Auto mode on nomadplains: segments up to this many rays, lanes beyond.  A segment march is the prepass's latency
// shape (one LPR-lane group per ray, a static deal of 128 rays a block at most): about 0.4 ms per round of blocks
// over the CUs, so it grows with n from 65,536 rays on, while the persistent lane kernel takes about 2.2 ms (its
// longest ray on one lane) from 1,024 rays to 262,144.  Measured (profiles/r08/ray_query.md): segments 0.97 ms
// against lanes 2.16 ms at 65,536 rays, 1.77 against 2.21 at 131,072, 2.44 against 2.42 at 196,608, 3.22 against
// 2.52 at 262,144: the crossing lies between 131,072 and 196,608.
constexpr int kAutoSegmentsMax = 128 * 1024;

// the prefix the three option blocks share: size, flags, eye[3], max_blocks
struct Options {
    uint32_t flags = 0;
    float eye[3] = {0.0f, 0.0f, 0.0f};
    uint32_t max_blocks = 0;
};
using FieldOptions = Options;

// The version-1 prefix of the caller's option block `opt` (not null), read through its size field: a size below
// `size_v1`, the family's first version, is an error (false, nothing read beyond the size); a larger one is a
// later version whose extra fields this build ignores.
inline bool parse_prefix(const void* opt, uint32_t size_v1, Options* out)
{
    uint32_t size;
    std::memcpy(&size, opt, 4);
    if (size < size_v1) return false;
    const char* p = static_cast<const char*>(opt);
    std::memcpy(&out->flags, p + 4, 4);
    std::memcpy(out->eye, p + 8, 12);
    std::memcpy(&out->max_blocks, p + 20, 4);
    return true;
}

inline bool both_shapes_forced(uint32_t flags, const char** why)
{
    if (!(flags & kForceSegments) || !(flags & kForceLanes)) return false;
    *why = "RT_RAYS_FORCE_SEGMENTS and RT_RAYS_FORCE_LANES are both set";
    return true;
}

// `opt` is the caller's rt_ray_options (may be null: the defaults), read as far as the first version reaches.
inline int parse_options(const void* opt, Options* out, const char** why)
{
    *out = Options{};
    if (!opt) return OK;
    if (!parse_prefix(opt, kOptSizeV1, out)) {
        *why = "rt_ray_options.size is smaller than the struct's first version";
        return INVALID;
    }
    return both_shapes_forced(out->flags, why) ? INVALID : OK;
}

inline int check_count(int n, const char** why)
{
    if (n < 0 || n > kMaxRays) {
        *why = "the ray count must be 0..2^26";
        return INVALID;
    }
    return OK;
}

struct Plan {
    int shape = LANES;
    int bs = 1024, lpr = 1; // threads per block, lanes per ray
    uint32_t blocks = 0;
};

// n >= 1 rays; nomadplains: the compute's landscape is it (the only one with a segment shape); cus: the CUs a
// persistent grid may take; prepass_bs1 / prepass_lpr1: the one-frame prepass's block size and lanes per ray.
inline int plan(int n, bool nomadplains, uint32_t flags, uint32_t max_blocks, int cus, int prepass_bs1,
                int prepass_lpr1, Plan* out, const char** why)
{
    Plan p;
    if (flags & kForceSegments) {
        if (!nomadplains) {
            *why = "the segment shape exists for nomadplains only";
            return UNSUPPORTED;
        }
        p.shape = SEGMENTS;
    } else if (flags & kForceLanes) {
        p.shape = LANES;
    } else {
        p.shape = nomadplains && n <= kAutoSegmentsMax ? SEGMENTS : LANES;
    }
    if (p.shape == SEGMENTS) {
        // the prepass's ladder by batch size (launch_camerarays_l), in rays: up to 2 frames the one-frame
        // shape, up to 4 frames 16 rays of 32 lanes per block, up to 16 frames 64 rays of 8, beyond 128 of 4
        if (n <= 2 * 1024) {
            p.bs = prepass_bs1;
            p.lpr = prepass_lpr1;
        } else if (n <= 4 * 1024) {
            p.bs = 512;
            p.lpr = 32;
        } else if (n <= 16 * 1024) {
            p.bs = 512;
            p.lpr = 8;
        } else {
            p.bs = 512;
            p.lpr = 4;
        }
        const uint32_t per_block = (uint32_t)(p.bs / p.lpr);
        p.blocks = ((uint32_t)n + per_block - 1u) / per_block;
    } else {
        p.bs = 1024;
        p.lpr = 1;
        uint32_t b = (uint32_t)(cus > 0 ? cus : 1);
        if (max_blocks && max_blocks < b) b = max_blocks;
        const uint32_t need = ((uint32_t)n + 1023u) / 1024u;
        p.blocks = need < b ? need : b;
    }
    *out = p;
    return OK;
}

// ---- surface queries (rt_terrain_trace_surface): their own option block, the same shapes ----

// rt_surface_options.flags beside kEye / kForceSegments / kForceLanes (RT_SURFACE_*)
constexpr uint32_t kSurfParams = 8u, kSurfRayRange = 16u;
// the first version of rt_surface_options: size, flags, eye[3], max_blocks, t_min, t_max, stepmod, max_steps
constexpr uint32_t kSurfOptSizeV1 = 40u;
// the values a tracescreen pixel gets with an empty CellDistance (tracescreen.hlsl:20, tracing.hlsl:3-4)
constexpr float kSurfTMin = 0.01f, kSurfTMax = 5000.0f, kSurfStepmod = 1.0f;
// Auto mode on nomadplains for surface queries: segments up to this many rays, lanes beyond.  The refined march
// is about 1.3x the prepass's iterations, so the segment shape's static deal grows sooner than the ray queries'
// (kAutoSegmentsMax).  Measured (profiles/r10/surface_query.md): segments 0.82 ms against lanes 2.82 ms at 32,768
// rays, 1.61 against 2.89 at 65,536, 3.24 against 2.96 at 131,072, 4.82 against 3.00 at 196,608, 6.41 against
// 3.11 at 262,144.  Segments are linear in n from 65,536 on (24.7 us per 1,024 rays), which puts the crossing
// near 119,000 rays; the rule sits just below it.
constexpr int kSurfAutoSegmentsMax = 112 * 1024;

struct SurfOptions : Options {
    float t_min = kSurfTMin, t_max = kSurfTMax, stepmod = kSurfStepmod;
    uint32_t max_steps = 0; // 0: unbounded
};

inline bool finite_f(float x) { return x - x == 0.0f; }

// `opt` is the caller's rt_surface_options (may be null: the defaults), read as far as the first version
// reaches.  The four trailing fields count with RT_SURFACE_PARAMS only.
inline int parse_surface_options(const void* opt, SurfOptions* out, const char** why)
{
    *out = SurfOptions{};
    if (!opt) return OK;
    if (!parse_prefix(opt, kSurfOptSizeV1, out)) {
        *why = "rt_surface_options.size is smaller than the struct's first version";
        return INVALID;
    }
    if (both_shapes_forced(out->flags, why)) return INVALID;
    const char* p = static_cast<const char*>(opt);
    if (out->flags & kSurfParams) {
        std::memcpy(&out->t_min, p + 24, 4);
        std::memcpy(&out->t_max, p + 28, 4);
        std::memcpy(&out->stepmod, p + 32, 4);
        std::memcpy(&out->max_steps, p + 36, 4);
        if (!finite_f(out->stepmod) || !(out->stepmod > 0.0f)) {
            *why = "rt_surface_options.stepmod must be finite and above 0";
            return INVALID;
        }
        if (!(out->t_max >= out->t_min)) { // (a NaN bound too)
            *why = "rt_surface_options.t_max is below t_min";
            return INVALID;
        }
    }
    return OK;
}

// the kernels count a ray's iterations in an int: a cap beyond it is no cap that a march could reach
inline int surface_max_steps(uint32_t max_steps) { return max_steps > 0x7fffffffu ? 0x7fffffff : (int)max_steps; }

// the plan of a surface query: plan() with the surface queries' own auto rule
inline int plan_surface(int n, bool nomadplains, uint32_t flags, uint32_t max_blocks, int cus, int prepass_bs1,
                        int prepass_lpr1, Plan* out, const char** why)
{
    uint32_t f = flags & (kForceSegments | kForceLanes);
    if (!f && nomadplains) f = n <= kSurfAutoSegmentsMax ? kForceSegments : kForceLanes;
    return plan(n, nomadplains, f, max_blocks, cus, prepass_bs1, prepass_lpr1, out, why);
}

// ---- shaded queries (rt_terrain_shade_rays): the surface queries' option block, the lanes shape only ----

// the plan of a shaded query: always lanes (there is no segment shape), its grid min(ceil(n / 1024), cus,
// max_blocks); cus: the CUs a persistent grid may take
inline int plan_shade(int n, uint32_t flags, uint32_t max_blocks, int cus, Plan* out, const char** why)
{
    if (flags & kForceSegments) {
        *why = "shaded queries have no segment shape";
        return UNSUPPORTED;
    }
    return plan(n, false, kForceLanes, max_blocks, cus, 0, 0, out, why);
}

// ---- point shading (rt_terrain_shade_points): its own option block, the lanes shape only ----

// the first version of rt_point_options: size, flags, eye[3], max_blocks, ao_samples, seed
constexpr uint32_t kPointOptSizeV1 = 32u;
// ao_dir packs the AO ray's index into 4 bits
constexpr uint32_t kPointMaxAO = 16u;

struct PointOptions : Options {
    uint32_t ao_samples = 0, seed = 0;
};

// `opt` is the caller's rt_point_options (may be null: the defaults), read as far as the first version reaches.
inline int parse_point_options(const void* opt, PointOptions* out, const char** why)
{
    *out = PointOptions{};
    if (!opt) return OK;
    if (!parse_prefix(opt, kPointOptSizeV1, out)) {
        *why = "rt_point_options.size is smaller than the struct's first version";
        return INVALID;
    }
    if (out->flags & ~kEye) {
        *why = "rt_point_options.flags has bits other than RT_RAYS_EYE";
        return INVALID;
    }
    const char* p = static_cast<const char*>(opt);
    std::memcpy(&out->ao_samples, p + 24, 4);
    std::memcpy(&out->seed, p + 28, 4);
    if (out->ao_samples > kPointMaxAO) {
        *why = "rt_point_options.ao_samples is above 16";
        return INVALID;
    }
    return OK;
}

// the plan of a point shading query of n >= 1 points: always lanes, its grid min(ceil(n / 1024), cus, max_blocks)
inline Plan plan_points(int n, uint32_t max_blocks, int cus)
{
    Plan p;
    const char* why = "";
    plan(n, false, kForceLanes, max_blocks, cus, 0, 0, &p, &why);
    return p;
}

// ---- field queries (rt_terrain_sample_field, rt_terrain_sample_lattice): density and normal at points ----

// rt_field_options.flags beside kEye (RT_FIELD_NORMAL); every other bit is an error
constexpr uint32_t kFieldNormal = 32u;
// the first version of rt_field_options: size, flags, eye[3], max_blocks
constexpr uint32_t kFieldOptSizeV1 = 24u;
constexpr uint32_t kMaxLatticeDim = 4096u;
// iy rows of a lattice strip (k_fieldlattice: a wave walks 64 ix by this many iy of one iz, and on nomadplains
// computes its columns' steep noise once per strip).  Measured on a 256 x 128 x 256 lattice
// (profiles/r12/field_query.md): 0.2187 ms at 1 row, 0.2052 at 4, 0.2034 at 8, 0.2048 at 16, 0.2119 at 32;
// 0.2065 at 8 rows without the column reuse; the point form 0.2113.
constexpr uint32_t kFieldRows = 8u;
// waves of a field kernel's block (1024 threads)
constexpr uint32_t kFieldWaves = 16u;

// `opt` is the caller's rt_field_options (may be null: the defaults), read as far as the first version reaches.
inline int parse_field_options(const void* opt, FieldOptions* out, const char** why)
{
    *out = FieldOptions{};
    if (!opt) return OK;
    if (!parse_prefix(opt, kFieldOptSizeV1, out)) {
        *why = "rt_field_options.size is smaller than the struct's first version";
        return INVALID;
    }
    if (out->flags & ~(kEye | kFieldNormal)) {
        *why = "rt_field_options.flags has bits other than RT_RAYS_EYE and RT_FIELD_NORMAL";
        return INVALID;
    }
    return OK;
}

struct Lattice {
    float origin[3], spacing[3];
    uint32_t dims[3];
};

// `lat` is the caller's rt_lattice (36 bytes); *n: its points (0: nothing to do)
inline int check_lattice(const void* lat, Lattice* out, uint32_t* n, const char** why)
{
    if (!lat) {
        *why = "null rt_lattice";
        return INVALID;
    }
    std::memcpy(out, lat, sizeof(Lattice));
    uint64_t total = 1;
    for (int i = 0; i < 3; ++i) {
        if (out->dims[i] > kMaxLatticeDim) {
            *why = "a lattice dimension is above 4096";
            return INVALID;
        }
        if (!finite_f(out->origin[i]) || !finite_f(out->spacing[i])) {
            *why = "the lattice's origin and spacing must be finite";
            return INVALID;
        }
        total *= out->dims[i];
    }
    if (total > (uint64_t)kMaxRays) {
        *why = "the lattice has more than 2^26 points";
        return INVALID;
    }
    *n = (uint32_t)total;
    return OK;
}

struct FieldPlan {
    uint32_t blocks = 0; // of 1024 threads, striding over the work
    uint32_t rows = 1;   // (lattice) iy rows per strip
    bool column = false; // (lattice) nomadplains' steep noise once per strip column
};

inline uint32_t field_grid(uint32_t need, uint32_t max_blocks, int cus)
{
    uint32_t b = (uint32_t)(cus > 0 ? cus : 1);
    if (max_blocks && max_blocks < b) b = max_blocks;
    return need < b ? need : b;
}

// n >= 1 points from memory: tiles of 1024, grid min(tiles, cus, max_blocks)
inline FieldPlan plan_field_points(uint32_t n, uint32_t max_blocks, int cus)
{
    FieldPlan p;
    p.blocks = field_grid((n + 1023u) / 1024u, max_blocks, cus);
    return p;
}

// strips of a lattice whose dims are all >= 1: 64 ix by `rows` iy of one iz
inline uint32_t lattice_strips(const uint32_t dims[3], uint32_t rows)
{
    return ((dims[0] + 63u) / 64u) * ((dims[1] + rows - 1u) / rows) * dims[2];
}

// a lattice of >= 1 points (check_lattice passed): grid min(ceil(strips / 16), cus, max_blocks)
inline FieldPlan plan_field_lattice(const uint32_t dims[3], bool nomadplains, uint32_t max_blocks, int cus)
{
    FieldPlan p;
    p.rows = dims[1] < kFieldRows ? dims[1] : kFieldRows;
    p.column = nomadplains && p.rows > 1u;
    const uint32_t strips = lattice_strips(dims, p.rows);
    p.blocks = field_grid((strips + kFieldWaves - 1u) / kFieldWaves, max_blocks, cus);
    return p;
}

// ---- the host forms' device block: one allocation holding a query's arrays ----

// bytes per element of the arrays: a packed ray, a packed point (or normal), a ray result, a surface or shaded
// result, a shaded point's result, an RGBA8 pixel, a ray's or surface ray's step count, a shaded ray's or point's two
constexpr size_t kRayBytes = 32, kPointBytes = 16, kRayResultBytes = 16, kSurfResultBytes = 32, kPointResultBytes = 16,
                 kPixelBytes = 4, kStepsBytes = 4, kShadeStepsBytes = 8;
// a field result's bytes per point: the density, or with the normal {n.xyz, d}
inline size_t field_stride(uint32_t flags) { return (flags & kFieldNormal) ? 16 : 4; }
// a lattice's occupancy: one bit a point, ceil(nx / 32) words a row
inline size_t occupancy_bytes(const uint32_t dims[3])
{
    return (size_t)((dims[0] + 31u) / 32u) * dims[1] * dims[2] * 4;
}

constexpr int kBlockParts = 5;
struct BlockLayout {
    size_t offset[kBlockParts] = {};
    size_t total = 0;
};

// parts <= kBlockParts sizes in bytes, in order; 0: the part is absent and takes no space.  Every present part
// starts at a multiple of 16 (the kernels' float4 accesses), so the total is the present parts' sizes, each
// rounded up to 16.
inline BlockLayout block_layout(const size_t* bytes, int parts)
{
    BlockLayout l;
    for (int i = 0; i < parts && i < kBlockParts; ++i) {
        l.offset[i] = l.total;
        l.total += (bytes[i] + 15) / 16 * 16;
    }
    return l;
}

// point i of a packed field query: x y z _
inline void pack_points(const float* points, int n, float* packed)
{
    for (int i = 0; i < n; ++i) {
        float* r = packed + (size_t)i * 4;
        r[0] = points[3 * (size_t)i];
        r[1] = points[3 * (size_t)i + 1];
        r[2] = points[3 * (size_t)i + 2];
        r[3] = 0.0f;
    }
}

// ray i of a packed query with its range: ox oy oz t_min_i dx dy dz t_max_i (ranges: 2n floats)
inline void pack_ranges(const float* ranges, int n, float* packed)
{
    for (int i = 0; i < n; ++i) {
        packed[(size_t)i * 8 + 3] = ranges[2 * (size_t)i];
        packed[(size_t)i * 8 + 7] = ranges[2 * (size_t)i + 1];
    }
}

// ray i of a packed query: ox oy oz _ dx dy dz _
inline void pack(const float* origins, const float* dirs, int n, float* packed)
{
    for (int i = 0; i < n; ++i) {
        float* r = packed + (size_t)i * 8;
        r[0] = origins[3 * (size_t)i];
        r[1] = origins[3 * (size_t)i + 1];
        r[2] = origins[3 * (size_t)i + 2];
        r[3] = 0.0f;
        r[4] = dirs[3 * (size_t)i];
        r[5] = dirs[3 * (size_t)i + 1];
        r[6] = dirs[3 * (size_t)i + 2];
        r[7] = 0.0f;
    }
}

// ---- mesh extraction (rt_terrain_extract_mesh): a surface-nets mesh of a lattice's density ----
//
// A cell row is the cells (cx, cy, cz) of one (cy, cz); it is cut into mask words of 64 consecutive cx, so bit b of
// word j of a row is cell cx = 64 j + b.  A word carries four 64-bit masks (MeshMasks) and, after the scan, the
// number of vertices and of quads that precede it in cell order.

// the masks of one word: active cells, and the cells whose corner-0 edge along x / y / z crosses the surface and is
// interior (the other two cell coordinates >= 1): each such bit is one quad
struct MeshMasks {
    uint64_t active, ex, ey, ez;
};
constexpr size_t kMeshMaskBytes = 32, kMeshOffsetBytes = 8, kMeshVertexBytes = 16, kMeshTriangleBytes = 12;

#if defined(__HIPCC__)
#define RTQ_HD __host__ __device__
#else
#define RTQ_HD
#endif

// points 64 j .. 64 j + 63 of an occupancy row of occ_words words (the padding bits are 0) in *lo, and the same
// shifted by one point, 64 j + 1 .. 64 j + 64, in *hi; points beyond the row read as 0
RTQ_HD inline void mesh_row_bits(const uint32_t* row, uint32_t occ_words, uint32_t j, uint64_t* lo, uint64_t* hi)
{
    const uint32_t w = 2u * j;
    const uint64_t w0 = w < occ_words ? row[w] : 0u, w1 = w + 1u < occ_words ? row[w + 1u] : 0u,
                   w2 = w + 2u < occ_words ? row[w + 2u] : 0u;
    *lo = w0 | (w1 << 32);
    *hi = (*lo >> 1) | ((w2 & 1u) << 63);
}

// The masks of word j of cell row (cy, cz) of a lattice of nx points a row (64 j < nx - 1), from the occupancy
// rows of its four point rows: r00 = (cy, cz), r10 = (cy + 1, cz), r01 = (cy, cz + 1), r11 = (cy + 1, cz + 1).
RTQ_HD inline MeshMasks mesh_masks(const uint32_t* r00, const uint32_t* r10, const uint32_t* r01, const uint32_t* r11,
                                   uint32_t occ_words, uint32_t j, uint32_t nx, uint32_t cy, uint32_t cz)
{
    uint64_t l00, h00, l10, h10, l01, h01, l11, h11;
    mesh_row_bits(r00, occ_words, j, &l00, &h00);
    mesh_row_bits(r10, occ_words, j, &l10, &h10);
    mesh_row_bits(r01, occ_words, j, &l01, &h01);
    mesh_row_bits(r11, occ_words, j, &l11, &h11);
    const uint32_t cells = nx - 1u - 64u * j; // of this word and the row's later ones
    const uint64_t valid = cells >= 64u ? ~0ull : (1ull << cells) - 1ull;
    const uint64_t any = l00 | h00 | l10 | h10 | l01 | h01 | l11 | h11;
    const uint64_t all = l00 & h00 & l10 & h10 & l01 & h01 & l11 & h11;
    const uint64_t x_in = j ? valid : valid & ~1ull; // cx >= 1
    MeshMasks m;
    m.active = any & ~all & valid;
    m.ex = cy >= 1u && cz >= 1u ? (l00 ^ h00) & valid : 0ull;
    m.ey = cz >= 1u ? (l00 ^ l10) & x_in : 0ull;
    m.ez = cy >= 1u ? (l00 ^ l01) & x_in : 0ull;
    return m;
}

RTQ_HD inline uint32_t mesh_popc(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }

// The scratch block of a mesh extraction, laid out by block_layout: the lattice's densities (one float a point),
// its occupancy words, the mask words (MeshMasks each) and a uint32 pair per mask word -- the word's vertex and
// quad counts, which the scan replaces by the counts that precede the word.
struct MeshScratch {
    uint32_t points = 0;    // nx ny nz
    uint32_t cells = 0;     // (nx - 1)(ny - 1)(nz - 1), 0 when a dim is below 2
    uint32_t row_words = 0; // mask words per cell row: ceil((nx - 1) / 64)
    uint32_t words = 0;     // row_words (ny - 1)(nz - 1): about points / 64 (2^20 at most) unless the rows are short
    BlockLayout lay;        // parts: densities, occupancy, masks, offsets; total 0 without cells
};
enum { MESH_DENSITY = 0, MESH_OCCUPANCY = 1, MESH_MASKS = 2, MESH_OFFSETS = 3 };

// dims of a lattice that check_lattice passed
inline MeshScratch mesh_scratch(const uint32_t dims[3])
{
    MeshScratch s;
    s.points = dims[0] * dims[1] * dims[2];
    if (dims[0] < 2u || dims[1] < 2u || dims[2] < 2u) return s;
    s.cells = (dims[0] - 1u) * (dims[1] - 1u) * (dims[2] - 1u);
    s.row_words = (dims[0] - 1u + 63u) / 64u;
    s.words = s.row_words * (dims[1] - 1u) * (dims[2] - 1u);
    const size_t bytes[4] = {(size_t)s.points * 4, occupancy_bytes(dims), (size_t)s.words * kMeshMaskBytes,
                             (size_t)s.words * kMeshOffsetBytes};
    s.lay = block_layout(bytes, 4);
    return s;
}

// The grids of the passes after the density pass; a block strides over the work.  The count pass takes a mask word
// a thread and the emit pass a word a wave, both in blocks of kMeshThreads threads: light kernels without LDS, eight
// blocks a CU resident, so their grid is capped at 8 blocks a CU (or at max_blocks).  The normal pass is a field
// kernel (1024 threads, the noise tables in LDS, a block a CU) over at most `vertices` vertices: the capacity, and
// no more than the cells.
constexpr uint32_t kMeshThreads = 256u, kMeshWaves = kMeshThreads / 64u;
struct MeshPlan {
    uint32_t count_blocks = 0, emit_blocks = 0, normal_blocks = 0;
};
inline MeshPlan plan_mesh(const MeshScratch& s, uint32_t max_vertices, uint32_t max_blocks, int cus)
{
    MeshPlan p;
    const int light = 8 * (cus > 0 ? cus : 1);
    p.count_blocks = field_grid((s.words + kMeshThreads - 1u) / kMeshThreads, max_blocks, light);
    p.emit_blocks = field_grid((s.words + kMeshWaves - 1u) / kMeshWaves, max_blocks, light);
    const uint32_t v = max_vertices < s.cells ? max_vertices : s.cells;
    p.normal_blocks = field_grid((v + 1023u) / 1024u, max_blocks, cus);
    return p;
}

// ---- distance fields (rt_terrain_distance_field): exact squared lattice distance to the other state ----
//
// A separable transform to both sets, the inside points and the outside points.  The x pass (k_distrows) works on
// the occupancy words alone: for every point the distance along its row to the nearest inside point and to the
// nearest outside point, 16 bits each in one word (kDistRowFar: the row has none).  The y pass (k_distcolumns) turns
// those into the squared distance within the point's (x, y) plane, a uint32 per set (RT_DIST_FAR: none), and the z
// pass (k_distfinish) into the squared distance to the set the point itself is not in.

constexpr uint32_t kDistFar = 0xffffffffu; // RT_DIST_FAR
constexpr uint32_t kDistRowFar = 0xffffu;  // a row distance is 4095 at most
// the first version of rt_distance_options: size, flags, eye[3], max_blocks, max_cells
constexpr uint32_t kDistOptSizeV1 = 28u;
// a finite d2 is 3 * 4095^2 at most, below 7093^2: a max_cells from here on bounds nothing
constexpr uint32_t kDistMaxCells = 7093u;

struct DistanceOptions : Options {
    uint32_t max_cells = 0; // 0: unbounded
};

// `opt` is the caller's rt_distance_options (may be null: the defaults), read as far as the first version reaches.
inline int parse_distance_options(const void* opt, DistanceOptions* out, const char** why)
{
    *out = DistanceOptions{};
    if (!opt) return OK;
    if (!parse_prefix(opt, kDistOptSizeV1, out)) {
        *why = "rt_distance_options.size is smaller than the struct's first version";
        return INVALID;
    }
    if (out->flags & ~kEye) {
        *why = "rt_distance_options.flags has bits other than RT_RAYS_EYE";
        return INVALID;
    }
    std::memcpy(&out->max_cells, static_cast<const char*>(opt) + 24, 4);
    return OK;
}

// what max_cells means to the kernels: `reach`, the largest offset a column scan has to look at (the dims bound it
// anyway), and `limit2`, the largest d2 that stays finite
struct DistanceBound {
    uint32_t reach = kMaxLatticeDim, limit2 = kDistFar - 1u;
};
inline DistanceBound distance_bound(uint32_t max_cells)
{
    DistanceBound b;
    if (max_cells && max_cells < kDistMaxCells) {
        b.reach = max_cells;
        b.limit2 = max_cells * max_cells;
    }
    return b;
}

// distance is defined on an isotropic lattice only: |sx| == |sy| == |sz| != 0 (a lattice check_lattice passed)
inline bool distance_isotropic(const float spacing[3])
{
    const float a = spacing[0] < 0.0f ? -spacing[0] : spacing[0], b = spacing[1] < 0.0f ? -spacing[1] : spacing[1],
                c = spacing[2] < 0.0f ? -spacing[2] : spacing[2];
    return a != 0.0f && a == b && a == c;
}

// The part of an occupancy row that one of its words, w, needs: the word's inside and outside points (the padding
// bits beyond nx cleared in both) and, per set, the distance from the word's first point, 32 w, back to the set's
// nearest point in an earlier word and from the word's bit 31, point 32 w + 31, on to its nearest point in a later
// word (kDistRowFar: none).
struct DistRowWord {
    uint32_t bits[2];          // [0] inside points, [1] outside points
    uint32_t left[2], right[2];
};

RTQ_HD inline uint32_t dist_clz(uint32_t m) { return (uint32_t)__builtin_clz(m); } // m != 0
RTQ_HD inline uint32_t dist_ctz(uint32_t m) { return (uint32_t)__builtin_ctz(m); } // m != 0

// the points of word w of a row of nx points (32 w < nx) that exist
RTQ_HD inline uint32_t dist_valid_bits(uint32_t nx, uint32_t w)
{
    const uint32_t left = nx - 32u * w;
    return left >= 32u ? 0xffffffffu : (1u << left) - 1u;
}

// row: the ceil(nx / 32) occupancy words of one point row, whatever their padding bits hold; 32 w < nx.  Both word
// loops are bounded by the row's words.
RTQ_HD inline DistRowWord dist_row_word(const uint32_t* row, uint32_t nx, uint32_t w)
{
    const uint32_t words = (nx + 31u) / 32u;
    DistRowWord r;
    for (uint32_t set = 0; set < 2u; ++set) {
        const uint32_t flip = set ? 0xffffffffu : 0u;
        r.bits[set] = (row[w] ^ flip) & dist_valid_bits(nx, w);
        r.left[set] = r.right[set] = kDistRowFar;
        for (uint32_t v = w; v-- > 0u;) {
            const uint32_t m = row[v] ^ flip; // (an earlier word has no padding)
            if (m) {
                r.left[set] = 32u * (w - v) - 31u + dist_clz(m);
                break;
            }
        }
        for (uint32_t v = w + 1u; v < words; ++v) {
            const uint32_t m = (row[v] ^ flip) & dist_valid_bits(nx, v);
            if (m) {
                r.right[set] = 32u * (v - w) - 31u + dist_ctz(m);
                break;
            }
        }
    }
    return r;
}

// the distance of the word's point b (32 w + b < nx) to the nearest point of `set` in its row, or kDistRowFar
RTQ_HD inline uint32_t dist_row_point(const DistRowWord& r, uint32_t set, uint32_t b)
{
    const uint32_t below = r.bits[set] & (0xffffffffu >> (31u - b)), above = r.bits[set] & (0xffffffffu << b);
    uint32_t dl = kDistRowFar, dr = kDistRowFar;
    if (below) dl = b - (31u - dist_clz(below));
    else if (r.left[set] != kDistRowFar) dl = r.left[set] + b;
    if (above) dr = dist_ctz(above) - b;
    else if (r.right[set] != kDistRowFar) dr = r.right[set] + (31u - b);
    return dl < dr ? dl : dr;
}

// what k_distrows stores for a point: the distance to the nearest inside point in the low half, to the nearest
// outside point in the high half
RTQ_HD inline uint32_t dist_row_pack(const DistRowWord& r, uint32_t b)
{
    return dist_row_point(r, 0u, b) | (dist_row_point(r, 1u, b) << 16);
}

// The row arithmetic of the x pass for one word: in[b] / out[b] for every point 32 w + b < nx (the other entries
// are left alone).
inline void dist_row(const uint32_t* row, uint32_t nx, uint32_t w, uint16_t in[32], uint16_t out[32])
{
    const DistRowWord r = dist_row_word(row, nx, w);
    for (uint32_t b = 0; b < 32u && 32u * w + b < nx; ++b) {
        const uint32_t p = dist_row_pack(r, b);
        in[b] = (uint16_t)(p & 0xffffu);
        out[b] = (uint16_t)(p >> 16);
    }
}

// The scratch block of a distance field, laid out by block_layout: the lattice's occupancy words (used when the
// terrain's own occupancy is asked for), the x pass's word per point, and the y pass's two uint32 planes (inside
// set, outside set).
struct DistanceScratch {
    uint32_t points = 0; // nx ny nz
    BlockLayout lay;     // parts: occupancy, rows, planes; total 0 without points
};
enum { DIST_OCCUPANCY = 0, DIST_ROWS = 1, DIST_PLANES = 2 };

// dims of a lattice that check_lattice passed
inline DistanceScratch distance_scratch(const uint32_t dims[3])
{
    DistanceScratch s;
    s.points = dims[0] * dims[1] * dims[2];
    if (s.points == 0) return s;
    const size_t bytes[3] = {occupancy_bytes(dims), (size_t)s.points * 4, (size_t)s.points * 8};
    s.lay = block_layout(bytes, 3);
    return s;
}

// The grid of the three passes: a thread a point in blocks of kDistThreads threads, a block striding over tiles of
// kDistThreads consecutive points.  Light kernels without LDS, eight blocks a CU resident, so the grid is capped at
// 8 blocks a CU (or at max_blocks).
constexpr uint32_t kDistThreads = 256u;
struct DistancePlan {
    uint32_t blocks = 0;
};
inline DistancePlan plan_distance(uint32_t points, uint32_t max_blocks, int cus)
{
    DistancePlan p;
    p.blocks = field_grid((points + kDistThreads - 1u) / kDistThreads, max_blocks, 8 * (cus > 0 ? cus : 1));
    return p;
}

// ---- path fields (rt_terrain_path_field): the cheapest 3-4-5 chamfer path from seeds through passable points ----
//
// The cost is the least fixed point of cost(p) = min(cost(p), cost(q) + w(p - q)) over the 26 neighbours q, so the
// kernels may relax in any order.  k_pathinit forms the passable words (not blocked, and with a clearance d2 far),
// sets every cost far and clears the tile flags and counters; k_pathseed sets the passable seeds to 0 and marks
// their tiles; each k_pathsweep launch relaxes the tiles marked for it to their local fixed point in LDS and marks
// the neighbours of the tiles that changed for the next launch; k_pathfinish writes the flow, counts the reached
// points and writes the status.

constexpr uint32_t kPathFar = 0xffffffffu; // RT_PATH_FAR
constexpr uint32_t kPathNone = 255u;       // RT_PATH_NONE
constexpr uint32_t kPathStay = 13u;        // the move code of (0, 0, 0)
// the first version of rt_path_options: size, flags, eye[3], max_blocks, clearance_cells, max_cost, max_sweeps
constexpr uint32_t kPathOptSizeV1 = 36u;
constexpr uint32_t kPathMaxClearance = 4095u;
constexpr uint32_t kPathMaxSeeds = 1u << 26;
constexpr uint32_t kPathMaxSweeps = 4096u; // of the device form
constexpr uint32_t kPathBatch = 16u;       // sweeps between two looks of the host form at the active counter

struct PathOptions : Options {
    uint32_t clearance_cells = 0, max_cost = 0, max_sweeps = 0;
};

// `opt` is the caller's rt_path_options (may be null: the defaults), read as far as the first version reaches.
inline int parse_path_options(const void* opt, PathOptions* out, const char** why)
{
    *out = PathOptions{};
    if (!opt) return OK;
    if (!parse_prefix(opt, kPathOptSizeV1, out)) {
        *why = "rt_path_options.size is smaller than the struct's first version";
        return INVALID;
    }
    if (out->flags & ~kEye) {
        *why = "rt_path_options.flags has bits other than RT_RAYS_EYE";
        return INVALID;
    }
    const char* p = static_cast<const char*>(opt);
    std::memcpy(&out->clearance_cells, p + 24, 4);
    std::memcpy(&out->max_cost, p + 28, 4);
    std::memcpy(&out->max_sweeps, p + 32, 4);
    if (out->clearance_cells > kPathMaxClearance) {
        *why = "rt_path_options.clearance_cells is above 4095";
        return INVALID;
    }
    return OK;
}

// the largest cost that is stored: max_cost, or without one everything below the far value (a finite cost is below
// 5 * 2^26, far below it)
inline uint32_t path_limit(uint32_t max_cost) { return max_cost ? max_cost : kPathFar - 1u; }

// The moves: code c = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1), 0..26, 13 is "stay".
RTQ_HD inline void path_move(uint32_t c, int* dx, int* dy, int* dz)
{
    *dx = (int)(c % 3u) - 1;
    *dy = (int)(c / 3u % 3u) - 1;
    *dz = (int)(c / 9u) - 1;
}
// 3 for a face move, 4 for an edge move, 5 for a corner move (the 3-4-5 chamfer, thirds of a cell); 0 for "stay"
RTQ_HD inline uint32_t path_weight(int dx, int dy, int dz)
{
    const uint32_t k = (uint32_t)(dx != 0) + (uint32_t)(dy != 0) + (uint32_t)(dz != 0);
    return k ? 2u + k : 0u;
}

// The flow of a point of finite cost `cost` > 0 at (ix, iy, iz): the smallest move code c whose neighbour q is a
// lattice point with cost(q) + w(c) == cost; kPathNone when there is none (an unconverged field).  at(i): the cost
// of point i.  The far value is never added to.
template <class At>
RTQ_HD inline uint32_t path_flow(At at, const uint32_t dims[3], uint32_t ix, uint32_t iy, uint32_t iz, uint32_t cost)
{
    for (uint32_t c = 0; c < 27u; ++c) {
        if (c == kPathStay) continue;
        int dx, dy, dz;
        path_move(c, &dx, &dy, &dz);
        const uint32_t qx = ix + (uint32_t)dx, qy = iy + (uint32_t)dy, qz = iz + (uint32_t)dz; // below 0 wraps: >= dim
        if (qx >= dims[0] || qy >= dims[1] || qz >= dims[2]) continue;
        const uint32_t v = at((qz * dims[1] + qy) * dims[0] + qx);
        if (v != kPathFar && v + path_weight(dx, dy, dz) == cost) return c;
    }
    return kPathNone;
}

// The tiles: 32 x 4 x 4 points, an x run of a tile is one occupancy word.  Tile index (tz * ty_n + ty) * tx_n + tx.
constexpr uint32_t kPathTileX = 32u, kPathTileY = 4u, kPathTileZ = 4u;
constexpr uint32_t kPathTilePoints = kPathTileX * kPathTileY * kPathTileZ; // a thread a point
// the tile with its one-point halo, as the sweep holds it in LDS
constexpr uint32_t kPathHaloX = kPathTileX + 2u, kPathHaloY = kPathTileY + 2u, kPathHaloZ = kPathTileZ + 2u;
constexpr uint32_t kPathHaloPoints = kPathHaloX * kPathHaloY * kPathHaloZ;

struct PathTiles {
    uint32_t n[3] = {0, 0, 0};
    uint32_t total = 0;
};
// dims all >= 1
RTQ_HD inline PathTiles path_tiles(const uint32_t dims[3])
{
    PathTiles t;
    t.n[0] = (dims[0] + kPathTileX - 1u) / kPathTileX;
    t.n[1] = (dims[1] + kPathTileY - 1u) / kPathTileY;
    t.n[2] = (dims[2] + kPathTileZ - 1u) / kPathTileZ;
    t.total = t.n[0] * t.n[1] * t.n[2];
    return t;
}
RTQ_HD inline uint32_t path_tile_of(const PathTiles& t, uint32_t ix, uint32_t iy, uint32_t iz)
{
    return ((iz / kPathTileZ) * t.n[1] + iy / kPathTileY) * t.n[0] + ix / kPathTileX;
}

// the counters of a path field, the last part of its scratch block (uint32 each)
enum {
    PATH_CNT_ACTIVE = 0, // [3]: sweep k reads [k % 3], the tiles marked for it, counts into [(k + 1) % 3], clears [(k + 2) % 3]
    PATH_CNT_WORKED = 3, // [2]: sweep k sets [k & 1] once a tile of it changed, and clears [(k + 1) & 1]
    PATH_CNT_SWEEPS = 5, // sweeps in which a tile changed
    PATH_CNT_VISITS = 6, // active tiles visited
    PATH_CNT_WORDS = 16
};

// The scratch block of a path field, laid out by block_layout: the lattice's occupancy words (used when the
// terrain's own occupancy is asked for); with a clearance the distance field's scratch block followed by its d2, a
// uint32 a point; the passable words; the two tile flag arrays, a uint32 a tile each; the counters.
struct PathScratch {
    uint32_t points = 0;
    PathTiles tiles;
    size_t d2_offset = 0; // of d2 within the PATH_DISTANCE part
    BlockLayout lay;      // total 0 without points
};
enum { PATH_OCCUPANCY = 0, PATH_DISTANCE = 1, PATH_PASSABLE = 2, PATH_FLAGS = 3, PATH_COUNTERS = 4 };

// dims of a lattice that check_lattice passed
inline PathScratch path_scratch(const uint32_t dims[3], uint32_t clearance_cells)
{
    PathScratch s;
    s.points = dims[0] * dims[1] * dims[2];
    if (s.points == 0) return s;
    s.tiles = path_tiles(dims);
    s.d2_offset = clearance_cells ? distance_scratch(dims).lay.total : 0;
    const size_t bytes[5] = {occupancy_bytes(dims), clearance_cells ? s.d2_offset + (size_t)s.points * 4 : 0,
                             occupancy_bytes(dims), (size_t)s.tiles.total * 8, (size_t)PATH_CNT_WORDS * 4};
    s.lay = block_layout(bytes, 5);
    return s;
}

// The grids: the sweep a block of kPathTilePoints threads a tile, striding over the tile flags, four blocks a CU
// resident; the point passes (init, finish) as the distance passes.
struct PathPlan {
    uint32_t sweep_blocks = 0, point_blocks = 0;
};
inline PathPlan plan_path(const PathScratch& s, uint32_t max_blocks, int cus)
{
    PathPlan p;
    p.sweep_blocks = field_grid(s.tiles.total, max_blocks, 4 * (cus > 0 ? cus : 1));
    p.point_blocks = plan_distance(s.points, max_blocks, cus).blocks;
    return p;
}

// ---- visibility fields (rt_terrain_visibility_field): line of sight to observers on the occupancy bits ----
//
// One kernel, k_visibility, a thread a point: for each observer the walk of include/frosttrace.h from the point
// towards the observer (the rule is symmetric) or along the direction, over the occupancy words alone.  The walk
// is VisWalk and vis_sees below, host and device, so tests/tools/visquery_check.cpp runs the code the kernel runs.

// the first version of rt_visibility_options: size, flags, eye[3], max_blocks, max_range
constexpr uint32_t kVisOptSizeV1 = 28u;
constexpr uint32_t kVisMaxObservers = 32u;
constexpr int32_t kVisMaxDirection = 4095;               // of a direction's components, in magnitude
constexpr uint32_t kVisMaxRange = 2u * (kMaxLatticeDim - 1u); // no two lattice points are farther apart
enum { VIS_POINT = 0, VIS_DIRECTION = 1 };                // an observer's kind

struct VisibilityOptions : Options {
    uint32_t max_range = 0; // 0: unbounded
};

// `opt` is the caller's rt_visibility_options (may be null: the defaults), read as far as the first version reaches.
inline int parse_visibility_options(const void* opt, VisibilityOptions* out, const char** why)
{
    *out = VisibilityOptions{};
    if (!opt) return OK;
    if (!parse_prefix(opt, kVisOptSizeV1, out)) {
        *why = "rt_visibility_options.size is smaller than the struct's first version";
        return INVALID;
    }
    if (out->flags & ~kEye) {
        *why = "rt_visibility_options.flags has bits other than RT_RAYS_EYE";
        return INVALID;
    }
    std::memcpy(&out->max_range, static_cast<const char*>(opt) + 24, 4);
    if (out->max_range > kVisMaxRange) {
        *why = "rt_visibility_options.max_range is above 8190";
        return INVALID;
    }
    return OK;
}

// an observer record x, y, z, kind that the definition admits on a lattice of these dims
RTQ_HD inline bool vis_observer_valid(const int32_t o[4], const uint32_t dims[3])
{
    if (o[3] == VIS_POINT) // (a negative coordinate wraps: >= dim)
        return (uint32_t)o[0] < dims[0] && (uint32_t)o[1] < dims[1] && (uint32_t)o[2] < dims[2];
    if (o[3] != VIS_DIRECTION) return false;
    for (int i = 0; i < 3; ++i)
        if (o[i] > kVisMaxDirection || o[i] < -kVisMaxDirection) return false;
    return (o[0] | o[1] | o[2]) != 0;
}

// The crossing events of a walk whose axis i crosses a boundary at t = (2 k + 1) / (2 n[i]), k = 0, 1, ...
// (n[i] = |d_i| or |u_i|, 4095 at most; 0: the axis never crosses).  With a_i = 2 k_i + 1 the next crossing of axis
// i, t_i <= t_j is a_i n[j] <= a_j n[i]: the walk holds the three differences a_i n[j] - a_j n[i] and moves them by
// additions when an axis steps, so an event costs no multiply.  An axis with n[i] == 0 compares later than every
// axis that crosses (its difference keeps the sign of a n[j] > 0), and so does an axis that has taken all n[i] steps
// of a point walk (its t is above 1), so neither needs a case of its own.  While no axis has taken more than 4096
// steps every difference is below 8193 * 4095 < 2^25 in magnitude.
struct VisWalk {
    int32_t n[3];
    int32_t dxy, dxz, dyz;
    RTQ_HD void start(int32_t nx, int32_t ny, int32_t nz)
    {
        n[0] = nx, n[1] = ny, n[2] = nz;
        dxy = ny - nx, dxz = nz - nx, dyz = nz - ny;
    }
    // the next event: the axes that cross at the earliest time, x 1, y 2, z 4 (one at least while an n is not 0)
    RTQ_HD uint32_t step()
    {
        const bool sx = dxy <= 0 && dxz <= 0, sy = dxy >= 0 && dyz <= 0, sz = dxz >= 0 && dyz >= 0;
        if (sx) dxy += 2 * n[1], dxz += 2 * n[2];
        if (sy) dxy -= 2 * n[0], dyz += 2 * n[2];
        if (sz) dxz -= 2 * n[0], dyz -= 2 * n[1];
        return (uint32_t)sx | (uint32_t)sy << 1 | (uint32_t)sz << 2;
    }
};

// The occupancy words as one run of bits: point (ix, iy, iz) is bit (iz ny + iy) row_bits + ix, word bit >> 5, bit
// bit & 31 of it; below 2^31 for a lattice of 2^26 points.  A step along x, y, z moves it by 1, row_bits, plane_bits.
struct VisGrid {
    uint32_t nx, ny, nz;
    uint32_t row_bits, plane_bits;
};
RTQ_HD inline VisGrid vis_grid(const uint32_t dims[3])
{
    VisGrid g;
    g.nx = dims[0], g.ny = dims[1], g.nz = dims[2];
    g.row_bits = (dims[0] + 31u) / 32u * 32u;
    g.plane_bits = g.row_bits * dims[1];
    return g;
}

// Whether the lattice point p = (ix, iy, iz) sees the valid observer o (vis_observer_valid).  blocked(bit): the
// occupancy bit of the point at that bit index; it is asked for cells of the lattice between the ends only, never
// for p or a point observer.  range2: max_range^2, 0 for none.  The walk starts at p.  A point walk ends at o after
// |d_x| + |d_y| + |d_z| axis steps, a directional walk where it leaves the lattice, so the loop runs nx + ny + nz
// times at most.
template <class Blocked>
RTQ_HD inline bool vis_sees(Blocked blocked, const VisGrid& g, uint32_t ix, uint32_t iy, uint32_t iz, const int32_t o[4],
                            uint32_t range2)
{
    const bool directional = o[3] == VIS_DIRECTION;
    const int32_t dx = directional ? o[0] : o[0] - (int32_t)ix, dy = directional ? o[1] : o[1] - (int32_t)iy,
                  dz = directional ? o[2] : o[2] - (int32_t)iz;
    const int32_t nx = dx < 0 ? -dx : dx, ny = dy < 0 ? -dy : dy, nz = dz < 0 ? -dz : dz;
    int32_t left = 0x7fffffff; // axis steps to the observer; a direction has no end
    if (!directional) {
        if (range2 && (uint32_t)(dx * dx + dy * dy + dz * dz) > range2) return false;
        left = nx + ny + nz;
        if (left == 0) return true;
    }
    // (a step below 0 wraps, and a negative bit step is its two's complement)
    const uint32_t sx = dx < 0 ? ~0u : 1u, sy = dy < 0 ? ~0u : 1u, sz = dz < 0 ? ~0u : 1u;
    const uint32_t bx = sx, by = dy < 0 ? 0u - g.row_bits : g.row_bits, bz = dz < 0 ? 0u - g.plane_bits : g.plane_bits;
    uint32_t x = ix, y = iy, z = iz, bit = (iz * g.ny + iy) * g.row_bits + ix;
    VisWalk w;
    w.start(nx, ny, nz);
    for (;;) {
        const uint32_t axes = w.step();
        if (axes & 1u) x += sx, bit += bx;
        if (axes & 2u) y += sy, bit += by;
        if (axes & 4u) z += sz, bit += bz;
        if (x >= g.nx || y >= g.ny || z >= g.nz) return true; // left the lattice unblocked (a point walk never does)
        if (!directional) {
            left -= (int32_t)((axes & 1u) + (axes >> 1 & 1u) + (axes >> 2));
            if (left <= 0) return true; // at the observer, which is not tested
        } else if (range2) {
            const int32_t ex = (int32_t)(x - ix), ey = (int32_t)(y - iy), ez = (int32_t)(z - iz);
            if ((uint32_t)(ex * ex + ey * ey + ez * ez) > range2) return true;
        }
        if (blocked(bit)) return false;
    }
}

// the occupancy bit at a bit index of vis_grid's numbering
RTQ_HD inline bool vis_bit(const uint32_t* occupancy, uint32_t bit) { return (occupancy[bit >> 5] >> (bit & 31u)) & 1u; }

// The scratch block of a visibility field, laid out by block_layout: the lattice's occupancy words (used when the
// terrain's own occupancy is asked for) and the counters, VIS_CNT_WORDS uint32, of which the first four are the
// host form's status words.
constexpr uint32_t VIS_CNT_WORDS = 16u;
struct VisibilityScratch {
    uint32_t points = 0; // nx ny nz
    BlockLayout lay;     // parts: occupancy, counters; total 0 without points
};
enum { VIS_OCCUPANCY = 0, VIS_COUNTERS = 1 };

// dims of a lattice that check_lattice passed
inline VisibilityScratch visibility_scratch(const uint32_t dims[3])
{
    VisibilityScratch s;
    s.points = dims[0] * dims[1] * dims[2];
    if (s.points == 0) return s;
    const size_t bytes[2] = {occupancy_bytes(dims), (size_t)VIS_CNT_WORDS * 4};
    s.lay = block_layout(bytes, 2);
    return s;
}

// The grid: a thread a point in blocks of kDistThreads threads striding over the points, as the distance passes;
// no LDS, eight blocks a CU resident.
struct VisibilityPlan {
    uint32_t blocks = 0;
};
inline VisibilityPlan plan_visibility(uint32_t points, uint32_t max_blocks, int cus)
{
    VisibilityPlan p;
    p.blocks = plan_distance(points, max_blocks, cus).blocks;
    return p;
}

// ---- region fields (rt_terrain_region_field): the connected regions of the free or of the blocked points ----
//
// A union-find over the path field's tiles in a fixed number of launches, with `label` itself as the forest: word p
// holds the index of another point of p's region that is not above p (its parent), p itself at a root, kRegionNone
// at a non-member.  k_regionlocal forms the member words and labels every tile on its own in LDS, so label[p] is
// the tile-local root; k_regionmerge unites the trees over every link that leaves a tile; k_regionflatten stores
// find(p) in every word and counts the points of every root; k_regionfinish writes the sizes and the status.
// region_find and region_unite below are what the kernels run and what tests/tools/regionquery_check.cpp runs.
//
// The invariant everything rests on: a forest word only ever falls, and only to the index of a point of the same
// final region.  A read that returns an older value therefore returns an older ancestor of the same tree: it costs
// steps, never correctness.

constexpr uint32_t kRegionNone = 0xffffffffu; // RT_REGION_NONE
// the first version of rt_region_options: size, flags, eye[3], max_blocks, clearance_cells, connectivity, state
constexpr uint32_t kRegionOptSizeV1 = 36u;
enum { REGION_FREE = 0, REGION_SOLID = 1 };

struct RegionOptions : Options {
    uint32_t clearance_cells = 0, connectivity = 26, state = REGION_FREE; // (connectivity 0 is read as 26)
};

// `opt` is the caller's rt_region_options (may be null: the defaults), read as far as the first version reaches.
inline int parse_region_options(const void* opt, RegionOptions* out, const char** why)
{
    *out = RegionOptions{};
    if (!opt) return OK;
    if (!parse_prefix(opt, kRegionOptSizeV1, out)) {
        *why = "rt_region_options.size is smaller than the struct's first version";
        return INVALID;
    }
    if (out->flags & ~kEye) {
        *why = "rt_region_options.flags has bits other than RT_RAYS_EYE";
        return INVALID;
    }
    const char* p = static_cast<const char*>(opt);
    std::memcpy(&out->clearance_cells, p + 24, 4);
    std::memcpy(&out->connectivity, p + 28, 4);
    std::memcpy(&out->state, p + 32, 4);
    if (out->clearance_cells > kPathMaxClearance) {
        *why = "rt_region_options.clearance_cells is above 4095";
        return INVALID;
    }
    if (out->connectivity == 0u) out->connectivity = 26u;
    if (out->connectivity != 6u && out->connectivity != 26u) {
        *why = "rt_region_options.connectivity is not 0, 6 or 26";
        return INVALID;
    }
    if (out->state > (uint32_t)REGION_SOLID) {
        *why = "rt_region_options.state is not 0 (free) or 1 (solid)";
        return INVALID;
    }
    if (out->state == (uint32_t)REGION_SOLID && out->clearance_cells) {
        *why = "rt_region_options.clearance_cells must be 0 with state 1 (solid)";
        return INVALID;
    }
    return OK;
}

// The backward moves: the moves whose neighbour has the smaller linear index, so that every link is taken once, from
// its larger end.  Of the 26 moves they are the path field's codes 0..12 (the codes below "stay"), of the 6 face
// moves the codes 4, 10 and 12: (0, 0, -1), (0, -1, 0), (-1, 0, 0).  With their negations they are all the moves.
RTQ_HD inline uint32_t region_backward_count(uint32_t connectivity) { return connectivity == 6u ? 3u : 13u; }
RTQ_HD inline void region_backward_move(uint32_t connectivity, uint32_t k, int* dx, int* dy, int* dz)
{
    path_move(connectivity == 6u ? (k == 0u ? 4u : k == 1u ? 10u : 12u) : k, dx, dy, dz);
}

// The root of x's tree, with path halving.  A: the access policy of the forest words, with
//   uint32_t load(uint32_t i)              the word of point i (on the device a relaxed load at agent scope),
//   uint32_t fall(uint32_t i, uint32_t v)  word i = min(word i, v), the word's value before (on the device atomicMin),
//   void fault()                           a fail-safe bound ended a loop.
// x is a member.  Variant: x, which strictly falls (a parent is below its child); the bound, the lattice's points at
// most, can therefore not be hit by a forest; if it is hit the loop ends all the same.
template <class A>
RTQ_HD inline uint32_t region_find(A& a, uint32_t x, uint32_t bound)
{
    for (uint32_t k = 0; k < bound; ++k) {
        const uint32_t p = a.load(x);
        if (p >= x) return x; // a root (a forest holds no word above its index)
        const uint32_t g = a.load(p);
        if (g >= p) return p;
        a.fall(x, g); // halving: g is an ancestor of x, below the word's value; another thread may have lowered it more
        x = g;
    }
    a.fault();
    return x;
}

// Unite the trees of the members x and y, lock-free: find both roots, let the larger root's word fall to the
// smaller root, and if the word had already fallen (another thread got there first, or the root that was read was
// an older value) go on from the value it held: that is a point of the same tree below the root.  Variant: the
// larger of the two roots, which strictly falls from one round to the next; the bound as in region_find.
template <class A>
RTQ_HD inline void region_unite(A& a, uint32_t x, uint32_t y, uint32_t bound)
{
    for (uint32_t k = 0; k < bound; ++k) {
        x = region_find(a, x, bound);
        y = region_find(a, y, bound);
        if (x == y) return;
        if (x < y) {
            const uint32_t t = x;
            x = y;
            y = t;
        }
        const uint32_t old = a.fall(x, y); // x > y
        if (old >= x) return;              // x was a root and hangs below y now
        x = old;
    }
    a.fault();
}

// the forest as a plain array: the stand-alone checker's policy (one thread)
struct RegionHostForest {
    uint32_t* w;
    uint32_t faults = 0;
    uint32_t load(uint32_t i) { return w[i]; }
    uint32_t fall(uint32_t i, uint32_t v)
    {
        const uint32_t old = w[i];
        if (v < old) w[i] = v;
        return old;
    }
    void fault() { ++faults; }
};

// the counters of a region field, the last part of its scratch block (uint32 each)
enum {
    REGION_CNT_FAULT = 0,  // loops that a fail-safe bound ended: status[0] is 1 while this is 0
    REGION_CNT_STATUS = 8, // [4]: the host form's status words
    REGION_CNT_WORDS = 16
};

// The scratch block of a region field, laid out by block_layout: the lattice's occupancy words (used when the
// terrain's own occupancy is asked for); with a clearance the distance field's scratch block followed by its d2, a
// uint32 a point; the member words; the region counts, a uint32 a point (the count of a region at its root's
// index); the counters.
struct RegionScratch {
    uint32_t points = 0;
    PathTiles tiles;
    size_t d2_offset = 0; // of d2 within the REGION_DISTANCE part
    BlockLayout lay;      // total 0 without points
};
enum { REGION_OCCUPANCY = 0, REGION_DISTANCE = 1, REGION_MEMBER = 2, REGION_COUNTS = 3, REGION_COUNTERS = 4 };

// dims of a lattice that check_lattice passed
inline RegionScratch region_scratch(const uint32_t dims[3], uint32_t clearance_cells)
{
    RegionScratch s;
    s.points = dims[0] * dims[1] * dims[2];
    if (s.points == 0) return s;
    s.tiles = path_tiles(dims);
    s.d2_offset = clearance_cells ? distance_scratch(dims).lay.total : 0;
    const size_t bytes[5] = {occupancy_bytes(dims), clearance_cells ? s.d2_offset + (size_t)s.points * 4 : 0,
                             occupancy_bytes(dims), (size_t)s.points * 4, (size_t)REGION_CNT_WORDS * 4};
    s.lay = block_layout(bytes, 5);
    return s;
}

// The grids: k_regionlocal and k_regionflatten a block of kPathTilePoints threads a tile, striding over the tiles,
// four blocks a CU resident, as the path sweep; k_regionmerge and k_regionfinish a thread a point as the distance
// passes.
struct RegionPlan {
    uint32_t tile_blocks = 0, point_blocks = 0;
};
inline RegionPlan plan_region(const RegionScratch& s, uint32_t max_blocks, int cus)
{
    RegionPlan p;
    p.tile_blocks = field_grid(s.tiles.total, max_blocks, 4 * (cus > 0 ? cus : 1));
    p.point_blocks = plan_distance(s.points, max_blocks, cus).blocks;
    return p;
}

} // namespace rtq
