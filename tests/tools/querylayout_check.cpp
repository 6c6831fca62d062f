// Stand-alone check of what the query families share in gpgpuraytrace_amd/csrc/rt_rayquery.h: the layout of the
// host forms' device block (block_layout with the per-element strides, for the part lists of the five host forms)
// and the one option-prefix parser behind parse_options, parse_surface_options and parse_field_options (never read
// past the caller's size).
// Built with -fsanitize=address,undefined by tests/test_ray_query_host.py; its own main.
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "rt_rayquery.h"

#define CHECK(x)                                                           \
    do {                                                                   \
        if (!(x)) {                                                        \
            std::printf("querylayout_check FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static_assert(sizeof(size_t) == 8, "the block of 2^26 rays is beyond 32 bits");
static_assert(std::is_same<decltype(rtq::kRayBytes), const size_t>::value, "strides multiply in size_t");
static_assert(rtq::kRayBytes == 32 && rtq::kPointBytes == 16 && rtq::kRayResultBytes == 16 &&
                  rtq::kSurfResultBytes == 32 && rtq::kPixelBytes == 4 && rtq::kStepsBytes == 4 &&
                  rtq::kShadeStepsBytes == 8,
              "the kernels' strides");

// a part list as a host form writes it, and the element sizes it must come to (64-bit, computed apart)
struct Form {
    std::vector<size_t> bytes;
    std::vector<uint64_t> want;
};

// every property of the layout of one part list
static int check_layout(const Form& f)
{
    const int parts = (int)f.bytes.size();
    CHECK(parts >= 1 && parts <= rtq::kBlockParts && f.want.size() == f.bytes.size());
    for (int i = 0; i < parts; ++i) CHECK((uint64_t)f.bytes[i] == f.want[i]); // no 32-bit product on the way
    const rtq::BlockLayout l = rtq::block_layout(f.bytes.data(), parts);
    uint64_t end = 0, sum = 0; // the end of the last present part, the present parts rounded up to 16
    for (int i = 0; i < parts; ++i) {
        if (f.bytes[i] == 0) continue;
        CHECK(l.offset[i] % 16 == 0);
        CHECK(l.offset[i] >= end); // in order, no overlap
        end = (uint64_t)l.offset[i] + f.want[i];
        sum += (f.want[i] + 15) / 16 * 16;
    }
    CHECK(l.total >= end && l.total == sum);
    // an absent part adds nothing: the layout of the present parts alone is the same
    std::vector<size_t> present;
    std::vector<int> index;
    for (int i = 0; i < parts; ++i)
        if (f.bytes[i]) {
            present.push_back(f.bytes[i]);
            index.push_back(i);
        }
    const rtq::BlockLayout p = rtq::block_layout(present.data(), (int)present.size());
    CHECK(p.total == l.total);
    for (size_t k = 0; k < present.size(); ++k) CHECK(p.offset[k] == l.offset[index[k]]);
    return 0;
}

// the option block of a family: `v1` bytes on the heap at their exact size; parse(block) -> the code, and through
// *o the prefix read
template <class Opt, class Parse>
static int check_prefix(uint32_t v1, Parse parse)
{
    const char* why = "";
    Opt o;
    CHECK(parse(nullptr, &o, &why) == rtq::OK && o.flags == 0 && o.max_blocks == 0 && o.eye[0] == 0.0f);
    for (uint32_t size : {0u, 4u, 8u, v1 - 1u}) { // too short: only the size word is read
        std::vector<unsigned char> small(4);
        std::memcpy(small.data(), &size, 4);
        why = "";
        CHECK(parse(small.data(), &o, &why) == rtq::INVALID && why[0] != 0);
        CHECK(o.flags == 0 && o.max_blocks == 0); // the defaults stay
    }
    for (uint32_t size : {v1, v1 + 4u, 4096u}) { // a later, longer version: the buffer stays at the first one's size
        std::vector<unsigned char> buf(v1, 0);
        const uint32_t flags = rtq::kEye, max_blocks = 7;
        const float eye[3] = {1.5f, -2.0f, 3.25f};
        std::memcpy(buf.data(), &size, 4);
        std::memcpy(buf.data() + 4, &flags, 4);
        std::memcpy(buf.data() + 8, eye, 12);
        std::memcpy(buf.data() + 20, &max_blocks, 4);
        CHECK(parse(buf.data(), &o, &why) == rtq::OK);
        CHECK(o.flags == rtq::kEye && o.eye[0] == 1.5f && o.eye[1] == -2.0f && o.eye[2] == 3.25f && o.max_blocks == 7);
    }
    return 0;
}

int main()
{
    using namespace rtq;
    static_assert(std::is_same<FieldOptions, Options>::value, "one type for the prefix");
    static_assert(std::is_base_of<Options, SurfOptions>::value, "the surface options begin with the prefix");

    // nothing, and one part
    {
        const BlockLayout none = block_layout(nullptr, 0);
        CHECK(none.total == 0);
        const size_t one[] = {5};
        const BlockLayout l = block_layout(one, 1);
        CHECK(l.offset[0] == 0 && l.total == 16);
    }

    // the five host forms' part lists, for every combination of their optional parts
    for (uint32_t n : {1u, 3u, 1023u, 1025u, 1u << 26}) {
        const uint64_t N = n;
        for (int steps = 0; steps < 2; ++steps) {
            // rt_terrain_trace_rays: rays, results, steps
            if (check_layout({{n * kRayBytes, n * kRayResultBytes, steps ? n * kStepsBytes : 0},
                              {N * 32, N * 16, steps ? N * 4 : 0}}))
                return 1;
            // rt_terrain_trace_surface: rays, results, steps
            if (check_layout({{n * kRayBytes, n * kSurfResultBytes, steps ? n * kStepsBytes : 0},
                              {N * 32, N * 32, steps ? N * 4 : 0}}))
                return 1;
            // rt_terrain_shade_rays: rays, results, pixels, steps (two counts a ray)
            for (int res = 0; res < 2; ++res)
                for (int px = 0; px < 2; ++px)
                    if (check_layout({{n * kRayBytes, res ? n * kSurfResultBytes : 0, px ? n * kPixelBytes : 0,
                                       steps ? n * kShadeStepsBytes : 0},
                                      {N * 32, res ? N * 32 : 0, px ? N * 4 : 0, steps ? N * 8 : 0}}))
                        return 1;
        }
        for (uint32_t flags : {0u, kFieldNormal, kEye | kFieldNormal}) {
            const uint64_t stride = (flags & kFieldNormal) ? 16 : 4;
            CHECK(field_stride(flags) == stride);
            // rt_terrain_sample_field: points, results
            if (check_layout({{n * kPointBytes, n * field_stride(flags)}, {N * 16, N * stride}})) return 1;
            // rt_terrain_sample_lattice: results, occupancy; n points as rows of at most 4096
            const uint32_t big[3] = {4096, 4096, 4}, row[3] = {n, 1, 1};
            const uint32_t* dims = n > kMaxLatticeDim ? big : row;
            CHECK((uint64_t)dims[0] * dims[1] * dims[2] == N);
            const uint64_t occ = (uint64_t)((dims[0] + 31) / 32) * dims[1] * dims[2] * 4;
            for (int res = 0; res < 2; ++res)
                for (int oc = 0; oc < 2; ++oc)
                    if (check_layout({{res ? n * field_stride(flags) : 0, oc ? occupancy_bytes(dims) : 0},
                                      {res ? N * stride : 0, oc ? occ : 0}}))
                        return 1;
        }
    }

    // 2^26 rays: the ray part alone is 2^31 bytes
    {
        const uint32_t n = 1u << 26;
        const size_t parts[] = {n * kRayBytes, n * kSurfResultBytes, n * kPixelBytes, n * kShadeStepsBytes};
        const BlockLayout l = block_layout(parts, 4);
        CHECK(parts[0] == (size_t)1 << 31);
        CHECK(l.offset[1] == (size_t)1 << 31 && l.offset[2] == (size_t)1 << 32);
        CHECK(l.offset[3] == ((size_t)1 << 32) + ((size_t)1 << 28));
        CHECK(l.total == ((size_t)1 << 32) + ((size_t)1 << 28) + ((size_t)1 << 29));
    }

    // the largest lattice, 4096 x 4096 x 4 with normals and occupancy: n * 16 bytes of results, then
    // ceil(nx / 32) * ny * nz * 4 bytes of occupancy
    {
        const uint32_t dims[3] = {4096, 4096, 4}, n = 1u << 26;
        const size_t parts[] = {n * field_stride(kFieldNormal), occupancy_bytes(dims)};
        CHECK(parts[0] == (size_t)1 << 30 && parts[1] == (size_t)128 * 4096 * 4 * 4);
        const BlockLayout l = block_layout(parts, 2);
        CHECK(l.offset[0] == 0 && l.offset[1] == (size_t)1 << 30 && l.total == ((size_t)1 << 30) + ((size_t)1 << 23));
        // a row that is no multiple of 32 points, a result that is no multiple of 16 bytes
        const uint32_t odd[3] = {33, 5, 3};
        const size_t small[] = {(size_t)33 * 5 * 3 * field_stride(0), occupancy_bytes(odd)};
        CHECK(small[0] == 1980 && small[1] == 2 * 5 * 3 * 4);
        const BlockLayout s = block_layout(small, 2);
        CHECK(s.offset[1] == 1984 && s.total == 1984 + 128);
    }

    // the three option parsers over the one prefix parser
    if (check_prefix<Options>(kOptSizeV1, parse_options)) return 1;
    if (check_prefix<SurfOptions>(kSurfOptSizeV1, parse_surface_options)) return 1;
    if (check_prefix<FieldOptions>(kFieldOptSizeV1, parse_field_options)) return 1;
    CHECK(kOptSizeV1 == 24 && kSurfOptSizeV1 == 40 && kFieldOptSizeV1 == 24);
    std::printf("querylayout_check ok\n");
    return 0;
}
