// rt_kernels.hip -- HIP kernels for gfx950 (MI355X).
//
//   k_camerarays   <- Media/common/shaders/camerarays.hlsl:12-21
//   k_order        <- Graphics/Terrain.cpp:356-439 (setTargetDepths: host code in
//                     the reference; on the device here so a frame needs no
//                     GPU->CPU->GPU round trip)
//   k_order (+ the longest-first tile order), k_trace, k_finish
//                  <- Media/common/shaders/tracescreen.hlsl:16-76 (split pipeline below)
//   k_shard_copy   -- tile-cyclic shard pack/unpack for the multi-GPU gather
//
// k_trace is a persistent kernel: one 1024-thread workgroup per CU keeps the noise
// tables (128 KiB) in LDS and every wave pulls 8x8-pixel work units from a device-wide
// atomic queue, so a finished wave takes new work instead of idling until the slowest
// wave of its workgroup retires.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "rt_kernels.h"
#include "rt_rayquery.h"
#include "rt_shader.h"
#include "rt_variants.h"

using namespace rts;
using rtm::f3;

namespace {

// LDS image (rts::NoiseView): perm2D texels at offset 0 (64 KiB), the paired lane-private
// gradients gxy at kLdsGxy (32 KiB) and gz at kLdsGz (32 KiB, 8 of every 16 B used), then the
// nomadplains FBM octave constants (NoiseView::oct): (S, 0.35 S, 1/S, 0) for N = 0..RT_NP_OCTAVES + 2
// (.w is unused and stays 0; the entries past the last octave are padding).  A kernel declares it as its
// ONLY static LDS array, so it sits at LDS address 0 and the texel address needs no base (other LDS a
// kernel needs is carved after it).
constexpr int kPermWords = 128 * 128;
constexpr int kNpOct = RT_NP_OCTAVES + 3;
constexpr int kOctWords = kNpOct * 4;
constexpr int kOctBase = (int)kLdsGz / 4 + (int)(kLdsGz - kLdsGxy) / 4; // words
constexpr int kNoiseLdsWords = kOctBase + kOctWords;
static_assert(kNoiseLdsWords % 4 == 0, "LDS carved after the noise image stays 16-byte aligned");
static_assert(kLdsGxy == (uint32_t)kPermWords * 4u, "gxy follows the perm2D texels");

__device__ __forceinline__ void load_noise_lds(uint32_t* lds, const uint32_t* __restrict__ perm2d,
                                               const float4* __restrict__ grad, const RtConsts* __restrict__ k)
{
    {
        float4* oct = reinterpret_cast<float4*>(lds + kOctBase);
        const int i = threadIdx.x;
        if (i < kNpOct) {
            const int n = i <= RT_NP_OCTAVES ? i : RT_NP_OCTAVES;
            oct[i] = make_float4(k->np_scale[n], k->np_scale_y[n], k->np_rcp[n], 0.0f);
        }
    }
    float4* gxy = reinterpret_cast<float4*>(lds + kLdsGxy / 4);
    float4* gz = reinterpret_cast<float4*>(lds + kLdsGz / 4); // gxy's slot layout, 8 of 16 B used
    for (int i = threadIdx.x; i < 128 * 16; i += blockDim.x) {
        int e = i >> 4;
        float4 g0 = grad[e], g1 = grad[(e + 1) & 127];
        gxy[i] = make_float4(g0.x, g1.x, g0.y, g1.y);
        gz[i] = make_float4(g0.z, g1.z, 0.0f, 0.0f);
    }
    uint4* p = reinterpret_cast<uint4*>(lds);
    const uint4* src = reinterpret_cast<const uint4*>(perm2d);
    for (int i = threadIdx.x; i < kPermWords / 4; i += blockDim.x) p[i] = src[i];
    __syncthreads();
}

// A buffer pointer read from a FrameTable, as a global-address-space pointer: plain pointers
// loaded from memory are generic, and their accesses flat instructions that wait on the LDS
// counter too.
template <class T>
__device__ __forceinline__ T __attribute__((address_space(1)))* gptr(T* p)
{
    return (T __attribute__((address_space(1)))*)p;
}
__device__ __forceinline__ void gstore(float4* p, float4 v)
{
    typedef float v4f __attribute__((ext_vector_type(4)));
    *(v4f __attribute__((address_space(1)))*)p = v4f{v.x, v.y, v.z, v.w};
}

__device__ __forceinline__ Ctx make_ctx(const RtConsts* k, const uint32_t* lds)
{
    Ctx c;
    c.nz.img = reinterpret_cast<const char*>(lds);
    c.nz.oct = reinterpret_cast<const float4*>(lds + kOctBase);
    c.nz.so16 = kLdsGxy | ((threadIdx.x & (RT_LDS_SLOTS - 1u)) * 16u);
    c.nz.calls = 0;
    c.nz.lds_calls = nullptr;
    c.nz.phase = RT_PHASE_OTHER;
    c.k = k;
    c.kf = (KPtr)k;
    c.eye = rtm::mk(k->eye[0], k->eye[1], k->eye[2]);
    c.sun = rtm::mk(k->sun[0], k->sun[1], k->sun[2]);
    return c;
}

// A query kernel's context: its LOD eye (nomadplains' octave count, getNormal's eps) is a kernel argument in
// place of the constant block's Eye -- wave-uniform, and the compute's constants stay as the frame loop left them.
struct QueryEye {
    float x, y, z;
};
__device__ __forceinline__ Ctx make_ctx(const RtConsts* k, const uint32_t* lds, QueryEye e)
{
    Ctx c = make_ctx(k, lds);
    c.eye = rtm::mk(e.x, e.y, e.z);
    return c;
}

// STATS kernels: a lane's noise count (NoiseView::calls) into the frame statistics
__device__ __forceinline__ void stats_noise(RtStats* stats, uint64_t calls)
{
    atomicAdd(&stats->noise_calls, (unsigned long long)(calls & 0xffffffffull));
    if (calls >> 32) atomicAdd(&stats->noise_waves, (unsigned long long)(calls >> 32));
}

__device__ __forceinline__ float uniform_f(float x)
{
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}

// prepass frame f of a batch: its camerarays block (camera) as kf, Eye/Sun uniform
__device__ __forceinline__ Ctx frame_ctx_cam(const Ctx& c, const FrameTable* __restrict__ ft, uint32_t f)
{
    Ctx cf = c;
    cf.kf = (KPtr)ft->kcam[f];
    cf.eye = rtm::mk(uniform_f(cf.kf->eye[0]), uniform_f(cf.kf->eye[1]), uniform_f(cf.kf->eye[2]));
    cf.sun = rtm::mk(uniform_f(cf.kf->sun[0]), uniform_f(cf.kf->sun[1]), uniform_f(cf.kf->sun[2]));
    return cf;
}

// ---------------------------------------------------------------------------
// camerarays.hlsl:12-21.  One thread per prepass cell (32x32).
// ft != null: frame blockIdx.y of a batch (its constants and CameraResults from the table).
template <int L, bool STATS>
__global__ void __launch_bounds__(64) k_camerarays(const RtConsts* __restrict__ k, const uint32_t* __restrict__ perm2d,
                                                   const float4* __restrict__ grad, float4* __restrict__ out,
                                                   RtStats* stats, const FrameTable* __restrict__ ft)
{
    if (ft) out = ft->cam[blockIdx.y];
    __shared__ __attribute__((aligned(16))) uint32_t lds[kNoiseLdsWords];
    load_noise_lds(lds, perm2d, grad, k);
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= RT_CAMERA_RES * RT_CAMERA_RES) return;
    Ctx c = make_ctx(k, lds);
    if (ft) c = frame_ctx_cam(c, ft, blockIdx.y);
    int tx = i % RT_CAMERA_RES, ty = i / RT_CAMERA_RES;
    const float r31 = rtm::rcp(31.0f);
    uint32_t pxs = (uint32_t)(((float)tx * r31) * k->screen[0]);
    uint32_t pys = (uint32_t)(((float)ty * r31) * k->screen[1]);
    f3 p, dir;
    get_pixel_ray(c, (float)pxs, (float)pys, &p, &dir);
    RayResult rr = trace_ray<L, false, true>(c, p, RT_CAMERA_NEAR, RT_CAMERA_FAR, 2.0f, dir, 0);
    if (rr.density < 0.0f) rr.pd.w = RT_CAMERA_FAR;
    out[i] = make_float4(rr.pd.x, rr.pd.y, rr.pd.z, rr.pd.w);
    if constexpr (STATS) {
        atomicAdd(&stats->prepass_steps, (unsigned long long)rr.steps);
        stats_noise(stats, c.nz.calls);
    }
}

// camerarays.hlsl:12-21 for nomadplains with one 32-lane group per prepass ray:
// the prepass is 1024 sequential marches of ~350 steps, so it is bound by the
// latency of one step, and spreading each step's 17 FBM octaves + steep noise over
// a lane group (rts::density_nomadplains_seg<LPR>, LPR lanes per ray) shortens that chain ~4x.
template <bool STATS, int BS, int LPR>
__global__ void __launch_bounds__(BS) k_camerarays_group(const RtConsts* __restrict__ k,
                                                          const uint32_t* __restrict__ perm2d,
                                                          const float4* __restrict__ grad, float4* __restrict__ out,
                                                          RtStats* stats, const FrameTable* __restrict__ ft)
{
    constexpr int L = RT_NOMADPLAINS;
    if (ft) out = ft->cam[blockIdx.y];
    __shared__ __attribute__((aligned(16))) uint32_t lds[kNoiseLdsWords];
    load_noise_lds(lds, perm2d, grad, k);
    const int i = blockIdx.x * (BS / LPR) + (int)(threadIdx.x / LPR);
    if (i >= RT_CAMERA_RES * RT_CAMERA_RES) return; // whole groups leave together
    Ctx c = make_ctx(k, lds);
    if (ft) c = frame_ctx_cam(c, ft, blockIdx.y);
    const uint32_t j = threadIdx.x & (LPR - 1u), base = threadIdx.x & 63u & ~(LPR - 1u);
    const SegOctaves<LPR> g = seg_octaves<LPR>(c, j);
    int tx = i % RT_CAMERA_RES, ty = i / RT_CAMERA_RES;
    const float r31 = rtm::rcp(31.0f);
    uint32_t pxs = (uint32_t)(((float)tx * r31) * k->screen[0]);
    uint32_t pys = (uint32_t)(((float)ty * r31) * k->screen[1]);
    f3 p, dir;
    get_pixel_ray(c, (float)pxs, (float)pys, &p, &dir);
    March<L, false> st;
    march_begin(c, st, p, RT_CAMERA_NEAR, 2.0f, dir);
    uint32_t noise = 0;
    while (march_live<L, false, true>(c, st, RT_CAMERA_FAR, 0)) {
        auto dens = [&](f3 q) {
            uint32_t used;
            float d = density_nomadplains_seg<LPR>(c, g, q, j, base, &used);
            noise += used + 1u;
            return d;
        };
        march_step_with<L, false, true>(c, st, dens);
    }
    RayResult rr = march_result(st);
    if (rr.density < 0.0f) rr.pd.w = RT_CAMERA_FAR;
    if (j == 0) {
        out[i] = make_float4(rr.pd.x, rr.pd.y, rr.pd.z, rr.pd.w);
        if constexpr (STATS) {
            atomicAdd(&stats->prepass_steps, (unsigned long long)rr.steps);
            atomicAdd(&stats->noise_calls, (unsigned long long)noise);
        }
    }
}

// ---------------------------------------------------------------------------
// Terrain.cpp:356-439 with the host's std::min/std::max argument order.  `depth(x, y)` reads the
// CameraResults depth of prepass ray (x, y) (coordinates already clamped to the 32 x 32 grid): from an
// LDS copy (k_order) or straight from the frame's CameraResults (the gated launch's lanes).
template <class Depth>
__device__ __forceinline__ float cd_get_depth(Depth depth, int x, int y)
{
    x = x < 0 ? 0 : (x >= RT_CAMERA_RES ? RT_CAMERA_RES - 1 : x);
    y = y < 0 ? 0 : (y >= RT_CAMERA_RES ? RT_CAMERA_RES - 1 : y);
    return depth(x, y);
}
template <class Depth>
__device__ __forceinline__ float cd_interp(Depth d, int x, int y)
{
    if (x < 0) {
        float m = cd_get_depth(d, x + 1, y);
        float dd = cd_get_depth(d, x + 2, y) - m;
        return m - dd;
    }
    if (x >= RT_CAMERA_RES) {
        float m = cd_get_depth(d, x - 1, y);
        float dd = cd_get_depth(d, x - 2, y) - m;
        return m - dd;
    }
    if (y < 0) {
        float m = cd_get_depth(d, x, y + 1);
        float dd = cd_get_depth(d, x, y + 2) - m;
        return m - dd;
    }
    if (y >= RT_CAMERA_RES) {
        float m = cd_get_depth(d, x, y - 1);
        float dd = cd_get_depth(d, x, y - 2) - m;
        return m - dd;
    }
    return cd_get_depth(d, x, y);
}

// setTargetDepths (Terrain.cpp:398-439) of cell (xpos, ypos): its (dmin, dmax) bracket from the 5 x 5
// neighbourhood of prepass depths
template <class Depth>
__device__ __forceinline__ float2 cell_bracket(Depth depth, int xpos, int ypos)
{
    float dmin = cd_interp(depth, xpos, ypos);
    float dmax = dmin;
    for (int xp = -2; xp <= 2; ++xp) {
        for (int yp = -2; yp <= 2; ++yp) {
            float d = cd_interp(depth, xpos + xp, ypos + yp);
            dmin = (dmin < d) ? dmin : d;
            dmax = (d < dmax) ? dmax : d;
        }
    }
    dmin = dmin * 0.96f - 0.01f;
    dmax = dmax * 1.22f + 0.4f;
    dmin = (RT_CAMERA_NEAR < dmin) ? dmin : RT_CAMERA_NEAR;
    dmax = (dmax < RT_CAMERA_FAR) ? dmax : RT_CAMERA_FAR;
    return make_float2(dmin, dmax);
}

// a prepass depth read straight from CameraResults another wave stored with sc1 (FusedPrepass, the
// gated launch): an sc1 global_load_dword, after the poll of the writers' flag or counter matched
__device__ __forceinline__ float cam_depth_sc1(const float4* cam, int x, int y)
{
    typedef const float __attribute__((address_space(1))) gfloat;
    return __hip_atomic_load((gfloat*)(reinterpret_cast<const float*>(cam + y * RT_CAMERA_RES + x) + 3),
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// setTargetDepths of one frame by a 1024-thread block (thread = cell), depth scratch in LDS
__device__ __forceinline__ void cell_depths_frame(const float4* __restrict__ cam, float2* __restrict__ cells,
                                                  float* s_d)
{
    const int i = threadIdx.x;
    __syncthreads(); // s_d's previous frame is no longer read
    // sc1 (L1-bypassing) load: a fused prepass wrote these in another kernel (FusedPrepass; the
    // hand-off's loads are all global_load_dword sc1 after k_order's poll and barrier)
    s_d[i] = cam_depth_sc1(cam, i % RT_CAMERA_RES, i / RT_CAMERA_RES);
    __syncthreads();
    cells[i] = cell_bracket([&](int x, int y) { return s_d[y * RT_CAMERA_RES + x]; }, i % RT_CAMERA_RES,
                            i / RT_CAMERA_RES);
}

// ===========================================================================
// Screen pipeline: tracescreen.hlsl:16-76 over a batch of frames in four launches.
//   k_order     : longest-first 32x32 tile order per frame (scheduling only).
//   k_trace     : persistent; primary march (tracing.hlsl:47-105) per 8x8 unit, the hit
//                 shading + first shadow step, the long shadow / AO rays (LDS rings).
//   k_finish    : sky colour of the misses + in-order AA average + UNORM8.
// Sample t = (u*64 + j)*AA + a: AA sample a of lane-slot j of 8x8 unit u.
// A batch of n_frames frames: unit g of the launch is unit g % n_units of frame g / n_units
// (frame-major, so a frame's tail overlaps the next frame's units), and sample ids are
// global: frame f's sample t is f * frame_samples + t (frame_samples = n_units * 64 * AA).
struct UnitMap {
    uint32_t off_x, off_y, ext_x, ext_y, tiles32_x, tile_first, tile_stride, n_units;
    uint32_t n_frames, frame_samples;
    uint32_t frame_rot; // 1: frame f of a batch traces shard (tile_first + f) % tile_stride
    uint32_t order_batch; // k_order: 1 one longest-first order over the batch, 0 one per frame (frame-major)
    uint32_t cells_from_cam; // k_order first derives each frame's CellDistance from its CameraResults
    // 1: one sample per pixel, no float output, <= 1 AO ray per hit: hit pixels are finished in k_trace
    // where their last ray ends (fit_pixel), and k_finish only finishes the hits that have a long shadow
    // beside their AO ray (their bit in hitmask); with no AO, no k_finish at all
    uint32_t fit;
    // 1: one sample per pixel, no float output, >= 2 AO rays per hit: a hit whose shadow ends at its first
    // step (no long shadow) keeps its colour in its block's colour pool beside its AO counter slot, and the
    // AO ray that completes the count stores the pixel (fitm in k_trace); the rest go through k_finish,
    // flagged as with fit
    uint32_t fitm;
    // 1: out8[f] is this rank's PACKED shard buffer of frame f (k_shard_copy's layout: the shard's k-th tile
    // at k * 1024 pixels, rows of 32 within the tile), written in place of the framebuffer, so a sharded
    // batch needs no pack launch before its gather (RGBA8 only; rt_terrain_render_batch_packed)
    uint32_t packed;
};

// Where pixel (px, py) of lane `lane` of unit u goes in its frame's RGBA8 output: the framebuffer row-major,
// or (UnitMap::packed) the unit's tile u >> 4 of the shard at 1024 pixels each, row (sub >> 2) * 8 +
// (lane >> 3) and column (sub & 3) * 8 + (lane & 7) of the tile (sub = u & 15; unit_pixel's mapping)
__device__ __forceinline__ uint32_t out_index(const UnitMap& m, uint32_t u, uint32_t lane, uint32_t px, uint32_t py,
                                              uint32_t W)
{
    if (m.packed)
        return (u >> 4) * 1024u + ((u & 15u) >> 2) * 256u + (lane >> 3) * 32u + (u & 3u) * 8u + (lane & 7u);
    return py * W + px;
}
// the same from a frame's sample id tl = u * 64 + lane (one sample per pixel): its bits 0-2 (lane & 7) stay,
// 6-7 (u & 3) -> 3-4, 3-5 (lane >> 3) -> 5-7, 8-9 -> 8-9 (sub >> 2), 10.. (the shard's tile) stay
__device__ __forceinline__ uint32_t packed_index(uint32_t tl)
{
    return (tl & ~0xf8u) | ((tl >> 3) & 0x18u) | ((tl << 2) & 0xe0u);
}

__device__ __forceinline__ bool unit_pixel(const UnitMap& m, uint32_t f, uint32_t u, uint32_t lane, uint32_t W,
                                           uint32_t H, uint32_t* px, uint32_t* py)
{
    const uint32_t first = m.frame_rot ? (m.tile_first + f) % m.tile_stride : m.tile_first;
    // 8x8 units (16x4 and 32x2 measured 1% and 3% slower at C3: rows near the horizon
    // diverge more along x than an 8x8 block does along y)
    uint32_t T = (u >> 4) * m.tile_stride + first, sub = u & 15u;
    uint32_t gx = (T % m.tiles32_x) * 32u + (sub & 3u) * 8u + (lane & 7u);
    uint32_t gy = (T / m.tiles32_x) * 32u + (sub >> 2) * 8u + (lane >> 3);
    *px = gx + m.off_x;
    *py = gy + m.off_y;
    return gx < m.ext_x && gy < m.ext_y && *px < W && *py < H;
}

__device__ __forceinline__ bool sample_pixel(const UnitMap& m, uint32_t f, uint32_t t, uint32_t aa, uint32_t W,
                                             uint32_t H, uint32_t* px, uint32_t* py, uint32_t* a)
{
    uint32_t pix = t / aa;
    *a = t - pix * aa;
    return unit_pixel(m, f, pix >> 6, pix & 63u, W, H, px, py);
}

__device__ __forceinline__ uint32_t wave_fetch(uint32_t* counter, uint32_t lane, uint32_t n = 1u)
{
    uint32_t u = 0;
    if (lane == 0) u = atomicAdd(counter, n);
    return __builtin_amdgcn_readfirstlane(u);
}

// Set bits of `mask` below this lane (its rank among the lanes of `mask`): v_mbcnt_lo/hi, so no
// 64-bit lane mask stays live in VGPRs across the persistent kernels' loops.
__device__ __forceinline__ uint32_t lane_rank(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Per-sample RayResult of the primary march: 3 float4 (pd, fcolord, density).
// the unit index a wave takes first: wave-slot-major over the grid (row w holds order indices
// w * blocks .. w * blocks + blocks - 1, and wave slot w of each block takes the next one of its row in
// the order the blocks START), see k_trace
__device__ __forceinline__ uint32_t first_unit_index(uint32_t* __restrict__ counters, uint32_t lane)
{
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    return w * gridDim.x + wave_fetch(&counters[RT_CTR_FIRST + w], lane);
}

// A hit's record in its block's hit queue (the shading input; misses store none): the primary
// RayResult and the sample id t.  With fog live (greenrocks): 3 float4 (pd + dist, fcolord,
// (density, steps, -, t)).  Without, fcolord is 0 and is not stored, and the hit position is not
// either: the shading re-derives it from the pixel's ray and the last sample's distance
// (march_result's fma), so the record is one float4 (sd, dist, density, t).  The queue is a stack
// per block (hits shade in any order), written densely at its top: the few KiB near the top are
// rewritten over and over and stay in the XCD's L2 (write-back), instead of a sample-indexed array
// whose sparsely written lines (the hit lanes of each unit) each cost a write-back and a re-fetch,
// or a ring whose whole capacity cycles through the L2 (scripts/ubench_l2wb.hip: 16 KiB rewritten
// per block stays in L2, 64 KiB per block is written back on every pass).
template <int L>
struct HitRec {
    // float4 per record (RT_DIAG_HITPAD: a fog-free record padded to 2 with a zero float4, to see what the
    // hit stack's bytes cost in HBM writes)
    static constexpr uint32_t N = FogLive<L>::value ? 3u : (RT_DIAG_HITPAD ? 2u : 1u);
};
template <int L>
__device__ __forceinline__ void hit_store(float4* __restrict__ r, uint32_t t, const RayResult& rr)
{
    if constexpr (FogLive<L>::value) {
        r[0] = make_float4(rr.pd.x, rr.pd.y, rr.pd.z, rr.pd.w);
        r[1] = make_float4(rr.fc.x, rr.fc.y, rr.fc.z, rr.fc.w);
        r[2] = make_float4(rr.density, rr.steps, 0.0f, __uint_as_float(t));
    } else {
        r[0] = make_float4(rr.sd, rr.pd.w, rr.density, __uint_as_float(t));
        if constexpr (RT_DIAG_HITPAD) r[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// Longest-first tile order for k_trace.  A frame's critical path is its few
// grazing units (hundreds of march steps near the horizon); in screen order they
// start half-way through the queue and finish long after the rest.  The prepass
// cells already say where they are: a tile whose cells' depth bracket
// log2(far/near) is wide starts its rays far in front of the surface they hit (or
// graze).  One workgroup buckets the shard's 32x32 tiles by that key (64 buckets,
// descending); the order only decides which wave takes a unit when, never what
// it computes.
// The order spans the whole batch: entry i = (frame << 24) | tile, the batch's tiles of all frames
// longest-first.  Frame-major order (each frame longest-first in turn) left the last frame's
// grazing units to start in the last twelfth of the launch: at an 8-way shard, where a frame's
// share of the launch is shorter than one such unit, they set the batch time (k_trace 5.7 ms for
// 4.0 ms of work).  One workgroup; frame by frame it loads the frame's cell keys and buckets its
// tiles (the bucket bytes stay in LDS for the scatter pass when they fit).
constexpr uint32_t kOrderLdsBuckets = 144u * 1024u;
constexpr uint32_t kOrderBatchUnitsPerWave = 4u;
__global__ void __launch_bounds__(1024) k_order(const FrameTable* __restrict__ ft, UnitMap m,
                                                uint32_t* __restrict__ order, uint32_t* __restrict__ counters,
                                                const uint32_t* wait_ctl, uint32_t wait_total, uint32_t* zero_ctl,
                                                uint32_t* host_flag, uint32_t* gate, uint32_t* claims)
{
    __shared__ float s_key[RT_CAMERA_RES * RT_CAMERA_RES];
    __shared__ uint32_t s_hist[64];
    __shared__ uint8_t s_b[kOrderLdsBuckets];
    // k_trace's work counters start at zero (k_trace follows on the stream), and so do the counters
    // of the next batch's prepass that k_trace runs (FusedPrepass)
    if (blockIdx.x == 0 && threadIdx.x < RT_CTR_BYTES / 4) counters[threadIdx.x] = 0u;
    if (zero_ctl && blockIdx.x == 0 && threadIdx.x < 2) zero_ctl[threadIdx.x] = 0u;
    if (gate) { // the gated launch: this workgroup's frames' task masks, ray counters and tile claims start at zero
        const uint32_t g0 = m.order_batch ? 0u : blockIdx.x, g1 = m.order_batch ? m.n_frames : blockIdx.x + 1u;
        for (uint32_t i = g0 * RT_GATE_WORDS + threadIdx.x; i < g1 * RT_GATE_WORDS; i += blockDim.x) gate[i] = 0u;
        const uint32_t nt = m.n_units >> 4; // order entries per frame (this workgroup writes entries [g0 nt, g1 nt))
        for (uint32_t i = g0 * nt + threadIdx.x; i < g1 * nt; i += blockDim.x) claims[i] = 0u;
    }
    if (wait_ctl) {
        // this batch's prepass runs inside the previous batch's k_trace (FusedPrepass): wait until its
        // rays are in (each task stored its line with sc1, waited, then added to ctl[1]).  The tasks are
        // taken before that kernel's waves may leave, and they are finished by resident waves, so the
        // wait ends; the bound (0.5 s of the 100 MHz clock) turns a broken protocol into a flagged error
        // (rt_device_check) instead of a hang.
        if (threadIdx.x == 0) {
            const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
            while (__hip_atomic_load(wait_ctl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < wait_total) {
                __builtin_amdgcn_s_sleep(8);
                if (__builtin_amdgcn_s_memrealtime() - t0 > 50000000ull) {
                    // fail safe: the frames of this batch may trace from incomplete CameraResults.  The
                    // device's sticky flag (rt_device_check) and the GPU's host-mapped word, which every
                    // later C-ABI call on this GPU reads (RT_ERR_STATE until rt_device_check clears it)
                    atomicOr(counters + RT_CTR_BYTES / 4, RT_FLAG_PREPASS_TIMEOUT);
                    if (host_flag) __hip_atomic_store(host_flag, RT_FLAG_PREPASS_TIMEOUT, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_SYSTEM);
                    break;
                }
            }
        }
        __syncthreads(); // every load of the CameraResults after the poll
    }
    // setTargetDepths (Terrain.cpp:398-439) of this workgroup's frames first: the device path's
    // CellDistance comes from the prepass's CameraResults (one launch fewer than a separate kernel)
    if (m.cells_from_cam) {
        const uint32_t c0 = m.order_batch ? 0u : blockIdx.x, c1 = m.order_batch ? m.n_frames : blockIdx.x + 1u;
        for (uint32_t f = c0; f < c1; ++f) cell_depths_frame(ft->cam[f], ft->cells[f], s_key);
        __syncthreads(); // the cells are stored before load_keys reads them (same workgroup)
    }
    if (threadIdx.x < 64) s_hist[threadIdx.x] = 0;
    const uint32_t n_tiles = m.n_units >> 4;
    const bool cached = n_tiles * m.n_frames <= kOrderLdsBuckets;
    uint32_t f = 0;
    auto load_keys = [&]() {
        __syncthreads(); // the previous frame's keys are no longer read
        const float2* cells = ft->cells[f];
        for (int i = threadIdx.x; i < RT_CAMERA_RES * RT_CAMERA_RES; i += blockDim.x) {
            float2 cd = cells[i];
            s_key[i] = __log2f(cd.y / cd.x);
        }
        __syncthreads();
    };
    auto bucket = [&](uint32_t tile) -> uint32_t {
        const RtConsts* k = ft->k[f];
        const uint32_t W = (uint32_t)k->width, H = (uint32_t)k->height;
        float key = 0.0f;
        // corner pixels of the tile: unit 0 lane 0, unit 3 lane 7, unit 12 lane 56, unit 15 lane 63
        for (uint32_t corner = 0; corner < 4; ++corner) {
            uint32_t px, py;
            uint32_t u = tile * 16u + (corner & 1u) * 3u + (corner >> 1) * 12u;
            uint32_t lane = (corner & 1u) * 7u + (corner >> 1) * 56u;
            if (!unit_pixel(m, f, u, lane, W, H, &px, &py)) {
                if (!unit_pixel(m, f, tile * 16u, 0u, W, H, &px, &py)) continue;
                px = px + (corner & 1u) * 31u < W ? px + (corner & 1u) * 31u : W - 1u;
                py = py + (corner >> 1) * 31u < H ? py + (corner >> 1) * 31u : H - 1u;
            }
            float spx = (float)px * k->rcp_w, spy = (float)py * k->rcp_h;
            uint32_t cell = (uint32_t)rtm::fma(rtm::floor(spy * 32.0f), 32.0f, rtm::floor(spx * 32.0f));
            key = fmaxf(key, s_key[cell]);
        }
        int b = (int)(key * 3.3f);
        return (uint32_t)(b < 0 ? 0 : (b > 63 ? 63 : b));
    };
    // frames [g0, g1) share one longest-first order: the whole batch (one workgroup), or frame
    // blockIdx.x alone (a workgroup per frame)
    {
        const uint32_t g0 = m.order_batch ? 0u : blockIdx.x, g1 = m.order_batch ? m.n_frames : blockIdx.x + 1u;
        for (f = g0; f < g1; ++f) {
            load_keys();
            for (uint32_t t = threadIdx.x; t < n_tiles; t += blockDim.x) {
                const uint32_t b = bucket(t);
                if (cached) s_b[f * n_tiles + t] = (uint8_t)b;
                atomicAdd(&s_hist[b], 1u);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t run = g0 * n_tiles;
            for (int b = 63; b >= 0; --b) {
                uint32_t c = s_hist[b];
                s_hist[b] = run;
                run += c;
            }
        }
        for (f = g0; f < g1; ++f) {
            if (cached) __syncthreads();
            else load_keys();
            for (uint32_t t = threadIdx.x; t < n_tiles; t += blockDim.x) {
                const uint32_t b = cached ? (uint32_t)s_b[f * n_tiles + t] : bucket(t);
                order[atomicAdd(&s_hist[b], 1u)] = (f << 24) | t;
            }
        }
    }
}

// Shading (tracescreen.hlsl:28-35, nomadplains/color.hlsl:8-72).  Per hit, the
// uniform work -- getNormal (3 densities), getColor up to the shadow ray (20-octave
// albedo FBM), the Rayleigh/Mie sky -- and the FIRST shadow-march step
// (color.hlsl:51).  About 70% of shadow rays end there (the surface faces away from
// the low sun, or the first sample is already inside the terrain) and those samples
// are finished on the spot; the rest become long shadow rays (2..~120 steps).
// A long ray's finishing inputs (albedo+specular rgb and brightness, fcolord with fog live,
// rayleigh rgb and skyAmount) go to a slot of its block's fin pool (fin_store), its march state to
// a 3-float4 record (long_pack).
constexpr uint32_t kShadowRec = 3;

// Lanes idle before a long-ray wave refills them: amortises the refill's divergent
// prologue against the idle lanes it leaves (knobs: rt_variants.h).
constexpr uint32_t kRefillIdle = RT_REFILL_IDLE;

// color.hlsl:53-71 after the shadow ray, then tracescreen.hlsl:33-35 fog and sky blends
__device__ __forceinline__ float4 shade_finish(const RtConsts* k, float4 cb, float4 fog, float4 ray,
                                               float shadow_density, float shadow_fog_w)
{
    float b = cb.w;
    if (shadow_density > 0.0f) b = b * 0.1f;
    else b = rtm::sat(b - shadow_fog_w);
    f3 col = rtm::mk(cb.x * fma(b, k->one_minus_shadow[0], k->shadow_color[0]),
                     cb.y * fma(b, k->one_minus_shadow[1], k->shadow_color[1]),
                     cb.z * fma(b, k->one_minus_shadow[2], k->shadow_color[2]));
    col = rtm::mk(rtm::lerp(col.x, fog.x, fog.w), rtm::lerp(col.y, fog.y, fog.w), rtm::lerp(col.z, fog.z, fog.w));
    col = rtm::mk(rtm::lerp(col.x, ray.x, ray.w), rtm::lerp(col.y, ray.y, ray.w), rtm::lerp(col.z, ray.z, ray.w));
    return make_float4(rtm::sat(col.x), rtm::sat(col.y), rtm::sat(col.z), 1.0f); // w = 1: a hit (AO applies)
}

// tracescreen.hlsl:22-27,36-38: the colour of a MISS sample (sky: Rayleigh/Mie + space noise, then the
// fog and sky-amount blends), saturated; w = 0 (no AO).  Computed where the primary march ends, so
// misses leave no RayResult behind.
__device__ __forceinline__ float4 miss_sample(const Ctx& c, float px, float py, float dist, f4 fog)
{
    f3 p, dir;
    get_pixel_ray(c, px, py, &p, &dir);
    f3 pdn = rtm::normalize(dir);
    float skyAmount = dist * 0.0005f;
    skyAmount = rtm::sat(skyAmount * skyAmount);
    SkyColor scat = get_rayleigh_mie(c, pdn);
    float space = get_space_color(c, pdn);
    f3 sky = rtm::mk((scat.mie.x + scat.rayleigh.x) + space, (scat.mie.y + scat.rayleigh.y) + space,
                     (scat.mie.z + scat.rayleigh.z) + space);
    f3 col = rtm::mk(rtm::lerp(sky.x, fog.x, fog.w), rtm::lerp(sky.y, fog.y, fog.w), rtm::lerp(sky.z, fog.z, fog.w));
    col = rtm::mk(rtm::lerp(col.x, sky.x, skyAmount), rtm::lerp(col.y, sky.y, skyAmount),
                  rtm::lerp(col.z, sky.z, skyAmount));
    return make_float4(rtm::sat(col.x), rtm::sat(col.y), rtm::sat(col.z), 0.0f);
}

// Loads of data another wave of this kernel (on this CU) wrote: bypass the CU's L1 (a line cached
// there earlier would be stale), served by the XCD's L2 the producer wrote through: `sc1` loads.
// Not nontemporal ones: an nt load marks the line evict-first, so the per-block LIFO hit stack and
// fin pool, whose few lines are rewritten over and over, were written back to HBM after every pop
// (profiles/r04/traffic_attribution.md).  ld_rec: record i (16-B units) of a block-local array (a
// uniform base, so a buffer load); ld_fresh: any address (the fin[t] fallback), waited at once.
typedef float v4f_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld_rec(const float4* base, uint32_t i)
{
    const __amdgpu_buffer_rsrc_t r =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float4*>(base), (short)0, 0x7fffffff, 0x00020000);
    const v4f_t v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)(i * 16u), 0, 16 /* sc1 */);
    return make_float4(v.x, v.y, v.z, v.w);
}
// word i of a buffer with a uniform base (one offset register per lane): sc1 (another wave or workgroup
// wrote it in this launch) or plain
__device__ __forceinline__ uint32_t ld_u32(const uint32_t* base, uint32_t i, bool sc1 = true)
{
    const __amdgpu_buffer_rsrc_t r =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(base), (short)0, 0x7fffffff, 0x00020000);
    return sc1 ? __builtin_amdgcn_raw_buffer_load_b32(r, (int)(i * 4u), 0, 16 /* sc1 */)
               : __builtin_amdgcn_raw_buffer_load_b32(r, (int)(i * 4u), 0, 0);
}
__device__ __forceinline__ float4 ld_fresh(const float4* p)
{
    v4f_t v;
    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
    return make_float4(v.x, v.y, v.z, v.w);
}

// A hit's finished sample.  With one sample per pixel only hits reach `samples` (misses are
// finished where their march ends) and every sample k_finish reads is a hit, so the record is the
// colour alone: 12 B (a float3 array over the same buffer); with AA, misses are stored too and w
// marks the hits (16 B).
// An opaque copy of a lane value: address arithmetic on it cannot be hoisted above this point, so a
// store's 64-bit address is formed where the store is (one VGPR live before it, not two).
__device__ __forceinline__ uint32_t late(uint32_t x)
{
    asm volatile("" : "+v"(x));
    return x;
}

__device__ __forceinline__ void sample_store(const RtConsts* k, float4* __restrict__ samples, uint32_t t, float4 v)
{
    t = late(t);
    if (k->aa_samples == 1) { // 3 floats at 12-byte stride (a float3 vector type would pad to 16)
        float* c = reinterpret_cast<float*>(samples) + 3u * t;
        c[0] = v.x;
        c[1] = v.y;
        c[2] = v.z;
    } else {
        samples[t] = v;
    }
}

// The AO extension's per-sample count of occluded AO rays: one byte per sample (at most 16 AO
// rays), four to a word, so a count's atomic add and k_finish's read touch a quarter of the lines
// a word per sample did (and the per-launch memset a quarter of the bytes).
__device__ __forceinline__ void ao_count(uint32_t* __restrict__ aocc, uint32_t t)
{
    atomicAdd(&aocc[t >> 2], 1u << ((t & 3u) * 8u));
}
// UnitMap::fitm with AO: a sample k_finish finishes carries kFinFlag in its byte (plain stores, k_trace)
constexpr uint32_t kFinFlag = 0x80u;
__device__ __forceinline__ uint32_t ao_occluded(const uint32_t* __restrict__ aocc, uint32_t t)
{
    return (aocc[t >> 2] >> ((t & 3u) * 8u)) & 0x7fu;
}

struct ShadeHit {
    float4 cb, fog, ray;
    bool more; // the shadow ray is still marching after its first step
    f3 hp, n;  // hit position and normal (AO rays start here)
    float prec; // shadow-ray stepmod (AO rays reuse it)
    uint32_t px, py, a;
};


// frame f's context (f wave-uniform): its constant block (camera, sun) as cf.kf, its Eye and
// SunDirection in scalar registers; the launch's block c.k stays the source of every
// frame-invariant constant (scalar loads in the hot loops)
__device__ __forceinline__ Ctx frame_ctx(const Ctx& c, const FrameTable* __restrict__ ft, uint32_t f)
{
    Ctx cf = c;
    cf.kf = (KPtr)ft->k[f];
    cf.eye = rtm::mk(uniform_f(cf.kf->eye[0]), uniform_f(cf.kf->eye[1]), uniform_f(cf.kf->eye[2]));
    cf.sun = rtm::mk(uniform_f(cf.kf->sun[0]), uniform_f(cf.kf->sun[1]), uniform_f(cf.kf->sun[2]));
    return cf;
}

// the frame a global sample id belongs to
__device__ __forceinline__ uint32_t frame_of(const UnitMap& m, uint32_t t)
{
    return m.n_frames == 1u ? 0u : t / m.frame_samples;
}

// body(f) once per distinct frame f among the `valid` lanes, with exactly the lanes of
// frame f active (f wave-uniform).  A batch of hits or rays mixes frames only around the
// point where the frame-major unit order moves on to the next frame.
template <class Body>
__device__ __forceinline__ void per_frame(bool valid, uint32_t f_lane, Body body)
{
    uint64_t pend = __ballot(valid);
    while (pend) {
        const uint32_t f = (uint32_t)__builtin_amdgcn_readlane((int)f_lane, (int)__builtin_ctzll(pend));
        const bool mine = valid && f_lane == f;
        pend &= ~__ballot(mine);
        if (mine) body(f);
    }
}

// Per-frame values a long ray needs on its own lane: the frame's Eye (the octave count of
// every density sample) and its normalised SunDirection (a shadow ray's direction).
struct FrameRays {
    float v[RT_MAX_BATCH][6];
    uint32_t* out8[RT_MAX_BATCH]; // the frames' RGBA8 framebuffers (UnitMap::fit: pixels stored by long rays)
};
__device__ __forceinline__ void frame_rays_load(FrameRays& s, const FrameTable* __restrict__ ft, uint32_t n_frames)
{
    if (threadIdx.x < n_frames) {
        const RtConsts* k = ft->k[threadIdx.x];
        const f3 sun = rtm::mk(k->sun[0], k->sun[1], k->sun[2]);
        const f3 sd = rtm::scale(sun, rtm::rcp(rtm::length(sun))); // tracing.hlsl:60-61
        s.v[threadIdx.x][0] = k->eye[0];
        s.v[threadIdx.x][1] = k->eye[1];
        s.v[threadIdx.x][2] = k->eye[2];
        s.v[threadIdx.x][3] = sd.x;
        s.v[threadIdx.x][4] = sd.y;
        s.v[threadIdx.x][5] = sd.z;
        s.out8[threadIdx.x] = ft->out8[threadIdx.x];
    }
}

// tracescreen.hlsl:22-35 (hit branch) through the first shadow-march step.  r0..r2: the hit's
// record (hit_store), t: the global sample id (buffers), tl: the sample within its frame (pixel).
template <int L>
__device__ __forceinline__ ShadeHit shade_hit(const Ctx& c, const UnitMap& m, float4 r0, float4 r1, float4 r2,
                                              uint32_t t, uint32_t tl, March<L, true>& st)
{
    const RtConsts* k = c.k;
    const uint32_t W = (uint32_t)k->width, H = (uint32_t)k->height, aa = (uint32_t)k->aa_samples;
    ShadeHit h;
    float4 pdw, dn;
    if constexpr (FogLive<L>::value) {
        pdw = r0;
        h.fog = r1;
        dn = r2;
    } else { // hit_store's fog-free layout; fcolord is 0
        (void)r1;
        (void)r2;
        pdw = make_float4(r0.x, 0.0f, 0.0f, r0.y); // (sd, -, -, dist) until the position is re-derived
        dn = make_float4(r0.z, 0.0f, 0.0f, 0.0f);
        h.fog = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    uint32_t px, py, a;
    sample_pixel(m, m.frame_rot ? (t - tl) / m.frame_samples : 0u, tl, aa, W, H, &px, &py, &a);
    h.px = px;
    h.py = py;
    h.a = a;
    f3 p, dir;
    get_pixel_ray(c, (float)px + k->aa_off[a][0], (float)py + k->aa_off[a][1], &p, &dir);
    if constexpr (!FogLive<L>::value) {
        // the primary march's last sample: march_begin's normalised direction, the step's fma
        const f3 md = rtm::scale(dir, rtm::rcp(rtm::length(dir)));
        const float sd = pdw.x;
        pdw = make_float4(fma(md.x, sd, p.x), fma(md.y, sd, p.y), fma(md.z, sd, p.z), pdw.w);
    }
    f3 hp = rtm::mk(pdw.x, pdw.y, pdw.z);
    h.hp = hp;
    // color.hlsl:51 traceRay(p, 0.4, 100, precision, SunDirection, fog, skiprefine): the first step,
    // taken before the normal and the colour (it needs neither; precision is the hit distance's),
    // so the colour's FBM and the step's density never hold their live values at the same time
    h.prec = shade_precision(pdw.w);
    march_begin(c, st, hp, 0.4f, h.prec, c.sun);
    if (march_live<L, true, true>(c, st, 100.0f, 0)) march_step<L, true, true>(c, st);
    h.more = march_live<L, true, true>(c, st, 100.0f, 0);
    f3 pdn = rtm::normalize(dir);
    float skyAmount = pdw.w * 0.0005f;
    skyAmount = rtm::sat(skyAmount * skyAmount);
    f4 pd = {pdw.x, pdw.y, pdw.z, dn.x}; // getNormal(float4(rr.pd.xyz, rr.density)) :31
    f3 n = get_normal<L>(c, pd);
    h.n = n;
    ShadePre sp = shade_pre<L>(c, hp, n, pdn, pdw.w);
    // color.hlsl:63-66: the specular term does not depend on the shadow
    float specular = rtm::sat(rtm::pow_nonneg(rtm::max(sp.spec_dot, 0.0f), 40.0f)) * sp.spec_k;
    SkyColor scat = get_rayleigh_mie(c, pdn);
    h.cb = make_float4(sp.col[0] + specular, sp.col[1] + specular, sp.col[2] + specular, sp.brightness);
    h.ray = make_float4(scat.rayleigh.x, scat.rayleigh.y, scat.rayleigh.z, skyAmount);
    return h;
}

// A long ray's `aux` word: an AO ray (sign bit set: kAuxAO, its occlusion counted in aocc for k_finish;
// or, with UnitMap::fit, kAuxAOCand | rgb24 = its hit's pixel if the ray is occluded, stored where the
// ray ends), or a shadow ray whose finishing inputs (fin_store) sit in its block's fin pool slot aux
// (< kFinSlots), or at fin[t] when the pool was empty (kAuxFinT).
constexpr uint32_t kAuxAO = 0xffffffffu, kAuxAOCand = 0x80000000u, kAuxFinT = 0x7ffffffeu;
__device__ __forceinline__ bool aux_ao(uint32_t aux) { return (int32_t)aux < 0; }
// With AO_SAMPLES >= 2 a hit's AO rays count their occlusion in a slot of the block's AO
// counters in LDS (kAuxAOSlot | slot, TraceQueues::ao_ctr): the ray that completes the count stores it,
// one plain byte store per hit; an idle lane holding kAuxSlotFree | slot returns the slot to the free list
// at its wave's next refill.  No free slot: the hit's rays count by device atomics (kAuxAO).
constexpr uint32_t kAuxAOSlot = 0xc0000000u, kAuxSlotFree = 0x60000000u;
__device__ __forceinline__ bool aux_ao_slot(uint32_t aux) { return (aux & 0xff000000u) == kAuxAOSlot; }
__device__ __forceinline__ bool aux_slot_free(uint32_t aux) { return (aux & 0xff000000u) == kAuxSlotFree; }

// Long-ray record (48 B): (p, dist), (step, aux, iters, t), (shadow fog | AO dir; a fog-free
// landscape's shadow leaves the third float4 unwritten).  A shadow ray's direction is SunDirection /
// length(SunDirection) (tracing.hlsl:60-61) for every ray; an AO ray carries its own (normalised)
// direction in the fog slot, since AO rays march without fog.  The density d is not kept: a stored
// ray is live, so its next step overwrites d before anything reads it; nor is lastStep, which only
// the refinement after a hit reads (tracing.hlsl:76-79) and SKIPREFINE rays break before it.
template <int L>
__device__ __forceinline__ void long_pack(const March<L, true>& st, uint32_t t, uint32_t aux, float4* r)
{
    r[0] = make_float4(st.p.x, st.p.y, st.p.z, st.dist);
    r[1] = make_float4(st.step, __uint_as_float(aux), __uint_as_float((uint32_t)st.iters), __uint_as_float(t));
    if (aux_ao(aux)) r[2] = make_float4(st.dir.x, st.dir.y, st.dir.z, 0.0f);
    else if constexpr (March<L, true>::FOG) r[2] = make_float4(st.f.x, st.f.y, st.f.z, st.f.w);
    // no fog: a shadow ray's f is +0 throughout (march_step), so r2 is neither written nor read
}

template <int L>
__device__ __forceinline__ uint32_t long_unpack(const float4 r0, const float4 r1, const float4 r2, f3 sun_dir,
                                                March<L, true>& st, uint32_t* aux)
{
    *aux = __float_as_uint(r1.y);
    st.p = rtm::mk(r0.x, r0.y, r0.z);
    st.dist = r0.w;
    st.step = r1.x;
    st.lastStep = 0.0f; // not read (SKIPREFINE)
    st.d = 0.0f;
    st.iters = (int)__float_as_uint(r1.z);
    if (aux_ao(*aux)) {
        st.dir = rtm::mk(r2.x, r2.y, r2.z);
        st.f = {0.0f, 0.0f, 0.0f, 0.0f};
        st.fog = false;
    } else {
        st.dir = sun_dir;
        // without fog the stored f is the +0 long_pack wrote: restating it as a constant lets the
        // compiler drop f from the long-ray loops' live state
        if constexpr (March<L, true>::FOG) st.f = {r2.x, r2.y, r2.z, r2.w};
        else st.f = {0.0f, 0.0f, 0.0f, 0.0f};
        st.fog = true;
    }
    return __float_as_uint(r1.w);
}

// AO ray k of a shaded hit, at its start (AO extension, rt_shader.h ao_dir)
template <int L>
__device__ __forceinline__ void ao_begin(const Ctx& c, const ShadeHit& h, uint32_t kk, March<L, true>& st)
{
    march_begin(c, st, h.hp, 0.4f, h.prec, ao_dir(h.n, h.px, h.py, h.a, kk), false);
}

// The inputs a long shadow ray needs to finish its sample: (albedo + specular, brightness), fcolord
// (fog-live landscapes only; 0 otherwise) and (rayleigh, skyAmount): FinRec<L>::N float4 at f, a
// slot of the block's fin pool or fin[t].
template <int L>
struct FinRec {
    static constexpr uint32_t N = FogLive<L>::value ? 3u : 2u;
};
template <int L>
__device__ __forceinline__ void fin_store(float4* __restrict__ f, const ShadeHit& h)
{
    if constexpr (FogLive<L>::value) {
        f[0] = h.cb;
        f[1] = h.fog;
        f[2] = h.ray;
    } else {
        f[0] = h.cb;
        f[1] = h.ray;
    }
}

// UnitMap::fit: k_finish's arithmetic for a pixel of one sample, (0 + v * ao) * rcp(1) per channel, as
// UNORM8 (tracescreen.hlsl:67-75 with AA_SAMPLES 1), where the hit's last ray ends
__device__ __forceinline__ uint32_t fit_pixel(float4 v, float ao)
{
    const float ia = rtm::rcp(1.0f);
    return unorm8((0.0f + v.x * ao) * ia) | (unorm8((0.0f + v.y * ao) * ia) << 8) |
           (unorm8((0.0f + v.z * ao) * ia) << 16) | 0xff000000u;
}

// UnitMap::fit: store the final pixel of sample t (one sample per pixel) from a lane of any frame
__device__ __forceinline__ void fit_store(const RtConsts* k, const UnitMap& m, const FrameRays& fr, uint32_t t,
                                          uint32_t px8)
{
    const uint32_t f = frame_of(m, t), W = (uint32_t)k->width;
    const uint32_t tl = t - f * m.frame_samples;
    if (m.packed) { // out_index's packed position is a bit permutation of the sample id (one sample per pixel)
        gptr(fr.out8[f])[late(packed_index(tl))] = px8;
        return;
    }
    uint32_t px, py;
    unit_pixel(m, f, tl >> 6, t & 63u, W, (uint32_t)k->height, &px, &py);
    gptr(fr.out8[f])[(size_t)late(py) * W + px] = px8;
}

// A long ray left its loop: a shadow ray finishes its sample from its fin record (with fit and no AO,
// its pixel); an AO ray counts its occlusion for k_finish, or (fit) stores its hit's occluded pixel.
template <int L>
__device__ __forceinline__ void long_finish(const RtConsts* k, const UnitMap& m, const FrameRays& fr,
                                            const float4* __restrict__ fin, const float4* __restrict__ finp,
                                            float4* __restrict__ samples, uint32_t* __restrict__ aocc, uint32_t t,
                                            uint32_t aux, const March<L, true>& st)
{
    if (aux_ao(aux)) {
        if (st.d > 0.0f) {
            if (aux == kAuxAO) {
                // fit: the hit's one AO ray, after the shading's kFinFlag store (ordered by the push)
                if (m.fit) reinterpret_cast<uint8_t*>(aocc)[late(t)] = (uint8_t)(kFinFlag | 1u);
                // one AO ray per hit: its count has one writer, a plain byte store (no device atomic)
                else if (k->ao_samples == 1) reinterpret_cast<uint8_t*>(aocc)[late(t)] = 1u;
                else if (!(RT_DIAG_SKIP & 8)) ao_count(aocc, t);
            } else if (!(RT_DIAG_SKIP & 2)) {
                fit_store(k, m, fr, t, aux | 0xff000000u);
            }
        }
    } else {
        constexpr uint32_t FR = FinRec<L>::N;
        float4 f0, f1, fog = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (aux == kAuxFinT) { // the pool was empty: fin[t] (rare)
            const float4* f = fin + (size_t)FR * t;
            f0 = ld_fresh(f);
            if constexpr (FogLive<L>::value) fog = ld_fresh(f + 1);
            f1 = ld_fresh(f + FR - 1u);
        } else {
            f0 = ld_rec(finp, FR * aux);
            if constexpr (FogLive<L>::value) fog = ld_rec(finp, FR * aux + 1u);
            f1 = ld_rec(finp, FR * aux + FR - 1u);
        }
        const float4 v = shade_finish(k, f0, fog, f1, st.d, st.f.w);
        if (m.fit && k->ao_samples == 0) {
            if (!(RT_DIAG_SKIP & 2)) fit_store(k, m, fr, t, fit_pixel(v, 1.0f));
        } else if (!(RT_DIAG_SKIP & 4)) {
            sample_store(k, samples, t, v);
        }
    }
}

// ===========================================================================
// Fused trace (default pipeline): the primary march, the hit shading and the long
// shadow rays in ONE persistent kernel, so the latency-bound shading phases run in
// the shadow of the VALU-bound primary march instead of after it.  Each CU keeps
// two block-local queues, fed and drained by its own 16 waves:
//   hits  : the records of primary hits (hit_store; pushed by a wave when it finishes a unit),
//           a stack per block in HBM (its top lines live in the XCD's L2);
//   longs : march state of shadow rays still live after their first step (pushed
//           by a wave when it finishes a shading batch), a ring in LDS.
// A wave's next job, in priority order: march long shadows (lane refill from the
// ring) when enough are queued; shade a batch of 64 queued hits; march the next
// primary unit from the global longest-first queue.  Queue operations hold a
// per-block LDS lock.  Every hand-off stays on one CU: the producer's global stores
// (hit records, fin) complete (s_waitcnt) before the push publishes them, and the consumer
// reads them with L1-bypassing loads from the XCD's L2.  A full long ring spills to the block's
// spill stack in HBM (the same block consumes it, so the hand-off stays on one CU like the LDS
// ring's own): a block never hands work to another kernel.
constexpr uint32_t kLongRing = 570; // fills the CU's LDS: 128 KiB tables + 4 KiB plane + the ring
// A block's fin pool: slots of FinRec<L>::N float4 in HBM for the finishing inputs of its long
// shadow rays, handed out from a LIFO free list in LDS, so the few hundred slots in use at a time
// are the same lines over and over and stay in the XCD's L2 (fin[t] instead: a sparse write and a
// re-fetch per long shadow).  An empty pool falls back to fin[t].
constexpr uint32_t kFinSlots = RT_FIN_SLOTS;
// AO counter slots per block (AO_SAMPLES >= 2; the LDS the ring and the tables leave)
constexpr uint32_t kAoSlots = RT_AO_SLOTS;
static_assert(kAoSlots % 2u == 0u && kAoSlots <= 256u && kAoSlots <= RT_AO_POOL_SLOTS,
              "AO slots: pairs of u16 counters, u8 indices, a colour each in the pool");
constexpr uint32_t kLongBatch = RT_LONG_BATCH; // queued long rays that make a wave switch to them
constexpr uint32_t kCompactLive = RT_COMPACT_LIVE; // live lanes below which a dry wave hands its rays back
// After the unit queue drains (nomadplains): a long-ray wave left with at most kSegHandBack live rays
// and an empty ring hands them back, and a wave that finds at most kSegQueue rays queued marches them
// as segments of kSegLanes lanes per ray (density_nomadplains_seg: the octaves spread over the
// segment), cutting the per-step latency that sets a launch's last few hundred microseconds.
constexpr uint32_t kSegLanes = RT_SEG_LANES, kSegHandBack = RT_SEG_HANDBACK, kSegQueue = RT_SEG_QUEUE;
// a prepass task (FusedPrepass / GatedPrepass: 8 rays) is marched by kPrepassSplit waves of 64 / RT_PREPASS_LPR rays
constexpr uint32_t kPrepassSplit = RT_FUSE_RAYS_PER_TASK / (64u / RT_PREPASS_LPR);
static_assert(kPrepassSplit >= 1u && RT_PREPASS_LPR >= RT_FUSE_RAYS_PER_TASK && RT_PREPASS_LPR <= 32, "prepass lanes per ray");
// A primary unit's last few rays (nomadplains): once at most kPrimarySeg rays of an 8x8 unit are
// still marching, they continue as segments of 64 / kPrimarySeg lanes per ray (primary_seg in
// k_trace) instead of keeping 64 lanes on a few rays' octave loops.  0: off.
constexpr uint32_t kPrimarySeg = RT_PRIMARY_SEG;
static_assert(kPrimarySeg == 0u || kPrimarySeg == 4u || kPrimarySeg == 8u || kPrimarySeg == 16u, "lanes per ray");
// The instrumented (STATS) kernels take the same segment tail (their counters cost registers there:
// they spill, the product does not), so their march and noise counts pass through the product's code.
constexpr bool kStatsPrimarySeg = RT_STATS_PRIMARY_SEG != 0;

// STATS kernels: a k_trace block's march-step and hit counters (LDS atomics; the block's last wave
// adds them to the frame statistics)
struct BlockStats {
    enum { PRIMARY = 0, SHADOW = 1, AO = 2, HITS = 3, NOISE = 4, NOISE_WAVES = 5 };
    unsigned long long v[6];
    uint32_t done, pad;
};

struct TraceQueues {
    uint32_t lock;
    uint32_t h_top, pad0; // the block's hit stack (HBM, hit_cap records): records [0, h_top) are queued
    uint32_t l_head, l_tail;
    uint32_t active;  // waves inside a primary unit or a shading batch (they may still push)
    uint32_t drained; // the global unit queue is exhausted
    uint32_t pad;
    uint32_t ls_top; // the block's long-ray spill stack (HBM, long_spill_cap records): [0, ls_top) queued
    uint32_t pad1;
    uint32_t f_top;            // free slots of the block's fin pool: fin_free[0, f_top)
    uint32_t overflow;         // RT_FLAG_*: a queue push past its bound was dropped (published at exit)
    // the gated launch (GatedPrepass), per block so that no wave holds them in registers: the block's tile
    // scan position, every frame's prepass seen done, the frames whose CellDistance is seen flagged
    uint32_t gscan, gate_all, gate_cells;
    uint32_t near_end; // a wave of this block took one of the last RT_NEAR_UNITS x (wave slots) units

    float4 longs[kLongRing * kShadowRec];
    uint16_t fin_free[kFinSlots];
    uint32_t ao_ctr[kAoSlots / 2]; // AO slot s: bits 16 (s & 1) + 0..4 rays finished, + 5..9 occluded
    uint8_t ao_free[kAoSlots];     // free AO slots: ao_free[0, ao_top)
    uint32_t ao_top;
};

// A fresh read of a ring field another wave may have written: a relaxed workgroup-scope atomic
// load.  (A volatile read kept its generic pointer -- the address-space inference leaves volatile
// accesses alone -- so every ring poll was a flat load with system-scope cache bits, waiting on
// the vector memory counter too, with the fields' 64-bit flat addresses held in VGPRs.)
template <class T>
__device__ __forceinline__ T vload(const T& x)
{
    return __hip_atomic_load(&x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ void q_lock(uint32_t* lock, uint32_t lane)
{
    if (lane == 0) {
        while (atomicCAS(lock, 0u, 1u) != 0u) __builtin_amdgcn_s_sleep(1);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ void q_unlock(uint32_t* lock, uint32_t lane)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) atomicExch(lock, 0u);
}

// Diagnostic builds only (rt_variants.h): the live-lane histogram and k_trace's per-wave timeline
// (RT_WT_FIELDS u64 per wave slot, scripts/wave_trace.py).
RT_DIAG_LIVE_HIST(__device__ unsigned long long g_live_hist[65];)
WT(__device__ unsigned long long g_wave_trace[RT_WT_MAX_WAVES * RT_WT_FIELDS];)

// k_trace's block: 16 waves (4 per SIMD, 128 VGPRs each) for the fog-free landscapes; the fog-live
// one (greenrocks: fog state in every march and record) and simple (its two-plane density) need
// more than 128 VGPRs and run 12 waves (3 per SIMD, up to 168 VGPRs) instead of spilling.
template <int L>
struct TraceThreads {
    static constexpr uint32_t value = 64u * ((L == RT_GREENROCKS || L == RT_SIMPLE) ? RT_TRACE_WAVES_WIDE : RT_TRACE_WAVES_FAST);
};
static_assert(RT_CTR_FIRST + RT_TRACE_WAVES_FAST <= RT_CTR_BYTES / 4 && RT_CTR_FIRST + RT_TRACE_WAVES_WIDE <= RT_CTR_BYTES / 4,
              "a first-unit counter per wave slot inside the zeroed work counters");

// GATED: the gated launch's instantiation (GatedPrepass, opt-in RT_DEVICE_GATED; nomadplains, no STATS).  The
// product instantiations (GATED false) carry none of its task, scan and claim paths.
template <int L, bool STATS, bool GATED = false>
__global__ void __launch_bounds__(TraceThreads<L>::value) k_trace(const RtConsts* __restrict__ k, const FrameTable* __restrict__ ft,
                                                const uint32_t* __restrict__ perm2d,
                                                const float4* __restrict__ grad,
                                                UnitMap m, const uint32_t* __restrict__ order,
                                                uint64_t* __restrict__ hitmask, float4* __restrict__ samples,
                                                float4* __restrict__ fin, float4* __restrict__ finpool,
                                                float4* __restrict__ cpool,
                                                float4* __restrict__ hitq,
                                                float4* __restrict__ spill_long, uint32_t hit_cap,
                                                uint32_t long_spill_cap,
                                                uint32_t* __restrict__ aocc, uint32_t* __restrict__ counters,
                                                RtStats* stats, uint32_t long_batch, uint32_t refill_idle,
                                                uint32_t compact_live, uint32_t long_ring_cap, uint32_t fin_slots,
                                                FusedPrepass np, GatedPrepass gp)
{
    // one LDS array (the noise image at address 0, then the frame table, the rings and the STATS
    // kernels' block counters)
    __shared__ __attribute__((aligned(16))) uint32_t
        lds[kNoiseLdsWords + (sizeof(FrameRays) + sizeof(TraceQueues) + sizeof(BlockStats)) / 4];
    FrameRays& s_fr = *reinterpret_cast<FrameRays*>(lds + kNoiseLdsWords);
    TraceQueues& q = *reinterpret_cast<TraceQueues*>(lds + kNoiseLdsWords + sizeof(FrameRays) / 4);
    BlockStats& s_st =
        *reinterpret_cast<BlockStats*>(lds + kNoiseLdsWords + (sizeof(FrameRays) + sizeof(TraceQueues)) / 4);
    frame_rays_load(s_fr, ft, m.n_frames);
    if (threadIdx.x == 0) {
        q.lock = 0;
        q.h_top = 0;
        q.l_head = q.l_tail = 0;
        q.active = 0;
        q.drained = 0;
        q.ls_top = 0;
        q.f_top = fin_slots;
        q.overflow = 0;
        q.gscan = q.gate_all = q.gate_cells = 0;
        q.near_end = 0;
        if constexpr (STATS) s_st = BlockStats{};
    }
    for (uint32_t i = threadIdx.x; i < fin_slots; i += blockDim.x) q.fin_free[i] = (uint16_t)i;
    for (uint32_t i = threadIdx.x; i < kAoSlots; i += blockDim.x) {
        q.ao_free[i] = (uint8_t)i;
        if (i < kAoSlots / 2u) q.ao_ctr[i] = 0u;
    }
    if (threadIdx.x == 0) q.ao_top = kAoSlots;
    load_noise_lds(lds, perm2d, grad, k);
    const uint32_t lane = __lane_id(); // v_mbcnt of constants: rematerialisable (threadIdx & 63 spilled)
    Ctx c = make_ctx(k, lds); // k: frame-invariant constants (per-frame ones: frame_ctx / s_fr)
    if constexpr (STATS) c.nz.lds_calls = (__attribute__((address_space(3))) unsigned long long*)&s_st.v[BlockStats::NOISE];
    const uint32_t W = (uint32_t)k->width, H = (uint32_t)k->height, aa = (uint32_t)k->aa_samples;
    const int max_steps = k->max_steps;
    // the primary march's sky exit (rt_shader.h sky_exit; rt_variants.h RT_SKY_EXIT): the product kernels only, the
    // STATS kernels march every ray out (their step and noise counts are the oracle's)
    constexpr bool kSky = RT_SKY_EXIT && L == RT_NOMADPLAINS && (!STATS || RT_SKY_EXIT_STATS);
    const uint32_t n_total = (uint32_t)__builtin_amdgcn_readfirstlane(m.n_units * m.n_frames); // units (an SGPR)
    // this block's hit stack and long-ray spill stack (hit_cap / long_spill_cap records per block)
    constexpr uint32_t HR = HitRec<L>::N;
    float4* const hq = hitq + (size_t)blockIdx.x * hit_cap * HR;
    float4* const finp = finpool + (size_t)blockIdx.x * kFinSlots * FinRec<L>::N;
    float4* const cpl = cpool + (size_t)blockIdx.x * RT_AO_POOL_SLOTS; // fitm: the AO slots' hit colours
    float4* const lspill = spill_long + (size_t)blockIdx.x * long_spill_cap * kShadowRec;
    // queued work of the block: long rays in the LDS ring + spill stack, hits in the hit queue
    auto queued_long = [&]() { return vload(q.l_tail) - vload(q.l_head) + vload(q.ls_top); };
    auto queued_hits = [&]() { return vload(q.h_top); };
    // STATS: march steps and hits go to the block's LDS counters (no VGPRs held across the loops)
    auto stat = [&](int i, uint32_t v) {
        if constexpr (STATS) atomicAdd(&s_st.v[i], (unsigned long long)v);
    };

    // wt: begin, end, t_unit, t_shade, t_long, n_unit, n_shade, n_long, last unit end, t_idle, hw_id, xcc_id,
    // loop iterations, long rays finished (lane), max long-ray iters (lane), last iteration, max primary iters (lane)
    WT(unsigned long long wt[RT_WT_FIELDS] = {}; wt[10] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
       wt[11] = __builtin_amdgcn_s_getreg((31 << 11) | 20); uint32_t wl_rays = 0, wl_maxit = 0, wp_maxit = 0;)
    // push the lanes' long rays (shadow continuations or AO starts) to the ring, or to the
    // block's spill stack when the LDS ring is full (stored before the tail publishes them)
    auto push_recs = [&](bool want, auto pack) {
        const uint64_t lb = __ballot(want);
        if (!lb) return;
        const uint32_t n = (uint32_t)__popcll(lb), rank = lane_rank(lb);
        q_lock(&q.lock, lane);
        const uint32_t lh = vload(q.l_head), lt = vload(q.l_tail);
        if (lt - lh + n <= long_ring_cap) {
            if (want) pack(&q.longs[((lt + rank) % kLongRing) * kShadowRec]);
            if (lane == 0) q.l_tail = lt + n;
        } else {
            // the spill stack's bound (rt_spill_caps) holds by the work priorities; a push past it is
            // dropped and flagged (rt_device_check), never written over queued rays
            const uint32_t stl = (uint32_t)__builtin_amdgcn_readfirstlane(vload(q.ls_top));
            const bool fits = stl + n <= long_spill_cap;
            if (want && fits) pack(lspill + (size_t)(stl + rank) * kShadowRec);
            __builtin_amdgcn_s_waitcnt(0);
            if (lane == 0) {
                q.ls_top = fits ? stl + n : stl;
                q.overflow |= fits ? 0u : RT_FLAG_SPILL_OVERFLOW;
            }
        }
        q_unlock(&q.lock, lane);
    };
    auto push_long = [&](bool want, const March<L, true>& st, uint32_t t, uint32_t aux) {
        push_recs(want, [&](float4* r) { long_pack(st, t, aux, r); });
    };

    // the fin pool slots of finished shadow rays (idle lanes whose aux is a slot) go back to the free
    // list; the lock is held
    auto free_fin_locked = [&](bool live, uint32_t& aux) {
        const bool pend = !live && aux < kFinSlots;
        const uint64_t pb = __ballot(pend);
        if (pb) {
            const uint32_t top = vload(q.f_top);
            if (pend) {
                q.fin_free[top + lane_rank(pb)] = (uint16_t)aux;
                aux = kAuxAO;
            }
            if (lane == 0) q.f_top = top + (uint32_t)__popcll(pb);
        }
        if constexpr (kAoSlots > 0u) { // and the AO slots of completed counts
            const bool pa = !live && aux_slot_free(aux);
            const uint64_t ab = __ballot(pa);
            if (ab) {
                const uint32_t top = vload(q.ao_top);
                if (pa) {
                    q.ao_free[top + lane_rank(ab)] = (uint8_t)(aux & 255u);
                    aux = kAuxAO;
                }
                if (lane == 0) q.ao_top = top + (uint32_t)__popcll(ab);
            }
        }
    };
    // an AO ray with a counter slot left the march: count it; the ray that completes the hit's count stores
    // it (one byte that only this lane writes), clears the slot and keeps it to free (kAuxSlotFree)
    auto ao_slot_finish = [&](const March<L, true>& st, uint32_t t, uint32_t& aux) {
        const uint32_t sl = aux & 255u, sh = (sl & 1u) * 16u;
        const uint32_t occ1 = st.d > 0.0f ? 1u : 0u;
        const uint32_t old = atomicAdd(&q.ao_ctr[sl >> 1], (1u | (occ1 << 5)) << sh) >> sh;
        if ((old & 31u) + 1u == (uint32_t)k->ao_samples) {
            const uint32_t occ = ((old >> 5) & 31u) + occ1;
            if (m.fitm && !(old & (1u << 10))) { // no long shadow: the pixel, from the colour the shading left
                const float4 v = ld_rec(cpl, sl);
                const uint32_t at = __float_as_uint(v.w);
                if (!(RT_DIAG_SKIP & 2)) gptr(s_fr.out8[at >> 23])[at & 0x7fffffu] = fit_pixel(v, ao_factor(occ, k->ao_samples));
            } else if (occ != 0u) { // k_finish's count (fitm: after the shading's kFinFlag)
                reinterpret_cast<uint8_t*>(aocc)[late(t)] = (uint8_t)((m.fitm ? kFinFlag : 0u) | occ);
            }
            atomicAnd(&q.ao_ctr[sl >> 1], ~(0xffffu << sh));
            aux = kAuxSlotFree | sl;
        } else {
            aux = kAuxAO;
        }
    };

    // ---- a batch of long rays, lane refill from the ring ----
    auto do_shadow = [&]() {
        March<L, true> st;
        st.d = 0.0f;
        st.iters = 0;
        bool live = false;
        uint32_t t = 0, aux = kAuxAO; // aux: the lane's ray (long_pack); on an idle lane, a fin slot to free
        Ctx cl = c; // cl.eye: the frame of the lane's ray (set on refill)
        cl.nz.phase = RT_PHASE_LONG;
        for (;;) {
            if (live && !march_live<L, true, true>(cl, st, aux_ao(aux) ? RT_AO_END : 100.0f, 0)) {
                WT(wl_rays++; wl_maxit = max(wl_maxit, (uint32_t)st.iters);)
                stat(aux_ao(aux) ? BlockStats::AO : BlockStats::SHADOW, (uint32_t)st.iters);
                if (kAoSlots > 0u && aux_ao_slot(aux)) ao_slot_finish(st, t, aux);
                else long_finish<L>(k, m, s_fr, fin, finp, samples, aocc, t, aux, st);
                live = false;
            }
            const uint64_t idle = __ballot(!live);
            const uint32_t nidle = (uint32_t)__popcll(idle);
            if (nidle >= refill_idle && queued_long() != 0u) {
                q_lock(&q.lock, lane);
                free_fin_locked(live, aux);
                const uint32_t head = vload(q.l_head), tail = vload(q.l_tail);
                const uint32_t take = (tail - head) < nidle ? (tail - head) : nidle;
                // the block's spill stack tops up what the LDS ring cannot give (from its top)
                const uint32_t sl = vload(q.ls_top);
                const uint32_t more = sl < nidle - take ? sl : nidle - take;
                const uint32_t rank = lane_rank(idle);
                const bool mine = ((idle >> lane) & 1ull) && rank < take + more;
                auto take_ray = [&](float4 r0, float4 r1, float4 r2) {
                    t = long_unpack(r0, r1, r2, rtm::mk(0.0f, 0.0f, 0.0f), st, &aux);
                    const float* fr = s_fr.v[frame_of(m, t)];
                    cl.eye = rtm::mk(fr[0], fr[1], fr[2]);
                    if (!aux_ao(aux)) st.dir = rtm::mk(fr[3], fr[4], fr[5]);
                    live = true;
                };
                if (mine && rank < take) {
                    const float4* r = &q.longs[((head + rank) % kLongRing) * kShadowRec];
                    take_ray(r[0], r[1], r[2]);
                } else if (mine) {
                    const uint32_t ri = (sl - more + rank - take) * kShadowRec;
                    take_ray(ld_rec(lspill, ri), ld_rec(lspill, ri + 1u), ld_rec(lspill, ri + 2u));
                }
                if (more) __builtin_amdgcn_s_waitcnt(0); // the spill records are read before a push reuses them
                if (lane == 0) {
                    q.l_head = head + take;
                    q.ls_top = sl - more;
                }
                q_unlock(&q.lock, lane);
            }
            const uint64_t lv = __ballot(live);
            // The ring ran dry and few lanes are left: rather than march them on
            // mostly empty lanes, hand them back to the ring (another wave will merge
            // them with new rays) and go do other work, while there still is some.
            const bool drained_now = vload(q.drained) != 0u;
            bool hand_back = lv != 0ull && (uint32_t)__popcll(lv) < compact_live && queued_long() == 0u && !drained_now;
            if constexpr (L == RT_NOMADPLAINS && kSegLanes > 0u) // after the drain: few rays go to segment waves
                hand_back = hand_back || (drained_now && lv != 0ull && (uint32_t)__popcll(lv) <= kSegHandBack &&
                                          queued_long() == 0u);
            if (lv == 0ull || hand_back) {
                if (__ballot(!live && (aux < kFinSlots || aux_slot_free(aux)))) {
                    q_lock(&q.lock, lane);
                    free_fin_locked(live, aux);
                    q_unlock(&q.lock, lane);
                }
                if (hand_back) push_long(live, st, t, aux);
                c.nz.calls = cl.nz.calls;
                return;
            }
            RT_DIAG_LONG_STEPS(if (live && (RT_COUNT_LONG_STEPS == 1 || (RT_COUNT_LONG_STEPS == 2) == (vload(q.drained) != 0u))) {
                cl.nz.phase = RT_COUNT_PHASE;
                count_noise(cl.nz);
                cl.nz.phase = RT_PHASE_LONG;
            })
            WT(wt[26]++;)
            if (live) march_step<L, true, true>(cl, st);
        }
    };

    // ---- after the drain: up to 64 / kSegLanes queued long rays, a segment of lanes per ray ----
    auto do_shadow_seg = [&]() {
        if constexpr (L == RT_NOMADPLAINS && kSegLanes > 0u) {
            constexpr uint32_t LPR = kSegLanes ? kSegLanes : 8u, RPW = 64u / LPR; // (8 only to compile the discarded branch when off)
            // late(): the segment's lane values (and the octave scales derived from them) are formed
            // here, not hoisted into the kernel's prologue where they would stay live throughout
            March<L, true> st;
            st.d = 0.0f;
            st.iters = 0;
            uint32_t t = 0, aux = kAuxAO;
            bool live = false;
            Ctx cl = c;
            cl.nz.phase = RT_PHASE_LONG;
            q_lock(&q.lock, lane);
            const uint32_t head = vload(q.l_head), tail = vload(q.l_tail);
            const uint32_t take = (tail - head) < RPW ? (tail - head) : RPW;
            const uint32_t sl = vload(q.ls_top);
            const uint32_t more = sl < RPW - take ? sl : RPW - take;
            if (const uint32_t grp = late(lane) / LPR; grp < take + more) { // every lane of the segment unpacks the same record
                float4 r0, r1, r2;
                if (grp < take) {
                    const float4* r = &q.longs[((head + grp) % kLongRing) * kShadowRec];
                    r0 = r[0];
                    r1 = r[1];
                    r2 = r[2];
                } else {
                    const uint32_t ri = (sl - more + grp - take) * kShadowRec;
                    r0 = ld_rec(lspill, ri);
                    r1 = ld_rec(lspill, ri + 1u);
                    r2 = ld_rec(lspill, ri + 2u);
                }
                t = long_unpack(r0, r1, r2, rtm::mk(0.0f, 0.0f, 0.0f), st, &aux);
                const float* fr = s_fr.v[frame_of(m, t)];
                cl.eye = rtm::mk(fr[0], fr[1], fr[2]);
                if (!aux_ao(aux)) st.dir = rtm::mk(fr[3], fr[4], fr[5]);
                live = true;
            }
            __builtin_amdgcn_s_waitcnt(0); // the spill records are read before their slots can be reused
            if (lane == 0) {
                q.l_head = head + take;
                q.ls_top = sl - more;
            }
            q_unlock(&q.lock, lane);
            const uint32_t lid = late(lane);
            const uint32_t j = lid & (LPR - 1u), base = lid & ~(LPR - 1u);
            const SegOctaves<LPR> g = seg_octaves<LPR>(c, j);
            for (;;) {
                if (live && !march_live<L, true, true>(cl, st, aux_ao(aux) ? RT_AO_END : 100.0f, 0)) {
                    if (j == 0u) { // every lane of the segment holds the same ray: its first lane finishes it
                        stat(aux_ao(aux) ? BlockStats::AO : BlockStats::SHADOW, (uint32_t)st.iters);
                        if (kAoSlots > 0u && aux_ao_slot(aux)) ao_slot_finish(st, t, aux);
                        else long_finish<L>(k, m, s_fr, fin, finp, samples, aocc, t, aux, st);
                    }
                    live = false;
                }
                if (!__ballot(live)) break;
                WT(wt[25]++;)
                if (live) {
                    auto dens = [&](f3 q0) {
                        uint32_t used;
                        const float d = density_nomadplains_seg<LPR>(cl, g, q0, j, base, &used);
                        if constexpr (STATS) { // the same noise count as density_nomadplains: octaves + steep noise
                            if (j == 0u) atomicAdd(&s_st.v[BlockStats::NOISE], (unsigned long long)(used + 1u));
                            if (lane == (uint32_t)__builtin_ctzll(__ballot(1)))
                                atomicAdd(&s_st.v[BlockStats::NOISE_WAVES], (unsigned long long)SegOctaves<LPR>::R);
                        }
                        return d;
                    };
                    march_step_with<L, true, true>(cl, st, dens);
                }
            }
            // the segments' finished shadows return their fin pool slots (one lane per segment holds it)
            uint32_t fa = j == 0u ? aux : kAuxAO;
            if (__ballot(fa < kFinSlots || aux_slot_free(fa))) {
                q_lock(&q.lock, lane);
                free_fin_locked(false, fa);
                q_unlock(&q.lock, lane);
            }
        }
    };

    // ---- a primary unit's last <= kPrimarySeg live rays, a segment of 64 / kPrimarySeg lanes per ray ----
    // lb: the unit's live rays; st: every lane's march (the finished rays' final states stay in
    // their lanes).  The live rays' states move to their segments (ray r of lb to lanes r*LPR ..),
    // march there with the density's octaves spread over the segment (density_nomadplains_seg,
    // bit-identical to density_nomadplains; pow_nonneg_wave for the step factor, bit-identical to
    // pow_nonneg) and come back when every segment's ray has left the march.
    auto primary_seg = [&](const Ctx& cf, March<L, true>& st, bool lv, uint64_t lb, float spx, float spy, bool sky) {
        if constexpr (L == RT_NOMADPLAINS && kPrimarySeg > 0u && (!STATS || kStatsPrimarySeg)) {
            constexpr uint32_t LPR = 64u / (kPrimarySeg ? kPrimarySeg : 8u);
            const uint32_t lid = late(lane);
            const uint32_t j = lid & (LPR - 1u), grp = lid / LPR, base = lid & ~(LPR - 1u);
            const uint32_t n = (uint32_t)__popcll(lb);
            // the lane of live ray grp (scalar loop over lb's <= kPrimarySeg set bits)
            uint32_t src = lid;
            uint64_t rem = lb;
            for (uint32_t r = 0; r < n; ++r) {
                const uint32_t sl = (uint32_t)__builtin_ctzll(rem);
                rem &= rem - 1ull;
                src = grp == r ? sl : src;
            }
            March<L, true> sg;
            sg.p = rtm::mk(__shfl(st.p.x, (int)src), __shfl(st.p.y, (int)src), __shfl(st.p.z, (int)src));
            sg.dir = rtm::mk(__shfl(st.dir.x, (int)src), __shfl(st.dir.y, (int)src), __shfl(st.dir.z, (int)src));
            sg.sd = __shfl(st.sd, (int)src);
            sg.dist = __shfl(st.dist, (int)src);
            sg.step = __shfl(st.step, (int)src);
            sg.lastStep = __shfl(st.lastStep, (int)src);
            sg.d = __shfl(st.d, (int)src);
            sg.iters = __shfl(st.iters, (int)src);
            sg.f = {0.0f, 0.0f, 0.0f, 0.0f}; // no fog in nomadplains (March::FOG is false)
            sg.fog = false;
            bool live = grp < n;
            const SegOctaves<LPR> g = seg_octaves<LPR>(cf, j);
            for (;;) {
                if (live && !march_live<L, true, false>(cf, sg, RT_CAMERA_FAR, max_steps)) live = false;
                if constexpr (kSky) { // (a segment's lanes hold one ray: they leave together)
                    if (live && sky && sky_exit(sg.p.y, sg.dir.y, sg.dist)) live = false;
                }
                if (!__ballot(live)) break;
                if (live) {
                    auto dens = [&](f3 q0) {
                        uint32_t used;
                        const float d = density_nomadplains_seg<LPR, true>(cf, g, q0, j, base, &used);
                        if constexpr (STATS) { // the same noise count as density_nomadplains: octaves + steep noise
                            if (j == 0u) atomicAdd(&s_st.v[BlockStats::NOISE], (unsigned long long)(used + 1u));
                            if (lane == (uint32_t)__builtin_ctzll(__ballot(1)))
                                atomicAdd(&s_st.v[BlockStats::NOISE_WAVES], (unsigned long long)SegOctaves<LPR>::R);
                        }
                        return d;
                    };
                    march_step_with<L, true, false>(cf, sg, dens);
                }
            }
            // back to the rays' lanes (the march changes only these fields)
            const int back = (int)(lane_rank(lb) * LPR);
            const float sd = __shfl(sg.sd, back), dist = __shfl(sg.dist, back), step = __shfl(sg.step, back);
            const float last = __shfl(sg.lastStep, back), d = __shfl(sg.d, back);
            const int iters = __shfl(sg.iters, back);
            if (lv) {
                st.sd = sd;
                st.dist = dist;
                st.step = step;
                st.lastStep = last;
                st.d = d;
                st.iters = iters;
            }
            // every ray's origin and direction again, as march_begin formed them (the pixel ray,
            // normalised): they are not held across the segments' march
            f3 p, dir;
            get_pixel_ray(cf, spx, spy, &p, &dir);
            st.p = p;
            st.dir = rtm::scale(dir, rtm::rcp(rtm::length(dir)));
        }
    };

    // ---- a batch of up to 64 queued hits: shading + first shadow step ----
    auto do_shade = [&]() {
        q_lock(&q.lock, lane);
        const uint32_t top = vload(q.h_top);
        const uint32_t take = top < 64u ? top : 64u;
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0;
        if (lane < take) {
            const uint32_t ri = (top - take + lane) * HR;
            r0 = ld_rec(hq, ri);
            if constexpr (HR == 3u) {
                r1 = ld_rec(hq, ri + 1u);
                r2 = ld_rec(hq, ri + 2u);
            }
        }
        __builtin_amdgcn_s_waitcnt(0); // read before the slots can be reused
        if (lane == 0) q.h_top = top - take;
        q_unlock(&q.lock, lane);
        const uint32_t t = __float_as_uint(HR == 3u ? r2.w : r0.w);
        March<L, true> st;
        bool more = false;
        uint32_t aux = kAuxAO;
        uint32_t ao_aux = kAuxAO; // the hit's AO ray: counted (kAuxAO) or carrying its occluded pixel (fit)
        const bool valid = lane < take;
        // AO_SAMPLES >= 2: a counter slot per hit (LDS), popped from the free list (none left: kAuxAO)
        if (kAoSlots > 0u && k->ao_samples >= 2) {
            const uint64_t vb = __ballot(valid);
            if (vb) {
                q_lock(&q.lock, lane);
                const uint32_t top = vload(q.ao_top), n = (uint32_t)__popcll(vb), rank = lane_rank(vb);
                const uint32_t got = n < top ? n : top;
                if (valid && rank < got) ao_aux = kAuxAOSlot | (uint32_t)q.ao_free[top - 1u - rank];
                if (lane == 0) q.ao_top = top - got;
                q_unlock(&q.lock, lane);
            }
        }
        ShadeHit h;
        per_frame(valid, valid ? frame_of(m, t) : 0u, [&](uint32_t f) {
            Ctx cf = frame_ctx(c, ft, f);
            cf.nz.phase = RT_PHASE_SHADE;
            h = shade_hit<L>(cf, m, r0, r1, r2, t, t - f * m.frame_samples, st);
            c.nz.calls = cf.nz.calls;
            more = h.more;
            if (!more) {
                const float4 v = shade_finish(k, h.cb, h.fog, h.ray, st.d, st.f.w);
                if (m.fit) {
                    // the pixel is final now (no AO), or its unoccluded value is (ao_factor(0, 1) = 1) and
                    // the AO ray carries the occluded one (ao_factor(1, 1)); no sample, no k_finish
                    if (!(RT_DIAG_SKIP & 2)) {
                        const uint32_t tl = t - f * m.frame_samples; // (one sample per pixel)
                        gptr(ft->out8[f])[m.packed ? late(packed_index(tl)) : late(h.py) * W + h.px] = fit_pixel(v, 1.0f);
                    }
                    if (k->ao_samples) ao_aux = kAuxAOCand | (fit_pixel(v, ao_factor(1u, 1)) & 0xffffffu);
                } else if (m.fitm && aux_ao_slot(ao_aux)) {
                    // the colour the AO ray completing the count finishes with, and where: frame << 23 | pixel
                    const uint32_t tl = t - f * m.frame_samples;
                    cpl[late(ao_aux & 255u)] =
                        make_float4(v.x, v.y, v.z, __uint_as_float((f << 23) | (m.packed ? packed_index(tl) : h.py * W + h.px)));
                } else if (!(RT_DIAG_SKIP & 4)) {
                    sample_store(k, samples, t, v);
                }
                stat(BlockStats::SHADOW, (uint32_t)st.iters);
            }
            // the long shadows' finishing inputs: a fin pool slot each (this frame's lanes are the
            // active ones: the first of them takes the lock), fin[t] when the pool is empty
            const uint64_t mb = __ballot(more);
            if (mb) {
                const uint32_t lead = (uint32_t)__builtin_ctzll(__ballot(1));
                q_lock(&q.lock, lane - lead);
                const uint32_t top = vload(q.f_top), n = (uint32_t)__popcll(mb), rank = lane_rank(mb);
                const uint32_t got = n < top ? n : top;
                if (more) aux = rank < got ? (uint32_t)q.fin_free[top - 1u - rank] : kAuxFinT;
                if (lane == lead) q.f_top = top - got;
                q_unlock(&q.lock, lane - lead);
                if (more && !(RT_DIAG_SKIP & 16)) fin_store<L>(aux == kAuxFinT ? fin + (size_t)FinRec<L>::N * t : finp + (size_t)FinRec<L>::N * aux, h);
            }
        });
        // fitm: the hits whose pixel the AO counter's completion does not store (a long shadow, or no slot)
        // are k_finish's.  Plain stores, no atomics (a device-scope atomic costs a 32-B HBM write on gfx950,
        // L2 or not: scripts/ubench_atomic.hip): the sample's aocc byte becomes kFinFlag and the unit's
        // hitmask word, zero from the unit, becomes nonzero (every writer stores the same value); a long
        // shadow's slot marks it (bit 10: its completion stores the flagged count).  fit with its one AO ray: the
        // hits with a long shadow are k_finish's in the same way (their AO ray adds its count to the flag,
        // long_finish)
        const bool kfin = valid && ((m.fit && k->ao_samples && more) || (m.fitm && (more || !aux_ao_slot(ao_aux))));
        if (kfin) {
            reinterpret_cast<uint8_t*>(aocc)[late(t)] = (uint8_t)kFinFlag;
            hitmask[t >> 6] = 1ull;
        }
        if (m.fitm && more && aux_ao_slot(ao_aux))
            atomicOr(&q.ao_ctr[(ao_aux & 255u) >> 1], (1u << 10) << ((ao_aux & 1u) * 16u));
        if (__ballot(more)) {
            __builtin_amdgcn_s_waitcnt(0); // the fin record is in L2 before the ray is visible
            push_long(more, st, t, aux);
        }
        // AO extension: the hit's AO rays start as long rays (fit: after its unoccluded pixel is stored,
        // which an occluded AO ray overwrites)
        if (m.fit || m.fitm) __builtin_amdgcn_s_waitcnt(0);
        for (int kk = 0; kk < k->ao_samples; ++kk) {
            March<L, true> ao;
            if (valid) ao_begin(c, h, (uint32_t)kk, ao);
            push_long(valid, ao, t, ao_aux);
        }
    };

    // ---- a task of the NEXT batch's camerarays prepass (FusedPrepass; camerarays.hlsl:12-21) ----
    // 8 rays, one 8-lane segment each (ray r on lanes 8r..8r+7), marched as k_camerarays_group marches
    // them: the octaves of each density sample spread over the segment (density_nomadplains_seg,
    // bit-identical to density_nomadplains), that frame's camerarays constants, frame 0's launch
    // constants.  The 8 results form one 128-B line of CameraResults, stored whole by one sc1
    // instruction; after the store is acknowledged the task adds 8 to ctl[1] (the next k_order polls it).
    // own (the gated launch, GatedPrepass): a task of THIS batch's prepass (pft = ft); after its line it
    // flags the task (sc1 store) and adds 8 to its frame's ray counter; the frame's last task derives the
    // frame's CellDistance (the API's array: units compute their own cells' brackets, gate_ready)
    auto do_prepass = [&](const FrameTable* __restrict__ pft, uint32_t qt, bool own) {
        if constexpr (L == RT_NOMADPLAINS) {
            constexpr uint32_t LPR = RT_PREPASS_LPR, RPW = 64u / LPR; // lanes per ray, rays per wave
            constexpr uint32_t WPF = RT_CAMERA_RES * RT_CAMERA_RES / RPW;   // waves per frame
            const uint32_t f = qt / WPF;
            const uint32_t ray0 = (qt - f * WPF) * RPW;
            const uint32_t ray = ray0 + late(lane) / LPR;
            const uint32_t lid = late(lane);
            const uint32_t j = lid & (LPR - 1u), base = lid & ~(LPR - 1u);
            Ctx cp = c;
            cp.k = pft->kcam[0];
            cp.kf = (KPtr)pft->kcam[f];
            cp.eye = rtm::mk(uniform_f(cp.kf->eye[0]), uniform_f(cp.kf->eye[1]), uniform_f(cp.kf->eye[2]));
            cp.sun = rtm::mk(uniform_f(cp.kf->sun[0]), uniform_f(cp.kf->sun[1]), uniform_f(cp.kf->sun[2]));
            const uint32_t tx = ray % RT_CAMERA_RES, ty = ray / RT_CAMERA_RES;
            const float r31 = rtm::rcp(31.0f);
            const uint32_t pxs = (uint32_t)(((float)tx * r31) * cp.k->screen[0]);
            const uint32_t pys = (uint32_t)(((float)ty * r31) * cp.k->screen[1]);
            f3 p, dir;
            get_pixel_ray(cp, (float)pxs, (float)pys, &p, &dir);
            March<L, false> st;
            march_begin(cp, st, p, RT_CAMERA_NEAR, 2.0f, dir);
            const SegOctaves<LPR> g = seg_octaves<LPR>(cp, j);
            __builtin_amdgcn_s_setprio(RT_FUSE_PRIO); // latency-bound: the next batch's k_order waits for these rays
            while (march_live<L, false, true>(cp, st, RT_CAMERA_FAR, 0)) {
                auto dens = [&](f3 q0) {
                    uint32_t used;
                    return density_nomadplains_seg<LPR, false>(cp, g, q0, j, base, &used);
                };
                march_step_with<L, false, true>(cp, st, dens);
            }
            __builtin_amdgcn_s_setprio(0);
            RayResult rr = march_result(st);
            if (rr.density < 0.0f) rr.pd.w = RT_CAMERA_FAR;
            if (j == 0u) {
                typedef float v4f __attribute__((ext_vector_type(4)));
                const v4f v = {rr.pd.x, rr.pd.y, rr.pd.z, rr.pd.w};
                float4* dst = pft->cam[f] + ray;
                asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(dst), "v"(v) : "memory");
            }
            asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
            if (!own) {
                if (lane == 0) __hip_atomic_fetch_add(np.ctl + 1, RPW, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            typedef uint32_t __attribute__((address_space(1))) guint;
            guint* gf = (guint*)(gp.gate + f * RT_GATE_WORDS);
            uint32_t old = 0;
            if (lane == 0) {
                const uint32_t task = ray0 / RT_FUSE_RAYS_PER_TASK; // = ray row * 4 + ray column / 8
                // a task's last wave (its add to the task's counter returned the other waves' rays) flags it;
                // the earlier waves' lines were acknowledged before their adds
                bool whole = true;
                if constexpr (RPW < RT_FUSE_RAYS_PER_TASK)
                    whole = __hip_atomic_fetch_add(gf + RT_GATE_TASKS + task, RPW, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT) == RT_FUSE_RAYS_PER_TASK - RPW;
                if (whole) {
                    __hip_atomic_fetch_or(gf + (task >> 5), 1u << (task & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    old = __hip_atomic_fetch_add(gf + RT_GATE_CTR, (uint32_t)RT_FUSE_RAYS_PER_TASK, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            if ((uint32_t)__builtin_amdgcn_readfirstlane(old) == RT_CAMERA_RES * RT_CAMERA_RES - RT_FUSE_RAYS_PER_TASK) {
                // the frame's last task (its add returned last): every ray is in.  Its CellDistance (8-B sc1
                // stores), waited, then the cells flag: later units read their brackets from it (gate_cells)
                if (gp.debug & 2u) { // (RT_DEVICE_DEBUG_GATE_STRESS: late, ~200 us of the 100 MHz clock)
                    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
                    while (__builtin_amdgcn_s_memrealtime() - t0 < 20000ull) __builtin_amdgcn_s_sleep(8);
                }
                const float4* cam = pft->cam[f];
                typedef unsigned long long __attribute__((address_space(1))) gu64;
                gu64* cells = (gu64*)pft->cells[f];
                for (uint32_t c = late(lane); c < RT_CAMERA_RES * RT_CAMERA_RES; c += 64u) {
                    const float2 b = cell_bracket([&](int x, int y) { return cam_depth_sc1(cam, x, y); },
                                                  (int)(c % RT_CAMERA_RES), (int)(c / RT_CAMERA_RES));
                    __hip_atomic_store(cells + c, (unsigned long long)__float_as_uint(b.x) |
                                                      ((unsigned long long)__float_as_uint(b.y) << 32),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
                if (lane == 0) __hip_atomic_store(gf + RT_GATE_CTR + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    };

    // ---- the gated launch (GatedPrepass): which unit next? ----
    // Units are claimed by tile, in k_order's longest-first order, from the tiles whose prepass rays are in:
    // the scan starts at the first tile with units left (counters[RT_CTR_SCAN]), reads 64 order entries
    // and their claim counters (claims[i]: units of order entry i taken, atomic adds) per step, and takes the
    // first unit of the first READY tile with units left.  A tile is ready when every task (8 rays of a row)
    // holding a CameraResults ray its cells' setTargetDepths reads has set its bit in the frame's task mask
    // (rows cy0 - 2 .. cy1 + 2, columns cx0 - 2 .. cx1 + 2 of its pixels' cells; the cell index grows with
    // the pixel, so the corner pixels bound them).  So units run in the longest-first order among the ready
    // ones, on any block (no unit waits in a block that took it).  sc1 loads throughout (the hand-off: a
    // task wave stored its line sc1 and waited before its mask bit).
    typedef const uint32_t __attribute__((address_space(1))) gcuint;
    auto ld_sc1 = [&](const uint32_t* p) {
        return __hip_atomic_load((gcuint*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    // tile order entry e (frame << 24 | shard tile) against its frame's task mask w0..w3
    auto tile_ready = [&](uint32_t e, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) -> bool {
        const uint32_t f = e >> 24, first = m.frame_rot ? (m.tile_first + f) % m.tile_stride : m.tile_first;
        const uint32_t T = (e & 0xffffffu) * m.tile_stride + first;
        const uint32_t gx = (T % m.tiles32_x) * 32u, gy = (T / m.tiles32_x) * 32u;
        const uint32_t px0 = gx + m.off_x, py0 = gy + m.off_y;
        if (gx >= m.ext_x || gy >= m.ext_y || px0 >= W || py0 >= H) return true; // no pixel: nothing to wait for
        const uint32_t xe = m.off_x + m.ext_x < W ? m.off_x + m.ext_x : W, ye = m.off_y + m.ext_y < H ? m.off_y + m.ext_y : H;
        const uint32_t px1 = px0 + 31u < xe ? px0 + 31u : xe - 1u, py1 = py0 + 31u < ye ? py0 + 31u : ye - 1u;
        auto cell_of = [&](uint32_t p, float r) { return (int)rtm::floor(((float)p * r) * 32.0f); };
        const int cx0 = cell_of(px0, k->rcp_w) - 2, cx1 = cell_of(px1, k->rcp_w) + 2;
        const int cy0 = cell_of(py0, k->rcp_h) - 2, cy1 = cell_of(py1, k->rcp_h) + 2;
        const int xlo = cx0 < 0 ? 0 : cx0, xhi = cx1 > RT_CAMERA_RES - 1 ? RT_CAMERA_RES - 1 : cx1;
        const int ylo = cy0 < 0 ? 0 : cy0, yhi = cy1 > RT_CAMERA_RES - 1 ? RT_CAMERA_RES - 1 : cy1;
        // the row's tasks tlo .. thi as a 4-bit group (task = row * 4 + x / 8: bits 4 (row % 8) .. of word row / 8)
        const uint32_t g = ((2u << (xhi / RT_FUSE_RAYS_PER_TASK)) - 1u) & ~((1u << (xlo / RT_FUSE_RAYS_PER_TASK)) - 1u);
        bool ok = true;
        for (int r = ylo; r <= yhi; ++r) {
            const uint32_t w = (r >> 3) == 0 ? w0 : (r >> 3) == 1 ? w1 : (r >> 3) == 2 ? w2 : w3;
            ok = ok && ((w >> ((r & 7) * 4)) & g) == g;
        }
        return ok;
    };
    // one scan step per call: 64 order entries from the block's scan position q.gscan (the global head when
    // it is behind it); 1: a unit (f, u) claimed; 0: none ready in this step (the next call looks further, and
    // starts over at the head once past the end); -1: no unit left anywhere
    auto gated_fetch = [&](uint32_t* pf, uint32_t* pu) -> int {
        const uint32_t nt = n_total >> 4; // order entries (tiles) of the batch
        bool gate_all = vload(q.gate_all) != 0u;
        if (!gate_all) { // every frame's prepass done? (its ray counter; lanes < n_frames)
            const uint32_t gw = lane < m.n_frames ? ld_u32(gp.gate, late(lane * RT_GATE_WORDS + RT_GATE_CTR))
                                                  : (uint32_t)(RT_CAMERA_RES * RT_CAMERA_RES);
            gate_all = __ballot(gw < (uint32_t)(RT_CAMERA_RES * RT_CAMERA_RES)) == 0ull;
            if (gate_all && lane == 0) q.gate_all = 1u;
        }
        if (gate_all) {
            // every prepass ray is in: the units in order by the queue counter (one atomic per unit, as without
            // the gate), each claimed by its bit in its tile's word (claims[i], 16 units); a unit the scan took
            // while the prepass ran (its bit set) is skipped
            for (int tries = 0; tries < 16; ++tries) {
                const uint32_t qi = wave_fetch(&counters[RT_CTR_PRIMARY], lane);
                if (qi >= n_total) return -1;
                uint32_t old = 0u;
                if (lane == 0) old = atomicOr(gp.claims + late(qi >> 4), 1u << (qi & 15u));
                if (!((__builtin_amdgcn_readfirstlane(old) >> (qi & 15u)) & 1u)) {
                    const uint32_t e = __builtin_amdgcn_readfirstlane(order[qi >> 4]);
                    *pf = e >> 24;
                    *pu = (e & 0xffffffu) * 16u + (qi & 15u);
                    return 1;
                }
            }
            return 0;
        }
        // while the prepass runs: a scan step of 64 tiles from the block's position (the head when behind it)
        const uint32_t h = (uint32_t)__builtin_amdgcn_readfirstlane(ld_sc1(counters + RT_CTR_SCAN));
        if (h >= nt) return -1;
        const uint32_t gs = vload(q.gscan);
        const uint32_t base = gs > h && gs < nt ? gs : h;
        const uint32_t i = late(base + lane); // (late: no per-lane scan address hoisted into the prologue)
        uint32_t e = 0u, c = 0xffffu;
        if (i < nt) { // buffer loads: uniform bases, one offset register
            e = ld_u32(order, i, false);
            c = ld_u32(gp.claims, i);
        }
        const bool left = (c & 0xffffu) != 0xffffu;
        const uint64_t lb = __ballot(left);
        if (base == h) { // the head moves past the tiles with no unit left
            const uint32_t nh = lb ? base + (uint32_t)__builtin_ctzll(lb) : base + 64u;
            if (nh > h && lane == 0) atomicMax(counters + RT_CTR_SCAN, nh);
        }
        if (lane == 0) q.gscan = base + 64u; // the block's next step (a hint: racing waves may repeat one)
        bool ready = left;
        if (left) { // the tile's frame's task mask (sc1 loads of its four words)
            const uint32_t gw = (e >> 24) * RT_GATE_WORDS;
            ready = tile_ready(e, ld_u32(gp.gate, gw), ld_u32(gp.gate, gw + 1u), ld_u32(gp.gate, gw + 2u),
                               ld_u32(gp.gate, gw + 3u));
        }
        // the wave's first try is the ready tile at or after its own slot in the step, so the waves scanning one
        // step spread their claims over its ready tiles (within a step the order is longest-first only roughly
        // anyway); the slot from the wave's hardware id, read when needed (no register held for it)
        const uint64_t rdy = __ballot(ready);
        const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);
        const uint64_t from = rdy & (~0ull << ((hw ^ (hw >> 6) ^ (hw >> 12)) & 63u));
        for (uint64_t rb = from ? from : rdy; rb; rb &= rb - 1ull) {
            const uint32_t l = (uint32_t)__builtin_ctzll(rb);
            uint32_t cl = (uint32_t)__builtin_amdgcn_readlane((int)c, (int)l) | 0xffff0000u;
            while (cl != 0xffffffffu) { // the tile's first unclaimed unit, by its bit
                const uint32_t kk = (uint32_t)__builtin_ctz(~cl);
                uint32_t old = 0u;
                if (lane == 0) old = atomicOr(gp.claims + late(base + l), 1u << kk);
                old = (uint32_t)__builtin_amdgcn_readfirstlane(old);
                if (!((old >> kk) & 1u)) {
                    const uint32_t el = (uint32_t)__builtin_amdgcn_readlane((int)e, (int)l);
                    *pf = el >> 24;
                    *pu = (el & 0xffffffu) * 16u + kk;
                    if (lane == 0) q.gscan = base; // (this step again next time: its tile may have units left)
                    return 1;
                }
                cl |= old;
            }
        }
        return 0;
    };

    // ---- one 8x8 primary unit ----
    auto do_unit = [&](uint32_t f, uint32_t u) {
        bool cells_in = true; // (the gated launch: the frame's CellDistance is stored, flagged by its last task)
        if constexpr (GATED) {
            cells_in = (vload(q.gate_cells) >> f) & 1u;
            if (!cells_in && ld_sc1(gp.gate + f * RT_GATE_WORDS + RT_GATE_CTR + 1) != 0u) {
                cells_in = true;
                if (lane == 0) atomicOr(&q.gate_cells, 1u << f);
            }
        }
        Ctx cf = frame_ctx(c, ft, f);
        cf.nz.phase = RT_PHASE_PRIMARY;
        uint32_t px, py;
        const bool valid = unit_pixel(m, f, u, lane, W, H, &px, &py);
        const float pxf = (float)px, pyf = (float)py;
        float plane_x = 0.0f;
        if (valid) {
            float spx = pxf * k->rcp_w, spy = pyf * k->rcp_h;
            const uint32_t cell = (uint32_t)rtm::fma(rtm::floor(spy * 32.0f), 32.0f, rtm::floor(spx * 32.0f));
            if (GATED && !cells_in) {
                // the gated launch before the frame's CellDistance is flagged: the cell's setTargetDepths from
                // its CameraResults (gate_ready passed)
                const float4* cam = ft->cam[f];
                plane_x = cell_bracket([&](int x, int y) { return cam_depth_sc1(cam, x, y); }, (int)(cell % RT_CAMERA_RES),
                                       (int)(cell / RT_CAMERA_RES)).x;
            } else if (GATED) { // flagged in this launch: an sc1 load of the bracket the frame's last task stored
                typedef const float __attribute__((address_space(1))) gcfloat;
                plane_x = __hip_atomic_load((gcfloat*)(ft->cells[f] + cell), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                plane_x = gptr(ft->cells[f])[cell].x;
            }
        }
        // the host vouches for the ceiling with these constants (read per unit: not held across the other loops)
        [[maybe_unused]] const bool sky = kSky && k->sky_exit != 0;
        for (uint32_t a = 0; a < aa; ++a) {
            const uint32_t t = f * m.frame_samples + (u * 64u + lane) * aa + a;
            March<L, true> st;
            st.d = 0.0f;
            bool lv = false;
            if (valid) {
                f3 p, dir;
                get_pixel_ray(cf, pxf + k->aa_off[a][0], pyf + k->aa_off[a][1], &p, &dir);
                march_begin(cf, st, p, plane_x, 1.0f, dir);
                lv = true;
            }
            __builtin_amdgcn_s_setprio(0);
            // The march as a loop of the lanes, not of the wave: a lane leaves it when its ray does, the wave
            // when its last lane has, and inside it the active lanes are the live rays.  The march state
            // is then the loop's only carried value and each step updates it in place (as `if (lv) step`
            // in a loop of the wave, every step first copied the state for the lanes that skip it).
            uint32_t it = 0;
            while (lv) {
                lv = march_live<L, true, false>(cf, st, RT_CAMERA_FAR, max_steps);
                if (!lv) break;
                // a provable miss leaves before its next step (sky_exit, rt_shader.h): st.d <= 0 stays
                if constexpr (kSky) {
                    if (sky && sky_exit(st.p.y, st.dir.y, st.dist)) {
                        lv = false;
                        break;
                    }
                }
                [[maybe_unused]] const uint64_t lb = __ballot(1); // the live rays
                RT_DIAG_LIVE_HIST(if (lane == (uint32_t)__builtin_ctzll(lb)) atomicAdd(&g_live_hist[__popcll(lb)], 1ull);)
                RT_DIAG_PRIMARY_STEPS({
                    cf.nz.phase = RT_COUNT_PHASE;
                    count_noise(cf.nz);
                    cf.nz.phase = RT_PHASE_PRIMARY;
                })
                // few rays left: they go to the segments, below (lv stays set)
                if constexpr (L == RT_NOMADPLAINS && kPrimarySeg > 0u && (!STATS || kStatsPrimarySeg)) {
                    if ((uint32_t)__popcll(lb) <= kPrimarySeg) break;
                }
                march_step<L, true, false>(cf, st);
                if (it == 96u) __builtin_amdgcn_s_setprio(1);
                else if (it == 224u) __builtin_amdgcn_s_setprio(2);
                else if (it == 384u) __builtin_amdgcn_s_setprio(3);
                ++it;
            }
            if constexpr (L == RT_NOMADPLAINS && kPrimarySeg > 0u && (!STATS || kStatsPrimarySeg)) {
                // the unit's last <= kPrimarySeg live rays finish on a segment of lanes each
                if (const uint64_t lb = __ballot(lv)) primary_seg(cf, st, lv, lb, pxf + k->aa_off[a][0], pyf + k->aa_off[a][1], sky);
            }
            __builtin_amdgcn_s_setprio(0);
            const bool hit = valid && st.d > 0.0f;
            WT(if (valid) wp_maxit = max(wp_maxit, (uint32_t)st.iters);)
            RayResult rr;
            if (valid) {
                rr = march_result(st);
                stat(BlockStats::PRIMARY, (uint32_t)st.iters);
                if (!hit) {
                    const float4 v = miss_sample(cf, pxf + k->aa_off[a][0], pyf + k->aa_off[a][1], rr.pd.w, rr.fc);
                    if (aa == 1u) { // the pixel is final (k_finish's sum of one sample times rcp(1) is v itself)
                        const uint32_t px8 = unorm8(v.x) | (unorm8(v.y) << 8) | (unorm8(v.z) << 16) | 0xff000000u;
                        if (m.packed) { // a packed shard buffer (no float output then)
                            if (!(RT_DIAG_SKIP & 1)) gptr(ft->out8[f])[packed_index(late(u * 64u + lane))] = px8;
                        } else {
                            const size_t o = (size_t)py * W + px;
                            if (!(RT_DIAG_SKIP & 1)) gptr(ft->out8[f])[o] = px8;
                            if (float4* o32 = ft->out32[f]) gstore(o32 + o, make_float4(v.x, v.y, v.z, 1.0f));
                        }
                    } else {
                        samples[t] = v;
                    }
                }
            }
            const uint64_t hb = __ballot(hit);
            // k_finish skips the misses; with fit it finishes only the hits the shading marks
            if (lane == 0) hitmask[(f * m.n_units + u) * aa + a] = (m.fit || m.fitm) ? 0ull : hb;
            if (hb) {
                // the hits' records go on the block's hit stack in rank order (dense lines), stored
                // before the top publishes them.  The stack does not overflow: a wave starts a unit
                // only while fewer than 64 hits are queued, so at most 63 + 16 waves x 64 x aa are
                // (rt_spill_caps' hit_cap); a push past it is dropped and flagged (rt_device_check).
                const uint32_t n = (uint32_t)__popcll(hb), rank = lane_rank(hb);
                if (hit) stat(BlockStats::HITS, 1u);
                q_lock(&q.lock, lane);
                const uint32_t top = vload(q.h_top);
                const bool fits = (uint32_t)__builtin_amdgcn_readfirstlane(top) + n <= hit_cap;
                if (hit && fits) hit_store<L>(hq + (size_t)(top + rank) * HR, t, rr);
                __builtin_amdgcn_s_waitcnt(0);
                if (lane == 0) {
                    if (fits) q.h_top = top + n;
                    else q.overflow |= RT_FLAG_HIT_OVERFLOW;
                }
                q_unlock(&q.lock, lane);
            }
        }
        c.nz.calls = cf.nz.calls;
    };

    // First unit of every wave is dealt wave-slot-major (wave slot w takes the next order index of row
    // w, w * blocks + j, j counted in the order the blocks start): the costliest units (k_order puts
    // them first) land one per SIMD instead of filling the first few CUs' SIMDs four deep, which sets
    // the frame time when there are barely more units than waves (an 8-way shard has ~4k units for 4k
    // waves); and a block that starts late (its CU still held by the other batch's k_trace tail, a
    // copy or a collective kernel) takes the cheapest units of each row, not a fixed set of the costliest.
    const uint32_t n_static = gridDim.x * (blockDim.x >> 6);
    const uint32_t first_qi = first_unit_index(counters, lane); // scalar, formed before the loop
    bool first_unit = true;
    bool np_open = np.tasks != 0u; // the next batch's prepass tasks may remain (FusedPrepass)
    bool gp_open = GATED && gp.tasks != 0u; // this batch's own prepass tasks may remain (GatedPrepass)
    if constexpr (GATED) {
        if (gp.debug & 1u) { // RT_DEVICE_DEBUG_GATE_STRESS: this CU's L1 holds the frames' previous CellDistance
            float acc = 0.0f;
            for (uint32_t f = 0; f < m.n_frames; ++f)
                for (uint32_t i = lane; i < RT_CAMERA_RES * RT_CAMERA_RES; i += 64u) acc += ft->cells[f][i].x;
            asm volatile("" : : "v"(acc));
        }
    }
    WT(wt[0] = __builtin_amdgcn_s_memrealtime();)
    for (;;) {
        if constexpr (L == RT_NOMADPLAINS) {
            // the gated launch: this batch's own prepass before anything else (every unit waits for some
            // of its rays).  Tasks are taken by resident waves, so every taken task finishes.
            if (GATED && gp_open) {
                const uint32_t qt = wave_fetch(&counters[RT_CTR_GATE], lane);
                if (qt < gp.tasks * kPrepassSplit) {
                    WT(const unsigned long long tp = __builtin_amdgcn_s_memrealtime();)
                    do_prepass(ft, qt, true);
                    WT(const unsigned long long tq = __builtin_amdgcn_s_memrealtime(); wt[21] += tq - tp; wt[22] = tq;)
                    continue;
                }
                gp_open = false;
            }
            // the next batch's prepass first (after a wave's static first unit): its k_order waits for it.
            // A wave leaves only after it found no task left, so every task is taken by a resident wave.
            if (np_open && !first_unit) {
                const uint32_t qt = wave_fetch(np.ctl, lane);
                if (qt < np.tasks * kPrepassSplit) {
                    do_prepass(np.ft, qt, false);
                    continue;
                }
                np_open = false;
            }
        }
        const uint32_t lp = queued_long();
        const uint32_t hp = queued_hits();
        const bool drained = vload(q.drained) != 0u;
        WT(const unsigned long long t0 = __builtin_amdgcn_s_memrealtime(); wt[12]++;
           wt[15] = t0; if (drained && wt[18] == 0) { wt[18] = t0; wt[19] = lp; wt[20] = hp; })
        // near the queue's end the long rays are taken from a smaller backlog (RT_NEAR_LONG_BATCH), so the
        // block's backlog at the drain -- what its post-drain tail marches -- is small
        const uint32_t lb_now = (RT_NEAR_UNITS > 0 && vload(q.near_end) != 0u) ? (uint32_t)RT_NEAR_LONG_BATCH : long_batch;
        if (lp >= lb_now || (drained && lp > 0u)) {
            if constexpr (L == RT_NOMADPLAINS && kSegLanes > 0u) {
                if (drained && lp <= kSegQueue) {
                    do_shadow_seg();
                    WT(const unsigned long long ds = __builtin_amdgcn_s_memrealtime() - t0; wt[4] += ds; wt[7]++;
                       wt[23] += ds; wt[24]++;)
                    continue;
                }
            }
            do_shadow();
            WT(const unsigned long long dl = __builtin_amdgcn_s_memrealtime() - t0; wt[4] += dl; wt[7]++; wt[27] += dl;)
            continue;
        }
        if (hp >= 64u || (drained && hp > 0u)) {
            if (lane == 0) atomicAdd(&q.active, 1u);
            do_shade();
            if (lane == 0) atomicSub(&q.active, 1u);
            WT(wt[3] += __builtin_amdgcn_s_memrealtime() - t0; wt[6]++;)
            continue;
        }
        if (GATED ? !drained : (!drained || first_unit)) {
            // (without the gated launch a wave's static first unit is taken even after the queue drained)
            if (lane == 0) atomicAdd(&q.active, 1u);
            bool run = false;
            uint32_t f = 0, u = 0;
            if constexpr (GATED) { // the gated launch: the first unit of a ready tile, longest-first
                const int got = __builtin_amdgcn_readfirstlane(gated_fetch(&f, &u)); // (wave-uniform)
                run = got > 0;
                if (got < 0) {
                    if (lane == 0) q.drained = 1u;
                } // (0: no ready tile in this step; the next call looks further)
            } else {
                const uint32_t qi = first_unit ? first_qi : n_static + wave_fetch(&counters[RT_CTR_PRIMARY], lane);
                first_unit = false;
                if (RT_NEAR_UNITS > 0 && qi + (uint32_t)RT_NEAR_UNITS * n_static >= n_total && lane == 0) q.near_end = 1u;
                if (qi < n_total) {
                    // the batch's tiles longest-first across its frames: entry (frame << 24) | tile
                    const uint32_t e = __builtin_amdgcn_readfirstlane(order[qi >> 4]);
                    f = e >> 24;
                    u = (e & 0xffffffu) * 16u + (qi & 15u);
                    run = true;
                } else if (lane == 0) {
                    q.drained = 1u;
                }
            }
            WT(if (!run) wt[9] += __builtin_amdgcn_s_memrealtime() - t0;) // (a fetch that found no unit: idle)
            if (run) { // (do_unit inlined once; f and u are wave-uniform: say so, for the divergence analysis)
                do_unit((uint32_t)__builtin_amdgcn_readfirstlane(f), (uint32_t)__builtin_amdgcn_readfirstlane(u));
                WT(const unsigned long long t1 = __builtin_amdgcn_s_memrealtime(); wt[2] += t1 - t0; wt[5]++; wt[8] = t1;)
            }
            if (lane == 0) atomicSub(&q.active, 1u);
            continue;
        }
        // drained and nothing queued: leave once no wave of the block can still push
        if (vload(q.active) == 0u && queued_long() == 0u && queued_hits() == 0u) break;
        __builtin_amdgcn_s_sleep(2);
        WT(wt[9] += __builtin_amdgcn_s_memrealtime() - t0;)
    }
    // a dropped push (never, by rt_spill_caps' bound) becomes the device's sticky flag (rt_device_check)
    if (lane == 0) {
        const uint32_t ov = vload(q.overflow);
        if (ov) atomicOr(counters + RT_CTR_BYTES / 4, ov);
    }
    WT(wt[1] = __builtin_amdgcn_s_memrealtime();
       for (int o = 32; o >= 1; o >>= 1) {
           wl_rays += __shfl_xor(wl_rays, o, 64);
           wl_maxit = max(wl_maxit, (uint32_t)__shfl_xor(wl_maxit, o, 64));
           wp_maxit = max(wp_maxit, (uint32_t)__shfl_xor(wp_maxit, o, 64));
       }
       wt[13] = wl_rays; wt[14] = wl_maxit; wt[16] = wp_maxit;
       const uint32_t slot = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
       if (lane < RT_WT_FIELDS && slot < RT_WT_MAX_WAVES) {
           unsigned long long v = 0;
           for (int f = 0; f < RT_WT_FIELDS; ++f) v = (lane == (uint32_t)f) ? wt[f] : v;
           g_wave_trace[slot * RT_WT_FIELDS + lane] = v;
       })
    if constexpr (STATS) {
        // the block's last wave out adds its counters to the frame statistics
        uint32_t done = 0;
        if (lane == 0) done = atomicAdd(&s_st.done, 1u);
        if (__builtin_amdgcn_readfirstlane(done) == (blockDim.x >> 6) - 1u && lane == 0) {
            atomicAdd(&stats->primary_steps, vload(s_st.v[BlockStats::PRIMARY]));
            atomicAdd(&stats->shadow_steps, vload(s_st.v[BlockStats::SHADOW]));
            atomicAdd(&stats->ao_steps, vload(s_st.v[BlockStats::AO]));
            atomicAdd(&stats->hits, vload(s_st.v[BlockStats::HITS]));
            atomicAdd(&stats->noise_calls, vload(s_st.v[BlockStats::NOISE]));
            atomicAdd(&stats->noise_waves, vload(s_st.v[BlockStats::NOISE_WAVES]));
        }
    }
}

// tracescreen.hlsl:67-75: the sum of the saturated samples in AA order, / AA, UNORM8 store.  Misses
// were coloured by k_trace (with one sample per pixel their pixels are already final there, and the
// unit's hit ballot says which lanes remain), hits by the shading / long-ray paths; w marks a hit,
// whose AO factor applies.  Persistent over 8x8 units, strided statically (wave w takes units w,
// w + n_waves, ...): the per-unit work is so short that a shared queue atomic would serialise it.
__global__ void __launch_bounds__(1024) k_finish(const RtConsts* __restrict__ k, const FrameTable* __restrict__ ft,
                                                 UnitMap m, const uint64_t* __restrict__ hitmask,
                                                 const float4* __restrict__ samples, uint32_t* __restrict__ aocc)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t W = (uint32_t)k->width, H = (uint32_t)k->height, aa = (uint32_t)k->aa_samples;
    const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
    const uint32_t total = m.n_units * m.n_frames;
    for (uint32_t g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); g < total; g += n_waves) {
        const uint32_t f = __builtin_amdgcn_readfirstlane(g / m.n_units), u = g - f * m.n_units;
        auto* out8 = gptr(ft->out8[f]);
        float4* out32 = ft->out32[f];
        uint32_t px, py;
        if (!unit_pixel(m, f, u, lane, W, H, &px, &py)) continue;
        // one sample per pixel: k_trace wrote the misses' pixels, only the hits remain (fit: only the
        // units whose hitmask word is nonzero, and in them the samples flagged kFinFlag)
        if (m.fit || m.fitm) {
            if (hitmask[f * m.n_units + u] == 0ull) continue;
            const uint32_t t = f * m.frame_samples + u * 64u + lane;
            if (!((aocc[t >> 2] >> ((t & 3u) * 8u)) & kFinFlag)) continue; // (its word is cleared by a flagged lane or is 0)
        } else if (aa == 1u && !((hitmask[f * m.n_units + u] >> lane) & 1ull)) {
            continue;
        }
        float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
        for (uint32_t a = 0; a < aa; ++a) {
            const uint32_t t = f * m.frame_samples + (u * 64u + lane) * aa + a;
            float4 v;
            if (aa == 1u) { // sample_store's colour-only record of a hit
                const float* c = reinterpret_cast<const float*>(samples) + 3u * t;
                v = make_float4(c[0], c[1], c[2], 1.0f);
            } else {
                v = samples[t];
            }
            if (v.w > 0.0f && k->ao_samples > 0) { // AO extension: ao multiplies the saturated sample
                const float ao = ao_factor(ao_occluded(aocc, t), k->ao_samples);
                v = make_float4(v.x * ao, v.y * ao, v.z * ao, v.w);
            }

            c0 = c0 + v.x;
            c1 = c1 + v.y;
            c2 = c2 + v.z;
        }
        // the next launch on these buffers counts from zero: every counted sample is read above, and
        // the words are cleared once all of them are (a word's other samples belong to this lane or to
        // lanes of this unit, whose reads in the same loop iterations precede these stores), so no
        // per-launch memset of the counts precedes k_trace
        if (k->ao_samples > 0) {
            const uint32_t t0 = f * m.frame_samples + (u * 64u + lane) * aa;
            for (uint32_t w = t0 >> 2; w <= (t0 + aa - 1u) >> 2; ++w) aocc[w] = 0u;
        }
        float ia = rtm::rcp((float)aa);
        c0 = c0 * ia;
        c1 = c1 * ia;
        c2 = c2 * ia;
        size_t o = out_index(m, u, lane, px, py, (uint32_t)k->width);
        if (!(RT_DIAG_SKIP & 64)) out8[o] = unorm8(c0) | (unorm8(c1) << 8) | (unorm8(c2) << 16) | 0xff000000u;
        if (out32) gstore(out32 + o, make_float4(c0, c1, c2, 1.0f));
    }
}

// Tile-cyclic shard transport: one 256-thread block per 32x32 tile.
// RecorderWinAPI::write's pixel conversion (RecorderWinAPI.cpp:244-253): the R8G8B8A8
// backbuffer DWORD dwc becomes dwc & 0xFF00 | (dwc & 0xFF) << 16 | (dwc & 0xFF0000) >> 16,
// i.e. bytes (B, G, R, 0) = MFVideoFormat_RGB32, row y at dst + y * pitch.  One v_perm_b32
// per pixel, 4 pixels (16 B) per thread: a pure HBM stream (read W*H*4 B, write W*H*4 B).
__global__ void __launch_bounds__(256) k_bgrx(const uint32_t* __restrict__ fb, uint32_t* __restrict__ dst, int w,
                                              int h, int pitch_words)
{
    const int quads = (w + 3) >> 2;
    const int y = blockIdx.y;
    for (int qx = blockIdx.x * blockDim.x + threadIdx.x; qx < quads; qx += gridDim.x * blockDim.x) {
        const int x = qx << 2;
        const uint32_t* src = fb + (size_t)y * w + x;
        uint32_t* out = dst + (size_t)y * pitch_words + x;
        // perm selector: result bytes (B, G, R, 0) from (R, G, B, A) = bytes 2, 1, 0 and constant 0 (0x0c)
        constexpr uint32_t sel = 0x0c000102u;
        if (x + 4 <= w && ((w & 3) == 0) && ((pitch_words & 3) == 0)) {
            const uint4 v = *reinterpret_cast<const uint4*>(src);
            uint4 o;
            o.x = __builtin_amdgcn_perm(0u, v.x, sel);
            o.y = __builtin_amdgcn_perm(0u, v.y, sel);
            o.z = __builtin_amdgcn_perm(0u, v.z, sel);
            o.w = __builtin_amdgcn_perm(0u, v.w, sel);
            *reinterpret_cast<uint4*>(out) = o;
        } else {
            for (int i = 0; i < 4 && x + i < w; ++i) out[i] = __builtin_amdgcn_perm(0u, src[i], sel);
        }
    }
}

// The readback ring's frame snapshot (rt_readback_submit): the W*H RGBA8 words of a framebuffer into a tightly
// packed device staging slot, so that the next trace may overwrite the framebuffer while the slot's copy to the
// host is still running.  Both buffers are one 1-D array (hipMalloc'd, so 16-byte aligned; tight rows): 16 B per
// thread, the grid sized to the work, and the thread after the last quad copies the W*H mod 4 tail words.  BGRX:
// RecorderWinAPI::write's conversion on the way (k_bgrx's selector).  A pure HBM stream (read and write W*H*4 B).
template <bool BGRX>
__global__ void __launch_bounds__(256) k_snapshot(const uint32_t* __restrict__ fb, uint32_t* __restrict__ dst,
                                                  uint32_t words)
{
    constexpr uint32_t sel = 0x0c000102u; // (B, G, R, 0) from (R, G, B, A)
    const uint32_t quads = words >> 2;
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q < quads) {
        uint4 v = reinterpret_cast<const uint4*>(fb)[q];
        if (BGRX) {
            v.x = __builtin_amdgcn_perm(0u, v.x, sel);
            v.y = __builtin_amdgcn_perm(0u, v.y, sel);
            v.z = __builtin_amdgcn_perm(0u, v.z, sel);
            v.w = __builtin_amdgcn_perm(0u, v.w, sel);
        }
        reinterpret_cast<uint4*>(dst)[q] = v;
    } else if (q == quads) {
        for (uint32_t i = quads << 2; i < words; ++i) dst[i] = BGRX ? __builtin_amdgcn_perm(0u, fb[i], sel) : fb[i];
    }
}

// Shard transport: job blockIdx.y copies tile blockIdx.x of its shard (tile blockIdx.x * count +
// shard, row-major) between its framebuffer and its packed buffer (1024 RGBA8 pixels per tile,
// row-major in the tile).  Thread t moves pixels 4 (t & 7) .. +3 of tile row t >> 3: one 16-byte
// access each way when the row segment lies inside the frame and both pointers allow it.  Pixels
// outside the frame are neither read nor written.  A batch's pack or unpack (rank 0 unpacks
// (N-1) x B shards per batch) is one launch instead of one per frame and rank: those small
// launches queue behind the other batch's persistent k_trace and each costs a dispatch.
__global__ void __launch_bounds__(256) k_shard_copy(ShardJobs jobs, int w, int h, int count, int pack)
{
    const int job = blockIdx.y;
    const int tiles_x = (w + 31) / 32, total = tiles_x * ((h + 31) / 32);
    const int tile = (int)blockIdx.x * count + jobs.shard[job];
    if (tile >= total) return; // a shard smaller than the grid (ragged shards)
    const int r = (int)threadIdx.x >> 3, c = ((int)threadIdx.x & 7) * 4;
    const int x = (tile % tiles_x) * 32 + c, y = (tile / tiles_x) * 32 + r;
    if (y >= h || x >= w) return;
    uint32_t* fb = jobs.fb[job] + (size_t)y * w + x;
    uint32_t* pk = jobs.packed[job] + (size_t)blockIdx.x * 1024 + r * 32 + c;
    if (x + 3 < w && (((uintptr_t)fb | (uintptr_t)pk) & 15u) == 0) {
        if (pack) *reinterpret_cast<uint4*>(pk) = *reinterpret_cast<const uint4*>(fb);
        else *reinterpret_cast<uint4*>(fb) = *reinterpret_cast<const uint4*>(pk);
    } else {
        for (int i = 0; i < 4 && x + i < w; ++i) {
            if (pack) pk[i] = fb[i];
            else fb[i] = pk[i];
        }
    }
}

// ft == nullptr: one frame (a.consts -> out); else frames 0..n-1 of the table (blockIdx.y).
template <int L>
void launch_camerarays_l(const RtLaunch& a, float4* out, const FrameTable* ft, uint32_t n)
{
    if constexpr (L == RT_NOMADPLAINS) {
        // one LPR-lane group per ray.  A block holds the noise tables (one block per CU), so
        // a batch packs more rays per block to keep every frame's prepass in one dispatch
        // round: 8 rays of 32 lanes (256 threads) up to 2 frames, 16 up to 4, and beyond 64
        // rays of 8 lanes (512 threads, <= 256 blocks for <= 16 frames; 4 lanes up to 24 frames).  Fewer lanes per ray
        // lengthen a step (3 noise rounds instead of 1) but keep a 12-frame prepass in one
        // round: 1.4 -> 0.7 ms per batch, +1.8% at C3 (32 rays of 32 lanes took two rounds).
        auto go = [&](auto bs_tag, auto lpr_tag) {
            constexpr int BS = decltype(bs_tag)::value, LPR = decltype(lpr_tag)::value;
            dim3 grid(RT_CAMERA_RES * RT_CAMERA_RES / (BS / LPR), n), block(BS);
            if (a.stats)
                hipLaunchKernelGGL((k_camerarays_group<true, BS, LPR>), grid, block, 0, a.stream, a.consts, a.perm2d,
                                   a.grad, out, a.stats, ft);
            else
                hipLaunchKernelGGL((k_camerarays_group<false, BS, LPR>), grid, block, 0, a.stream, a.consts,
                                   a.perm2d, a.grad, out, a.stats, ft);
        };
        using C512 = std::integral_constant<int, 512>;
        using L32 = std::integral_constant<int, 32>;
        if (n <= 2) go(std::integral_constant<int, RT_PREPASS_BS1>{}, std::integral_constant<int, RT_PREPASS_LPR1>{});
        else if (n <= 4) go(C512{}, L32{});
        else if (n <= 16) go(C512{}, std::integral_constant<int, 8>{}); // 64 rays of 16 lanes per 1024 threads: same
        else go(C512{}, std::integral_constant<int, 4>{}); // > 16 frames: 128 rays of 4 lanes, <= 192 blocks for 24
        return;
    }
    dim3 grid(RT_CAMERA_RES * RT_CAMERA_RES / 64, n), block(64);
    if (a.stats)
        hipLaunchKernelGGL((k_camerarays<L, true>), grid, block, 0, a.stream, a.consts, a.perm2d, a.grad, out, a.stats,
                           ft);
    else
        hipLaunchKernelGGL((k_camerarays<L, false>), grid, block, 0, a.stream, a.consts, a.perm2d, a.grad, out, a.stats,
                           ft);
}

template <int L>
void launch_split_l(const RtLaunch& a, uint32_t ox, uint32_t oy, uint32_t ex, uint32_t ey, uint32_t first,
                    uint32_t stride)
{
    UnitMap m;
    uint32_t tiles_x = (ex + 31) / 32, tiles_y = (ey + 31) / 32, total = tiles_x * tiles_y;
    // a batch rotates the shards over its frames (frame f traces shard (first + f) % stride), so
    // each rank's share of a batch mixes the tile classes of every shard.  Measured at C3 with
    // 12-frame batches (one-GPU shard simulation): the slowest of 4 ranks
    // went from 4-7% above the mean to 3.49x/4 scaling; N=2 and N=8 within noise.  n_units is
    // the largest shard's; the trailing units of a smaller shard map past the tile range and
    // unit_pixel rejects every lane of them.
    const uint32_t rot = a.n_frames > 1u && stride > 1u ? 1u : 0u;
    if (!rot && first >= total) return;
    m.off_x = ox;
    m.off_y = oy;
    m.ext_x = ex;
    m.ext_y = ey;
    m.tiles32_x = tiles_x;
    m.tile_first = first;
    m.tile_stride = stride;
    m.n_units = ((total - (rot ? 0u : first) + stride - 1) / stride) * 16u; // rot: the largest shard
    m.frame_rot = rot;
    m.n_frames = a.n_frames;
    m.frame_samples = m.n_units * 64u * (uint32_t)a.aa;
    uint32_t blocks = (uint32_t)(a.num_cus > 0 ? a.num_cus : 256);
    uint32_t need = (m.n_units * m.n_frames + 15u) / 16u;
    uint32_t pblocks = need < blocks ? need : blocks;
    m.order_batch = RT_ORDER_BATCH >= 0 ? (uint32_t)RT_ORDER_BATCH
                                        : (uint32_t)(m.n_frames > 1u && m.n_units < kOrderBatchUnitsPerWave * pblocks * 16u);
    // k_finish holds no LDS: up to 2 blocks per CU
    uint32_t fblocks = need < 2u * blocks ? need : 2u * blocks;
    dim3 blk(1024);
    m.cells_from_cam = (uint32_t)a.cells_from_cam;
    m.fit = (uint32_t)a.fit;
    m.fitm = kAoSlots > 0u ? (uint32_t)a.fitm : 0u;
    m.packed = (uint32_t)a.packed;
    // k_order: setTargetDepths (cells_from_cam), the work counters' reset, the tile order
    // (fuse_next.ctl is zeroed even with no tasks: RT_DEVICE_DEBUG_WITHHOLD_FUSE's timeout test)
    hipLaunchKernelGGL(k_order, dim3(m.order_batch ? 1u : m.n_frames), blk, 0, a.stream, a.frames, m, a.order, a.queue,
                       a.wait_ctl, a.wait_total, a.fuse_next.ctl, a.host_flag, a.gated.tasks ? a.gated.gate : nullptr,
                       a.gated.claims);
    if (a.after_order) (void)hipEventRecord(a.after_order, a.stream);
    if (a.after_order_fuse) (void)hipEventRecord(a.after_order_fuse, a.stream);
    // primary + shading + long rays; what does not fit a CU's LDS rings goes to its spill stacks
    auto primary = [&](auto stats_tag) {
        constexpr bool S = decltype(stats_tag)::value;
        const RtConsts* k0 = a.frames_host.k[0];
        // the gated launch's own instantiation (nomadplains without STATS: the runtime never gates others)
        constexpr bool kCanGate = L == RT_NOMADPLAINS && !S;
        auto* kern = (kCanGate && a.gated.tasks) ? k_trace<L, S, kCanGate> : k_trace<L, S, false>;
        hipLaunchKernelGGL(kern, dim3(pblocks), dim3(TraceThreads<L>::value), 0, a.stream, k0, a.frames,
                           a.perm2d, a.grad, m,
                           a.order, a.hitmask, a.samples, a.fin, a.finpool, a.cpool, a.hitq, a.spill_long, a.hit_cap,
                           a.long_spill_cap, a.aocc, a.queue, a.stats, kLongBatch, kRefillIdle, kCompactLive,
                           a.small_rings ? 64u : kLongRing, a.small_rings ? 8u : kFinSlots, a.fuse_next, a.gated);
        // fit without AO: every hit pixel is final in k_trace
        if (!(m.fit && a.ao_samples == 0))
            hipLaunchKernelGGL(k_finish, dim3(fblocks), blk, 0, a.stream, k0, a.frames, m, a.hitmask, a.samples, a.aocc);
    };
    if (a.stats) primary(std::true_type{});
    else primary(std::false_type{});
}

} // namespace

void rt_launch_camerarays(const RtLaunch& a, float4* out)
{
    switch (a.landscape) {
    case RT_TESTING: launch_camerarays_l<RT_TESTING>(a, out, nullptr, 1u); break;
    case RT_SIMPLE: launch_camerarays_l<RT_SIMPLE>(a, out, nullptr, 1u); break;
    case RT_GREENROCKS: launch_camerarays_l<RT_GREENROCKS>(a, out, nullptr, 1u); break;
    default: launch_camerarays_l<RT_NOMADPLAINS>(a, out, nullptr, 1u); break;
    }
}

void rt_launch_camerarays_batch(const RtLaunch& a)
{
    switch (a.landscape) {
    case RT_TESTING: launch_camerarays_l<RT_TESTING>(a, nullptr, a.frames, a.n_frames); break;
    case RT_SIMPLE: launch_camerarays_l<RT_SIMPLE>(a, nullptr, a.frames, a.n_frames); break;
    case RT_GREENROCKS: launch_camerarays_l<RT_GREENROCKS>(a, nullptr, a.frames, a.n_frames); break;
    default: launch_camerarays_l<RT_NOMADPLAINS>(a, nullptr, a.frames, a.n_frames); break;
    }
}

void rt_launch_tracescreen(const RtLaunch& a, uint32_t ox, uint32_t oy, uint32_t ex, uint32_t ey, uint32_t first,
                           uint32_t stride)
{
    if (ex == 0 || ey == 0 || stride == 0) return;
    switch (a.landscape) {
    case RT_TESTING: launch_split_l<RT_TESTING>(a, ox, oy, ex, ey, first, stride); break;
    case RT_SIMPLE: launch_split_l<RT_SIMPLE>(a, ox, oy, ex, ey, first, stride); break;
    case RT_GREENROCKS: launch_split_l<RT_GREENROCKS>(a, ox, oy, ex, ey, first, stride); break;
    default: launch_split_l<RT_NOMADPLAINS>(a, ox, oy, ex, ey, first, stride); break;
    }
}

void rt_launch_bgrx(hipStream_t s, const uint32_t* fb, uint32_t* dst, int w, int h, int pitch_words)
{
    const int quads = (w + 3) / 4;
    const int bx = (quads + 255) / 256;
    hipLaunchKernelGGL(k_bgrx, dim3(bx, h), dim3(256), 0, s, fb, dst, w, h, pitch_words);
}

void rt_launch_snapshot(hipStream_t s, const uint32_t* fb, uint32_t* dst, size_t words, int bgrx)
{
    if (words == 0 || words > 0xffffffffull) return; // (rt_readback_create rejects such a device)
    const uint32_t n = (uint32_t)words;
    const uint32_t threads = (n >> 2) + ((n & 3u) ? 1u : 0u); // one per quad, one more for the tail words
    const uint32_t blocks = (threads + 255u) / 256u;
    if (bgrx) hipLaunchKernelGGL(k_snapshot<true>, dim3(blocks), dim3(256), 0, s, fb, dst, n);
    else hipLaunchKernelGGL(k_snapshot<false>, dim3(blocks), dim3(256), 0, s, fb, dst, n);
}

void rt_launch_shard_copy(hipStream_t s, const ShardJobs& jobs, int n, int w, int h, int count, int pack)
{
    if (n <= 0 || n > RT_SHARD_JOBS) return;
    // shard 0 holds the most tiles: its count is the grid's x extent
    const size_t tiles = rt_shard_tiles(w, h, 0, count);
    if (tiles == 0) return;
    hipLaunchKernelGGL(k_shard_copy, dim3((unsigned)tiles, (unsigned)n), dim3(256), 0, s, jobs, w, h, count, pack);
}

// ---------------------------------------------------------------------------
// The queries' launch dispatch (host side): a launch's run-time choices as its kernel's template arguments.
namespace {

template <int V>
using Int = std::integral_constant<int, V>;

// f(Int<L>) with the launch's landscape
template <class F>
void with_landscape(const RtLaunch& a, F f)
{
    switch (a.landscape) {
    case RT_TESTING: f(Int<RT_TESTING>{}); break;
    case RT_SIMPLE: f(Int<RT_SIMPLE>{}); break;
    case RT_GREENROCKS: f(Int<RT_GREENROCKS>{}); break;
    default: f(Int<RT_NOMADPLAINS>{}); break;
    }
}

// f(std::true_type) or f(std::false_type)
template <class F>
void with_bool(bool b, F f)
{
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// f(Int<BS>, Int<LPR>) with a segment shape's (block size, lanes per ray), one of the pairs of the prepass's
// ladder; false: no such pair (f not called)
template <class F>
bool with_segment(int bs, int lpr, F f)
{
    if (bs == RT_PREPASS_BS1 && lpr == RT_PREPASS_LPR1) f(Int<RT_PREPASS_BS1>{}, Int<RT_PREPASS_LPR1>{});
    else if (bs == 512 && lpr == 32) f(Int<512>{}, Int<32>{});
    else if (bs == 512 && lpr == 8) f(Int<512>{}, Int<8>{});
    else if (bs == 512 && lpr == 4) f(Int<512>{}, Int<4>{});
    else return false;
    return true;
}

} // namespace

// ---------------------------------------------------------------------------
// Ray and surface queries (rt_terrain_trace_rays, rt_terrain_trace_surface): traceRay for rays read from memory
// instead of getPixelRay's, in two kernel shapes that a policy per family completes.  Ray i is two 16-byte loads
// (ox oy oz _ | dx dy dz _).  The LOD eye is a kernel argument (QueryEye).
//   A ray query is camerarays.hlsl:12-21: skiprefine, and the prepass's range, stepmod and no cap as compile-time
//   constants.  Its result is one 16-byte store.
//   A surface query is the march tracescreen runs for its pixels (skiprefine off, tracescreen.hlsl:20) and
//   getNormal (tracing.hlsl:107-116); the march's parameters are kernel arguments, and with RANGE the rays' spare
//   words are t_min_i and t_max_i.  Its result is two 16-byte stores: pd.xyz, pd.w | normal, density (the normal
//   0 where density <= 0: no hit).
// Both store the march loop's iteration count with STEPS.
namespace {

#ifdef RT_QUERY_UTIL
// diagnostic build (scripts/*_query_bench.py) of the lane kernels' waves: march steps, live lanes summed over
// them, visits of the refill point with work beside the refill (a wave's ended lanes' normals together; shading
// visits in k_shadequery, visits that claim points in k_shadepoints), lanes summed over those (both 0 for ray
// queries)
__device__ unsigned long long g_query_util[4];
#endif

// a ray's march: march_begin's arguments and the distance the march ends at
struct QueryRay {
    f3 p, dir;
    float t0, endd;
};

// A family's policy: SKIPREFINE, a ray's march from its two loads and the query's arguments (Args, the kernels'
// last parameter before the counter), and the store of an ended ray, `normal` being getNormal.
struct RayArgs {
    QueryEye eye;
};
template <bool STEPS>
struct RayPolicy {
    using Args = RayArgs;
    static constexpr bool SKIPREFINE = true, NORMAL = false, kSteps = STEPS;
    static __device__ __forceinline__ QueryRay ray(const Args&, float4 o, float4 d)
    {
        return QueryRay{rtm::mk(o.x, o.y, o.z), rtm::mk(d.x, d.y, d.z), RT_CAMERA_NEAR, RT_CAMERA_FAR};
    }
    static __device__ __forceinline__ float t_max(const Args&) { return RT_CAMERA_FAR; }
    static __device__ __forceinline__ float stepmod(const Args&) { return 2.0f; }
    static __device__ __forceinline__ int max_steps(const Args&) { return 0; }
    template <class M, class Normal>
    static __device__ __forceinline__ void store(const M& st, float4* __restrict__ out, uint32_t* __restrict__ steps,
                                                 uint32_t i, Normal)
    {
        RayResult rr = march_result(st);
        if (rr.density < 0.0f) rr.pd.w = RT_CAMERA_FAR;
        gstore(out + i, make_float4(rr.pd.x, rr.pd.y, rr.pd.z, rr.pd.w));
        if constexpr (STEPS) steps[i] = (uint32_t)st.iters;
    }
};

// (the shaded queries' arguments too)
struct SurfArgs {
    QueryEye eye;
    float t_min, t_max, stepmod;
    int max_steps;
};
template <bool STEPS, bool RANGE>
struct SurfPolicy {
    using Args = SurfArgs;
    static constexpr bool SKIPREFINE = false, NORMAL = true, kSteps = STEPS;
    static __device__ __forceinline__ QueryRay ray(const Args& a, float4 o, float4 d)
    {
        return QueryRay{rtm::mk(o.x, o.y, o.z), rtm::mk(d.x, d.y, d.z), RANGE ? o.w : a.t_min, RANGE ? d.w : a.t_max};
    }
    static __device__ __forceinline__ float t_max(const Args& a) { return a.t_max; }
    static __device__ __forceinline__ float stepmod(const Args& a) { return a.stepmod; }
    static __device__ __forceinline__ int max_steps(const Args& a) { return a.max_steps; }
    template <class M, class Normal>
    static __device__ __forceinline__ void store(const M& st, float4* __restrict__ out, uint32_t* __restrict__ steps,
                                                 uint32_t i, Normal normal)
    {
        const RayResult rr = march_result(st);
        f3 nrm = rtm::mk(0.0f, 0.0f, 0.0f);
        if (rr.density > 0.0f) nrm = normal(f4{rr.pd.x, rr.pd.y, rr.pd.z, rr.density});
        gstore(out + 2 * (size_t)i, make_float4(rr.pd.x, rr.pd.y, rr.pd.z, rr.pd.w));
        gstore(out + 2 * (size_t)i + 1, make_float4(nrm.x, nrm.y, nrm.z, rr.density));
        if constexpr (STEPS) steps[i] = (uint32_t)st.iters;
    }
};

// Segments (nomadplains, few rays: a pick is one ray, and on one lane its longest march takes milliseconds):
// k_camerarays_group with the ray loaded.  One LPR-lane segment per ray, a static deal: the latency shape of the
// prepass.  The march state is replicated over the segment, so the hit test is segment-uniform: the whole segment
// takes a surface query's normal, its three taps through density_nomadplains_seg, and lane 0 stores.  That store
// is spelled out here: through the policy's store the STEPS instantiations took two more VGPRs
// (profiles/r15/query_fold.md).
template <class P, int BS, int LPR>
__global__ void __launch_bounds__(BS) k_query_seg(const RtConsts* __restrict__ k, const uint32_t* __restrict__ perm2d,
                                                  const float4* __restrict__ grad, const float4* __restrict__ rays,
                                                  float4* __restrict__ out, uint32_t* __restrict__ steps, uint32_t n,
                                                  typename P::Args a)
{
    constexpr int L = RT_NOMADPLAINS;
    __shared__ __attribute__((aligned(16))) uint32_t lds[kNoiseLdsWords];
    load_noise_lds(lds, perm2d, grad, k);
    const uint32_t i = blockIdx.x * (uint32_t)(BS / LPR) + threadIdx.x / (uint32_t)LPR;
    if (i >= n) return; // whole segments leave together
    Ctx c = make_ctx(k, lds, a.eye);
    const uint32_t j = threadIdx.x & (LPR - 1u), base = threadIdx.x & 63u & ~(LPR - 1u);
    const SegOctaves<LPR> g = seg_octaves<LPR>(c, j);
    const QueryRay r = P::ray(a, rays[2 * (size_t)i], rays[2 * (size_t)i + 1]);
    auto dens = [&](f3 q) {
        uint32_t used;
        return density_nomadplains_seg<LPR>(c, g, q, j, base, &used);
    };
    March<L, false> st;
    march_begin(c, st, r.p, r.t0, P::stepmod(a), r.dir);
    while (march_live<L, false, P::SKIPREFINE>(c, st, r.endd, P::max_steps(a)))
        march_step_with<L, false, P::SKIPREFINE>(c, st, dens);
    if constexpr (P::NORMAL) {
        const RayResult rr = march_result(st);
        f3 nrm = rtm::mk(0.0f, 0.0f, 0.0f);
        if (rr.density > 0.0f) nrm = get_normal_with(c, f4{rr.pd.x, rr.pd.y, rr.pd.z, rr.density}, dens);
        if (j == 0) {
            gstore(out + 2 * (size_t)i, make_float4(rr.pd.x, rr.pd.y, rr.pd.z, rr.pd.w));
            gstore(out + 2 * (size_t)i + 1, make_float4(nrm.x, nrm.y, nrm.z, rr.density));
            if constexpr (P::kSteps) steps[i] = (uint32_t)st.iters;
        }
    } else {
        if (j == 0) P::store(st, out, steps, i, 0);
    }
}

// Lanes (every landscape, many rays): persistent, one 1024-thread block per CU with the noise tables in
// LDS once, one lane per ray.  Rays differ in length by more than 100x, so no static deal: a wave whose
// live lanes fall to `refill_live` or fewer stores its ended rays, claims as many new ones from the
// query's counter (one atomic per refill, wave_fetch) and hands them to its idle lanes by rank.  Results
// go to out[ray], so the order of the claims does not show.  The ended lanes of a wave evaluate their normals
// together where their results are stored: at the refill and at the end.
template <int L, class P>
__global__ void __launch_bounds__(1024) k_query_lanes(const RtConsts* __restrict__ k, const uint32_t* __restrict__ perm2d,
                                                      const float4* __restrict__ grad, const float4* __restrict__ rays,
                                                      float4* __restrict__ out, uint32_t* __restrict__ steps, uint32_t n,
                                                      typename P::Args a, uint32_t* __restrict__ counter,
                                                      uint32_t refill_live)
{
    // (diagnostic) this wave's march steps and its live lanes summed over them; its stores of hits, and their lanes
    RT_DIAG_QUERY_UTIL(uint32_t util_wave = 0, util_lane = 0, util_nwave = 0, util_nlane = 0;)
    __shared__ __attribute__((aligned(16))) uint32_t lds[kNoiseLdsWords];
    load_noise_lds(lds, perm2d, grad, k);
    Ctx c = make_ctx(k, lds, a.eye);
    const uint32_t lane = threadIdx.x & 63u;
    auto normal = [&](f4 pd) { return get_normal<L>(c, pd); };
    March<L, false> st{};
    float endd = P::t_max(a); // per lane where the rays carry their ranges
    uint32_t idx = 0;
    bool has = false, live = false; // has: idx is a ray of the query whose result is not stored yet
    bool more = true;               // (uniform) the counter has not passed n
    for (;;) {
        uint64_t lv = __ballot(live);
        if (more && (uint32_t)__popcll(lv) <= refill_live) {
            const uint32_t cnt = 64u - (uint32_t)__popcll(lv); // >= 1: refill_live <= 63
            const uint32_t first = wave_fetch(counter, lane, cnt);
            RT_DIAG_QUERY_UTIL(if (const uint64_t nm = __ballot(!live && has && st.d > 0.0f); P::NORMAL && nm) {
                ++util_nwave;
                util_nlane += (uint32_t)__popcll(nm);
            })
            if (!live) {
                if (has) P::store(st, out, steps, idx, normal);
                idx = first + lane_rank(~lv);
                has = idx < n;
                if (has) {
                    const QueryRay r = P::ray(a, rays[2 * (size_t)idx], rays[2 * (size_t)idx + 1]);
                    endd = r.endd;
                    march_begin(c, st, r.p, r.t0, P::stepmod(a), r.dir);
                    live = march_live<L, false, P::SKIPREFINE>(c, st, endd, P::max_steps(a));
                }
            }
            more = first + cnt < n;
            lv = __ballot(live);
        }
        if (!lv) {
            if (!more) break;
            continue; // every new ray ended before its first step: claim again
        }
        RT_DIAG_QUERY_UTIL(++util_wave; util_lane += (uint32_t)__popcll(lv);)
        if (live) {
            march_step<L, false, P::SKIPREFINE>(c, st);
            live = march_live<L, false, P::SKIPREFINE>(c, st, endd, P::max_steps(a));
        }
    }
    RT_DIAG_QUERY_UTIL(if (const uint64_t nm = __ballot(has && st.d > 0.0f); P::NORMAL && nm) {
        ++util_nwave;
        util_nlane += (uint32_t)__popcll(nm);
    })
    if (has) P::store(st, out, steps, idx, normal);
    RT_DIAG_QUERY_UTIL(if (lane == 0) {
        atomicAdd(&g_query_util[0], (unsigned long long)util_wave);
        atomicAdd(&g_query_util[1], (unsigned long long)util_lane);
        atomicAdd(&g_query_util[2], (unsigned long long)util_nwave);
        atomicAdd(&g_query_util[3], (unsigned long long)util_nlane);
    })
}

// the one place a SurfArgs is built: surface and shaded queries alike
SurfArgs surf_args(const float eye[3], const RtMarchParams& m)
{
    return SurfArgs{{eye[0], eye[1], eye[2]}, m.t_min, m.t_max, m.stepmod, m.max_steps};
}

// f(STEPS, RANGE) as two bool tags
template <class F>
void with_steps_range(bool steps, bool range, F f)
{
    with_bool(steps, [&](auto steps_tag) { with_bool(range, [&](auto range_tag) { f(steps_tag, range_tag); }); });
}

// f(P*, P::Args) with the query's policy P (its family, STEPS and RANGE) and arguments
template <class F>
void with_policy(const RtTraceQuery& q, F f)
{
    with_steps_range(q.steps != nullptr, q.surface && q.march.ray_range, [&](auto steps_tag, auto range_tag) {
        constexpr bool STEPS = decltype(steps_tag)::value, RANGE = decltype(range_tag)::value;
        if (q.surface) f((SurfPolicy<STEPS, RANGE>*)nullptr, surf_args(q.eye, q.march));
        else if constexpr (!RANGE) f((RayPolicy<STEPS>*)nullptr, RayArgs{{q.eye[0], q.eye[1], q.eye[2]}});
    });
}

} // namespace

bool rt_launch_tracequery(const RtLaunch& a, const RtTraceQuery& q)
{
    if (q.n == 0 || q.blocks == 0) return true;
    if (q.lpr > 1 && a.landscape != RT_NOMADPLAINS) return false;
    // the live-lane count at or below which a wave refills (RT_RAYQ_REFILL; at most 63, so a refill claims >= 1 ray)
    constexpr uint32_t thr = RT_RAYQ_REFILL < 63 ? RT_RAYQ_REFILL : 63;
    bool found = true;
    with_policy(q, [&](auto* policy, auto args) {
        using P = std::remove_pointer_t<decltype(policy)>;
        if (q.lpr > 1) { // segments
            found = with_segment(q.bs, q.lpr, [&](auto bs_tag, auto lpr_tag) {
                constexpr int BS = decltype(bs_tag)::value, LPR = decltype(lpr_tag)::value;
                hipLaunchKernelGGL((k_query_seg<P, BS, LPR>), dim3(q.blocks), dim3(BS), 0, a.stream, a.consts, a.perm2d,
                                   a.grad, q.rays, q.results, q.steps, q.n, args);
            });
            return;
        }
        with_landscape(a, [&](auto l_tag) {
            hipLaunchKernelGGL((k_query_lanes<decltype(l_tag)::value, P>), dim3(q.blocks), dim3(1024), 0, a.stream,
                               a.consts, a.perm2d, a.grad, q.rays, q.results, q.steps, q.n, args, q.counter, thr);
        });
    });
    return found;
}

// ---------------------------------------------------------------------------
// Shaded queries (rt_terrain_shade_rays): the sample tracescreen.hlsl:16-48 computes for a pixel ray -- the refined
// primary march with fog, then for a hit getNormal, getColor with its shadow march, the fog and sky blends, for a
// miss the sky -- for rays read from memory.  One sample per ray, no AO.  Ray i is the surface queries' two 16-byte
// loads; its result is two 16-byte stores (colour, pd.w | pd.xyz, density), a packed RGBA8 word and two step
// counts (primary, shadow), each where its pointer is set.
namespace {

template <bool STEPS>
__device__ __forceinline__ void store_shade_result(float4* __restrict__ out, uint32_t* __restrict__ out8,
                                                   uint32_t* __restrict__ steps, uint32_t i, f3 col, float dist,
                                                   int shadow_iters)
{
    if (out) gstore(out + 2 * (size_t)i, make_float4(col.x, col.y, col.z, dist));
    if (out8) out8[i] = unorm8(col.x) | (unorm8(col.y) << 8) | (unorm8(col.z) << 16) | 0xff000000u;
    if constexpr (STEPS) steps[2 * (size_t)i + 1] = (uint32_t)shadow_iters;
}

// Lanes (every landscape): k_query_lanes' persistent grid and refill, a lane's ray in one of two marches: PRIMARY
// (refining, to the ray's range and the cap) then, for a hit, SHADOW (skiprefine, to 100, no cap).  Both kinds
// step in the one march_step_with of the loop, skiprefine per lane.  Everything else runs where a wave visits
// the refill point, for all its lanes that ended a march since the last visit:
//   an ended PRIMARY: the sky's scattering; a hit then takes getNormal and getColor up to its shadow ray and goes
//     live again as that ray (SHADOW), a miss takes the space colour, blends and stores;
//   an ended SHADOW: the rest of getColor, the fog and sky blends, the store;
//   a lane without a ray claims one from the query's counter.
// A SHADOW lane carries beside its March the hit's ShadePre, distance, fog and rayleigh term; the hit's position
// is the shadow march's origin and the density is stored when the primary ends.
// The loop ends when the counter has passed n, no lane is live and no lane holds a ray: a visit is due whenever
// the live lanes are few enough and there is something to do (rays to claim, or a lane with an ended march), a
// visit claims at least one ray or moves every ended march on by one phase (of two a ray), and a wave with no
// live lane always visits or leaves.
template <int L, bool STEPS, bool RANGE>
__global__ void __launch_bounds__(1024) k_shadequery(const RtConsts* __restrict__ k, const uint32_t* __restrict__ perm2d,
                                                     const float4* __restrict__ grad, const float4* __restrict__ rays,
                                                     float4* __restrict__ out, uint32_t* __restrict__ out8,
                                                     uint32_t* __restrict__ steps, uint32_t n, SurfArgs a,
                                                     uint32_t* __restrict__ counter, uint32_t refill_live)
{
    RT_DIAG_QUERY_UTIL(uint32_t util_wave = 0, util_lane = 0, util_swave = 0, util_slane = 0;)
    __shared__ __attribute__((aligned(16))) uint32_t lds[kNoiseLdsWords];
    load_noise_lds(lds, perm2d, grad, k);
    Ctx c = make_ctx(k, lds, a.eye);
    const uint32_t lane = threadIdx.x & 63u;
    auto dens = [&](f3 q) { return get_density<L>(c, q); };
    March<L, true> st{};
    ShadePre sp{};                       // SHADOW: getColor's terms before its shadow ray
    f4 pfog = {0.0f, 0.0f, 0.0f, 0.0f}; // SHADOW: the primary's fcolord
    f3 ray = rtm::mk(0.0f, 0.0f, 0.0f); // SHADOW: scat.rayleigh
    float pdist = 0.0f;                  // SHADOW: the primary's pd.w
    float endd = a.t_max;                // the live march's end: the ray's range, 100 for a shadow ray
    uint32_t idx = 0;
    bool has = false, live = false; // has: idx is a ray of the query whose result is not stored yet
    bool shadow = false;            // the lane's march is its ray's shadow march
    bool more = true;               // (uniform) the counter has not passed n
    for (;;) {
        uint64_t lv = __ballot(live);
        if ((uint32_t)__popcll(lv) <= refill_live && (more || __ballot(has && !live))) {
            const bool ended = has && !live;
            RT_DIAG_QUERY_UTIL(if (const uint64_t sm = __ballot(ended && !shadow)) {
                ++util_swave;
                util_slane += (uint32_t)__popcll(sm);
            })
            if (ended && !shadow) { // tracescreen.hlsl:20-38 after the primary march
                const RayResult rr = march_result(st);
                // normalize(dir_i): march_begin's dir * rcp(length(dir)) is rtm::normalize's own product
                const f3 pdn = st.dir;
                if (out) gstore(out + 2 * (size_t)idx + 1, make_float4(rr.pd.x, rr.pd.y, rr.pd.z, rr.density));
                if constexpr (STEPS) steps[2 * (size_t)idx] = (uint32_t)st.iters;
                const SkyColor scat = get_rayleigh_mie(c, pdn);
                if (rr.density > 0.0f) {
                    const f3 hp = rtm::mk(rr.pd.x, rr.pd.y, rr.pd.z);
                    const f3 nrm = get_normal<L>(c, f4{hp.x, hp.y, hp.z, rr.density});
                    sp = shade_pre<L>(c, hp, nrm, pdn, rr.pd.w);
                    pdist = rr.pd.w;
                    if constexpr (March<L, true>::FOG) pfog = rr.fc;
                    ray = scat.rayleigh;
                    // color.hlsl:51 traceRay(p, 0.4, 100, precision, SunDirection, fog, skiprefine)
                    march_begin(c, st, hp, 0.4f, sp.precision, c.sun);
                    endd = 100.0f;
                    shadow = true;
                    live = march_live_skip(c, st, endd, 0, true);
                } else {
                    const float space = get_space_color(c, pdn);
                    const f3 sky = rtm::mk((scat.mie.x + scat.rayleigh.x) + space, (scat.mie.y + scat.rayleigh.y) + space,
                                           (scat.mie.z + scat.rayleigh.z) + space);
                    float sa = rr.pd.w * 0.0005f;
                    sa = rtm::sat(sa * sa);
                    f3 col = rtm::mk(rtm::lerp(sky.x, rr.fc.x, rr.fc.w), rtm::lerp(sky.y, rr.fc.y, rr.fc.w),
                                     rtm::lerp(sky.z, rr.fc.z, rr.fc.w));
                    col = rtm::mk(rtm::lerp(col.x, sky.x, sa), rtm::lerp(col.y, sky.y, sa), rtm::lerp(col.z, sky.z, sa));
                    store_shade_result<STEPS>(out, out8, steps, idx, col, rr.pd.w, 0);
                    has = false;
                }
            }
            if (has && !live && shadow) { // color.hlsl:53-71 after the shadow ray, tracescreen.hlsl:33-35
                f3 col = shade_post(c, sp, st.d, st.f.w);
                float sa = pdist * 0.0005f;
                sa = rtm::sat(sa * sa);
                col = rtm::mk(rtm::lerp(col.x, pfog.x, pfog.w), rtm::lerp(col.y, pfog.y, pfog.w),
                              rtm::lerp(col.z, pfog.z, pfog.w));
                col = rtm::mk(rtm::lerp(col.x, ray.x, sa), rtm::lerp(col.y, ray.y, sa), rtm::lerp(col.z, ray.z, sa));
                store_shade_result<STEPS>(out, out8, steps, idx, col, pdist, st.iters);
                has = false;
                shadow = false;
            }
            if (more) {
                const uint64_t idle = __ballot(!has);
                const uint32_t cnt = (uint32_t)__popcll(idle);
                const uint32_t first = wave_fetch(counter, lane, cnt);
                if (!has) {
                    idx = first + lane_rank(idle);
                    has = idx < n;
                    if (has) {
                        const float4 o = rays[2 * (size_t)idx], d = rays[2 * (size_t)idx + 1];
                        endd = RANGE ? d.w : a.t_max;
                        march_begin(c, st, rtm::mk(o.x, o.y, o.z), RANGE ? o.w : a.t_min, a.stepmod, rtm::mk(d.x, d.y, d.z));
                        live = march_live_skip(c, st, endd, a.max_steps, false);
                    }
                }
                more = first + cnt < n;
            }
            lv = __ballot(live);
        }
        if (!lv) {
            if (!more && !__ballot(has)) break;
            continue; // lanes hold marches that ended before their first step, or there are rays to claim: visit again
        }
        RT_DIAG_QUERY_UTIL(++util_wave; util_lane += (uint32_t)__popcll(lv);)
        if (live) {
            march_step_with<L, true, false>(c, st, dens, shadow);
            live = march_live_skip(c, st, endd, shadow ? 0 : a.max_steps, shadow);
        }
    }
    RT_DIAG_QUERY_UTIL(if (lane == 0) {
        atomicAdd(&g_query_util[0], (unsigned long long)util_wave);
        atomicAdd(&g_query_util[1], (unsigned long long)util_lane);
        atomicAdd(&g_query_util[2], (unsigned long long)util_swave);
        atomicAdd(&g_query_util[3], (unsigned long long)util_slane);
    })
}

} // namespace

bool rt_launch_shadequery(const RtLaunch& a, const RtShadeQuery& q)
{
    if (q.n == 0 || q.blocks == 0) return true;
    if (!q.counter || (!q.results && !q.rgba8)) return false;
    constexpr uint32_t thr = RT_SHADEQ_REFILL < 63 ? RT_SHADEQ_REFILL : 63;
    const SurfArgs sa = surf_args(q.eye, q.march);
    with_landscape(a, [&](auto l_tag) {
        with_steps_range(q.steps != nullptr, q.march.ray_range, [&](auto steps_tag, auto range_tag) {
            constexpr bool STEPS = decltype(steps_tag)::value, RANGE = decltype(range_tag)::value;
            hipLaunchKernelGGL((k_shadequery<decltype(l_tag)::value, STEPS, RANGE>), dim3(q.blocks), dim3(1024), 0,
                               a.stream, a.consts, a.perm2d, a.grad, q.rays, q.results, q.rgba8, q.steps, q.n, sa,
                               q.counter, thr);
        });
    });
    return true;
}

// ---------------------------------------------------------------------------
// Point shading (rt_terrain_shade_points): getColor with its shadow ray and the AO factor of K hemisphere rays at
// points the caller holds, as a frame computes both for a pixel whose primary ray ended there -- no primary march,
// no fog or sky blend.  Point i is two 16-byte loads (x y z _ | nx ny nz _); its result is one 16-byte store
// (colour, ao), a packed RGBA8 word (ao times the saturated colour) and two step counts (shadow, the AO rays'
// sum), each where its pointer is set.
namespace {

// (wave-uniform) the LOD eye and viewpoint, the AO rays a point and the hash's py
struct PointArgs {
    QueryEye eye;
    uint32_t ao, seed;
};

// Lanes (every landscape): k_shadequery's persistent grid and refill, a lane's point in one of 1 + K marches, one
// after another: SHADOW (to 100, with fog), then AO ray 0 .. K - 1 (to 25, without).  `phase` counts the marches
// begun after the shadow's: 0 is SHADOW, k + 1 is AO ray k.  All are skiprefine and step in the one
// march_step_with of the loop.  Everything else runs where a wave visits the refill point, for all its lanes
// that ended a march since the last visit:
//   an ended SHADOW: the rest of getColor; the colour takes the place of the albedo in the lane's ShadePre;
//   an ended AO ray: its occlusion is counted;
//   either then begins the point's next AO ray, or after the last stores the point;
//   a lane without a point claims one from the query's counter, takes getColor up to its shadow ray (on
//     nomadplains the 20-octave colour FBM, so for all the newly claimed lanes together) and begins that ray.
// A lane carries beside its March the point's ShadePre (the shadow stepmod is the AO rays' too), its normal and
// the counts; the position is the marches' origin (March::p).
// The loop ends when the counter has passed n, no lane is live and no lane holds a point: a visit is due whenever
// the live lanes are few enough and there is something to do (points to claim, or a lane with an ended march), a
// visit claims at least one point or moves every ended march on by one phase (of 1 + K a point, the last one's
// end being the store), and a wave with no live lane always visits or leaves.
template <int L, bool STEPS>
__global__ void __launch_bounds__(1024) k_shadepoints(const RtConsts* __restrict__ k, const uint32_t* __restrict__ perm2d,
                                                      const float4* __restrict__ grad, const float4* __restrict__ points,
                                                      const float4* __restrict__ normals, float4* __restrict__ out,
                                                      uint32_t* __restrict__ out8, uint32_t* __restrict__ steps,
                                                      uint32_t n, PointArgs a, uint32_t* __restrict__ counter,
                                                      uint32_t refill_live)
{
    // (diagnostic) this wave's march steps and its live lanes summed over them; its visits that began shadow rays
    // (the colour's FBM), and their lanes
    RT_DIAG_QUERY_UTIL(uint32_t util_wave = 0, util_lane = 0, util_swave = 0, util_slane = 0;)
    __shared__ __attribute__((aligned(16))) uint32_t lds[kNoiseLdsWords];
    load_noise_lds(lds, perm2d, grad, k);
    Ctx c = make_ctx(k, lds, a.eye);
    const uint32_t lane = threadIdx.x & 63u;
    auto dens = [&](f3 q) { return get_density<L>(c, q); };
    March<L, true> st{};
    ShadePre sp{};                       // getColor's terms before its shadow ray; col: the colour once that ray ended
    f3 nrm = rtm::mk(0.0f, 0.0f, 0.0f); // n_i
    uint32_t idx = 0, phase = 0, occ = 0;
    uint32_t it_shadow = 0, it_ao = 0; // (STEPS) the shadow march's iterations, the ended AO marches' sum
    bool has = false, live = false;    // has: idx is a point of the query whose result is not stored yet
    bool more = true;                  // (uniform) the counter has not passed n
    for (;;) {
        uint64_t lv = __ballot(live);
        if ((uint32_t)__popcll(lv) <= refill_live && (more || __ballot(has && !live))) {
            if (has && !live) {
                if (phase == 0u) { // color.hlsl:53-71 after the shadow ray
                    const f3 col = shade_post(c, sp, st.d, st.f.w);
                    sp.col[0] = col.x;
                    sp.col[1] = col.y;
                    sp.col[2] = col.z;
                    if constexpr (STEPS) it_shadow = (uint32_t)st.iters;
                } else { // ambient_occlusion's count
                    if (st.d > 0.0f) ++occ;
                    if constexpr (STEPS) it_ao += (uint32_t)st.iters;
                }
                if (phase < a.ao) { // AO ray `phase` (rt_shader.h ao_dir: px = i, py = seed, a = 0)
                    march_begin(c, st, st.p, 0.4f, sp.precision, ao_dir(nrm, idx, a.seed, 0u, phase), false);
                    ++phase;
                    live = march_live<L, true, true>(c, st, RT_AO_END, 0);
                } else {
                    const float ao = a.ao ? ao_factor(occ, (int)a.ao) : 1.0f;
                    if (out) gstore(out + idx, make_float4(sp.col[0], sp.col[1], sp.col[2], ao));
                    if (out8)
                        out8[idx] = unorm8(rtm::sat(sp.col[0]) * ao) | (unorm8(rtm::sat(sp.col[1]) * ao) << 8) |
                                    (unorm8(rtm::sat(sp.col[2]) * ao) << 16) | 0xff000000u;
                    if constexpr (STEPS) {
                        steps[2 * (size_t)idx] = it_shadow;
                        steps[2 * (size_t)idx + 1] = it_ao;
                    }
                    has = false;
                }
            }
            if (more) {
                const uint64_t idle = __ballot(!has);
                const uint32_t cnt = (uint32_t)__popcll(idle);
                const uint32_t first = wave_fetch(counter, lane, cnt);
                bool fresh = false;
                if (!has) {
                    idx = first + lane_rank(idle);
                    has = fresh = idx < n;
                }
                RT_DIAG_QUERY_UTIL(if (const uint64_t sm = __ballot(fresh)) {
                    ++util_swave;
                    util_slane += (uint32_t)__popcll(sm);
                })
                if (fresh) {
                    const float4 pw = points[idx], nw = normals[idx];
                    const f3 p = rtm::mk(pw.x, pw.y, pw.z), v = rtm::sub(p, c.eye);
                    nrm = rtm::mk(nw.x, nw.y, nw.z);
                    sp = shade_pre<L>(c, p, nrm, rtm::normalize(v), rtm::length(v));
                    phase = 0u;
                    occ = 0u;
                    it_ao = 0u;
                    // color.hlsl:51 traceRay(p, 0.4, 100, precision, SunDirection, fog, skiprefine)
                    march_begin(c, st, p, 0.4f, sp.precision, c.sun);
                    live = march_live<L, true, true>(c, st, 100.0f, 0);
                }
                more = first + cnt < n;
            }
            lv = __ballot(live);
        }
        if (!lv) {
            if (!more && !__ballot(has)) break;
            continue; // lanes hold marches that ended before their first step, or there are points to claim: visit again
        }
        RT_DIAG_QUERY_UTIL(++util_wave; util_lane += (uint32_t)__popcll(lv);)
        if (live) {
            march_step_with<L, true, false>(c, st, dens, /*skiprefine*/ true);
            live = march_live<L, true, true>(c, st, phase ? RT_AO_END : 100.0f, 0);
        }
    }
    RT_DIAG_QUERY_UTIL(if (lane == 0) {
        atomicAdd(&g_query_util[0], (unsigned long long)util_wave);
        atomicAdd(&g_query_util[1], (unsigned long long)util_lane);
        atomicAdd(&g_query_util[2], (unsigned long long)util_swave);
        atomicAdd(&g_query_util[3], (unsigned long long)util_slane);
    })
}

} // namespace

bool rt_launch_shadepoints(const RtLaunch& a, const RtPointQuery& q)
{
    if (q.n == 0 || q.blocks == 0) return true;
    if (!q.counter || !q.points || !q.normals || (!q.results && !q.rgba8) || q.ao_samples > 16u) return false;
    // the live-lane count at or below which a wave visits its refill point (RT_POINTQ_REFILL; at most 63)
    constexpr uint32_t thr = RT_POINTQ_REFILL < 63 ? RT_POINTQ_REFILL : 63;
    const PointArgs pa{{q.eye[0], q.eye[1], q.eye[2]}, q.ao_samples, q.seed};
    with_landscape(a, [&](auto l_tag) {
        with_bool(q.steps != nullptr, [&](auto steps_tag) {
            hipLaunchKernelGGL((k_shadepoints<decltype(l_tag)::value, decltype(steps_tag)::value>), dim3(q.blocks),
                               dim3(1024), 0, a.stream, a.consts, a.perm2d, a.grad, q.points, q.normals, q.results,
                               q.rgba8, q.steps, q.n, pa, q.counter, thr);
        });
    });
    return true;
}

// ---------------------------------------------------------------------------
// Field queries (rt_terrain_sample_field, rt_terrain_sample_lattice): getDensity, and with NORMAL getNormal
// (tracing.hlsl:107-116, for every point, inside or outside), at points instead of along rays.  The eye (nomadplains'
// octave count, getNormal's eps) is a kernel argument, as in the ray queries.  A point's result is one float, or with
// NORMAL one float4 {n.xyz, d}.  One 1024-thread block per CU at most (the noise tables fill its LDS); a block
// strides over the work, so the tables are loaded once per block whatever the size of the query.
namespace {

template <int L, bool NORMAL>
__device__ __forceinline__ void store_field_result(const Ctx& c, f3 p, float d, void* __restrict__ out, uint32_t i)
{
    if constexpr (NORMAL) {
        const f3 nrm = get_normal<L>(c, f4{p.x, p.y, p.z, d});
        gstore((float4*)out + i, make_float4(nrm.x, nrm.y, nrm.z, d));
    } else {
        ((float*)out)[i] = d;
    }
}

// Points from memory: point i is one 16-byte load (x y z _), tiles of 1024 consecutive points dealt to the blocks
// round robin.  n <= 2^26.
template <int L, bool NORMAL>
__global__ void __launch_bounds__(1024) k_fieldpoints(const RtConsts* __restrict__ k, const uint32_t* __restrict__ perm2d,
                                                      const float4* __restrict__ grad,
                                                      const float4* __restrict__ points, void* __restrict__ out,
                                                      uint32_t n, QueryEye e)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[kNoiseLdsWords];
    load_noise_lds(lds, perm2d, grad, k);
    Ctx c = make_ctx(k, lds, e);
    const uint32_t tiles = (n + 1023u) / 1024u;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t i = t * 1024u + threadIdx.x;
        if (i < n) {
            const float4 q = points[i];
            const f3 p = rtm::mk(q.x, q.y, q.z);
            store_field_result<L, NORMAL>(c, p, get_density<L>(c, p), out, i);
        }
    }
}

// A lattice: point (ix, iy, iz) at fmaf(i, spacing, origin) per axis, result index (iz * ny + iy) * nx + ix; no
// coordinates are read.  A wave takes strips of 64 consecutive ix by `rows` consecutive iy of one iz and walks
// them in y: its stores are whole rows, its hit ballot is the strip row's two occupancy words (each written once,
// whole, by one lane), and all its lanes share y, so the wave tests of the density (terraces, floor lift, pow)
// skip as often as they can.  With COLUMN (nomadplains) a lane computes the steep noise of its (ix, iz) column
// once per strip.  nx * ny * nz <= 2^26; out or occ may be null (not both).
struct FieldLattice {
    float ox, oy, oz, sx, sy, sz;
    uint32_t nx, ny, nz, rows;
};

template <int L, bool NORMAL, bool COLUMN>
__global__ void __launch_bounds__(1024) k_fieldlattice(const RtConsts* __restrict__ k, const uint32_t* __restrict__ perm2d,
                                                       const float4* __restrict__ grad, void* __restrict__ out,
                                                       uint32_t* __restrict__ occ, FieldLattice g, QueryEye e)
{
    static_assert(!COLUMN || L == RT_NOMADPLAINS, "the column shape is nomadplains'");
    __shared__ __attribute__((aligned(16))) uint32_t lds[kNoiseLdsWords];
    load_noise_lds(lds, perm2d, grad, k);
    Ctx c = make_ctx(k, lds, e);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const uint32_t xc = (g.nx + 63u) / 64u, yc = (g.ny + g.rows - 1u) / g.rows, strips = xc * yc * g.nz;
    const uint32_t words = (g.nx + 31u) / 32u; // occupancy words per (iy, iz) row
    for (uint32_t s = blockIdx.x * waves + wave; s < strips; s += gridDim.x * waves) {
        const uint32_t cx = s % xc, r = s / xc, cy = r % yc, iz = r / yc;
        const uint32_t ix = cx * 64u + lane, iy0 = cy * g.rows, iy1 = iy0 + g.rows < g.ny ? iy0 + g.rows : g.ny;
        const bool valid = ix < g.nx;
        const float px = fmaf((float)ix, g.sx, g.ox), pz = fmaf((float)iz, g.sz, g.oz);
        float sn = 0.0f;
        if constexpr (COLUMN) {
            if (valid) sn = np_steep_noise(c, rtm::mk(px, 0.0f, pz));
        }
        for (uint32_t iy = iy0; iy < iy1; ++iy) {
            const uint32_t row = iz * g.ny + iy;
            float d = 0.0f;
            if (valid) {
                const f3 p = rtm::mk(px, fmaf((float)iy, g.sy, g.oy), pz);
                if constexpr (COLUMN) d = density_nomadplains_column(c, p, sn);
                else d = get_density<L>(c, p);
                if (out) store_field_result<L, NORMAL>(c, p, d, out, row * g.nx + ix);
            }
            if (occ) {
                const uint64_t hit = __ballot(valid && d > 0.0f); // tracescreen.hlsl:29
                const uint32_t w = cx * 2u + (lane >> 5);
                if ((lane & 31u) == 0u && w < words) occ[(size_t)row * words + w] = (uint32_t)(hit >> (lane & 32u));
            }
        }
    }
}

template <int L, bool NORMAL>
void launch_fieldquery(const RtLaunch& a, const RtFieldQuery& q)
{
    const QueryEye e{q.eye[0], q.eye[1], q.eye[2]};
    if (q.points) {
        hipLaunchKernelGGL((k_fieldpoints<L, NORMAL>), dim3(q.blocks), dim3(1024), 0, a.stream, a.consts, a.perm2d,
                           a.grad, q.points, q.results, q.n, e);
        return;
    }
    const FieldLattice g{q.origin[0], q.origin[1], q.origin[2], q.spacing[0], q.spacing[1], q.spacing[2],
                         q.dims[0],   q.dims[1],   q.dims[2],   RT_FIELD_ROWS > 0 ? (uint32_t)RT_FIELD_ROWS : q.rows};
    if constexpr (L == RT_NOMADPLAINS) {
        if (q.column && RT_FIELD_COLUMN) {
            hipLaunchKernelGGL((k_fieldlattice<L, NORMAL, true>), dim3(q.blocks), dim3(1024), 0, a.stream, a.consts,
                               a.perm2d, a.grad, q.results, q.occupancy, g, e);
            return;
        }
    }
    hipLaunchKernelGGL((k_fieldlattice<L, NORMAL, false>), dim3(q.blocks), dim3(1024), 0, a.stream, a.consts, a.perm2d,
                       a.grad, q.results, q.occupancy, g, e);
}

} // namespace

bool rt_launch_fieldquery(const RtLaunch& a, const RtFieldQuery& q)
{
    if (q.n == 0 || q.blocks == 0) return true;
    if (q.points ? !q.results : ((!q.results && !q.occupancy) || q.rows == 0)) return false;
    with_landscape(a, [&](auto l_tag) {
        // occupancy alone needs no normal
        with_bool(q.normal && q.results, [&](auto normal_tag) {
            launch_fieldquery<decltype(l_tag)::value, decltype(normal_tag)::value>(a, q);
        });
    });
    return true;
}

// ---------------------------------------------------------------------------
// Mesh extraction (rt_terrain_extract_mesh): a surface-nets mesh of a lattice whose densities and occupancy words
// k_fieldlattice has written (include/frosttrace.h has the definition, rt_rayquery.h the scratch layout and the
// mask arithmetic).  Four passes on one stream; the counts stay in device memory and every pass reads them there.
namespace {

struct MeshGrid {
    float ox, oy, oz, sx, sy, sz;
    uint32_t nx, ny, nz;       // points; all >= 2
    uint32_t row_words, words; // mask words per cell row and in all
};

// Classification from the occupancy bits alone: one thread per mask word (64 consecutive cx of one cell row)
// reads the words of the row's four point rows and stores the word's four masks and its vertex and quad counts.
__global__ void __launch_bounds__(rtq::kMeshThreads) k_meshcount(const uint32_t* __restrict__ occ, uint64_t* __restrict__ masks,
                                                    uint2* __restrict__ offsets, MeshGrid g)
{
    const uint32_t occ_words = (g.nx + 31u) / 32u;
    for (uint32_t w = blockIdx.x * rtq::kMeshThreads + threadIdx.x; w < g.words; w += gridDim.x * rtq::kMeshThreads) {
        const uint32_t j = w % g.row_words, row = w / g.row_words, cy = row % (g.ny - 1u), cz = row / (g.ny - 1u);
        const uint32_t* r00 = occ + ((size_t)cz * g.ny + cy) * occ_words;
        const uint32_t* r01 = r00 + (size_t)g.ny * occ_words;
        const rtq::MeshMasks m = rtq::mesh_masks(r00, r00 + occ_words, r01, r01 + occ_words, occ_words, j, g.nx, cy, cz);
        ulonglong2* out = reinterpret_cast<ulonglong2*>(masks) + 2 * (size_t)w;
        out[0] = make_ulonglong2(m.active, m.ex);
        out[1] = make_ulonglong2(m.ey, m.ez);
        offsets[w] = make_uint2(rtq::mesh_popc(m.active), rtq::mesh_popc(m.ex) + rtq::mesh_popc(m.ey) + rtq::mesh_popc(m.ez));
    }
}

__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// The exclusive scan of the words' counts, in place, by one block: chunks of 4096 words (4 consecutive words a
// thread: a wave scan, the 16 wave totals through LDS, the running totals in every thread), then the mesh's totals
// to counts: vertices, triangles (two a quad).  A lattice of 2^26 points in full rows has 2^20 words: 256 chunks.
__global__ void __launch_bounds__(1024) k_meshscan(uint2* __restrict__ offsets, uint32_t words,
                                                   uint32_t* __restrict__ counts)
{
    __shared__ uint2 s_wave[16];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t run_v = 0, run_q = 0;
    uint2 c[4], next[4];
    auto load = [&](uint32_t base, uint2(&into)[4]) {
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            const uint32_t w = base + threadIdx.x * 4u + i;
            into[i] = w < words ? offsets[w] : make_uint2(0u, 0u);
        }
    };
    load(0u, c);
    for (uint32_t base = 0; base < words; base += 4096u) {
        const uint32_t w0 = base + threadIdx.x * 4u;
        load(base + 4096u, next); // the next chunk's counts arrive while this one is scanned
        uint32_t tv = 0, tq = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            tv += c[i].x;
            tq += c[i].y;
        }
        const uint32_t iv = wave_inclusive_sum(tv, lane), iq = wave_inclusive_sum(tq, lane);
        if (lane == 63u) s_wave[wave] = make_uint2(iv, iq);
        __syncthreads();
        uint32_t ev = run_v + iv - tv, eq = run_q + iq - tq; // what precedes this thread's first word
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) {
            const uint2 t = s_wave[k];
            if (k < wave) {
                ev += t.x;
                eq += t.y;
            }
            run_v += t.x;
            run_q += t.y;
        }
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            if (w0 + i < words) offsets[w0 + i] = make_uint2(ev, eq);
            ev += c[i].x;
            eq += c[i].y;
        }
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) c[i] = next[i];
        __syncthreads(); // s_wave is rewritten by the next chunk
    }
    if (threadIdx.x == 0) {
        counts[0] = run_v;
        counts[1] = 2u * run_q;
    }
}

// the index of the vertex of active cell (cx, cy, cz): the vertices before its word and those of the word's lower bits
__device__ __forceinline__ uint32_t mesh_vertex_index(const uint64_t* __restrict__ masks, const uint2* __restrict__ offsets,
                                                      const MeshGrid& g, uint32_t cx, uint32_t cy, uint32_t cz)
{
    const size_t w = ((size_t)cz * (g.ny - 1u) + cy) * g.row_words + (cx >> 6);
    return offsets[w].x + rtq::mesh_popc(masks[4 * w] & ((1ull << (cx & 63u)) - 1ull));
}

// one crossing of a cell: edge E (0..11, the header's order) between corners A and B of the 8 densities d
template <int E>
__device__ __forceinline__ void mesh_crossing(const float (&d)[8], float& sx, float& sy, float& sz, uint32_t& n)
{
    constexpr int AXIS = E >> 2, P = E & 1, Q = (E >> 1) & 1;
    // the corner offsets on the other two axes, the lower axis first
    constexpr int KX = AXIS == 0 ? 0 : P, KY = AXIS == 0 ? P : (AXIS == 1 ? 0 : Q), KZ = AXIS == 2 ? 0 : Q;
    constexpr int A = KX + 2 * KY + 4 * KZ, B = A + (1 << AXIS);
    const float da = d[A], db = d[B];
    if ((da > 0.0f) != (db > 0.0f)) {
        const float t = __fdiv_rn(da, __fsub_rn(da, db));
        sx = __fadd_rn(sx, AXIS == 0 ? t : (float)KX);
        sy = __fadd_rn(sy, AXIS == 1 ? t : (float)KY);
        sz = __fadd_rn(sz, AXIS == 2 ? t : (float)KZ);
        ++n;
    }
}

// the two triangles of quad q over the vertices A B C D, wound by the lower endpoint's side
__device__ __forceinline__ void mesh_store_quad(uint32_t* __restrict__ tri, uint32_t max_triangles, uint32_t q,
                                                bool inside, uint32_t A, uint32_t B, uint32_t C, uint32_t D)
{
    const uint32_t second = inside ? B : D, fourth = inside ? D : B;
    uint32_t* t = tri + 6 * (size_t)q;
    if (2u * q < max_triangles) {
        t[0] = A;
        t[1] = second;
        t[2] = C;
    }
    if (2u * q + 1u < max_triangles) {
        t[3] = A;
        t[4] = C;
        t[5] = fourth;
    }
}

// Vertices and indices: a wave takes a mask word, a lane a cell.  An active cell reads its 8 densities, places its
// vertex and stores it at the word's offset plus the active cells below it in the word; each edge bit stores its
// quad's 6 indices at the word's quad offset plus the edge bits below it in (cell, axis) order.  Every store is
// guarded by its capacity.
__global__ void __launch_bounds__(rtq::kMeshThreads) k_meshemit(const float* __restrict__ dens, const uint64_t* __restrict__ masks,
                                                   const uint2* __restrict__ offsets, MeshGrid g,
                                                   float4* __restrict__ vertices, uint32_t max_vertices,
                                                   uint32_t* __restrict__ tri, uint32_t max_triangles)
{
    const uint32_t lane = threadIdx.x & 63u, waves = blockDim.x >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t w = blockIdx.x * waves + (threadIdx.x >> 6); w < g.words; w += gridDim.x * waves) {
        const uint64_t act = masks[4 * (size_t)w];
        if (!((act >> lane) & 1ull)) continue; // (every cell with an edge bit is active)
        const uint64_t ex = masks[4 * (size_t)w + 1], ey = masks[4 * (size_t)w + 2], ez = masks[4 * (size_t)w + 3];
        const uint2 off = offsets[w];
        const uint32_t j = w % g.row_words, row = w / g.row_words, cy = row % (g.ny - 1u), cz = row / (g.ny - 1u);
        const uint32_t cx = j * 64u + lane;
        const size_t p0 = ((size_t)cz * g.ny + cy) * g.nx + cx, dy = g.nx, dz = (size_t)g.nx * g.ny;
        const float d[8] = {dens[p0],      dens[p0 + 1],      dens[p0 + dy],      dens[p0 + dy + 1],
                            dens[p0 + dz], dens[p0 + dz + 1], dens[p0 + dz + dy], dens[p0 + dz + dy + 1]};
        float lx = 0.0f, ly = 0.0f, lz = 0.0f;
        uint32_t n = 0;
        mesh_crossing<0>(d, lx, ly, lz, n);
        mesh_crossing<1>(d, lx, ly, lz, n);
        mesh_crossing<2>(d, lx, ly, lz, n);
        mesh_crossing<3>(d, lx, ly, lz, n);
        mesh_crossing<4>(d, lx, ly, lz, n);
        mesh_crossing<5>(d, lx, ly, lz, n);
        mesh_crossing<6>(d, lx, ly, lz, n);
        mesh_crossing<7>(d, lx, ly, lz, n);
        mesh_crossing<8>(d, lx, ly, lz, n);
        mesh_crossing<9>(d, lx, ly, lz, n);
        mesh_crossing<10>(d, lx, ly, lz, n);
        mesh_crossing<11>(d, lx, ly, lz, n);
        const float cnt = (float)n;
        lx = __fdiv_rn(lx, cnt);
        ly = __fdiv_rn(ly, cnt);
        lz = __fdiv_rn(lz, cnt);
        const uint32_t vi = off.x + rtq::mesh_popc(act & below);
        if (vi < max_vertices) {
            const uint32_t cell = (cz * (g.ny - 1u) + cy) * (g.nx - 1u) + cx;
            gstore(vertices + vi, make_float4(fmaf(__fadd_rn((float)cx, lx), g.sx, g.ox),
                                              fmaf(__fadd_rn((float)cy, ly), g.sy, g.oy),
                                              fmaf(__fadd_rn((float)cz, lz), g.sz, g.oz), __uint_as_float(cell)));
        }
        const uint32_t bx = (uint32_t)(ex >> lane) & 1u, by = (uint32_t)(ey >> lane) & 1u, bz = (uint32_t)(ez >> lane) & 1u;
        if (!(bx | by | bz)) continue;
        const uint32_t q = off.y + rtq::mesh_popc(ex & below) + rtq::mesh_popc(ey & below) + rtq::mesh_popc(ez & below);
        const bool inside = d[0] > 0.0f;
        // the cells around the edge from corner 0 along the axis: A = c - u - v, B = c - v, C = c, D = c - u with
        // (u, v) the next two axes in cyclic order
        if (bx) // u = y, v = z
            mesh_store_quad(tri, max_triangles, q, inside, mesh_vertex_index(masks, offsets, g, cx, cy - 1u, cz - 1u),
                            mesh_vertex_index(masks, offsets, g, cx, cy, cz - 1u), vi,
                            mesh_vertex_index(masks, offsets, g, cx, cy - 1u, cz));
        if (by) // u = z, v = x
            mesh_store_quad(tri, max_triangles, q + bx, inside, mesh_vertex_index(masks, offsets, g, cx - 1u, cy, cz - 1u),
                            mesh_vertex_index(masks, offsets, g, cx - 1u, cy, cz), vi,
                            mesh_vertex_index(masks, offsets, g, cx, cy, cz - 1u));
        if (bz) // u = x, v = y
            mesh_store_quad(tri, max_triangles, q + bx + by, inside,
                            mesh_vertex_index(masks, offsets, g, cx - 1u, cy - 1u, cz),
                            mesh_vertex_index(masks, offsets, g, cx, cy - 1u, cz), vi,
                            mesh_vertex_index(masks, offsets, g, cx - 1u, cy, cz));
    }
}

// The normal pass: k_fieldpoints over the compacted vertices (x y z, the cell word ignored) -> {getNormal,
// getDensity}, its bound min(counts[0], max_vertices) read from device memory.
template <int L>
__global__ void __launch_bounds__(1024) k_meshnormals(const RtConsts* __restrict__ k, const uint32_t* __restrict__ perm2d,
                                                      const float4* __restrict__ grad,
                                                      const float4* __restrict__ vertices, float4* __restrict__ out,
                                                      const uint32_t* __restrict__ counts, uint32_t max_vertices,
                                                      QueryEye e)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[kNoiseLdsWords];
    load_noise_lds(lds, perm2d, grad, k);
    Ctx c = make_ctx(k, lds, e);
    const uint32_t have = counts[0], n = have < max_vertices ? have : max_vertices;
    const uint32_t tiles = (n + 1023u) / 1024u;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t i = t * 1024u + threadIdx.x;
        if (i < n) {
            const float4 q = vertices[i];
            const f3 p = rtm::mk(q.x, q.y, q.z);
            store_field_result<L, true>(c, p, get_density<L>(c, p), out, i);
        }
    }
}

} // namespace

bool rt_launch_meshquery(const RtLaunch& a, const RtMeshQuery& q)
{
    if (q.words == 0 || q.dims[0] < 2u || q.dims[1] < 2u || q.dims[2] < 2u) return false;
    if (!q.density || !q.occupancy || !q.masks || !q.offsets || !q.counts) return false;
    if ((q.max_vertices && !q.vertices) || (q.max_triangles && !q.triangles)) return false;
    if (q.count_blocks == 0 || q.emit_blocks == 0 || (q.normals && q.max_vertices && q.normal_blocks == 0)) return false;
    const MeshGrid g{q.origin[0], q.origin[1], q.origin[2], q.spacing[0], q.spacing[1], q.spacing[2],
                     q.dims[0],   q.dims[1],   q.dims[2],   q.row_words,  q.words};
    uint2* offsets = reinterpret_cast<uint2*>(q.offsets);
    hipLaunchKernelGGL(k_meshcount, dim3(q.count_blocks), dim3(rtq::kMeshThreads), 0, a.stream, q.occupancy, q.masks, offsets, g);
    hipLaunchKernelGGL(k_meshscan, dim3(1), dim3(1024), 0, a.stream, offsets, q.words, q.counts);
    if (q.max_vertices || q.max_triangles) // (a counting call stores nothing)
        hipLaunchKernelGGL(k_meshemit, dim3(q.emit_blocks), dim3(rtq::kMeshThreads), 0, a.stream, q.density, q.masks, offsets, g,
                           q.vertices, q.max_vertices, q.triangles, q.max_triangles);
    if (q.normals && q.max_vertices) {
        const QueryEye e{q.eye[0], q.eye[1], q.eye[2]};
        with_landscape(a, [&](auto l_tag) {
            hipLaunchKernelGGL((k_meshnormals<decltype(l_tag)::value>), dim3(q.normal_blocks), dim3(1024), 0, a.stream,
                               a.consts, a.perm2d, a.grad, q.vertices, q.normals, q.counts, q.max_vertices, e);
        });
    }
    return true;
}

// ---------------------------------------------------------------------------
// Distance fields (rt_terrain_distance_field): the exact squared lattice distance of every point to the nearest
// point of the other state, from the occupancy words alone (include/frosttrace.h has the definition, rt_rayquery.h
// the scratch layout and the row arithmetic).  A separable transform to both sets, inside and outside, in three
// passes on one stream.  Every pass takes a thread a point in result order, so consecutive lanes are consecutive
// ix (a wave may run over a row's end into the next row) and every load and store of a wave is a run of
// consecutive words.  The y and z passes scan outward from the point, o = 1, 2, ..., and stop once o * o can no
// longer improve on the best found (or o passes max_cells): exact, with no per-thread stack and no LDS.  Every
// loop is bounded by a dim.
namespace {

struct DistGrid {
    uint32_t nx, ny, nz, points;
    uint32_t reach, limit2; // rtq::distance_bound
};

// the x pass: the row distances to both sets (rtq::dist_row_pack), 16 bits each.  The lanes of one occupancy word
// walk the row's words together, so those loads are the same address in 32 lanes.
__global__ void __launch_bounds__(rtq::kDistThreads) k_distrows(const uint32_t* __restrict__ occ, uint32_t* __restrict__ rows,
                                                               DistGrid g)
{
    const uint32_t words = (g.nx + 31u) / 32u;
    for (uint32_t i = blockIdx.x * rtq::kDistThreads + threadIdx.x; i < g.points; i += gridDim.x * rtq::kDistThreads) {
        const uint32_t row = i / g.nx, ix = i - row * g.nx;
        const rtq::DistRowWord r = rtq::dist_row_word(occ + (size_t)row * words, g.nx, ix >> 5);
        rows[i] = rtq::dist_row_pack(r, ix & 31u);
    }
}

// one neighbour of the y pass at offset o (oo = o * o): its row distances folded into both bests
__device__ __forceinline__ void dist_fold_row(uint32_t w, uint32_t oo, uint32_t& best_in, uint32_t& best_out)
{
    const uint32_t a = w & 0xffffu, b = w >> 16;
    if (a != rtq::kDistRowFar) best_in = min(best_in, a * a + oo);
    if (b != rtq::kDistRowFar) best_out = min(best_out, b * b + oo);
}

// the y pass: h(iy) = min over k of g(k)^2 + (iy - k)^2 down the column (ix, iz), for both sets, into the two planes
__global__ void __launch_bounds__(rtq::kDistThreads) k_distcolumns(const uint32_t* __restrict__ rows, uint32_t* __restrict__ planes,
                                                                  DistGrid g)
{
    for (uint32_t i = blockIdx.x * rtq::kDistThreads + threadIdx.x; i < g.points; i += gridDim.x * rtq::kDistThreads) {
        const uint32_t iy = (i / g.nx) % g.ny, up = iy, down = g.ny - 1u - iy;
        uint32_t best_in = rtq::kDistFar, best_out = rtq::kDistFar;
        dist_fold_row(rows[i], 0u, best_in, best_out);
        const uint32_t span = up > down ? up : down, last = span < g.reach ? span : g.reach;
        for (uint32_t o = 1u; o <= last; ++o) {
            const uint32_t oo = o * o;
            if (oo >= best_in && oo >= best_out) break;
            if (o <= up) dist_fold_row(rows[i - o * g.nx], oo, best_in, best_out);
            if (o <= down) dist_fold_row(rows[i + o * g.nx], oo, best_in, best_out);
        }
        planes[i] = best_in;
        planes[(size_t)g.points + i] = best_out;
    }
}

// the z pass: the same down the column (ix, iy) over the plane of the set the point is not in, then max_cells and
// the stores.  RT_DIST_FAR is never added to.
__global__ void __launch_bounds__(rtq::kDistThreads) k_distfinish(const uint32_t* __restrict__ occ, const uint32_t* __restrict__ planes,
                                                                 uint32_t* __restrict__ d2_out, float* __restrict__ dist_out,
                                                                 float abs_spacing, DistGrid g)
{
    const uint32_t words = (g.nx + 31u) / 32u, plane = g.nx * g.ny;
    for (uint32_t i = blockIdx.x * rtq::kDistThreads + threadIdx.x; i < g.points; i += gridDim.x * rtq::kDistThreads) {
        const uint32_t row = i / g.nx, ix = i - row * g.nx, iz = row / g.ny, up = iz, down = g.nz - 1u - iz;
        const bool inside = (occ[(size_t)row * words + (ix >> 5)] >> (ix & 31u)) & 1u;
        const uint32_t* __restrict__ h = planes + (inside ? (size_t)g.points : 0); // an inside point: the outside set
        uint32_t best = h[i];
        const uint32_t span = up > down ? up : down, last = span < g.reach ? span : g.reach;
        for (uint32_t o = 1u; o <= last; ++o) {
            const uint32_t oo = o * o;
            if (oo >= best) break;
            if (o <= up) {
                const uint32_t v = h[i - o * plane];
                if (v != rtq::kDistFar) best = min(best, v + oo);
            }
            if (o <= down) {
                const uint32_t v = h[i + o * plane];
                if (v != rtq::kDistFar) best = min(best, v + oo);
            }
        }
        const uint32_t d2 = best > g.limit2 ? rtq::kDistFar : best;
        if (d2_out) d2_out[i] = d2;
        if (dist_out) {
            const float d = d2 == rtq::kDistFar ? __builtin_inff() : rtm::sqrt((float)d2) * abs_spacing;
            dist_out[i] = inside ? -d : d;
        }
    }
}

} // namespace

bool rt_launch_distancequery(const RtLaunch& a, const RtDistanceQuery& q)
{
    const uint64_t points = (uint64_t)q.dims[0] * q.dims[1] * q.dims[2];
    if (points == 0 || points > (1u << 26) || q.blocks == 0) return false;
    if (q.dims[0] > rtq::kMaxLatticeDim || q.dims[1] > rtq::kMaxLatticeDim || q.dims[2] > rtq::kMaxLatticeDim) return false;
    if (!q.occupancy || !q.rows || !q.planes || (!q.d2 && !q.distance)) return false;
    const DistGrid g{q.dims[0], q.dims[1], q.dims[2], (uint32_t)points, q.reach, q.limit2};
    const dim3 grid(q.blocks), block(rtq::kDistThreads);
    hipLaunchKernelGGL(k_distrows, grid, block, 0, a.stream, q.occupancy, q.rows, g);
    hipLaunchKernelGGL(k_distcolumns, grid, block, 0, a.stream, q.rows, q.planes, g);
    hipLaunchKernelGGL(k_distfinish, grid, block, 0, a.stream, q.occupancy, q.planes, q.d2, q.distance, q.abs_spacing, g);
    return true;
}

// ---------------------------------------------------------------------------
// Path fields (rt_terrain_path_field): the cost of the cheapest 3-4-5 chamfer path from the seeds to every point
// through the passable points, and its first move (include/frosttrace.h has the definition, rt_rayquery.h the
// schedule, the tiles, the moves and the scratch layout).  The cost is the least fixed point of an integer
// relaxation, so the order of the relaxations is free: a sweep launch relaxes every tile marked for it in LDS and
// marks the neighbours of the tiles it changed for the next launch.  Stream order is the only barrier between
// sweeps; no workgroup waits on another, and every loop is bounded by a dim, a count or the tile's points.
namespace {

struct PathGrid {
    uint32_t nx, ny, nz, points;
    uint32_t tnx, tny, tnz, tiles;
    uint32_t limit; // rtq::path_limit: a candidate above it is never stored
};

__device__ __forceinline__ uint32_t path_words(const PathGrid& g) { return (g.nx + 31u) / 32u; }

// mark tile (tx + dx, ty + dy, tz + dz), if the lattice has it, in `flags`, and count it once in *active
__device__ __forceinline__ void path_mark(uint32_t* flags, uint32_t* active, const PathGrid& g, uint32_t tx, uint32_t ty,
                                          uint32_t tz, int dx, int dy, int dz)
{
    const uint32_t qx = tx + (uint32_t)dx, qy = ty + (uint32_t)dy, qz = tz + (uint32_t)dz; // below 0 wraps: >= count
    if (qx >= g.tnx || qy >= g.tny || qz >= g.tnz) return;
    uint32_t* f = flags + (qz * g.tny + qy) * g.tnx + qx;
    if (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    if (atomicExch(f, 1u) == 0u) atomicAdd(active, 1u);
}

// Word w = row * words + j of the passable words: not blocked, a point that exists, and with a clearance (d2 not
// null) a far d2.  k_pathinit and k_regionlocal form their words with it.
__device__ __forceinline__ uint32_t path_passable_word(const uint32_t* __restrict__ occ, const uint32_t* __restrict__ d2,
                                                       uint32_t nx, uint32_t row, uint32_t j, uint32_t w)
{
    uint32_t open = ~occ[w] & rtq::dist_valid_bits(nx, j);
    if (d2) {
        const uint32_t* __restrict__ r = d2 + (size_t)row * nx + 32u * j;
        const uint32_t seen = open;
        for (uint32_t b = 0; b < 32u; ++b)
            if (((seen >> b) & 1u) && r[b] != rtq::kDistFar) open &= ~(1u << b);
    }
    return open;
}

// the passable words (not blocked, a point that exists, and with a clearance a far d2), every cost far, the tile
// flags, the counters and the status cleared
__global__ void __launch_bounds__(rtq::kDistThreads) k_pathinit(const uint32_t* __restrict__ occ, const uint32_t* __restrict__ d2,
                                                               uint32_t* __restrict__ passable, uint32_t* __restrict__ cost,
                                                               uint32_t* __restrict__ flags, uint32_t* counters, uint32_t* status,
                                                               PathGrid g)
{
    const uint32_t words = path_words(g), all_words = words * g.ny * g.nz;
    const uint32_t first = blockIdx.x * rtq::kDistThreads + threadIdx.x, stride = gridDim.x * rtq::kDistThreads;
    for (uint32_t i = first; i < g.points; i += stride) cost[i] = rtq::kPathFar;
    for (uint32_t i = first; i < 2u * g.tiles; i += stride) flags[i] = 0u;
    if (first < (uint32_t)rtq::PATH_CNT_WORDS) counters[first] = 0u;
    if (first < 4u) status[first] = 0u;
    for (uint32_t w = first; w < all_words; w += stride) {
        const uint32_t row = w / words, j = w - row * words;
        passable[w] = path_passable_word(occ, d2, g.nx, row, j, w);
    }
}

// the seeds: cost 0 at the passable ones, their tile and its neighbours marked for sweep 0
__global__ void __launch_bounds__(rtq::kDistThreads) k_pathseed(const uint32_t* __restrict__ seeds, uint32_t n_seeds,
                                                               const uint32_t* __restrict__ passable, uint32_t* __restrict__ cost,
                                                               uint32_t* flags, uint32_t* counters, PathGrid g)
{
    const uint32_t words = path_words(g);
    for (uint32_t i = blockIdx.x * rtq::kDistThreads + threadIdx.x; i < n_seeds; i += gridDim.x * rtq::kDistThreads) {
        const uint32_t s = seeds[i];
        if (s >= g.points) continue;
        const uint32_t row = s / g.nx, ix = s - row * g.nx, iy = row % g.ny, iz = row / g.ny;
        if (!((passable[(size_t)row * words + (ix >> 5)] >> (ix & 31u)) & 1u)) continue;
        cost[s] = 0u;
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx)
                    path_mark(flags, counters + rtq::PATH_CNT_ACTIVE, g, ix / rtq::kPathTileX, iy / rtq::kPathTileY,
                              iz / rtq::kPathTileZ, dx, dy, dz);
    }
}

// One sweep.  A block strides over the tiles and takes those marked for this sweep: the tile's costs with a
// one-point halo into LDS, the 26 moves relaxed there (a thread a point) until no point of the tile falls, the
// points that fell stored, and the neighbouring tiles marked for the next sweep.  Only this block stores the
// tile's points; a halo cost read while its owner lowers it is still the cost of a real path, and the owner's
// mark brings this tile back in the next sweep.
__global__ void __launch_bounds__(rtq::kPathTilePoints) k_pathsweep(uint32_t* cost, const uint32_t* __restrict__ passable,
                                                                   uint32_t* flags, uint32_t* counters, uint32_t sweep, PathGrid g)
{
    __shared__ uint32_t c[rtq::kPathHaloPoints];
    const uint32_t tid = threadIdx.x;
    uint32_t* cur = flags + (sweep & 1u) * g.tiles;
    uint32_t* next = flags + ((sweep + 1u) & 1u) * g.tiles;
    uint32_t* active = counters + rtq::PATH_CNT_ACTIVE;
    if (blockIdx.x == 0 && tid == 0) {
        active[(sweep + 2u) % 3u] = 0u;
        counters[rtq::PATH_CNT_WORKED + ((sweep + 1u) & 1u)] = 0u;
    }
    if (active[sweep % 3u] == 0u) return; // nothing marked for this sweep
    const uint32_t words = path_words(g);
    const uint32_t lx = tid % rtq::kPathTileX, ly = tid / rtq::kPathTileX % rtq::kPathTileY,
                   lz = tid / (rtq::kPathTileX * rtq::kPathTileY);
    const uint32_t me = ((lz + 1u) * rtq::kPathHaloY + ly + 1u) * rtq::kPathHaloX + lx + 1u;
    for (uint32_t t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        if (cur[t] == 0u) continue; // (the same for the whole block)
        const uint32_t tx = t % g.tnx, ty = t / g.tnx % g.tny, tz = t / (g.tnx * g.tny);
        const uint32_t x0 = tx * rtq::kPathTileX, y0 = ty * rtq::kPathTileY, z0 = tz * rtq::kPathTileZ;
        for (uint32_t h = tid; h < rtq::kPathHaloPoints; h += rtq::kPathTilePoints) {
            const uint32_t hx = h % rtq::kPathHaloX, hy = h / rtq::kPathHaloX % rtq::kPathHaloY,
                           hz = h / (rtq::kPathHaloX * rtq::kPathHaloY);
            const uint32_t qx = x0 + hx - 1u, qy = y0 + hy - 1u, qz = z0 + hz - 1u; // below 0 wraps: >= dim
            uint32_t v = rtq::kPathFar;
            if (qx < g.nx && qy < g.ny && qz < g.nz) v = cost[((size_t)qz * g.ny + qy) * g.nx + qx];
            c[h] = v;
        }
        const uint32_t ix = x0 + lx, iy = y0 + ly, iz = z0 + lz;
        const bool exists = ix < g.nx && iy < g.ny && iz < g.nz;
        const size_t row = (size_t)iz * g.ny + iy;
        const bool open = exists && ((passable[row * words + tx] >> lx) & 1u);
        __syncthreads();
        if (tid == 0) {
            cur[t] = 0u;
            atomicAdd(counters + rtq::PATH_CNT_VISITS, 1u);
        }
        const uint32_t before = c[me];
        uint32_t mine = before;
        bool settled = false;
        for (uint32_t pass = 0; pass < rtq::kPathTilePoints; ++pass) {
            uint32_t best = mine;
            if (open) {
#pragma unroll
                for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) {
                            if (!dx && !dy && !dz) continue;
                            const uint32_t v = c[(int)me + (dz * (int)rtq::kPathHaloY + dy) * (int)rtq::kPathHaloX + dx];
                            const uint32_t cand = v + rtq::path_weight(dx, dy, dz);
                            if (v != rtq::kPathFar && cand < best) best = cand; // (far is never added to)
                        }
            }
            const bool lower = best < mine && best <= g.limit;
            if (!__syncthreads_or(lower)) {
                settled = true;
                break;
            }
            if (lower) c[me] = mine = best;
            __syncthreads();
        }
        const bool changed = mine != before;
        if (changed) cost[row * g.nx + ix] = mine;
        if (__syncthreads_or(changed)) {
            // the tile itself again only if the bound ended the loop before the local fixed point
            if (tid < 27u && (tid != rtq::kPathStay || !settled)) {
                int dx, dy, dz;
                rtq::path_move(tid, &dx, &dy, &dz);
                path_mark(next, active + (sweep + 1u) % 3u, g, tx, ty, tz, dx, dy, dz);
            }
            if (tid == 32u && atomicExch(counters + rtq::PATH_CNT_WORKED + (sweep & 1u), 1u) == 0u)
                atomicAdd(counters + rtq::PATH_CNT_SWEEPS, 1u);
        }
    }
}

// the flow, the reached points (a wave reduction, an atomic a wave) and the status, after `sweeps` sweeps
__global__ void __launch_bounds__(rtq::kDistThreads) k_pathfinish(const uint32_t* __restrict__ cost, uint8_t* __restrict__ flow,
                                                                 const uint32_t* counters, uint32_t* status,
                                                                 uint32_t sweeps, PathGrid g)
{
    const uint32_t dims[3] = {g.nx, g.ny, g.nz};
    uint32_t reached = 0u;
    for (uint32_t i = blockIdx.x * rtq::kDistThreads + threadIdx.x; i < g.points; i += gridDim.x * rtq::kDistThreads) {
        const uint32_t v = cost[i];
        reached += v != rtq::kPathFar;
        if (!flow) continue;
        uint32_t f = v == rtq::kPathFar ? rtq::kPathNone : rtq::kPathStay;
        if (v != rtq::kPathFar && v != 0u) {
            const uint32_t row = i / g.nx;
            f = rtq::path_flow([&](uint32_t q) { return cost[q]; }, dims, i - row * g.nx, row % g.ny, row / g.ny, v);
        }
        flow[i] = (uint8_t)f;
    }
    for (int off = 32; off > 0; off >>= 1) reached += __shfl_down(reached, off, 64);
    if ((threadIdx.x & 63u) == 0u && reached) atomicAdd(status + 2, reached);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        status[0] = counters[rtq::PATH_CNT_ACTIVE + sweeps % 3u] == 0u ? 1u : 0u;
        status[1] = counters[rtq::PATH_CNT_SWEEPS];
        status[3] = 0u;
    }
}

} // namespace

bool rt_launch_pathquery(const RtLaunch& a, const RtPathQuery& q)
{
    const uint64_t points = (uint64_t)q.dims[0] * q.dims[1] * q.dims[2];
    if (points == 0 || points > (1u << 26) || q.sweep_blocks == 0 || q.point_blocks == 0) return false;
    if (q.dims[0] > rtq::kMaxLatticeDim || q.dims[1] > rtq::kMaxLatticeDim || q.dims[2] > rtq::kMaxLatticeDim) return false;
    if (!q.passable || !q.flags || !q.counters || !q.cost || !q.status) return false;
    const rtq::PathTiles t = rtq::path_tiles(q.dims);
    const PathGrid g{q.dims[0], q.dims[1], q.dims[2], (uint32_t)points, t.n[0], t.n[1], t.n[2], t.total, q.limit};
    const dim3 pgrid(q.point_blocks), pblock(rtq::kDistThreads);
    switch (q.stage) {
    case RT_PATH_INIT: {
        if (!q.occupancy || !q.seeds || q.n_seeds == 0 || q.n_seeds > rtq::kPathMaxSeeds) return false;
        hipLaunchKernelGGL(k_pathinit, pgrid, pblock, 0, a.stream, q.occupancy, q.d2, q.passable, q.cost, q.flags, q.counters,
                           q.status, g);
        const uint32_t need = (q.n_seeds + rtq::kDistThreads - 1u) / rtq::kDistThreads;
        hipLaunchKernelGGL(k_pathseed, dim3(need < q.point_blocks ? need : q.point_blocks), pblock, 0, a.stream, q.seeds,
                           q.n_seeds, q.passable, q.cost, q.flags, q.counters, g);
        return true;
    }
    case RT_PATH_SWEEP:
        if (q.sweeps == 0 || q.sweeps > rtq::kPathMaxSweeps) return false;
        for (uint32_t k = 0; k < q.sweeps; ++k)
            hipLaunchKernelGGL(k_pathsweep, dim3(q.sweep_blocks), dim3(rtq::kPathTilePoints), 0, a.stream, q.cost, q.passable,
                               q.flags, q.counters, q.first_sweep + k, g);
        return true;
    case RT_PATH_FINISH:
        hipLaunchKernelGGL(k_pathfinish, pgrid, pblock, 0, a.stream, q.cost, q.flow, q.counters, q.status, q.first_sweep, g);
        return true;
    default:
        return false;
    }
}

// ---------------------------------------------------------------------------
// Visibility fields (rt_terrain_visibility_field): for every point the mask of the observers it has a free line of
// sight to, from the occupancy words alone (include/frosttrace.h has the definition, rt_rayquery.h the walk,
// rtq::vis_sees, and the scratch layout).  A thread a point in result order, the observers in a loop inside it: the
// observer record is the same in every lane, a wave's 64 points are consecutive ix of a row (or of the rows that
// follow), so its lanes walk near-parallel lines and mostly read the same occupancy word; the mask is put together
// in a register and stored once.  No LDS, no workgroup waits on another; every walk is bounded by the dims' sum.
namespace {

struct VisParams {
    uint32_t nx, ny, nz, points;
    uint32_t range2; // max_range squared, 0: none
    uint32_t n_observers;
};

__global__ void __launch_bounds__(rtq::kDistThreads) k_visibility(const uint32_t* __restrict__ occ, const int32_t* __restrict__ observers,
                                                                 uint32_t* __restrict__ mask, uint32_t* counters, VisParams p)
{
    const uint32_t dims[3] = {p.nx, p.ny, p.nz};
    const rtq::VisGrid g = rtq::vis_grid(dims);
    uint32_t seeing = 0u, bits = 0u;
    for (uint32_t i = blockIdx.x * rtq::kDistThreads + threadIdx.x; i < p.points; i += gridDim.x * rtq::kDistThreads) {
        const uint32_t row = i / p.nx, ix = i - row * p.nx, iz = row / p.ny, iy = row - iz * p.ny;
        uint32_t m = 0u;
        for (uint32_t k = 0; k < p.n_observers; ++k) {
            const int32_t o[4] = {observers[4u * k], observers[4u * k + 1u], observers[4u * k + 2u], observers[4u * k + 3u]};
            if (!rtq::vis_observer_valid(o, dims)) continue; // (the same in every lane) it sees nothing
            if (rtq::vis_sees([&](uint32_t bit) { return rtq::vis_bit(occ, bit); }, g, ix, iy, iz, o, p.range2)) m |= 1u << k;
        }
        mask[i] = m;
        seeing += m != 0u;
        bits += (uint32_t)__popc(m);
    }
    if (!counters) return;
    // the status: a reduction in the wave, then two atomics a wave
    for (int off = 32; off > 0; off >>= 1) {
        seeing += __shfl_down(seeing, off, 64);
        bits += __shfl_down(bits, off, 64);
    }
    if ((threadIdx.x & 63u) == 0u && bits) {
        atomicAdd(counters + 0, seeing);
        atomicAdd(counters + 1, bits);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        uint32_t valid = 0u;
        for (uint32_t k = 0; k < p.n_observers; ++k) valid += rtq::vis_observer_valid(observers + 4u * k, dims);
        counters[2] = valid;
    }
}

} // namespace

bool rt_launch_visibilityquery(const RtLaunch& a, const RtVisibilityQuery& q)
{
    const uint64_t points = (uint64_t)q.dims[0] * q.dims[1] * q.dims[2];
    if (points == 0 || points > (1u << 26) || q.blocks == 0) return false;
    if (q.dims[0] > rtq::kMaxLatticeDim || q.dims[1] > rtq::kMaxLatticeDim || q.dims[2] > rtq::kMaxLatticeDim) return false;
    if (!q.occupancy || !q.observers || !q.mask || q.n_observers == 0 || q.n_observers > rtq::kVisMaxObservers) return false;
    const VisParams p{q.dims[0], q.dims[1], q.dims[2], (uint32_t)points, q.range2, q.n_observers};
    hipLaunchKernelGGL(k_visibility, dim3(q.blocks), dim3(rtq::kDistThreads), 0, a.stream, q.occupancy, q.observers, q.mask,
                       q.counters, p);
    return true;
}

// ---------------------------------------------------------------------------
// Region fields (rt_terrain_region_field): for every point the smallest point index of its connected region of
// members, the free (passable) or the blocked points (include/frosttrace.h has the definition, rt_rayquery.h the
// forest, region_find / region_unite and the scratch layout).  A union-find with `label` as the forest, in a fixed
// number of launches: no sweeps, nothing to converge.
//
// What the kernels keep:
//  * A forest word only ever falls, and only to the index of a point of the same final region.  A stale read is
//    therefore a read of an older ancestor: it costs steps, never correctness.
//  * In k_regionmerge and k_regionflatten every access to a forest word that another workgroup may write is an
//    atomic read-modify-write (atomicMin) or a relaxed load / store at agent scope (RegionForest below, and the
//    store of k_regionflatten).  The member words and, in k_regionfinish, the labels and counts are written by an
//    earlier launch only and are read plainly.
//  * Stream order is the only barrier between the launches.  No workgroup waits for a value another must write: no
//    spin, no cooperative launch, no grid barrier.
//  * Every loop has a strictly decreasing integer as its variant (a point index, a root, the points of a tile still
//    to settle) and a hard bound derived from it, the lattice's points at most; a bound that is hit bumps
//    REGION_CNT_FAULT, which clears status[0], and leaves the loop.  Every kernel ends whatever the words hold.
//  * No kernel uses scratch memory.
namespace {

struct RegionGrid {
    uint32_t nx, ny, nz, points;
    uint32_t tnx, tny, tnz, tiles;
    uint32_t faces; // 1: connectivity 6, the face moves only
};

// the forest words on the device: rtq::region_find's and region_unite's access policy
struct RegionForest {
    uint32_t* w;
    uint32_t* faults;
    __device__ __forceinline__ uint32_t load(uint32_t i) { return __hip_atomic_load(w + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint32_t fall(uint32_t i, uint32_t v) { return atomicMin(w + i, v); }
    __device__ __forceinline__ void fault() { atomicAdd(faults, 1u); }
};

// the halo index of the tile's thread (point) l
__device__ __forceinline__ uint32_t region_halo_index(uint32_t l)
{
    const uint32_t lx = l % rtq::kPathTileX, ly = l / rtq::kPathTileX % rtq::kPathTileY, lz = l / (rtq::kPathTileX * rtq::kPathTileY);
    return ((lz + 1u) * rtq::kPathHaloY + ly + 1u) * rtq::kPathHaloX + lx + 1u;
}

// One block a tile.  The tile's 16 member words (path_passable_word, or the blocked points that exist), then the
// tile's members labelled in LDS to their local fixed point: every member takes the minimum over its linked members
// in the tile and jumps along the labels (a label is the thread index of a member of the same local component that
// is not above the point), until no label falls.  After k passes every member within k links of its component's
// minimum holds it, and a tile has 512 points, so 512 passes are enough and the bound cannot be hit.  label[p] is
// the global index of the tile-local root, kRegionNone at a non-member: a forest with label[p] <= p.  The count
// words (when something is counted) and the status are zeroed here.  The halo of the LDS tile stays kRegionNone.
__global__ void __launch_bounds__(rtq::kPathTilePoints) k_regionlocal(const uint32_t* __restrict__ occ, const uint32_t* __restrict__ d2,
                                                                     uint32_t* __restrict__ member, uint32_t* __restrict__ label,
                                                                     uint32_t* __restrict__ counts, uint32_t* counters,
                                                                     uint32_t* status, uint32_t solid, RegionGrid g)
{
    __shared__ uint32_t c[rtq::kPathHaloPoints];
    __shared__ uint32_t mw[rtq::kPathTileY * rtq::kPathTileZ];
    const uint32_t tid = threadIdx.x, words = (g.nx + 31u) / 32u;
    const uint32_t lx = tid % rtq::kPathTileX, ly = tid / rtq::kPathTileX % rtq::kPathTileY,
                   lz = tid / (rtq::kPathTileX * rtq::kPathTileY);
    const uint32_t me = region_halo_index(tid);
    if (status && blockIdx.x == 0 && tid < 4u) status[tid] = 0u;
    for (uint32_t h = tid; h < rtq::kPathHaloPoints; h += rtq::kPathTilePoints) c[h] = rtq::kRegionNone;
    for (uint32_t t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        const uint32_t tx = t % g.tnx, ty = t / g.tnx % g.tny, tz = t / (g.tnx * g.tny);
        const uint32_t x0 = tx * rtq::kPathTileX, y0 = ty * rtq::kPathTileY, z0 = tz * rtq::kPathTileZ;
        const uint32_t ix = x0 + lx, iy = y0 + ly, iz = z0 + lz;
        const bool exists = ix < g.nx && iy < g.ny && iz < g.nz;
        const uint32_t row = iz * g.ny + iy;
        __syncthreads(); // the tile before is done with c and mw
        if (lx == 0u) {
            uint32_t m = 0u;
            if (iy < g.ny && iz < g.nz) {
                const uint32_t w = row * words + tx;
                m = solid ? occ[w] & rtq::dist_valid_bits(g.nx, tx) : path_passable_word(occ, d2, g.nx, row, tx, w);
                member[w] = m;
            }
            mw[tid / rtq::kPathTileX] = m;
        }
        __syncthreads();
        const bool in = (mw[tid / rtq::kPathTileX] >> lx) & 1u; // (a member exists: the words hold no padding bit)
        uint32_t mine = in ? tid : rtq::kRegionNone;
        c[me] = mine;
        __syncthreads();
        bool settled = false;
        for (uint32_t pass = 0; pass < rtq::kPathTilePoints; ++pass) {
            uint32_t best = mine;
            if (in) {
#pragma unroll
                for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) {
                            const int k = (dx != 0) + (dy != 0) + (dz != 0);
                            if (k == 0 || (k > 1 && g.faces)) continue;
                            const uint32_t v = c[(int)me + (dz * (int)rtq::kPathHaloY + dy) * (int)rtq::kPathHaloX + dx];
                            best = min(best, v); // (kRegionNone at a non-member and in the halo)
                        }
                // jump along the labels: best strictly falls, nine halvings of 512 at most are worth taking
                for (uint32_t j = 0; j < 9u; ++j) {
                    const uint32_t v = c[region_halo_index(best)];
                    if (v >= best) break;
                    best = v;
                }
            }
            const bool lower = best < mine;
            if (!__syncthreads_or(lower)) {
                settled = true;
                break;
            }
            if (lower) c[me] = mine = best;
            __syncthreads();
        }
        if (!settled && tid == 0u) atomicAdd(counters + rtq::REGION_CNT_FAULT, 1u);
        if (exists) {
            const uint32_t i = row * g.nx + ix;
            uint32_t root = rtq::kRegionNone;
            if (in) {
                const uint32_t rx = mine % rtq::kPathTileX, ry = mine / rtq::kPathTileX % rtq::kPathTileY,
                               rz = mine / (rtq::kPathTileX * rtq::kPathTileY);
                root = ((z0 + rz) * g.ny + y0 + ry) * g.nx + x0 + rx;
            }
            label[i] = root;
            if (counts) counts[i] = 0u;
        }
    }
}

// A thread a point.  Each member takes each of its backward links (rtq::region_backward_move: 13 of the 26 moves, 3
// of the 6) that leave its tile and unites the two trees (rtq::region_unite).  The links inside a tile are
// k_regionlocal's, and every link between two tiles is backward from one of its ends, so after this launch two
// members are in one tree iff they are in one region.  Of a run of parallel links along a row only the first is
// united (below): in open space that leaves a link a row and move, not a link a point and move.
__global__ void __launch_bounds__(rtq::kDistThreads) k_regionmerge(const uint32_t* __restrict__ member, uint32_t* label,
                                                                  uint32_t* counters, RegionGrid g)
{
    const uint32_t words = (g.nx + 31u) / 32u, moves = rtq::region_backward_count(g.faces ? 6u : 26u);
    RegionForest f{label, counters + rtq::REGION_CNT_FAULT};
    for (uint32_t i = blockIdx.x * rtq::kDistThreads + threadIdx.x; i < g.points; i += gridDim.x * rtq::kDistThreads) {
        const uint32_t row = i / g.nx, ix = i - row * g.nx, iz = row / g.ny, iy = row - iz * g.ny;
        const uint32_t mine = member[row * words + (ix >> 5)], lx = ix & 31u;
        if (!((mine >> lx) & 1u)) continue;
        const bool run = lx && ((mine >> (lx - 1u)) & 1u); // the point before in the row is a member of this tile
        for (uint32_t k = 0; k < moves; ++k) {
            int dx, dy, dz;
            rtq::region_backward_move(g.faces ? 6u : 26u, k, &dx, &dy, &dz);
            const uint32_t qx = ix + (uint32_t)dx, qy = iy + (uint32_t)dy, qz = iz + (uint32_t)dz; // below 0 wraps: >= dim
            if (qx >= g.nx || qy >= g.ny || qz >= g.nz) continue;
            if (qx / rtq::kPathTileX == ix / rtq::kPathTileX && qy / rtq::kPathTileY == iy / rtq::kPathTileY &&
                qz / rtq::kPathTileZ == iz / rtq::kPathTileZ)
                continue; // inside the tile: k_regionlocal's
            const uint32_t qrow = qz * g.ny + qy;
            const uint32_t theirs = member[qrow * words + (qx >> 5)], qlx = qx & 31u;
            if (!((theirs >> qlx) & 1u)) continue;
            // The same link one point back along the row, from p - 1 to q - 1, joins the same two trees when both are
            // members of the same two tiles: p - 1 and p are face neighbours in one tile, q - 1 and q in the other, and
            // k_regionlocal has put each pair into one tree.  So only the first link of such a run is united.
            if (run && qlx && ((theirs >> (qlx - 1u)) & 1u)) continue;
            rtq::region_unite(f, i, qrow * g.nx + qx, g.points);
        }
    }
}

// One block a tile, a thread a point: label[p] = find(p), the root, which is the region's smallest index because a
// parent is never above its child.  No tree changes its root in this launch; a word falls to its root and is read
// by other finds on the way, old or new.  Then the counts (counts not null): the members of a wave that share the
// first lane's root add once to the tile's table in LDS (keyed by root, open addressing over 512 slots for 512
// points at most, so a free or equal slot is found within 512 probes), the others each for themselves, and the
// tile issues one global atomic per root it holds.  The largest region usually holds nearly every member: a global
// atomic a point would serialise on one word.
__global__ void __launch_bounds__(rtq::kPathTilePoints) k_regionflatten(const uint32_t* __restrict__ member, uint32_t* label,
                                                                       uint32_t* counts, uint32_t* counters, RegionGrid g)
{
    __shared__ uint32_t key[rtq::kPathTilePoints], val[rtq::kPathTilePoints];
    const uint32_t tid = threadIdx.x, words = (g.nx + 31u) / 32u;
    const uint32_t lx = tid % rtq::kPathTileX, ly = tid / rtq::kPathTileX % rtq::kPathTileY,
                   lz = tid / (rtq::kPathTileX * rtq::kPathTileY);
    RegionForest f{label, counters + rtq::REGION_CNT_FAULT};
    for (uint32_t t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        const uint32_t tx = t % g.tnx, ty = t / g.tnx % g.tny, tz = t / (g.tnx * g.tny);
        const uint32_t ix = tx * rtq::kPathTileX + lx, iy = ty * rtq::kPathTileY + ly, iz = tz * rtq::kPathTileZ + lz;
        const uint32_t row = iz * g.ny + iy;
        const bool in = iy < g.ny && iz < g.nz && ((member[row * words + tx] >> lx) & 1u);
        uint32_t root = rtq::kRegionNone;
        if (in) {
            const uint32_t i = row * g.nx + ix;
            root = rtq::region_find(f, i, g.points);
            if (root != i) __hip_atomic_store(label + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (!counts) continue;
        __syncthreads(); // the tile before is done with the table
        key[tid] = rtq::kRegionNone;
        val[tid] = 0u;
        __syncthreads();
        const uint32_t first = __shfl(root, __builtin_ctzll(__ballot(in) | (1ull << 63)), 64);
        const uint64_t same = __ballot(in && root == first);
        const bool leader = in && root == first && (uint32_t)__builtin_ctzll(same) == (tid & 63u);
        if (in && (leader || root != first)) {
            const uint32_t add = leader ? (uint32_t)__popcll(same) : 1u;
            uint32_t slot = root % rtq::kPathTilePoints;
            bool placed = false;
            for (uint32_t probe = 0; probe < rtq::kPathTilePoints; ++probe) {
                const uint32_t old = atomicCAS(&key[slot], rtq::kRegionNone, root);
                if (old == rtq::kRegionNone || old == root) {
                    atomicAdd(&val[slot], add);
                    placed = true;
                    break;
                }
                slot = (slot + 1u) % rtq::kPathTilePoints;
            }
            if (!placed) f.fault();
        }
        __syncthreads();
        if (key[tid] != rtq::kRegionNone) atomicAdd(counts + key[tid], val[tid]);
    }
}

// A thread a point: size[p] = the count at p's root (0 at a non-member), and the status: the roots, the members
// and the largest count by a reduction in the wave and then in the block, and an atomic a block and word where the
// block has something to add (every block adds to the same three words); status[0] from the fault counter.
// label and counts are final when this launch starts.
__global__ void __launch_bounds__(rtq::kDistThreads) k_regionfinish(const uint32_t* __restrict__ label, const uint32_t* __restrict__ counts,
                                                                   uint32_t* __restrict__ size, const uint32_t* counters,
                                                                   uint32_t* status, RegionGrid g)
{
    uint32_t regions = 0u, members = 0u, largest = 0u;
    for (uint32_t i = blockIdx.x * rtq::kDistThreads + threadIdx.x; i < g.points; i += gridDim.x * rtq::kDistThreads) {
        const uint32_t l = label[i];
        const uint32_t n = l < g.points ? counts[l] : 0u; // (kRegionNone is no point)
        if (size) size[i] = n;
        members += l != rtq::kRegionNone;
        if (l == i) {
            ++regions;
            largest = max(largest, n);
        }
    }
    if (!status) return; // (the same in every thread)
    __shared__ uint32_t part[3][rtq::kDistThreads / 64u];
    for (int off = 32; off > 0; off >>= 1) {
        regions += __shfl_down(regions, off, 64);
        members += __shfl_down(members, off, 64);
        largest = max(largest, (uint32_t)__shfl_down(largest, off, 64));
    }
    if ((threadIdx.x & 63u) == 0u) {
        part[0][threadIdx.x / 64u] = regions;
        part[1][threadIdx.x / 64u] = members;
        part[2][threadIdx.x / 64u] = largest;
    }
    __syncthreads();
    if (threadIdx.x != 0u) return;
    // the words are shared by every block: an atomic only where this block has something to add
    regions = members = largest = 0u;
    for (uint32_t w = 0; w < rtq::kDistThreads / 64u; ++w) {
        regions += part[0][w];
        members += part[1][w];
        largest = max(largest, part[2][w]);
    }
    if (regions) atomicAdd(status + 1, regions);
    if (members) atomicAdd(status + 2, members);
    if (largest) atomicMax(status + 3, largest);
    if (blockIdx.x == 0) status[0] = counters[rtq::REGION_CNT_FAULT] == 0u ? 1u : 0u;
}

} // namespace

bool rt_launch_regionquery(const RtLaunch& a, const RtRegionQuery& q)
{
    const uint64_t points = (uint64_t)q.dims[0] * q.dims[1] * q.dims[2];
    if (points == 0 || points > (1u << 26) || q.tile_blocks == 0 || q.point_blocks == 0) return false;
    if (q.dims[0] > rtq::kMaxLatticeDim || q.dims[1] > rtq::kMaxLatticeDim || q.dims[2] > rtq::kMaxLatticeDim) return false;
    if (!q.occupancy || !q.member || !q.counters || !q.label) return false;
    if ((q.solid && q.d2) || (!q.counts && (q.size || q.status)) || (q.counts && !q.size && !q.status)) return false;
    const rtq::PathTiles t = rtq::path_tiles(q.dims);
    const RegionGrid g{q.dims[0], q.dims[1], q.dims[2], (uint32_t)points, t.n[0], t.n[1], t.n[2], t.total, q.faces ? 1u : 0u};
    const dim3 tgrid(q.tile_blocks), tblock(rtq::kPathTilePoints), pgrid(q.point_blocks), pblock(rtq::kDistThreads);
    hipLaunchKernelGGL(k_regionlocal, tgrid, tblock, 0, a.stream, q.occupancy, q.d2, q.member, q.label, q.counts, q.counters,
                       q.status, q.solid ? 1u : 0u, g);
    hipLaunchKernelGGL(k_regionmerge, pgrid, pblock, 0, a.stream, q.member, q.label, q.counters, g);
    hipLaunchKernelGGL(k_regionflatten, tgrid, tblock, 0, a.stream, q.member, q.label, q.counts, q.counters, g);
    if (q.counts)
        hipLaunchKernelGGL(k_regionfinish, pgrid, pblock, 0, a.stream, q.label, q.counts, q.size, q.counters, q.status, g);
    return true;
}

// ---------------------------------------------------------------------------
// Diagnostics: device evaluation of the numeric primitives, noise3d and
// getDensity for the primitive-level parity tests (tests/test_gpu_parity.py).
namespace {

__global__ void k_debug_math(int op, const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y,
                             int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (op == 12) {
        // octave-count sweep: d2 = the float with bits bits(a[0]) + i; counts (in y[0..2] as
        // uint32) unflagged estimates that differ from np_octaves_exact, flagged lanes, and
        // how many of the swept d2 exist
        const float d2 = rtm::fbits(rtm::bits(a[0]) + (uint32_t)i);
        bool near;
        const int est = rts::np_octaves_estimate(d2, &near);
        uint32_t* cnt = reinterpret_cast<uint32_t*>(y);
        if (!near && est != rts::np_octaves_exact(d2)) atomicAdd(&cnt[0], 1u);
        const uint64_t bn = __ballot(near), ba = __ballot(true);
        if (__lane_id() == 0) {
            if (bn) atomicAdd(&cnt[1], (uint32_t)__popcll(bn));
            atomicAdd(&cnt[2], (uint32_t)__popcll(ba));
        }
        return;
    }
    if (op == 14) { // k_trace's sky exit for the triple (p.y, dir.y, dist) at a[3 i]: 1 or 0
        y[i] = rts::sky_exit(a[3 * i], a[3 * i + 1], a[3 * i + 2]) ? 1.0f : 0.0f;
        return;
    }
    if (op == 15) { // the AO direction about the normal a[3 i] for the key (px, py, a, k): the bits of b[4 i ..]
        const f3 d = rts::ao_dir(rtm::mk(a[3 * i], a[3 * i + 1], a[3 * i + 2]), rtm::bits(b[4 * i]), rtm::bits(b[4 * i + 1]),
                                 rtm::bits(b[4 * i + 2]), rtm::bits(b[4 * i + 3]));
        y[3 * i] = d.x;
        y[3 * i + 1] = d.y;
        y[3 * i + 2] = d.z;
        return;
    }
    // op 16, the sweep: a = 4 uint32 words (start pattern, odd multiplier, element op, mask), x = the float with
    // bits (start + i * multiplier) & mask, evaluated with the element op and b[0]; no input array
    const bool sweep = op == 16;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(a);
    const int j = sweep ? 0 : i;
    float x = sweep ? rtm::fbits((w[0] + (uint32_t)i * w[1]) & w[3]) : a[i], v = 0.0f;
    if (sweep) op = (int)w[2];
    switch (op) {
    case 0: v = rtm::exp2(x); break;
    case 1: v = rtm::log2(x); break;
    case 2: v = rtm::exp(x); break;
    case 3: v = rtm::sin(x); break;
    case 4: v = rtm::cos(x); break;
    case 5: v = rtm::sqrt(x); break;
    case 6: v = rtm::rcp(x); break;
    case 7: v = rtm::rcp(rtm::sqrt(x)); break;
    case 8: v = rtm::pow(x, b[j]); break;
    case 9: v = rtm::max(x, b[j]); break;
    case 10: v = rtm::min(x, b[j]); break;
    case 11: v = rtm::pow_nonneg(x, b[j]); break;
    case 13: v = rtm::pow_nonneg_wave(x, b[j]); break; // (a wave = 64 consecutive elements)
    case 17: v = rtm::log2_nonneg(x); break;
    default: v = 0.0f; break;
    }
    y[i] = v;
}

template <int L>
__global__ void __launch_bounds__(256) k_debug_noise(const RtConsts* __restrict__ k, const uint32_t* __restrict__ perm2d,
                                                     const float4* __restrict__ grad, const float* __restrict__ xyz,
                                                     float* __restrict__ out, int n, int density)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[kNoiseLdsWords];
    load_noise_lds(lds, perm2d, grad, k);
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ctx c = make_ctx(k, lds);
    f3 p = rtm::mk(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    // density 2: noise3d_z0(x, y) (z ignored); 3: its FAST variant (|x|, |y| < kFastCellRange)
    if (density == 2) {
        out[i] = noise3d_z0(c.nz, p.x, p.y);
    } else if (density == 3) {
        out[i] = noise3d_z0<true>(c.nz, p.x, p.y);
    } else {
        out[i] = density ? get_density<L>(c, p) : noise3d(c.nz, p.x, p.y, p.z);
    }
}

// sky.hlsl:26-36,83-137 for one view direction per thread: (mie, rayleigh, space)
__global__ void __launch_bounds__(256) k_debug_sky(const RtConsts* __restrict__ k, const uint32_t* __restrict__ perm2d,
                                                   const float4* __restrict__ grad, const float* __restrict__ dirs,
                                                   float* __restrict__ out, int n)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[kNoiseLdsWords];
    load_noise_lds(lds, perm2d, grad, k);
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ctx c = make_ctx(k, lds);
    const f3 d = rtm::mk(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
    const SkyColor sc = get_rayleigh_mie(c, d);
    const float space = get_space_color(c, d);
    float* o = out + 7 * i;
    o[0] = sc.mie.x;
    o[1] = sc.mie.y;
    o[2] = sc.mie.z;
    o[3] = sc.rayleigh.x;
    o[4] = sc.rayleigh.y;
    o[5] = sc.rayleigh.z;
    o[6] = space;
}

// scripts/batch_shard_sim.py's coupled transport model (diagnostics): one wave that stores the 100 MHz
// clock when it starts (stamp, if set), waits until base[0] + until_ticks (base set: a stamp of an earlier
// launch; a peer's side of a transfer becoming ready), then spins `ticks` more (the transfer), holding a CU
// like a collective's kernel.  Vector stores only.
__global__ void __launch_bounds__(64) k_debug_spin(const unsigned long long* base, unsigned long long until_ticks,
                                                  unsigned long long ticks, unsigned long long* stamp)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    if (stamp && threadIdx.x == 0) *stamp = t0;
    const unsigned long long ready = base ? base[0] + until_ticks : t0;
    const unsigned long long end = (ready > t0 ? ready : t0) + ticks;
    while (__builtin_amdgcn_s_memrealtime() < end) __builtin_amdgcn_s_sleep(16);
}

} // namespace

void rt_launch_debug_spin(hipStream_t s, const unsigned long long* base, unsigned long long until_ticks,
                          unsigned long long ticks, unsigned long long* stamp)
{
    hipLaunchKernelGGL(k_debug_spin, dim3(1), dim3(64), 0, s, base, until_ticks, ticks, stamp);
}

void rt_launch_debug_sky(const RtLaunch& a, const float* dirs, float* out, int n)
{
    hipLaunchKernelGGL(k_debug_sky, dim3((n + 255) / 256), dim3(256), 0, a.stream, a.consts, a.perm2d, a.grad, dirs, out, n);
}

void rt_launch_debug_math(hipStream_t s, int op, const float* a, const float* b, float* y, int n)
{
    hipLaunchKernelGGL(k_debug_math, dim3((n + 255) / 256), dim3(256), 0, s, op, a, b, y, n);
}

void rt_launch_debug_noise(const RtLaunch& a, const float* xyz, float* out, int n, int density)
{
    dim3 g((n + 255) / 256), b(256);
    switch (a.landscape) {
    case RT_TESTING: hipLaunchKernelGGL(k_debug_noise<RT_TESTING>, g, b, 0, a.stream, a.consts, a.perm2d, a.grad, xyz, out, n, density); break;
    case RT_SIMPLE: hipLaunchKernelGGL(k_debug_noise<RT_SIMPLE>, g, b, 0, a.stream, a.consts, a.perm2d, a.grad, xyz, out, n, density); break;
    case RT_GREENROCKS: hipLaunchKernelGGL(k_debug_noise<RT_GREENROCKS>, g, b, 0, a.stream, a.consts, a.perm2d, a.grad, xyz, out, n, density); break;
    default: hipLaunchKernelGGL(k_debug_noise<RT_NOMADPLAINS>, g, b, 0, a.stream, a.consts, a.perm2d, a.grad, xyz, out, n, density); break;
    }
}

#ifdef RT_LIVE_HIST
// diagnostic build: copies (and with reset != 0 clears) the live-lanes-per-primary-step histogram
extern "C" int rt_debug_live_hist(unsigned long long* out, int reset)
{
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_live_hist), 65 * 8) != hipSuccess) return -1;
    if (reset) {
        static const unsigned long long zero[65] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_live_hist), zero, 65 * 8) != hipSuccess) return -1;
    }
    return 65;
}
#endif

#ifdef RT_QUERY_UTIL
// diagnostic build: copies (and with reset != 0 clears) the query lane kernels' g_query_util, summed over the
// launches since the last reset
extern "C" int rt_debug_query_util(unsigned long long* out, int reset)
{
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_query_util), 32) != hipSuccess) return -1;
    if (reset) {
        static const unsigned long long zero[4] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_query_util), zero, 32) != hipSuccess) return -1;
    }
    return 4;
}
#endif

#ifdef RT_WAVE_TRACE
// copies the last k_trace launch's per-wave timeline (RT_WT_FIELDS u64 per wave slot)
extern "C" int rt_debug_wave_trace(unsigned long long* out, int max_waves)
{
    const int n = max_waves < RT_WT_MAX_WAVES ? max_waves : RT_WT_MAX_WAVES;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_trace), (size_t)n * RT_WT_FIELDS * 8) != hipSuccess) return -1;
    return RT_WT_FIELDS;
}
#endif
