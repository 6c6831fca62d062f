// rt_kernels.h -- host-side launch interface of the HIP kernels.
#pragma once

#include <hip/hip_runtime.h>

#include "rt_types.h"

// work counters (one 128-byte block, zeroed by k_order before every k_trace: the unit queue, then one
// first-unit counter per wave slot of a k_trace block), then the device's sticky flags (zeroed at
// device creation and by rt_device_check only): a k_trace queue push that would exceed its bound
// raises a flag instead of storing (rt_spill_caps)
// RT_CTR_GATE / RT_CTR_SCAN: the gated launch's prepass task counter and its tile scan's start (GatedPrepass)
enum { RT_CTR_PRIMARY = 0, RT_CTR_FIRST = 1, RT_CTR_GATE = 24, RT_CTR_SCAN = 25 };
#define RT_CTR_BYTES 128
#define RT_QUEUE_BYTES 192
enum { RT_FLAG_HIT_OVERFLOW = 1u, RT_FLAG_SPILL_OVERFLOW = 2u, RT_FLAG_PREPASS_TIMEOUT = 4u };

// A frame batch: up to RT_MAX_BATCH frames of one resolution, landscape and shard traced by
// one sequence of launches (rt_terrain_render_batch).  Each frame keeps its own constant
// block (camera, sun), CameraResults, CellDistance and framebuffer; the kernels find them
// through this table in device memory.  A single frame is a batch of one.
#define RT_MAX_BATCH 24
struct FrameTable {
    const RtConsts* k[RT_MAX_BATCH];    // tracescreen's constant block
    const RtConsts* kcam[RT_MAX_BATCH]; // camerarays' constant block (its own cbuffers)
    float4* cam[RT_MAX_BATCH];   // CameraResults, float4[1024]
    float2* cells[RT_MAX_BATCH]; // CellDistance, float2[1024]
    uint32_t* out8[RT_MAX_BATCH];
    float4* out32[RT_MAX_BATCH]; // may be null
};

// The NEXT batch's camerarays prepass fused into this batch's k_trace (nomadplains):
// `tasks` tasks of 8 rays (RT_PREPASS_LPR lanes per ray) of the frames of `ft` (their camerarays constant
// blocks kcam, their CameraResults cam), taken from ctl[0]; a finished wave stores its rays' CameraResults
// (sc1; one whole 128-B line per 8-ray wave) and adds its rays to ctl[1]; that batch's k_order waits for ctl[1] to reach
// its rays (frames x 1024) before it reads them.  tasks == 0: none.
#define RT_FUSE_RAYS_PER_TASK 8
#define RT_FUSE_TASKS_PER_FRAME (RT_CAMERA_RES * RT_CAMERA_RES / RT_FUSE_RAYS_PER_TASK)
struct FusedPrepass {
    const FrameTable* ft;
    uint32_t* ctl;
    uint32_t tasks;
};

// The batch's OWN camerarays prepass inside its k_trace (the gated launch, nomadplains; DESIGN.md
// section 7): `tasks` = frames x RT_FUSE_TASKS_PER_FRAME tasks of 8 rays, taken first by the waves
// (top priority), each storing its 8 CameraResults as one whole 128-B line (sc1) and then, per frame
// (RT_GATE_WORDS words at gate + f * RT_GATE_WORDS, zeroed by k_order), setting its bit in the frame's
// task mask (words 0-3; task = ray row * 4 + ray column / 8) and adding 8 to the frame's ray counter
// (word RT_GATE_CTR; the task that completes the frame derives the frame's CellDistance and flags it in
// word RT_GATE_CTR + 1).  Units are claimed by tile (claims[i]: units of order entry i taken) in k_order's
// longest-first order from the tiles whose cells' prepass rays (the 5x5 neighbourhoods setTargetDepths
// reads) are in, so units start while the prepass's long rays still march.  tasks == 0: off (the prepass
// ran before; cells from k_order).
#define RT_GATE_WORDS 256 // per frame: the task mask (words 0-3), the ray counter and the cells flag on a line of
#define RT_GATE_CTR 32    // their own, the per-task wave counters (words 128-255)
#define RT_GATE_TASKS 128
// lanes per prepass ray in k_trace's prepass tasks (a task's 8 rays are marched by 8 / (64 / LPR) waves):
// 8 = one wave per task, 3 rounds of the 18 octave values per step.  32 (one round, 4 waves per task) was
// measured slower inside k_trace: the rays' latency there is set by the units sharing their SIMDs
// (profiles/r05/gated_ab.md)
#ifndef RT_PREPASS_LPR
#define RT_PREPASS_LPR 8
#endif
struct GatedPrepass {
    uint32_t* gate;   // RT_MAX_BATCH x RT_GATE_WORDS
    uint32_t* claims; // per order entry (tile of the batch): its units claimed so far
    uint32_t tasks;
    // RT_DEVICE_DEBUG_GATE_STRESS (diagnostic): 1 = every wave first reads its frames' previous CellDistance with
    // plain loads (the CU's L1 then holds lines the frame's last task rewrites), 2 = that task waits ~200 us
    // before it stores CellDistance (more units start from CameraResults, the rest read the flagged cells late)
    uint32_t debug;
};

struct RtLaunch {
    hipStream_t stream;
    int landscape;
    const RtConsts* consts;   // device copy of the constant block
    const uint32_t* perm2d;   // device texPerm2D (128*128 texels)
    const float4* grad;       // device CBNoise.permGradients (128 float4)
    RtStats* stats;           // nullptr = uninstrumented kernels
    uint32_t* queue;          // RT_CTR_BYTES of device work counters
    int num_cus;              // compute units (persistent grid size)
    // per-sample buffers, rt_split_samples() entries per frame (sample t, see rt_kernels.hip)
    float4* samples;          // saturated colour of hit samples (written by S, read by R)
    // k_trace's per-block queues in HBM, consumed by the same block; capacities per block
    // (rt_spill_caps: the bound on a block's queued work)
    float4* hitq;             // hit queue: primary hit records (1 float4, 3 with fog), hit_cap per block
    float4* spill_long;       // long-ray records (3 float4) the LDS ring cannot hold, long_spill_cap per block
    uint32_t hit_cap, long_spill_cap;
    int cells_from_cam;       // k_order derives CellDistance from CameraResults (setTargetDepths) first
    int small_rings;          // diagnostic (RT_DEVICE_DEBUG_SMALL_RINGS): k_trace's LDS long ring holds 64 entries, its fin pool 8
    int fit;                  // hit pixels finish in k_trace (aa 1, <= 1 AO ray, no float output; UnitMap::fit)
    float4* fin;              // 3 float4 per sample: shading inputs a long shadow ray needs to finish
    float4* finpool;          // the same per block in a pool of RT_FIN_SLOTS slots of 3 float4 (fin is the fallback)
    float4* cpool;            // per block RT_AO_POOL_SLOTS colours: a multi-AO hit's colour for its last AO ray (fitm)
    int fitm;                 // hit pixels without a long shadow finish in k_trace with >= 2 AO rays (UnitMap::fitm)
    uint32_t* aocc;           // per sample: occluded AO rays (AO extension), a byte each, 4 per word
    int ao_samples;           // AO rays per primary hit (0 = off)
    int aa;                   // AA samples per pixel
    uint32_t* order;          // k_order's tile order (rt_split_samples/1024 entries per frame)
    uint64_t* hitmask;        // per 8x8 unit and AA sample: the primary hits' ballot (k_trace -> k_finish)
    const FrameTable* frames; // device table of the batch's frames
    FrameTable frames_host;   // the same pointers on the host
    uint32_t n_frames;        // frames in the batch (1..RT_MAX_BATCH)
    hipEvent_t after_order;   // recorded after k_order when set (its read of CameraResults is done)
    FusedPrepass fuse_next;   // the next batch's prepass, run inside this k_trace (tasks 0: none); k_order zeroes its ctl
    const uint32_t* wait_ctl; // this batch's prepass ran inside the previous k_trace: k_order waits for wait_ctl[1]
    uint32_t wait_total;      //   to reach this many rays
    hipEvent_t after_order_fuse; // recorded after k_order when set: fuse_next's counters are zeroed (its batch's
                                 // own k_order, on another stream, polls them only after this event)
    uint32_t* host_flag;      // host-mapped word of the GPU: k_order stores RT_FLAG_PREPASS_TIMEOUT there when its
                              // wait for a fused prepass times out (every later C-ABI call on the GPU fails)
    GatedPrepass gated;       // this batch's prepass inside its own k_trace (tasks 0: off)
    int packed;               // frames.out8[f] are packed shard buffers (UnitMap::packed; no float output)
};

void rt_launch_camerarays(const RtLaunch& a, float4* camera_results);
// the prepass of every frame of a.frames (-> CameraResults); with a.cells_from_cam the
// tracescreen launch derives CellDistance from them first (setTargetDepths, in k_order)
void rt_launch_camerarays_batch(const RtLaunch& a);
// Trace the region [off, off+ext) in 32x32-pixel tiles of every frame of a.frames (cells and
// outputs from the table), tile-cyclic sharding: a single frame traces the tiles t (row-major
// over the region) with t % tile_stride == tile_first; in a batch of n > 1 frames with
// tile_stride > 1, frame f traces shard (tile_first + f) % tile_stride (per-frame rotation).
void rt_launch_tracescreen(const RtLaunch& a, uint32_t off_x, uint32_t off_y, uint32_t ext_x, uint32_t ext_y,
                           uint32_t tile_first, uint32_t tile_stride);

// The march of a surface or shaded query's rays: t_min, t_max, stepmod and max_steps (0: unbounded) hold for every
// ray; with ray_range the rays' spare words are t_min_i and t_max_i instead.
struct RtMarchParams {
    float t_min, t_max, stepmod;
    int max_steps;
    bool ray_range;
};

// A ray or surface query: n rays packed as ox oy oz _ dx dy dz _ (two float4 each), marched with the launch's
// landscape, noise tables and constants and `eye` in place of Eye; steps[n], if set, takes the march loops'
// iteration counts.
//   A ray query (rt_terrain_trace_rays; `surface` false, `march` unused): camerarays.hlsl:12-21 -> results[n].
//   A surface query (rt_terrain_trace_surface; `surface` true): the refined march tracescreen runs for its pixels
//   (traceRay with skiprefine off, tracing.hlsl:47-105) with `march`, and getNormal (:107-116) -> results[2n]
//   (pd.xyz, pd.w | normal, density; the normal 0 where density <= 0).
// lpr > 1: one lpr-lane segment per ray in blocks of bs threads (nomadplains; the prepass's pairs: rt_rayquery.h
// Plan).  lpr == 1: the persistent lane kernel, `blocks` blocks of 1024 threads claiming rays from *counter,
// which the caller zeroes on the stream before every launch.  false: no such kernel (nothing launched).
struct RtTraceQuery {
    const float4* rays;
    float4* results;
    uint32_t* steps; // may be null
    uint32_t n;
    float eye[3];
    int bs, lpr;
    uint32_t blocks;
    uint32_t* counter;
    bool surface;
    RtMarchParams march;
};
bool rt_launch_tracequery(const RtLaunch& a, const RtTraceQuery& q);

// A shaded query (rt_terrain_shade_rays): the sample tracescreen.hlsl:16-48 computes (one sample, no AO) for the
// same packed rays -> results[2n] (colour, pd.w | pd.xyz, density), rgba8[n] and steps[2n] (primary, shadow
// iterations), each if set; results or rgba8 must be.  The constants (a.consts) carry the query's eye, for the
// sky.  Parameters as a surface query's; the lanes shape only (bs 1024), so the counter is required.
struct RtShadeQuery {
    const float4* rays;
    float4* results; // may be null
    uint32_t* rgba8; // may be null
    uint32_t* steps; // may be null
    uint32_t n;
    float eye[3];
    uint32_t blocks;
    uint32_t* counter;
    RtMarchParams march;
};
bool rt_launch_shadequery(const RtLaunch& a, const RtShadeQuery& q);

// A point shading query (rt_terrain_shade_points): getColor with its shadow ray and the AO factor of ao_samples
// (0..16) hemisphere rays hashed from (point index, seed) at n points x y z _ with normals nx ny nz _ (one float4
// each) -> results[n] (colour, ao), rgba8[n] (ao times the saturated colour) and steps[2n] (shadow iterations, the
// AO rays' sum), each if set; results or rgba8 must be.  `eye` is in place of Eye and the viewpoint of the
// colour; the constants are the compute's as they are.  The lanes shape only (bs 1024), so the counter is
// required.  false: nothing launched.
struct RtPointQuery {
    const float4* points;
    const float4* normals;
    float4* results; // may be null
    uint32_t* rgba8; // may be null
    uint32_t* steps; // may be null
    uint32_t n;
    float eye[3];
    uint32_t ao_samples, seed;
    uint32_t blocks;
    uint32_t* counter;
};
bool rt_launch_shadepoints(const RtLaunch& a, const RtPointQuery& q);

// A field query (rt_terrain_sample_field / rt_terrain_sample_lattice): getDensity, with `normal` also getNormal
// (tracing.hlsl:107-116, for every point), with the launch's landscape, noise tables and constants and `eye` in
// place of Eye.  points set: n points x y z _ (one float4 each) -> results[n], float or with `normal` float4
// {n.xyz, d}.  points null: the lattice of dims points at fmaf(i, spacing, origin), n their product, result index
// (iz * ny + iy) * nx + ix -> results (may be null) and occupancy (may be null; d > 0, one bit a point,
// ceil(nx / 32) words a row), in strips of 64 ix by `rows` iy; `column`: nomadplains' steep noise once per strip
// column.  `blocks` blocks of 1024 threads stride over the work.  false: no such kernel (nothing launched).
struct RtFieldQuery {
    const float4* points;
    void* results;
    uint32_t* occupancy;
    uint32_t n;
    float eye[3];
    bool normal;
    uint32_t blocks;
    float origin[3], spacing[3];
    uint32_t dims[3];
    uint32_t rows;
    bool column;
};
bool rt_launch_fieldquery(const RtLaunch& a, const RtFieldQuery& q);

// A mesh extraction's passes after the density pass (rt_terrain_extract_mesh; the definition is in
// include/frosttrace.h, the scratch layout rtq::MeshScratch): the lattice's densities and occupancy words are in
// `density` and `occupancy` (a lattice RtFieldQuery wrote them on the same stream).  k_meshcount fills `masks`
// (4 uint64 a mask word) and the words' vertex and quad counts in `offsets` (2 uint32 a word), k_meshscan turns
// those into the counts preceding each word and writes counts[0..1] (vertices, triangles), k_meshemit stores the
// first max_vertices vertices (x y z, cell index bits) and the first max_triangles triangles (3 uint32), and with
// `normals` k_meshnormals stores {getNormal, getDensity} of the first min(counts[0], max_vertices) vertices, with
// the launch's landscape, tables and constants and `eye` in place of Eye.  All dims >= 2; vertices / triangles
// may be null with a capacity of 0.  count_blocks and emit_blocks are blocks of rtq::kMeshThreads threads,
// normal_blocks of 1024.  false: nothing launched.
struct RtMeshQuery {
    const float* density;
    const uint32_t* occupancy;
    uint64_t* masks;
    uint32_t* offsets;
    uint32_t row_words, words; // mask words per cell row and in all
    float origin[3], spacing[3];
    uint32_t dims[3];
    float4* vertices;
    float4* normals; // may be null: no normal pass
    uint32_t max_vertices;
    uint32_t* triangles;
    uint32_t max_triangles;
    uint32_t* counts;
    float eye[3];
    uint32_t count_blocks, emit_blocks, normal_blocks;
};
bool rt_launch_meshquery(const RtLaunch& a, const RtMeshQuery& q);

// A distance field's three passes (rt_terrain_distance_field; the definition is in include/frosttrace.h, the
// scratch layout and the row arithmetic in rt_rayquery.h): `occupancy` holds the lattice's words in
// rt_terrain_sample_lattice's layout, the padding bits anything (the caller's, or a lattice RtFieldQuery's on the
// same stream).  k_distrows fills `rows` (a word a point), k_distcolumns the two planes of `planes` (points uint32
// each: inside set, outside set), k_distfinish stores d2 and / or distance (either may be null, not both).
// reach / limit2: rtq::distance_bound; abs_spacing: |spacing[0]|, read with `distance` only.  All dims >= 1 with
// a product of 2^26 at most; blocks of rtq::kDistThreads threads.  false: nothing launched.
struct RtDistanceQuery {
    const uint32_t* occupancy;
    uint32_t* rows;
    uint32_t* planes;
    uint32_t dims[3];
    uint32_t reach, limit2;
    float abs_spacing;
    uint32_t* d2;
    float* distance;
    uint32_t blocks;
};
bool rt_launch_distancequery(const RtLaunch& a, const RtDistanceQuery& q);

// A path field's passes (rt_terrain_path_field; the definition is in include/frosttrace.h, the schedule, the tiles
// and the scratch layout in rt_rayquery.h).  `stage` chooses what one call enqueues on a.stream:
//   RT_PATH_INIT:   k_pathinit (passable words from `occupancy` and, if not null, `d2`; cost far; flags, counters and
//                   status cleared) and k_pathseed (`seeds`, n_seeds of them);
//   RT_PATH_SWEEP:  `sweeps` launches of k_pathsweep, numbered first_sweep, first_sweep + 1, ...;
//   RT_PATH_FINISH: k_pathfinish after first_sweep sweeps in all: `flow` (may be null), the reached count, status.
// flags: two arrays of `tiles` words; counters: rtq::PATH_CNT_WORDS words.  All dims >= 1 with a product of 2^26 at
// most.  false: nothing launched.
enum { RT_PATH_INIT = 0, RT_PATH_SWEEP = 1, RT_PATH_FINISH = 2 };
struct RtPathQuery {
    int stage;
    const uint32_t* occupancy;
    const uint32_t* d2;
    const uint32_t* seeds;
    uint32_t n_seeds;
    uint32_t* passable;
    uint32_t* flags;
    uint32_t* counters;
    uint32_t dims[3];
    uint32_t limit; // rtq::path_limit
    uint32_t first_sweep, sweeps;
    uint32_t* cost;
    uint8_t* flow;
    uint32_t* status;
    uint32_t sweep_blocks, point_blocks;
};
bool rt_launch_pathquery(const RtLaunch& a, const RtPathQuery& q);

// A visibility field's one pass (rt_terrain_visibility_field; the definition is in include/frosttrace.h, the walk and
// the scratch layout in rt_rayquery.h): k_visibility stores for every point the mask of the observers it sees.
// `occupancy` as in RtDistanceQuery; `observers`: n_observers (1..rtq::kVisMaxObservers) records x, y, z, kind, an
// invalid one seeing nothing; range2: max_range squared, 0 for none.  counters (may be null: nothing is counted):
// four words that are 0 when the kernel starts, zeroed on a.stream by the caller, and hold the status after it.
// All dims >= 1 with a product of 2^26 at most; blocks of rtq::kDistThreads threads.  false: nothing launched.
struct RtVisibilityQuery {
    const uint32_t* occupancy;
    const int32_t* observers;
    uint32_t n_observers;
    uint32_t dims[3];
    uint32_t range2;
    uint32_t* mask;
    uint32_t* counters;
    uint32_t blocks;
};
bool rt_launch_visibilityquery(const RtLaunch& a, const RtVisibilityQuery& q);

// A region field's passes (rt_terrain_region_field; the definition is in include/frosttrace.h, the forest, find and
// unite and the scratch layout in rt_rayquery.h), enqueued on a.stream: k_regionlocal (the member words from
// `occupancy` and, if not null, `d2`; every tile labelled on its own), k_regionmerge, k_regionflatten and, when
// `counts` is not null, k_regionfinish.  member: the lattice's word count; counts: a word a point, or null when
// neither `size` nor `status` is asked for (both null then): nothing is counted and k_regionfinish is not launched.
// counters: rtq::REGION_CNT_WORDS words that are 0 when the first kernel starts, zeroed on a.stream by the caller.
// solid: members are the blocked points (d2 null).  faces: connectivity 6.  All dims >= 1 with a product of 2^26
// at most.  false: nothing launched.
struct RtRegionQuery {
    const uint32_t* occupancy;
    const uint32_t* d2;
    uint32_t* member;
    uint32_t* counts;
    uint32_t* counters;
    uint32_t dims[3];
    bool solid, faces;
    uint32_t* label;
    uint32_t* size;
    uint32_t* status;
    uint32_t tile_blocks, point_blocks;
};
bool rt_launch_regionquery(const RtLaunch& a, const RtRegionQuery& q);

#define RT_TILE 32
#define RT_FIN_SLOTS 1536 // k_trace's fin pool slots per block
#define RT_AO_POOL_SLOTS 256 // k_trace's AO counter slots per block (LDS) and their colours (cpool)
// k_trace's queue capacities per block (1024 threads = 16 waves): the hit queue and the long-ray
// spill stack.  A wave starts a primary unit only while fewer than 64 hits are queued and starts
// shading only while fewer than 128 long rays are (k_trace's work priority), so a block never
// queues more than 64 + 16 * 64 * aa hits or 128 + 16 * 64 * (1 + ao) long rays plus 16 compaction
// hand-backs of < 64: the rings cannot fill.
inline void rt_spill_caps(int aa, int ao, uint32_t* hits, uint32_t* longs)
{
    *hits = 64u * (uint32_t)aa * 17u + 64u;
    *longs = 64u * 16u * (uint32_t)(ao + 2) + 256u;
}
// samples the split pipeline addresses for a w x h frame: whole 32x32 tiles x AA
inline size_t rt_split_samples(int w, int h, int aa)
{
    return (size_t)((w + RT_TILE - 1) / RT_TILE) * ((h + RT_TILE - 1) / RT_TILE) * RT_TILE * RT_TILE * (size_t)aa;
}
inline size_t rt_shard_tiles(int w, int h, int rank, int count)
{
    size_t tx = (size_t)(w + RT_TILE - 1) / RT_TILE, ty = (size_t)(h + RT_TILE - 1) / RT_TILE, total = tx * ty;
    return total > (size_t)rank ? (total - (size_t)rank + (size_t)count - 1) / (size_t)count : 0;
}
// RGBA8 framebuffer -> BGRX rows (RecorderWinAPI::write's swizzle), dst pitch in uint32 words
void rt_launch_bgrx(hipStream_t s, const uint32_t* fb, uint32_t* dst, int w, int h, int pitch_words);
// The readback ring's snapshot: `words` RGBA8 words of a framebuffer into a tight staging slot (both 16-byte
// aligned), converted to BGRX on the way if bgrx != 0.  words < 2^32.
void rt_launch_snapshot(hipStream_t s, const uint32_t* fb, uint32_t* dst, size_t words, int bgrx);
// Shard transport jobs of one launch (a kernel argument: 2.5 KiB): job j copies shard shard[j]
// of the w x h framebuffer fb[j] to packed[j] (pack != 0: 1024 px per tile, tiles ascending) or back.
#define RT_SHARD_JOBS 128
struct ShardJobs {
    uint32_t* fb[RT_SHARD_JOBS];
    uint32_t* packed[RT_SHARD_JOBS];
    int shard[RT_SHARD_JOBS];
};
void rt_launch_shard_copy(hipStream_t s, const ShardJobs& jobs, int n, int w, int h, int count, int pack);

// diagnostics (primitive-level parity tests)
void rt_launch_debug_math(hipStream_t s, int op, const float* a, const float* b, float* y, int n);
void rt_launch_debug_noise(const RtLaunch& a, const float* xyz, float* out, int n, int density);
void rt_launch_debug_sky(const RtLaunch& a, const float* dirs, float* out, int n);
void rt_launch_debug_spin(hipStream_t s, const unsigned long long* base, unsigned long long until_ticks,
                          unsigned long long ticks, unsigned long long* stamp);
