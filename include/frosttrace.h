/*
 * frosttrace.h -- C-ABI drop-in boundary of the MI355X-native terrain ray-marcher.
 *
 * Every entry point replaces one call of the reference engine's dispatch-and-
 * readback surface (paths relative to /root/reference/gpuraytrace):
 *
 *   IDevice         Factories/IDevice.h:16-54, DeviceFactory.cpp:6-29
 *   ICompute        Factories/ICompute.h:16-59 (implemented by Adapters/ComputeDirect3D.cpp)
 *   IShaderVariable Graphics/IShaderVariable.h:7-40 (ShaderVariableDirect3D.cpp:195-202)
 *   IShaderArray    Graphics/IShaderVariable.h:42-61 (UAVBufferD3D :92-193, StructuredBufferD3D :204-281)
 *   ITexture        Factories/ITexture.h:38-63 (TextureDirect3D.cpp:40-164)
 *   VFS::addPath    Common/VFS.h (landscape selection, Terrain.cpp:23)
 *
 * Conventions: plain C types only; opaque handles; functions return RT_OK (0) or
 * a negative RT_ERR_* code and set a thread-local message (rt_last_error()).
 * Lookups that the reference answers with nullptr (missing variable/array)
 * return NULL here too.  All GPU work is enqueued on the device's HIP stream;
 * calls that hand data to the host (rt_array_map, rt_device_readback*) block.
 */
#ifndef FROSTTRACE_H
#define FROSTTRACE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 9

enum {
    RT_OK = 0,
    RT_ERR_INVALID = -1,    /* bad handle / argument */
    RT_ERR_HIP = -2,        /* HIP runtime error (message carries hipGetErrorString) */
    RT_ERR_NOT_FOUND = -3,  /* unknown shader file / entry / landscape */
    RT_ERR_UNSUPPORTED = -4,/* operation the reference also rejects (e.g. map on an SRV array) */
    RT_ERR_STATE = -5       /* e.g. run() before create()/swap(), missing texture */
};

/* DeviceDirect3D.cpp:113-126 swap-chain format R8G8B8A8_UNORM is always
 * produced; RT_DEVICE_FLOAT_OUTPUT additionally keeps the pre-quantisation
 * float4 colour (texOut's float4 value, tracescreen.hlsl:75) for parity. */
enum {
    RT_DEVICE_FLOAT_OUTPUT = 1u,
    RT_DEVICE_STATS = 2u,
    RT_DEVICE_GRAPH = 4u,
    /* 8u, 16u: retired in ABI 6 (ABI <= 5 RT_DEVICE_SEG_TAIL_OFF / _ON, no effect since ABI 4);
     * rt_device_create rejects them, as every unknown flag */
    RT_DEVICE_DEBUG_SMALL_RINGS = 32u,
    RT_DEVICE_DEBUG_WITHHOLD_FUSE = 64u,
    RT_DEVICE_GATED = 128u,
    RT_DEVICE_DEBUG_GATE_STRESS = 512u,
    RT_DEVICE_DEFERRED = 1024u,
    RT_DEVICE_DEBUG_DEFER_SMALL = 2048u
};
/* RT_DEVICE_GRAPH: rt_terrain_render / rt_terrain_render_feed capture the frame's launches
 * into two hipGraphs (prepass + setTargetDepths, tracescreen) on first use and replay them
 * every frame; a changed launch argument (shader swap, buffers, shard, stats) re-captures.
 * No reference counterpart (the D3D frame loop re-records its dispatches every frame).
 * RT_DEVICE_DEBUG_SMALL_RINGS (ABI 4, diagnostic): the trace kernel's per-CU LDS long-ray ring holds
 * 64 entries instead of 570 and its fin pool 8 slots instead of 1536, so queued long rays take the
 * per-block spill rings in HBM and most long shadows the fin[t] fallback (the parity tests run
 * frames through those paths); same bits, slower.
 * RT_DEVICE_GATED (ABI 7, opt-in): a full nomadplains render this device leads (rt_terrain_render /
 * _batch, not the camera feed, not the instrumented RT_DEVICE_STATS kernels) is ONE gated launch: the
 * trace kernel runs the batch's prepass rays first and starts each 8x8 unit as soon as the prepass rays
 * its cells' setTargetDepths reads are in; the frame's last prepass task writes its CellDistance.  Same
 * bits as the default sequence (the camerarays prepass as its own launch, then setTargetDepths and the
 * trace).  Measured slower on MI355X (prepass rays that share their SIMDs with
 * units march 2-3x slower than alone), so it is not the default.
 * RT_DEVICE_DEBUG_WITHHOLD_FUSE (ABI 7, diagnostic): a trace this device leads that would run the next
 * batch's fused prepass (rt_terrain_trace_ahead) runs none of its tasks, so that batch's bounded wait
 * times out: the fail-safe's test (rt_device_check below).
 * RT_DEVICE_DEBUG_GATE_STRESS (ABI 8, diagnostic, with RT_DEVICE_GATED): the gated launch's cross-CU hand-off of a
 * frame's CellDistance under stress -- every trace wave first reads the frame's previous CellDistance with
 * plain loads (its CU's L1 holds lines that the frame's last prepass task then rewrites) and that task waits
 * ~200 us before it stores them, so units read the flagged cells late, on CUs whose L1 holds the old ones.
 * RT_DEVICE_DEFERRED (ABI 9): deferred submission for the one-frame-per-call loop.  rt_terrain_render queues
 * its frame's prepass (or has it queued) and uploads both constant blocks, but its setTargetDepths + trace are
 * launched by the NEXT rt_terrain_render, whose own frame's prepass then runs inside that trace kernel
 * (nomadplains, a trace that has tiles, the same noise tables): a D3D driver's batching of a frame's
 * dispatches until the next submission, without a prepass launch that waits for the trace's CUs.  Every other
 * call that launches on, reads, waits on or reconfigures the device -- rt_device_flush, _synchronize,
 * _readback*, _stats*, _kernel_time, _set_stream, _wait_event, _record_event, _check, _framebuffer, _stream,
 * _destroy, rt_device_present while recording (synchronously; not with rt_recorder_set_async), any other render, prepass or shard call, a map / unmap / write
 * or device pointer of its arrays, a compute run / swap / destroy / set_texture, a texture init / destroy,
 * rt_device_defer_batch -- launches a pending
 * frame first.  rt_device_present without a recorder launches nothing (there is no display): a caller that
 * reads the framebuffer through its own stream calls rt_device_flush or rt_device_record_event first.  Same
 * bits as without the flag.  At one frame to a launch (the default; rt_device_defer_batch), a device of fewer than
 * 1280 x 720 pixels renders every frame as without the flag: its trace is shorter than the prepass it would carry
 * (profiles/r06/deferred.md).
 * RT_DEVICE_DEBUG_DEFER_SMALL (ABI 9, diagnostic, with RT_DEVICE_DEFERRED): the one-frame deferral at every frame
 * size, so that tests run it on small frames. */

/* ITexture.h:7-33 enum values */
enum { RT_TEXTURE_1D = 0, RT_TEXTURE_2D = 1, RT_TEXTURE_3D = 2 };
enum { RT_FORMAT_UNKNOWN = 0, RT_FORMAT_R8G8B8A8_SNORM = 1, RT_FORMAT_R8G8B8A8_UNORM = 2, RT_FORMAT_R8G8B8A8_UINT = 3 };

typedef struct rt_device_s* rt_device;
typedef struct rt_compute_s* rt_compute;
typedef struct rt_texture_s* rt_texture;
typedef struct rt_variable_s* rt_variable;
typedef struct rt_array_s* rt_array;
typedef struct rt_recorder_s* rt_recorder;

typedef struct {
    unsigned long long primary_steps; /* traceRay iterations, primary rays */
    unsigned long long shadow_steps;  /* traceRay iterations, shadow rays */
    unsigned long long prepass_steps; /* traceRay iterations, camerarays */
    unsigned long long hits;          /* primary hits == shadow rays */
    unsigned long long noise_calls;   /* noise3d evaluations (BASELINE.md algorithmic work unit) */
    unsigned long long ao_steps;      /* traceRay iterations, AO rays (build extension RT_AO_SAMPLES) */
    unsigned long long noise_wave_iters; /* wave64 iterations of the noise3d evaluations outside the prepass
                                          * (noise_calls / (64 * this) = SIMD lane utilisation of the
                                          * noise work; ABI 2) */
} rt_stats;

/* ---- diagnostics ---- */
const char* rt_last_error(void);
int rt_abi_version(void);

/* ---- VFS (Common/VFS.cpp:19-31; Terrain.cpp:23 adds "Media/<landscape>") ----
 * The most recently added "Media/<name>" path selects the landscape whose
 * shaders rt_compute_create() loads (nomadplains, testing, simple, greenrocks). */
int rt_vfs_add_path(const char* path);
int rt_vfs_clear(void);

/* ---- IDevice ----
 * rt_device_create  <- DeviceFactory::construct + DeviceDirect3D::create (DeviceDirect3D.cpp:77-227):
 *                      `ordinal` is the -g adapter index (:128-141), width/height the window size.
 * rt_device_present <- IDevice::present (DeviceDirect3D.cpp:234-257): frame boundary.
 * rt_device_flush   <- IDevice::flush (DeviceDirect3D.cpp:259-262).
 * rt_device_readback<- the present() staging readback (:244-256): RGBA8 rows, `row_pitch` bytes apart. */
int rt_device_create(int ordinal, int width, int height, unsigned flags, rt_device* out);
void rt_device_destroy(rt_device dev);
int rt_device_present(rt_device dev);
int rt_device_flush(rt_device dev);
int rt_device_synchronize(rt_device dev);
int rt_device_readback(rt_device dev, void* dst, size_t row_pitch);
int rt_device_readback_float(rt_device dev, float* dst); /* W*H*4 floats, needs RT_DEVICE_FLOAT_OUTPUT */
/* rt_device_readback_bgrx <- the recorder's readback (DeviceDirect3D.cpp:242-256) with
 * RecorderWinAPI::write's pixel conversion (RecorderWinAPI.cpp:244-253) done on the GPU:
 * rows of W uint32 (B, G, R, 0) = MFVideoFormat_RGB32, `row_pitch` bytes apart. */
int rt_device_readback_bgrx(rt_device dev, void* dst, size_t row_pitch);
int rt_device_size(rt_device dev, int* width, int* height);
void* rt_device_framebuffer(rt_device dev);       /* device pointer, W*H uint32 RGBA8 */
void* rt_device_stream(rt_device dev);            /* hipStream_t */
/* NULL = the device's own stream.  Devices' own streams are reference-counted: a device that
 * borrows another device's stream keeps it alive, so the owner may be destroyed first (its stream
 * is destroyed with its last user).  A stream no device created (the caller's) must outlive every
 * device using it: rt_device_destroy synchronizes the stream its device uses. */
int rt_device_set_stream(rt_device dev, void* hip_stream);
/* (ABI 4) devices currently holding `hip_stream` (its owner while alive + its borrowers); 0 for a
 * stream no live device created. */
int rt_stream_refs(void* hip_stream);
int rt_device_stats(rt_device dev, rt_stats* out, int reset); /* needs RT_DEVICE_STATS */
/* (ABI 4) the same with the caller's struct size: writes min(size, sizeof(rt_stats)) bytes, so a
 * caller built against an older, shorter rt_stats is never written past its struct. */
int rt_device_stats_sized(rt_device dev, rt_stats* out, size_t size, int reset);
/* HIP-event timing of the dominant kernel (tracescreen) on the device stream:
 * enable, then rt_device_kernel_time returns the summed elapsed ms and launch count
 * since the last call (synchronises). */
int rt_device_set_profiling(rt_device dev, int enable);
int rt_device_kernel_time(rt_device dev, double* total_ms, int* launches);
/* RT_DEVICE_GRAPH bookkeeping: graphs captured and graph launches since device creation. */
int rt_device_graph_info(rt_device dev, unsigned long long* captures, unsigned long long* launches);
/* (ABI 7) Counters of the renders a device led: RT_INFO_GATED_LAUNCHES = renders whose prepass ran inside
 * their trace kernel (the gated launch), RT_INFO_PREPASS_LAUNCHES = renders with a prepass launch of
 * their own, RT_INFO_PRESTREAM_RENDERS = those of them whose prepass ran on the device's prepass stream
 * (rt_terrain_render with a frame in flight).  No reference counterpart (the tests check which sequence
 * ran). */
/* (ABI 9) RT_INFO_DEFERRED_FUSED: RT_DEVICE_DEFERRED renders whose prepass ran inside the previous frame's
 * trace kernel. */
enum { RT_INFO_GATED_LAUNCHES = 0, RT_INFO_PREPASS_LAUNCHES = 1, RT_INFO_PRESTREAM_RENDERS = 2, RT_INFO_DEFERRED_FUSED = 3 };
int rt_device_info(rt_device dev, int key, unsigned long long* out);
/* (ABI 8) The trace kernel of the renders this device leads launches (CUs - n) persistent blocks instead of
 * one per CU (0 <= n < CUs; default 0), so n CUs stay free beside it for another stream's kernels -- a
 * collective's (RCCL's receive on rank 0 at N > 1, which otherwise queues behind the other batch's trace
 * until its tail) or a transport copy.  Same bits.  No reference counterpart. */
int rt_device_reserve_cus(rt_device dev, int n);
/* (ABI 9) An RT_DEVICE_DEFERRED device traces `frames` (1..4; default 1) frames to a launch: each rt_terrain_render
 * of the whole frame (shard 0 of 1) snapshots its frame's constant blocks into a frame slot of the device (its own
 * CameraResults, CellDistance and framebuffers) and queues it; every frames-th render launches the oldest
 * `frames` queued frames' setTargetDepths + trace as one batch, with the next `frames` frames' prepasses inside
 * that trace kernel.  A flush (the calls listed under RT_DEVICE_DEFERRED) launches everything queued; its last
 * frame writes the device's framebuffers and the compute pair's CellDistance and CameraResults, the others write
 * their slots (scratch: the reference's DISCARD swap chain never shows a frame that was not presented to a
 * reader).  Same bits per frame.  Changing it launches what is queued.  No reference counterpart (the D3D
 * runtime queues up to three frames). */
int rt_device_defer_batch(rt_device dev, int frames);
/* (ABI 6) Stream handoff without a host synchronisation.  `hip_event` is a hipEvent_t the caller
 * owns (a C++ host's, or torch.cuda.Event.cuda_event).  rt_device_wait_event: the work the device
 * queues from now on waits for the event -- e.g. buffers the caller filled on its own stream, then
 * recorded the event there (rt_shard_unpack's source, the split prepass's gathered CameraResults).
 * rt_device_record_event: records the event after everything queued on the device so far; the
 * caller's stream waits for it (hipStreamWaitEvent) before it reads the device's outputs.  The
 * device streams are non-blocking, so without one of these (or a host synchronisation) a caller's
 * stream and a device's run in no order.  No reference counterpart (D3D11 orders one immediate
 * context implicitly). */
int rt_device_wait_event(rt_device dev, void* hip_event);
int rt_device_record_event(rt_device dev, void* hip_event);
/* (ABI 6) Queue-overflow check: k_trace's per-block queues (hit stack, long-ray spill ring) are
 * bounded by its work priorities (rt_spill_caps); a push that would exceed a bound is not stored and
 * raises a sticky flag on the device instead of overwriting queued work.  rt_device_check
 * synchronises the device stream and returns RT_ERR_STATE (the message names the queue) if any
 * flag was raised since the last check, clearing it; RT_OK otherwise.
 * (ABI 7) Fail-safe of the fused prepass (rt_terrain_trace_ahead): when a batch's bounded wait for
 * its prepass rays times out (0.5 s; never expected), its frames may be wrong.  The kernel then also
 * sets a host-mapped word of its GPU, and from then on every call that launches on, synchronises or
 * reads a device of that GPU (rt_terrain_*, rt_compute_run, rt_device_present / synchronize /
 * readback*, rt_array_map, rt_shard_*) returns RT_ERR_STATE, until rt_device_check on a device of
 * that GPU reports and clears it.  A host that follows the reference's call sequence and never calls
 * rt_device_check therefore cannot read such a frame silently. */
int rt_device_check(rt_device dev);

/* ---- Asynchronous frame readback (ABI 9, additive) ----
 * rt_device_readback* and a recording rt_device_present end in a host synchronisation, so a host that looks at
 * every frame (a window blit, the recorder, the reference's render / present / readback loop) never has a frame
 * in flight.  A readback ring hands frames to the host without one.  No reference counterpart (the reference
 * maps its staging texture in present(), DeviceDirect3D.cpp:244-256).
 * rt_readback_create  (ABI 9, additive) a ring of `depth` (1..8) captures of `dev`'s frames, RT_READBACK_RGBA8
 *                     (rt_device_readback's bytes) or RT_READBACK_BGRX (rt_device_readback_bgrx's).  It owns
 *                     `depth` device staging slots, `depth` pinned host slots (W*H*4 bytes, tight rows), one
 *                     non-blocking copy stream and two events per slot (timing disabled), all made here: no call
 *                     below allocates.  An allocation failure frees what was made and returns the error.
 * rt_readback_submit  (ABI 9, additive) captures the frame rt_device_readback would return if called now -- the
 *                     latest render's -- and returns its ticket (0, 1, 2, ...).  It never waits for the GPU: a
 *                     snapshot kernel copies the framebuffer into a staging slot on the device stream (so the
 *                     next trace may overwrite the framebuffer), and the copy stream carries the slot to pinned
 *                     memory behind an event.  Only the framebuffer is touched: the frames-in-flight path of
 *                     rt_terrain_render goes on (the next prepass still runs on the prepass stream), and an
 *                     RT_DEVICE_GRAPH device re-captures nothing.  With every slot still the caller's it returns
 *                     RT_ERR_STATE ("ring full") and queues nothing.  On an RT_DEVICE_DEFERRED device it does NOT
 *                     launch a pending frame: the capture is attached to the newest rendered frame and queued
 *                     right behind that frame's trace by whichever call launches it, from the buffer the frame
 *                     really wrote; with nothing pending it is queued at once.  A capture whose frame is dropped
 *                     on a launch error fails (wait and ready return RT_ERR_STATE; release frees it).  At K frames
 *                     to a launch (rt_device_defer_batch) a frame's trace goes out up to 2K-1 renders after its
 *                     own, so a consumer that waits for a newer ticket than n-(2K-1) launches the queue early,
 *                     and one that lags fewer than 2K+1 frames leaves the GPU nothing queued while it waits
 *                     (a ring of 2K+2 keeps K = 2 at its rate, profiles/r07/readback_ring.md).
 * rt_readback_ready   (ABI 9, additive) 1 = the capture is in its pinned slot, 0 = not yet (always, while its
 *                     frame is not launched), < 0 = error.  Launches nothing.
 * rt_readback_wait    (ABI 9, additive) launches what is pending if the capture is not queued yet, waits for that
 *                     capture's event only (not the stream), then checks the fail-safe word (rt_device_check):
 *                     if it is set, RT_ERR_STATE, *pixels = NULL and the capture has failed; else *pixels is the
 *                     pinned slot, valid until rt_readback_release.  Waiting twice is allowed.
 * rt_readback_release (ABI 9, additive) returns a capture's slot to the ring after a successful wait, a ready
 *                     result of 1, or a failure; in any order.  RT_ERR_STATE for a capture still in flight.
 * An unknown or released ticket is RT_ERR_INVALID everywhere.
 * rt_readback_destroy (ABI 9, additive) drains the copy stream and cancels attached captures.  rt_device_destroy
 *                     before it detaches the ring (as a recorder): every later call returns RT_ERR_STATE. */
enum { RT_READBACK_RGBA8 = 0, RT_READBACK_BGRX = 1 };
typedef struct rt_readback_s* rt_readback;
int rt_readback_create(rt_device dev, int format, int depth, rt_readback* out);
int rt_readback_submit(rt_readback rb, unsigned long long* ticket);
int rt_readback_ready(rt_readback rb, unsigned long long ticket);
int rt_readback_wait(rt_readback rb, unsigned long long ticket, const void** pixels);
int rt_readback_release(rt_readback rb, unsigned long long ticket);
void rt_readback_destroy(rt_readback rb);

/* ---- ITexture (IDevice::createTexture + ITexture::create(dims, fmt, w, h, data, binding, cpu)) ---- */
int rt_texture_create(rt_device dev, rt_texture* out);
int rt_texture_init(rt_texture tex, int dimensions, int format, int width, int height, const void* data,
                    int binding, int cpu_access);
void rt_texture_destroy(rt_texture tex);

/* ---- ICompute ----
 * rt_compute_create     <- IDevice::createCompute (DeviceDirect3D.cpp:264-267)
 * rt_compute_load       <- ICompute::create(directory, file, entry, ThreadSize, macros)
 *                          (ComputeDirect3D.cpp:403-465).  Files: "tracescreen.hlsl",
 *                          "camerarays.hlsl"; macros RECORDING, AA_SAMPLES and the build
 *                          extension RT_MAX_STEPS.  A failed load keeps the previous shader.
 * rt_compute_swap       <- ICompute::swap (:508-528): 1 if a new shader became current;
 *                          invalidates the handles from rt_compute_get_*.
 * rt_compute_run        <- ICompute::run (:530-581): dispatch (dx,dy,dz) groups of the
 *                          compiled thread size; silent no-op without a current shader.
 * rt_compute_set_texture<- ICompute::setTexture (:583-614), borrowed (not owned).
 * rt_compute_get_*      <- getVariable/getArray/getBuffer by reflected name (NULL if absent;
 *                          getBuffer is always NULL, as the reference's CBuffer=0 mask makes it). */
int rt_compute_create(rt_device dev, rt_compute* out);
void rt_compute_destroy(rt_compute cs);
int rt_compute_load(rt_compute cs, const char* directory, const char* file, const char* entry, int tx, int ty, int tz,
                    const char* const* macro_names, const char* const* macro_values, int n_macros);
int rt_compute_swap(rt_compute cs);
int rt_compute_run(rt_compute cs, unsigned dispatch_x, unsigned dispatch_y, unsigned dispatch_z);
int rt_compute_set_texture(rt_compute cs, int stage, rt_texture tex);
int rt_compute_thread_size(rt_compute cs, int* x, int* y, int* z);
rt_variable rt_compute_get_variable(rt_compute cs, const char* name);
rt_array rt_compute_get_array(rt_compute cs, const char* name);
void* rt_compute_get_buffer(rt_compute cs, const char* name);

/* ---- IShaderVariable ---- write copies exactly the reflected size (cbuffer shadow, uploaded lazily on run) */
int rt_variable_write(rt_variable var, const void* data);
size_t rt_variable_size(rt_variable var);
const char* rt_variable_name(rt_variable var);

/* ---- IShaderArray ----
 * create: allocate `elements` x reflected stride.  UAV arrays (CameraResults): map = blocking
 * device->host copy, unmap = host->device copy back; write unsupported.  SRV arrays
 * (CellDistance): write = full upload; map/unmap unsupported.  As UAVBufferD3D/StructuredBufferD3D. */
int rt_array_create(rt_array arr, unsigned elements);
void* rt_array_map(rt_array arr);
int rt_array_unmap(rt_array arr);
int rt_array_write(rt_array arr, const void* data);
size_t rt_array_stride(rt_array arr);
void* rt_array_device_pointer(rt_array arr);

/* ---- Terrain::render without the host round trip (Terrain.cpp:105-136) ----
 * Runs camera_cs (prepass) -> setTargetDepths on the device (Terrain.cpp:398-439) ->
 * screen_cs over the whole screen, all enqueued on the device stream.  Equivalent to the
 * reference sequence run(2,2,1); CameraResults map/unmap; setTargetDepths; CellDistance
 * write; tiled run(...).  With shard_count > 1 only screen tiles t (32x32 pixels,
 * row-major tile index) with t % shard_count == shard_rank are traced.
 * Frames in flight (ABI 7, same bits): from a device's second consecutive rt_terrain_render on,
 * the prepass runs on the device's own prepass stream, ordered after the previous frame's
 * setTargetDepths (the last reader of CameraResults) and before this frame's setTargetDepths, so it
 * overlaps the previous frame's trace; the device stream stays the order a host sees (synchronise,
 * readbacks, events).  Any other call that touches the device's arrays or launches on it (a batch, the
 * feed, an ahead prepass, rt_compute_run, rt_array_unmap / write, a stream change, rt_device_wait_event)
 * makes the next render prepass in line.  A host writing CameraResults through rt_array_device_pointer on its own
 * must synchronise first.  Not for RT_DEVICE_GRAPH, RT_DEVICE_STATS or RT_DEVICE_GATED devices. */
int rt_terrain_render(rt_compute camera_cs, rt_compute screen_cs, int shard_rank, int shard_count);
/* rt_terrain_render_feed: rt_terrain_render that also hands the frame's 1024 CameraResults
 * (camerarays.hlsl:12-21, Terrain::getCameraView) to the host as soon as the prepass ends,
 * without waiting for tracescreen -- the feed of Flyby::fly (Gameplay/Flyby.cpp:26-196, which
 * reads the previous frame's view).  rt_terrain_feed_wait blocks until that copy has landed and
 * copies it (1024 x float4: hit xyz, depth) to `camera_results`. */
int rt_terrain_render_feed(rt_compute camera_cs, rt_compute screen_cs, int shard_rank, int shard_count);
int rt_terrain_feed_wait(rt_compute camera_cs, float* camera_results);
/* rt_terrain_render_batch: rt_terrain_render for n (1..24; 16 before ABI 6) frames at once -- frame i is
 * (camera_cs[i], screen_cs[i]), each with its own constants (camera, sun), CameraResults,
 * CellDistance and device framebuffer.  All frames must share one GPU, resolution,
 * landscape, macro set and noise tables.  Every frame's prepass runs in one launch, and one
 * tracescreen launch traces all frames' units frame-major, so one frame's last rays overlap
 * the next frame's units instead of idling the GPU.  Enqueued on the stream of frame 0's
 * device with frame 0's device buffers and counters; streams of frames on other devices
 * wait for the batch.  No reference counterpart (the reference renders one frame per
 * Terrain::render); each frame's pixels equal its rt_terrain_render frame bit for bit.
 * Sharded (shard_count > 1, n > 1): frame i traces shard (shard_rank + i) % shard_count, a
 * per-frame rotation that evens out the ranks' work; rt_shard_pack/unpack frame i with that
 * shard index. */
int rt_terrain_render_batch(const rt_compute* camera_cs, const rt_compute* screen_cs, int n, int shard_rank,
                            int shard_count);
/* (ABI 7) rt_terrain_render_batch of a shard (shard_count >= 2) whose pixels go straight to a packed
 * device buffer instead of the framebuffers: frame i's shard at dst_device + i * frame_stride, in
 * rt_shard_pack's layout (its k-th tile at k * 4 KiB, rows of 32 pixels).  The trace kernels store there
 * directly, so a rank's batch needs no rt_shard_pack_batch launch before its gather (the pack queued
 * behind the other batch in flight; parallel.run_batch's direct pack).  RGBA8-only devices
 * (RT_ERR_UNSUPPORTED with RT_DEVICE_FLOAT_OUTPUT); the framebuffers are not written. */
int rt_terrain_render_batch_packed(const rt_compute* camera_cs, const rt_compute* screen_cs, int n, int shard_rank,
                                   int shard_count, void* dst_device, size_t frame_stride);
/* The same batch in two phases, for a prepass split across ranks (one process per GPU):
 * rt_terrain_prepass_batch runs the camerarays prepass of frames [first, first + count) only
 * and writes frame f's 1024 CameraResults to camera_out + f * 1024 float4 (a device buffer of
 * n * 16 KiB); the ranks' shares are then exchanged with one all-gather of that buffer, and
 * rt_terrain_trace_batch runs setTargetDepths + tracescreen of all n frames from camera_in
 * (the gathered buffer), copying each frame's results into its CameraResults array too.
 * The prepass is deterministic, so the frames equal rt_terrain_render_batch's bit for bit. */
int rt_terrain_prepass_batch(const rt_compute* camera_cs, const rt_compute* screen_cs, int n, int first, int count,
                             void* camera_out);
int rt_terrain_trace_batch(const rt_compute* camera_cs, const rt_compute* screen_cs, int n, int shard_rank,
                           int shard_count, const void* camera_in);
/* (ABI 5) The prepass one batch ahead, for a stream of batches (FrameRing(lookahead=True),
 * parallel.run_batch): rt_terrain_prepass_ahead queues the batch's camerarays prepass (into each
 * frame's CameraResults) on the GPU's side stream -- one per GPU, created on first use -- after
 * the last setTargetDepths of the batches screen_cs[0]'s device leads (their last read of those
 * arrays).  Issued before the previous batch's trace, it gets CUs before that trace's persistent
 * kernel holds them all.  rt_terrain_trace_ahead then runs setTargetDepths + tracescreen of the
 * batch after that prepass; for frames the pending prepass did not cover (other computes, more
 * frames, or camera constants written since) it renders the full batch (rt_terrain_render_batch)
 * instead, so the frames always equal rt_terrain_render_batch's bit for bit.  One ahead prepass
 * per leading device at a time (RT_ERR_STATE otherwise); not on RT_DEVICE_GRAPH devices.
 * No reference counterpart (Terrain::render runs its prepass in line, Terrain.cpp:105-136). */
int rt_terrain_prepass_ahead(const rt_compute* camera_cs, const rt_compute* screen_cs, int n);
int rt_terrain_trace_ahead(const rt_compute* camera_cs, const rt_compute* screen_cs, int n, int shard_rank,
                           int shard_count);
/* Tile-cyclic shard transport: pack this rank's tiles from the framebuffer into a
 * contiguous device buffer (RGBA8, 32x32-pixel tiles in tile order), or unpack a rank's
 * packed tiles into the framebuffer.  Byte counts from rt_shard_bytes. */
size_t rt_shard_bytes(rt_device dev, int shard_rank, int shard_count);
int rt_shard_pack(rt_device dev, int shard_rank, int shard_count, void* dst_device);
int rt_shard_unpack(rt_device dev, int shard_rank, int shard_count, const void* src_device);
/* The same for n frames in one launch (ABI 3): job i packs shard shard_ranks[i] of devs[i]'s
 * framebuffer into dst_device[i] (or unpacks src_device[i] into it).  Every device has the same
 * size; the launch runs on devs[0]'s stream, and devices on other streams are ordered around it
 * (their earlier work before, their later work after).  A batch's root unpacks its (N-1) x B
 * shards with one call (parallel.run_batch) instead of one launch each. */
int rt_shard_pack_batch(const rt_device* devs, const int* shard_ranks, int shard_count, void* const* dst_device,
                        int n);
int rt_shard_unpack_batch(const rt_device* devs, const int* shard_ranks, int shard_count,
                          const void* const* src_device, int n);

/* ---- host helpers (Noise.cpp:39-94, Camera.cpp, Terrain.cpp:285-311) ----
 * rt_noise_generate: the engine's noise tables; rand_kind 0 = MSVC CRT rand (the
 * reference's shipping platform), 1 = glibc rand.  perm2d: 128*128*4 bytes,
 * grad: 128*4 floats. */
int rt_noise_generate(uint32_t seed, int rand_kind, uint8_t* perm2d, float* grad);
/* Terrain::setTargetDepths (Terrain.cpp:398-439) on the host: CameraResults float4[1024] ->
 * CellDistance float2[1024], for engines that keep the reference's readback round trip. */
int rt_terrain_set_target_depths(const float* camera_results, float* cell_distance);

/* ---- ray queries (ABI 9, additive; no reference counterpart) ----
 * What a ray of the host's own hits: picking, placement, collision (Gameplay/Flyby.cpp:44-90 reads the prepass
 * hits for this, along the 1024 directions of the last frame only), height and depth maps.  A query is n rays
 * (origin_i, dir_i) and one LOD eye E per call; the compute supplies the landscape, the noise tables and the
 * landscape constants (either kind of compute, camerarays or tracescreen).  Result i is the CameraResults
 * element camerarays.hlsl:12-21 would have written for a pixel ray with p = origin_i and dir = dir_i:
 *     rr = traceRay(origin_i, 0.01, 5000, stepmod 2, dir_i, calcfog off, skiprefine on)    (tracing.hlsl:47-105)
 *     result_i = float4(rr.pd.xyz, rr.density < 0 ? 5000 : rr.pd.w),  steps_i = the loop's iteration count
 * so a hit is result.w < 5000, bit for bit what a prepass of such a camera stores.
 *   dir   is used as given, as the prepass uses its un-normalised p - Eye: its LENGTH enters the first step
 *         (tracing.hlsl:54), and the march then runs along dir / |dir|.  A zero dir gives (0, 0, 0, 0.01) and
 *         0 steps.  Non-finite inputs give unspecified results (the march still ends).
 *   E     replaces Eye wherever the density reads it (nomadplains' octave count, length(p - Eye)): the query
 *         sees the terrain at the level of detail the viewer at E sees.  Without RT_RAYS_EYE it is the compute's
 *         current Eye variable.  One per call, not per ray.
 *   No step cap (the prepass passes none); results in ray order.
 * rt_ray_options (opt may be NULL: all defaults): size = sizeof(rt_ray_options) of the caller's header (later
 *   versions append fields); RT_RAYS_FORCE_SEGMENTS / RT_RAYS_FORCE_LANES pick the kernel shape (default: by n
 *   and landscape; identical bits either way): segments march one ray on a group of lanes (nomadplains only:
 *   RT_ERR_UNSUPPORTED elsewhere; the prepass's latency shape, for few rays), lanes march a ray per lane in a
 *   persistent grid whose waves refill from a counter (every landscape; the throughput shape).  max_blocks
 *   caps that grid (0: every CU less rt_device_reserve_cus).
 * rt_terrain_trace_rays: host arrays, xyz interleaved (origins, dirs: 3n floats; results: 4n floats; steps: n
 *   uint32 or NULL); blocking, like rt_array_map.
 * rt_terrain_trace_rays_device: device arrays (rays: n x 8 floats ox oy oz _ dx dy dz _, 16-byte aligned;
 *   results n x 4 floats; steps n uint32 or NULL), enqueued on the compute's device stream with no host
 *   synchronisation: order other streams with rt_device_wait_event / rt_device_record_event.
 * Both: n == 0 is RT_OK and launches nothing.  RT_ERR_INVALID: n < 0, n > 2^26, a NULL compute or required
 *   array, opt->size below the first version (24), both force flags.  RT_ERR_STATE without texPerm2D bound, or
 *   with the fail-safe word set.  A query reads no frame state and changes none: it flushes no deferred frame,
 *   invalidates no ahead / fused prepass or captured graph, and uploads the constants it needs to a copy of
 *   its own, so it may run between any two renders. */
enum { RT_RAYS_EYE = 1, RT_RAYS_FORCE_SEGMENTS = 2, RT_RAYS_FORCE_LANES = 4 };
typedef struct {
    uint32_t size;
    uint32_t flags;
    float eye[3];
    uint32_t max_blocks;
} rt_ray_options;
int rt_terrain_trace_rays(rt_compute cs, const float* origins, const float* dirs, int n,
                          const rt_ray_options* opt, float* results, uint32_t* steps);
int rt_terrain_trace_rays_device(rt_compute cs, const void* rays_device, int n,
                                 const rt_ray_options* opt, void* results_device, void* steps_device);

/* ---- surface queries (ABI 9, additive; no reference counterpart) ----
 * Where a ray of the host's own meets the SURFACE, and the surface's normal there: picking and placement.
 * rt_terrain_trace_rays above returns the prepass's answer -- the first sample that landed inside the terrain,
 * up to metres below the surface, and no normal.  A surface query runs the refined march tracescreen runs for
 * its pixels and getNormal.  For ray i with origin_i and dir_i and one LOD eye E per call:
 *     rr       = traceRay(origin_i, t_min, t_max, stepmod, dir_i, calcfog off, skiprefine OFF)  (tracing.hlsl:47-105)
 *     hit      = rr.density > 0                                                          (tracescreen.hlsl:29)
 *     n        = hit ? getNormal(float4(rr.pd.xyz, rr.density)) : (0, 0, 0)               (tracing.hlsl:107-116)
 *     result_i = { float4(rr.pd.xyz, rr.pd.w), float4(n, rr.density) },  steps_i = the loop's iteration count
 * so result_i is 8 floats: position, distance | unit normal, density; a hit is result_i[7] > 0.
 *   dir   is used as given, as for rt_terrain_trace_rays: its LENGTH enters the first step (tracing.hlsl:54).
 *   E     replaces Eye in getDensity (nomadplains' octave count) AND in getNormal's eps = 0.005 |p - Eye|.
 *         Without RT_RAYS_EYE it is the compute's current Eye variable.  One per call.
 *   Defaults: t_min 0.01, t_max 5000, stepmod 1, max_steps 0 (unbounded) -- what a tracescreen pixel gets with an
 *         empty CellDistance.  With RT_SURFACE_PARAMS the option block's t_min, t_max, stepmod and max_steps
 *         hold instead (they are not read without the flag).  RECORDING and the landscape constants come from
 *         the compute.
 *   Refinement always ends on an inside sample: after a hit the step shrinks x0.3 and the loop condition is
 *         tested next, after a miss the step grows.  rr.pd.xyz is the last sample and rr.pd.w the loop's dist
 *         after the back-off, exactly as the reference returns them.
 *   max_steps > 0: a ray with steps_i == max_steps was ended by the cap and may be mid-refinement (its last
 *         sample need not be inside, nor near the surface).
 *   A zero dir gives, with the default range, 0 steps and { (0, 0, 0, t_min), (0, 0, 0, 0) }.  Non-finite
 *         inputs, or a zero dir with a large t_min, give unspecified results; the march still ends.
 *   Per-ray range: with RT_SURFACE_RAY_RANGE the packed ray's two spare words are t_min_i and t_max_i
 *         (ox oy oz t_min_i dx dy dz t_max_i) and replace t_min / t_max: segment queries such as line of
 *         sight between two points, or a start plane per ray as CellDistance gives tracescreen.  Without the
 *         flag the words are ignored.  The host form sets it itself when ranges != NULL (2n floats).
 * rt_surface_options (opt may be NULL: all defaults): size = sizeof(rt_surface_options) of the caller's header
 *   (later versions append fields); flags: RT_RAYS_EYE, RT_RAYS_FORCE_SEGMENTS, RT_RAYS_FORCE_LANES as above
 *   (identical bits in either shape), RT_SURFACE_PARAMS, RT_SURFACE_RAY_RANGE; max_blocks as above.
 * rt_terrain_trace_surface: host arrays, xyz interleaved (origins, dirs: 3n floats; ranges: 2n floats or NULL;
 *   results: 8n floats; steps: n uint32 or NULL); blocking.
 * rt_terrain_trace_surface_device: device arrays (rays n x 8 floats, 16-byte aligned; results n x 8 floats,
 *   16-byte aligned; steps n uint32 or NULL), enqueued on the compute's device stream with no host
 *   synchronisation: order other streams with rt_device_wait_event / rt_device_record_event.
 * Both: n == 0 is RT_OK and launches nothing.  RT_ERR_INVALID: n < 0, n > 2^26, a NULL compute or required
 *   array, opt->size below the first version (40), both force flags, and with RT_SURFACE_PARAMS a stepmod that
 *   is <= 0 or not finite or t_max < t_min.  RT_ERR_UNSUPPORTED: forced segments off nomadplains.  RT_ERR_STATE
 *   without texPerm2D bound, or with the fail-safe word set.  A query reads no frame state and changes none: it
 *   flushes no deferred frame, invalidates no ahead / fused prepass or captured graph, and uploads the
 *   constants it needs to a copy of its own, so it may run between any two renders. */
enum { RT_SURFACE_PARAMS = 8, RT_SURFACE_RAY_RANGE = 16 };
typedef struct {
    uint32_t size;
    uint32_t flags;
    float eye[3];
    uint32_t max_blocks;
    float t_min, t_max, stepmod;
    uint32_t max_steps;
} rt_surface_options;
int rt_terrain_trace_surface(rt_compute cs, const float* origins, const float* dirs, const float* ranges, int n,
                             const rt_surface_options* opt, float* results, uint32_t* steps);
int rt_terrain_trace_surface_device(rt_compute cs, const void* rays_device, int n,
                                    const rt_surface_options* opt, void* results_device, void* steps_device);

/* ---- shaded queries (ABI 9, additive; no reference counterpart) ----
 * What a ray of the host's own LOOKS like: terrain colour, sun shadow, fog and sky exactly as a frame shows them.
 * Reflection and light probes, cube maps and panoramas, fisheye or off-axis cameras, the colour of a picked
 * point.  For ray i with origin_i and dir_i and one eye E per call the result is what tracescreen.hlsl:16-48
 * computes for one sample:
 *     pdn   = normalize(dir_i)
 *     rr    = traceRay(origin_i, t_min, t_max, stepmod, dir_i, calcfog ON, skiprefine OFF)       (cap: max_steps)
 *     scat  = getRayleighMieColor(pdn);  skyAmount = saturate((rr.pd.w * 0.0005)^2)
 *     hit   = rr.density > 0
 *     hit : n = getNormal(float4(rr.pd.xyz, rr.density))
 *           color = getColor(rr.pd.xyz, n, pdn, rr.pd.w)     (its shadow ray: traceRay(p, 0.4, 100,
 *                                                    precision(rr.pd.w), SunDirection, fog ON, skiprefine ON))
 *           color = lerp(lerp(color, rr.fcolord.rgb, rr.fcolord.w), scat.rayleigh, skyAmount)
 *     miss: sky = scat.mie + scat.rayleigh + getSpaceColor(pdn)
 *           color = lerp(lerp(sky, rr.fcolord.rgb, rr.fcolord.w), sky, skyAmount)
 *     result_i = { float4(color.rgb, rr.pd.w), float4(rr.pd.xyz, rr.density) }     color NOT saturated
 *     rgba8_i  = unorm8(saturate(color.rgb)), alpha 255       what a frame stores for a pixel of one sample
 *     steps_i  = { primary iterations, shadow iterations (0 for a miss) }
 *   dir   is used as given, as in the other queries: its LENGTH enters the first step (tracing.hlsl:54).
 *   E     replaces Eye wherever the shaders read it: the density's level of detail, getNormal's eps and the sky.
 *         Without RT_RAYS_EYE it is the compute's current Eye variable.  One per call.
 *   SunDirection, RECORDING and the landscape constants come from the compute, which must be a TRACESCREEN
 *         compute (camerarays has no SunDirection).  Its AA_SAMPLES, RT_MAX_STEPS and RT_AO_SAMPLES macros are
 *         ignored: one sample per ray, the option block's max_steps is the cap.
 *   NO ambient occlusion: the result is the sample before any AO factor, whatever the compute was built with
 *         (rt_terrain_shade_points gives the AO factor at a point, e.g. at result_i's pd.xyz).
 *         Nor a segment shape or a sun per ray; the option block's size field leaves room for them later.
 *   A zero dir or non-finite inputs give unspecified results; the kernel still ends.
 * The option block is rt_surface_options, parsed as for the surface queries: RT_RAYS_EYE, RT_SURFACE_PARAMS
 *   (t_min, t_max, stepmod, max_steps; defaults 0.01, 5000, 1, unbounded), RT_SURFACE_RAY_RANGE and max_blocks
 *   mean what they mean there.  There is one kernel shape, the lanes': RT_RAYS_FORCE_LANES changes nothing and
 *   RT_RAYS_FORCE_SEGMENTS is RT_ERR_UNSUPPORTED.
 * rt_terrain_shade_rays: host arrays (origins, dirs: 3n floats; ranges: 2n floats or NULL; results: 8n floats or
 *   NULL; rgba8: n uint32 (R in the low byte) or NULL; steps: 2n uint32 or NULL); blocking.
 * rt_terrain_shade_rays_device: device arrays (rays n x 8 floats, 16-byte aligned; results n x 8 floats, 16-byte
 *   aligned, or NULL; rgba8 n uint32 or NULL; steps 2n uint32 or NULL), enqueued on the compute's device stream
 *   with no host synchronisation.
 * Both: at least one of results and rgba8.  n == 0 is RT_OK and launches nothing.  RT_ERR_INVALID: n < 0,
 *   n > 2^26, a NULL compute or rays, results and rgba8 both NULL, the option block's errors as above, a
 *   camerarays compute.  RT_ERR_STATE without texPerm2D bound, or with the fail-safe word set.  A query reads no
 *   frame state and changes none: it flushes no deferred frame, invalidates no ahead / fused prepass or captured
 *   graph, and uploads the constants it needs to a copy of its own, so it may run between any two renders. */
int rt_terrain_shade_rays(rt_compute screen_cs, const float* origins, const float* dirs, const float* ranges, int n,
                          const rt_surface_options* opt, float* results, uint32_t* rgba8, uint32_t* steps);
int rt_terrain_shade_rays_device(rt_compute screen_cs, const void* rays_device, int n, const rt_surface_options* opt,
                                 void* results_device, void* rgba8_device, void* steps_device);

/* ---- point shading (ABI 9, additive; no reference counterpart) ----
 * What the terrain LOOKS like at a point the host already holds, without a view ray: its colour with the sun's
 * shadow, and how occluded it is.  Vertex colours and AO for an extracted mesh (rt_terrain_extract_mesh's vertices
 * and normals arrays are read as they are), light and AO probes, the tint of a decal or an object at an
 * rt_terrain_trace_surface hit, per-vertex AO for any mesh laid on the terrain.  For point i with position p_i and
 * normal n_i, one eye E per call and K = ao_samples, the result is what a frame computes for a pixel whose primary
 * ray ended at p_i, before the view ray's fog and sky blends:
 *     dist   = length(p_i - E);  pdn = (p_i - E) * rcp(dist)                            (normalize(p_i - E))
 *     color  = getColor(p_i, n_i, pdn, dist)            (color.hlsl of the landscape; its shadow ray: traceRay(p_i,
 *                                               0.4, 100, precision(dist), SunDirection, fog ON, skiprefine ON))
 *     K > 0 : for k = 0..K-1:  rr_k = traceRay(p_i, 0.4, 25, precision(dist), ao_dir(n_i, px = i, py = seed, a = 0, k),
 *                                              fog OFF, skiprefine ON);  occ += rr_k.density > 0
 *             ao = fma(-0.6, occ * rcp(K), 1)                          (the AO extension of the frames, unchanged)
 *     K == 0: ao = 1
 *     result_i = float4(color.rgb, ao)                 color NOT saturated and NOT multiplied by ao
 *     rgba8_i  = unorm8(saturate(color.rgb) * ao), alpha 255        a frame's rule: ao multiplies the saturated colour
 *     steps_i  = { shadow iterations, sum of the K AO rays' iterations }
 *   E     replaces Eye in the density's level of detail, as in every query, and is the viewpoint dist and pdn come
 *         from: the specular term, simple's colour detail, and the shadow and AO rays' precision.  Without
 *         RT_RAYS_EYE it is the compute's current Eye variable.  One per call.  p_i == E gives unspecified results;
 *         the kernel still ends.
 *   n_i   is used as given (a frame passes getNormal's unit normal).  A zero or non-finite normal, or a non-finite
 *         point, gives unspecified results; the kernel still ends.
 *   The AO directions are a hash of (i, seed, k): the same call gives the same bits, and another seed decorrelates
 *         two bakes.  i is the point's index in the call.
 *   SunDirection, RECORDING and the landscape constants come from the compute, which must be a TRACESCREEN compute
 *         (camerarays has no SunDirection).  Its RT_AO_SAMPLES, AA_SAMPLES and RT_MAX_STEPS macros are ignored.
 * Layouts: points are n x 4 floats x y z _ and normals n x 4 floats nx ny nz _, the spare words ignored: the field
 *   queries' packed points and RT_FIELD_NORMAL results, and rt_terrain_extract_mesh's vertices (spare word: the cell
 *   index) and normals (spare word: the density).  results n x 4 floats; rgba8 n uint32 (R in the low byte); steps
 *   2n uint32.
 * rt_point_options (opt may be NULL: all defaults, K = 0 and seed 0): size = sizeof(rt_point_options) of the
 *   caller's header (later versions append fields; the first version is 32 bytes); flags: RT_RAYS_EYE, every other
 *   bit is an error; max_blocks caps the persistent grid (0: every CU less rt_device_reserve_cus); ao_samples 0..16
 *   (ao_dir packs k into 4 bits); seed any uint32.
 * rt_terrain_shade_points: host arrays (points, normals: 3n floats each; results: 4n floats or NULL; rgba8: n
 *   uint32 or NULL; steps: 2n uint32 or NULL); blocking.
 * rt_terrain_shade_points_device: device arrays (points, normals and results 16-byte aligned; results, rgba8 and
 *   steps may be NULL), enqueued on the compute's device stream with no host synchronisation: order other streams
 *   with rt_device_wait_event / rt_device_record_event.
 * Both: at least one of results and rgba8.  n == 0 is RT_OK and launches nothing.  RT_ERR_INVALID: n < 0,
 *   n > 2^26, a NULL compute, points or normals, results and rgba8 both NULL, opt->size below 32, unknown flags,
 *   ao_samples above 16, a camerarays compute.  RT_ERR_STATE without texPerm2D bound, or with the fail-safe word
 *   set.  A query reads no frame state and changes none: it flushes no deferred frame, invalidates no ahead / fused
 *   prepass or captured graph, and uploads the constants it needs to a copy of its own, so it may run between any
 *   two renders.
 * Out of scope: the view ray's fog and sky blends (rt_terrain_shade_rays has them); a sun or an eye per point;
 *   getNormal inside the call (pass rt_terrain_sample_field's RT_FIELD_NORMAL results or the mesh's normals); a
 *   caller-chosen AO range or strength. */
typedef struct {
    uint32_t size;
    uint32_t flags;
    float eye[3];
    uint32_t max_blocks;
    uint32_t ao_samples;
    uint32_t seed;
} rt_point_options;
int rt_terrain_shade_points(rt_compute screen_cs, const float* points, const float* normals, int n,
                            const rt_point_options* opt, float* results, uint32_t* rgba8, uint32_t* steps);
int rt_terrain_shade_points_device(rt_compute screen_cs, const void* points_device, const void* normals_device, int n,
                                   const rt_point_options* opt, void* results_device, void* rgba8_device,
                                   void* steps_device);

/* ---- field queries (ABI 9, additive; no reference counterpart) ----
 * What the terrain IS at a place, without a ray: the density field itself (getDensity, > 0 inside) and its normal.
 * Voxel and occupancy grids for collision and path finding, density volumes for mesh export or a slice through the
 * world, inside/outside tests for spawn points and buoyancy.  For point p and one eye E per call:
 *     d        = getDensity(p)                                                    (terrain.hlsl of the landscape)
 *     result_i = d                                                                one float a point
 *   with RT_FIELD_NORMAL:
 *     n        = getNormal(float4(p, d))                                          (tracing.hlsl:107-116)
 *     result_i = float4(n, d)                                                     16-byte aligned in the device forms
 *   E     replaces Eye in getDensity (nomadplains' octave count) and in getNormal's eps = 0.005 |p - E|.  Without
 *         RT_RAYS_EYE it is the compute's current Eye variable.  One per call.
 *   The normal is computed for EVERY point, inside or outside (the gradient direction of the field, as the shaders
 *         take it: one-sided differences over eps).  Where all three differences are zero (p == E is one case) the
 *         normal is unspecified.  Non-finite points give unspecified results.
 * A lattice (rt_lattice) is dims[0] x dims[1] x dims[2] = nx x ny x nz points computed on the device: point
 *   (ix, iy, iz) has the coordinate fmaf((float)i, spacing, origin) on each axis (ONE rounding) and the result index
 *   (iz * ny + iy) * nx + ix.  Its results are bit for bit the point form's for the same coordinates.  A spacing may
 *   be negative or zero.
 *   occupancy (optional) is one bit per lattice point, d > 0 (the hit test of tracescreen.hlsl:29), packed in
 *   uint32 words: ceil(nx / 32) words per (iy, iz) row, word index (iz * ny + iy) * ceil(nx / 32) + ix / 32, bit
 *   ix % 32; the padding bits of a row's last word are 0.  At least one of results and occupancy must be given;
 *   occupancy alone computes no normal.
 * rt_field_options (opt may be NULL: all defaults): size = sizeof(rt_field_options) of the caller's header (later
 *   versions append fields); flags: RT_RAYS_EYE (as above) and RT_FIELD_NORMAL, every other bit is an error;
 *   max_blocks caps the grid (0: every CU less rt_device_reserve_cus).
 * rt_terrain_sample_field: host arrays (points: 3n floats x y z; results: n floats, or 4n with RT_FIELD_NORMAL);
 *   blocking.
 * rt_terrain_sample_field_device: device arrays (points n x 4 floats x y z _, 16-byte aligned, the spare word
 *   ignored; results n floats, or n x 4 floats 16-byte aligned), enqueued on the compute's device stream with no
 *   host synchronisation: order other streams with rt_device_wait_event / rt_device_record_event.
 * rt_terrain_sample_lattice / _device: the same two forms for a lattice (results nx ny nz floats, or x 4; occupancy
 *   ceil(nx / 32) ny nz uint32); no coordinates are uploaded or read.
 * All: n == 0 or a dims product of 0 is RT_OK and launches nothing.  RT_ERR_INVALID: n < 0, n or nx ny nz above
 *   2^26, a dim above 4096, a non-finite origin or spacing, a NULL compute, lattice or required array, results and
 *   occupancy both NULL, opt->size below the first version (24), unknown flags.  RT_ERR_STATE without texPerm2D
 *   bound, or with the fail-safe word set.  Either kind of compute.  A query reads no frame state and changes none:
 *   it flushes no deferred frame, invalidates no ahead / fused prepass or captured graph, and uploads the constants
 *   it needs to a copy of its own, so it may run between any two renders.
 * Mesh extraction over a lattice is rt_terrain_extract_mesh below.  Out of scope: the fog field (getFog); an eye
 *   per point; a caller-chosen eps for the normal; finite differences between lattice neighbours (the normal is
 *   getNormal's, three more density samples a point). */
enum { RT_FIELD_NORMAL = 32 };
typedef struct {
    uint32_t size;
    uint32_t flags;
    float eye[3];
    uint32_t max_blocks;
} rt_field_options;
typedef struct {
    float origin[3];
    float spacing[3];
    uint32_t dims[3]; /* nx, ny, nz */
} rt_lattice;
int rt_terrain_sample_field(rt_compute cs, const float* points, int n, const rt_field_options* opt, float* results);
int rt_terrain_sample_field_device(rt_compute cs, const void* points_device, int n, const rt_field_options* opt,
                                   void* results_device);
int rt_terrain_sample_lattice(rt_compute cs, const rt_lattice* lat, const rt_field_options* opt, float* results,
                              uint32_t* occupancy);
int rt_terrain_sample_lattice_device(rt_compute cs, const rt_lattice* lat, const rt_field_options* opt,
                                     void* results_device, void* occupancy_device);

/* ---- mesh extraction (ABI 9, additive; no reference counterpart) ----
 * The terrain's surface inside a lattice as an indexed triangle mesh, extracted on the device by surface nets: a
 * collision or navigation mesh, an export, a proxy for rasterised LOD.  Only the cells that carry surface come back.
 * The lattice is an rt_lattice exactly as rt_terrain_sample_lattice reads it; D(ix, iy, iz) is its density and a
 *   point is inside when D > 0 (the occupancy test).
 * Cells are (cx, cy, cz) with 0 <= c < n - 1 per axis, cell index (cz (ny - 1) + cy) (nx - 1) + cx.  Corner k of a
 *   cell has bit 0 = +x, bit 1 = +y, bit 2 = +z.  A cell is ACTIVE when its 8 corners are not all inside and not all
 *   outside.  A lattice with a dim below 2 has no cells: both counts are 0 and nothing else is written.
 * Edges: a cell has 12, in this order: 0-3 run along x with (ky, kz) = (0,0) (1,0) (0,1) (1,1); 4-7 along y with
 *   (kx, kz) in the same pattern; 8-11 along z with (kx, ky) in the same pattern.  An edge from its lower endpoint a to
 *   its upper endpoint b CROSSES when inside(a) != inside(b).
 * The vertex of an active cell: for each crossing edge t = d_a / (d_a - d_b) (one IEEE subtract, one correctly
 *   rounded divide); the crossing's local coordinate is t on the edge's axis and the 0 / 1 corner offsets on the
 *   other two.  The local vertex l is the float32 sum (from 0) of the crossings' local coordinates in edge order,
 *   divided (correctly rounded) by the float crossing count; no contraction anywhere.  The world coordinate per axis
 *   is fmaf((float)c + l, spacing, origin): the inner add is one float32 rounding, the fma one.  Every step is
 *   monotone, so a vertex lies inside its cell's closed box, exactly, in lattice terms.
 * Vertices are ordered by ascending cell index.  A vertex is 4 words: x y z and the cell index as uint32 bits.
 * normals (optional): entry i is float4(getNormal(float4(p_i, d_i)), d_i) with d_i = getDensity(p_i): bit for bit
 *   what rt_terrain_sample_field with RT_FIELD_NORMAL returns for the vertex positions, with the same eye rule
 *   (RT_RAYS_EYE).
 * Faces: take a cell c and an axis a.  The lattice edge from c's corner 0 along a is INTERIOR when c's other two
 *   coordinates are >= 1.  Every interior crossing edge gives one quad over the vertices of the four cells around
 *   it; quads are ordered by ascending owning cell c, then axis x, y, z.  With (u, v) the next two axes in cyclic
 *   order after a -- (y, z) for x, (z, x) for y, (x, y) for z -- the four cells are A = c - u - v, B = c - v, C = c,
 *   D = c - u.  A lower endpoint that is inside gives the triangles (A, B, C), (A, C, D); one that is outside gives
 *   (A, D, C), (A, C, B): geometric normals point out of the terrain, towards decreasing density, as getNormal's do.
 *   A triangle is 3 uint32 vertex indices; triangles 2q and 2q + 1 belong to quad q.  The mesh is open at the
 *   lattice's boundary.
 * Non-finite densities give unspecified output; the kernels still end.
 * counts[0..1] always receive the mesh's FULL vertex and triangle counts.  The first min(count, capacity) entries of
 *   vertices (4 words each), normals (4 floats each, may be NULL: no normal pass runs) and triangles (3 uint32 each)
 *   are written and nothing beyond them; a truncated call's arrays are a prefix of the full call's.  A capacity of 0
 *   with a NULL array is a counting call.
 * opt is an rt_field_options parsed as for the lattice (RT_RAYS_EYE, max_blocks; RT_FIELD_NORMAL is ignored).
 * rt_terrain_mesh_scratch_bytes: the device form's scratch block for the lattice (its densities, occupancy words,
 *   mask words and offsets); 0 for an invalid lattice or one without cells.
 * rt_terrain_extract_mesh: host arrays; blocking; the density is computed on the device, nothing but the counts
 *   and the written prefixes is downloaded.
 * rt_terrain_extract_mesh_device: device arrays (scratch, vertices and normals 16-byte aligned), enqueued on the
 *   compute's device stream; it allocates nothing and never synchronises the host: the counts stay on the device
 *   and every later pass reads them there.  RT_ERR_INVALID when scratch_bytes is below
 *   rt_terrain_mesh_scratch_bytes(lat).
 * Both: RT_ERR_INVALID for the lattice's and the option block's errors (as rt_terrain_sample_lattice), a NULL
 *   compute, lattice or counts, a capacity above 0 with a NULL array.  RT_ERR_STATE without texPerm2D bound, or with
 *   the fail-safe word set.  Either kind of compute.  An extraction reads no frame state and changes none: it flushes
 *   no deferred frame and invalidates no ahead / fused prepass or captured graph, so it may run between any two
 *   renders. */
size_t rt_terrain_mesh_scratch_bytes(const rt_lattice* lat);
int rt_terrain_extract_mesh(rt_compute cs, const rt_lattice* lat, const rt_field_options* opt, float* vertices,
                            float* normals, uint32_t max_vertices, uint32_t* triangles, uint32_t max_triangles,
                            uint32_t counts[2]);
int rt_terrain_extract_mesh_device(rt_compute cs, const rt_lattice* lat, const rt_field_options* opt,
                                   void* scratch_device, size_t scratch_bytes, void* vertices_device,
                                   void* normals_device, uint32_t max_vertices, void* triangles_device,
                                   uint32_t max_triangles, void* counts_device);

/* ---- distance fields (ABI 9, additive; no reference counterpart) ----
 * How far every point of a lattice is from the terrain's surface, in lattice terms and exactly: the clearance of an
 * agent of radius r in an occupancy grid, a sphere's collision test, a safe spawn volume, a navigation cost.  The
 * density is no distance (a noise sum with terraces and a pow); this is one, formed on the device from the
 * occupancy bits alone, so only the field the caller asks for comes back.
 * The lattice is an rt_lattice exactly as rt_terrain_sample_lattice reads it.  A point is INSIDE when its occupancy
 *   bit is set, which for the terrain's own occupancy means getDensity > 0.  For the lattice point p = (ix, iy, iz):
 *     d2(p) = min over the lattice points q of the same lattice with inside(q) != inside(p)
 *             of (qx-ix)^2 + (qy-iy)^2 + (qz-iz)^2                     uint32, in cells^2, exact
 *           = RT_DIST_FAR  when there is no such q (the lattice is all inside or all outside)
 *                          or, with max_cells = R > 0, when that minimum exceeds R * R
 *     distance(p) = s * (sqrt((float)d2) * |spacing[0]|), s = +1 outside, -1 inside: one conversion, one correctly
 *                   rounded square root and one multiply, each rounded to nearest; +-INFINITY for RT_DIST_FAR
 *   both at index (iz * ny + iy) * nx + ix, as the lattice's results.  The largest finite d2 is 3 * 4095^2 < 2^26, and
 *   the far value is never added to, so no sum overflows.  d2 is at least 1.
 * distance is positive in free space and negative in the ground.  The surface crosses the segment from p to its
 *   nearest q, so |distance| is an UPPER bound of the true clearance, tight to less than one cell diagonal
 *   (sqrt(3) |spacing|): a caller that needs a safe radius subtracts that.
 * distance is defined for an isotropic lattice only, |spacing[0]| == |spacing[1]| == |spacing[2]| != 0 (the signs
 *   may differ); otherwise asking for it is RT_ERR_INVALID.  d2 is a lattice metric and defined for any spacing,
 *   0 and negative included.
 * occupancy_in NULL: the terrain's own occupancy, computed on the device as rt_terrain_sample_lattice computes its
 *   occupancy words (RT_RAYS_EYE and max_blocks as there, either kind of compute), into the scratch block.
 * occupancy_in not NULL: the caller's words in rt_terrain_sample_lattice's layout, ceil(nx / 32) words per point row,
 *   bit ix % 32 of word ix / 32; the terrain is not evaluated.  The padding bits of a row's last word are ignored
 *   whatever they hold.  This is the form for edited voxel grids.
 * opt (NULL: the defaults) is an rt_distance_options: size >= 28, flags RT_RAYS_EYE or 0, eye, max_blocks (the cap
 *   of every pass's grid, 0: none), max_cells (0: unbounded).  max_cells bounds the work as well as the answer: a
 *   lattice that is all inside or all outside, or has wide regions far from any surface, costs a scan of whole
 *   columns without it.
 * At least one of d2 and distance is required; a NULL one is not written.
 * rt_terrain_distance_scratch_bytes: the device form's scratch block for the lattice: its occupancy words, one
 *   word a point for the x pass and two for the y pass, each part rounded up to 16 bytes; 0 for an invalid lattice
 *   or one without points.
 * rt_terrain_distance_field: host arrays; blocking; nothing but the arrays asked for is downloaded.
 * rt_terrain_distance_field_device: device arrays (4-byte aligned), enqueued on the compute's device stream; it
 *   allocates nothing and never synchronises the host.  RT_ERR_INVALID when scratch_bytes is below
 *   rt_terrain_distance_scratch_bytes(lat), and nothing is written.
 * Both: RT_ERR_INVALID for the lattice's errors (as rt_terrain_sample_lattice), a NULL compute or lattice,
 *   opt->size < 28, flags other than RT_RAYS_EYE, distance on an anisotropic or zero spacing, d2 and distance both
 *   NULL.  RT_ERR_STATE without texPerm2D bound, or with the fail-safe word set.  A dims product of 0 is RT_OK and
 *   launches nothing.  A distance field reads no frame state and changes none: it flushes no deferred frame and
 *   invalidates no ahead / fused prepass or captured graph, so it may run between any two renders.
 * Out of scope: sub-cell refinement of the distance from the densities; anisotropic metric distances; trilinear
 *   sampling of the field at free points; a sphere-sweep query; an eye per point. */
#define RT_DIST_FAR 0xFFFFFFFFu
typedef struct { uint32_t size, flags; float eye[3]; uint32_t max_blocks; uint32_t max_cells; } rt_distance_options; /* 28 bytes, v1 */
size_t rt_terrain_distance_scratch_bytes(const rt_lattice* lat);
int rt_terrain_distance_field(rt_compute cs, const rt_lattice* lat, const rt_distance_options* opt,
                              const uint32_t* occupancy_in, uint32_t* d2, float* distance);
int rt_terrain_distance_field_device(rt_compute cs, const rt_lattice* lat, const rt_distance_options* opt,
                                     const void* occupancy_in_device, void* scratch_device, size_t scratch_bytes,
                                     void* d2_device, void* distance_device);

/* ---- path fields (ABI 9, additive; no reference counterpart) ----
 * The step from "where may I stand" to "how do I get there": for every point of a lattice the cost of the cheapest
 * path from a set of seed points through the passable points, and optionally the move that starts that path back
 * to a seed (a flow field, what a crowd steers by).  Formed on the device from the occupancy bits; a clearance uses
 * the distance passes above.  The answer is unique: it is the least fixed point of an integer relaxation, so the
 * kernels may relax in any order and still equal a Dijkstra search bit for bit.
 * The lattice is an rt_lattice exactly as rt_terrain_sample_lattice reads it; point index and occupancy word layout
 *   as there.
 * Blocked and passable.  A point is BLOCKED when its occupancy bit is set.
 *   occupancy_in NULL: the terrain's own occupancy, computed on the device into the scratch block as the distance
 *     field does it (RT_RAYS_EYE and max_blocks as there, either kind of compute).
 *   occupancy_in not NULL: the caller's words; the terrain is not evaluated.  The padding bits of a row's last word
 *     are ignored whatever they hold.
 *   clearance_cells = R > 0: a point is PASSABLE iff it is not blocked and its d2 is greater than R * R, d2 exactly
 *     rt_terrain_distance_field's (the squared distance of an outside point to the nearest blocked point; far when
 *     the lattice has none).  R == 0: passable iff not blocked.
 * Moves.  The 26 neighbours.  Move code c = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1), 0..26, 13 is "stay".  Weight w(c)
 *   is 3 for a face move, 4 for an edge move, 5 for a corner move: the 3-4-5 chamfer, in thirds of a cell.  A move is
 *   allowed when both of its ends are passable lattice points.
 * Seeds.  seeds[0 .. n_seeds) are linear point indices, (iz * ny + iy) * nx + ix.  Duplicates are allowed.  A seed
 *   that is blocked or impassable contributes nothing.  A seed at or beyond nx * ny * nz is RT_ERR_INVALID in the
 *   host form; the device form cannot check, so its kernel skips such a seed.
 * Cost.
 *     cost(p) = min over seeds s and move sequences from s to p of the sum of w      uint32, exact
 *             = 0 at a passable seed
 *             = RT_PATH_FAR where p is impassable, unreachable, or, with max_cost = M > 0, where that minimum
 *               exceeds M
 *   max_cost bounds the work as well as the answer: a candidate above M is never stored or propagated.  That is
 *   still exact, because every prefix of a cheapest path is cheaper than the whole path.  The largest finite cost is
 *   below 5 * 2^26 (a path visits a point once, and a lattice has 2^26 points at most), and the far value is never
 *   added to, so no sum overflows.
 * Flow (optional, uint8 a point).  The smallest move code c for which the neighbour q = p + move(c) has
 *   cost(q) + w(c) == cost(p): the first step of a cheapest path back to a seed.  13 at a point of cost 0,
 *   RT_PATH_NONE where the cost is far.  The flow is determined by cost alone.  (In an unconverged field a point
 *   whose neighbours have fallen since it was written may have no such c: RT_PATH_NONE.)
 * World length.  cost * |spacing| / 3 on an isotropic lattice.  In open space the chamfer length of the offset
 *   (a, b, c), a >= b >= c >= 0, is a + (b + c) / 3; against the Euclidean sqrt(a^2 + b^2 + c^2) it lies between
 *   -5.7% (at (1, 1, 0): 4/3 for sqrt 2) and +10.6% (at (1, 1/3, 1/3): 11/9 for sqrt(11)/3).
 * Status (4 uint32): [0] 1 when the relaxation converged, else 0; [1] sweeps that did work; [2] points with a
 *   finite cost; [3] 0.  When [0] == 0 every written cost is an upper bound of the true cost (the cost of a real
 *   path), and the cost of a passable seed is 0.
 * opt (NULL: the defaults) is an rt_path_options: size >= 36, flags RT_RAYS_EYE or 0, eye, max_blocks (the cap of
 *   every pass's grid, 0: none), clearance_cells (<= 4095), max_cost (0: unbounded), max_sweeps.
 * cost is required; flow may be NULL; status may be NULL in the host form and is required in the device form.
 *   n_seeds is 1 .. 2^26.
 * rt_terrain_path_scratch_bytes: the device form's scratch block for the lattice and opt->clearance_cells: the
 *   occupancy words; with a clearance the distance scratch and a word a point for d2; the passable words; two tile
 *   flag arrays (a word a tile of 32 x 4 x 4 points each); 64 bytes of counters; each part rounded up to 16 bytes.
 *   0 for an invalid lattice or option block, or a lattice without points.
 * rt_terrain_path_field: host arrays; blocking.  max_sweeps == 0 sweeps until converged; that ends, because every
 *   working sweep lowers at least one non-negative integer.  A positive max_sweeps stops there and returns RT_OK
 *   with status[0] == 0 if the field has not converged.  Nothing but the arrays asked for is downloaded.
 * rt_terrain_path_field_device: device arrays (4-byte aligned but flow), enqueued on the compute's device stream; it
 *   allocates nothing and never synchronises the host.  max_sweeps must be 1..4096: it enqueues an initialisation,
 *   exactly that many sweep launches and a finish pass; a sweep launch that finds nothing active ends at once.
 *   With H the greatest number of moves on any cheapest path, max_sweeps >= H + 2 converges; every move costs at
 *   least 3, so H <= (largest finite cost) / 3.
 * Both: RT_ERR_INVALID for the lattice's errors (as rt_terrain_sample_lattice), a NULL compute or lattice,
 *   opt->size < 36, flags other than RT_RAYS_EYE, clearance_cells > 4095, n_seeds outside 1..2^26, NULL seeds or
 *   cost, and in the device form a NULL status, max_sweeps outside 1..4096 or a scratch block that is NULL or below
 *   rt_terrain_path_scratch_bytes; nothing is written then.  RT_ERR_STATE as for the distance field (texPerm2D bound
 *   and the fail-safe word clear, with a given occupancy too).  A dims product of 0 is RT_OK and launches nothing.
 *   Like every query it reads no frame state and changes none.
 * Out of scope: continuing an unconverged field; per-seed start costs and per-cell traversal weights; a rule
 *   against diagonal moves between two blocked cells (a clearance of one cell or more is the remedy);
 *   walkable-surface (gravity) navigation; sub-cell paths, any-angle smoothing, anisotropic weights, an eye per
 *   point. */
#define RT_PATH_FAR 0xFFFFFFFFu
#define RT_PATH_NONE 255u
typedef struct { uint32_t size, flags; float eye[3]; uint32_t max_blocks, clearance_cells, max_cost, max_sweeps; } rt_path_options; /* 36 bytes, v1 */
size_t rt_terrain_path_scratch_bytes(const rt_lattice* lat, const rt_path_options* opt);
int rt_terrain_path_field(rt_compute cs, const rt_lattice* lat, const rt_path_options* opt, const uint32_t* occupancy_in,
                          const uint32_t* seeds, uint32_t n_seeds, uint32_t* cost, uint8_t* flow, uint32_t status[4]);
int rt_terrain_path_field_device(rt_compute cs, const rt_lattice* lat, const rt_path_options* opt, const void* occupancy_in_device,
                                 const void* seeds_device, uint32_t n_seeds, void* scratch_device, size_t scratch_bytes,
                                 void* cost_device, void* flow_device, void* status_device);

/* ---- visibility fields (ABI 9, additive; no reference counterpart) ----
 * What can be seen from here, and what is lit: for every point of a lattice one bit per observer, set when the
 * straight line between them is free of blocked cells.  Cover and lookout points, sensor and tower placement, a
 * viewshed, the sun exposure of a whole volume.  Formed on the device from the occupancy bits alone, in integers, so
 * the answer is exact; rt_terrain_trace_rays with ranges answers the same for one pair of points at sub-cell
 * precision.
 * The lattice is an rt_lattice exactly as rt_terrain_sample_lattice reads it; point index and occupancy word layout
 *   as there.  A point is BLOCKED when its occupancy bit is set; the padding bits of a row's last word are ignored
 *   whatever they hold.  The CELL of a lattice point c is the open unit box round it, |x - c| < 1/2 on each axis, in
 *   lattice coordinates.
 * Observers.  observers[0 .. n_observers), n_observers in 1..32, four int32 each: x, y, z, kind.
 *   kind 0, a point observer: the lattice point (x, y, z), which must be a point of the lattice.
 *   kind 1, a directional observer: the integer direction u = (x, y, z) TOWARDS the light (the sense of
 *     SunDirection, along which the shadow ray travels); each |component| <= 4095, not all 0.
 *   An invalid observer (another kind, a point off the lattice, a zero direction, a component out of range) is
 *   RT_ERR_INVALID in the host form; the device form cannot check, so its kernel treats such an observer as seeing
 *   nothing: its bit is 0 everywhere.
 * Line of sight to a point observer o from the point p.  The cells BETWEEN them are the lattice points c, other than
 *   o and p, whose cell meets the open segment from o to p: there is a t in (0, 1) with |o + t (p - o) - c| < 1/2
 *   on all three axes.  Equivalently, as a walk: with d = p - o, axis i crosses a cell boundary at
 *   t = (2 k + 1) / (2 |d_i|), k = 0 .. |d_i| - 1; take the distinct crossing times in ascending order; at each,
 *   every axis that crosses then steps at once by sign(d_i) (a segment through a box edge or corner enters the
 *   diagonal cell directly and does not visit the cells it only touches); the positions after each event but the
 *   last are the cells between.  p SEES o iff no cell between is blocked.
 *     The two endpoints are not tested: a blocked surface point that is met first is seen, a blocked observer cell
 *     changes nothing, and p == o is seen.  The rule is symmetric in o and p.  Everything is decided in 32-bit
 *     integers: (2 k + 1) / |d_i| against (2 j + 1) / |d_j| is (2 k + 1) |d_j| against (2 j + 1) |d_i|, both below
 *     8191 * 4095 < 2^25.
 * Line of sight to a directional observer u from p.  The same walk along p + t u for t > 0, crossings at
 *   t = (2 k + 1) / (2 |u_i|), k = 0, 1, ... without end.  It stops at the first event whose position is not a point
 *   of the lattice: p is LIT when the walk leaves the lattice without having met a blocked cell.  p itself is not
 *   tested.
 * max_range = R > 0.  Point observer: the bit is 0 when |p - o|^2 > R^2, and no walk runs.  Directional observer:
 *   the walk also ends, lit, at the first visited cell c with |c - p|^2 > R^2; shadow casters beyond R do not
 *   count.  R == 0: unbounded.  R bounds the work as well as the answer.  R > 2 * 4095 = 8190 would equal unbounded
 *   (no two lattice points are farther apart) and is RT_ERR_INVALID.
 * Result.  mask, a uint32 a point at index (iz * ny + iy) * nx + ix: bit k is 1 iff the point sees observer k; bits
 *   n_observers .. 31 are 0.
 * Status (4 uint32, may be NULL in both forms): [0] points with a non-zero mask; [1] the sum of the masks' set bits
 *   (2^26 * 32 = 2^31 at most); [2] valid observers; [3] 0.
 * occupancy_in NULL: the terrain's own occupancy, computed on the device into the scratch block as the distance
 *   field does it (RT_RAYS_EYE and max_blocks as there, either kind of compute).
 * occupancy_in not NULL: the caller's words in rt_terrain_sample_lattice's layout; the terrain is not evaluated.
 * opt (NULL: the defaults) is an rt_visibility_options: size >= 28, flags RT_RAYS_EYE or 0, eye, max_blocks (the cap
 *   of every pass's grid, 0: none), max_range (0: unbounded, 8190 at most).
 * rt_terrain_visibility_scratch_bytes: the device form's scratch block for the lattice: its occupancy words and 64
 *   bytes of counters, each part rounded up to 16 bytes; 0 for an invalid lattice or one without points.
 * rt_terrain_visibility_field: host arrays; blocking.  It uploads the observers and any given occupancy and
 *   downloads nothing but mask and status.
 * rt_terrain_visibility_field_device: device arrays (4-byte aligned), enqueued on the compute's device stream; it
 *   allocates nothing and never synchronises the host.  A NULL status_device is not written.
 * Both: RT_ERR_INVALID for the lattice's errors (as rt_terrain_sample_lattice), a NULL compute or lattice,
 *   opt->size < 28, flags other than RT_RAYS_EYE, max_range > 8190, n_observers outside 1..32, NULL observers or
 *   mask, in the host form an invalid observer, and in the device form a scratch block that is NULL or below
 *   rt_terrain_visibility_scratch_bytes; nothing is written then.  RT_ERR_STATE as for the distance field (texPerm2D
 *   bound and the fail-safe word clear, with a given occupancy too).  A dims product of 0 is RT_OK and launches
 *   nothing.  Like every query it reads no frame state and changes none.
 * Out of scope: sub-cell or density-refined sight lines (rt_terrain_trace_rays with ranges); observers off the
 *   lattice; more than 32 observers a call; soft visibility or a count of occluders; hierarchical or
 *   distance-field skipping; an eye per point. */
typedef struct { uint32_t size, flags; float eye[3]; uint32_t max_blocks; uint32_t max_range; } rt_visibility_options; /* 28 bytes, v1 */
size_t rt_terrain_visibility_scratch_bytes(const rt_lattice* lat);
int rt_terrain_visibility_field(rt_compute cs, const rt_lattice* lat, const rt_visibility_options* opt,
                                const uint32_t* occupancy_in, const int32_t* observers, uint32_t n_observers,
                                uint32_t* mask, uint32_t status[4]);
int rt_terrain_visibility_field_device(rt_compute cs, const rt_lattice* lat, const rt_visibility_options* opt,
                                       const void* occupancy_in_device, const void* observers_device, uint32_t n_observers,
                                       void* scratch_device, size_t scratch_bytes, void* mask_device, void* status_device);

/* ---- region fields (ABI 9, additive; no reference counterpart) ----
 * Which points belong together: for every point of a lattice the label of its connected region of free space, or
 * of the ground.  Is B reachable from A at all, which pockets are sealed off, which parts of the ground float, did a
 * dig cut a region in two.  Formed on the device from the occupancy bits by a union-find in a fixed number of
 * launches: no sweeps, and no sweep count for the caller to guess.  The answer is unique and independent of any
 * order of work.
 * The lattice is an rt_lattice exactly as rt_terrain_sample_lattice reads it; point index and occupancy word layout
 *   as there.  A point is BLOCKED when its occupancy bit is set; the padding bits of a row's last word are ignored
 *   whatever they hold.
 *   occupancy_in NULL: the terrain's own occupancy, computed on the device into the scratch block as the distance
 *     field does it (RT_RAYS_EYE and max_blocks as there, either kind of compute).
 *   occupancy_in not NULL: the caller's words; the terrain is not evaluated.
 * Members.  state 0 (free): a point is a MEMBER iff it is passable in rt_terrain_path_field's exact sense: not
 *     blocked, and with clearance_cells = R > 0 its d2 greater than R * R, d2 exactly rt_terrain_distance_field's
 *     (the unchanged distance passes at max_cells = R, into the scratch block).
 *   state 1 (solid): a point is a member iff it is blocked.  clearance_cells must be 0, else RT_ERR_INVALID.
 * Links.  connectivity 26 (0 means 26, the default) links two members that are one of the path field's 26 moves
 *   apart; connectivity 6 links by the six face moves only.  A REGION is a class of the members under the links'
 *   transitive closure.  For state 0 at connectivity 26 a region is therefore exactly a set of points with a finite
 *   rt_terrain_path_field cost from one another.  There is no rule against a diagonal link between two non-members:
 *   the path field's choice, with the same remedy (a clearance, or connectivity 6).
 * Label (uint32 a point at index (iz * ny + iy) * nx + ix, required).  The smallest linear point index of the point's
 *   region; RT_REGION_NONE at a non-member.  A point p is its region's root iff label[p] == p.
 * Size (uint32 a point, optional; NULL is not written).  The number of points of the point's region, the same value
 *   at every point of it; 0 at a non-member.
 * Status (4 uint32; may be NULL in both forms): [0] 1 when the labelling completed, 0 when a fail-safe bound ended a
 *   loop of a kernel (every loop there has a strictly decreasing integer as its variant and cannot reach its bound
 *   on a forest; the bound is there because a kernel must end whatever it reads); [1] the number of regions; [2] the
 *   number of member points; [3] the size of the largest region, 0 when there is none.
 * opt (NULL: the defaults) is an rt_region_options: size >= 36, flags RT_RAYS_EYE or 0, eye, max_blocks (the cap of
 *   every pass's grid, 0: none), clearance_cells (<= 4095), connectivity (0, 6 or 26), state (0 or 1).
 * rt_terrain_region_scratch_bytes: the device form's scratch block for the lattice and opt->clearance_cells: the
 *   occupancy words; with a clearance the distance scratch and a word a point for d2; the member words; a word a
 *   point for the region counts; 64 bytes of counters; each part rounded up to 16 bytes.  0 for an invalid lattice
 *   or option block, or a lattice without points.  The forest of the union-find is label itself and needs no part.
 * rt_terrain_region_field: host arrays; blocking.  It uploads any given occupancy and downloads nothing but the
 *   arrays asked for.
 * rt_terrain_region_field_device: device arrays (4-byte aligned), enqueued on the compute's device stream; it
 *   allocates nothing and never synchronises the host.  Three kernel launches after the occupancy and distance
 *   passes when neither size nor status is asked for, four otherwise, whatever the lattice holds.
 * Both: RT_ERR_INVALID for the lattice's errors (as rt_terrain_sample_lattice), a NULL compute, lattice or label,
 *   opt->size < 36, flags other than RT_RAYS_EYE, clearance_cells > 4095, connectivity not 0, 6 or 26, state > 1,
 *   state 1 with a clearance, and in the device form a scratch block that is NULL or below
 *   rt_terrain_region_scratch_bytes; nothing is written then.  RT_ERR_STATE as for the distance field (texPerm2D
 *   bound and the fail-safe word clear, with a given occupancy too).  A dims product of 0 is RT_OK and launches
 *   nothing.  Like every query it reads no frame state and changes none.
 * Out of scope: 18-connectivity; a compact, renumbered label set or a per-region table (bounding boxes, centroids);
 *   labelling both states in one call; regions across two lattices; incremental relabelling after an edit; gravity
 *   or walkable-surface regions. */
#define RT_REGION_NONE 0xFFFFFFFFu
typedef struct { uint32_t size, flags; float eye[3]; uint32_t max_blocks, clearance_cells, connectivity, state; } rt_region_options; /* 36 bytes, v1 */
size_t rt_terrain_region_scratch_bytes(const rt_lattice* lat, const rt_region_options* opt);
int rt_terrain_region_field(rt_compute cs, const rt_lattice* lat, const rt_region_options* opt, const uint32_t* occupancy_in,
                            uint32_t* label, uint32_t* size, uint32_t status[4]);
int rt_terrain_region_field_device(rt_compute cs, const rt_lattice* lat, const rt_region_options* opt,
                                   const void* occupancy_in_device, void* scratch_device, size_t scratch_bytes,
                                   void* label_device, void* size_device, void* status_device);

/* ---- diagnostics (primitive-level parity tests; no reference counterpart) ----
 * rt_debug_math: device evaluation of the numeric primitives of DESIGN.md §Numerics
 *   (op 0 exp2, 1 log2, 2 exp, 3 sin, 4 cos, 5 sqrt, 6 rcp, 7 rsqrt, 8 pow, 9 max,
 *   10 min, 11 pow for x >= 0, 13 the march's wave-tested pow for x >= 0: a wave is 64
 *   consecutive elements, 17 log2 for finite x >= 0); host arrays of n floats (b may be NULL for unary ops).
 *   op 12 sweeps the nomadplains octave-count estimate over the n floats whose bit
 *   patterns follow bits(a[0]) and writes 3 uint32 to out: unflagged estimates that differ
 *   from the exact count, flagged estimates, patterns swept.
 *   op 14 evaluates the trace kernel's sky-exit predicate (a primary ray that does not descend and whose
 *   next sample lies above the nomadplains ceiling, 256) for n triples (p.y, dir.y, dist) at a[3 i] (a: 3 n
 *   floats, b unused): out[i] = 1 or 0, and out[n] (out: n + 1 floats) = the ceiling the host computed for
 *   the product's octave constants, which must not exceed 256.
 *   op 15 evaluates the AO extension's ray direction for n normals at a[3 i] (a: 3 n
 *   floats, used as given) and n keys (px, py, AA sample, AO ray) at b[4 i] (b: 4 n uint32 passed as float bit
 *   patterns, required): out[3 i ..] (out: 3 n floats) = the direction.
 *   op 16 sweeps one element op over n inputs that the kernel makes itself (no input array is allocated or
 *   copied): a = 4 uint32 words passed as float bit patterns (start pattern, odd multiplier, element op, mask),
 *   b[0] = the second operand of the pow ops (b may be NULL for the unary ones); input i is the float with the
 *   bit pattern (start + i * multiplier mod 2^32) & mask (mask 0xffffffff, or 0x7fffffff for x >= 0), and out[i]
 *   (out: n floats) = the element op of it.  Element ops: 0-8, 11, 13 and 17; a wave is still 64 consecutive
 *   elements, so op 13 under a multiplier other than 1 sees mixed magnitudes in one wave.
 *   op 17 is log2 for finite x >= 0 (the shading's mip level), an ordinary unary op and an element op of 16.
 * rt_debug_sky_ceiling (host only, no device): the nomadplains density's ceiling for n_oct octave weights
 *   np_rcp[0 .. n_oct) and the pow exponent, in double to *ceiling (may be NULL); returns 1 if the host
 *   would allow the sky exit with them (ceiling <= 256, and the n_grad float4 gradients at grad, if not
 *   NULL, are all edge vectors), 0 if it would switch the exit off, < 0 for bad arguments.
 * rt_debug_noise: noise3d (density = 0, noise.hlsl:153-179) or the compute's landscape
 *   getDensity (density = 1) at n points (xyz interleaved), with the compute's
 *   current tables and constants; density = 2: nomadplains' steep noise noise3d(x, y, 0)
 *   (z ignored), 3: its short-integer-path variant (|x|, |y| < 8192). */
int rt_debug_math(rt_device dev, int op, const float* a, const float* b, float* out, int n);
int rt_debug_sky_ceiling(const float* np_rcp, int n_oct, float expo, const float* grad, int n_grad, double* ceiling);
int rt_debug_noise(rt_compute cs, const float* xyz, float* out, int n, int density);
/* rt_debug_sky (ABI 4): the sky of n view directions (xyz interleaved) with the compute's current
 *   constants (Eye, SunDirection) and tables: 7 floats per direction, getRayleighMieColor's
 *   (mie.rgb, rayleigh.rgb) (sky.hlsl:83-137) and getSpaceColor (sky.hlsl:26-36). */
int rt_debug_sky(rt_compute cs, const float* dirs, float* out, int n);
/* rt_debug_spin (ABI 7, scripts/batch_shard_sim.py's coupled transport model): one 64-thread workgroup
 *   on `hip_stream` that stores the GPU's 100 MHz clock at its start to *stamp_device (if not NULL), waits
 *   until *base_device + until_ticks (base_device a stamp an earlier spin stored; NULL: no wait), then
 *   spins `ticks` more -- the CU a collective's kernel holds while it waits for its peer and transfers. */
int rt_debug_spin(void* hip_stream, const unsigned long long* base_device, unsigned long long until_ticks,
                  unsigned long long ticks, unsigned long long* stamp_device);
/* rt_debug_defer_slot (ABI 9, tests): the device pointers of frame slot `slot` of an RT_DEVICE_DEFERRED device
 *   tracing K >= 2 frames to a launch (rt_device_defer_batch): its RGBA8 framebuffer, CameraResults (1024
 *   float4) and CellDistance (1024 float2), where a queued frame that was not a flush's last one wrote them.
 *   Frame i of a sequence that started with an empty queue takes slot i % (2K).  RT_ERR_INVALID for a slot
 *   never used. */
int rt_debug_defer_slot(rt_device dev, int slot, void** fb8, void** camera_results, void** cell_distance);

/* ---- IRecorder (Factories/IRecorder.h; RecorderWinAPI.cpp; RecorderFactory.cpp) ----
 * rt_recorder_create   <- RecorderFactory::construct(device, frameRate, fixedSpeed) + create():
 *                         attaches to the device (DeviceDirect3D::setRecorder, :229-232).  The
 *                         Media Foundation WMV sink (:80, "output.wmv") becomes a raw-video sink:
 *                         `path` (default "output.rgb32") receives the frames as raw
 *                         MFVideoFormat_RGB32 rows (B, G, R, 0), `path`.txt one line per sample
 *                         "frame sample_time duration" in 100 ns units (IMFSample time stamps).
 * rt_recorder_start    <- IRecorder::start + BeginWriting (:205-216)
 * rt_recorder_stop     <- IRecorder::stop + Finalize (:218-224); no start after it (as the sink writer)
 * rt_recorder_write    <- RecorderWinAPI::write(frame, stride) on host RGBA8 rows (:226-279)
 * rt_device_present    writes the frame to an attached, recording recorder (DeviceDirect3D.cpp:242-256),
 *                      with the swizzle on the GPU.
 * rt_recorder_set_frame_time: Timer::getConstant() the next sample uses when !fixed_speed (:264-269). */
int rt_recorder_create(rt_device dev, int frame_rate, int fixed_speed, const char* path, rt_recorder* out);
int rt_recorder_start(rt_recorder rec);
int rt_recorder_stop(rt_recorder rec);
int rt_recorder_is_recording(rt_recorder rec);
int rt_recorder_set_frame_time(rt_recorder rec, float seconds);
int rt_recorder_write(rt_recorder rec, const void* frame, int stride);
int rt_recorder_info(rt_recorder rec, unsigned long long* frames, unsigned long long* next_sample_time,
                     unsigned long long* frame_duration);
void rt_recorder_destroy(rt_recorder rec);
/* rt_recorder_set_async (ABI 9, additive; no reference counterpart): depth 1..8 gives the recorder a BGRX readback
 * ring of its own, 0 (the default) takes it away.  With a ring a recording rt_device_present submits a capture
 * instead of waiting for the frame (on an RT_DEVICE_DEFERRED device it launches nothing), keeps the frame's time
 * stamp input (rt_recorder_set_frame_time) with it, then writes the samples of the older captures that are ready,
 * in order; with the ring full it first waits for the oldest and writes it.  rt_recorder_stop, _info, _destroy,
 * this call and rt_device_destroy write everything captured first, so `frames` always counts the recording
 * presents, and `path` and `path`.txt hold the synchronous recorder's bytes.  A capture whose wait fails (the
 * fail-safe word) writes no sample; the call that drained it returns the error.  No writer thread. */
int rt_recorder_set_async(rt_recorder rec, int depth);

/* ---- VariableManager (Common/VariableManager.{h,cpp}; main.cpp:99 `-m`) ----
 * The live-tweak TCP protocol (VariableManager.cpp:76-83): on connect the server sends every
 * registered variable as [1][name len:1][name][type len:1][type][size:2 LE][data]; a clear sends
 * [2]; the client writes a variable as [name len:1][name][data] (an unknown name closes the
 * connection).  Registered variables are the members of cbuffers named 'X...' (XTweakable's
 * SunDirection, tracing.hlsl:6-9); a write updates the compute's cbuffer shadow, uploaded on the
 * next launch.  As in ComputeDirect3D::create (:408, :188-197) every rt_compute_load clears the
 * registry and registers its own shader's variables -- so after Terrain::reload (tracescreen, then
 * camerarays, which has no 'X' cbuffer) the registry is empty, as in the reference.
 * rt_varmgr_register_compute (not in the reference) re-registers one compute's variables and
 * sends them to a connected client.  port <= 0 means 10666; bind_address NULL = 127.0.0.1. */
int rt_varmgr_start(int port, const char* bind_address);
int rt_varmgr_stop(void);
int rt_varmgr_count(void);
int rt_varmgr_register_compute(rt_compute cs);

#ifdef __cplusplus
}
#endif
#endif
