// rt_render_route.h -- the route one rt_terrain_render call takes (include/frosttrace.h), as a function of
// the device's and the frame's state.  The rules live here and nowhere else; rt_runtime.cpp fills the
// state and keeps the actions.  No HIP in here: tests/tools/render_route_check.cpp drives it stand-alone
// under ASan + UBSan.
#pragma once

#include <cstddef>

namespace rtr {

// rt_device_create's flags that a route depends on (RT_DEVICE_*; rt_runtime.cpp asserts the values)
constexpr unsigned kStats = 2u, kGraph = 4u, kGated = 128u, kDeferred = 1024u, kDebugDeferSmall = 2048u;

// RT_DEVICE_DEFERRED with one frame to a launch: frames of fewer pixels render as without the flag (at 256x256 the
// fused prepass outlasts the frame's trace: 0.642 against 0.585 ms a frame; neutral at 1280x720)
constexpr size_t kDeferFuseMinPixels = (size_t)1280 * 720;

enum Route {
    FULL_INLINE,      // prepass, setTargetDepths and trace in line on the device's stream
    SERIAL_PRESTREAM, // the prepass on the device's prepass stream, in the previous frame's trace tail
    SERIAL_FIRST,     // as FULL_INLINE, and it records ev_order: the next render may take the prepass stream
    DEFER_QUEUE,      // RT_DEVICE_DEFERRED, K >= 2 frames to a launch: the frame joins the queue
    DEFER_SMALL,      // RT_DEVICE_DEFERRED, a small frame: flush, then as a device without the flag
    DEFER_FUSE,       // RT_DEVICE_DEFERRED: the pending frame's trace runs this frame's prepass
    DEFER_INLINE      // RT_DEVICE_DEFERRED: flush, then this frame's prepass in line; its trace stays pending
};

struct State {
    unsigned flags = 0;      // the device's RT_DEVICE_* flags
    bool has_stream = false; // (false too when the computes name no device: the full render reports it)
    bool ahead_pending = false, ahead_in_pending = false, fuse_active = false; // fuse_state != FUSE_NONE
    bool serial_ok = false, order_recorded = false;
    int defer_k = 1;
    int shard_count = 1;
    size_t pixels = 0;                                      // width * height
    bool cam_nomadplains = false, scr_nomadplains = false;  // both computes have a shader of that landscape
    bool tables_equal = false;                              // the two shaders' noise tables hold the same bytes
    // the frame whose trace is pending on an RT_DEVICE_DEFERRED device (K = 1)
    struct Pending {
        bool pending = false;
        bool nomadplains = false;    // its tracescreen shader's landscape
        bool grad_dirty = false;     // that shader's noise gradients changed since they went up
        bool tables_equal = false;   // its noise tables against this frame's camerarays shader's
        bool rank_in_frame = false;  // its shard rank < the frame's tiles: its launch runs a k_trace
    } prev;
};

// nothing else holds the device's CameraResults, streams or kernels: the renders that may leave the full
// in-line render (a new device mode is added here)
inline bool plain(const State& s)
{
    return !(s.flags & (kGraph | kStats | kGated)) && s.has_stream && !s.ahead_pending && !s.ahead_in_pending &&
           !s.fuse_active;
}

// a device without RT_DEVICE_DEFERRED (and a small frame of one with it)
inline Route serial_route(const State& s)
{
    if (!plain(s)) return FULL_INLINE;
    return s.serial_ok && s.order_recorded ? SERIAL_PRESTREAM : SERIAL_FIRST;
}

inline Route route(const State& s)
{
    if (!(s.flags & kDeferred)) return serial_route(s);
    if (!(s.cam_nomadplains && s.scr_nomadplains && plain(s))) return FULL_INLINE;
    if (s.defer_k >= 2 && s.shard_count == 1 && s.tables_equal) return DEFER_QUEUE;
    // a small frame's trace is shorter than the prepass it would carry (profiles/r06/deferred.md)
    if (s.pixels < kDeferFuseMinPixels && !(s.flags & kDebugDeferSmall)) return DEFER_SMALL;
    // the pending frame's trace must run a k_trace (a single frame's shard past the last tile launches none)
    // with the noise tables this prepass reads: it loads them from the pending frame's tracescreen gradients,
    // which are up to date on the device unless a later write dirtied them
    const State::Pending& p = s.prev;
    const bool fuse = p.pending && p.nomadplains && !p.grad_dirty && p.tables_equal && p.rank_in_frame;
    return fuse ? DEFER_FUSE : DEFER_INLINE;
}

} // namespace rtr
