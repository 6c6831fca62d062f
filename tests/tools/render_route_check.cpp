// Stand-alone check of gpgpuraytrace_amd/csrc/rt_render_route.h: the route of one rt_terrain_render call for
// each state that decides it.  The expected routes were read off serial_render and deferred_render as they
// stood before the header existed.  Built with -fsanitize=address,undefined by tests/test_host.py; its own main.
#include <cstdio>
#include <initializer_list>

#include "rt_render_route.h"

using namespace rtr;

#define CHECK(x)                                                                 \
    do {                                                                         \
        if (!(x)) {                                                              \
            std::printf("render_route_check FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

// a nomadplains frame on an idle device with a stream that rendered such a frame before
static State plain_state(unsigned flags)
{
    State s;
    s.flags = flags;
    s.has_stream = true;
    s.serial_ok = s.order_recorded = true;
    s.pixels = kDeferFuseMinPixels;
    s.cam_nomadplains = s.scr_nomadplains = s.tables_equal = true;
    return s;
}

// RT_DEVICE_DEFERRED, a large frame and a pending frame this frame's prepass can ride on
static State deferred_state(int k)
{
    State s = plain_state(kDeferred);
    s.defer_k = k;
    s.prev.pending = s.prev.nomadplains = s.prev.tables_equal = s.prev.rank_in_frame = true;
    return s;
}

int main()
{
    State s;
    CHECK(route(s) == FULL_INLINE); // no device: the full render reports it

    // a device without RT_DEVICE_DEFERRED: the prepass stream, unless any one thing is in the way
    CHECK(route(plain_state(0)) == SERIAL_PRESTREAM);
    for (unsigned f : {kGraph, kStats, kGated}) CHECK(route(plain_state(f)) == FULL_INLINE);
    CHECK(route(plain_state(1u | 32u | 64u | 512u | kDebugDeferSmall)) == SERIAL_PRESTREAM); // the other flags
    bool State::*const blockers[] = {&State::ahead_pending, &State::ahead_in_pending, &State::fuse_active};
    for (auto m : blockers) {
        s = plain_state(0);
        s.*m = true;
        CHECK(route(s) == FULL_INLINE);
    }
    s = plain_state(0);
    s.has_stream = false;
    CHECK(route(s) == FULL_INLINE);
    s = plain_state(0);
    s.serial_ok = false;
    CHECK(route(s) == SERIAL_FIRST);
    s = plain_state(0);
    s.order_recorded = false;
    CHECK(route(s) == SERIAL_FIRST);
    s.has_stream = false; // (not plain wins over the first frame)
    CHECK(route(s) == FULL_INLINE);
    s = plain_state(0); // neither the landscape nor the frame size matters without the flag
    s.cam_nomadplains = s.scr_nomadplains = false;
    s.pixels = 1;
    CHECK(route(s) == SERIAL_PRESTREAM);

    // RT_DEVICE_DEFERRED, K = 1: fuse into the pending frame's trace; in line when any one of its facts fails
    CHECK(route(deferred_state(1)) == DEFER_FUSE);
    bool State::Pending::*const facts[] = {&State::Pending::pending, &State::Pending::nomadplains,
                                           &State::Pending::tables_equal, &State::Pending::rank_in_frame};
    for (auto m : facts) {
        s = deferred_state(1);
        s.prev.*m = false;
        CHECK(route(s) == DEFER_INLINE);
    }
    s = deferred_state(1);
    s.prev.grad_dirty = true;
    CHECK(route(s) == DEFER_INLINE);
    s = deferred_state(1); // serial_ok and order_recorded are the serial routes' business
    s.serial_ok = s.order_recorded = false;
    CHECK(route(s) == DEFER_FUSE);
    // another landscape, or anything that keeps a device without the flag in line: the full render
    s = deferred_state(1);
    s.cam_nomadplains = false;
    CHECK(route(s) == FULL_INLINE);
    s = deferred_state(1);
    s.scr_nomadplains = false;
    CHECK(route(s) == FULL_INLINE);
    for (unsigned f : {kGraph, kStats, kGated}) {
        s = deferred_state(2);
        s.flags |= f;
        CHECK(route(s) == FULL_INLINE);
    }
    for (auto m : blockers) {
        s = deferred_state(1);
        s.*m = true;
        CHECK(route(s) == FULL_INLINE);
    }
    s = deferred_state(1);
    s.has_stream = false;
    CHECK(route(s) == FULL_INLINE);
    // a small frame renders as without the flag, unless the debug flag keeps it deferred
    s = deferred_state(1);
    s.pixels = kDeferFuseMinPixels - 1;
    CHECK(route(s) == DEFER_SMALL);
    s.prev = State::Pending{};
    CHECK(route(s) == DEFER_SMALL);
    CHECK(serial_route(s) == SERIAL_PRESTREAM); // what the caller asks after its flush
    s.serial_ok = false;
    CHECK(serial_route(s) == SERIAL_FIRST);
    s = deferred_state(1);
    s.pixels = kDeferFuseMinPixels - 1;
    s.flags |= kDebugDeferSmall;
    CHECK(route(s) == DEFER_FUSE);
    s.prev.pending = false;
    CHECK(route(s) == DEFER_INLINE);
    static_assert(kDeferFuseMinPixels == (size_t)1280 * 720, "1280x720 is deferred");

    // K >= 2: the queue for whole frames with one set of noise tables, else the K = 1 routes
    for (int k : {2, 3, 4}) CHECK(route(deferred_state(k)) == DEFER_QUEUE);
    s = deferred_state(2);
    s.pixels = 1; // the queue takes small frames too
    s.prev = State::Pending{};
    CHECK(route(s) == DEFER_QUEUE);
    s = deferred_state(2);
    s.shard_count = 2;
    CHECK(route(s) == DEFER_FUSE);
    s.prev.pending = false;
    CHECK(route(s) == DEFER_INLINE);
    s = deferred_state(2);
    s.tables_equal = false;
    CHECK(route(s) == DEFER_FUSE);
    s.pixels = kDeferFuseMinPixels - 1;
    CHECK(route(s) == DEFER_SMALL);
    std::printf("render_route_check ok\n");
    return 0;
}
