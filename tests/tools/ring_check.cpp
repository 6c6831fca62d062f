// ring_check.cpp -- stand-alone check of the readback ring's host bookkeeping (gpgpuraytrace_amd/csrc/rt_ring.h).
// Built and run by tests/test_readback_ring_host.py with -fsanitize=address,undefined; no HIP, no library.
//   fill / full / release / wrap-around over many more tickets than slots, out-of-order release, stale tickets,
//   the attached -> in flight -> ready -> held walk, failures, and cancel.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_ring.h"

static int g_checks = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        ++g_checks;                                                          \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

// a capture's whole life through wait + release
static void finish(RtRing& r, unsigned long long t)
{
    const int s = r.find(t);
    CHECK(s >= 0);
    if (r.state(s) == RtRing::ATTACHED) CHECK(r.launched(s));
    CHECK(r.state(s) == RtRing::INFLIGHT);
    CHECK(!r.release(s)); // in flight: not the caller's yet
    CHECK(r.hold(s));
    CHECK(r.hold(s)); // waiting twice
    CHECK(r.release(s));
    CHECK(r.find(t) == -1); // stale from here on
    CHECK(!r.release(s));
}

static void fill_full_wrap(int depth)
{
    RtRing r(depth);
    CHECK(r.depth() == depth && r.live() == 0 && r.oldest() == -1);
    CHECK(r.find(0) == -1); // never issued
    unsigned long long t = 99;
    std::vector<unsigned long long> live;
    for (int i = 0; i < depth; ++i) {
        CHECK(r.peek() >= 0);
        const int s = r.submit(i % 2 ? RtRing::ATTACHED : RtRing::INFLIGHT, &t);
        CHECK(s >= 0 && t == (unsigned long long)i && r.ticket(s) == t && r.find(t) == s);
        live.push_back(t);
    }
    CHECK(r.live() == depth && r.peek() == -1);
    t = 99;
    CHECK(r.submit(RtRing::INFLIGHT, &t) == -1 && t == 99); // full: no ticket taken
    CHECK(r.next_ticket() == (unsigned long long)depth);
    // in-order consumer over 40 x depth tickets: release the oldest, submit, never full, tickets monotonic
    for (int i = 0; i < 40 * depth; ++i) {
        CHECK(r.ticket(r.oldest()) == live.front());
        finish(r, live.front());
        live.erase(live.begin());
        const unsigned long long want = r.next_ticket();
        const int s = r.submit(RtRing::INFLIGHT, &t);
        CHECK(s >= 0 && s < depth && t == want);
        live.push_back(t);
        CHECK(r.live() == depth && r.peek() == -1);
        for (unsigned long long u : live) CHECK(r.find(u) >= 0 && r.ticket(r.find(u)) == u);
        CHECK(r.find(live.front() - 1) == -1 && r.find(t + 1) == -1);
    }
    // out-of-order release: newest first, then every other one, then the rest
    finish(r, live.back());
    live.pop_back();
    CHECK(r.peek() >= 0 && r.live() == depth - 1);
    for (size_t i = 0; i < live.size(); i += 2) finish(r, live[i]);
    for (size_t i = 1; i < live.size(); i += 2) finish(r, live[i]);
    CHECK(r.live() == 0 && r.oldest() == -1);
    for (unsigned long long u = 0; u < r.next_ticket() + 3; ++u) CHECK(r.find(u) == -1);
}

static void states_and_cancel()
{
    RtRing r(4);
    unsigned long long a, b, c, d;
    const int sa = r.submit(RtRing::ATTACHED, &a), sb = r.submit(RtRing::INFLIGHT, &b);
    const int sc = r.submit(RtRing::INFLIGHT, &c), sd = r.submit(RtRing::ATTACHED, &d);
    CHECK(sa != sb && sb != sc && sc != sd && r.peek() == -1);
    CHECK(!r.ready(sa) && !r.hold(sa) && !r.release(sa)); // attached: nothing queued yet
    CHECK(!r.launched(sb));                               // already in flight
    CHECK(r.ready(sb) && r.state(sb) == RtRing::READY && !r.ready(sb));
    CHECK(r.hold(sc) && r.state(sc) == RtRing::HELD);
    CHECK(r.fail(sd) && r.state(sd) == RtRing::FAILED && !r.fail(sd) && !r.hold(sd) && !r.launched(sd));
    CHECK(r.oldest() == sa);
    // cancel: the attached one fails, the caller's captures (ready, held) and the failed one stay as they are
    CHECK(r.cancel() == 1);
    CHECK(r.state(sa) == RtRing::FAILED && r.state(sb) == RtRing::READY && r.state(sc) == RtRing::HELD);
    CHECK(r.find(a) == sa && r.find(d) == sd); // failed captures keep their tickets until released
    CHECK(r.release(sa) && r.release(sb) && r.release(sc) && r.release(sd));
    CHECK(r.live() == 0 && r.cancel() == 0);
    // a cancelled in-flight capture, and the slot's next life
    const int s = r.submit(RtRing::INFLIGHT, &a);
    CHECK(r.cancel() == 1 && r.state(s) == RtRing::FAILED && r.release(s));
    CHECK(r.submit(RtRing::ATTACHED, &b) >= 0 && b == a + 1);
    // out-of-range slots and depths are harmless
    CHECK(r.state(-1) == RtRing::FREE && r.state(99) == RtRing::FREE && !r.release(-1) && !r.hold(8) && !r.fail(4));
    CHECK(RtRing(0).depth() == 1 && RtRing(99).depth() == RtRing::MAX_DEPTH);
}

int main()
{
    for (int depth = 1; depth <= RtRing::MAX_DEPTH; ++depth) fill_full_wrap(depth);
    states_and_cancel();
    std::printf("ring_check ok: %d checks\n", g_checks);
    return 0;
}
