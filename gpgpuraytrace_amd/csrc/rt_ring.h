// rt_ring.h -- ticket and slot bookkeeping of the readback ring (rt_readback_*, include/frosttrace.h).
//
// Host only: no HIP call, no allocation after construction, so a stand-alone program can drive it
// (tests/test_readback_ring_host.py).  The runtime owns the buffers, streams and events; this class
// decides which slot a submit takes, which slot a ticket names and what state that capture is in.
//
//   FREE      nothing in the slot; a submit may take it
//   ATTACHED  a capture of a frame whose trace is not launched yet (RT_DEVICE_DEFERRED): nothing is queued
//   INFLIGHT  snapshot and copy are queued; the slot's done-event will fire
//   READY     the done-event was seen fired (rt_readback_ready == 1, or a wait without a set fail-safe word)
//   HELD      a wait handed the pinned slot to the caller
//   FAILED    the capture's frame was dropped, its enqueue failed, or the ring was detached / cancelled
// release() frees a READY, HELD or FAILED slot: a released slot's copy has completed by construction.
#ifndef RT_RING_H
#define RT_RING_H

#include <stdint.h>

class RtRing {
public:
    enum State { FREE = 0, ATTACHED = 1, INFLIGHT = 2, READY = 3, HELD = 4, FAILED = 5 };
    enum { MAX_DEPTH = 8 };

    explicit RtRing(int depth) : depth_(depth < 1 ? 1 : depth > MAX_DEPTH ? MAX_DEPTH : depth)
    {
        for (int i = 0; i < MAX_DEPTH; ++i) {
            state_[i] = FREE;
            ticket_[i] = 0;
        }
    }

    int depth() const { return depth_; }
    unsigned long long next_ticket() const { return next_; }

    // The slot the next submit takes: the first free one from the round-robin position on, or -1 when
    // every slot is still the caller's (ring full).  Takes nothing.
    int peek() const
    {
        for (int i = 0; i < depth_; ++i) {
            const int s = (int)((next_ + (unsigned long long)i) % (unsigned long long)depth_);
            if (state_[s] == FREE) return s;
        }
        return -1;
    }

    // Take peek()'s slot for a new capture in state `st` (ATTACHED or INFLIGHT); -1 when full.
    int submit(State st, unsigned long long* ticket)
    {
        const int s = peek();
        if (s < 0) return -1;
        state_[s] = st;
        ticket_[s] = next_;
        if (ticket) *ticket = next_;
        ++next_;
        return s;
    }

    // The slot of a live ticket, or -1 (never issued, or released: stale).
    int find(unsigned long long ticket) const
    {
        if (ticket >= next_) return -1;
        for (int s = 0; s < depth_; ++s)
            if (state_[s] != FREE && ticket_[s] == ticket) return s;
        return -1;
    }

    State state(int slot) const { return slot >= 0 && slot < depth_ ? state_[slot] : FREE; }
    unsigned long long ticket(int slot) const { return slot >= 0 && slot < depth_ ? ticket_[slot] : 0; }

    // The live capture with the smallest ticket (the recorder drains in order), or -1.
    int oldest() const
    {
        int best = -1;
        for (int s = 0; s < depth_; ++s)
            if (state_[s] != FREE && (best < 0 || ticket_[s] < ticket_[best])) best = s;
        return best;
    }

    int live() const
    {
        int n = 0;
        for (int s = 0; s < depth_; ++s) n += state_[s] != FREE;
        return n;
    }

    // State changes the runtime reports; each returns false (and changes nothing) from any other state.
    bool launched(int slot) { return move(slot, ATTACHED, INFLIGHT); }
    bool fail(int slot)
    {
        if (state(slot) != ATTACHED && state(slot) != INFLIGHT) return false;
        state_[slot] = FAILED;
        return true;
    }
    bool ready(int slot) { return move(slot, INFLIGHT, READY); }
    bool hold(int slot)
    {
        if (state(slot) != INFLIGHT && state(slot) != READY && state(slot) != HELD) return false;
        state_[slot] = HELD;
        return true;
    }
    bool release(int slot)
    {
        const State st = state(slot);
        if (st != READY && st != HELD && st != FAILED) return false;
        state_[slot] = FREE;
        return true;
    }

    // Every capture that is not the caller's yet fails (destroy / detach); returns how many.
    int cancel()
    {
        int n = 0;
        for (int s = 0; s < depth_; ++s) n += fail(s) ? 1 : 0;
        return n;
    }

private:
    bool move(int slot, State from, State to)
    {
        if (slot < 0 || slot >= depth_ || state_[slot] != from) return false;
        state_[slot] = to;
        return true;
    }
    int depth_;
    unsigned long long next_ = 0;
    State state_[MAX_DEPTH];
    unsigned long long ticket_[MAX_DEPTH];
};

#endif
