// A caller's ring of output slots, as every output stage of the stream pipeline keeps one (the rule is stated once, at
// ofx_session_stream_compose in include/ofx.h): pair p (1-based) goes to slot (p - 1) mod slots at base + slot * stride, and the
// ring holds the newest `slots` pairs the stage has written in this stream.  Plain host code without HIP in it, so that
// tests/test_out_ring.py compiles it into a stand-alone program (tools/out_ring_main.cpp).
#pragma once

#include <stddef.h>

namespace ofx_ring {

struct OutRing {
    char *base = nullptr; // the caller's buffer (nullptr: off)
    size_t stride = 0;    // bytes from slot to slot
    int slots = 0;
    long newest = 0;      // the newest pair the stage has written in this stream (0: none yet)

    bool on() const { return base != nullptr; }
    long index(long pair) const { return (pair - 1) % slots; }
    char *slot(long pair) const { return base + (size_t)index(pair) * stride; }
    // is `pair` among the newest `slots` pairs written?  (anything older has been overwritten, anything newer is not there yet)
    bool holds(long pair) const { return pair >= 1 && pair <= newest && pair > newest - slots; }
    void reset() { newest = 0; } // a new stream, or a new setting: nothing of it has been written
    void set(void *ring, size_t slot_stride, int n_slots) { base = static_cast<char *>(ring), stride = slot_stride, slots = n_slots, newest = 0; }
};

} // namespace ofx_ring
