// hq_stream.h — internal: the event-stream encoder shared by hq_stream.cpp (rows) and
// hq_wire.cpp (events decoded from the wire). Internal to libhipquorum.so.
#pragma once

#include <cstdint>

#include "../../include/hipquorum.h"

namespace hqs {

// One event as the wire decoder keeps it: the fields the quorum path reads (the hq_event's,
// narrowed) with the wire's bookkeeping. key: the attached worker's handle, or the cluster's index
// of first appearance; cat: 0 local ReadIndex, 1 received message, 2 tick, 3 proposal
struct WireEvent {
    uint32_t key;
    uint8_t cat, kind, reject, pad;
    uint32_t type, pad2;
    uint64_t from, term, log_index, hint, hint_high;
};
static_assert(sizeof(WireEvent) == 56, "56-byte wire records");

// the step's row of a wire event (host, and the device wire's row kernel)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline hq_event to_event(const WireEvent &r) {
    hq_event e{};
    e.kind = r.kind;
    e.type = r.type;
    e.from = r.from;
    e.term = r.term;
    e.log_index = r.log_index;
    e.hint = r.hint;
    e.hint_high = r.hint_high;
    e.reject = r.reject;
    return e;
}

// a row's fields into a wire event (to_event's inverse; key and cat are the wire's own)
inline void from_event(WireEvent &r, const hq_event &e) {
    r.kind = (uint8_t)e.kind;
    r.reject = e.reject != 0;
    r.type = e.type;
    r.from = e.from;
    r.term = e.term;
    r.log_index = e.log_index;
    r.hint = e.hint;
    r.hint_high = e.hint_high;
}

// one group's events ev[0 .. n) encoded at p as hq_events_encode does (its runs and repeat
// codes); NULL when fewer than HQ_EVENT_STREAM_MAX bytes are left before an event
uint8_t *encode_group(uint8_t *p, const uint8_t *end, const hq_event *ev, uint64_t n);
uint8_t *encode_group(uint8_t *p, const uint8_t *end, const WireEvent *ev, uint64_t n);

}  // namespace hqs
