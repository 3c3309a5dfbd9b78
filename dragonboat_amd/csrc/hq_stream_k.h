// hq_stream_k.h — internal: the byte codec of the compact event stream (include/hipquorum.h
// "event streams"), shared by the row entries (hq_stream.cpp) and the 16-byte-record encoder
// (hq_stream16.cpp): a step's events as one byte string per group, each event a header byte and
// LEB128 varints of only the fields its handler reads. The steady-state leader step
// (ReplicateResp / HeartbeatResp / proposals at the current term) takes 3-7 bytes per event
// instead of the 56-byte row. The device twin of the decoder is in hq_dstep_step.hip.
//
// Everything here is inline and in an unnamed namespace, as it was while one file held it: each
// unit folds these into its own loops (enc16_range holds encode16, run16 and put_run with no call
// out), and nothing of it is a symbol of the library.
#pragma once

#include <cstdint>
#include <cstring>

#include "../../include/hipquorum.h"

namespace hqs {
namespace {

// message types with a code of their own in the header (bits 3-5); 7 = the type follows
inline uint32_t type_code(uint32_t t) {
    switch (t) {
    case HQ_MSG_REPLICATE_RESP: return 0;
    case HQ_MSG_REQUEST_VOTE_RESP: return 1;
    case HQ_MSG_HEARTBEAT_RESP: return 2;
    case HQ_MSG_READ_INDEX: return 3;
    default: return 7;
    }
}
inline uint32_t code_type(uint32_t c) {
    static const uint32_t t[6] = {HQ_MSG_REPLICATE_RESP, HQ_MSG_REQUEST_VOTE_RESP,
                                  HQ_MSG_HEARTBEAT_RESP, HQ_MSG_READ_INDEX,
                                  HQ_MSG_REPLICATE_RESP, HQ_MSG_HEARTBEAT_RESP};
    return c < 6 ? t[c] : 0;
}

inline uint8_t *put(uint8_t *p, uint64_t v) {
    while (v >= 0x80) {
        *p++ = (uint8_t)(v | 0x80);
        v >>= 7;
    }
    *p++ = (uint8_t)v;
    return p;
}

inline bool get(const uint8_t *&p, const uint8_t *end, uint64_t &v) {
    v = 0;
    for (int shift = 0; shift < 64; shift += 7) {
        if (p >= end) return false;
        const uint8_t b = *p++;
        v |= (uint64_t)(b & 0x7F) << shift;
        if (b < 0x80) return true;
    }
    return false;
}

// a group's stream state the codes refer back to: its previous message term, its previous
// ReplicateResp's log_index (code 4), its previous HeartbeatResp's ctx (code 5; 0 / 0 at first),
// and the previous message a run (code 6) repeats: last 1 = a ReplicateResp, 2 = a HeartbeatResp
// (written with codes 0 / 4 / 2 / 5 or in a run), 0 = none or another type; last_reject its bit
struct Prev {
    uint64_t term = 0, index = 0, hint = 0, high = 0;
    bool have_index = false;
    uint8_t last = 0, last_reject = 0;
    bool run_seq = false;          // (decoder) the current run's senders are run_from, + 1, ..
    uint32_t run_from = 0;
};

// Runs (code 6): the acks of a steady leader's followers repeat one another but for the sender
// (every follower acks the same index, every follower's heartbeat ack carries the same ctx). A
// run of 3..kRunMax messages that repeat the group's previous message (its type, term, reject
// and index / ctx) is one header, a count and the senders: 2 + m bytes for 1-byte senders
// instead of 2 m. At most kRunMax events per run, so that a run with 10-byte senders still fits
// the HQ_EVENT_STREAM_MAX bytes the encoder asks for before each unit.
constexpr uint32_t kRunMin = 3, kRunMax = 6;
constexpr uint32_t kCodeRun = 6;

inline uint8_t last_of(uint32_t code) {
    return code == 0 || code == 4 ? 1 : code == 2 || code == 5 ? 2 : 0;
}

// does row e repeat the group's previous message (a run member)?
template <class Ev>
inline bool repeats(const Ev &e, const Prev &pv) {
    if (!pv.last || e.kind != HQ_EV_MESSAGE || (e.reject != 0) != (pv.last_reject != 0) ||
        e.term != pv.term)
        return false;
    if (pv.last == 1) return e.type == HQ_MSG_REPLICATE_RESP && e.log_index == pv.index;
    return e.type == HQ_MSG_HEARTBEAT_RESP && e.hint == pv.hint && e.hint_high == pv.high;
}

// a run of m messages repeating the previous one, senders from[0..m); senders s0, s0 + 1, ..
// (a leader's followers acking in node order) as the consecutive form: header bit 7, m, s0
template <class From>
inline uint8_t *put_run(uint8_t *p, uint32_t m, From from) {
    const uint64_t f0 = from(0);
    // s0 + m <= 2^32 - 1, compared without the sum: s0 near 2^64 must not wrap into the form
    bool seq = f0 <= 0xFFFFFFFFull - m;
    for (uint32_t j = 1; j < m && seq; ++j) seq = from(j) == f0 + j;
    if (seq) {
        *p++ = (uint8_t)(HQ_EV_MESSAGE | kCodeRun << 3 | 0x80);
        *p++ = (uint8_t)m;
        if (f0 < 0x80) *p++ = (uint8_t)f0;
        else p = put(p, f0);
        return p;
    }
    *p++ = (uint8_t)(HQ_EV_MESSAGE | kCodeRun << 3);
    *p++ = (uint8_t)m;                  // m <= kRunMax: one byte
    for (uint32_t j = 0; j < m; ++j) {
        const uint64_t f = from(j);
        if (f < 0x80) *p++ = (uint8_t)f;   // (a node id: one byte in the steady state)
        else p = put(p, f);
    }
    return p;
}

// the 1- and 2-byte varints inline
__attribute__((always_inline)) inline uint8_t *put_fast(uint8_t *p, uint64_t v) {
    if (v < 0x80) {
        *p = (uint8_t)v;
        return p + 1;
    }
    if (v < 0x4000) {
        p[0] = (uint8_t)(v | 0x80);
        p[1] = (uint8_t)(v >> 7);
        return p + 2;
    }
    return put(p, v);
}

// one event; returns the write position
template <class Ev>
inline uint8_t *encode(uint8_t *p, const Ev &e, Prev &pv) {
    const uint32_t kind = e.kind >= 1 && e.kind <= 5 ? e.kind : 0;   // 0: not a valid kind
    if (kind != HQ_EV_MESSAGE) {
        *p++ = (uint8_t)kind;
        if (kind == HQ_EV_READ) {
            p = put(p, e.hint);
            p = put_fast(p, e.hint_high);
        } else if (kind == HQ_EV_PROPOSE) {
            p = put_fast(p, e.log_index);
        }
        return p;
    }
    uint32_t code = type_code(e.type);
    if (code == 0) {
        if (pv.have_index && e.log_index == pv.index) code = 4;
        pv.index = e.log_index;
        pv.have_index = true;
    } else if (code == 2) {
        if (e.hint == pv.hint && e.hint_high == pv.high) code = 5;
        pv.hint = e.hint;
        pv.high = e.hint_high;
    }
    const bool same = e.term == pv.term;
    pv.last = last_of(code);
    pv.last_reject = e.reject ? 1 : 0;
    *p++ = (uint8_t)(HQ_EV_MESSAGE | code << 3 | (e.reject ? 0x40 : 0) | (same ? 0x80 : 0));
    if (code == 7) p = put(p, e.type);
    p = put_fast(p, e.from);
    if (!same) p = put(p, e.term);
    pv.term = e.term;
    if (code == 0 || code == 7) p = put_fast(p, e.log_index);
    if (code == 2 || code == 3 || code == 7) {
        p = put(p, e.hint);
        p = put_fast(p, e.hint_high);
    }
    return p;
}

// the rows events[e .. e1) that open with a run: its length (0 below kRunMin)
template <class Ev>
inline uint32_t run_rows(const Ev *events, uint64_t e, uint64_t e1, const Prev &pv) {
    uint32_t m = 0;
    while (m < kRunMax && e + m < e1 && repeats(events[e + m], pv)) ++m;
    return m >= kRunMin ? m : 0;
}

// the unit at row e of a group's rows [.., e1): a run of repeats of the previous message, or
// row e alone; returns the next row
template <class Ev>
__attribute__((always_inline)) inline uint64_t encode_unit(uint8_t *&p, const Ev *events, uint64_t e, uint64_t e1, Prev &pv) {
    if (pv.last) {
        const uint32_t m = run_rows(events, e, e1, pv);
        if (m) {
            p = put_run(p, m, [&](uint32_t j) { return events[e + j].from; });
            return e + m;
        }
    }
    p = encode(p, events[e], pv);
    return e + 1;
}

}  // namespace
}  // namespace hqs
