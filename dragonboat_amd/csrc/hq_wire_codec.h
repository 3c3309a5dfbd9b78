// hq_wire_codec.h — the one protobuf reader and writer of raftpb.Message (raft.proto:154-168) and
// raftpb.MessageBatch (:191-196), and the cluster-id table beside them. One source for the host
// decoder and encoder (hq_wire.cpp), the framer (hq_wire_frame.cpp) and the framing kernels
// (hq_wire_frame_dev.hip: the segment walker below), the decode kernels (hq_wire_dev.hip), the
// heartbeat marshaller (hq_heartbeat_wire.h: host worker and kernels) and the stand-alone
// sanitizer programs of the tests, so what runs on the GPU runs on the CPU under sanitizers first. Plain C++17 over <cstdint> and the public header. No table, no array indexed
// by a variable: the kernels keep everything in registers.
//
// What the reader accepts is any valid proto2 encoding (as Message.Unmarshal raft.pb.go:4831 /
// raft_optimized.go:654 do): fields in any order, a repeated scalar takes its last value, the
// tag's field number truncated to 32 bits, unknown fields skipped by wire type. The bytes come
// from the network: every loop consumes at least one byte per turn, a varint reads at most 10
// bytes, and nothing at or past `end` is read.
#pragma once

#include <cstdint>

#include "../../include/hipquorum.h"

#if defined(__HIPCC__)
#define HQ_WIRE_HD __host__ __device__ inline
#else
#define HQ_WIRE_HD inline
#endif

namespace hqw {

constexpr uint32_t kSnapshotReceived = 22;   // raft.proto MessageType

// ---- reading -----------------------------------------------------------------------------------
// A position is an index from `b` of type I: 32 bits over LDS, 64 bits over memory, size_t (a
// pointer difference) on the host.

// LEB128 at b[p ..): false at `end` before the last byte, or past 64 bits. The host takes the
// common one-byte varint first; the kernels keep the loop rolled. B is `const uint8_t *`, or
// anything else that gives the byte at a position by b[p] (Window below).
template <class I, class B>
HQ_WIRE_HD bool varint(B b, I &p, I end, uint64_t &v) {
#if !defined(__HIP_DEVICE_COMPILE__)
    if (p < end && b[p] < 0x80) {
        v = b[p++];
        return true;
    }
#endif
    v = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int shift = 0; shift < 64; shift += 7) {
        if (p >= end) return false;               // unexpected end of data in a varint
        const uint8_t x = b[p++];
        v |= (uint64_t)(x & 0x7F) << shift;
        if (x < 0x80) return true;
    }
    return false;                                 // varint overflows 64 bits
}

// why a read stopped: the code, and the field and wire type it stopped at
enum : uint32_t {
    kOk = 0,
    kVarintEnd,         // unexpected end of data in a varint
    kVarintOverflow,    // varint overflows 64 bits
    kFieldZero,         // illegal field number 0
    kWrongType,         // a known field with another wire type
    kGroup,             // unsupported wire type (groups are not part of raft.proto)
    kFieldEnd,          // unexpected end of data in a skipped field
    kBytesEnd,          // unexpected end of data in a length-delimited field
};
struct error {
    uint32_t code, field, wt;
};

// which of its two ways a varint that began at p0 failed: only an overflow consumes 10 bytes
template <class I>
HQ_WIRE_HD uint32_t varint_error(I p0, I p) {
    return p - p0 == 10 ? kVarintOverflow : kVarintEnd;
}

// a field of wire type wt hopped over (skipRaft, raft.pb.go:6293): kOk or why not
template <class I, class B>
HQ_WIRE_HD uint32_t skip(B b, I &p, I end, uint32_t wt) {
    uint64_t n = 0;
    const I p0 = p;
    switch (wt) {
    case 0:
        if (!varint(b, p, end, n)) return varint_error(p0, p);
        n = 0;
        break;
    case 1: n = 8; break;
    case 2:
        if (!varint(b, p, end, n)) return varint_error(p0, p);
        break;
    case 5: n = 4; break;
    default: return kGroup;
    }
    if ((uint64_t)(end - p) < n) return kFieldEnd;
    p += (I)n;
    return kOk;
}

// the `requests` header at p: its body's position and length; false when it is not one, or runs
// past end
template <class I, class B>
HQ_WIRE_HD bool header(B b, I &p, I end, uint64_t &n) {
    uint64_t tag;
    if (!varint(b, p, end, tag)) return false;
    if ((uint32_t)(tag >> 3) != 1 || (uint32_t)(tag & 7) != 2) return false;
    if (!varint(b, p, end, n)) return false;
    return (uint64_t)(end - p) >= n;
}

// raftpb.Message over b[0 .. end) into the fields the quorum path reads; entries counted, the
// snapshot noted. false: rejected, and e says why
template <class I>
HQ_WIRE_HD bool decode_message(const uint8_t *b, I end, hq_wire_message &m, error &e) {
    m = hq_wire_message{};
    m.ev.kind = HQ_EV_MESSAGE;
    e = error{kOk, 0, 0};
    I p = 0;
    while (p < end) {
        uint64_t tag;
        I p0 = p;
        if (!varint(b, p, end, tag)) return e.code = varint_error(p0, p), false;
        const uint32_t field = (uint32_t)(tag >> 3), wt = (uint32_t)(tag & 7);
        e.field = field;
        e.wt = wt;
        if (field == 0) return e.code = kFieldZero, false;
        uint64_t v = 0;
        if (field <= 10 || field == 13) {             // the varint fields
            if (wt != 0) return e.code = kWrongType, false;
            p0 = p;
            if (!varint(b, p, end, v)) return e.code = varint_error(p0, p), false;
        }
        switch (field) {
        case 1: m.ev.type = (uint32_t)v; break;
        case 2: m.to = v; break;
        case 3: m.ev.from = v; break;
        case 4: m.cluster_id = v; break;
        case 5: m.ev.term = v; break;
        case 6: m.log_term = v; break;
        case 7: m.ev.log_index = v; break;
        case 8: m.commit = v; break;
        case 9: m.ev.reject = v != 0; break;
        case 10: m.ev.hint = v; break;
        case 13: m.ev.hint_high = v; break;
        case 11:                                   // entries: counted and skipped
        case 12: {                                 // the snapshot: noted and skipped
            if (wt != 2) return e.code = kWrongType, false;
            uint64_t n;
            p0 = p;
            if (!varint(b, p, end, n)) return e.code = varint_error(p0, p), false;
            if ((uint64_t)(end - p) < n) return e.code = kBytesEnd, false;
            p += (I)n;
            if (field == 11) m.n_entries++;
            else m.has_snapshot = 1;
            break;
        }
        default:                                   // unknown: skipped by wire type
            if ((e.code = skip(b, p, end, wt)) != kOk) return false;
        }
    }
    return true;
}

// MessageBatch: on_message(field, body, n) for every `requests` field in order — the field (tag,
// length, body) starts at bytes[field], its n-byte body at bytes[body]; a non-zero return ends the
// walk with it — and on_other() before any other field; deployment_id, source_address's length
// and bin_ver into info, the messages handed on so far in info.n_messages. Any field order;
// unknown fields skipped; field 0, a known field's wrong wire type and a field past the end give
// HQ_E_INVAL.
template <class OnMessage, class OnOther>
inline int walk_batch(const uint8_t *bytes, size_t len, hq_wire_batch_info &info,
                      OnMessage &&on_message, OnOther &&on_other) {
    info = hq_wire_batch_info{};
    size_t p = 0;
    const size_t end = len;
    while (p < end) {
        const size_t f0 = p;
        uint64_t n;
        // the common case first: a Message (tag 0x0a) shorter than 128 bytes
        if (end - p >= 2 && bytes[p] == 0x0a && bytes[p + 1] < 0x80) {
            n = bytes[p + 1];
            p += 2;
            if ((uint64_t)(end - p) < n) return HQ_E_INVAL;
        } else {
            uint64_t tag;
            if (!varint(bytes, p, end, tag)) return HQ_E_INVAL;
            const uint32_t field = (uint32_t)(tag >> 3), wt = (uint32_t)(tag & 7);
            if (field != 1 || wt != 2) {
                on_other();
                uint64_t v;
                if (field == 2 && wt == 0) {              // deployment_id
                    if (!varint(bytes, p, end, info.deployment_id)) return HQ_E_INVAL;
                } else if (field == 3 && wt == 2) {       // source_address
                    if (!varint(bytes, p, end, v) || (uint64_t)(end - p) < v) return HQ_E_INVAL;
                    p += (size_t)v;
                    info.source_address_len = v;
                } else if (field == 4 && wt == 0) {       // bin_ver
                    if (!varint(bytes, p, end, v)) return HQ_E_INVAL;
                    info.bin_ver = (uint32_t)v;
                } else if (field <= 4) {                  // field 0, or a known field's wrong type
                    return HQ_E_INVAL;
                } else if (skip(bytes, p, end, wt) != kOk) {
                    return HQ_E_INVAL;
                }
                continue;
            }
            if (!varint(bytes, p, end, n) || (uint64_t)(end - p) < n) return HQ_E_INVAL;
        }
        const size_t body = p;                            // repeated Message requests
        p += (size_t)n;
        const int rc = on_message(f0, body, (size_t)n);
        if (rc) return rc;
        info.n_messages++;
    }
    return HQ_OK;
}

// ---- framing by segments -------------------------------------------------------------------------
// walk_batch's walk cut into pieces that can run side by side (hq_wire_frame_dev.hip; the host runs
// the same code under sanitizers, tests/test_wire_frame_segments.py). A batch is cut at the fixed
// positions k * S; segment k owns every field that STARTS in [k S, (k + 1) S), wherever it ends.
// Walked from its entry (the first field start at or past k S) a segment gives its fields exactly
// as walk_batch does, and its exit, the first field start at or past its end, which is the entry
// of the next segment that is not swallowed by a long field. Segment 0 enters at 0; a later one
// does not know its entry and guesses it (guess_entry). Nothing may depend on the guess:
// chain_batch walks the segments' records in order and takes a segment only when its entry is the
// exit handed to it, so by induction from segment 0 every segment it takes was walked from its
// true entry; a wrong guess leaves the batch unconfirmed (framed again by walk_batch).

// A stretch [lo, hi) of a batch kept at b (the kernels': in LDS); positions count from the batch
struct Window {
    const uint8_t *b;
    uint64_t lo, hi;
    HQ_WIRE_HD uint8_t operator[](uint64_t p) const { return b[p - lo]; }
};
// ... backed by the batch itself where the stretch ends (the guess's reads behind its window)
struct WindowOver {
    Window w;
    const uint8_t *batch;
    HQ_WIRE_HD uint8_t operator[](uint64_t p) const {
        return p >= w.lo && p < w.hi ? w.b[p - w.lo] : batch[p];
    }
};

constexpr uint32_t kFieldHead = 20;        // a field's tag and its length or value: two varints
constexpr uint64_t kNoEntry = ~0ull;       // no guess
constexpr uint32_t kGuessMessages = 4, kGuessFields = 8;
enum : uint32_t { kSeenDeployment = 1, kSeenSource = 2, kSeenBinVer = 4 };

struct Segment {                           // what the walk of one segment leaves
    uint64_t entry, exit;
    uint64_t n_messages, n_spans;          // spans: counted always, written while they fit
    uint64_t deployment_id, source_address_len;
    uint32_t bin_ver;
    uint32_t seen;                         // kSeen*: the batch's own fields this segment set
    uint32_t malformed;                    // walk_batch's HQ_E_INVAL, met from this entry
    uint32_t pad;
};

struct SegmentWalk {                       // a segment's walk under way
    Segment s;
    uint64_t pos;                          // the next field's start
    hq_wire_span cur;                      // the open span (count 0: none); `first` counts from
};                                         // the segment's first message

HQ_WIRE_HD void segment_begin(SegmentWalk &w, uint64_t entry) {
    w = SegmentWalk{};
    w.s.entry = w.s.exit = w.pos = entry;
}

template <class Put>
HQ_WIRE_HD void span_close(SegmentWalk &w, Put &&put) {
    if (!w.cur.count) return;
    put(w.s.n_spans, w.cur);
    w.s.n_spans++;
    w.cur = hq_wire_span{};
}

// hq_wire_frame.cpp's rule: the field at [off, off + size) is the segment's next message
template <class Put>
HQ_WIRE_HD void span_add(SegmentWalk &w, uint64_t off, uint64_t size, Put &&put) {
    const bool large = size > HQ_WIRE_SPAN_BYTES;
    if (w.cur.count && (large || w.cur.count == HQ_WIRE_SPAN_MESSAGES ||
                        w.cur.len + size > HQ_WIRE_SPAN_BYTES))
        span_close(w, put);
    if (!w.cur.count) {
        w.cur.offset = off;
        w.cur.first = (uint32_t)w.s.n_messages;
    }
    w.cur.len += size;
    w.cur.count++;
    if (large) {
        w.cur.flags = HQ_WIRE_SPAN_LARGE;
        span_close(w, put);
    }
    w.s.n_messages++;
}

// The walk from w.pos on, over bytes b that hold the batch's [.., hi) (hi <= len, the batch's
// length): every field that starts before seg_end, as walk_batch takes it; put(i, span) for the
// segment's i-th span. true: the segment is done (w.s.exit or w.s.malformed set; the open span
// closed); false: the field at w.pos needs bytes behind hi (it is walked only with kFieldHead
// bytes or the batch's end in sight: call again with a window that starts at w.pos).
template <class B, class Put>
HQ_WIRE_HD bool walk_segment(const B &b, uint64_t hi, uint64_t len, uint64_t seg_end,
                             SegmentWalk &w, Put &&put) {
    const uint64_t end = len;
    while (w.pos < seg_end) {
        uint64_t p = w.pos;
        if (hi < len && p + kFieldHead > hi) return false;
        const uint64_t f0 = p;
        uint64_t n;
        if (end - p >= 2 && b[p] == 0x0a && b[p + 1] < 0x80) {
            n = b[p + 1];
            p += 2;
            if (end - p < n) return w.s.malformed = 1, true;
        } else {
            uint64_t tag;
            if (!varint(b, p, end, tag)) return w.s.malformed = 1, true;
            const uint32_t field = (uint32_t)(tag >> 3), wt = (uint32_t)(tag & 7);
            if (field != 1 || wt != 2) {
                span_close(w, put);
                uint64_t v;
                if (field == 2 && wt == 0) {
                    if (!varint(b, p, end, v)) return w.s.malformed = 1, true;
                    w.s.deployment_id = v;
                    w.s.seen |= kSeenDeployment;
                } else if (field == 3 && wt == 2) {
                    if (!varint(b, p, end, v) || end - p < v) return w.s.malformed = 1, true;
                    p += v;
                    w.s.source_address_len = v;
                    w.s.seen |= kSeenSource;
                } else if (field == 4 && wt == 0) {
                    if (!varint(b, p, end, v)) return w.s.malformed = 1, true;
                    w.s.bin_ver = (uint32_t)v;
                    w.s.seen |= kSeenBinVer;
                } else if (field <= 4) {
                    return w.s.malformed = 1, true;
                } else if (skip(b, p, end, wt) != kOk) {
                    return w.s.malformed = 1, true;
                }
                w.pos = p;
                continue;
            }
            if (!varint(b, p, end, n) || end - p < n) return w.s.malformed = 1, true;
        }
        p += n;
        span_add(w, f0, p - f0, put);
        w.pos = p;
    }
    span_close(w, put);
    w.s.exit = w.pos;
    return true;
}

// Whether fields may start at q (< len): kGuessMessages `requests` fields back to back, or at
// most kGuessFields `requests` fields and fields of the batch's own (2, 3, 4) that end with the
// batch. An unknown field is not taken: what a message holds (fields 5 and up, and fields 1 to 4
// as varints) must not look like a batch. Reads at most kFieldHead bytes at each of at most
// kGuessFields places.
template <class B>
HQ_WIRE_HD bool guess_at(const B &b, uint64_t q, uint64_t len) {
    uint64_t p = q;
    uint32_t messages = 0;
    bool other = false;
    for (uint32_t f = 0; f < kGuessFields; ++f) {
        if (p == len) return true;
        uint64_t tag, v;
        if (!varint(b, p, len, tag)) return false;
        const uint32_t field = (uint32_t)(tag >> 3), wt = (uint32_t)(tag & 7);
        if (field == 1 && wt == 2) {
            if (!varint(b, p, len, v) || len - p < v) return false;
            p += v;
            if (!other && ++messages == kGuessMessages) return true;
        } else if ((field == 2 || field == 4) && wt == 0) {
            other = true;
            if (!varint(b, p, len, v)) return false;
        } else if (field == 3 && wt == 2) {
            other = true;
            if (!varint(b, p, len, v) || len - p < v) return false;
            p += v;
        } else {
            return false;
        }
    }
    return p == len;
}

// the first q in [lo, hi) that guess_at takes, or kNoEntry
template <class B>
HQ_WIRE_HD uint64_t guess_entry(const B &b, uint64_t lo, uint64_t hi, uint64_t len) {
    for (uint64_t q = lo; q < hi; ++q)
        if (guess_at(b, q, len)) return q;
    return kNoEntry;
}

// where segment k of a batch of len bytes cut every S bytes ends (it starts at k S)
HQ_WIRE_HD uint64_t segment_end(uint64_t k, uint64_t S, uint64_t len) {
    return (k + 1) * S < len ? (k + 1) * S : len;
}
HQ_WIRE_HD uint64_t segment_count(uint64_t S, uint64_t len) { return (len + S - 1) / S; }

enum : uint32_t { kFramed = 0, kMalformed = 1, kSpansDidNotFit = 2, kUnconfirmed = 3 };

struct SegmentPlace {                      // where a taken segment's output goes in its batch's;
    uint64_t first_message, first_span;    // first_span == kNoEntry: void (inside a long field)
};

// The chain over a batch's n segment records: status, the batch's counts and fields into r,
// each segment's place into place[0 .. n), the void segments counted. span_cap: what a
// segment's span region holds.
HQ_WIRE_HD void chain_batch(const Segment *seg, uint64_t n, uint64_t S, uint64_t len,
                            uint64_t span_cap, SegmentPlace *place, hq_wire_frame_result &r,
                            uint32_t &voids) {
    r = hq_wire_frame_result{};
    voids = 0;
    uint64_t cur = 0;
    bool fit = true;
    for (uint64_t k = 0; k < n; ++k) {
        if (cur >= segment_end(k, S, len)) {
            place[k] = SegmentPlace{0, kNoEntry};
            ++voids;
            continue;
        }
        const Segment s = seg[k];
        if (s.entry != cur) {
            r.status = kUnconfirmed;
            return;
        }
        place[k] = SegmentPlace{r.n_messages, r.n_spans};
        r.n_messages += s.n_messages;
        r.n_spans += s.n_spans;
        fit = fit && s.n_spans <= span_cap;
        if (s.seen & kSeenDeployment) r.deployment_id = s.deployment_id;
        if (s.seen & kSeenSource) r.source_address_len = s.source_address_len;
        if (s.seen & kSeenBinVer) r.bin_ver = s.bin_ver;
        if (s.malformed || r.n_messages > UINT32_MAX) {      // (a span's `first` is 32 bits)
            r.status = kMalformed;
            return;
        }
        cur = s.exit;
    }
    if (!fit) r.status = kSpansDidNotFit;
}

// ---- writing -----------------------------------------------------------------------------------

HQ_WIRE_HD uint32_t vlen(uint64_t v) {
    uint32_t k = 1;
    for (; v >= 0x80; v >>= 7) ++k;        // (at most 9 turns)
    return k;
}

HQ_WIRE_HD uint8_t *put_varint(uint8_t *p, uint64_t v) {
    for (; v >= 0x80; v >>= 7) *p++ = (uint8_t)(v | 0x80);
    *p++ = (uint8_t)v;
    return p;
}

HQ_WIRE_HD uint8_t *put_field(uint8_t *p, uint8_t tag, uint64_t v) {
    *p++ = tag;
    return put_varint(p, v);
}

// the empty Snapshot (Message field 12, nullable=false: always written) is 2 + 24 bytes
// (Snapshot.MarshalTo raft.pb.go:2142 over the empty Membership :2019)
constexpr uint32_t kEmptySnapshot = 24;

HQ_WIRE_HD uint8_t *put_empty_snapshot(uint8_t *p) {
    *p++ = 0x62;
    *p++ = kEmptySnapshot;
    *p++ = 0x12; *p++ = 0;
    *p++ = 0x18; *p++ = 0;
    *p++ = 0x20; *p++ = 0;
    *p++ = 0x28; *p++ = 0;
    *p++ = 0x32; *p++ = 2;
    *p++ = 0x08; *p++ = 0;
    *p++ = 0x48; *p++ = 0;
    *p++ = 0x50; *p++ = 0;
    *p++ = 0x58; *p++ = 0;
    *p++ = 0x60; *p++ = 0;
    *p++ = 0x68; *p++ = 0;
    *p++ = 0x70; *p++ = 0;
    return p;
}

// A Message's body as Message.MarshalTo writes it (raft.pb.go:2232-2296): fields 1-10 in order,
// no entries, the empty Snapshot, HintHigh. Its size, and the bytes at p (returns the byte after).
HQ_WIRE_HD uint32_t body_size(uint64_t type, uint64_t to, uint64_t from, uint64_t cluster_id,
                              uint64_t term, uint64_t log_term, uint64_t log_index, uint64_t commit,
                              uint64_t reject, uint64_t hint, uint64_t hint_high) {
    return 11 + 2 + kEmptySnapshot + vlen(type) + vlen(to) + vlen(from) + vlen(cluster_id) +
           vlen(term) + vlen(log_term) + vlen(log_index) + vlen(commit) + vlen(reject) + vlen(hint) +
           vlen(hint_high);
}

HQ_WIRE_HD uint8_t *put_body(uint8_t *p, uint64_t type, uint64_t to, uint64_t from,
                             uint64_t cluster_id, uint64_t term, uint64_t log_term,
                             uint64_t log_index, uint64_t commit, uint64_t reject, uint64_t hint,
                             uint64_t hint_high) {
    p = put_field(p, 0x08, type);
    p = put_field(p, 0x10, to);
    p = put_field(p, 0x18, from);
    p = put_field(p, 0x20, cluster_id);
    p = put_field(p, 0x28, term);
    p = put_field(p, 0x30, log_term);
    p = put_field(p, 0x38, log_index);
    p = put_field(p, 0x40, commit);
    p = put_field(p, 0x48, reject);
    p = put_field(p, 0x50, hint);
    p = put_empty_snapshot(p);
    return put_field(p, 0x68, hint_high);
}

// the batch's trailer: deployment_id (2), source_address (3), bin_ver (4); L is the length's type
// (32 bits in the kernels)
template <class L>
HQ_WIRE_HD L trailer_size(uint64_t deployment_id, L source_len) {
    return 1 + vlen(deployment_id) + 1 + vlen(source_len) + source_len + 1 + vlen(HQ_RPC_BIN_VERSION);
}

template <class L>
HQ_WIRE_HD uint8_t *put_trailer(uint8_t *dst, uint64_t deployment_id, const uint8_t *source,
                                L source_len) {
    uint8_t *p = put_field(dst, 0x10, deployment_id);
    p = put_field(p, 0x1a, source_len);
    for (L i = 0; i < source_len; ++i) *p++ = source[i];
    return put_field(p, 0x20, HQ_RPC_BIN_VERSION);
}

// ---- the cluster-id table ------------------------------------------------------------------------
// cluster id -> a 32-bit value: open addressing, linear probing, a power of two of slots

struct Slot {                              // key and value side by side: a lookup touches 16 bytes
    uint64_t key;
    uint32_t val, pad;
};
constexpr uint64_t kEmptyKey = ~0ull;      // the one key the table cannot hold: kept beside it

HQ_WIRE_HD uint64_t hash_id(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    return x ^ (x >> 33);
}

// the value of id, or false
HQ_WIRE_HD bool find(const Slot *slots, uint64_t n_slots, uint32_t has_empty, uint32_t empty_val,
                     uint64_t id, uint32_t &v) {
    bool found = false;
    if (id == kEmptyKey) {
        found = has_empty != 0;
        v = empty_val;
    } else {
        const uint64_t mask = n_slots - 1;
        uint64_t s = hash_id(id) & mask;
        for (uint64_t probe = 0; probe < n_slots; ++probe, s = (s + 1) & mask) {
            const uint64_t k = slots[s].key;
            if (k == id) {
                found = true;
                v = slots[s].val;
                break;
            }
            if (k == kEmptyKey) break;
        }
    }
    return found;
}

}  // namespace hqw
