// hq_wire_codec.h — the one protobuf reader and writer of raftpb.Message (raft.proto:154-168) and
// raftpb.MessageBatch (:191-196), and the cluster-id table beside them. One source for the host
// decoder and encoder (hq_wire.cpp), the framer (hq_wire_frame.cpp), the decode kernels
// (hq_wire_dev.hip), the heartbeat marshaller (hq_heartbeat_wire.h: host worker and kernels) and
// the stand-alone sanitizer programs of the tests, so what runs on the GPU runs on the CPU under
// sanitizers first. Plain C++17 over <cstdint> and the public header. No table, no array indexed
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
// common one-byte varint first; the kernels keep the loop rolled.
template <class I>
HQ_WIRE_HD bool varint(const uint8_t *b, I &p, I end, uint64_t &v) {
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
template <class I>
HQ_WIRE_HD uint32_t skip(const uint8_t *b, I &p, I end, uint32_t wt) {
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
template <class I>
HQ_WIRE_HD bool header(const uint8_t *b, I &p, I end, uint64_t &n) {
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
