// hq_heartbeat_wire.h — the Heartbeat marshaller of hq_worker_heartbeat_batches: one message and
// the MessageBatch trailer, byte for byte what hq_wire_encode_batch (hq_wire.cpp) writes for a
// Heartbeat. One source for the host worker (hq_worker.cpp), the kernels (hq_heartbeat_wire.hip)
// and the stand-alone sanitizer program of tests/test_heartbeat_wire_host.py, so the functions run
// on the CPU under sanitizers before they run on the GPU. No table, no array indexed by a
// variable: the kernels keep everything in registers.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define HQ_HBW_HD __host__ __device__ inline
#else
#define HQ_HBW_HD inline
#endif

// the fields of a Heartbeat that vary (Type 17; LogTerm, LogIndex, Reject 0; the empty Snapshot)
struct hb_fields {
    uint64_t to, from, cluster_id, term, commit, hint, hint_high;
};

// A Heartbeat's body: Type 2 bytes, LogTerm / LogIndex / Reject 2 bytes each, the Snapshot
// 2 + 24, and seven varint fields of 1 + (1 .. 10) bytes: 34 + 7 * 2 = 48 at least and
// 34 + 7 * 11 = 111 at most. 111 < 128, so the body's length prefix is ALWAYS one byte and a
// message is tag + length + body = 50 .. 113 bytes.
constexpr uint32_t kHbBodyFixed = 2 + 3 * 2 + 2 + 24;
constexpr uint32_t kHbBodyMin = kHbBodyFixed + 7 * 2, kHbBodyMax = kHbBodyFixed + 7 * 11;
constexpr uint32_t kHbMsgMin = 2 + kHbBodyMin, kHbMsgMax = 2 + kHbBodyMax;
static_assert(kHbBodyMax == 111 && kHbBodyMax < 128, "a Heartbeat body's length is a one-byte varint");
static_assert(kHbMsgMin == 50 && kHbMsgMax == 113, "50 .. 113 bytes per marshalled Heartbeat");

constexpr uint32_t kHbSourceMax = 256;     // source_address bytes (hq_heartbeat_wire_config)
constexpr uint32_t kHbBinVer = 210;        // HQ_RPC_BIN_VERSION
// the trailer: deployment_id 1 + (1 .. 10), source_address 1 + (1 .. 2) + len, bin_ver 1 + 2
constexpr uint32_t kHbTrailerMax = 11 + 3 + kHbSourceMax + 3;

HQ_HBW_HD uint32_t hb_vlen(uint64_t v) {
    uint32_t k = 1;
    for (; v >= 0x80; v >>= 7) ++k;        // (at most 9 turns)
    return k;
}

HQ_HBW_HD uint8_t *hb_put_varint(uint8_t *p, uint64_t v) {
    for (; v >= 0x80; v >>= 7) *p++ = (uint8_t)(v | 0x80);
    *p++ = (uint8_t)v;
    return p;
}

HQ_HBW_HD uint8_t *hb_put_field(uint8_t *p, uint8_t tag, uint64_t v) {
    *p++ = tag;
    return hb_put_varint(p, v);
}

// tag + length + body
HQ_HBW_HD uint32_t hb_msg_size(const hb_fields &f) {
    return 2 + kHbBodyFixed + 7 + hb_vlen(f.to) + hb_vlen(f.from) + hb_vlen(f.cluster_id) +
           hb_vlen(f.term) + hb_vlen(f.commit) + hb_vlen(f.hint) + hb_vlen(f.hint_high);
}

// writes hb_msg_size(f) bytes at dst; returns the byte after them
HQ_HBW_HD uint8_t *hb_msg_put(uint8_t *dst, const hb_fields &f) {
    uint8_t *p = dst;
    *p++ = 0x0a;                                  // requests (1), length-delimited
    *p++ = (uint8_t)(hb_msg_size(f) - 2);
    p = hb_put_field(p, 0x08, 17);                // Type: Heartbeat
    p = hb_put_field(p, 0x10, f.to);
    p = hb_put_field(p, 0x18, f.from);
    p = hb_put_field(p, 0x20, f.cluster_id);
    p = hb_put_field(p, 0x28, f.term);
    p = hb_put_field(p, 0x30, 0);                 // LogTerm
    p = hb_put_field(p, 0x38, 0);                 // LogIndex
    p = hb_put_field(p, 0x40, f.commit);
    p = hb_put_field(p, 0x48, 0);                 // Reject
    p = hb_put_field(p, 0x50, f.hint);
    // the empty Snapshot (12): 0x62, 24, then 12 00 18 00 20 00 28 00 32 02 08 00 48 00 50 00
    // 58 00 60 00 68 00 70 00 (hq_wire.cpp's kSnap)
    *p++ = 0x62;
    *p++ = 24;
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
    return hb_put_field(p, 0x68, f.hint_high);    // HintHigh (13)
}

// deployment_id (2), source_address (3), bin_ver (4)
HQ_HBW_HD uint32_t hb_trailer_size(uint64_t deployment_id, uint32_t source_len) {
    return 1 + hb_vlen(deployment_id) + 1 + hb_vlen(source_len) + source_len + 1 + hb_vlen(kHbBinVer);
}

// writes hb_trailer_size(...) bytes at dst (source_len <= kHbSourceMax); returns the byte after
HQ_HBW_HD uint8_t *hb_trailer_put(uint8_t *dst, uint64_t deployment_id, const uint8_t *source,
                                  uint32_t source_len) {
    uint8_t *p = hb_put_field(dst, 0x10, deployment_id);
    p = hb_put_field(p, 0x1a, source_len);
    for (uint32_t i = 0; i < source_len; ++i) *p++ = source[i];
    return hb_put_field(p, 0x20, kHbBinVer);
}
