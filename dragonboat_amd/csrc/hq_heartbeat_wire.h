// hq_heartbeat_wire.h — the Heartbeat marshaller of hq_worker_heartbeat_batches: one message and
// the MessageBatch trailer, written with hq_wire_codec.h's writers (as hq_wire_encode_batch writes
// any message). One source for the host worker (hq_worker_hb.cpp), the kernels
// (hq_heartbeat_wire.hip) and the stand-alone sanitizer program of
// tests/test_heartbeat_wire_host.py, so the functions run on the CPU under sanitizers before they
// run on the GPU. No table, no array indexed by a variable: the kernels keep everything in
// registers.
#pragma once

#include <cstdint>

#include "hq_wire_codec.h"


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

static_assert(kHbBodyFixed == 2 + 3 * 2 + 2 + hqw::kEmptySnapshot && kHbBinVer == HQ_RPC_BIN_VERSION,
              "the codec's snapshot and version");

// tag + length + body
HQ_WIRE_HD uint32_t hb_msg_size(const hb_fields &f) {
    return 2 + hqw::body_size(17, f.to, f.from, f.cluster_id, f.term, 0, 0, f.commit, 0, f.hint,
                              f.hint_high);
}

// writes hb_msg_size(f) bytes at dst; returns the byte after them
HQ_WIRE_HD uint8_t *hb_msg_put(uint8_t *dst, const hb_fields &f) {
    uint8_t *p = dst;
    *p++ = 0x0a;                                  // requests (1), length-delimited
    *p++ = (uint8_t)(hb_msg_size(f) - 2);
    // Type: Heartbeat; LogTerm, LogIndex and Reject 0
    return hqw::put_body(p, 17, f.to, f.from, f.cluster_id, f.term, 0, 0, f.commit, 0, f.hint,
                         f.hint_high);
}

// deployment_id (2), source_address (3), bin_ver (4)
HQ_WIRE_HD uint32_t hb_trailer_size(uint64_t deployment_id, uint32_t source_len) {
    return hqw::trailer_size(deployment_id, source_len);
}

// writes hb_trailer_size(...) bytes at dst (source_len <= kHbSourceMax); returns the byte after
HQ_WIRE_HD uint8_t *hb_trailer_put(uint8_t *dst, uint64_t deployment_id, const uint8_t *source,
                                  uint32_t source_len) {
    return hqw::put_trailer(dst, deployment_id, source, source_len);
}
