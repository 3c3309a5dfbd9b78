// hq_wire_frame.cpp — the host's share of the device wire decode: a raftpb.MessageBatch framed
// into spans (include/hipquorum.h "wire decode on the device"). Plain C++; no HIP, no worker.
//
// The walk is hq_wire.cpp's parse_batch (MessageBatch, raft.proto:191-196: any field order,
// unknown fields skipped, the same framing errors), but a `requests` field is only hopped over:
// its tag, its length and nothing of its body are read. What is inside a message is the decode
// kernel's business (hq_wire_dev.hip).
#include "../../include/hipquorum.h"

namespace {

struct Reader {
    const uint8_t *p, *end;

    bool varint(uint64_t &v) {
        v = 0;
        for (int shift = 0; shift < 64; shift += 7) {
            if (p >= end) return false;              // unexpected end of data in a varint
            const uint8_t b = *p++;
            v |= (uint64_t)(b & 0x7F) << shift;
            if (b < 0x80) return true;
        }
        return false;                                // varint overflows 64 bits
    }
    // a length-delimited field's body hopped over
    bool bytes(uint64_t &n) {
        if (!varint(n)) return false;
        if ((uint64_t)(end - p) < n) return false;
        p += n;
        return true;
    }
    bool skip(uint32_t wt) {
        uint64_t n = 0;
        switch (wt) {
        case 0: return varint(n);
        case 1: n = 8; break;
        case 2: return bytes(n);
        case 5: n = 4; break;
        default: return false;                       // groups are not part of raft.proto
        }
        if ((uint64_t)(end - p) < n) return false;
        p += n;
        return true;
    }
};

// the spans as they are formed: counted always, written while they fit
struct Spans {
    hq_wire_span *out;
    uint64_t cap, n = 0;
    hq_wire_span cur{};                              // cur.count == 0: no span open

    void close() {
        if (!cur.count) return;
        if (out && n < cap) out[n] = cur;
        ++n;
        cur = hq_wire_span{};
    }
    // message `index` is the field at [off, off + size): tag, length and body
    void add(uint64_t off, uint64_t size, uint32_t index) {
        const bool large = size > HQ_WIRE_SPAN_BYTES;
        if (cur.count && (large || cur.count == HQ_WIRE_SPAN_MESSAGES ||
                          cur.len + size > HQ_WIRE_SPAN_BYTES))
            close();
        if (!cur.count) {
            cur.offset = off;
            cur.first = index;
        }
        cur.len += size;
        cur.count++;
        if (large) {                                 // a span by itself
            cur.flags = HQ_WIRE_SPAN_LARGE;
            close();
        }
    }
};

}  // namespace

extern "C" int hq_wire_frame_batch(const uint8_t *bytes, size_t len, uint64_t base,
                                   hq_wire_span *spans, uint64_t cap, uint64_t *n_spans,
                                   hq_wire_batch_info *info) {
    if ((!bytes && len) || !n_spans) return HQ_E_INVAL;
    *n_spans = 0;
    hq_wire_batch_info bi{};
    Spans s{spans, cap};
    uint64_t count = 0;
    Reader r{bytes, bytes + len};
    while (r.p < r.end) {
        const uint8_t *const f0 = r.p;
        uint64_t tag;
        if (!r.varint(tag)) return HQ_E_INVAL;
        const uint32_t field = (uint32_t)(tag >> 3), wt = (uint32_t)(tag & 7);
        if (field == 1 && wt == 2) {                  // repeated Message requests
            uint64_t n;
            if (!r.bytes(n)) return HQ_E_INVAL;
            if (count >= UINT32_MAX) return HQ_E_INVAL;   // (a span's `first` is 32 bits)
            s.add(base + (uint64_t)(f0 - bytes), (uint64_t)(r.p - f0), (uint32_t)count);
            ++count;
            continue;
        }
        s.close();                                    // a span is `requests` fields back to back
        if (field == 2 && wt == 0) {                  // deployment_id
            if (!r.varint(bi.deployment_id)) return HQ_E_INVAL;
        } else if (field == 3 && wt == 2) {           // source_address
            uint64_t n;
            if (!r.bytes(n)) return HQ_E_INVAL;
            bi.source_address_len = n;
        } else if (field == 4 && wt == 0) {           // bin_ver
            uint64_t v;
            if (!r.varint(v)) return HQ_E_INVAL;
            bi.bin_ver = (uint32_t)v;
        } else if (field <= 4) {                      // field 0, or a known field's wrong type
            return HQ_E_INVAL;
        } else if (!r.skip(wt)) {
            return HQ_E_INVAL;
        }
    }
    s.close();
    bi.n_messages = count;
    *n_spans = s.n;
    if (info) *info = bi;
    return spans && s.n > cap ? HQ_E_STATE : HQ_OK;
}
