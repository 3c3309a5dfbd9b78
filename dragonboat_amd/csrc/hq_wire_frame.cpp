// hq_wire_frame.cpp — the host's share of the device wire decode: a raftpb.MessageBatch framed
// into spans (include/hipquorum.h "wire decode on the device"). Plain C++; no HIP, no worker. The
// batch is walked by hqw::walk_batch (hq_wire_codec.h); a `requests` field is only hopped over:
// what is inside a message is the decode kernel's business (hq_wire_dev.hip).
#include "../../include/hipquorum.h"
#include "hq_wire_codec.h"

namespace {

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
    hq_wire_batch_info bi;
    Spans s{spans, cap};
    const int rc = hqw::walk_batch(
        bytes, len, bi,
        [&](size_t field, size_t body, size_t n) {
            if (bi.n_messages >= UINT32_MAX) return HQ_E_INVAL;   // (a span's `first` is 32 bits)
            s.add(base + field, body + n - field, (uint32_t)bi.n_messages);
            return HQ_OK;
        },
        [&] { s.close(); });                          // a span is `requests` fields back to back
    if (rc) return rc;
    s.close();
    *n_spans = s.n;
    if (info) *info = bi;
    return spans && s.n > cap ? HQ_E_STATE : HQ_OK;
}
