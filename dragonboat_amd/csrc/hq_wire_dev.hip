// hq_wire_dev.hip — raftpb.Message decode on the device (include/hipquorum.h "wire decode on the
// device"): the spans hq_wire_frame_batch (hq_wire_frame.cpp) cut out of MessageBatch bytes,
// decoded into hq_wire_message records, one wave per span and one lane per message. The reader is
// hq_wire_codec.h's, the one the host decodes with. No byte outside a span is read, and the kernel
// waits on nothing but its own workgroup's two barriers.
//
// The device mode of hq_wire (hq_wire_attach_device) follows in the same file: the decoded records
// keyed by the worker's handle through a device hash table, sorted with the step's local events by
// (handle, category), turned into rows and per-handle offsets, and handed to the device step
// (hq_worker_step_device_rows) without returning to the host. With the framing on the device
// (hq_wire_set_device_framing) the step first frames the queued batches (hq_wire_frame_dev.hip),
// and the decode takes the spans where the framing left them.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <new>

#include "hq_dstep.h"
#include "hq_internal.h"
#include "hq_wire_codec.h"
#include "hq_wire_dev.h"

namespace {

using hqw::kEmptyKey;
using hqw::kSnapshotReceived;
using hqw::Slot;

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;   // a wave per span

// A wave's share of LDS: its span's bytes behind the low 4 bits of the span's address (so that a
// 16-byte word of memory is a 16-byte word of the stage), then where the hop found each message.
struct WaveStage {
    uint4 bytes[(HQ_WIRE_SPAN_BYTES + 16) / 16];
    uint32_t pos[HQ_WIRE_SPAN_MESSAGES];      // a message's body, from the span's first byte
    uint32_t len[HQ_WIRE_SPAN_MESSAGES];
    uint32_t framed;                          // the headers are where the span says
    uint32_t pad[3];
};

// the decode kernel's arguments; REC (the device mode): the records go out as the wire's 56-byte
// events with their batch in `key` and their entry count in `pad2`, the cluster ids aside, and a
// rejected message flags its batch
struct DecodeK {
    const uint8_t *bytes;
    uint64_t len;
    const hq_wire_span *spans;
    uint64_t n_spans;
    hq_wire_message *out;
    uint8_t *status;
    uint64_t n_messages;
    const uint32_t *span_batch;
    uint32_t *bad;
    hqs::WireEvent *recs;
    uint64_t *cids;
};

template <bool REC>
__global__ void __launch_bounds__(kThreads) k_wire_decode(const DecodeK a) {
    __shared__ WaveStage stage[kWaves];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t s = (uint64_t)blockIdx.x * kWaves + wave;
    WaveStage &st = stage[wave];

    hq_wire_span sp{};
    if (s < a.n_spans) sp = a.spans[s];
    const bool large = (sp.flags & HQ_WIRE_SPAN_LARGE) != 0;
    // a span this kernel can take: within the buffer, and within a wave's stage unless large
    const bool valid = sp.count >= 1 && sp.count <= HQ_WIRE_SPAN_MESSAGES && sp.offset <= a.len &&
                       sp.len <= a.len - sp.offset &&
                       (large ? sp.count == 1 : sp.len <= HQ_WIRE_SPAN_BYTES);
    const uint32_t count = sp.count <= HQ_WIRE_SPAN_MESSAGES ? sp.count : HQ_WIRE_SPAN_MESSAGES;
    const uint8_t *const g = a.bytes + sp.offset;
    const uint32_t L = (uint32_t)sp.len;                      // (staged spans: <= 4096)
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(g) & 15u);
    uint8_t *const sb = reinterpret_cast<uint8_t *>(st.bytes);

    // stage: whole 16-byte words of memory that lie inside the span as such, the span's ragged
    // first and last word byte by byte (nothing outside the span is read)
    if (valid && !large) {
        const uint4 *const g16 = reinterpret_cast<const uint4 *>(g - sh);
        const uint32_t words = (sh + L + 15) / 16;
        for (uint32_t c = lane; c < words; c += 64) {
            const uint32_t b0 = c * 16;
            if (b0 >= sh && b0 + 16 <= sh + L) {
                st.bytes[c] = g16[c];
            } else {
                for (uint32_t j = 0; j < 16; ++j)
                    if (b0 + j >= sh && b0 + j < sh + L) sb[b0 + j] = g[b0 + j - sh];
            }
        }
    }
    __syncthreads();

    // hop: one lane finds the span's headers
    if (valid && !large && lane == 0) {
        const uint8_t *const b = sb + sh;
        uint32_t p = 0, k = 0;
        for (; k < count; ++k) {
            uint64_t n;
            if (!hqw::header<uint32_t>(b, p, L, n)) break;
            st.pos[k] = p;
            st.len[k] = (uint32_t)n;
            p += (uint32_t)n;
        }
        st.framed = k == count && p == L;
    }
    __syncthreads();

    if (s >= a.n_spans || lane >= count) return;
    const uint64_t i = (uint64_t)sp.first + lane;
    if (i >= a.n_messages) return;
    bool ok = false;
    hq_wire_message m;
    hqw::error why;                                   // (the host's to put in words; unused here)
    if (valid && !large) {
        if (st.framed) ok = hqw::decode_message<uint32_t>(sb + sh + st.pos[lane], st.len[lane], m, why);
    } else if (valid) {                               // one message, one lane, from memory
        uint64_t p = 0, n;
        if (hqw::header<uint64_t>(g, p, sp.len, n) && p + n == sp.len)
            ok = hqw::decode_message<uint64_t>(g + p, n, m, why);
    }
    if (REC) {
        const uint32_t batch = a.span_batch[s];
        hqs::WireEvent r{};
        r.key = batch;
        r.cat = 1;
        r.kind = HQ_EV_MESSAGE;
        if (ok) {
            r.reject = m.ev.reject != 0;
            r.type = m.ev.type;
            r.pad2 = m.n_entries;
            r.from = m.ev.from;
            r.term = m.ev.term;
            r.log_index = m.ev.log_index;
            r.hint = m.ev.hint;
            r.hint_high = m.ev.hint_high;
            a.cids[i] = m.cluster_id;
        } else {
            a.bad[batch] = 1;                         // the whole batch goes (k_wire_keys)
        }
        a.recs[i] = r;
    } else {
        if (ok) a.out[i] = m;
        a.status[i] = ok ? 0 : 1;
    }
}

// ---- the device mode: keys, sort, rows ----

struct KeysK {
    const hqs::WireEvent *recs;
    const uint64_t *cids;
    const uint32_t *bad;
    uint64_t n_msgs, n;                               // records: the messages, then the locals
    const Slot *slots;
    uint64_t n_slots;                                 // a power of two
    uint32_t has_empty, empty_val;
    uint32_t sentinel;                                // 4 * groups: sorts behind every handle
    uint32_t *keys, *vals;
    unsigned long long *counters;                     // messages, entries, snapshot_received,
};                                                    // dropped_no_cluster

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// every record's sort key, handle * 4 + category, or the sentinel for a record that is dropped: a
// message of a batch with a malformed message, a SnapshotReceived, a cluster the worker does not
// run. The counters are the host path's (hq_wire_add_batch), for the batches that stay.
__global__ void __launch_bounds__(256) k_wire_keys(const KeysK a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long c[4] = {0, 0, 0, 0};
    if (i < a.n) {
        const hqs::WireEvent r = a.recs[i];
        uint32_t key = a.sentinel;
        if (i >= a.n_msgs) {                          // a local event: its handle resolved already
            key = r.key * 4 + r.cat;
        } else if (!a.bad[r.key]) {
            c[0] = 1;
            c[1] = r.pad2;
            if (r.type == kSnapshotReceived) {
                c[2] = 1;
            } else {
                uint32_t h = 0;
                if (hqw::find(a.slots, a.n_slots, a.has_empty, a.empty_val, a.cids[i], h)) key = h * 4 + 1;
                else c[3] = 1;
            }
        }
        a.keys[i] = key;
        a.vals[i] = (uint32_t)i;
    }
    for (int k = 0; k < 4; ++k) {
        const unsigned long long v = wave_sum(c[k]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&a.counters[k], v);
    }
}

// offsets[h] = the first sorted record whose key is at least 4 h, h = 0 .. n_groups (the last: the
// records that stay)
__global__ void __launch_bounds__(256) k_wire_offsets(const uint32_t *keys, uint64_t n,
                                                      uint64_t n_groups, uint64_t *offsets) {
    const uint64_t h = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (h > n_groups) return;
    const uint64_t want = h * 4;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    offsets[h] = lo;
}

// the sorted records that stay, as the step's rows
__global__ void __launch_bounds__(256) k_wire_rows(const hqs::WireEvent *recs, const uint32_t *vals,
                                                   const uint64_t *n_rows, hq_event *events) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= *n_rows) return;
    events[j] = hqs::to_event(recs[vals[j]]);
}

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct StageBlock {                                   // pinned staging: never moved once allocated
    uint8_t *host = nullptr, *dev = nullptr;
    size_t cap = 0, fill = 0;
};

}  // namespace

extern "C" int hq_wire_decode_dev(hq_ctx *ctx, const uint8_t *bytes, uint64_t len,
                                  const hq_wire_span *spans, uint64_t n_spans, hq_wire_message *out,
                                  uint8_t *status, uint64_t n_messages) {
    if (!ctx) return HQ_E_INVAL;
    if (n_spans == 0 || n_messages == 0) return HQ_OK;
    if (!spans || !out || !status || (!bytes && len))
        return hq::fail(ctx, HQ_E_INVAL, "hq_wire_decode_dev: NULL argument");
    const uint64_t blocks = (n_spans + kWaves - 1) / kWaves;
    if (blocks > 0x7FFFFFFFull)
        return hq::fail(ctx, HQ_E_INVAL, "hq_wire_decode_dev: more than 2^33 spans");
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    DecodeK k{};
    k.bytes = bytes;
    k.len = len;
    k.spans = spans;
    k.n_spans = n_spans;
    k.out = out;
    k.status = status;
    k.n_messages = n_messages;
    hipLaunchKernelGGL(k_wire_decode<false>, dim3((uint32_t)blocks), dim3(kThreads), 0, ctx->stream,
                       k);
    return hq::post_launch(ctx, "hq_wire_decode_dev");
}

// ------------------------------------------------------------------- the device mode ----------
struct hq_wire_dev {
    hq_worker *worker = nullptr;
    hq_ctx *ctx = nullptr;
    std::string err;
    // the queued batches: spans with absolute device addresses (the decode kernel's bytes = 0)
    std::vector<hq_wire_span> spans;
    std::vector<uint32_t> span_batch;
    std::vector<uint32_t> batch_index;                // hq_wire_add_batch's call index
    std::vector<uint64_t> batch_len;
    uint64_t n_msgs = 0;
    std::vector<StageBlock> stage;
    std::vector<uint32_t> rejected;
    // the handle table: built from the worker's live groups, extended when it has gained some and
    // rebuilt when groups were started or stopped (the worker's epoch has moved)
    std::vector<Slot> slots;
    uint64_t known = 0;                               // handles in the table
    uint64_t epoch = 0;                               // the worker's epoch the table was built under
    bool has_empty = false;
    uint32_t empty_val = 0;
    DevBuf d_slots, d_spans, d_span_batch, d_bad, d_recs, d_cids, d_keys, d_vals, d_events, d_offsets,
        d_counters, d_tmp;
    uint64_t *h_read = nullptr;                       // pinned: the counters and the rows' count
    uint32_t *h_bad = nullptr;
    size_t h_bad_cap = 0;
    // the framing on the device (hq_wire_set_device_framing): the batches queued as they came,
    // where the device reads them (refs: absolute addresses) and where the host does
    bool framing = false;
    uint64_t deployment_id = 0;
    std::vector<hq_wire_batch_ref> refs;
    std::vector<const uint8_t *> host_bytes;
    std::vector<uint8_t> frame_rejected;              // per batch: a framing error
    DevBuf d_refs, d_frame;                           // d_frame: totals, results, void segments
    uint8_t *h_frame = nullptr;                       // pinned: d_frame read back
    size_t h_frame_cap = 0;
    uint64_t frame_stats[4] = {0, 0, 0, 0};

    int fail(int code, const std::string &m) {
        err = m;
        return code;
    }
    int hip(hipError_t e, const char *what) {
        if (e == hipSuccess) return HQ_OK;
        return fail(e == hipErrorOutOfMemory ? HQ_E_NOMEM : HQ_E_DEVICE,
                    std::string(what) + ": " + hipGetErrorString(e));
    }
    // a device buffer of at least `bytes` (contents not kept)
    int ensure(DevBuf &b, size_t bytes) {
        if (bytes <= b.cap) return HQ_OK;
        if (b.p) (void)hipFree(b.p);
        b.p = nullptr;
        b.cap = 0;
        const size_t want = std::max<size_t>(bytes + bytes / 2, 4096);
        const int rc = hip(hipMalloc(&b.p, want), "hq_wire device buffer");
        if (!rc) b.cap = want;
        return rc;
    }
    // an id's first handle stays
    void insert(uint64_t id, uint32_t h) {
        uint32_t first;
        if (hqw::find(slots.data(), slots.size(), has_empty, empty_val, id, first)) return;
        if (id == kEmptyKey) {
            has_empty = true;
            empty_val = h;
            return;
        }
        const uint64_t mask = slots.size() - 1;
        uint64_t s = hqw::hash_id(id) & mask;
        while (slots[s].key != kEmptyKey) s = (s + 1) & mask;
        slots[s] = Slot{id, h, 0};
    }
    // the table holds every live group of the worker (load <= 1/2); uploaded when it has changed.
    // Handles keep their clusters while the worker's epoch stands: the table is then only extended;
    // once it has moved (hq_worker_start_groups / _stop_groups) the whole table is rebuilt from the
    // live handles, so a stopped cluster resolves to nothing and a restarted one to its new handle
    int extend(uint64_t G) {
        const uint64_t now = hq_worker_epoch(worker);
        if (G == known && now == epoch && d_slots.p) return HQ_OK;
        size_t want = 1024;
        while (want < 2 * G) want *= 2;
        std::vector<uint64_t> ids(G);
        std::vector<uint8_t> live(G);
        int rc = hq_worker_cluster_ids(worker, 0, G, ids.data());
        if (!rc) rc = hq_worker_live_handles(worker, 0, G, live.data());
        if (rc) return fail(rc, "hq_wire_step_device: the worker's groups");
        if (want != slots.size() || now != epoch) {
            slots.assign(want, Slot{kEmptyKey, 0, 0});
            has_empty = false;
            known = 0;
        }
        for (uint64_t h = known; h < G; ++h)
            if (live[h]) insert(ids[h], (uint32_t)h);
        known = G;
        epoch = now;
        rc = ensure(d_slots, slots.size() * sizeof(Slot));
        if (!rc)
            rc = hip(hipMemcpyAsync(d_slots.p, slots.data(), slots.size() * sizeof(Slot),
                                    hipMemcpyHostToDevice, ctx->stream), "hq_wire table upload");
        return rc;
    }
};

int hq_wire_dev_open(hq_worker *worker, hq_wire_dev **out) {
    hq_ctx *ctx = hq_worker_device_ctx(worker);
    if (!ctx || !out) return HQ_E_INVAL;
    hq_wire_dev *d = new (std::nothrow) hq_wire_dev();
    if (!d) return HQ_E_NOMEM;
    d->worker = worker;
    d->ctx = ctx;
    int rc = d->hip(hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc) rc = d->hip(hipHostMalloc(reinterpret_cast<void **>(&d->h_read), 64, hipHostMallocDefault),
                         "hq_wire pinned readback");
    if (rc) {
        delete d;
        return rc;
    }
    *out = d;
    return HQ_OK;
}

void hq_wire_dev_close(hq_wire_dev *d) {
    if (!d) return;
    (void)hipSetDevice(d->ctx->device);
    (void)hipStreamSynchronize(d->ctx->stream);
    for (DevBuf *b : {&d->d_slots, &d->d_spans, &d->d_span_batch, &d->d_bad, &d->d_recs, &d->d_cids,
                      &d->d_keys, &d->d_vals, &d->d_events, &d->d_offsets, &d->d_counters, &d->d_tmp,
                      &d->d_refs, &d->d_frame})
        if (b->p) (void)hipFree(b->p);
    for (StageBlock &s : d->stage)
        if (s.host) (void)hipHostFree(s.host);
    if (d->h_read) (void)hipHostFree(d->h_read);
    if (d->h_bad) (void)hipHostFree(d->h_bad);
    if (d->h_frame) (void)hipHostFree(d->h_frame);
    delete d;
}

const char *hq_wire_dev_error(const hq_wire_dev *d) { return d ? d->err.c_str() : ""; }

void hq_wire_dev_reset(hq_wire_dev *d) {
    d->spans.clear();
    d->span_batch.clear();
    d->batch_index.clear();
    d->batch_len.clear();
    d->n_msgs = 0;
    d->rejected.clear();
    d->refs.clear();
    d->host_bytes.clear();
    for (StageBlock &s : d->stage) s.fill = 0;
}

void hq_wire_dev_set_framing(hq_wire_dev *d, bool on, uint64_t deployment_id) {
    d->framing = on;
    d->deployment_id = deployment_id;
}

bool hq_wire_dev_framing(const hq_wire_dev *d) { return d->framing; }

void hq_wire_dev_frame_stats(const hq_wire_dev *d, uint64_t out[4]) {
    for (int k = 0; k < 4; ++k) out[k] = d->frame_stats[k];
}

// Where the device reads a batch: device memory as it is, pinned memory where the device maps it,
// any other memory copied into the pinned staging
static int place_batch(hq_wire_dev *d, const uint8_t *bytes, size_t len, const uint8_t **dev_out,
                       const uint8_t **host_out = nullptr) {
    int rc = d->hip(hipSetDevice(d->ctx->device), "hipSetDevice");
    if (rc) return rc;
    const uint8_t *dev = static_cast<const uint8_t *>(hq::device_view(bytes));
    if (host_out) *host_out = bytes;
    if (!dev) {
        StageBlock *blk = nullptr;
        for (StageBlock &s : d->stage)
            if (s.cap - s.fill >= len + 16) blk = &s;
        if (!blk) {
            StageBlock s;
            s.cap = std::max<size_t>(len + 16, size_t(4) << 20);
            rc = d->hip(hipHostMalloc(reinterpret_cast<void **>(&s.host), s.cap, hipHostMallocDefault),
                        "hq_wire pinned staging");
            if (!rc)
                rc = d->hip(hipHostGetDevicePointer(reinterpret_cast<void **>(&s.dev), s.host, 0),
                            "hq_wire pinned staging");
            if (rc) {
                if (s.host) (void)hipHostFree(s.host);
                return rc;
            }
            d->stage.push_back(s);
            blk = &d->stage.back();
        }
        std::memcpy(blk->host + blk->fill, bytes, len);
        dev = blk->dev + blk->fill;
        if (host_out) *host_out = blk->host + blk->fill;   // (the caller's bytes may go)
        blk->fill += (len + 15) & ~size_t(15);
    }
    *dev_out = dev;
    return HQ_OK;
}

int hq_wire_dev_queue(hq_wire_dev *d, const uint8_t *bytes, size_t len, uint32_t index) {
    const uint8_t *dev = nullptr, *host = nullptr;
    if (len) {
        const int rc = place_batch(d, bytes, len, &dev, &host);
        if (rc) return rc;
    }
    d->batch_index.push_back(index);
    d->batch_len.push_back(len);
    d->refs.push_back(hq_wire_batch_ref{reinterpret_cast<uintptr_t>(dev), len});
    d->host_bytes.push_back(host);                    // (should the step be framed here after all)
    return HQ_OK;
}

int hq_wire_dev_add_batch(hq_wire_dev *d, const uint8_t *bytes, size_t len, const hq_wire_span *spans,
                          uint64_t n_spans, uint64_t n_messages, uint32_t index) {
    if (d->n_msgs + n_messages >= (1ull << 31))
        return d->fail(HQ_E_STATE, "hq_wire_add_batch: a device step holds < 2^31 messages");
    const uint8_t *dev = nullptr;
    const int rc = place_batch(d, bytes, len, &dev);
    if (rc) return rc;
    const uint32_t b = (uint32_t)d->batch_index.size();
    d->batch_index.push_back(index);
    d->batch_len.push_back(len);
    for (uint64_t i = 0; i < n_spans; ++i) {
        hq_wire_span s = spans[i];
        s.offset += reinterpret_cast<uintptr_t>(dev);
        s.first += (uint32_t)d->n_msgs;
        d->spans.push_back(s);
        d->span_batch.push_back(b);
    }
    d->n_msgs += n_messages;
    return HQ_OK;
}

// one queued batch after hq_wire_frame_batch's verdict: counted, checked and its spans queued as
// hq_wire.cpp's add_batch_device and hq_wire_dev_add_batch do
static void queue_host_framed(hq_wire_dev *d, uint32_t b, const hq_wire_span *spans, uint64_t n_spans,
                              const hq_wire_batch_info &bi, hq_wire_stats *add) {
    add->batches++;
    add->bytes += d->batch_len[b];
    if (bi.deployment_id != d->deployment_id || bi.bin_ver != HQ_RPC_BIN_VERSION) {
        add->dropped_batches++;
        add->dropped_messages += bi.n_messages;
        return;
    }
    for (uint64_t i = 0; i < n_spans; ++i) {
        hq_wire_span s = spans[i];
        s.offset += d->refs[b].offset;
        s.first += (uint32_t)d->n_msgs;
        d->spans.push_back(s);
        d->span_batch.push_back(b);
    }
    d->n_msgs += bi.n_messages;
}

// The queued batches framed on the device: their spans in d_spans / d_span_batch (*on_device), the
// results read back and applied. With a batch that came back unconfirmed or with spans that did
// not fit, the whole step is framed here instead, into d->spans (arrival order stays).
static int frame_queued(hq_wire_dev *d, hq_wire_stats *add, bool *on_device, uint64_t *n_spans) {
    hq_ctx *ctx = d->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t nb = d->refs.size();
    const uint32_t S = HQ_WIRE_FRAME_SEGMENT, region = S / 128 + 8;
    uint64_t segs = 0;
    for (const hq_wire_batch_ref &r : d->refs) segs += (r.len + S - 1) / S;
    const uint64_t span_cap = segs * region;          // (what the segments' regions hold)
    const size_t o_results = 16, o_voids = o_results + nb * sizeof(hq_wire_frame_result),
                 frame_bytes = o_voids + nb * 4;
    d->spans.clear();
    d->span_batch.clear();
    d->n_msgs = 0;
    d->frame_rejected.assign(nb, 0);
    d->frame_stats[0] = segs;
    d->frame_stats[1] = d->frame_stats[2] = 0;
    *on_device = false;
    *n_spans = 0;
    if (!nb) return HQ_OK;
    int rc = d->hip(hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc) rc = d->ensure(d->d_refs, nb * sizeof(hq_wire_batch_ref));
    if (!rc) rc = d->ensure(d->d_frame, frame_bytes);
    if (!rc) rc = d->ensure(d->d_spans, span_cap * sizeof(hq_wire_span));
    if (!rc) rc = d->ensure(d->d_span_batch, span_cap * 4);
    if (!rc && frame_bytes > d->h_frame_cap) {
        if (d->h_frame) (void)hipHostFree(d->h_frame);
        d->h_frame = nullptr;
        d->h_frame_cap = 0;
        rc = d->hip(hipHostMalloc(reinterpret_cast<void **>(&d->h_frame), 2 * frame_bytes,
                                  hipHostMallocDefault), "hq_wire pinned readback");
        if (!rc) d->h_frame_cap = 2 * frame_bytes;
    }
    if (!rc)
        rc = d->hip(hipMemcpyAsync(d->d_refs.p, d->refs.data(), nb * sizeof(hq_wire_batch_ref),
                                   hipMemcpyHostToDevice, st), "hq_wire H2D");
    if (rc) return rc;
    uint8_t *const f = static_cast<uint8_t *>(d->d_frame.p);
    // the refs carry absolute addresses, so the buffer is all of memory
    rc = hq_wire_frame_launch(ctx, nullptr, UINT64_MAX, static_cast<const hq_wire_batch_ref *>(d->d_refs.p),
                              nb, S, segs, static_cast<hq_wire_span *>(d->d_spans.p), span_cap,
                              static_cast<uint32_t *>(d->d_span_batch.p),
                              reinterpret_cast<hq_wire_frame_result *>(f + o_results),
                              reinterpret_cast<uint64_t *>(f), reinterpret_cast<uint32_t *>(f + o_voids),
                              &d->deployment_id);
    // one readback: the sort needs the step's size on the host
    if (!rc) rc = hq::check_hip(ctx, hipMemcpyAsync(d->h_frame, f, frame_bytes, hipMemcpyDeviceToHost, st),
                                "hq_wire D2H");
    if (!rc) rc = hq::check_hip(ctx, hipStreamSynchronize(st), "hq_wire sync");
    if (rc) return d->fail(rc, ctx->err);
    const uint64_t *const totals = reinterpret_cast<const uint64_t *>(d->h_frame);
    const hq_wire_frame_result *const res =
        reinterpret_cast<const hq_wire_frame_result *>(d->h_frame + o_results);
    const uint32_t *const voids = reinterpret_cast<const uint32_t *>(d->h_frame + o_voids);
    for (uint64_t b = 0; b < nb; ++b) {
        d->frame_stats[1] += voids[b];
        d->frame_stats[2] += res[b].status >= 2;
    }
    if (d->frame_stats[2]) {                          // rare: framed here, as without the mode
        d->frame_stats[3]++;
        std::vector<hq_wire_span> spans(1024);
        for (uint64_t b = 0; b < nb; ++b) {
            hq_wire_batch_info bi;
            uint64_t n = 0;
            int frc = hq_wire_frame_batch(d->host_bytes[b], d->batch_len[b], 0, spans.data(), spans.size(),
                                          &n, &bi);
            if (frc == HQ_E_STATE) {
                spans.resize(n);
                frc = hq_wire_frame_batch(d->host_bytes[b], d->batch_len[b], 0, spans.data(), spans.size(),
                                          &n, &bi);
            }
            if (frc) d->frame_rejected[b] = 1;
            else queue_host_framed(d, (uint32_t)b, spans.data(), n, bi, add);
        }
        *n_spans = d->spans.size();
        return HQ_OK;
    }
    for (uint64_t b = 0; b < nb; ++b) {
        if (res[b].status) {
            d->frame_rejected[b] = 1;
            continue;
        }
        hq_wire_batch_info bi{};
        bi.n_messages = res[b].n_messages;
        bi.deployment_id = res[b].deployment_id;
        bi.bin_ver = res[b].bin_ver;
        queue_host_framed(d, (uint32_t)b, nullptr, 0, bi, add);
    }
    if (d->n_msgs != totals[0])
        return d->fail(HQ_E_DEVICE, "hq_wire_step_device: the framing's totals differ from its results");
    *on_device = true;
    *n_spans = totals[1];
    return HQ_OK;
}

int hq_wire_dev_step(hq_wire_dev *d, const hqs::WireEvent *locals, uint64_t n_locals,
                     hq_step_output *out, uint64_t counters[4], const uint32_t **rejected,
                     uint64_t *n_rejected, uint64_t *rejected_bytes, uint64_t *n_bad_message,
                     hq_wire_stats *add) {
    hq_ctx *ctx = d->ctx;
    hipStream_t st = ctx->stream;
    std::memset(out, 0, sizeof *out);
    std::memset(counters, 0, 4 * sizeof(uint64_t));
    *add = hq_wire_stats{};
    d->rejected.clear();
    *rejected = nullptr;
    *n_rejected = *rejected_bytes = *n_bad_message = 0;
    int rc = HQ_OK;
    bool spans_on_device = false;
    uint64_t ns = d->spans.size();
    if (d->framing) {
        rc = frame_queued(d, add, &spans_on_device, &ns);
        if (rc) return rc;
        for (uint64_t b = 0; b < d->frame_rejected.size(); ++b)   // (should the step end early)
            if (d->frame_rejected[b]) d->rejected.push_back(d->batch_index[b]);
        *rejected = d->rejected.data();
        *n_rejected = d->rejected.size();
    }
    const uint64_t nm = d->n_msgs, N = nm + n_locals, nb = d->batch_index.size();
    uint64_t G = 0;
    rc = hq_worker_group_count(d->worker, &G);
    if (rc) return d->fail(rc, "hq_wire_step_device: the worker's groups");
    if (N == 0 || G == 0) return HQ_OK;
    if (N >= (1ull << 31) || G >= (1ull << 30))
        return d->fail(HQ_E_STATE, "hq_wire_step_device: a step holds < 2^31 records, a worker < 2^30 groups");
    rc = d->hip(hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc) rc = d->extend(G);
    // the device buffers of the step
    size_t tmp = 0;
    const uint32_t sentinel = (uint32_t)(G * 4);
    int end_bit = 1;
    while (end_bit < 32 && (sentinel >> end_bit)) ++end_bit;
    if (!rc) rc = d->ensure(d->d_keys, 2 * N * 4);
    if (!rc) rc = d->ensure(d->d_vals, 2 * N * 4);
    uint32_t *keys_in = static_cast<uint32_t *>(d->d_keys.p), *keys_out = keys_in + N;
    uint32_t *vals_in = static_cast<uint32_t *>(d->d_vals.p), *vals_out = vals_in + N;
    if (!rc)
        rc = d->hip(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, keys_in, keys_out, vals_in,
                                                       vals_out, (int)N, 0, end_bit, st),
                    "hipcub sort size");
    if (!rc) rc = d->ensure(d->d_tmp, tmp);
    if (!rc && !spans_on_device) rc = d->ensure(d->d_spans, ns * sizeof(hq_wire_span));
    if (!rc && !spans_on_device) rc = d->ensure(d->d_span_batch, ns * 4);
    if (!rc) rc = d->ensure(d->d_bad, (nb + 1) * 4);
    if (!rc) rc = d->ensure(d->d_recs, N * sizeof(hqs::WireEvent));
    if (!rc) rc = d->ensure(d->d_cids, (nm + 1) * 8);
    if (!rc) rc = d->ensure(d->d_events, N * sizeof(hq_event));
    if (!rc) rc = d->ensure(d->d_offsets, (G + 1) * 8);
    if (!rc) rc = d->ensure(d->d_counters, 64);
    if (!rc && nb > d->h_bad_cap) {
        if (d->h_bad) (void)hipHostFree(d->h_bad);
        d->h_bad = nullptr;
        d->h_bad_cap = 0;
        rc = d->hip(hipHostMalloc(reinterpret_cast<void **>(&d->h_bad), nb * 2 * 4, hipHostMallocDefault),
                    "hq_wire pinned readback");
        if (!rc) d->h_bad_cap = nb * 2;
    }
    if (rc) return rc;
    hqs::WireEvent *recs = static_cast<hqs::WireEvent *>(d->d_recs.p);
    auto h2d = [&](void *dst, const void *src, size_t bytes) {
        if (!rc && bytes)
            rc = d->hip(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st), "hq_wire H2D");
    };
    if (!spans_on_device) {
        h2d(d->d_spans.p, d->spans.data(), ns * sizeof(hq_wire_span));
        h2d(d->d_span_batch.p, d->span_batch.data(), ns * 4);
    }
    h2d(recs + nm, locals, n_locals * sizeof(hqs::WireEvent));
    if (!rc) rc = d->hip(hipMemsetAsync(d->d_bad.p, 0, (nb + 1) * 4, st), "memset");
    if (!rc) rc = d->hip(hipMemsetAsync(d->d_counters.p, 0, 64, st), "memset");
    if (rc) return rc;
    // decode: the spans carry absolute addresses, so the buffer is all of memory
    if (ns) {
        DecodeK k{};
        k.bytes = nullptr;
        k.len = UINT64_MAX;
        k.spans = static_cast<const hq_wire_span *>(d->d_spans.p);
        k.n_spans = ns;
        k.n_messages = nm;
        k.span_batch = static_cast<const uint32_t *>(d->d_span_batch.p);
        k.bad = static_cast<uint32_t *>(d->d_bad.p);
        k.recs = recs;
        k.cids = static_cast<uint64_t *>(d->d_cids.p);
        rc = hq::pre_launch(ctx);
        if (rc) return d->fail(rc, ctx->err);
        hipLaunchKernelGGL(k_wire_decode<true>, dim3((uint32_t)((ns + kWaves - 1) / kWaves)),
                           dim3(kThreads), 0, st, k);
        rc = hq::post_launch(ctx, "k_wire_decode");
        if (rc) return d->fail(rc, ctx->err);
    }
    KeysK kk{};
    kk.recs = recs;
    kk.cids = static_cast<const uint64_t *>(d->d_cids.p);
    kk.bad = static_cast<const uint32_t *>(d->d_bad.p);
    kk.n_msgs = nm;
    kk.n = N;
    kk.slots = static_cast<const Slot *>(d->d_slots.p);
    kk.n_slots = d->slots.size();
    kk.has_empty = d->has_empty;
    kk.empty_val = d->empty_val;
    kk.sentinel = sentinel;
    kk.keys = keys_in;
    kk.vals = vals_in;
    kk.counters = static_cast<unsigned long long *>(d->d_counters.p);
    uint64_t *offsets = static_cast<uint64_t *>(d->d_offsets.p);
    hq_event *events = static_cast<hq_event *>(d->d_events.p);
    rc = hq::pre_launch(ctx);
    if (rc) return d->fail(rc, ctx->err);
    hipLaunchKernelGGL(k_wire_keys, dim3((uint32_t)((N + 255) / 256)), dim3(256), 0, st, kk);
    rc = hq::post_launch(ctx, "k_wire_keys");
    // stable, over the bits the key needs: node.handleEvents order per handle, arrival order
    // within a category
    if (!rc)
        rc = hq::check_hip(ctx, hipcub::DeviceRadixSort::SortPairs(d->d_tmp.p, tmp, keys_in, keys_out,
                                                                   vals_in, vals_out, (int)N, 0,
                                                                   end_bit, st), "hipcub sort");
    if (!rc) {
        hipLaunchKernelGGL(k_wire_offsets, dim3((uint32_t)((G + 1 + 255) / 256)), dim3(256), 0, st,
                           keys_out, N, G, offsets);
        rc = hq::post_launch(ctx, "k_wire_offsets");
    }
    if (!rc) {
        hipLaunchKernelGGL(k_wire_rows, dim3((uint32_t)((N + 255) / 256)), dim3(256), 0, st, recs,
                           vals_out, offsets + G, events);
        rc = hq::post_launch(ctx, "k_wire_rows");
    }
    // the counters, the rows' count and the batches' flags back: the step's size is the host's to
    // know (the device step sizes its buffers by it)
    if (!rc)
        rc = hq::check_hip(ctx, hipMemcpyAsync(d->h_read, d->d_counters.p, 32, hipMemcpyDeviceToHost, st),
                           "hq_wire D2H");
    if (!rc)
        rc = hq::check_hip(ctx, hipMemcpyAsync(d->h_read + 4, offsets + G, 8, hipMemcpyDeviceToHost, st),
                           "hq_wire D2H");
    if (!rc && nb)
        rc = hq::check_hip(ctx, hipMemcpyAsync(d->h_bad, d->d_bad.p, nb * 4, hipMemcpyDeviceToHost, st),
                           "hq_wire D2H");
    if (!rc) rc = hq::check_hip(ctx, hipStreamSynchronize(st), "hq_wire sync");
    if (rc) return d->fail(rc, ctx->err);
    for (int k = 0; k < 4; ++k) counters[k] = d->h_read[k];
    d->rejected.clear();
    for (uint64_t b = 0; b < nb; ++b) {
        if (d->framing && d->frame_rejected[b]) {     // a framing error: counted nowhere
            d->rejected.push_back(d->batch_index[b]);
        } else if (d->h_bad[b]) {
            d->rejected.push_back(d->batch_index[b]);
            *rejected_bytes += d->batch_len[b];
            ++*n_bad_message;
        }
    }
    *rejected = d->rejected.data();
    *n_rejected = d->rejected.size();
    const uint64_t n_rows = d->h_read[4];
    if (n_rows == 0) return HQ_OK;
    rc = hq_worker_step_device_rows(d->worker, G, nullptr, offsets, events, n_rows, out);
    if (rc) return d->fail(rc, hq_worker_last_error(d->worker));
    return HQ_OK;
}
