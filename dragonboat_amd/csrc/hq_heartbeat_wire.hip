// hq_heartbeat_wire.hip — the leader heartbeats of a device worker marshalled on the device
// (hq_worker_heartbeat_batches, include/hipquorum.h "leader heartbeats as MessageBatch bytes"):
// the messages of hq_worker_heartbeats, routed to destination hosts by the worker's route column
// and written as complete MessageBatch byte strings, one run of batches per destination, straight
// into pinned host memory. The sending side of hq_wire_dev.hip. Read-only on the resident state.
//
// On the context's stream behind the last step:
//   k_hbw_words   one lane per listed group: its word (hqhb::word_of, as k_hb_words), its route
//                 row (two 16-byte loads) checked against n_dest, the routed members' mask and the
//                 unrouted count
//   scan          hipcub ExclusiveSum over (routed | unrouted << 36), n + 1 items: each group's
//                 first message ordinal, the totals last. The host reads them (and the error word)
//   k_hbw_desc    per routed message, at its ordinal (group order, then member order): key = dest,
//                 value = pos << 4 | member
//   sort          stable hipcub SortPairs over the bits n_dest needs
//   k_hbw_dests   one lane per destination: its first sorted message (binary search)
//   scan          ExclusiveSum of the destinations' batch counts
//   k_hbw_sizes   one lane per sorted message: its fields again from the state, hb_msg_size, and
//                 the trailer's length when it ends a batch
//   scan          ExclusiveSum: byte offsets, the total last
//   k_hbw_encode  one workgroup per 256 sorted messages = one contiguous byte range: marshalled
//                 into LDS and copied out with 16-byte stores (byte stores for the ragged ends), or
//                 written directly when the range is over kStageBytes. The lane that starts a
//                 batch writes its table entry. Nothing is written when a total is over a
//                 capacity: the host grows the buffer and runs this kernel again
// No spinning, no waiting between workgroups, no atomics but the error word's atomicOr; every
// loop is bounded by a constant or a checked count.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>

#include "hq_heartbeat.h"
#include "hq_heartbeat_wire.h"
#include "hq_sidecar.h"

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kUnroutedShift = 36;               // scan item: routed | unrouted << 36
constexpr uint64_t kRoutedMask = (uint64_t(1) << kUnroutedShift) - 1;
// the encode kernel's LDS budget: 256 messages of 113 bytes are 28,928, so a workgroup's range
// fits unless it holds many trailers (small batch_messages, a long source); then it stores directly
constexpr uint32_t kStageBytes = 32768;

struct HbwK {
    const hq_dgroup *groups;
    const hq_dread *reads;
    const hq_dmember *members;
    uint64_t n_state_groups, n_state_members;
    const uint32_t *list;          // device; NULL: handle i
    uint64_t n;
    const uint16_t *routes;        // device [n_state_groups * 16]
    uint32_t n_dest, bm;           // bm: batch_messages, UINT32_MAX for "one batch"
    uint64_t deployment_id;
    const uint8_t *source;         // device
    uint32_t source_len, trailer_len;
    uint32_t *meta;                // device [n]: routed mask | unrouted << 16
    uint64_t *scan;                // device [n + 1]
    uint32_t *error;               // device
    uint64_t m;                    // routed messages (< 2^31)
    uint16_t *keys_in, *keys;      // device [m]: as written, sorted
    uint32_t *vals_in, *vals;
    uint32_t *dstart;              // device [n_dest + 1]: destination d's first sorted message
    uint64_t *bscan;               // device [n_dest + 1]: batches of the destinations before d
    uint32_t *sizes;               // device [m]
    uint64_t *offs;                // device [m + 1]
    uint8_t *bytes;                // pinned host [bytes_cap]
    hq_heartbeat_batch *batches;   // pinned host [batch_cap]
    uint64_t bytes_cap, batch_cap;
    uint64_t *totals;              // pinned host
};

struct RouteRow {                  // a group's 16 routes
    uint4 a, b;
};

__device__ inline RouteRow load_routes(const uint16_t *routes, uint64_t h) {
    const uint4 *p = reinterpret_cast<const uint4 *>(routes + h * kDMembers);
    return RouteRow{p[0], p[1]};
}

__device__ inline uint32_t route_pair(const RouteRow &r, int w) {   // (w a constant after unrolling)
    switch (w) {
        case 0: return r.a.x;
        case 1: return r.a.y;
        case 2: return r.a.z;
        case 3: return r.a.w;
        case 4: return r.b.x;
        case 5: return r.b.y;
        case 6: return r.b.z;
        default: return r.b.w;
    }
}

struct HbwCount {                  // item i of the first scan; item n: 0
    const uint32_t *meta;
    uint64_t n;
    __host__ __device__ uint64_t operator()(uint64_t i) const {
        if (i >= n) return 0;
        const uint32_t m = meta[i];
#if defined(__HIP_DEVICE_COMPILE__)
        const uint64_t routed = (uint64_t)__popc(m & 0xFFFFu);
#else
        const uint64_t routed = (uint64_t)__builtin_popcount(m & 0xFFFFu);
#endif
        return routed | (uint64_t)(m >> 16) << kUnroutedShift;
    }
};

__host__ __device__ inline uint64_t batches_of(uint64_t messages, uint32_t bm) {
    return (messages + bm - 1) / bm;
}

struct HbwBatches {                // destination d's batches; item n_dest: 0
    const uint32_t *dstart;
    uint32_t n_dest, bm;
    __host__ __device__ uint64_t operator()(uint64_t d) const {
        return d < n_dest ? batches_of((uint64_t)dstart[d + 1] - dstart[d], bm) : 0;
    }
};

struct HbwSize {                   // message j's bytes; item m: 0
    const uint32_t *sizes;
    uint64_t m;
    __host__ __device__ uint64_t operator()(uint64_t j) const { return j < m ? sizes[j] : 0; }
};

__global__ void __launch_bounds__(kBlock) k_hbw_words(HbwK k) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= k.n) return;
    const uint64_t h = k.list ? k.list[i] : i;
    uint32_t meta = 0;
    if (h >= k.n_state_groups) {
        atomicOr(k.error, kHbErrHandle);
    } else {
        uint32_t err = 0;
        uint64_t lo, hi;
        hqhb::GroupRef g;
        const uint32_t to =
            hqhb::word_of(k.groups, k.reads, k.members, k.n_state_members, h, &lo, &hi, &err, &g) &
            0xFFFFu;
        if (!err) {
            // every route of the group's members is checked, whatever the group sends now,
            // before any of them indexes anything
            const RouteRow row = load_routes(k.routes, h);
            uint32_t routed = 0, unrouted = 0;
#pragma unroll
            for (int o = 0; o < (int)kDMembers; ++o) {
                const uint32_t r = (route_pair(row, o >> 1) >> ((o & 1) * 16)) & 0xFFFFu;
                if ((uint32_t)o < g.n_members && r != HQ_ROUTE_NONE && r >= k.n_dest)
                    err |= kHbErrRoute;
                if ((to >> o) & 1) {
                    if (r == HQ_ROUTE_NONE) ++unrouted;
                    else routed |= 1u << o;
                }
            }
            meta = routed | unrouted << 16;
        }
        if (err) {
            atomicOr(k.error, err);
            meta = 0;
        }
    }
    k.meta[i] = meta;
}

__global__ void __launch_bounds__(kBlock) k_hbw_desc(HbwK k) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= k.n) return;
    const uint32_t routed = k.meta[i] & 0xFFFFu;
    if (!routed) return;
    uint64_t at = k.scan[i] & kRoutedMask;
    const uint64_t h = k.list ? k.list[i] : i;        // (checked by k_hbw_words: routed != 0)
    const RouteRow row = load_routes(k.routes, h);
#pragma unroll
    for (int o = 0; o < (int)kDMembers; ++o) {
        if (!((routed >> o) & 1)) continue;
        const uint32_t r = (route_pair(row, o >> 1) >> ((o & 1) * 16)) & 0xFFFFu;
        if (at < k.m) {
            k.keys_in[at] = (uint16_t)r;
            k.vals_in[at] = (uint32_t)i << 4 | (uint32_t)o;
        }
        ++at;
    }
}

__global__ void __launch_bounds__(kBlock) k_hbw_dests(HbwK k) {
    const uint32_t d = blockIdx.x * kBlock + threadIdx.x;
    if (d > k.n_dest) return;
    uint32_t lo = 0, hi = (uint32_t)k.m;              // the first sorted key >= d
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (k.keys[mid] < d) lo = mid + 1;
        else hi = mid;
    }
    k.dstart[d] = lo;
}

// sorted message j: its fields from the state, its destination and its place there
struct HbwMsg {
    hb_fields f;
    uint32_t dest, rank, dest_end;     // rank: j - the destination's first; dest_end: its last + 1
    bool ends_batch;
};

__device__ inline HbwMsg message_of(const HbwK &k, uint32_t j) {
    HbwMsg r;
    const uint32_t v = k.vals[j], pos = v >> 4, o = v & 15u;
    const uint64_t h = k.list ? k.list[pos] : pos;    // (checked by k_hbw_words)
    const hqhb::GroupRef g = hqhb::load_group(k.groups + h);
    const uint64_t *ids = reinterpret_cast<const uint64_t *>(k.groups + h);
    r.f.cluster_id = ids[0];
    r.f.from = ids[1];
    r.f.term = g.term;                                // finalizeMessageTerm
    r.f.hint = r.f.hint_high = 0;
    if (g.n_reads && g.n_reads <= kDReads) {
        const hq_dread *q = k.reads + h * kDReads + (g.n_reads - 1);
        r.f.hint = q->low;
        r.f.hint_high = q->high;
    }
    r.f.to = 0;
    r.f.commit = 0;
    const hq_dmember *m = k.members + g.mem;
    for (uint32_t s = 1; s < g.n_members && s < kDMembers; ++s) {
        const uint64_t *p = reinterpret_cast<const uint64_t *>(m + s);
        if (((uint32_t)(p[2] >> 16) & 0xFFu) != o) continue;
        r.f.to = p[0];
        r.f.commit = p[1] < g.committed ? p[1] : g.committed;   // sendHeartbeatMessage's min
    }
    r.dest = k.keys[j];                               // (< n_dest: checked before it was a key)
    const uint32_t d0 = k.dstart[r.dest];
    r.dest_end = k.dstart[r.dest + 1];
    r.rank = j - d0;
    r.ends_batch = j + 1 == r.dest_end || r.rank % k.bm == k.bm - 1;
    return r;
}

__global__ void __launch_bounds__(kBlock) k_hbw_sizes(HbwK k) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= k.m) return;
    const HbwMsg r = message_of(k, (uint32_t)j);
    k.sizes[j] = hb_msg_size(r.f) + (r.ends_batch ? k.trailer_len : 0u);
}

__global__ void __launch_bounds__(kBlock) k_hbw_encode(HbwK k) {
    __shared__ uint4 stage4[kStageBytes / 16 + 1];
    uint8_t *const stage = reinterpret_cast<uint8_t *>(stage4);
    const uint64_t n_bytes = k.offs[k.m], n_batches = k.bscan[k.n_dest];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        k.totals[4] = n_bytes;
        k.totals[5] = n_batches;
    }
    if (n_bytes > k.bytes_cap || n_batches > k.batch_cap) return;   // (the whole grid alike)
    const uint64_t j0 = (uint64_t)blockIdx.x * kBlock, j1 = min(j0 + (uint64_t)kBlock, k.m);
    const uint64_t base = k.offs[j0], len = k.offs[j1] - base;
    const bool staged = len <= kStageBytes;           // (the whole workgroup alike)
    // the staged bytes keep their place within a 16-byte word of the output
    const uint32_t shift = (uint32_t)base & 15u;
    const uint64_t j = j0 + threadIdx.x;
    if (j < j1) {
        const HbwMsg r = message_of(k, (uint32_t)j);
        const uint64_t at = k.offs[j];
        uint8_t *p = staged ? stage + shift + (at - base) : k.bytes + at;
        p = hb_msg_put(p, r.f);
        if (r.ends_batch) hb_trailer_put(p, k.deployment_id, k.source, k.source_len);
        if (r.rank % k.bm == 0) {                     // the batch's first message: its table entry
            const uint64_t b = k.bscan[r.dest] + r.rank / k.bm;
            const uint64_t jend = min(j + (uint64_t)k.bm, (uint64_t)r.dest_end);
            if (b < k.batch_cap)
                k.batches[b] = hq_heartbeat_batch{at, k.offs[jend] - at, r.dest, (uint32_t)(jend - j)};
        }
    }
    if (!staged) return;
    __syncthreads();
    // stage[x] is output byte base - shift + x, for x in [lo, hi); the 16-byte words wholly inside
    // go out as such, the ragged head and tail byte by byte
    const uint32_t lo = shift, hi = shift + (uint32_t)len;
    const uint32_t w0 = (lo + 15u) / 16u, w1 = hi / 16u;
    uint8_t *const out = k.bytes + (base - shift);    // 16-byte aligned (pinned allocations are)
    for (uint32_t w = w0 + threadIdx.x; w < w1; w += kBlock)
        reinterpret_cast<uint4 *>(out)[w] = stage4[w];
    if (threadIdx.x < 16) {
        const uint32_t x = lo + threadIdx.x;          // the head: [lo, min(hi, 16 w0))
        if (x < hi && x < w0 * 16u) out[x] = stage[x];
    } else if (threadIdx.x < 32 && w1 >= w0) {
        const uint32_t x = w1 * 16u + (threadIdx.x - 16);   // the tail: [16 w1, hi)
        if (x < hi) out[x] = stage[x];
    }
}

}  // namespace

struct hq_hbw_dev : hq::Sidecar {
    hq::DevBuf<RouteRow> routes;       // the route column, a row per group
    hq::DevBuf<uint32_t> list, meta;
    hq::DevBuf<uint64_t> scan;
    hq::DevBuf<uint8_t> source;        // kHbSourceMax bytes
    hq::DevBuf<uint16_t> keys;         // 2 m: as written, sorted
    hq::DevBuf<uint32_t> vals, dstart, sizes;
    hq::DevBuf<uint64_t> bscan, offs;
    hq::DevBuf<uint8_t> tmp;           // hipcub's temporary
    hq::PinBuf<uint8_t> bytes;         // pinned host
    hq::PinBuf<hq_heartbeat_batch> batches;
};
static_assert(sizeof(RouteRow) == kDMembers * sizeof(uint16_t), "a row is a group's routes");

int hq_hbw_dev_open(hq_ctx *ctx, hq_hbw_dev **out) {
    int rc = hq::sidecar_open(ctx, out, "hq_heartbeat_wire");
    if (!rc && (rc = (*out)->source.reserve(ctx, kHbSourceMax, "hq_heartbeat_wire source"))) {
        hq_hbw_dev_close(*out);
        *out = nullptr;
    }
    return rc;
}

void hq_hbw_dev_close(hq_hbw_dev *h) { hq::sidecar_close(h); }

int hq_hbw_dev_put_routes(hq_hbw_dev *h, const uint16_t *routes, uint64_t n_groups, uint64_t g0,
                          uint64_t g1) {
    hq_ctx *ctx = h->ctx;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc) return rc;
    if (n_groups > h->routes.cap()) {                 // a new column: every row again
        // (no kernel of an earlier call reads the old one: every return has waited for the stream)
        rc = h->routes.grow(ctx, n_groups, "hq_heartbeat_wire routes");
        if (rc) return rc;
        g0 = 0;
        g1 = n_groups;
    }
    if (g1 > n_groups) g1 = n_groups;
    if (g0 >= g1) return HQ_OK;
    rc = hq::check_hip(ctx, hipMemcpyAsync(h->routes + g0, routes + g0 * kDMembers, (g1 - g0) * sizeof(RouteRow),
                                           hipMemcpyHostToDevice, ctx->stream), "hq_heartbeat_wire routes");
    // (the rows are pageable host memory the caller may change after this returns)
    return hq::finish(ctx, rc, "hq_heartbeat_wire routes");
}

int hq_hbw_dev_run(hq_hbw_dev *h, const hq_dstate_view *st, uint64_t n_member_records, uint64_t n,
                   const uint32_t *groups, const hq_heartbeat_wire_config *cfg,
                   hq_heartbeat_batches *out, uint32_t *error) {
    hq_ctx *ctx = h->ctx;
    hipStream_t s = ctx->stream;
    const char *const what = "hq_worker_heartbeat_batches";
    *error = 0;
    if (st->n_groups > h->routes.cap())
        return hq::fail(ctx, HQ_E_STATE, "hq_worker_heartbeat_batches: the route column is short");
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc) rc = h->meta.grow(ctx, n, "hq_heartbeat_wire words");
    if (!rc) rc = h->scan.grow(ctx, n + 1, "hq_heartbeat_wire scan");
    if (!rc && groups) rc = h->list.grow(ctx, n, "hq_heartbeat_wire list");
    if (!rc) rc = h->dstart.grow(ctx, (size_t)cfg->n_dest + 1, "hq_heartbeat_wire destinations");
    if (!rc) rc = h->bscan.grow(ctx, (size_t)cfg->n_dest + 1, "hq_heartbeat_wire destinations");
    if (rc) return rc;

    HbwK k{};
    k.groups = st->groups;
    k.reads = st->reads;
    k.members = st->members;
    k.n_state_groups = st->n_groups;
    k.n_state_members = n_member_records;
    k.list = groups ? h->list.get() : nullptr;
    k.n = n;
    k.routes = reinterpret_cast<const uint16_t *>(h->routes.get());
    k.n_dest = cfg->n_dest;
    k.bm = cfg->batch_messages ? cfg->batch_messages : UINT32_MAX;
    k.deployment_id = cfg->deployment_id;
    k.source = h->source;
    k.source_len = cfg->source_len;
    k.trailer_len = hb_trailer_size(cfg->deployment_id, cfg->source_len);
    k.meta = h->meta;
    k.scan = h->scan;
    k.error = h->error();
    k.dstart = h->dstart;
    k.bscan = h->bscan;
    k.totals = h->totals;

    using Counting = hipcub::CountingInputIterator<uint64_t>;
    const hipcub::TransformInputIterator<uint64_t, HbwCount, Counting> counts(Counting(0),
                                                                             HbwCount{h->meta, n});
    const int items = (int)n;     // (n < 2^28)
    const int dests = (int)cfg->n_dest + 1;
    size_t tmp = 0;
    rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, counts, k.scan, items + 1, s),
                       "hipcub scan size");
    if (!rc) rc = h->tmp.grow(ctx, tmp, "hq_heartbeat_wire scan");
    if (rc) return rc;            // (nothing is queued yet; from here on every return is finish's)

    if (groups)
        rc = hq::check_hip(ctx, hipMemcpyAsync(h->list, groups, n * 4, hipMemcpyHostToDevice, s),
                           "hq_heartbeat_wire list");
    if (!rc && cfg->source_len)
        rc = hq::check_hip(ctx, hipMemcpyAsync(h->source, cfg->source, cfg->source_len,
                                               hipMemcpyHostToDevice, s), "hq_heartbeat_wire source");
    if (!rc) rc = hq::check_hip(ctx, hipMemsetAsync(h->error(), 0, 16, s), "memset");
    if (!rc) rc = hq::check_hip(ctx, hipEventRecord(h->ev0, s), "event");
    const uint32_t g1 = (uint32_t)((n + kBlock - 1) / kBlock);
    if (!rc) {
        hipLaunchKernelGGL(k_hbw_words, dim3(g1), dim3(kBlock), 0, s, k);
        rc = hq::check_hip(ctx, hipGetLastError(), "k_hbw_words");
    }
    if (!rc) {
        size_t t = h->tmp.cap();
        rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(h->tmp.get(), t, counts, k.scan, items + 1, s),
                           "hipcub scan");
    }
    if (!rc) rc = hq::check_hip(ctx, hipMemcpyAsync(h->totals, k.scan + n, 8, hipMemcpyDeviceToHost, s),
                                "hq_heartbeat_wire totals");
    if (!rc) rc = hq::check_hip(ctx, hipMemcpyAsync(h->totals + 1, h->error(), 4, hipMemcpyDeviceToHost, s),
                                "hq_heartbeat_wire totals");
    // (the list and the source are the caller's memory: they are on the device after this)
    rc = hq::finish(ctx, rc, what);
    if (rc) return rc;
    if ((uint32_t)h->totals[1]) {
        *error = (uint32_t)h->totals[1];
        return HQ_E_INVAL;
    }
    const uint64_t m = h->totals[0] & kRoutedMask, unrouted = h->totals[0] >> kUnroutedShift;
    std::memset(out, 0, sizeof *out);
    out->n_unrouted = unrouted;
    if (m == 0) return HQ_OK;     // nothing to send: no batch
    if (m >= (uint64_t(1) << 31))
        return hq::fail(ctx, HQ_E_INVAL, "hq_worker_heartbeat_batches: 2^31 or more messages in one call");

    // the batches at most: one more per destination than the full ones
    const uint64_t batches_max = std::min<uint64_t>(m, (uint64_t)cfg->n_dest + m / k.bm);
    // (the sort's two halves each 16-byte aligned for any m: they start at multiples of 8 items)
    const uint64_t half = (m + 7) & ~uint64_t(7);
    rc = h->keys.grow(ctx, 2 * half, "hq_heartbeat_wire keys");
    if (!rc) rc = h->vals.grow(ctx, 2 * half, "hq_heartbeat_wire values");
    if (!rc) rc = h->sizes.grow(ctx, m, "hq_heartbeat_wire sizes");
    if (!rc) rc = h->offs.grow(ctx, m + 1, "hq_heartbeat_wire offsets");
    if (!rc) rc = h->batches.grow(ctx, batches_max, "hq_heartbeat_wire batches");
    // (a first call's bytes: 58 per message and a trailer per destination, grown to what a call needs)
    if (!rc) rc = h->bytes.grow(ctx, m * 58 + (uint64_t)std::min<uint64_t>(m, cfg->n_dest) * k.trailer_len,
                                "hq_heartbeat_wire bytes");
    if (rc) return hq::finish(ctx, rc, what);
    k.m = m;
    k.keys_in = h->keys;
    k.keys = h->keys + half;
    k.vals_in = h->vals;
    k.vals = h->vals + half;
    k.sizes = h->sizes;
    k.offs = h->offs;

    int end_bit = 1;
    while (end_bit < 16 && ((cfg->n_dest - 1) >> end_bit)) ++end_bit;
    const hipcub::TransformInputIterator<uint64_t, HbwBatches, Counting> nbatches(
        Counting(0), HbwBatches{h->dstart, cfg->n_dest, k.bm});
    const hipcub::TransformInputIterator<uint64_t, HbwSize, Counting> sizes(Counting(0),
                                                                           HbwSize{h->sizes, m});
    size_t t1 = 0, t2 = 0, t3 = 0;
    rc = hq::check_hip(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, t1, k.keys_in, k.keys, k.vals_in,
                                                               k.vals, (int)m, 0, end_bit, s),
                       "hipcub sort size");
    if (!rc) rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, t2, nbatches, k.bscan,
                                                                      dests, s), "hipcub scan size");
    if (!rc) rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, t3, sizes, k.offs,
                                                                      (int)m + 1, s), "hipcub scan size");
    if (!rc) rc = h->tmp.grow(ctx, std::max(t1, std::max(t2, t3)), "hq_heartbeat_wire scan");
    if (rc) return hq::finish(ctx, rc, what);

    const uint32_t gm = (uint32_t)((m + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_hbw_desc, dim3(g1), dim3(kBlock), 0, s, k);
    rc = hq::check_hip(ctx, hipGetLastError(), "k_hbw_desc");
    if (!rc) {
        size_t t = h->tmp.cap();  // (the same temporary: the sort and the scans run one after another)
        rc = hq::check_hip(ctx, hipcub::DeviceRadixSort::SortPairs(h->tmp.get(), t, k.keys_in, k.keys, k.vals_in,
                                                                   k.vals, (int)m, 0, end_bit, s),
                           "hipcub sort");
    }
    if (!rc) {
        hipLaunchKernelGGL(k_hbw_dests, dim3((uint32_t)((dests + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                           s, k);
        rc = hq::check_hip(ctx, hipGetLastError(), "k_hbw_dests");
    }
    if (!rc) {
        size_t t = h->tmp.cap();
        rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(h->tmp.get(), t, nbatches, k.bscan, dests, s),
                           "hipcub scan");
    }
    if (!rc) {
        hipLaunchKernelGGL(k_hbw_sizes, dim3(gm), dim3(kBlock), 0, s, k);
        rc = hq::check_hip(ctx, hipGetLastError(), "k_hbw_sizes");
    }
    if (!rc) {
        size_t t = h->tmp.cap();
        rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(h->tmp.get(), t, sizes, k.offs, (int)m + 1, s),
                           "hipcub scan");
    }
    // the bytes and the table; again with larger buffers when a total passed a capacity (nothing
    // was written then; the sorted messages, the sizes and the scans stand)
    for (int pass = 0; !rc; ++pass) {
        k.bytes = h->bytes;
        k.batches = h->batches;
        k.bytes_cap = h->bytes.cap();
        k.batch_cap = h->batches.cap();
        hipLaunchKernelGGL(k_hbw_encode, dim3(gm), dim3(kBlock), 0, s, k);
        rc = hq::check_hip(ctx, hipGetLastError(), "k_hbw_encode");
        if (!rc) rc = hq::check_hip(ctx, hipEventRecord(h->ev1, s), "event");
        rc = hq::finish(ctx, rc, what);
        if (rc) return rc;
        if (h->totals[4] <= h->bytes.cap() && h->totals[5] <= h->batches.cap()) break;
        if (pass) return hq::fail(ctx, HQ_E_STATE, "hq_worker_heartbeat_batches: totals changed");
        rc = h->bytes.grow(ctx, h->totals[4], "hq_heartbeat_wire bytes");
        if (!rc) rc = h->batches.grow(ctx, h->totals[5], "hq_heartbeat_wire batches");
    }
    if (rc) return hq::finish(ctx, rc, what);

    out->bytes = h->bytes;
    out->n_bytes = h->totals[4];
    out->batches = h->batches;
    out->n_batches = h->totals[5];
    out->n_messages = m;
    out->gpu_ns = hq::elapsed_ns(h->ev0, h->ev1);
    return HQ_OK;
}
