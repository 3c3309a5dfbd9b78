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
#include <new>

#include "hq_heartbeat.h"
#include "hq_heartbeat_wire.h"
#include "hq_internal.h"

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

template <class T>
int grow_dev(hq_ctx *ctx, T **p, size_t *cap, size_t need, const char *what) {
    if (need <= *cap) return HQ_OK;
    const size_t want = need + need / 2;
    T *n = nullptr;
    int rc = hq::check_hip(ctx, hipMalloc(reinterpret_cast<void **>(&n), want * sizeof(T)), what);
    if (rc) return rc;
    if (*p) (void)hipFree(*p);
    *p = n;
    *cap = want;
    return HQ_OK;
}

template <class T>
int grow_pinned(hq_ctx *ctx, T **p, size_t *cap, size_t need, const char *what) {
    if (need <= *cap) return HQ_OK;
    const size_t want = need + need / 2;
    T *n = nullptr;
    int rc = hq::check_hip(ctx, hipHostMalloc(reinterpret_cast<void **>(&n), want * sizeof(T),
                                              hipHostMallocDefault), what);
    if (rc) return rc;
    if (*p) (void)hipHostFree(*p);
    *p = n;
    *cap = want;
    return HQ_OK;
}

}  // namespace

struct hq_hbw_dev {
    hq_ctx *ctx = nullptr;
    uint16_t *routes = nullptr;    // the route column, 16 per group
    size_t routes_cap = 0;         // (groups)
    uint32_t *list = nullptr, *meta = nullptr;
    uint64_t *scan = nullptr;
    uint32_t *error = nullptr;
    uint8_t *source = nullptr;     // kHbSourceMax bytes
    uint16_t *keys = nullptr;      // 2 m: as written, sorted
    uint32_t *vals = nullptr, *dstart = nullptr, *sizes = nullptr;
    uint64_t *bscan = nullptr, *offs = nullptr;
    void *tmp = nullptr;
    size_t list_cap = 0, meta_cap = 0, scan_cap = 0, keys_cap = 0, vals_cap = 0, dstart_cap = 0,
           sizes_cap = 0, bscan_cap = 0, offs_cap = 0, tmp_cap = 0;
    uint8_t *bytes = nullptr;      // pinned host
    hq_heartbeat_batch *batches = nullptr;
    uint64_t *totals = nullptr;
    size_t bytes_cap = 0, batch_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

int hq_hbw_dev_open(hq_ctx *ctx, hq_hbw_dev **out) {
    *out = new (std::nothrow) hq_hbw_dev();
    if (!*out) return HQ_E_NOMEM;
    hq_hbw_dev *h = *out;
    h->ctx = ctx;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    for (hipEvent_t *e : {&h->ev0, &h->ev1})
        if (!rc) rc = hq::check_hip(ctx, hipEventCreate(e), "event");
    if (!rc) rc = hq::check_hip(ctx, hipMalloc(reinterpret_cast<void **>(&h->error), 16),
                                "hq_heartbeat_wire error word");
    if (!rc) rc = hq::check_hip(ctx, hipMalloc(reinterpret_cast<void **>(&h->source), kHbSourceMax),
                                "hq_heartbeat_wire source");
    if (!rc)
        rc = hq::check_hip(ctx, hipHostMalloc(reinterpret_cast<void **>(&h->totals), 64,
                                              hipHostMallocDefault), "hq_heartbeat_wire totals");
    if (!rc) std::memset(h->totals, 0, 64);
    if (rc) {
        hq_hbw_dev_close(h);
        *out = nullptr;
    }
    return rc;
}

void hq_hbw_dev_close(hq_hbw_dev *h) {
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    for (void *p : {(void *)h->routes, (void *)h->list, (void *)h->meta, (void *)h->scan,
                    (void *)h->error, (void *)h->source, (void *)h->keys, (void *)h->vals,
                    (void *)h->dstart, (void *)h->sizes, (void *)h->bscan, (void *)h->offs, h->tmp})
        if (p) (void)hipFree(p);
    for (void *p : {(void *)h->bytes, (void *)h->batches, (void *)h->totals})
        if (p) (void)hipHostFree(p);
    for (hipEvent_t e : {h->ev0, h->ev1})
        if (e) (void)hipEventDestroy(e);
    delete h;
}

int hq_hbw_dev_put_routes(hq_hbw_dev *h, const uint16_t *routes, uint64_t n_groups, uint64_t g0,
                          uint64_t g1) {
    hq_ctx *ctx = h->ctx;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc) return rc;
    if (n_groups > h->routes_cap) {                   // a new column: every row again
        const size_t want = n_groups + n_groups / 2;
        uint16_t *n = nullptr;
        rc = hq::check_hip(ctx, hipMalloc(reinterpret_cast<void **>(&n), want * kDMembers * 2),
                           "hq_heartbeat_wire routes");
        if (rc) return rc;
        // (kernels of an earlier call have finished: every call ends with a synchronize)
        if (h->routes) (void)hipFree(h->routes);
        h->routes = n;
        h->routes_cap = want;
        g0 = 0;
        g1 = n_groups;
    }
    if (g1 > n_groups) g1 = n_groups;
    if (g0 >= g1) return HQ_OK;
    rc = hq::check_hip(ctx, hipMemcpyAsync(h->routes + g0 * kDMembers, routes + g0 * kDMembers,
                                           (g1 - g0) * kDMembers * 2, hipMemcpyHostToDevice,
                                           ctx->stream), "hq_heartbeat_wire routes");
    // (the rows are pageable host memory the caller may change after this returns)
    if (!rc) rc = hq::check_hip(ctx, hipStreamSynchronize(ctx->stream), "hq_heartbeat_wire routes");
    return rc;
}

int hq_hbw_dev_run(hq_hbw_dev *h, const hq_dstate_view *st, uint64_t n_member_records, uint64_t n,
                   const uint32_t *groups, const hq_heartbeat_wire_config *cfg,
                   hq_heartbeat_batches *out, uint32_t *error) {
    hq_ctx *ctx = h->ctx;
    hipStream_t s = ctx->stream;
    *error = 0;
    if (st->n_groups > h->routes_cap)
        return hq::fail(ctx, HQ_E_STATE, "hq_worker_heartbeat_batches: the route column is short");
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc) rc = grow_dev(ctx, &h->meta, &h->meta_cap, n, "hq_heartbeat_wire words");
    if (!rc) rc = grow_dev(ctx, &h->scan, &h->scan_cap, n + 1, "hq_heartbeat_wire scan");
    if (!rc && groups) rc = grow_dev(ctx, &h->list, &h->list_cap, n, "hq_heartbeat_wire list");
    if (!rc) rc = grow_dev(ctx, &h->dstart, &h->dstart_cap, (size_t)cfg->n_dest + 1,
                           "hq_heartbeat_wire destinations");
    if (!rc) rc = grow_dev(ctx, &h->bscan, &h->bscan_cap, (size_t)cfg->n_dest + 1,
                           "hq_heartbeat_wire destinations");
    if (rc) return rc;

    HbwK k{};
    k.groups = st->groups;
    k.reads = st->reads;
    k.members = st->members;
    k.n_state_groups = st->n_groups;
    k.n_state_members = n_member_records;
    k.list = groups ? h->list : nullptr;
    k.n = n;
    k.routes = h->routes;
    k.n_dest = cfg->n_dest;
    k.bm = cfg->batch_messages ? cfg->batch_messages : UINT32_MAX;
    k.deployment_id = cfg->deployment_id;
    k.source = h->source;
    k.source_len = cfg->source_len;
    k.trailer_len = hb_trailer_size(cfg->deployment_id, cfg->source_len);
    k.meta = h->meta;
    k.scan = h->scan;
    k.error = h->error;
    k.dstart = h->dstart;
    k.bscan = h->bscan;
    k.totals = h->totals;

    using Counting = hipcub::CountingInputIterator<uint64_t>;
    const hipcub::TransformInputIterator<uint64_t, HbwCount, Counting> counts(Counting(0),
                                                                             HbwCount{h->meta, n});
    const int items = (int)n;     // (n < 2^28)
    const int dests = (int)cfg->n_dest + 1;
    auto ensure_tmp = [&](size_t need) {
        if (need <= h->tmp_cap) return (int)HQ_OK;
        if (h->tmp) (void)hipFree(h->tmp);
        h->tmp = nullptr;
        h->tmp_cap = 0;
        int r = hq::check_hip(ctx, hipMalloc(&h->tmp, need + need / 2), "hq_heartbeat_wire scan");
        if (!r) h->tmp_cap = need + need / 2;
        return r;
    };
    size_t tmp = 0;
    rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, counts, h->scan, items + 1, s),
                       "hipcub scan size");
    if (!rc) rc = ensure_tmp(tmp);
    if (!rc && groups)
        rc = hq::check_hip(ctx, hipMemcpyAsync(h->list, groups, n * 4, hipMemcpyHostToDevice, s),
                           "hq_heartbeat_wire list");
    if (!rc && cfg->source_len)
        rc = hq::check_hip(ctx, hipMemcpyAsync(h->source, cfg->source, cfg->source_len,
                                               hipMemcpyHostToDevice, s), "hq_heartbeat_wire source");
    if (!rc) rc = hq::check_hip(ctx, hipMemsetAsync(h->error, 0, 16, s), "memset");
    if (!rc) rc = hq::check_hip(ctx, hipEventRecord(h->ev0, s), "event");
    if (rc) return rc;
    const uint32_t g1 = (uint32_t)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_hbw_words, dim3(g1), dim3(kBlock), 0, s, k);
    rc = hq::check_hip(ctx, hipGetLastError(), "k_hbw_words");
    if (!rc) {
        size_t t = h->tmp_cap;
        rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(h->tmp, t, counts, h->scan, items + 1, s),
                           "hipcub scan");
    }
    if (!rc) rc = hq::check_hip(ctx, hipMemcpyAsync(h->totals, h->scan + n, 8, hipMemcpyDeviceToHost, s),
                                "hq_heartbeat_wire totals");
    if (!rc) rc = hq::check_hip(ctx, hipMemcpyAsync(h->totals + 1, h->error, 4, hipMemcpyDeviceToHost, s),
                                "hq_heartbeat_wire totals");
    // (the list and the source are the caller's memory: they are on the device after this)
    if (!rc) rc = hq::check_hip(ctx, hipStreamSynchronize(s), "hq_worker_heartbeat_batches");
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
    rc = grow_dev(ctx, &h->keys, &h->keys_cap, 2 * half, "hq_heartbeat_wire keys");
    if (!rc) rc = grow_dev(ctx, &h->vals, &h->vals_cap, 2 * half, "hq_heartbeat_wire values");
    if (!rc) rc = grow_dev(ctx, &h->sizes, &h->sizes_cap, m, "hq_heartbeat_wire sizes");
    if (!rc) rc = grow_dev(ctx, &h->offs, &h->offs_cap, m + 1, "hq_heartbeat_wire offsets");
    if (!rc) rc = grow_pinned(ctx, &h->batches, &h->batch_cap, batches_max, "hq_heartbeat_wire batches");
    // (a first call's bytes: 58 per message and a trailer per destination, grown to what a call needs)
    if (!rc) rc = grow_pinned(ctx, &h->bytes, &h->bytes_cap,
                              m * 58 + (uint64_t)std::min<uint64_t>(m, cfg->n_dest) * k.trailer_len,
                              "hq_heartbeat_wire bytes");
    if (rc) return rc;
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
    if (!rc) rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, t2, nbatches, h->bscan,
                                                                      dests, s), "hipcub scan size");
    if (!rc) rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, t3, sizes, h->offs,
                                                                      (int)m + 1, s), "hipcub scan size");
    if (!rc) rc = ensure_tmp(std::max(t1, std::max(t2, t3)));
    if (rc) return rc;

    const uint32_t gm = (uint32_t)((m + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_hbw_desc, dim3(g1), dim3(kBlock), 0, s, k);
    rc = hq::check_hip(ctx, hipGetLastError(), "k_hbw_desc");
    if (!rc) {
        size_t t = h->tmp_cap;    // (the same temporary: the sort and the scans run one after another)
        rc = hq::check_hip(ctx, hipcub::DeviceRadixSort::SortPairs(h->tmp, t, k.keys_in, k.keys, k.vals_in,
                                                                   k.vals, (int)m, 0, end_bit, s),
                           "hipcub sort");
    }
    if (!rc) {
        hipLaunchKernelGGL(k_hbw_dests, dim3((uint32_t)((dests + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                           s, k);
        rc = hq::check_hip(ctx, hipGetLastError(), "k_hbw_dests");
    }
    if (!rc) {
        size_t t = h->tmp_cap;
        rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(h->tmp, t, nbatches, h->bscan, dests, s),
                           "hipcub scan");
    }
    if (!rc) {
        hipLaunchKernelGGL(k_hbw_sizes, dim3(gm), dim3(kBlock), 0, s, k);
        rc = hq::check_hip(ctx, hipGetLastError(), "k_hbw_sizes");
    }
    if (!rc) {
        size_t t = h->tmp_cap;
        rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(h->tmp, t, sizes, h->offs, (int)m + 1, s),
                           "hipcub scan");
    }
    // the bytes and the table; again with larger buffers when a total passed a capacity (nothing
    // was written then; the sorted messages, the sizes and the scans stand)
    for (int pass = 0; !rc; ++pass) {
        k.bytes = h->bytes;
        k.batches = h->batches;
        k.bytes_cap = h->bytes_cap;
        k.batch_cap = h->batch_cap;
        hipLaunchKernelGGL(k_hbw_encode, dim3(gm), dim3(kBlock), 0, s, k);
        rc = hq::check_hip(ctx, hipGetLastError(), "k_hbw_encode");
        if (!rc) rc = hq::check_hip(ctx, hipEventRecord(h->ev1, s), "event");
        if (!rc) rc = hq::check_hip(ctx, hipStreamSynchronize(s), "hq_worker_heartbeat_batches");
        if (rc) break;
        if (h->totals[4] <= h->bytes_cap && h->totals[5] <= h->batch_cap) break;
        if (pass) return hq::fail(ctx, HQ_E_STATE, "hq_worker_heartbeat_batches: totals changed");
        rc = grow_pinned(ctx, &h->bytes, &h->bytes_cap, h->totals[4], "hq_heartbeat_wire bytes");
        if (!rc) rc = grow_pinned(ctx, &h->batches, &h->batch_cap, h->totals[5], "hq_heartbeat_wire batches");
    }
    if (rc) return rc;

    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) != hipSuccess) {
        (void)hipGetLastError();
        ms = 0.f;
    }
    out->bytes = h->bytes;
    out->n_bytes = h->totals[4];
    out->batches = h->batches;
    out->n_batches = h->totals[5];
    out->n_messages = m;
    out->gpu_ns = (uint64_t)((double)ms * 1e6);
    return HQ_OK;
}
