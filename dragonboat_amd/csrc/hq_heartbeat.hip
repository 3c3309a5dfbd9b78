// hq_heartbeat.hip — the leader heartbeat broadcast over a device worker's resident state
// (hq_worker_heartbeats, include/hipquorum.h "leader heartbeat broadcast"): what
// broadcastHeartbeatMessage (raft.go:826-848) sends for each listed group, read where the step
// keeps remote.match, the committed index and the pending reads, and returned compact.
//
// Read-only, two kernels and a scan between them, all on the context's stream behind the last
// step:
//   k_hb_words   one lane per listed group: the group record (16-byte loads; with the implicit
//                list a wave's 64 records are 4 KB contiguous), its members' match and list
//                position, and the tail of its read queue when one is pending. The word goes to
//                the pinned host column (256 contiguous bytes per wave) and, with the "has a ctx"
//                bit, to a device column for the second kernel
//   scan         hipcub ExclusiveSum over (lags | ctxs << 36) per group, n + 1 items: the last
//                holds the totals; and a hipcub Sum of the groups' messages
//   k_hb_records the groups with a record write theirs at the scanned places, straight into
//                pinned host memory; a place at or past a buffer's capacity is not written (the
//                host sees the totals, grows the buffer and runs this kernel again)
// No spinning and no atomics but the one error-word atomicOr of a refused input.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <new>

#include "hq_heartbeat.h"
#include "hq_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kCtxShift = 36;                    // scan item: lags | ctxs << 36
constexpr uint64_t kLagMask = (uint64_t(1) << kCtxShift) - 1;
constexpr uint64_t kHasCtx = uint64_t(1) << 32;       // device column: word | has-ctx << 32

struct HbK {
    const hq_dgroup *groups;
    const hq_dread *reads;
    const hq_dmember *members;
    uint64_t n_state_groups, n_state_members;
    const uint32_t *list;          // device; NULL: handle i
    uint64_t n;
    uint32_t *words;               // pinned host [n]
    uint64_t *meta;                // device [n]: word | has-ctx << 32
    const uint64_t *scan;          // device [n + 1]
    hq_heartbeat_lag *lags;        // pinned host [lag_cap]
    hq_heartbeat_ctx *ctxs;        // pinned host [ctx_cap]
    uint64_t lag_cap, ctx_cap;
    uint64_t *totals;              // pinned host: lags, ctxs, the error word, messages
    uint32_t *error;               // device
    const uint64_t *n_messages;    // device: the Sum's result
};

using hqhb::GroupRef;
using hqhb::MemberRef;
using hqhb::load_group;
using hqhb::load_member;

struct HbMessages {               // group i's messages
    const uint64_t *meta;
    __host__ __device__ uint64_t operator()(uint64_t i) const {
#if defined(__HIP_DEVICE_COMPILE__)
        return (uint64_t)__popc((uint32_t)meta[i] & 0xFFFFu);
#else
        return (uint64_t)__builtin_popcount((uint32_t)meta[i] & 0xFFFFu);
#endif
    }
};

struct HbCount {                  // item i of the scan: group i's records; item n: 0
    const uint64_t *meta;
    uint64_t n;
    __host__ __device__ uint64_t operator()(uint64_t i) const {
        if (i >= n) return 0;
        const uint64_t m = meta[i];
#if defined(__HIP_DEVICE_COMPILE__)
        const uint64_t lags = (uint64_t)__popc((uint32_t)(m >> 16) & 0xFFFFu);
#else
        const uint64_t lags = (uint64_t)__builtin_popcount((uint32_t)(m >> 16) & 0xFFFFu);
#endif
        return lags | ((m >> 32) & 1) << kCtxShift;
    }
};

__global__ void __launch_bounds__(kBlock) k_hb_words(HbK k) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= k.n) return;
    const uint64_t h = k.list ? k.list[i] : i;
    uint32_t word = 0;
    uint64_t has_ctx = 0;
    if (h >= k.n_state_groups) {
        atomicOr(k.error, kHbErrHandle);
    } else {
        uint32_t err = 0;
        uint64_t lo = 0, hi = 0;
        word = hqhb::word_of(k.groups, k.reads, k.members, k.n_state_members, h, &lo, &hi, &err);
        if (err) atomicOr(k.error, err);
        has_ctx = word && (lo | hi) ? kHasCtx : 0;
    }
    k.words[i] = word;
    k.meta[i] = word | has_ctx;
}

__global__ void __launch_bounds__(kBlock) k_hb_records(HbK k) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i > k.n) return;
    if (i == k.n) {                                   // the totals, and what k_hb_words refused
        const uint64_t t = k.scan[k.n];
        k.totals[0] = t & kLagMask;
        k.totals[1] = t >> kCtxShift;
        k.totals[2] = *k.error;
        k.totals[3] = *k.n_messages;
        return;
    }
    const uint64_t meta = k.meta[i];
    const uint32_t behind = (uint32_t)(meta >> 16) & 0xFFFFu;
    if (!behind && !(meta & kHasCtx)) return;
    const uint64_t at = k.scan[i], h = k.list ? k.list[i] : i;
    const GroupRef g = load_group(k.groups + h);      // (checked by k_hb_words: meta != 0)
    if (meta & kHasCtx) {
        const uint64_t c = at >> kCtxShift;
        const hq_dread *r = k.reads + h * kDReads + (g.n_reads - 1);
        if (c < k.ctx_cap) k.ctxs[c] = hq_heartbeat_ctx{r->low, r->high, (uint32_t)i, 0};
    }
    if (!behind) return;
    const uint64_t l0 = at & kLagMask;
    const hq_dmember *m = k.members + g.mem;
    for (uint32_t s = 1; s < g.n_members; ++s) {
        const MemberRef r = load_member(m + s);
        const uint32_t o = r.order & 15u;
        if (!((behind >> o) & 1)) continue;
        // member order: as many records before it as behind bits below its own
        const uint64_t l = l0 + __popc(behind & ((1u << o) - 1));
        if (l < k.lag_cap) k.lags[l] = hq_heartbeat_lag{(uint32_t)i, o, r.match};
    }
}

}  // namespace

struct hq_hb_dev {
    hq_ctx *ctx = nullptr;
    uint32_t *list = nullptr;      // device copies / columns, grown on demand
    uint64_t *meta = nullptr, *scan = nullptr;
    uint64_t *misc = nullptr;      // the error word (its low half), the messages' sum
    void *scan_tmp = nullptr;
    size_t list_cap = 0, meta_cap = 0, scan_cap = 0, scan_tmp_cap = 0;   // (items; bytes)
    uint32_t *words = nullptr;     // pinned host
    hq_heartbeat_lag *lags = nullptr;
    hq_heartbeat_ctx *ctxs = nullptr;
    uint64_t *totals = nullptr;
    size_t words_cap = 0, lag_cap = 0, ctx_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

namespace {

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

int hq_hb_dev_open(hq_ctx *ctx, hq_hb_dev **out) {
    *out = new (std::nothrow) hq_hb_dev();
    if (!*out) return HQ_E_NOMEM;
    hq_hb_dev *h = *out;
    h->ctx = ctx;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    for (hipEvent_t *e : {&h->ev0, &h->ev1})
        if (!rc) rc = hq::check_hip(ctx, hipEventCreate(e), "event");
    if (!rc) rc = hq::check_hip(ctx, hipMalloc(reinterpret_cast<void **>(&h->misc), 16),
                                "hq_heartbeat error word");
    if (!rc)
        rc = hq::check_hip(ctx, hipHostMalloc(reinterpret_cast<void **>(&h->totals), 64,
                                              hipHostMallocDefault), "hq_heartbeat totals");
    if (rc) {
        hq_hb_dev_close(h);
        *out = nullptr;
    }
    return rc;
}

void hq_hb_dev_close(hq_hb_dev *h) {
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    for (void *p : {(void *)h->list, (void *)h->meta, (void *)h->scan, (void *)h->misc, h->scan_tmp})
        if (p) (void)hipFree(p);
    for (void *p : {(void *)h->words, (void *)h->lags, (void *)h->ctxs, (void *)h->totals})
        if (p) (void)hipHostFree(p);
    for (hipEvent_t e : {h->ev0, h->ev1})
        if (e) (void)hipEventDestroy(e);
    delete h;
}

int hq_hb_dev_run(hq_hb_dev *h, const hq_dstate_view *st, uint64_t n_member_records, uint64_t n,
                  const uint32_t *groups, hq_heartbeat_output *out, uint32_t *error) {
    hq_ctx *ctx = h->ctx;
    hipStream_t s = ctx->stream;
    *error = 0;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc) rc = grow_pinned(ctx, &h->words, &h->words_cap, n, "hq_heartbeat words");
    if (!rc) rc = grow_dev(ctx, &h->meta, &h->meta_cap, n, "hq_heartbeat words");
    if (!rc) rc = grow_dev(ctx, &h->scan, &h->scan_cap, n + 1, "hq_heartbeat scan");
    if (!rc && groups) rc = grow_dev(ctx, &h->list, &h->list_cap, n, "hq_heartbeat list");
    // (a first call's record buffers: a record for one group in four, grown to what a call needs)
    if (!rc) rc = grow_pinned(ctx, &h->lags, &h->lag_cap, std::max<uint64_t>(n / 4, 256),
                              "hq_heartbeat lags");
    if (!rc) rc = grow_pinned(ctx, &h->ctxs, &h->ctx_cap, std::max<uint64_t>(n / 4, 256),
                              "hq_heartbeat ctxs");
    if (rc) return rc;

    HbK k{};
    k.groups = st->groups;
    k.reads = st->reads;
    k.members = st->members;
    k.n_state_groups = st->n_groups;
    k.n_state_members = n_member_records;
    k.list = groups ? h->list : nullptr;
    k.n = n;
    k.words = h->words;
    k.meta = h->meta;
    k.scan = h->scan;
    k.totals = h->totals;
    k.error = reinterpret_cast<uint32_t *>(h->misc);
    k.n_messages = h->misc + 1;

    const hipcub::TransformInputIterator<uint64_t, HbCount, hipcub::CountingInputIterator<uint64_t>>
        counts(hipcub::CountingInputIterator<uint64_t>(0), HbCount{h->meta, n});
    const hipcub::TransformInputIterator<uint64_t, HbMessages, hipcub::CountingInputIterator<uint64_t>>
        messages(hipcub::CountingInputIterator<uint64_t>(0), HbMessages{h->meta});
    const int items = (int)n;     // (n < 2^28)
    size_t tmp = 0, tmp2 = 0;
    rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, counts, h->scan, items + 1, s),
                       "hipcub scan size");
    if (!rc)
        rc = hq::check_hip(ctx, hipcub::DeviceReduce::Sum(nullptr, tmp2, messages, h->misc + 1, items, s),
                           "hipcub sum size");
    tmp = std::max(tmp, tmp2);
    if (!rc && tmp > h->scan_tmp_cap) {
        if (h->scan_tmp) (void)hipFree(h->scan_tmp);
        h->scan_tmp = nullptr;
        h->scan_tmp_cap = 0;
        rc = hq::check_hip(ctx, hipMalloc(&h->scan_tmp, tmp + tmp / 2), "hq_heartbeat scan");
        if (!rc) h->scan_tmp_cap = tmp + tmp / 2;
    }
    if (!rc && groups)
        rc = hq::check_hip(ctx, hipMemcpyAsync(h->list, groups, n * 4, hipMemcpyHostToDevice, s),
                           "hq_heartbeat list");
    if (!rc) rc = hq::check_hip(ctx, hipMemsetAsync(h->misc, 0, 16, s), "memset");
    if (!rc) rc = hq::check_hip(ctx, hipEventRecord(h->ev0, s), "event");
    if (rc) return rc;
    const uint32_t g1 = (uint32_t)((n + kBlock - 1) / kBlock), g2 = (uint32_t)(n / kBlock + 1);
    hipLaunchKernelGGL(k_hb_words, dim3(g1), dim3(kBlock), 0, s, k);
    rc = hq::check_hip(ctx, hipGetLastError(), "k_hb_words");
    if (!rc) {
        size_t t = h->scan_tmp_cap;
        rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(h->scan_tmp, t, counts, h->scan,
                                                                  items + 1, s), "hipcub scan");
        t = h->scan_tmp_cap;      // (the same temporary: the two run one after the other)
        if (!rc)
            rc = hq::check_hip(ctx, hipcub::DeviceReduce::Sum(h->scan_tmp, t, messages, h->misc + 1,
                                                              items, s), "hipcub sum");
    }
    // the records; again with larger buffers when a total passed a capacity (nothing was written
    // out of bounds; the words, the column and the scan stand)
    for (int pass = 0; !rc; ++pass) {
        k.lags = h->lags;
        k.ctxs = h->ctxs;
        k.lag_cap = h->lag_cap;
        k.ctx_cap = h->ctx_cap;
        hipLaunchKernelGGL(k_hb_records, dim3(g2), dim3(kBlock), 0, s, k);
        rc = hq::check_hip(ctx, hipGetLastError(), "k_hb_records");
        if (!rc) rc = hq::check_hip(ctx, hipEventRecord(h->ev1, s), "event");
        if (!rc) rc = hq::check_hip(ctx, hipStreamSynchronize(s), "hq_worker_heartbeats");
        if (rc) break;
        if (h->totals[2]) {
            *error = (uint32_t)h->totals[2];
            return HQ_E_INVAL;
        }
        if (h->totals[0] <= h->lag_cap && h->totals[1] <= h->ctx_cap) break;
        if (pass) return hq::fail(ctx, HQ_E_STATE, "hq_worker_heartbeats: record totals changed");
        rc = grow_pinned(ctx, &h->lags, &h->lag_cap, h->totals[0], "hq_heartbeat lags");
        if (!rc) rc = grow_pinned(ctx, &h->ctxs, &h->ctx_cap, h->totals[1], "hq_heartbeat ctxs");
    }
    if (rc) return rc;

    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) != hipSuccess) {
        (void)hipGetLastError();
        ms = 0.f;
    }
    out->words = h->words;
    out->n_groups = n;
    out->lags = h->lags;
    out->n_lags = h->totals[0];
    out->ctxs = h->ctxs;
    out->n_ctxs = h->totals[1];
    out->n_messages = h->totals[3];
    out->gpu_ns = (uint64_t)((double)ms * 1e6);
    return HQ_OK;
}
