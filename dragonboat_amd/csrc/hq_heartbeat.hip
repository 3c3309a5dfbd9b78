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

#include "hq_heartbeat.h"
#include "hq_sidecar.h"

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

struct hq_hb_dev : hq::Sidecar {       // (dev: the error word in its low half, the messages' sum)
    hq::DevBuf<uint32_t> list;         // device copies / columns, grown on demand
    hq::DevBuf<uint64_t> meta, scan;
    hq::DevBuf<uint8_t> scan_tmp;      // hipcub's temporary
    hq::PinBuf<uint32_t> words;        // pinned host
    hq::PinBuf<hq_heartbeat_lag> lags;
    hq::PinBuf<hq_heartbeat_ctx> ctxs;
};

int hq_hb_dev_open(hq_ctx *ctx, hq_hb_dev **out) { return hq::sidecar_open(ctx, out, "hq_heartbeat"); }

void hq_hb_dev_close(hq_hb_dev *h) { hq::sidecar_close(h); }

int hq_hb_dev_run(hq_hb_dev *h, const hq_dstate_view *st, uint64_t n_member_records, uint64_t n,
                  const uint32_t *groups, hq_heartbeat_output *out, uint32_t *error) {
    hq_ctx *ctx = h->ctx;
    hipStream_t s = ctx->stream;
    const char *const what = "hq_worker_heartbeats";
    *error = 0;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc) rc = h->words.grow(ctx, n, "hq_heartbeat words");
    if (!rc) rc = h->meta.grow(ctx, n, "hq_heartbeat words");
    if (!rc) rc = h->scan.grow(ctx, n + 1, "hq_heartbeat scan");
    if (!rc && groups) rc = h->list.grow(ctx, n, "hq_heartbeat list");
    // (a first call's record buffers: a record for one group in four, grown to what a call needs)
    if (!rc) rc = h->lags.grow(ctx, std::max<uint64_t>(n / 4, 256), "hq_heartbeat lags");
    if (!rc) rc = h->ctxs.grow(ctx, std::max<uint64_t>(n / 4, 256), "hq_heartbeat ctxs");
    if (rc) return rc;

    uint64_t *const n_messages = h->dev + 1;
    HbK k{};
    k.groups = st->groups;
    k.reads = st->reads;
    k.members = st->members;
    k.n_state_groups = st->n_groups;
    k.n_state_members = n_member_records;
    k.list = groups ? h->list.get() : nullptr;
    k.n = n;
    k.words = h->words;
    k.meta = h->meta;
    k.scan = h->scan;
    k.totals = h->totals;
    k.error = h->error();
    k.n_messages = n_messages;

    const hipcub::TransformInputIterator<uint64_t, HbCount, hipcub::CountingInputIterator<uint64_t>>
        counts(hipcub::CountingInputIterator<uint64_t>(0), HbCount{h->meta, n});
    const hipcub::TransformInputIterator<uint64_t, HbMessages, hipcub::CountingInputIterator<uint64_t>>
        messages(hipcub::CountingInputIterator<uint64_t>(0), HbMessages{h->meta});
    const int items = (int)n;     // (n < 2^28)
    size_t tmp = 0, tmp2 = 0;
    rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, counts, h->scan.get(), items + 1, s),
                       "hipcub scan size");
    if (!rc)
        rc = hq::check_hip(ctx, hipcub::DeviceReduce::Sum(nullptr, tmp2, messages, n_messages, items, s),
                           "hipcub sum size");
    if (!rc) rc = h->scan_tmp.grow(ctx, std::max(tmp, tmp2), "hq_heartbeat scan");
    if (rc) return rc;            // (nothing is queued yet; from here on every return is finish's)

    if (groups)
        rc = hq::check_hip(ctx, hipMemcpyAsync(h->list, groups, n * 4, hipMemcpyHostToDevice, s),
                           "hq_heartbeat list");
    if (!rc) rc = hq::check_hip(ctx, hipMemsetAsync(h->dev, 0, 16, s), "memset");
    if (!rc) rc = hq::check_hip(ctx, hipEventRecord(h->ev0, s), "event");
    const uint32_t g1 = (uint32_t)((n + kBlock - 1) / kBlock), g2 = (uint32_t)(n / kBlock + 1);
    if (!rc) {
        hipLaunchKernelGGL(k_hb_words, dim3(g1), dim3(kBlock), 0, s, k);
        rc = hq::check_hip(ctx, hipGetLastError(), "k_hb_words");
    }
    if (!rc) {
        size_t t = h->scan_tmp.cap();
        rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(h->scan_tmp.get(), t, counts, h->scan.get(),
                                                                  items + 1, s), "hipcub scan");
        t = h->scan_tmp.cap();    // (the same temporary: the two run one after the other)
        if (!rc)
            rc = hq::check_hip(ctx, hipcub::DeviceReduce::Sum(h->scan_tmp.get(), t, messages, n_messages,
                                                              items, s), "hipcub sum");
    }
    // the records; again with larger buffers when a total passed a capacity (nothing was written
    // out of bounds; the words, the column and the scan stand)
    for (int pass = 0; !rc; ++pass) {
        k.lags = h->lags;
        k.ctxs = h->ctxs;
        k.lag_cap = h->lags.cap();
        k.ctx_cap = h->ctxs.cap();
        hipLaunchKernelGGL(k_hb_records, dim3(g2), dim3(kBlock), 0, s, k);
        rc = hq::check_hip(ctx, hipGetLastError(), "k_hb_records");
        if (!rc) rc = hq::check_hip(ctx, hipEventRecord(h->ev1, s), "event");
        rc = hq::finish(ctx, rc, what);
        if (rc) return rc;
        if (h->totals[2]) {
            *error = (uint32_t)h->totals[2];
            return HQ_E_INVAL;
        }
        if (h->totals[0] <= h->lags.cap() && h->totals[1] <= h->ctxs.cap()) break;
        if (pass) return hq::fail(ctx, HQ_E_STATE, "hq_worker_heartbeats: record totals changed");
        rc = h->lags.grow(ctx, h->totals[0], "hq_heartbeat lags");
        if (!rc) rc = h->ctxs.grow(ctx, h->totals[1], "hq_heartbeat ctxs");
    }
    if (rc) return hq::finish(ctx, rc, what);

    out->words = h->words;
    out->n_groups = n;
    out->lags = h->lags;
    out->n_lags = h->totals[0];
    out->ctxs = h->ctxs;
    out->n_ctxs = h->totals[1];
    out->n_messages = h->totals[3];
    out->gpu_ns = hq::elapsed_ns(h->ev0, h->ev1);
    return HQ_OK;
}
