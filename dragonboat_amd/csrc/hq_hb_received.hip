// hq_hb_received.hip — the follower side of heartbeats on a device worker
// (hq_worker_heartbeats_received; include/hipquorum.h "heartbeats received"): a step interval's
// received Heartbeats handled where the state lives, the replies and per-group results stored
// straight into pinned memory, and the contacts of the next tick marked in a device bitmap.
//
// One kernel, one lane per listed group:
//   k_hb_received  the record's second, third and fourth 16 bytes (term, committed | last |
//                  mem, state, flags: the quads of hqhb::load_group, and `last`), the group's
//                  messages in order from the staged input (40 bytes each), the transition of
//                  hq_hb_received.h, one 16-byte store per reply at its message's index and two
//                  per result at the group's position. The record goes back only when it changed:
//                  (term, committed) as one 16-byte store, the state quad only after a reset. Only
//                  a group that reset reads its node id, rewrites its members' match and active
//                  fields in the pool and drops its pending reads (n_reads = 0, as the step's
//                  reset). A contact is a 32-bit atomicOr into the pending bitmap; the six counts
//                  are wave ballots (the per-group ones) and wave sums (the per-message ones) with
//                  one atomic add per wave and count.
// No LDS, no scratch, no workgroup waiting for another; the message loop is bounded by the checked
// offsets. The pending bitmap is this module's: hq_tick.hip's kernels read it beside the staged
// contact list, and the tick clears it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "hq_hb_received.h"
#include "hq_sidecar.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kCounts = 6;            // n_resp, n_noop, n_contact, n_committed, n_state_changed, n_suspended
constexpr uint32_t kErrHandle = 1, kErrOffsets = 2, kErrRecord = 4;

using Quad = ulonglong2;
static_assert(sizeof(hq_hb_reply) == 16 && sizeof(hq_hb_group_result) == 32 && sizeof(hq_hb_received) == 40,
              "the ABI's record sizes");

struct RecvK {
    hq_dgroup *groups;
    hq_dmember *members;
    uint64_t n_state_groups, n_state_members;
    const uint32_t *handles;       // device [n]
    const uint64_t *offsets;       // device [n + 1]
    const uint64_t *msgs;          // device [n_msgs x 5]: from, term, commit, hint, hint_high
    uint64_t n, n_msgs;
    uint32_t check_quorum;
    Quad *replies;                 // pinned host [n_msgs]
    Quad *results;                 // pinned host [n x 2]
    uint32_t *pending;             // device bitmap, n_state_groups bits
    unsigned long long *counts;    // device [kCounts]
    uint32_t *error;               // device
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (uint32_t d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;                                        // (lane 0 holds the wave's sum)
}

__global__ void __launch_bounds__(kBlock) k_hb_received(RecvK k) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t n_resp = 0, n_noop = 0, flags = 0, n_resets = 0;
    if (i < k.n) {
        const uint64_t h = k.handles[i], lo = k.offsets[i], hi = k.offsets[i + 1];
        uint32_t err = 0;
        if (h >= k.n_state_groups) err |= kErrHandle;
        if (lo > hi || hi > k.n_msgs) err |= kErrOffsets;
        if (!err) {
            Quad *rec = reinterpret_cast<Quad *>(k.groups + h);
            const Quad b = rec[1], c = rec[2];       // term, committed | last, term_start
            const uint4 d = reinterpret_cast<const uint4 *>(rec)[3];   // mem, 8 bytes, pad1
            const hq_dgroup_fields f = hq_dgroup_decode(b.x, b.y, d);
            const uint32_t n_members = f.n_members, state0 = f.state;
            const bool suspended = (f.flags & kDSuspended) != 0;
            if (n_members > kDMembers || (uint64_t)d.x + n_members > k.n_state_members) err |= kErrRecord;
            if (!err) {
                hq_hbr_group g{b.x, b.y, c.x, state0, false};
                hq_hbr_acc a{0, 0, 0, 0};
                if (suspended) {
                    a.flags = HQ_HBR_SUSPENDED;
                    for (uint64_t m = lo; m < hi; ++m) k.replies[m] = Quad{0, 0};
                } else {
                    for (uint64_t m = lo; m < hi; ++m) {
                        const uint64_t *p = k.msgs + m * 5;
                        const hq_hb_received msg{p[0], p[1], p[2], p[3], p[4]};
                        const uint32_t type = hbr_message(g, a, msg, k.check_quorum);
                        k.replies[m] = Quad{type ? g.term : 0, (uint64_t)type};
                        n_resp += type == HQ_MSG_HEARTBEAT_RESP;
                        n_noop += type == HQ_MSG_NOOP;
                    }
                    if (g.term != b.x || g.committed != b.y) rec[1] = Quad{g.term, g.committed};
                    if (g.reset) {
                        // raft.reset: votes cleared, pending reads dropped, the members' matches
                        // and active flags (the step's reset, hq_dstep_step.hip)
                        uint4 q = d;
                        q.y = (d.y & 0xFFFFu) | (uint32_t)HQ_STATE_FOLLOWER << 16;   // granted 0
                        q.z = d.z & 0xFF00FF00u;                                     // rejected, n_reads 0
                        reinterpret_cast<uint4 *>(rec)[3] = q;
                        const uint64_t node_id = rec[0].y;
                        uint64_t *mp = reinterpret_cast<uint64_t *>(k.members + d.x);
                        for (uint32_t s = 0; s < n_members; ++s, mp += 3) {
                            mp[1] = mp[0] == node_id ? g.last : 0;
                            mp[2] &= ~(uint64_t)0xFF00u;                             // active
                        }
                    }
                    if (a.flags & HQ_HBR_CONTACT) atomicOr(k.pending + (h >> 5), 1u << (h & 31u));
                }
                flags = a.flags;
                n_resets = a.n_resets;
                k.results[2 * i] = Quad{g.term, a.commit};
                k.results[2 * i + 1] =
                    Quad{a.leader, (uint64_t)g.state | (uint64_t)a.flags << 32 | (uint64_t)a.n_resets << 48};
            }
        }
        if (err) atomicOr(k.error, err);
    }
    const uint64_t contact = __ballot(flags & HQ_HBR_CONTACT), committed = __ballot(flags & HQ_HBR_COMMITTED),
                   changed = __ballot(n_resets != 0), suspended = __ballot(flags & HQ_HBR_SUSPENDED);
    const uint32_t resp = wave_sum(n_resp), noop = wave_sum(n_noop);
    if (lane == 0) {
        if (resp) atomicAdd(k.counts + 0, (unsigned long long)resp);
        if (noop) atomicAdd(k.counts + 1, (unsigned long long)noop);
        if (contact) atomicAdd(k.counts + 2, (unsigned long long)__popcll(contact));
        if (committed) atomicAdd(k.counts + 3, (unsigned long long)__popcll(committed));
        if (changed) atomicAdd(k.counts + 4, (unsigned long long)__popcll(changed));
        if (suspended) atomicAdd(k.counts + 5, (unsigned long long)__popcll(suspended));
    }
}

}  // namespace

struct hq_hbr_dev : hq::Sidecar {      // (dev: the kCounts counts, then the error word; totals: the same)
    hq::DevBuf<uint32_t> pending;      // device bitmap: the contacts of the next tick; every word
                                       // defined (zero beyond what was marked)
    bool marked = false;               // a run may have set a bit since the last clear
    hq::DevBuf<uint32_t> handles;      // device: a call's input
    hq::DevBuf<uint64_t> offsets, msgs;
    hq::PinBuf<hq_hb_reply> replies;   // pinned
    hq::PinBuf<hq_hb_group_result> results;
};

int hq_hbr_dev_open(hq_ctx *ctx, hq_hbr_dev **out) {
    return hq::sidecar_open(ctx, out, "hq_hb_received counts", (kCounts + 1) * 8);
}

void hq_hbr_dev_close(hq_hbr_dev *r) { hq::sidecar_close(r); }

namespace {

// the pending bitmap grown with the handle space: the old words copied, the new ones zero
int grow_pending(hq_hbr_dev *r, uint64_t n_groups) {
    return r->pending.grow_keep(r->ctx, hq::words32(n_groups), r->marked ? r->pending.cap() : 0, 0,
                                "hq_hb_received contacts");
}

}  // namespace

int hq_hbr_dev_run(hq_hbr_dev *r, const hq_dstate_mut *st, uint64_t n_member_records,
                   const hq_hb_received_input *in, hq_hb_received_output *out) {
    hq_ctx *ctx = r->ctx;
    hipStream_t s = ctx->stream;
    const char *const what = "hq_worker_heartbeats_received";
    const uint64_t n = in->n_groups;
    if (n == 0 || n >= (1ull << 28)) return HQ_E_INVAL;
    const uint64_t n_msgs = in->offsets[n];
    if (n_msgs >= (1ull << 31)) return HQ_E_INVAL;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc) rc = grow_pending(r, st->n_groups);
    if (!rc) rc = r->handles.grow(ctx, n, what);
    if (!rc) rc = r->offsets.grow(ctx, n + 1, what);
    if (!rc) rc = r->msgs.grow(ctx, std::max<uint64_t>(n_msgs, 1) * 5, what);
    if (!rc) rc = r->replies.grow(ctx, std::max<uint64_t>(n_msgs, 1), what);
    if (!rc) rc = r->results.grow(ctx, n, what);
    if (rc) return rc;

    RecvK k{};
    k.groups = st->groups;
    k.members = st->members;
    k.n_state_groups = st->n_groups;
    k.n_state_members = n_member_records;
    k.handles = r->handles;
    k.offsets = r->offsets;
    k.msgs = r->msgs;
    k.n = n;
    k.n_msgs = n_msgs;
    k.check_quorum = in->check_quorum;
    k.replies = reinterpret_cast<Quad *>(r->replies.get());
    k.results = reinterpret_cast<Quad *>(r->results.get());
    k.pending = r->pending;
    k.counts = reinterpret_cast<unsigned long long *>(r->dev.get());
    k.error = reinterpret_cast<uint32_t *>(r->dev + kCounts);

    rc = hq::check_hip(ctx, hipMemsetAsync(r->dev, 0, (kCounts + 1) * 8, s), what);
    if (!rc) rc = hq::check_hip(ctx, hipMemcpyAsync(r->handles, in->groups, n * 4, hipMemcpyHostToDevice, s), what);
    if (!rc)
        rc = hq::check_hip(ctx, hipMemcpyAsync(r->offsets, in->offsets, (n + 1) * 8, hipMemcpyHostToDevice, s), what);
    if (!rc && n_msgs)
        rc = hq::check_hip(ctx, hipMemcpyAsync(r->msgs, in->msgs, n_msgs * sizeof(hq_hb_received),
                                               hipMemcpyHostToDevice, s), what);
    // (gpu_ns is the kernel's time: the input's copies before it are the link's, not the kernel's)
    if (!rc) rc = hq::check_hip(ctx, hipEventRecord(r->ev0, s), "event");
    if (!rc) {
        r->marked = true;                            // (from here on a bit may be set)
        hipLaunchKernelGGL(k_hb_received, dim3((uint32_t)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, k);
        rc = hq::check_hip(ctx, hipGetLastError(), "k_hb_received");
    }
    if (!rc)
        rc = hq::check_hip(ctx, hipMemcpyAsync(r->totals, r->dev, (kCounts + 1) * 8, hipMemcpyDeviceToHost, s),
                           what);
    if (!rc) rc = hq::check_hip(ctx, hipEventRecord(r->ev1, s), "event");
    rc = hq::finish(ctx, rc, what);
    if (rc) return rc;
    if ((uint32_t)r->totals[kCounts])
        return hq::fail(ctx, HQ_E_STATE, "hq_hb_received: a listed handle, its offsets or its resident record "
                                         "is not what the host checked (internal)");
    out->replies = r->replies;
    out->n_msgs = n_msgs;
    out->results = r->results;
    out->n_groups = n;
    out->n_resp = r->totals[0];
    out->n_noop = r->totals[1];
    out->n_contact = r->totals[2];
    out->n_committed = r->totals[3];
    out->n_state_changed = r->totals[4];
    out->n_suspended = r->totals[5];
    out->gpu_ns = hq::elapsed_ns(r->ev0, r->ev1);
    return HQ_OK;
}

int hq_hbr_dev_pending(hq_hbr_dev *r, uint64_t n_groups, uint32_t **bitmap) {
    *bitmap = nullptr;
    if (!r || !r->marked) return HQ_OK;
    int rc = hq::check_hip(r->ctx, hipSetDevice(r->ctx->device), "hipSetDevice");
    if (!rc) rc = grow_pending(r, n_groups);
    if (!rc) *bitmap = r->pending;
    return rc;
}

void hq_hbr_dev_consumed(hq_hbr_dev *r) { r->marked = false; }

int hq_hbr_dev_clear(hq_hbr_dev *r) {
    if (!r || !r->marked) return HQ_OK;
    hq_ctx *ctx = r->ctx;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc)
        rc = hq::check_hip(ctx, hipMemsetAsync(r->pending, 0, r->pending.cap() * 4, ctx->stream),
                           "hq_hb_received contacts");
    rc = hq::finish(ctx, rc, "hq_hb_received contacts");
    if (!rc) r->marked = false;
    return rc;
}
