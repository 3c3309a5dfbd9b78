// hq_heartbeat.h — the leader heartbeat broadcast of a device worker (hq_worker_heartbeats),
// shared between hq_worker_hb.cpp (plain C++: the flush, the checks, the host worker's own form) and
// hq_heartbeat.hip (the kernels and their buffers). Internal to libhipquorum.so.
#pragma once

#include <cstdint>

#include "../../include/hipquorum.h"
#include "hq_dstep.h"

struct hq_hb_dev;     // the buffers of one device worker's heartbeat calls

// hq_hb_dev_run's *error
constexpr uint32_t kHbErrHandle = 1;   // a listed handle at or beyond the state's group count
constexpr uint32_t kHbErrState = 2;    // a group record the kernels cannot take (internal)

int hq_hb_dev_open(hq_ctx *ctx, hq_hb_dev **out);
void hq_hb_dev_close(hq_hb_dev *h);
// The heartbeats of groups[0 .. n) (host memory; NULL: handles 0 .. n - 1; 0 < n < 2^28) over the
// resident state `st` of n_member_records members. HQ_E_INVAL with *error set when a kernel
// refused its input (then *out is not written); *out's arrays are h's pinned buffers, valid until
// its next run.
int hq_hb_dev_run(hq_hb_dev *h, const hq_dstate_view *st, uint64_t n_member_records, uint64_t n,
                  const uint32_t *groups, hq_heartbeat_output *out, uint32_t *error);

// ---- hq_worker_heartbeat_batches: the same heartbeats marshalled on the device as MessageBatch
// bytes (hq_heartbeat_wire.hip; the marshaller itself is hq_heartbeat_wire.h) ----
struct hq_hbw_dev;    // the buffers of one device worker's calls, and its route column

constexpr uint32_t kHbErrRoute = 4;    // hq_hbw_dev_run's *error: a route >= n_dest (not HQ_ROUTE_NONE)

int hq_hbw_dev_open(hq_ctx *ctx, hq_hbw_dev **out);
void hq_hbw_dev_close(hq_hbw_dev *h);
// rows [g0, g1) of the host column `routes` (16 words per group, n_groups groups) to the device
// column, which is grown to n_groups rows (then every row is copied)
int hq_hbw_dev_put_routes(hq_hbw_dev *h, const uint16_t *routes, uint64_t n_groups, uint64_t g0,
                          uint64_t g1);
// As hq_hb_dev_run, for the checked cfg; the route column holds st->n_groups rows. *out's arrays
// are h's pinned buffers, valid until its next run.
int hq_hbw_dev_run(hq_hbw_dev *h, const hq_dstate_view *st, uint64_t n_member_records, uint64_t n,
                   const uint32_t *groups, const hq_heartbeat_wire_config *cfg,
                   hq_heartbeat_batches *out, uint32_t *error);

#if defined(__HIPCC__)
// What the kernels of hq_heartbeat.hip and hq_heartbeat_wire.hip read of the resident records.
namespace hqhb {

// a member's fields the broadcast reads: match, and its position in the caller's list
struct MemberRef {
    uint64_t match;
    uint32_t order;
};

__device__ inline MemberRef load_member(const hq_dmember *m) {
    const uint64_t *p = reinterpret_cast<const uint64_t *>(m);
    const uint64_t tail = p[2];                       // role, active, order, pad
    return MemberRef{p[1], (uint32_t)(tail >> 16) & 0xFFu};
}

// the group's fields of the broadcast (hq_dgroup_load, hq_dstep.h)
struct GroupRef {
    uint64_t term, committed;
    uint32_t mem, n_members, n_voting, n_reads;
    bool sends;                                       // a leader that is not suspended
};

__device__ inline GroupRef load_group(const hq_dgroup *g) {
    const hq_dgroup_fields f = hq_dgroup_load(g);
    return GroupRef{f.term, f.committed, f.mem, f.n_members, f.n_voting, f.n_reads,
                    f.state == HQ_STATE_LEADER && !(f.flags & kDSuspended)};
}

// the record checks the kernels rely on (the worker's own uploads satisfy them); a record without
// members is a vacant handle's tombstone (hq_worker_stop_groups), which sends nothing
__device__ inline bool group_ok(uint64_t n_state_members, const GroupRef &g) {
    return (g.n_members >= 1 || !g.sends) && g.n_members <= kDMembers && g.n_voting <= g.n_members &&
           g.n_reads <= kDReads && (uint64_t)g.mem + g.n_members <= n_state_members;
}

// The word of group h (h below the state's group count): bit i — member i of the caller's list
// is sent a Heartbeat, bit 16 + i — its match is behind the committed index; *lo / *hi the ctx the
// heartbeats carry (readIndex.peepCtx: the queue's tail, or 0 / 0). A record the kernels cannot
// take gives 0 and kHbErrState in *err.
__device__ inline uint32_t word_of(const hq_dgroup *groups, const hq_dread *reads,
                                   const hq_dmember *members, uint64_t n_state_members, uint64_t h,
                                   uint64_t *lo, uint64_t *hi, uint32_t *err,
                                   GroupRef *group = nullptr) {
    const GroupRef g = load_group(groups + h);
    if (group) *group = g;
    *lo = *hi = 0;
    if (!group_ok(n_state_members, g)) {
        *err |= kHbErrState;
        return 0;
    }
    if (!g.sends) return 0;
    if (g.n_reads) {
        const hq_dread *r = reads + h * kDReads + (g.n_reads - 1);
        *lo = r->low;
        *hi = r->high;
    }
    const bool zero_ctx = (*lo | *hi) == 0;
    // pool order: the node, the other voting members, the observers (with a zero ctx)
    const uint32_t end = zero_ctx ? g.n_members : g.n_voting;
    const hq_dmember *m = members + g.mem;
    uint32_t word = 0;
    bool bad = false;
    for (uint32_t s = 1; s < end; ++s) {
        const MemberRef r = load_member(m + s);
        bad |= r.order >= kDMembers;
        const uint32_t bit = 1u << (r.order & 15u);
        word |= bit | (r.match < g.committed ? bit << 16 : 0u);
    }
    if (bad) {
        *err |= kHbErrState;
        return 0;
    }
    return word;
}

}  // namespace hqhb
#endif
