// hq_hb_received.h — the follower side of heartbeats on a step worker
// (hq_worker_heartbeats_received, include/hipquorum.h "heartbeats received"): what Peer.Handle does
// with a received Heartbeat as a function of the resident (term, state, committed, last_index):
// onMessageTermNotMatched (raft.go:1416-1452), handleFollowerHeartbeat / handleCandidateHeartbeat
// (raft.go:1869-1873, 1963-1966), handleHeartbeatMessage (raft.go:1302-1310) and leaderIsAvailable
// (raft.go:1859-1861). Shared between hq_worker_hbrecv.cpp (plain C++: the C entries, the checks,
// the host worker's own loop), hq_hb_received.hip (the kernel over a device worker's resident
// records) and a stand-alone test program: the per-message transition below is the one source all
// three compile. Internal to libhipquorum.so.
#pragma once

#include <cstdint>

#include "../../include/hipquorum.h"
#include "hq_dstep.h"

#if defined(__HIPCC__)
#define HQ_HBR_HD __host__ __device__
#else
#define HQ_HBR_HD
#endif

// what the path reads and writes of a group: the caller loads it from its record, runs the group's
// messages through hbr_message and stores back what changed. `reset`: becomeFollower
// ran at least once (raft.reset, raft.go:991-1010): the caller clears the votes, drops the pending
// reads and resets the members (every match 0 but the node's own at `last`, active flags cleared).
struct hq_hbr_group {
    uint64_t term, committed, last;
    uint32_t state;
    bool reset;
};

// a group's result as it accumulates over its messages (hq_hb_group_result's commit, leader,
// flags and n_resets)
struct hq_hbr_acc {
    uint64_t commit, leader;
    uint32_t flags, n_resets;
};

HQ_HBR_HD inline void hbr_become_follower(hq_hbr_group &g, hq_hbr_acc &a, uint64_t term) {
    g.state = HQ_STATE_FOLLOWER;                                   // raft.go:949-957
    g.term = term;
    g.reset = true;
    if (a.n_resets < 0xFFFFu) ++a.n_resets;
}

// One received Heartbeat handled by a group that is not suspended. Returns the reply's type (0:
// none); its term is g.term after the call.
HQ_HBR_HD inline uint32_t hbr_message(hq_hbr_group &g, hq_hbr_acc &a, const hq_hb_received &m,
                                      uint32_t check_quorum) {
    if (m.term != 0 && m.term > g.term) {                          // raft.go:1425-1438
        hbr_become_follower(g, a, m.term);
    } else if (m.term != 0 && m.term < g.term) {                   // raft.go:1439-1450
        return check_quorum ? HQ_MSG_NOOP : 0u;
    }
    if (g.state == HQ_STATE_LEADER) return 0u;                     // raft.go:2043-2057: no handler
    if (g.state == HQ_STATE_CANDIDATE) hbr_become_follower(g, a, g.term);   // raft.go:1963-1966
    a.flags |= HQ_HBR_CONTACT;                                     // raft.go:1869-1873
    a.leader = m.from;
    if (m.commit > g.last) {                                       // commitTo: the host's log decides
        a.flags |= HQ_HBR_COMMIT_ABOVE_LAST;
    } else if (m.commit > g.committed) {                           // logentry.go commitTo
        g.committed = m.commit;
        a.flags |= HQ_HBR_COMMITTED;
    }
    if (m.commit > a.commit) a.commit = m.commit;
    return HQ_MSG_HEARTBEAT_RESP;                                  // raft.go:1302-1310
}

// ---- the device path (hq_hb_received.hip) ----
struct hq_hbr_dev;                         // a device worker's pending contacts and its calls' buffers

int hq_hbr_dev_open(hq_ctx *ctx, hq_hbr_dev **out);
void hq_hbr_dev_close(hq_hbr_dev *r);
// The checked input over the resident state `st` (every listed handle below st->n_groups, each at
// most once; n_msgs = offsets[n_groups] < 2^31), of n_member_records members. *out's arrays are
// r's pinned buffers, valid until its next run. Waits for its kernel, also when something failed.
// HQ_E_STATE when the kernel met a record it cannot take (nothing of that group is written).
int hq_hbr_dev_run(hq_hbr_dev *r, const hq_dstate_mut *st, uint64_t n_member_records,
                   const hq_hb_received_input *in, hq_hb_received_output *out);
// The pending contacts as a device bitmap of at least `n_groups` bits (bit h of word h / 32) for
// the tick's kernels (hq_tick.hip), which read it, and clear a set timer's bit in it; *bitmap is
// NULL when no run has marked any since the last clear. hq_hbr_dev_clear zeroes it and waits.
int hq_hbr_dev_pending(hq_hbr_dev *r, uint64_t n_groups, uint32_t **bitmap);
int hq_hbr_dev_clear(hq_hbr_dev *r);
// the tick zeroed the bitmap it was handed
void hq_hbr_dev_consumed(hq_hbr_dev *r);
