// hq_worker_k.h — the step worker of libhipquorum.so (include/hipquorum.h "step worker"): the
// caller side of the quorum kernels, in the shape of dragonboat's execEngine.processSteps
// (execengine.go:923-1000) driving node.handleEvents (node.go:1113-1157) for many groups. This
// header is the worker's record types and `struct hq_worker`; its roles are one file each:
//   hq_worker.cpp        the group store and its loaders, open / close
//   hq_worker_host.cpp   the host worker's step (events on the host, decisions in GPU passes)
//   hq_worker_dev.cpp    the device worker's mirror and step; the step entry points
//   hq_worker_hb.cpp     leader heartbeats, compact and as MessageBatch bytes
//   hq_worker_lists.cpp  membership changes and the listed groups' fetch / resume
//   hq_worker_lifecycle.cpp  groups started and stopped on a running worker, pool compaction
//   hq_worker_tick.cpp   the Raft timers: one tick of every group, the listed timers' get / set
//   hq_worker_hbrecv.cpp received heartbeats: the follower side, and the replies as wire messages
// All of them plain C++ (no HIP headers): the worker is a client of the same ABI a cgo binding
// would use. Every C entry's body runs inside `guarded` (hq_guard.h).
//
// A device worker's calls beside the step each have a device module behind an opaque struct
// (hq_hb_dev, hq_hbw_dev, hq_cfg_dev, hq_groups_dev, hq_pool_dev, hq_tick_dev, hq_hbr_dev: kernels
// and their buffers in the .hip file of the same name). The modules share one scaffold,
// hq_sidecar.h: owning buffers, one open and one close, and one rule that the worker relies on:
// nothing of a call stays queued behind its return, whatever it returns (but a successful
// hq_tick_dev_invalidate, which the tick, get or set after tick_flush is queued behind). So a list,
// a config or a staging buffer handed to hq_*_dev_* is the caller's again when the call is back.
//
// Storage is flat: one fixed-size record per group, its members in one pool (voting slots
// first, in slot order, so packing a group's match row is a contiguous copy) and pending
// ReadIndex queues in a pool of fixed 8-entry blocks.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/hipquorum.h"
#include "hq_config.h"
#include "hq_dstep.h"
#include "hq_groups.h"
#include "hq_hb_received.h"
#include "hq_guard.h"
#include "hq_heartbeat.h"
#include "hq_heartbeat_wire.h"
#include "hq_pool.h"
#include "hq_tick.h"

namespace hq::wk {

constexpr uint32_t kMaxReads = 8;         // pending ReadIndex ctxs per group (k_ri_multi K_max)
constexpr uint16_t kNoAck = 0xFFFF;
constexpr uint16_t kMaxOrdinal = 0xFFF0;  // acks per run before a run is cut
constexpr uint32_t kNone = 0xFFFFFFFFu;

struct Member {                           // a remote, witness or observer of one group
    uint64_t node_id, match;
    uint8_t role, active;
    uint8_t order;                        // position in the caller's member list
    uint8_t pad[5];
};

struct ReadStatus {                       // readStatus (readindex.go:21-26)
    uint64_t index, from, low, high;
    uint16_t ord[HQ_MAX_VOTERS];          // first-ack ordinal in the current run
    uint8_t confirmed;                    // slots confirmed in earlier runs (ordinal 0)
};

struct ReadQueue {                        // readIndex.queue with its pending statuses
    uint32_t n;
    ReadStatus r[kMaxReads];
};

enum : uint8_t {
    kSuspended = 1, kTouched = 2, kInWork = 4,
    kCommitDue = 8, kRiDue = 16, kVoteDue = 32, kCqDue = 64,
    kDue = kCommitDue | kRiDue | kVoteDue | kCqDue,
    kVacant = 128,                        // a stopped group's handle: a tombstone (kSuspended, no
                                          // members, follower) until a start reuses it
};

struct Group {
    uint64_t cluster_id, node_id, term, committed, last, term_start;
    uint64_t committed0, cursor, ev_end;  // current step
    uint32_t mem;                         // first member in the pool; [0] is the node itself
    uint32_t rq;                          // read queue block, kNone when empty
    uint16_t ord;                         // acks recorded in the current run
    uint8_t n_members, mem_cap, n_voting, state, granted, rejected, flags;
    bool has(uint8_t f) const { return flags & f; }
    void set(uint8_t f) { flags |= f; }
    void clear(uint8_t f) { flags &= (uint8_t)~f; }
    bool pending() const { return flags & kDue; }
};

enum Verdict { CONSUMED, BARRIER, FALLBACK };

// Who a leader's heartbeat goes to (broadcastHeartbeatMessage, raft.go:826-848): the ctx it
// carries and the receiving members by their place in the caller's member list. The device's
// view of the same rule is hb_targets (hq_heartbeat.h).
struct HeartbeatTo {
    uint64_t lo, hi;                      // readIndex.peepCtx: the queue's tail, 0 / 0 for none
    const Member *by_order[kDMembers];
};

inline uint64_t now_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

inline hq_dmember to_device_member(const Member &m) {    // a pool record as the device keeps it
    return hq_dmember{m.node_id, m.match, m.role, m.active, m.order, {0, 0, 0, 0, 0}};
}

}  // namespace hq::wk

struct hq_worker {
    using Member = hq::wk::Member;
    using ReadStatus = hq::wk::ReadStatus;
    using ReadQueue = hq::wk::ReadQueue;
    using Group = hq::wk::Group;
    using Verdict = hq::wk::Verdict;
    using HeartbeatTo = hq::wk::HeartbeatTo;

    hq_ctx *ctx = nullptr;
    int device = -1;
    uint32_t n_max = 0;
    // HQ_WORKER_ON_DEVICE: the group state lives on the GPU (hq_dstep*.hip) and a step is one
    // launch pair; the host records below are a mirror, refreshed from the device on demand
    hq_dstep *dstep = nullptr;
    bool host_stale = false;              // the device holds newer state than the mirror
    uint64_t dev_groups = 0, dev_members = 0;   // records already on the device
    std::vector<uint32_t> dirty;          // handles changed on the host since the last upload
    hq_dstep_out dout{};
    hq_hb_dev *hb = nullptr;              // device worker: hq_worker_heartbeats' buffers (first call)
    std::vector<uint32_t> hb_words;       // host worker: its heartbeat output
    std::vector<hq_heartbeat_lag> hb_lags;
    std::vector<hq_heartbeat_ctx> hb_ctxs;
    // hq_worker_heartbeat_batches: the route column (16 words per group; rows [lo, hi) not yet on
    // the device), a device worker's buffers (first call), a host worker's output
    std::vector<uint16_t> routes;
    uint64_t routes_lo = 0, routes_hi = 0, routes_on_dev = 0;   // (rows the device column holds)
    hq_hbw_dev *hbw = nullptr;
    std::vector<uint8_t> hbw_bytes;
    std::vector<hq_heartbeat_batch> hbw_batches;
    std::vector<hb_fields> hbw_msgs;
    std::vector<uint64_t> hbw_first;
    // hq_worker_config_changes: a device worker's buffers (first call), the call's descriptors
    // and its output (a host worker's status column; the commit records of both)
    hq_cfg_dev *cfg = nullptr;
    std::vector<hq_cfg_desc> cc_desc;
    std::vector<uint8_t> cc_cap;          // a moving group's new member range
    std::vector<uint32_t> cc_status;
    std::vector<hq_commit_event> cc_commits;
    uint64_t readbacks = 0;               // sync_from_device calls that copied the state back
    // hq_worker_get_groups / _set_groups: a device worker's buffers (first call) and the last
    // get_groups' output
    hq_groups_dev *grp = nullptr;
    std::vector<hq_worker_group> gg_groups;
    std::vector<hq_member> gg_members;
    std::vector<hq_read_status> gg_reads;
    std::vector<uint64_t> gg_moff, gg_roff;
    std::vector<uint16_t> gg_granted, gg_rejected, gg_rconf;
    std::vector<hq_event> decoded;        // host worker: a stream step's rows
    std::vector<uint64_t> sized_off, sized_boff;   // host worker: a sized stream's prefixes
    std::vector<uint32_t> sized_groups;            // and its implicit handles
    std::string err;
    std::vector<Group> groups;
    std::vector<Member> pool;
    std::vector<ReadQueue> rqs;
    std::vector<uint32_t> rq_free;
    std::unordered_map<uint64_t, uint32_t> index;   // cluster_id -> handle (live groups only)
    // group lifecycle (hq_worker_lifecycle.cpp): the vacant handles as a stack, the count of
    // start / stop calls that changed anything, a device worker's compaction buffers (first call)
    std::vector<uint32_t> vacant;
    uint64_t epoch = 0;
    hq_pool_dev *poolc = nullptr;
    // raft timers (hq_worker_tick.cpp): the checked config (tick_on: one was set); a host worker's
    // timers, one per handle, its contact bitmap and its due lists; a device worker's timer array
    // and buffers (first call) and the handles whose timers come back reset (or all of them)
    bool tick_on = false, tick_reset_all = false;
    hq_tick_params tick_p{};
    std::vector<hq_tick_timer> timers;
    std::vector<uint32_t> tk_contact, tk_lists[kTickLists];
    hq_tick_dev *tickd = nullptr;
    std::vector<uint32_t> tick_resets;
    // received heartbeats (hq_worker_hbrecv.cpp): a host worker's output and its pending contacts
    // (bit h of word h / 32; hr_marked: a bit may be set); a device worker's buffers and pending
    // contacts (first call)
    std::vector<hq_hb_reply> hr_replies;
    std::vector<hq_hb_group_result> hr_results;
    std::vector<uint32_t> hr_pending, hr_seen;    // (hr_seen: a call's listed handles, for its checks)
    bool hr_marked = false;
    hq_hbr_dev *hbr = nullptr;
    // step scratch (`touched`: the groups a call has marked kTouched, unmarked before it returns)
    const hq_step_input *in = nullptr;
    std::vector<uint32_t> work, next_work, touched;
    std::vector<uint32_t> l_commit, l_ri, l_vote, l_cq;
    // outputs
    std::vector<hq_commit_event> commits;
    std::vector<hq_ready_to_read> ready;
    std::vector<hq_read_index_resp> resps;
    std::vector<hq_state_change> states;
    std::vector<hq_dropped_read> dropped;
    std::vector<uint64_t> deferred;
    std::vector<uint64_t> fallback;
    uint64_t decisions = 0;
    uint64_t t_pack = 0, t_device = 0, t_apply = 0;
    // staging: one pinned host buffer mirrored by one device buffer per pass
    void *host = nullptr, *dev = nullptr;
    size_t cap = 0;

    int fail(int code, const std::string &m) {
        err = m;
        return code;
    }
    int hq(int rc, const char *what) {
        if (rc) err = std::string(what) + ": " + hq_last_error(ctx);
        return rc;
    }
    Member *members(Group &g) { return pool.data() + g.mem; }
    int member_of(const Group &g, uint64_t id) const {
        const Member *m = pool.data() + g.mem;
        for (int i = 0; i < g.n_members; ++i)
            if (m[i].node_id == id) return i;
        return -1;
    }
    ReadQueue *reads(const Group &g) { return g.rq == hq::wk::kNone ? nullptr : &rqs[g.rq]; }
    const ReadQueue *reads(const Group &g) const {
        return g.rq == hq::wk::kNone ? nullptr : &rqs[g.rq];
    }
    uint32_t rq_alloc() {
        if (!rq_free.empty()) {
            const uint32_t i = rq_free.back();
            rq_free.pop_back();
            rqs[i].n = 0;
            return i;
        }
        rqs.emplace_back();
        rqs.back().n = 0;
        return (uint32_t)rqs.size() - 1;
    }
    void rq_release(Group &g) {
        if (g.rq != hq::wk::kNone) rq_free.push_back(g.rq);
        g.rq = hq::wk::kNone;
    }
    void unmark_touched() {
        for (uint32_t h : touched) groups[h].clear(hq::wk::kTouched | hq::wk::kInWork);
        touched.clear();
    }
    // the group store (hq_worker.cpp)
    int check_group(const hq_worker_group *src, const hq_member *m, int *self, int *n_voting);
    int load_group(Group &g, const hq_worker_group *src, const hq_member *m, bool fresh);
    int add_group(const hq_worker_group *g, const hq_member *members, uint32_t *handle);
    int check_listed(const char *entry, uint64_t h);
    // the host worker's step (hq_worker_host.cpp)
    int reserve(size_t bytes);
    int step(const hq_step_input *in, hq_step_output *out);
    int step_body(const hq_step_input *in, hq_step_output *out);
    int run_pass();
    // (the per-event chain: `inline`, defined and used in hq_worker_host.cpp alone, so that the
    // compiler may fold it into step as it did while the record types, and with them these
    // functions, had internal linkage)
    inline Verdict handle(Group &g, const hq_event &e, uint64_t ei);
    inline Verdict read_index(Group &g, uint64_t from, uint64_t low, uint64_t high, uint64_t ei);
    inline void advance(Group &g);
    // reference state transitions (host bookkeeping of raft.go:949-1010)
    inline void reset(Group &g, uint64_t term);   // (defined below: hq_worker_hbrecv.cpp resets too)
    inline void become_follower(Group &g, uint64_t term, uint32_t reason);
    inline void become_leader(Group &g);
    void push_state(const Group &g, uint32_t reason) {
        states.push_back({g.cluster_id, g.term, g.state, reason});
    }
    void defer(uint64_t ei) { deferred.push_back(ei); }
    // device mode (hq_worker_dev.cpp)
    void to_device_record(const Group &g, hq_dgroup &d, hq_dread *r, hq_dmember *m = nullptr) const;
    int sync_to_device();
    int sync_from_device();
    int step_on_device(const hq_dstep_in &in, hq_step_output *out);
    int device_step_done(int rc, const hq_dstep_in &in, hq_step_output *out, uint64_t t0,
                         uint64_t t1);
    int step_stream(const hq_step_stream *in, hq_step_output *out);
    // heartbeats (hq_worker_hb.cpp)
    bool heartbeat_to(const Group &g, HeartbeatTo &to) const;
    int heartbeats(uint64_t n, const uint32_t *list, hq_heartbeat_output *out);
    int heartbeat_batches(uint64_t n, const uint32_t *list, const hq_heartbeat_wire_config *cfg,
                          hq_heartbeat_batches *out);
    // membership changes and listed groups (hq_worker_lists.cpp)
    template <class Handle, class Check>
    int check_distinct(uint64_t n, const char *twice, Handle &&handle_of, Check &&check);
    int config_desc(const Group &g, const hq_config_change &c, uint32_t limit, hq_cfg_desc &d);
    void config_edit(Group &g, uint32_t h, const hq_cfg_desc &d, uint8_t new_cap);
    int config_changes(uint64_t n, const hq_config_change *ch, hq_config_output *out);
    bool emit_group(const hq_dgroup &d, const hq_dread *r, const hq_dmember *m);
    int get_groups(uint64_t n, const uint32_t *handles, hq_groups_output *out);
    int set_groups(uint64_t n, const hq_worker_group *gs, const hq_member *ms, uint64_t *gpu_ns);
    // group lifecycle (hq_worker_lifecycle.cpp)
    bool live(uint64_t h) const { return h < groups.size() && !groups[h].has(hq::wk::kVacant); }
    void reset_route_row(uint32_t h);
    int scatter_records(const char *entry, uint64_t n, const uint32_t *hs, uint64_t *gpu_ns);
    int start_groups(uint64_t n, const hq_worker_group *gs, const hq_member *ms, uint32_t *handles,
                     uint64_t *gpu_ns);
    int stop_groups(uint64_t n, const uint32_t *handles, uint64_t *gpu_ns);
    uint64_t live_member_records() const;
    int compact(uint64_t *gpu_ns);
    // raft timers (hq_worker_tick.cpp)
    void tick_touch(uint32_t h);
    int tick_flush(const char *entry);
    int set_tick_config(const hq_tick_config *cfg);
    int tick(uint64_t n_contact, const uint32_t *contact, hq_tick_output *out);
    int get_timers(uint64_t n, const uint32_t *handles, hq_timer *out);
    int set_timers(uint64_t n, const uint32_t *handles, const hq_timer *ts);
    // received heartbeats (hq_worker_hbrecv.cpp)
    bool contact_pending(uint64_t h) const {
        return hr_marked && (h >> 5) < hr_pending.size() && ((hr_pending[h >> 5] >> (h & 31u)) & 1u);
    }
    int clear_pending_contacts();
    int heartbeats_received(const hq_hb_received_input *in, hq_hb_received_output *out);
};

inline void hq_worker::reset(Group &g, uint64_t term) {   // raft.reset, raft.go:991-1010
    g.term = term;
    g.granted = g.rejected = 0;
    rq_release(g);
    Member *m = members(g);
    for (int i = 0; i < g.n_members; ++i) {          // resetRemotes/Observers/Witnesses
        m[i].match = m[i].node_id == g.node_id ? g.last : 0;
        m[i].active = 0;
    }
}

// Marks each of a list's n groups kTouched while they are checked, so that a group listed twice
// is seen, and always unmarks them (hq_worker_lists.cpp, hq_worker_lifecycle.cpp): handle_of(i, h) finds entry i's group (or fails), check(i, h)
// is the entry's own check. A refused list changes nothing.
template <class Handle, class Check>
int hq_worker::check_distinct(uint64_t n, const char *twice, Handle &&handle_of, Check &&check) {
    struct Unmark {
        hq_worker &w;
        ~Unmark() { w.unmark_touched(); }
    } unmark{*this};
    touched.clear();
    touched.reserve(n);
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t h = 0;
        if (int rc = handle_of(i, h)) return rc;
        if (groups[h].has(hq::wk::kTouched)) return fail(HQ_E_INVAL, twice);
        if (int rc = check(i, h)) return rc;
        groups[h].set(hq::wk::kTouched);
        touched.push_back(h);
    }
    return HQ_OK;
}

// A C entry of the worker: HQ_E_INVAL for no worker, else the body's code, or an exception's
// (hq_guard.h) with its message in hq_worker_last_error.
template <class Body>
int guarded(hq_worker *w, const char *entry, Body &&body) {
    if (!w) return HQ_E_INVAL;
    return hq::guard(entry, [w](int code, const std::string &m) { w->fail(code, m); }, body);
}
