// hq_dstep_step.hip — the step kernels of the step worker's device engine (hq_worker_open_ex,
// HQ_WORKER_ON_DEVICE): the whole quorum side of execEngine.processSteps / node.handleEvents (execengine.go:923-1000,
// node.go:1113-1157) for many Raft groups in one launch, their state resident in HBM.
//
// One thread owns one group of the step and takes its events in order, exactly as the reference
// takes a node's queue one message at a time: Peer.Handle's membership filter (peer.go:186-198),
// onMessageTermNotMatched (raft.go:1416-1452), remote.tryUpdate + tryCommit per ReplicateResp
// (remote.go:123-133, raft.go:888-909, 1671-1700), the confirmed-set insert and readIndex.confirm
// per HeartbeatResp (readindex.go:77-116, raft.go:1702-1760), handleLeaderReadIndex
// (raft.go:1636-1669), the first-wins vote tally (raft.go:1062-1080, 1968-1985), CheckQuorum
// (raft.go:380-390, 1582-1588), campaign (raft.go:1082-1117), appendEntries (raft.go:911-922)
// and the state transitions (raft.go:949-1010). Every decision is taken at the event that
// triggers it, so no event waits for another's decision and a step is one launch, whatever the
// events (the host worker cuts runs at such barriers and needs several passes).
//
// The outputs are lists whose lengths are not known in advance: the kernel runs twice. Pass A
// takes every group's events, counts its records (and adds each wave's counts into per-wave
// sums), saves the state it found and writes the new state in place; the per-wave sums are
// scanned (hipcub, or k_scan_layout for a small step), k_step_lite scans the lanes of each wave
// by shuffles, and pass B replays, from the saved state, only the groups that have records other
// than their commit and one ReadyToRead — with the commits as a column (k_step_lite writes every
// group's word from the saved and the new committed index, and copies out the single
// ReadyToReads pass A kept) no group of a steady step is replayed — writing every record at its
// place, in input group order (each group's records as the host worker lists them; the host
// worker lists a step's records pass by pass). A step with an input error writes no state:
// k_step_restore puts the saved state back.
#include "hq_dstep_k.h"
#include "hq_launch.h"

namespace {

__device__ __forceinline__ bool is_response(uint32_t t) {   // internal/raft/utils.go
    return t == HQ_MSG_REPLICATE_RESP || t == HQ_MSG_REQUEST_VOTE_RESP ||
           t == HQ_MSG_HEARTBEAT_RESP || t == 20 || t == 8 || t == 9;
}

// A group's bytes read through one cached aligned 8-byte word: a varint byte costs a shift
// instead of a dependent byte load (a group's ~24 bytes take 3-4 loads instead of ~24; the
// input region keeps 8 bytes of slack past its last byte, so the aligned word never leaves it)
struct ByteReader {
    const uint8_t *p, *end;
    uintptr_t wa = 1;             // address of the cached word (never a valid aligned one at start)
    uint64_t w = 0;

    __device__ __forceinline__ bool more() const { return p < end; }
    __device__ __forceinline__ uint32_t next() {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        if ((a & ~uintptr_t(7)) != wa) {
            wa = a & ~uintptr_t(7);
            w = *reinterpret_cast<const uint64_t *>(wa);
        }
        ++p;
        return (uint32_t)(w >> (8 * (a & 7))) & 0xFF;
    }
};

// the device twin of hq_stream.cpp's decoder: one LEB128 varint
__device__ __forceinline__ bool dvar(ByteReader &r, uint64_t &v) {
    v = 0;
    for (int sh = 0; sh < 64; sh += 7) {
        if (!r.more()) return false;
        const uint32_t b = r.next();
        v |= (uint64_t)(b & 0x7F) << sh;
        if (b < 0x80) return true;
    }
    return false;
}

// a group's stream state the codes refer back to (hq_stream.cpp's Prev): its previous message
// term, its previous ReplicateResp's log_index (code 4), its previous HeartbeatResp's ctx (code
// 5), the previous message a run repeats (code 6; last 1 ReplicateResp, 2 HeartbeatResp, bit 2
// its reject, bit 3 a run in the consecutive form) and the run's events still to come (and, in
// the consecutive form, the next member's sender)
struct DPrev {
    uint64_t term = 0, index = 0, hint = 0, high = 0;
    bool have_index = false;
    uint32_t last = 0, run = 0, run_from = 0;
};

// one event of a group's stream
__device__ bool decode_event(ByteReader &r, DPrev &pv, hq_event &v) {
    v = hq_event{};
    if (pv.run == 0) {
        if (!r.more()) return false;
        // (peek: a run header is taken here, any other header below)
        const uintptr_t a = reinterpret_cast<uintptr_t>(r.p);
        if ((a & ~uintptr_t(7)) != r.wa) {
            r.wa = a & ~uintptr_t(7);
            r.w = *reinterpret_cast<const uint64_t *>(r.wa);
        }
        const uint32_t h0 = (uint32_t)(r.w >> (8 * (a & 7))) & 0xFF;
        if ((h0 & 7) == HQ_EV_MESSAGE && ((h0 >> 3) & 7) == 6) {
            (void)r.next();
            uint64_t m;
            if (!(pv.last & 3) || !dvar(r, m) || m == 0 || m > 0xFFFF) return false;
            pv.run = (uint32_t)m;
            pv.last &= 7u;
            if (h0 & 0x80) {       // the consecutive form: the first sender, the rest follow
                uint64_t f0;
                // (m <= 0xFFFF above; compared without the sum, which wraps for f0 near 2^64)
                if (!dvar(r, f0) || f0 > 0xFFFFFFFFull - m) return false;
                pv.run_from = (uint32_t)f0;
                pv.last |= 8u;
            }
        }
    }
    if (pv.run) {                  // a run member: the previous message with another sender
        --pv.run;
        v.kind = HQ_EV_MESSAGE;
        v.type = (pv.last & 3) == 1 ? HQ_MSG_REPLICATE_RESP : HQ_MSG_HEARTBEAT_RESP;
        v.reject = (pv.last >> 2) & 1;
        v.term = pv.term;
        if ((pv.last & 3) == 1) {
            v.log_index = pv.index;
        } else {
            v.hint = pv.hint;
            v.hint_high = pv.high;
        }
        if (pv.last & 8u) {
            v.from = pv.run_from++;
            return true;
        }
        return dvar(r, v.from);
    }
    const uint32_t h = r.next();
    v.kind = h & 7;
    if (v.kind == HQ_EV_READ) return dvar(r, v.hint) && dvar(r, v.hint_high);
    if (v.kind == HQ_EV_PROPOSE) return dvar(r, v.log_index);
    if (v.kind != HQ_EV_MESSAGE) return true;
    const uint32_t code = (h >> 3) & 7;
    uint64_t t = code == 0 || code == 4 ? HQ_MSG_REPLICATE_RESP
               : code == 1 ? HQ_MSG_REQUEST_VOTE_RESP
               : code == 2 || code == 5 ? HQ_MSG_HEARTBEAT_RESP
               : code == 3 ? HQ_MSG_READ_INDEX : 0;
    if (code == 7 && !dvar(r, t)) return false;
    if (code == 4 && !pv.have_index) return false;  // repeats an index the group has not sent
    v.type = (uint32_t)t;
    v.reject = (h >> 6) & 1;
    if (!dvar(r, v.from)) return false;
    if (!(h & 0x80) && !dvar(r, pv.term)) return false;
    v.term = pv.term;
    if ((code == 0 || code == 7) && !dvar(r, v.log_index)) return false;
    if (code == 4) v.log_index = pv.index;
    if ((code == 2 || code == 3 || code == 7) && !(dvar(r, v.hint) && dvar(r, v.hint_high)))
        return false;
    if (code == 5) {
        v.hint = pv.hint;
        v.hint_high = pv.high;
    }
    if (code == 0 || code == 4) {
        pv.index = v.log_index;
        pv.have_index = true;
    }
    if (code == 2 || code == 5) {
        pv.hint = v.hint;
        pv.high = v.hint_high;
    }
    pv.last = (code == 0 || code == 4 ? 1u : code == 2 || code == 5 ? 2u : 0u) | v.reject << 2;
    return true;
}

constexpr uint32_t kStageReady = 64;   // ReadyToRead records staged per wave in pass B
constexpr uint32_t kStageBytes = 16384;  // pass A: a workgroup's stream bytes staged in LDS

// pass A's chained scan of the ReadyToRead places (StepK::tiles, kTileVal): how long a tile waits
// for a predecessor's word before it gives up (kErrScan; the host then
// re-runs the copy-out without pass A's records): 0.1 s of the device's 100-MHz constant clock
// (wall_clock64, hipDeviceAttributeWallClockRate), whatever each poll costs
constexpr uint64_t kScanWaitTicks = 10000000;
__device__ __forceinline__ uint64_t tile_word(uint32_t step, uint32_t chunk, bool incl, uint32_t v) {
    return (uint64_t)step << 32 | (uint64_t)(chunk & 7) << 29 | (uint64_t)incl << 28 | (v & kTileVal);
}
__device__ __forceinline__ uint64_t tile_load(const uint64_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void tile_store(uint64_t *p, uint64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A workgroup's place in its launch: a ticket drawn at its start, so that a tile's predecessor in
// the chained scan has always started before it (resident or done: no wait on a workgroup not yet
// dispatched)
__device__ __forceinline__ uint32_t draw_ticket(uint32_t *ctr) {
    __shared__ uint32_t t;
    if (threadIdx.x == 0) t = atomicAdd(ctr, 1u);
    __syncthreads();
    return t;
}

// One group's state and its output cursor. WRITE = false: counting pass on a private copy;
// WRITE = true: the same sequence writing records and, at the end, the new state.
template <bool WRITE, int MC>   // MC: member slots held in registers (8 or MC)
struct Engine {
    const StepK &a;
    uint64_t i;                   // position of the group in the step's list
    hq_dgroup g;
    const hq_dmember *gm;         // the group's member records (node ids and roles read-only)
    // member state in registers: every index below is a compile-time constant (unrolled loops,
    // selects), so nothing of it lives in scratch; only the pending reads (rd) are indexed at run
    // time, and they are touched only while a group has reads pending
    uint64_t match[MC];
    uint64_t ids[MC];
    uint32_t active;              // bit s = member s active
    hq_dread *rd;                 // the pending reads: a separate local array (run-time indexed)
    uint32_t cnt[kLists];
    uint32_t base[kLists];
    // pass B: the wave's ReadyToRead records are staged in LDS from record stage_lo on (the
    // records of a wave's groups are consecutive) and written out by the wave as one contiguous
    // run of 16-byte lane stores: a 32-byte record stored per lane leaves half-filled lines
    // whose writes cross PCIe as small packets
    hq_ready_to_read *stage = nullptr;
    uint32_t stage_lo = 0;
    uint64_t c0 = 0;              // the group's committed index before the step
    // pass B over a group whose single ReadyToRead pass A put in its tile's slot (a step in list
    // mode replays every group): the record is not written again nor counted in the list
    bool slotted = false;

    __device__ __forceinline__ Engine(const StepK &k, uint64_t idx, uint32_t h, hq_dread *reads)
        : a(k), i(idx), rd(reads) {
        // pass A: the group's state (then saved, and overwritten by its new state); pass B: the
        // state pass A saved (node ids and roles never change in a step: the live records)
        g = WRITE ? k.groups_old[h] : k.groups[h];
        gm = k.members + g.mem;
        active = 0;
#pragma unroll
        for (uint32_t s = 0; s < MC; ++s) {
            match[s] = 0;
            ids[s] = 0;
            if (s < g.n_members) {
                match[s] = WRITE ? k.match_old[g.mem + s] : gm[s].match;
                ids[s] = gm[s].node_id;
                active |= (uint32_t)(WRITE ? (g.pad1 >> s) & 1 : gm[s].active != 0) << s;
            }
        }
        const hq_dread *rs = (WRITE ? k.reads_old : k.reads) + (uint64_t)h * kDReads;
        for (uint32_t r = 0; r < g.n_reads; ++r) rd[r] = rs[r];
        for (int l = 0; l < kLists; ++l) {
            cnt[l] = 0;           // pass B: the wave's base + the counts of the lanes before
            base[l] = WRITE ? k.scan[(uint64_t)l * k.nw + (idx >> 6)] - k.scan[(uint64_t)l * k.nw] +
                                  k.pre[(uint64_t)l * k.n + idx]
                            : 0;
        }
    }

    __device__ __forceinline__ uint32_t quorum() const { return g.n_voting / 2 + 1; }   // raft.go:372-374
    __device__ __forceinline__ int member_of(uint64_t id) const {
        int m = -1;
#pragma unroll
        for (int s = MC - 1; s >= 0; --s)           // the first match wins
            m = (s < (int)g.n_members && ids[s] == id) ? s : m;
        return m;
    }
    __device__ __forceinline__ uint64_t match_of(int mi) const {
        uint64_t v = 0;
#pragma unroll
        for (int s = 0; s < (int)MC; ++s) v = s == mi ? match[s] : v;
        return v;
    }
    __device__ __forceinline__ void set_match(int mi, uint64_t v) {
#pragma unroll
        for (int s = 0; s < (int)MC; ++s) match[s] = s == mi ? v : match[s];
    }
    __device__ __forceinline__ uint32_t slot(int l) { return base[l] + cnt[l]++; }
    template <class T>
    __device__ __forceinline__ T *list(int l) const {   // (uniform: scalar loads of the layout)
        return reinterpret_cast<T *>(a.out + a.layout->off[l]);
    }

    // -- outputs ----------------------------------------------------------------------------
    __device__ __forceinline__ void ready(uint64_t index, uint64_t low, uint64_t high) {
        if (WRITE && slotted) return;
        const uint32_t p = slot(kReady);
        const hq_ready_to_read r{g.cluster_id, index, low, high};
        const int64_t delta = (int64_t)(index - c0);
        if (!WRITE) {
            if (p == 0) a.ready_slot[i] = r;              // k_step_lite copies it out
            if (a.ready_wide && delta != (int64_t)(int32_t)delta) atomicOr(a.ready_wide, 1u);
        } else if (a.layout->ready_compact) {
            list<hq_ready_compact>(kReady)[p] =
                hq_ready_compact{low, high, (uint32_t)i, (int32_t)delta};
        } else if (stage && p - stage_lo < kStageReady) {
            stage[p - stage_lo] = r;
        } else {
            list<hq_ready_to_read>(kReady)[p] = r;
        }
    }
    __device__ __forceinline__ void resp(uint64_t to, uint64_t index, uint64_t hint, uint64_t high) {
        const uint32_t p = slot(kResps);
        if (WRITE)
            list<hq_read_index_resp>(kResps)[p] = hq_read_index_resp{g.cluster_id, to, index, hint, high};
    }
    __device__ __forceinline__ void state_change(uint32_t reason) {
        const uint32_t p = slot(kStates);
        if (WRITE) list<hq_state_change>(kStates)[p] = hq_state_change{g.cluster_id, g.term, g.state, reason};
    }
    __device__ __forceinline__ void dropped(uint64_t low, uint64_t high, uint64_t from, uint32_t reason) {
        const uint32_t p = slot(kDropped);
        if (WRITE)
            list<hq_dropped_read>(kDropped)[p] = hq_dropped_read{g.cluster_id, low, high, from, reason, 0};
    }
    __device__ __forceinline__ void defer(uint64_t e) {
        const uint32_t p = slot(kDeferred);
        if (WRITE) list<uint64_t>(kDeferred)[p] = e;
    }

    // -- reference state transitions (raft.go:949-1010) --------------------------------------
    __device__ __forceinline__ void reset(uint64_t term) {
        g.term = term;
        g.granted = g.rejected = 0;
        g.n_reads = 0;                                   // r.readIndex = newReadIndex()
#pragma unroll
        for (uint32_t s = 0; s < MC; ++s)         // resetRemotes/Observers/Witnesses
            match[s] = s < g.n_members && ids[s] == g.node_id ? g.last : 0;
        active = 0;
    }
    __device__ __forceinline__ void become_follower(uint64_t term, uint32_t reason) {
        g.state = HQ_STATE_FOLLOWER;
        reset(term);
        state_change(reason);
    }
    __device__ __forceinline__ void become_leader() {
        g.state = HQ_STATE_LEADER;
        reset(g.term);
        state_change(HQ_REASON_VOTE);
        // the no-op of p72: the first entry of the new term; the node's own remote follows it
        g.term_start = g.last + 1;
        g.last += 1;
        match[0] = g.last;
        if (g.n_voting == 1) try_commit();               // appendEntries: single-node tryCommit
    }

    // raft.tryCommit (raft.go:888-909): the quorum-th largest match of the voting members, then
    // entryLog.tryCommit (logentry.go:378-393) with term(q) == term <=> term_start <= q <= last
    // (the leader's entries carry its term and terms never decrease, entryutils.go:44-47)
    // The quorum-th largest by an 8-input sorting network (19 compare-exchanges; the slots past
    // n_voting enter as 0, below or tied with every voting match, so the q-th largest of the 8
    // is that of the n, q <= n) instead of counting, for every slot, the slots at or above it
    // (64 compares): the same value, a third of the instructions on every updating ack.
    __device__ __forceinline__ void try_commit() {
        static_assert(HQ_MAX_VOTERS == 8, "the network sorts 8 voting slots");
        cnt[kDecisions]++;
        const uint32_t n = g.n_voting, q = quorum();
        uint64_t v[8];
#pragma unroll
        for (uint32_t s = 0; s < 8; ++s) v[s] = s < n ? match[s] : 0;
        auto cx = [&](int i, int j) {                    // v[i] >= v[j] afterwards
            const uint64_t a = v[i], b = v[j];
            const bool gt = a > b;
            v[i] = gt ? a : b;
            v[j] = gt ? b : a;
        };
        cx(0, 2); cx(1, 3); cx(4, 6); cx(5, 7);
        cx(0, 4); cx(1, 5); cx(2, 6); cx(3, 7);
        cx(0, 1); cx(2, 3); cx(4, 5); cx(6, 7);
        cx(2, 4); cx(3, 5);
        cx(1, 4); cx(3, 6);
        cx(1, 2); cx(3, 4); cx(5, 6);
        uint64_t best = 0;
#pragma unroll
        for (uint32_t s = 0; s < 8; ++s) best = s + 1 == q ? v[s] : best;
        if (best > g.committed && best >= g.term_start && best <= g.last)
            g.committed = best;                          // commitTo (logentry.go:323-332)
    }

    // handleLeaderReadIndex (raft.go:1636-1669) and readIndex.addRequest (readindex.go:43-67);
    // returns false for the worker's fallback contract (see include/hipquorum.h)
    __device__ __forceinline__ bool read_index(uint64_t from, uint64_t low, uint64_t high, uint64_t e) {
        if (g.state != HQ_STATE_LEADER) {
            defer(e);                                    // forwarded / dropped (raft.go:1875, 1937)
            return true;
        }
        const int fm = member_of(from);
        const uint32_t role = fm >= 0 ? gm[fm].role : 0xFF;
        if (role == HQ_ROLE_WITNESS) {
            dropped(low, high, from, HQ_DROP_WITNESS);
            return true;
        }
        if (g.n_voting == 1) {                           // isSingleNodeQuorum
            ready(g.committed, low, high);
            if (from != g.node_id && role == HQ_ROLE_OBSERVER) resp(from, g.committed, low, high);
            return true;
        }
        // hasCommittedEntryAtCurrentTerm (raft.go:1612-1621)
        if (!(g.committed >= g.term_start && g.committed <= g.last)) {
            dropped(low, high, from, HQ_DROP_NOT_READY);
            return true;
        }
        for (uint32_t k = 0; k < g.n_reads; ++k)
            if (rd[k].low == low && rd[k].high == high) return true;   // already pending
        if (g.n_reads && g.committed < rd[g.n_reads - 1].index) return false;  // reference panics
        if (g.n_reads >= kDReads) return false;
        hq_dread &r = rd[g.n_reads++];
        r = hq_dread{};
        r.index = g.committed;
        r.from = from;
        r.low = low;
        r.high = high;
        return true;
    }

    // readIndex.confirm (readindex.go:77-116) + handleReadIndexLeaderConfirmation
    // (raft.go:1740-1760) for the ack of voting slot mi
    __device__ __forceinline__ bool confirm(uint64_t hint, uint64_t high, int mi) {
        uint32_t k = 0;
        while (k < g.n_reads && !(rd[k].low == hint && rd[k].high == high)) ++k;
        if (k == g.n_reads) return true;                 // not pending
        if (mi >= (int)g.n_voting) return false;         // an observer acking a ctx
        rd[k].confirmed |= (uint8_t)(1u << mi);          // p.confirmed[from] = struct{}{}
        cnt[kDecisions]++;
        if ((uint32_t)__popc(rd[k].confirmed) + 1 < quorum()) return true;
        const uint64_t index = rd[k].index;              // the rewrite of readindex.go:97-105
        for (uint32_t r = 0; r <= k; ++r) {
            if (rd[r].from == 0 || rd[r].from == g.node_id) ready(index, rd[r].low, rd[r].high);
            else resp(rd[r].from, index, hint, high);
        }
        for (uint32_t r = k + 1; r < g.n_reads; ++r) rd[r - k - 1] = rd[r];
        g.n_reads -= (uint8_t)(k + 1);
        return true;
    }

    // one event; false: the group leaves the device path at this event (fallback)
    __device__ __forceinline__ bool handle(const hq_event &ev, uint64_t e) {
        switch (ev.kind) {
        case HQ_EV_READ:
            return read_index(0, ev.hint, ev.hint_high, e);
        case HQ_EV_CHECK_QUORUM: {                       // raft.go:1582-1588, 380-390
            if (g.state != HQ_STATE_LEADER) return true;
            cnt[kDecisions]++;
            const uint32_t vm = (1u << g.n_voting) - 1u;
            const bool has = (uint32_t)__popc((active | 1u) & vm) >= quorum();
            active &= ~vm;                               // setNotActive (remote.go:196-198)
            if (!has) become_follower(g.term, HQ_REASON_CHECK_QUORUM);
            return true;
        }
        case HQ_EV_ELECTION:                             // raft.go:1485-1515, campaign 1082-1117
            if (g.state == HQ_STATE_LEADER) return true;
            g.state = HQ_STATE_CANDIDATE;
            reset(g.term + 1);
            state_change(HQ_REASON_CAMPAIGN);
            g.granted = 1;                               // the self vote
            cnt[kDecisions]++;
            if (g.n_voting == 1) become_leader();        // isSingleNodeQuorum
            return true;
        case HQ_EV_PROPOSE:                              // handleLeaderPropose -> appendEntries
            if (g.state != HQ_STATE_LEADER) {
                defer(e);                                // forwarded / dropped (raft.go:1845, 1932)
                return true;
            }
            g.last += ev.log_index;
            if (match[0] < g.last) match[0] = g.last;
            if (g.n_voting == 1) try_commit();
            return true;
        case HQ_EV_MESSAGE:
            break;
        default:
            return false;
        }
        const uint32_t type = ev.type;
        if (type != HQ_MSG_REPLICATE_RESP && type != HQ_MSG_HEARTBEAT_RESP &&
            type != HQ_MSG_REQUEST_VOTE_RESP && type != HQ_MSG_READ_INDEX)
            return false;
        const int mi = member_of(ev.from);
        if (mi < 0 && is_response(type)) return true;    // Peer.Handle drop (peer.go:191-197)
        if (ev.term != 0 && ev.term != g.term) {         // onMessageTermNotMatched
            if (ev.term < g.term) return true;
            become_follower(ev.term, HQ_REASON_HIGHER_TERM);
        }
        if (g.state == HQ_STATE_LEADER) {
            switch (type) {
            case HQ_MSG_REPLICATE_RESP:                  // handleLeaderReplicateResp
                if (!ev.reject && match_of(mi) < ev.log_index) {
                    if (ev.log_index > g.last) return false;   // a follower acks only what it got
                    set_match(mi, ev.log_index);         // remote.tryUpdate
                    try_commit();
                }
                active |= 1u << mi;
                return true;
            case HQ_MSG_HEARTBEAT_RESP:                  // handleLeaderHeartbeatResp
                if (ev.hint != 0 && !confirm(ev.hint, ev.hint_high, mi)) return false;
                active |= 1u << mi;
                return true;
            case HQ_MSG_READ_INDEX:
                return read_index(ev.from, ev.hint, ev.hint_high, e);
            default:
                return true;                             // RequestVoteResp: no leader handler
            }
        }
        if (g.state == HQ_STATE_CANDIDATE && type == HQ_MSG_REQUEST_VOTE_RESP) {
            if (mi >= (int)g.n_voting) return true;      // observer vote dropped (:1969-1972)
            const uint8_t bit = (uint8_t)(1u << mi);
            if (!((g.granted | g.rejected) & bit)) {     // first response wins (:1071-1073)
                if (ev.reject) g.rejected |= bit;
                else g.granted |= bit;
            }
            cnt[kDecisions]++;
            const uint32_t q = quorum();
            if ((uint32_t)__popc(g.granted) == q) become_leader();            // :1977-1980
            else if ((uint32_t)__popc(g.rejected) == q)                      // :1981-1984
                become_follower(g.term, HQ_REASON_VOTE);
            return true;
        }
        if (type == HQ_MSG_READ_INDEX) return read_index(ev.from, ev.hint, ev.hint_high, e);
        return true;                                     // no handler in this state
    }

    // the group's events: rows (STREAM = false) or its bytes [p, end) of the stream; an event
    // that does not decode is a fallback like one the path does not take
    // (2-byte size words, a.bytes_only: the events are the group's bytes decoded to their end —
    // e1 is not known and a suspended group's events are still decoded to be counted; bytes that
    // do not decode are an input error, as the host worker's decoder makes them, not a fallback)
    template <bool STREAM>
    __device__ __forceinline__ void run(uint64_t e0, uint64_t e1, const uint8_t *p, const uint8_t *end) {
        const uint64_t committed0 = c0 = g.committed;
        DPrev pv;
        ByteReader br{p, end};
        const bool by_bytes = STREAM && a.bytes_only;
        uint64_t e = e0;
        for (;; ++e) {
            if (by_bytes ? !(br.more() || pv.run) : e >= e1) break;
            hq_event ev;
            bool dec = true;
            if (STREAM && (by_bytes || !(g.flags & kDSuspended))) dec = decode_event(br, pv, ev);
            if (by_bytes && !dec) {
                if (!WRITE) atomicOr(a.error, (uint32_t)kErrBoffsets);
                break;
            }
            if (g.flags & kDSuspended) {
                defer(e);
                continue;
            }
            bool ok;
            if (STREAM) {
                ok = dec && handle(ev, e);
            } else {
                ev = a.events[e];
                ok = handle(ev, e);
            }
            if (!ok) {                                   // this event and the rest are deferred
                g.flags |= kDSuspended;
                const uint32_t p = slot(kFallback);
                if (WRITE) list<uint64_t>(kFallback)[p] = g.cluster_id;
                defer(e);
            } else if (STREAM && pv.run) {               // the run's other members at once
                e += take_run(pv, by_bytes ? ~0ull : e1 - e - 1);
            }
        }
        cnt[kEvents] = (uint32_t)(e - e0);
        // a group that took all its events must have used all its bytes: left-over bytes mean the
        // sizes were split wrongly between groups, which the host decoder rejects as HQ_E_INVAL
        // (hq_stream.cpp); pass A makes it an input error, so no state is written
        if (STREAM && !WRITE && !by_bytes && !(g.flags & kDSuspended) && (br.p != br.end || pv.run))
            atomicOr(a.error, (uint32_t)kErrBoffsets);
        if (!WRITE && g.committed - committed0 > 0xFFFFFFFFull && a.wide)
            atomicOr(a.wide, 1u);                        // no 4-byte advance column this step
        if (!WRITE && a.spec_col)                        // the advance column, ahead of the layout
            reinterpret_cast<uint32_t *>(a.out)[i] = (uint32_t)(g.committed - committed0);
        if (WRITE && a.layout->commit_column) {
            // every listed group's word: k_step_lite wrote it (from the saved and the new state)
        } else if (g.committed != committed0) {
            const uint32_t p = slot(kCommits);
            if (WRITE) list<hq_commit_event>(kCommits)[p] = hq_commit_event{g.cluster_id, g.committed};
        }
    }

    // The rest of a run whose members are consecutive node ids (the event just handled was its
    // first or an earlier member) taken at once where each member could only raise its match
    // (ReplicateResp) and mark its member active: a leader at the run's term, a ReplicateResp
    // run within the log (or rejecting) or a HeartbeatResp run without a ctx. Each member that
    // raises its match is a tryCommit decision; tryCommit runs once after the last: the quorum-th
    // largest match only rises as matches rise, so it ends where the member-by-member calls end
    // (and the run holds no event that reads the committed index). Returns the members taken;
    // otherwise (0) the loop takes them one at a time (also when the run claims more events than
    // the group has left, `room`: the loop then reports the bad sizes).
    __device__ __forceinline__ uint32_t take_run(DPrev &pv, uint64_t room) {
        const uint32_t kind = pv.last & 3;
        const bool rej = (pv.last >> 2) & 1;
        if (!(pv.last & 8u) || pv.run > room || g.state != HQ_STATE_LEADER || (g.flags & kDSuspended) ||
            (pv.term != 0 && pv.term != g.term) ||
            !(kind == 2 ? pv.hint == 0 : (rej || pv.index <= g.last)))
            return 0;
        const uint32_t m = pv.run;
        uint32_t upd = 0;
        for (uint32_t j = 0; j < m; ++j) {
            const int mi = member_of(pv.run_from + j);
            if (mi < 0) continue;                        // Peer.Handle drop (peer.go:191-197)
            if (kind == 1 && !rej && match_of(mi) < pv.index) {
                set_match(mi, pv.index);                 // remote.tryUpdate
                ++upd;
            }
            active |= 1u << mi;
        }
        pv.run_from += m;
        pv.run = 0;
        if (upd) {
            try_commit();
            cnt[kDecisions] += upd - 1;
        }
        return m;
    }

    // pass A, before the group's events: its state as the step found it
    __device__ __forceinline__ void save_old(uint32_t h) {
        hq_dgroup o = g;
        o.pad1 = active;
        a.groups_old[h] = o;
#pragma unroll
        for (uint32_t s = 0; s < MC; ++s)
            if (s < g.n_members) a.match_old[g.mem + s] = match[s];
        for (uint32_t r = 0; r < g.n_reads; ++r) a.reads_old[(uint64_t)h * kDReads + r] = rd[r];
    }

    __device__ __forceinline__ void store(uint32_t h) {
        a.groups[h] = g;
        hq_dmember *m = a.members + g.mem;
#pragma unroll
        for (uint32_t s = 0; s < MC; ++s) {
            if (s < g.n_members) {
                m[s].match = match[s];
                m[s].active = (uint8_t)((active >> s) & 1);
            }
        }
        for (uint32_t r = 0; r < g.n_reads; ++r) a.reads[(uint64_t)h * kDReads + r] = rd[r];
    }
};

// Pass A over a stream, the advance column speculated (StepK::spec_ready): the ReadyToRead records
// of the tile's groups that pass B does not replay (one record, kept in ready_slot), written at
// their final places in the host region during pass A — their PCIe writes then overlap the step's
// input reads instead of following pass A as k_step_lite's. A record's place is the count of
// records of the groups before it in input order: the tile's first place comes from a chained
// scan over the launch's tiles in start order (a tile publishes its count, looks back over its
// predecessors' words until an inclusive one, publishes its own inclusive prefix); the launch's
// first tile takes the inclusive prefix an earlier launch of the step left in the tile of the
// group before its first (0 for group 0). The records are staged in LDS at their places (the
// holes, the places of groups pass B replays, are written by pass B afterwards) and stored as
// one contiguous run of 16-byte stores. All threads of the workgroup call this.
__device__ void ready_tail(const StepK &a, uint64_t tile, uint32_t chunk, bool member, bool first,
                          uint64_t i, uint32_t cnt, bool one, uint4 *sbuf) {
    __shared__ uint32_t s_w[256 / 64], s_excl, s_any, s_first, s_ok;
    __shared__ unsigned long long s_first_i;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) {
        s_any = 0;
        s_first = 0;
    }
    uint32_t x = cnt;             // inclusive scan over the wave's lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        x += lane >= d ? y : 0u;
    }
    if (lane == 63) s_w[wv] = x;
    __syncthreads();              // (also: every thread is done with the staged bytes in sbuf)
    if (member) s_any = 1;
    if (first) {                  // (one group of the launch is its first)
        s_first = 1;
        s_first_i = i;
    }
    uint32_t before = 0, agg = 0;
#pragma unroll
    for (int w = 0; w < 256 / 64; ++w) {
        before += w < wv ? s_w[w] : 0u;
        agg += s_w[w];
    }
    __syncthreads();
    if (!s_any) return;           // no group of this launch: no tile waits for this one
    if (wv == 0) {                // the first wave looks back, 64 tiles per round trip
        const uint32_t step = a.step_no;
        uint32_t excl = 0;
        bool ok = true;
        if (s_first) {
            if (s_first_i > 0) {  // written by an earlier launch of this step
                const uint64_t w = tile_load(a.tiles + (s_first_i - 1) / 256);
                ok = (uint32_t)(w >> 32) == step && ((w >> 28) & 1) &&
                     (uint32_t)((w >> 29) & 7) < chunk;
                excl = (uint32_t)w & kTileVal;
            }
        } else if (tile == 0 || a.test_scan_fail) {
            ok = false;
        } else {
            if (lane == 0) tile_store(a.tiles + tile, tile_word(step, chunk, false, agg));
            // lane k reads tile hi - k; a window is taken once every tile up to the nearest
            // inclusive word (or all 64) has published for this launch
            int64_t hi = (int64_t)tile - 1;
            const uint64_t t_wait = wall_clock64();
            for (;;) {
                const int64_t p = hi - lane;
                const uint64_t w = p >= 0 ? tile_load(a.tiles + p) : 0;
                const bool ready = p >= 0 && (uint32_t)(w >> 32) == step &&
                                   (uint32_t)((w >> 29) & 7) == (chunk & 7);
                const uint64_t rdy = __ballot(ready), inc = __ballot(ready && ((w >> 28) & 1));
                const uint64_t need = inc ? (inc & (0 - inc)) * 2 - 1 : ~0ull;   // lanes 0 .. k
                if ((rdy & need) == need) {
                    uint32_t v = (lane < 64 - __clzll((long long)need) || !inc) && ready
                                     ? (uint32_t)w & kTileVal : 0u;
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
                    excl += v;
                    if (inc) break;
                    hi -= 64;
                    if (hi < 0) {     // no inclusive word before: cannot be
                        ok = false;
                        break;
                    }
                    continue;
                }
                if (wall_clock64() - t_wait > kScanWaitTicks) {
                    ok = false;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        if (lane == 0) {
            if (!ok) atomicOr(a.error, (uint32_t)kErrScan);
            tile_store(a.tiles + tile, tile_word(step, chunk, true, excl + agg));
            s_excl = excl;
            s_ok = ok;
        }
    }
    __syncthreads();
    const uint32_t lo = s_excl;
    // (a region too small: the layout reports the overflow and the regrown step's k_step_lite
    // writes every record)
    if (!s_ok || agg == 0 || a.ready_off + (uint64_t)(lo + agg) * sizeof(hq_ready_to_read) > a.out_cap)
        return;
    constexpr uint32_t kCap = kStageBytes / sizeof(hq_ready_to_read);
    hq_ready_to_read *stage = reinterpret_cast<hq_ready_to_read *>(sbuf);
    hq_ready_to_read *dst = reinterpret_cast<hq_ready_to_read *>(a.out + a.ready_off) + lo;
    const uint32_t pos = before + x - cnt;   // the tile's records before this group's
    if (one) {
        const hq_ready_to_read r = a.ready_slot[i];
        if (pos < kCap) stage[pos] = r;
        else dst[pos] = r;
    }
    __syncthreads();
    const uint32_t nq = 2 * min(agg, kCap);
    const uint4 *src = reinterpret_cast<const uint4 *>(stage);
    uint4 *out = reinterpret_cast<uint4 *>(dst);
    for (uint32_t q = threadIdx.x; q < nq; q += 256) out[q] = src[q];
}

// HQ_WORKER_READY_SLOTS: tile `tile`'s slotted records (one per slotted thread, the thread's
// group = the tile's 256-group block in order) staged in LDS in group order and stored as one
// contiguous run of 16-byte stores at the tile's slot, the count beside it. No place depends on
// another tile, so pass A writes them while it still reads the stream (the link's other
// direction). buf: >= kSlotTileBytes of LDS no thread still reads. All threads of the workgroup
// call this.
__device__ void slot_store(const StepK &a, uint64_t tile, bool slotted, const hq_ready_compact &rec,
                           uint4 *buf) {
    __shared__ uint32_t s_w[256 / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t bal = __ballot(slotted);
    if (lane == 0) s_w[wv] = (uint32_t)__popcll(bal);
    __syncthreads();              // (also: every thread is done with what buf held)
    uint32_t before = 0, agg = 0;
#pragma unroll
    for (int w = 0; w < 256 / 64; ++w) {
        before += w < wv ? s_w[w] : 0u;
        agg += s_w[w];
    }
    hq_ready_compact *stage = reinterpret_cast<hq_ready_compact *>(buf);
    if (slotted) stage[before + __popcll(bal & ((1ull << lane) - 1))] = rec;
    __syncthreads();
    char *dst = a.out + a.slot_off + tile * kSlotTileBytes;
    const uint32_t nbytes = agg * (uint32_t)sizeof(hq_ready_compact);
    for (uint32_t q = threadIdx.x; q < nbytes / 16; q += 256)
        reinterpret_cast<uint4 *>(dst)[q] = buf[q];
    if (threadIdx.x == 0) {
        if (nbytes & 8)           // (an odd record count: the last 8 bytes)
            reinterpret_cast<uint2 *>(dst)[nbytes / 8 - 1] =
                reinterpret_cast<const uint2 *>(buf)[nbytes / 8 - 1];
        reinterpret_cast<uint32_t *>(a.out + a.cnt_off)[tile] = agg;
    }
}

template <bool WRITE, bool STREAM, int MC>
__device__ __forceinline__ void step_groups(const StepK &a, uint64_t blk, uint32_t chunk = 0) {
    // pass A: the wave's counts summed in LDS, added to wsum by one lane (i_begin is a multiple
    // of 64: the wave's groups are one wave of the scan)
    __shared__ uint32_t wtot[WRITE ? 1 : 256 / 64][kLists];
    if (!WRITE && (threadIdx.x & 63) < kLists) wtot[threadIdx.x >> 6][threadIdx.x & 63] = 0;
    uint64_t i = a.i_begin + blk * 256 + threadIdx.x;
    // pass A over a stream stages the workgroup's bytes in LDS first (below): every thread takes
    // part in that, so until then a thread with no group to step clears `act` instead of leaving
    constexpr bool STAGE = !WRITE && STREAM;
    bool act = true;
    if (WRITE && (a.layout->error | a.layout->overflow)) return;   // nothing written this time
    if (WRITE && a.layout->commit_column) {
        // the commits are a column (k_step_lite wrote it from pass A's state): pass B takes
        // only the groups with other records, packed at the front of the grid
        if (i >= a.layout->len[kRerun]) return;
        i = a.rerun_list[i];
    } else if (i >= a.i_end) {
        if (!STAGE) return;
        act = false;
    }
    uint64_t e0 = 0, e1 = 0, b0 = 0, b1 = 0;
    if (act && STREAM && a.prefix) {
        const uint64_t x0 = a.prefix[i], x1 = a.prefix[i + 1];
        e0 = x0 >> 32;
        e1 = x1 >> 32;
        b0 = x0 & 0xFFFFFFFFu;
        b1 = x1 & 0xFFFFFFFFu;
        if (!WRITE) {
            // the sizes' totals must be the ones the copies were sized by (checked once)
            // (2-byte words carry no events: the layout checks the events pass A counted)
            if (i + 1 == a.n && a.own_lo == 0 &&
                ((!a.bytes_only && e1 != a.n_events) || b1 != a.n_bytes))
                atomicOr(a.error, (uint32_t)kErrBoffsets);
            if (b1 < a.own_lo || b1 >= a.own_hi) act = false;   // another chunk's group
        }
    } else if (act) {
        e0 = a.offsets[i];
        e1 = a.offsets[i + 1];
        if (STREAM) {
            b0 = a.boffsets[i];
            b1 = a.boffsets[i + 1];
        }
    }
    if (!STAGE && !act) return;
    // (pass A over a stream: a group of this launch, input errors or not, and the launch's first)
    const bool member = act;
    const bool first = member && (a.prefix ? i == 0 || b0 < a.own_lo : i == a.i_begin);
    const uint32_t h = !act ? 0u : a.handles ? a.handles[i] : (uint32_t)i;   // NULL: 0 .. n - 1
    if (!WRITE && act) {          // validate this group's entry; a bad one is not stepped
        uint32_t err = 0;
        if (h >= a.n_handles) err |= kErrHandle;
        if (e1 < e0 || (!STREAM && e1 > a.n_events) || (STREAM && a.prefix && e1 > a.n_events))
            err |= kErrOffsets;
        if (STREAM && (b1 < b0 || b1 > a.n_bytes)) err |= kErrBoffsets;
        if (!(err & kErrHandle) && atomicExch(a.stamp + h, a.step_no) == a.step_no)
            err |= kErrTwice;
        if (err) {
            atomicOr(a.error, err);
            for (int l = 0; l < kLists; ++l) a.counts[(uint64_t)l * a.n + i] = 0;
            a.rerun[i] = 0;       // not stepped: nothing to restore
            act = false;
        }
    }
    // Pass A reads each group's bytes once, a thread per group: the workgroup's groups' bytes
    // are one contiguous range, loaded into LDS by all its threads in coalesced 16-byte loads
    // (a zero-copy stream in pinned host memory read lane by lane in 8-byte words crossed the
    // link at 41 GB/s), each thread then decoding its own from LDS; a range larger than the
    // buffer is read in place. The aligned 16-byte blocks around the range never leave the
    // pages of its bytes.
    const uint8_t *src0 = a.bytes + b0;
    __shared__ uint4 sbuf[STAGE ? kStageBytes / 16 : 1];
    if constexpr (STAGE) {
        __shared__ unsigned long long s_lo, s_hi;
        if (threadIdx.x == 0) {
            s_lo = ~0ull;
            s_hi = 0;
        }
        __syncthreads();
        const uint64_t base = reinterpret_cast<uint64_t>(a.bytes);
        if (act && b1 > b0) {
            atomicMin(&s_lo, (unsigned long long)(base + b0));
            atomicMax(&s_hi, (unsigned long long)(base + b1));
        }
        __syncthreads();
        const uint64_t lo = s_lo & ~15ull, hi = (s_hi + 15) & ~15ull;
        const bool fits = s_hi > s_lo && hi - lo <= kStageBytes;
        if (fits) {               // every load issued before the first LDS store: one round
            constexpr int kU = kStageBytes / (256 * 16);   // trip over the link, not kU
            uint4 v[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const uint64_t o = (threadIdx.x + 256ull * u) * 16;
                if (o < hi - lo) v[u] = *reinterpret_cast<const uint4 *>(lo + o);
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const uint64_t o = (threadIdx.x + 256ull * u) * 16;
                if (o < hi - lo) sbuf[o / 16] = v[u];
            }
        }
        __syncthreads();
        if (act && fits) src0 = reinterpret_cast<const uint8_t *>(sbuf) + (base + b0 - lo);
    }
    uint32_t n_ready = 0;
    bool one_ready = false, slotted = false;
    hq_ready_compact srec{};
    if (act) {
        hq_dread reads[kDReads];
        Engine<WRITE, MC> eng(a, i, h, reads);   // (pass B: i_begin = 0, i / 64 is its wave)
        if (!WRITE) eng.save_old(h);
        if (WRITE && STREAM && a.bytes_only) e0 = eng.base[kEvents];   // (the events' scan)
        if (WRITE && a.slots) eng.slotted = (a.rerun[i] & 8) != 0;
        __shared__ hq_ready_to_read stage[WRITE ? 256 / 64 : 1][WRITE ? kStageReady : 1];
        // list mode: the wave's groups are consecutive and so are their records, staged from its
        // first active lane's on; column mode: the groups replayed are a sparse subset whose records
        // lie between k_step_lite's, so each is stored where it goes
        const bool staged = WRITE && !a.layout->commit_column && !a.layout->ready_compact;
        if (staged) {
            eng.stage = stage[threadIdx.x >> 6];
            eng.stage_lo = __builtin_amdgcn_readfirstlane(eng.base[kReady]);
        }
        if (STREAM)
            eng.template run<true>(e0, e1, src0, src0 + (b1 - b0));
        else
            eng.template run<false>(e0, e1, nullptr, nullptr);
        if (staged) {                 // the staged records out, 16 contiguous bytes per lane
            const uint64_t act = __ballot(1);
            const int last = 63 - __clzll((long long)act);
            const uint32_t end = __shfl(eng.base[kReady] + eng.cnt[kReady], last);
            const uint32_t nrec = min(end - eng.stage_lo, kStageReady);
            const uint32_t rank = __popcll(act & ((1ull << (threadIdx.x & 63)) - 1));
            const uint32_t nact = __popcll(act);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's LDS stores landed
            __builtin_amdgcn_wave_barrier();
            const uint4 *src = reinterpret_cast<const uint4 *>(eng.stage);
            uint4 *dst = reinterpret_cast<uint4 *>(eng.template list<hq_ready_to_read>(kReady) +
                                                   eng.stage_lo);
            for (uint32_t q = rank; q < 2 * nrec; q += nact) dst[q] = src[q];
        }
        if (!WRITE) {                 // the new state in place (pass B replays from the saved one)
            const bool others = (eng.cnt[kResps] | eng.cnt[kStates] | eng.cnt[kDropped] |
                                 eng.cnt[kDeferred] | eng.cnt[kFallback]) != 0;
            const bool rerun = others || eng.cnt[kReady] > 1;
            one_ready = !rerun && eng.cnt[kReady] == 1;
            if (a.slots && one_ready) {   // the record goes to the tile's slot, out of the list
                const hq_ready_to_read r = a.ready_slot[i];
                const int64_t delta = (int64_t)(r.index - eng.c0);
                if (delta == (int64_t)(int32_t)delta) {
                    slotted = true;
                    one_ready = false;
                    srec = hq_ready_compact{r.ctx_low, r.ctx_high, (uint32_t)i, (int32_t)delta};
                    eng.cnt[kReady] = 0;
                    eng.cnt[kSlotted] = 1;
                }
            }
            n_ready = eng.cnt[kReady];
            eng.cnt[kRerun] = rerun;
            for (int l = 0; l < kLists; ++l) a.counts[(uint64_t)l * a.n + i] = eng.cnt[l];
            a.rerun[i] = (uint8_t)(2 | rerun | (one_ready ? 4 : 0) | (slotted ? 8 : 0));
            eng.store(h);
            uint32_t *wt = wtot[threadIdx.x >> 6];   // (the lanes that left early add nothing)
            for (int l = 0; l < kLists; ++l)
                if (eng.cnt[l]) atomicAdd(wt + l, eng.cnt[l]);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            if ((int)(threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1) {
                for (int l = 0; l < kLists; ++l) {
                    const uint32_t v = wt[l];
                    if (v) atomicAdd(a.wsum + (uint64_t)l * a.nw + (i >> 6), v);
                }
            }
        }
    }
    if constexpr (STAGE) {
        if (a.spec_ready)
            ready_tail(a, (a.i_begin >> 8) + blk, chunk, member, first, i, n_ready, one_ready, sbuf);
        else if (a.slots)
            slot_store(a, (a.i_begin >> 8) + blk, slotted, srec, sbuf);
    }
}

template <bool WRITE, bool STREAM, int MC>
__global__ __launch_bounds__(256) void k_step(const StepK a) {
    if constexpr (!WRITE && STREAM) {   // tiles in start order (ready_tail's chained scan)
        const uint32_t b = draw_ticket(a.tickets + a.chunk);
        if (b >= gridDim.x) {     // tickets not zeroed: report, step nothing
            if (threadIdx.x == 0) atomicOr(a.error, (uint32_t)kErrTicket);
            return;
        }
        step_groups<WRITE, STREAM, MC>(a, b, a.chunk);
    } else {
        step_groups<WRITE, STREAM, MC>(a, blockIdx.x);
    }
}

template <bool WRITE, bool STREAM, int MC>
__global__ __launch_bounds__(256) void k_step_jobs(const JobMap m) {
    uint32_t b = blockIdx.x;
    if constexpr (!WRITE && STREAM) {
        b = draw_ticket(m.tickets + m.chunk);
        if (b >= gridDim.x) {
            if (threadIdx.x == 0) atomicOr(m.ks[m.job0].error, (uint32_t)kErrTicket);
            return;
        }
    }
    const uint32_t j = job_of(m, b);
    step_groups<WRITE, STREAM, MC>(m.ks[m.job0 + j], b - m.blk0[j], m.chunk);
}

// Between the layout and pass B: with the commits as a column, every listed group's word from
// the committed index pass A saved and the one it wrote (the advance, or the new index), and the
// positions of the groups with other records packed in order for pass B; in list mode nothing
__device__ __forceinline__ void lite_groups(const StepK &a, uint64_t blk, uint32_t *tickets) {
    const uint64_t i = blk * 256 + threadIdx.x;
    if (tickets && threadIdx.x < kTickets) tickets[threadIdx.x] = 0;   // (pass A's are done)
    if (i < a.ws) a.wsum[i] = 0;  // (scanned already; the grid covers ws: 11 n / 64 + 12 <= max(n, 256))
    __shared__ __align__(16) hq_ready_to_read stage[256 / 64][kStageReady];
    static_assert(sizeof(stage) >= kSlotTileBytes, "the slot staging fits the list's");
    if (a.slots && !a.spec_valid && !(a.layout->error | a.layout->overflow)) {
        // the output region grew after pass A wrote the slots into the old one: this tile's
        // slots again, from the records pass A kept (whole workgroup; the tiles are pass A's)
        const bool s = i < a.n && (a.rerun[i] & 8);
        hq_ready_compact rec{};
        if (s) {
            const hq_ready_to_read r = a.ready_slot[i];
            const uint32_t h = a.handles ? a.handles[i] : (uint32_t)i;
            rec = hq_ready_compact{r.ctx_low, r.ctx_high, (uint32_t)i,
                                   (int32_t)(int64_t)(r.index - a.groups_old[h].committed)};
        }
        slot_store(a, blk, s, rec, reinterpret_cast<uint4 *>(&stage[0][0]));
        __syncthreads();          // (stage is the list's staging below)
    }
    const bool in = i < a.n;
    if ((a.layout->error | a.layout->overflow) || !__ballot(in)) return;   // (whole waves)
    const uint32_t col = a.layout->commit_column;
    const uint8_t rr = in ? a.rerun[i] : 0;
    const int lane = threadIdx.x & 63;
    // the counts of the lanes before in the wave (pass A's counts, scanned across the wave):
    // stored for the groups pass B replays (with the column: those with other records; in list
    // mode: all), kReady's and kRerun's kept for below; a wave with no replayed group scans those two
    const bool replay = in && (!col || (rr & 1));
    const bool any = __ballot(replay) != 0;
    uint32_t pre_ready = 0, pre_rerun = 0;
    for (int l = 0; l < kLists; ++l) {
        if (!any && l != kReady && l != kRerun) continue;
        const uint32_t c = in ? a.counts[(uint64_t)l * a.n + i] : 0;
        uint32_t x = c;           // inclusive scan over the wave's lanes
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d, 64);
            x += lane >= d ? y : 0u;
        }
        if (replay) a.pre[(uint64_t)l * a.n + i] = x - c;
        if (l == kReady) pre_ready = x - c;
        if (l == kRerun) pre_rerun = x - c;
    }
    if (!col) return;
    const bool col32 = col == kColumn32;
    // the single ReadyToReads pass A kept: the wave's records are consecutive in the list (its
    // groups are), staged in LDS at their places and stored as one contiguous run of 16-byte
    // lane stores; the places of the replayed groups' records are holes pass B fills afterwards
    // (stage: declared above)
    if (!(col32 && a.spec_valid && a.spec_ready)) {   // (else pass A wrote them: ready_tail)
        constexpr uint64_t l = kReady;
        const uint64_t w = i >> 6;
        const uint32_t lo = a.scan[l * a.nw + w] - a.scan[l * a.nw];
        const uint32_t cnt = a.scan[l * a.nw + w + 1] - a.scan[l * a.nw + w];   // the wave's
        hq_ready_to_read *st = stage[threadIdx.x >> 6];
        const uint32_t pos = lo + pre_ready;
        const uint32_t nrec = min(cnt, kStageReady);
        if (a.layout->ready_compact) {
            // 24-byte records (the group's position and index - its committed index before the
            // step, which pass A saved), stored as 8-byte lane words
            hq_ready_compact *stc = reinterpret_cast<hq_ready_compact *>(st);
            hq_ready_compact *dst = reinterpret_cast<hq_ready_compact *>(a.out + a.layout->off[kReady]);
            if (rr & 4) {
                const hq_ready_to_read r = a.ready_slot[i];
                const uint32_t h = a.handles ? a.handles[i] : (uint32_t)i;
                const hq_ready_compact c{r.ctx_low, r.ctx_high, (uint32_t)i,
                                         (int32_t)(int64_t)(r.index - a.groups_old[h].committed)};
                if (pos - lo < kStageReady) stc[pos - lo] = c;
                else dst[pos] = c;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            const uint2 *src = reinterpret_cast<const uint2 *>(stc);
            uint2 *out = reinterpret_cast<uint2 *>(dst + lo);
            for (uint32_t q = lane; q < 3 * nrec; q += 64) out[q] = src[q];
        } else {
            hq_ready_to_read *dst = reinterpret_cast<hq_ready_to_read *>(a.out + a.layout->off[kReady]);
            if (rr & 4) {
                if (pos - lo < kStageReady) st[pos - lo] = a.ready_slot[i];
                else dst[pos] = a.ready_slot[i];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            const uint4 *src = reinterpret_cast<const uint4 *>(st);
            uint4 *out = reinterpret_cast<uint4 *>(dst + lo);
            for (uint32_t q = lane; q < 2 * nrec; q += 64) out[q] = src[q];
        }
    }
    if (!in) return;
    if (!(col32 && a.spec_valid)) {   // (pass A wrote the advance words)
        const uint32_t h = a.handles ? a.handles[i] : (uint32_t)i;
        const uint64_t c0 = a.groups_old[h].committed, c1 = a.groups[h].committed;
        char *cw = a.out + a.layout->off[kCommits];
        if (col32)
            reinterpret_cast<uint32_t *>(cw)[i] = (uint32_t)(c1 - c0);
        else
            reinterpret_cast<uint64_t *>(cw)[i] = c1 != c0 ? c1 : 0;
    }
    if (rr & 1) {                 // the wave's base + the lanes before
        const uint64_t l = kRerun;
        a.rerun_list[a.scan[l * a.nw + (i >> 6)] - a.scan[l * a.nw] + pre_rerun] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(256) void k_step_lite(const StepK a) {
    lite_groups(a, blockIdx.x, blockIdx.x == 0 ? a.tickets : nullptr);
}

__global__ __launch_bounds__(256) void k_step_lite_jobs(const JobMap m) {
    const uint32_t j = job_of(m, blockIdx.x);
    lite_groups(m.ks[m.job0 + j], blockIdx.x - m.blk0[j], blockIdx.x == 0 ? m.tickets : nullptr);
}

// A step with an input error writes no group state: the groups pass A stepped get back the
// state it saved (the host launches this only when k_layout reported an error)
__global__ __launch_bounds__(256) void k_step_restore(const StepK a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n || !(a.rerun[i] & 2)) return;
    const uint32_t h = a.handles ? a.handles[i] : (uint32_t)i;
    hq_dgroup g = a.groups_old[h];
    const uint32_t act = g.pad1;
    g.pad1 = 0;
    a.groups[h] = g;
    for (uint32_t s = 0; s < g.n_members; ++s) {
        a.members[g.mem + s].match = a.match_old[g.mem + s];
        a.members[g.mem + s].active = (uint8_t)((act >> s) & 1);
    }
    for (uint32_t r = 0; r < g.n_reads; ++r)
        a.reads[(uint64_t)h * kDReads + r] = a.reads_old[(uint64_t)h * kDReads + r];
}

}  // namespace

namespace hq {

int launch_step(hq_ctx *ctx, bool write, bool stream, bool small, const StepArgs &ka) {
    const StepK &k = static_cast<const StepK &>(ka);
    const dim3 grid((unsigned)((k.i_end - k.i_begin + 255) / 256)), blk(256);
    int rc = pre_launch(ctx);
    if (rc) return rc;
    dispatch_bool(write, [&](auto w) {
        dispatch_bool(stream, [&](auto st) {
            dispatch<8, kDMembers>(small ? 8u : kDMembers, [&](auto mc) {
                hipLaunchKernelGGL((k_step<decltype(w)::value, decltype(st)::value,
                                           (int)decltype(mc)::value>),
                                   grid, blk, 0, ctx->stream, k);
            });
        });
    });
    return post_launch(ctx, write ? "k_step<write>" : "k_step<count>");
}

int launch_step_jobs(hq_ctx *ctx, bool write, bool small, const JobArgs &ma) {
    const JobMap &m = static_cast<const JobMap &>(ma);
    int rc = pre_launch(ctx);
    if (rc) return rc;
    dispatch_bool(write, [&](auto w) {       // (the jobs are streams: STREAM = true only)
        dispatch<8, kDMembers>(small ? 8u : kDMembers, [&](auto mc) {
            hipLaunchKernelGGL((k_step_jobs<decltype(w)::value, true, (int)decltype(mc)::value>),
                               dim3(m.blk0[m.count]), dim3(256), 0, ctx->stream, m);
        });
    });
    return post_launch(ctx, write ? "k_step_jobs<write>" : "k_step_jobs<count>");
}

int launch_step_lite(hq_ctx *ctx, hipStream_t s, const StepArgs &ka) {
    const StepK &k = static_cast<const StepK &>(ka);
    return launch(ctx, s, "k_step_lite", k_step_lite, (k.n + 255) / 256, 256, k);
}
int launch_step_lite_jobs(hq_ctx *ctx, hipStream_t s, const JobArgs &ma) {
    const JobMap &m = static_cast<const JobMap &>(ma);
    return launch(ctx, s, "k_step_lite_jobs", k_step_lite_jobs, m.blk0[m.count], 256, m);
}
int launch_step_restore(hq_ctx *ctx, hipStream_t s, const StepArgs &ka) {
    const StepK &k = static_cast<const StepK &>(ka);
    return launch(ctx, s, "k_step_restore", k_step_restore, (k.n + 255) / 256, 256, k);
}

}  // namespace hq
