// hq_worker_host.cpp — the host worker's step (hq_worker_k.h), whole and in one translation unit:
// its functions call each other per event.
//
// Host work per event is the reference's bookkeeping only — Peer.Handle's membership filter
// (peer.go:186-198), onMessageTermNotMatched (raft.go:1416-1452), remote.tryUpdate
// (remote.go:123-133), the ReadIndex confirmed-set insert (readindex.go:83) and the first-wins
// vote insert (raft.go:1071-1073). Every quorum decision is a kernel launch through the C-ABI:
// tryCommit (hq_commit_dev, term-start form), the ReadIndex release with its index rewrite
// (hq_readindex_multi_dev), the vote outcome (hq_vote_dev) and leaderHasQuorum
// (hq_check_quorum_dev). A group's events are taken in order until one needs a decision not
// yet taken (a "run"); all runs of a pass are decided in one GPU batch, applied, and the next
// pass continues where they stopped.
#include "hq_worker_k.h"

using namespace hq::wk;

namespace {

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

bool is_response_type(uint32_t t) {       // isResponseMessageType (internal/raft/utils.go)
    return t == HQ_MSG_REPLICATE_RESP || t == HQ_MSG_REQUEST_VOTE_RESP ||
           t == HQ_MSG_HEARTBEAT_RESP || t == 20 /* ReadIndexResp */ ||
           t == 8 /* SnapshotStatus */ || t == 9 /* Unreachable */;
}

}  // namespace

// (hq_worker::reset, raft.reset: hq_worker_k.h)
void hq_worker::become_follower(Group &g, uint64_t term, uint32_t reason) {
    g.state = HQ_STATE_FOLLOWER;                    // raft.go:949-957
    reset(g, term);
    push_state(g, reason);
}

void hq_worker::become_leader(Group &g) {
    g.state = HQ_STATE_LEADER;                      // raft.go:977-989
    reset(g, g.term);
    push_state(g, HQ_REASON_VOTE);
    // the no-op of p72: first entry of the new term; the node's own remote follows the log
    g.term_start = g.last + 1;
    g.last += 1;
    members(g)[0].match = g.last;
    if (g.n_voting == 1) g.set(kCommitDue);         // appendEntries: single-node tryCommit
}

// ------------------------------------------------------------------------------ events -----
Verdict hq_worker::read_index(Group &g, uint64_t from, uint64_t low, uint64_t high,
                              uint64_t ei) {
    if (g.state != HQ_STATE_LEADER) {
        if (g.has(kVoteDue)) return BARRIER;        // the vote may have made it leader
        defer(ei);                                  // forwarded / dropped (raft.go:1875, 1937)
        return CONSUMED;
    }
    // handleLeaderReadIndex (raft.go:1636-1669)
    const int fm = member_of(g, from);
    const uint8_t role = fm >= 0 ? members(g)[fm].role : 0xFF;
    if (role == HQ_ROLE_WITNESS) {
        dropped.push_back({g.cluster_id, low, high, from, HQ_DROP_WITNESS, 0});
        return CONSUMED;
    }
    if (g.has(kCommitDue)) return BARRIER;          // needs the committed index
    if (g.n_voting == 1) {                          // isSingleNodeQuorum: quorum() == 1
        ready.push_back({g.cluster_id, g.committed, low, high});
        if (from != g.node_id && role == HQ_ROLE_OBSERVER)
            resps.push_back({g.cluster_id, from, g.committed, low, high});
        return CONSUMED;
    }
    // hasCommittedEntryAtCurrentTerm (raft.go:1612-1621): term(committed) == r.term
    if (!(g.committed >= g.term_start && g.committed <= g.last)) {
        dropped.push_back({g.cluster_id, low, high, from, HQ_DROP_NOT_READY, 0});
        return CONSUMED;
    }
    // readIndex.addRequest (readindex.go:43-67)
    ReadQueue *q = reads(g);
    if (q) {
        for (uint32_t i = 0; i < q->n; ++i)
            if (q->r[i].low == low && q->r[i].high == high)
                return g.has(kRiDue) ? BARRIER : CONSUMED;   // already pending (or released)
        if (q->n && g.committed < q->r[q->n - 1].index) return FALLBACK;  // reference panics
        if (q->n >= kMaxReads) return g.has(kRiDue) ? BARRIER : FALLBACK;
    } else {
        g.rq = rq_alloc();
        q = &rqs[g.rq];
    }
    ReadStatus &s = q->r[q->n++];
    s.index = g.committed;
    s.from = from;
    s.low = low;
    s.high = high;
    s.confirmed = 0;
    std::fill(std::begin(s.ord), std::end(s.ord), kNoAck);
    return CONSUMED;
}

Verdict hq_worker::handle(Group &g, const hq_event &e, uint64_t ei) {
    switch (e.kind) {
    case HQ_EV_READ:
        return read_index(g, 0, e.hint, e.hint_high, ei);
    case HQ_EV_CHECK_QUORUM:
        if (g.state != HQ_STATE_LEADER) return g.has(kVoteDue) ? BARRIER : CONSUMED;
        if (g.has(kCqDue)) return BARRIER;
        g.set(kCqDue);
        return CONSUMED;
    case HQ_EV_ELECTION:
        if (g.pending()) return BARRIER;
        if (g.state == HQ_STATE_LEADER) return CONSUMED;   // leader ignores Election
        // campaign: becomeCandidate + the self vote (raft.go:959-975, 1082-1095)
        g.state = HQ_STATE_CANDIDATE;
        reset(g, g.term + 1);
        push_state(g, HQ_REASON_CAMPAIGN);
        g.granted = 1;
        g.set(kVoteDue);                            // isSingleNodeQuorum -> the vote kernel
        return CONSUMED;
    case HQ_EV_PROPOSE:
        if (g.pending() && (g.state != HQ_STATE_LEADER || g.has(kCqDue))) return BARRIER;
        if (g.state != HQ_STATE_LEADER) {
            defer(ei);                              // forwarded / dropped (raft.go:1845, 1932)
            return CONSUMED;
        }
        // appendEntries (raft.go:911-922)
        g.last += e.log_index;
        if (members(g)[0].match < g.last) members(g)[0].match = g.last;
        if (g.n_voting == 1) g.set(kCommitDue);
        return CONSUMED;
    case HQ_EV_MESSAGE:
        break;
    default:
        return FALLBACK;
    }
    const uint32_t type = e.type;
    if (type != HQ_MSG_REPLICATE_RESP && type != HQ_MSG_HEARTBEAT_RESP &&
        type != HQ_MSG_REQUEST_VOTE_RESP && type != HQ_MSG_READ_INDEX)
        return FALLBACK;
    const int mi = member_of(g, e.from);
    if (mi < 0 && is_response_type(type)) return CONSUMED;      // Peer.Handle drop
    if (e.term != 0 && e.term != g.term) {                      // onMessageTermNotMatched
        if (e.term < g.term) return CONSUMED;
        if (g.pending()) return BARRIER;            // decisions of the run come first
        become_follower(g, e.term, HQ_REASON_HIGHER_TERM);
    }
    if (g.state == HQ_STATE_LEADER) {
        switch (type) {
        case HQ_MSG_REPLICATE_RESP: {               // handleLeaderReplicateResp (:1671-1700)
            Member &rp = members(g)[mi];
            if (!e.reject && rp.match < e.log_index) {
                if (e.log_index > g.last) return FALLBACK;  // a follower can only ack what it got
                rp.match = e.log_index;             // remote.tryUpdate
                g.set(kCommitDue);                  // -> tryCommit
            }
            rp.active = 1;
            return CONSUMED;
        }
        case HQ_MSG_HEARTBEAT_RESP: {               // handleLeaderHeartbeatResp (:1702-1714)
            ReadQueue *q = e.hint != 0 ? reads(g) : nullptr;
            if (q) {                                // handleReadIndexLeaderConfirmation
                for (uint32_t i = 0; i < q->n; ++i) {
                    ReadStatus &r = q->r[i];
                    if (r.low != e.hint || r.high != e.hint_high) continue;
                    if (mi >= g.n_voting) return FALLBACK;   // an observer acking a ctx
                    if (g.ord >= kMaxOrdinal) return BARRIER;
                    if (!((r.confirmed >> mi) & 1) && r.ord[mi] == kNoAck) {
                        r.ord[mi] = ++g.ord;        // p.confirmed[from] = struct{}{}
                        g.set(kRiDue);
                    }
                    break;
                }
            }
            members(g)[mi].active = 1;
            return CONSUMED;
        }
        case HQ_MSG_READ_INDEX:
            return read_index(g, e.from, e.hint, e.hint_high, ei);
        default:
            return CONSUMED;                        // RequestVoteResp: no leader handler
        }
    }
    if (g.state == HQ_STATE_CANDIDATE) {
        if (type == HQ_MSG_REQUEST_VOTE_RESP) {     // handleCandidateRequestVoteResp
            if (mi >= g.n_voting) return CONSUMED;  // observer vote dropped (:1969-1972)
            if (!(((g.granted | g.rejected) >> mi) & 1)) {   // first response wins
                if (e.reject) g.rejected |= (uint8_t)(1u << mi);
                else g.granted |= (uint8_t)(1u << mi);
            }
            g.set(kVoteDue);
            return CONSUMED;
        }
        if (g.has(kVoteDue)) return BARRIER;        // may be leader by now
    }
    if (type == HQ_MSG_READ_INDEX) return read_index(g, e.from, e.hint, e.hint_high, ei);
    return CONSUMED;                                // no handler in this state
}

void hq_worker::advance(Group &g) {
    while (g.cursor < g.ev_end) {
        const uint64_t ei = g.cursor;
        if (g.has(kSuspended)) {
            defer(ei);
            ++g.cursor;
            continue;
        }
        const Verdict v = handle(g, in->events[ei], ei);
        if (v == BARRIER) return;
        if (v == FALLBACK) {
            g.set(kSuspended);
            fallback.push_back(g.cluster_id);
            continue;                               // this event and the rest are deferred
        }
        ++g.cursor;
    }
}

// ------------------------------------------------------------------------------ GPU pass ---
int hq_worker::reserve(size_t bytes) {
    if (bytes <= cap) return HQ_OK;
    size_t want = std::max(bytes, cap * 2);
    want = std::max<size_t>(want, 1 << 20);
    if (host) hq_free_pinned(ctx, host);
    if (dev) hq_free_dev(ctx, dev);
    host = dev = nullptr;
    cap = 0;
    int rc = hq(hq_alloc_pinned(ctx, want, &host), "hq_alloc_pinned");
    if (!rc) rc = hq(hq_malloc_dev(ctx, want, &dev), "hq_malloc_dev");
    if (rc) return rc;
    cap = want;
    return HQ_OK;
}

namespace {
// Carves one staging region into aligned arrays; host and device share the offsets.
struct Layout {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off = align_up(off + std::max<size_t>(bytes, 1), 256);
        return o;
    }
};
}  // namespace

int hq_worker::run_pass() {
    const uint64_t Gc = l_commit.size(), Gr = l_ri.size(), Gv = l_vote.size(), Gq = l_cq.size();
    const uint32_t N = n_max;
    uint32_t K = 1;
    for (uint32_t gi : l_ri) K = std::max<uint32_t>(K, rqs[groups[gi].rq].n);
    const uint64_t sc = align_up(std::max<uint64_t>(Gc, 1), 2);   // even stride: 16-B loads
    // inputs
    Layout L;
    const size_t c_match = L.take(8 * N * sc), c_nv = L.take(Gc), c_cin = L.take(8 * Gc),
                 c_last = L.take(8 * Gc), c_ts = L.take(8 * Gc);
    const size_t r_ord = L.take(2 * (size_t)K * N * Gr), r_idx = L.take(8 * (size_t)K * Gr),
                 r_np = L.take(Gr), r_nv = L.take(Gr);
    const size_t v_gr = L.take(Gv), v_rj = L.take(Gv), v_nv = L.take(Gv);
    const size_t q_act = L.take(Gq), q_nv = L.take(Gq);
    const size_t in_bytes = L.off;
    // outputs
    const size_t c_out = L.take(8 * Gc), c_chg = L.take(8 * ((Gc + 63) / 64)),
                 c_fb = L.take(8 * ((Gc + 63) / 64));
    // (the released indexes are not read back: the compact release, each released entry's index
    // taken from its closing ctx below)
    const size_t r_cnt = L.take(Gr), r_be = L.take(Gr), r_fb = L.take(8 * ((Gr + 63) / 64));
    const size_t v_out = L.take(8 * ((Gv + 31) / 32)), v_fb = L.take(8 * ((Gv + 63) / 64));
    const size_t q_hq = L.take(8 * ((Gq + 63) / 64)), q_fb = L.take(8 * ((Gq + 63) / 64));
    const size_t total = L.off;
    int rc = reserve(total);
    if (rc) return rc;
    auto H = [&](size_t o) { return static_cast<uint8_t *>(host) + o; };
    auto D = [&](size_t o) { return static_cast<uint8_t *>(dev) + o; };

    // pack (the SoA layout of DESIGN.md §2): voting slot s of a group is pool entry s
    const uint64_t t0 = now_ns();
    {
        uint64_t *match = reinterpret_cast<uint64_t *>(H(c_match));
        uint8_t *nv = H(c_nv);
        uint64_t *cin = reinterpret_cast<uint64_t *>(H(c_cin));
        uint64_t *last = reinterpret_cast<uint64_t *>(H(c_last));
        uint64_t *ts = reinterpret_cast<uint64_t *>(H(c_ts));
        for (uint64_t j = 0; j < Gc; ++j) {
            const Group &g = groups[l_commit[j]];
            const Member *m = pool.data() + g.mem;
            uint32_t s = 0;
            for (; s < g.n_voting; ++s) match[s * sc + j] = m[s].match;
            for (; s < N; ++s) match[s * sc + j] = 0;
            nv[j] = g.n_voting;
            cin[j] = g.committed;
            last[j] = g.last;
            ts[j] = g.term_start;
        }
        uint16_t *ord = reinterpret_cast<uint16_t *>(H(r_ord));
        uint64_t *idx = reinterpret_cast<uint64_t *>(H(r_idx));
        uint8_t *np = H(r_np), *rnv = H(r_nv);
        for (uint64_t j = 0; j < Gr; ++j) {
            const Group &g = groups[l_ri[j]];
            const ReadQueue &q = rqs[g.rq];
            np[j] = (uint8_t)q.n;
            rnv[j] = g.n_voting;
            for (uint32_t k = 0; k < K; ++k) {
                const ReadStatus *r = k < q.n ? &q.r[k] : nullptr;
                idx[(uint64_t)k * Gr + j] = r ? r->index : 0;
                for (uint32_t s = 0; s < N; ++s)
                    ord[((uint64_t)k * N + s) * Gr + j] =
                        !r ? kNoAck : ((r->confirmed >> s) & 1) ? 0 : r->ord[s];
            }
        }
        uint8_t *gr = H(v_gr), *rj = H(v_rj), *vnv = H(v_nv);
        for (uint64_t j = 0; j < Gv; ++j) {
            const Group &g = groups[l_vote[j]];
            gr[j] = g.granted;
            rj[j] = g.rejected;
            vnv[j] = g.n_voting;
        }
        uint8_t *act = H(q_act), *qnv = H(q_nv);
        for (uint64_t j = 0; j < Gq; ++j) {
            const Group &g = groups[l_cq[j]];
            const Member *m = pool.data() + g.mem;
            uint8_t a = 0;
            for (uint32_t s = 0; s < g.n_voting; ++s) a |= (uint8_t)(m[s].active << s);
            act[j] = a;
            qnv[j] = g.n_voting;
        }
    }

    // one H2D, the decisions, one D2H, one sync
    const uint64_t t1 = now_ns();
    t_pack += t1 - t0;
    rc = hq(hq_memcpy_async(ctx, dev, host, in_bytes, 0), "hq_memcpy_async(H2D)");
    if (!rc && Gc) {
        hq_commit_args a{};
        a.G = Gc;
        a.n_max = N;
        a.form = HQ_FORM_TERM_START;
        a.match_stride = sc;
        a.match = reinterpret_cast<const uint64_t *>(D(c_match));
        a.n_voting = D(c_nv);
        a.committed_in = reinterpret_cast<const uint64_t *>(D(c_cin));
        a.committed_out = reinterpret_cast<uint64_t *>(D(c_out));
        a.last_index = reinterpret_cast<const uint64_t *>(D(c_last));
        a.term_start = reinterpret_cast<const uint64_t *>(D(c_ts));
        a.changed = reinterpret_cast<uint64_t *>(D(c_chg));
        a.fallback = reinterpret_cast<uint64_t *>(D(c_fb));
        rc = hq(hq_commit_dev(ctx, &a), "hq_commit_dev");
    }
    if (!rc && Gr)
        rc = hq(hq_readindex_multi_dev(ctx, Gr, K, N, reinterpret_cast<const uint16_t *>(D(r_ord)),
                                       reinterpret_cast<const uint64_t *>(D(r_idx)), D(r_np),
                                       D(r_nv), 0, nullptr, D(r_cnt), D(r_be),
                                       reinterpret_cast<uint64_t *>(D(r_fb))),
                "hq_readindex_multi_dev");
    if (!rc && Gv)
        rc = hq(hq_vote_dev(ctx, Gv, D(v_gr), D(v_rj), D(v_nv), 0,
                            reinterpret_cast<uint64_t *>(D(v_out)),
                            reinterpret_cast<uint64_t *>(D(v_fb))),
                "hq_vote_dev");
    if (!rc && Gq)
        rc = hq(hq_check_quorum_dev(ctx, Gq, D(q_act), D(q_nv), 0, 0,
                                    reinterpret_cast<uint64_t *>(D(q_hq)),
                                    reinterpret_cast<uint64_t *>(D(q_fb))),
                "hq_check_quorum_dev");
    if (!rc) rc = hq(hq_memcpy_async(ctx, H(in_bytes), D(in_bytes), total - in_bytes, 1),
                     "hq_memcpy_async(D2H)");
    if (!rc) rc = hq(hq_sync(ctx), "hq_sync");
    if (rc) return rc;
    decisions += Gc + Gr + Gv + Gq;
    const uint64_t t2 = now_ns();
    t_device += t2 - t1;

    // every group handed to a kernel satisfies its contract; a fallback bit is an internal error
    auto any = [&](size_t o, uint64_t G) {
        const uint64_t *w = reinterpret_cast<const uint64_t *>(H(o));
        for (uint64_t i = 0; i < (G + 63) / 64; ++i)
            if (w[i]) return true;
        return false;
    };
    if (any(c_fb, Gc) || any(r_fb, Gr) || any(v_fb, Gv) || any(q_fb, Gq))
        return fail(HQ_E_STATE, "a kernel refused a packed group (worker contract bug)");

    // apply, per group in the reference's order: commit, ReadIndex release, vote, CheckQuorum
    const uint64_t *cout = reinterpret_cast<const uint64_t *>(H(c_out));
    for (uint64_t j = 0; j < Gc; ++j) {
        Group &g = groups[l_commit[j]];
        g.committed = cout[j];                      // commitTo (logentry.go:323-332)
        g.clear(kCommitDue);
    }
    const uint8_t *cnt = H(r_cnt), *be = H(r_be);
    for (uint64_t j = 0; j < Gr; ++j) {
        Group &g = groups[l_ri[j]];
        ReadQueue &q = rqs[g.rq];
        const uint32_t c = cnt[j];
        for (uint32_t i = 0; i < c; ++i) {
            uint32_t k = i;                         // the ctx whose confirm() released entry i
            while (k < c && !((be[j] >> k) & 1)) ++k;
            if (k >= c) return fail(HQ_E_STATE, "ReadIndex release without a closing ctx");
            const ReadStatus &s = q.r[i];
            // confirm() rewrites every released entry's index to the closing ctx's
            // (readindex.go:96-104): what the kernel's released_index column would hold
            const uint64_t index = q.r[k].index;
            if (s.from == 0 || s.from == g.node_id)
                ready.push_back({g.cluster_id, index, s.low, s.high});
            else
                resps.push_back({g.cluster_id, s.from, index, q.r[k].low, q.r[k].high});
        }
        std::copy(q.r + c, q.r + q.n, q.r);         // r.queue = r.queue[done:]
        q.n -= c;
        for (uint32_t i = 0; i < q.n; ++i) {        // carry the run's confirmations over
            ReadStatus &r = q.r[i];
            for (uint32_t s = 0; s < HQ_MAX_VOTERS; ++s) {
                if (r.ord[s] != kNoAck) r.confirmed |= (uint8_t)(1u << s);
                r.ord[s] = kNoAck;
            }
        }
        if (q.n == 0) rq_release(g);
        g.ord = 0;
        g.clear(kRiDue);
    }
    const uint64_t *outc = reinterpret_cast<const uint64_t *>(H(v_out));
    for (uint64_t j = 0; j < Gv; ++j) {
        Group &g = groups[l_vote[j]];
        g.clear(kVoteDue);
        const uint32_t o = (uint32_t)((outc[j >> 5] >> (2 * (j & 31))) & 3);
        if (o == HQ_OUTCOME_LEADER) become_leader(g);
        else if (o == HQ_OUTCOME_FOLLOWER) become_follower(g, g.term, HQ_REASON_VOTE);
    }
    const uint64_t *hqb = reinterpret_cast<const uint64_t *>(H(q_hq));
    for (uint64_t j = 0; j < Gq; ++j) {
        Group &g = groups[l_cq[j]];
        g.clear(kCqDue);
        Member *m = members(g);
        for (uint32_t s = 0; s < g.n_voting; ++s) m[s].active = 0;   // setNotActive
        if (!((hqb[j >> 6] >> (j & 63)) & 1)) become_follower(g, g.term, HQ_REASON_CHECK_QUORUM);
    }
    t_apply += now_ns() - t2;
    return HQ_OK;
}

// ------------------------------------------------------------------------------ step -------
// (an exception on the way leaves no group marked: the worker stays usable, hq_guard.h)
int hq_worker::step(const hq_step_input *inp, hq_step_output *out) {
    try {
        return step_body(inp, out);
    } catch (...) {
        unmark_touched();
        throw;
    }
}

int hq_worker::step_body(const hq_step_input *inp, hq_step_output *out) {
    const uint64_t t0 = now_ns();
    uint64_t t_pass = 0;
    in = inp;
    commits.clear();
    ready.clear();
    resps.clear();
    states.clear();
    dropped.clear();
    deferred.clear();
    fallback.clear();
    decisions = 0;
    t_pack = t_device = t_apply = 0;
    uint64_t passes = 0;

    // the groups with events, each with its slice of the event array (node.mq per node)
    work.clear();
    touched.clear();
    int rc = HQ_OK;
    for (uint64_t i = 0; i < in->n_groups; ++i) {
        const uint32_t gi = in->groups[i];
        const uint64_t b = in->offsets[i], e = in->offsets[i + 1];
        if (gi >= groups.size()) { rc = fail(HQ_E_INVAL, "hq_worker_step: unknown group handle"); break; }
        if (e < b) { rc = fail(HQ_E_INVAL, "hq_worker_step: offsets decrease"); break; }
        Group &g = groups[gi];
        if (g.has(kTouched)) { rc = fail(HQ_E_INVAL, "hq_worker_step: a group is listed twice"); break; }
        touched.push_back(gi);
        g.set(kTouched);
        g.committed0 = g.committed;
        if (b == e) continue;
        g.cursor = b;
        g.ev_end = e;
        g.set(kInWork);
        work.push_back(gi);
    }

    while (!rc && !work.empty()) {
        l_commit.clear();
        l_ri.clear();
        l_vote.clear();
        l_cq.clear();
        for (uint32_t gi : work) {
            Group &g = groups[gi];
            g.clear(kInWork);
            advance(g);
            if (g.has(kCommitDue)) l_commit.push_back(gi);
            if (g.has(kRiDue)) l_ri.push_back(gi);
            if (g.has(kVoteDue)) l_vote.push_back(gi);
            if (g.has(kCqDue)) l_cq.push_back(gi);
        }
        if (l_commit.empty() && l_ri.empty() && l_vote.empty() && l_cq.empty()) break;
        const uint64_t tp = now_ns();
        rc = run_pass();
        t_pass += now_ns() - tp;
        if (rc) break;
        ++passes;
        next_work.clear();
        for (const auto *l : {&l_commit, &l_ri, &l_vote, &l_cq})
            for (uint32_t gi : *l) {
                Group &g = groups[gi];
                if (g.has(kInWork)) continue;
                if (g.cursor < g.ev_end || g.pending()) {
                    g.set(kInWork);
                    next_work.push_back(gi);
                }
            }
        work.swap(next_work);
    }
    for (uint32_t gi : touched) {
        Group &g = groups[gi];
        g.clear(kTouched | kInWork);
        if (g.committed != g.committed0) commits.push_back({g.cluster_id, g.committed});
    }
    if (rc) return rc;

    out->commits = commits.data();
    out->n_commits = commits.size();
    out->ready = ready.data();
    out->n_ready = ready.size();
    out->read_resps = resps.data();
    out->n_read_resps = resps.size();
    out->state_changes = states.data();
    out->n_state_changes = states.size();
    out->dropped_reads = dropped.data();
    out->n_dropped_reads = dropped.size();
    out->deferred = deferred.data();
    out->n_deferred = deferred.size();
    out->fallback_groups = fallback.data();
    out->n_fallback_groups = fallback.size();
    out->gpu_passes = passes;
    out->decisions = decisions;
    out->pass_ns = t_pass;
    out->pack_ns = t_pack;
    out->device_ns = t_device;
    out->apply_ns = t_apply;
    out->handle_ns = now_ns() - t0 - t_pass;
    return HQ_OK;
}
