// hq_config.hip — membership changes applied to a device worker's resident state
// (hq_worker_config_changes, include/hipquorum.h "membership changes"): addNode / addObserver /
// addWitness / removeNode (raft.go:1136-1199) as an edit of a group's member records where the
// step keeps them, with removeNode's tryCommit (raft.go:1194-1198) taken on the spot.
//
// One kernel on the context's stream behind the last step, one lane per change. The host has
// validated the list and turned each change into a descriptor from its mirror's structure (member
// ids, roles and positions are the host's own even while the mirror's values are stale); the lane
// reads the group's record, decides SUSPENDED / FALLBACK from what only the device holds (flags,
// votes, the pending reads' confirmed sets), moves the 24-byte member records, remaps the slot
// bitmaps (hq_config.h), takes the commit decision and writes a status word and the new committed
// index to pinned host columns. The groups of a call are distinct: no races, no atomics but the
// error word's atomicOr, no spinning, no LDS. Every loop is bounded by kDMembers / kDReads and
// every record index is checked against the state's sizes before it is used.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hq_config.h"
#include "hq_sidecar.h"

namespace {

constexpr int kBlock = 256;

struct CfgK {
    hq_dgroup *groups;
    hq_dread *reads;
    hq_dmember *members;
    uint64_t n_state_groups, n_state_members;
    const hq_cfg_desc *desc;       // device [n]
    uint64_t n;
    uint32_t *status;              // pinned host [n]
    uint64_t *committed;           // pinned host [n]
    uint32_t *error;               // device
};

struct Rec {                       // a member record as three words: node_id, match,
    uint64_t id, match, tail;      // role | active << 8 | order << 16
};

__device__ __forceinline__ Rec load_rec(const hq_dmember *m) {
    const uint64_t *p = reinterpret_cast<const uint64_t *>(m);
    return Rec{p[0], p[1], p[2]};
}
__device__ __forceinline__ void store_rec(hq_dmember *m, const Rec &r) {
    uint64_t *p = reinterpret_cast<uint64_t *>(m);
    p[0] = r.id;
    p[1] = r.match;
    p[2] = r.tail;
}

// The group record's fields the edit reads and writes, in registers: words 3-7 of the 64-byte
// record (committed, last, term_start; mem, n_members, n_voting, state, granted; rejected, flags,
// n_reads and the padding, kept as it is). Words, not the struct: a struct copy with byte fields
// is an alloca the compiler parks in LDS.
struct Grp {
    uint64_t committed, last, term_start, tail_keep;
    uint32_t mem, n_members, n_voting, state, granted, rejected, flags, n_reads;
};

__device__ __forceinline__ Grp load_grp(const hq_dgroup *g) {
    const uint64_t *p = reinterpret_cast<const uint64_t *>(g);
    const uint64_t a = p[6], b = p[7];
    Grp r;
    r.committed = p[3];
    r.last = p[4];
    r.term_start = p[5];
    r.mem = (uint32_t)a;
    r.n_members = (uint32_t)(a >> 32) & 0xFFu;
    r.n_voting = (uint32_t)(a >> 40) & 0xFFu;
    r.state = (uint32_t)(a >> 48) & 0xFFu;
    r.granted = (uint32_t)(a >> 56) & 0xFFu;
    r.rejected = (uint32_t)b & 0xFFu;
    r.flags = (uint32_t)(b >> 8) & 0xFFu;
    r.n_reads = (uint32_t)(b >> 16) & 0xFFu;
    r.tail_keep = b & ~uint64_t(0xFFFFFF);
    return r;
}
__device__ __forceinline__ void store_grp(hq_dgroup *g, const Grp &r) {
    uint64_t *p = reinterpret_cast<uint64_t *>(g);
    p[3] = r.committed;
    p[6] = (uint64_t)r.mem | (uint64_t)r.n_members << 32 | (uint64_t)r.n_voting << 40 |
           (uint64_t)r.state << 48 | (uint64_t)r.granted << 56;
    p[7] = (uint64_t)r.rejected | (uint64_t)r.flags << 8 | (uint64_t)r.n_reads << 16 | r.tail_keep;
}

struct Dsc {                       // a descriptor's fields (hq_cfg_desc, three words)
    uint64_t node_id;
    uint32_t group, new_mem, kind, src, dst, slot, role, order, n_members, n_voting;
};
__device__ __forceinline__ Dsc load_desc(const hq_cfg_desc *d) {
    const uint64_t *p = reinterpret_cast<const uint64_t *>(d);
    const uint64_t a = p[1], b = p[2];
    return Dsc{p[0], (uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b & 0xFFu, (uint32_t)(b >> 8) & 0xFFu,
               (uint32_t)(b >> 16) & 0xFFu, (uint32_t)(b >> 24) & 0xFFu, (uint32_t)(b >> 32) & 0xFFu,
               (uint32_t)(b >> 40) & 0xFFu, (uint32_t)(b >> 48) & 0xFFu, (uint32_t)(b >> 56) & 0xFFu};
}

// raft.tryCommit (raft.go:888-909) + entryLog.tryCommit (logentry.go:378-393) as the step's pass A
// takes it: the quorum-th largest voting match by the same 8-input network, committed iff
// q > committed && term_start <= q <= last. Returns the new committed index, or 0.
__device__ __forceinline__ uint64_t try_commit(const Grp &g, const hq_dmember *m) {
    static_assert(HQ_MAX_VOTERS == 8, "the network sorts 8 voting slots");
    const uint32_t n = g.n_voting, q = n / 2 + 1;
    uint64_t v[8];
#pragma unroll
    for (uint32_t s = 0; s < 8; ++s) v[s] = s < n ? reinterpret_cast<const uint64_t *>(m + s)[1] : 0;
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
    return best > g.committed && best >= g.term_start && best <= g.last ? best : 0;
}

__global__ void __launch_bounds__(kBlock) k_cfg_apply(CfgK k) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= k.n) return;
    const Dsc d = load_desc(k.desc + i);
    // what the lane is told, checked before anything is indexed with it
    if (d.group >= k.n_state_groups) {
        atomicOr(k.error, kCfgErrHandle);
        k.status[i] = HQ_CC_SUSPENDED;
        k.committed[i] = 0;
        return;
    }
    Grp g = load_grp(k.groups + d.group);
    const uint32_t n = g.n_members, nv = g.n_voting;
    bool ok = d.kind <= kCfgFallback && n >= 1 && n <= kDMembers && nv >= 1 && nv <= n &&
              nv <= HQ_MAX_VOTERS && g.n_reads <= kDReads && n == d.n_members && nv == d.n_voting &&
              (uint64_t)g.mem + n <= k.n_state_members;
    if (d.kind == kCfgRemove)
        ok = ok && d.src >= 1 && d.src < n && d.order < n && (d.slot == kCfgNoSlot ? d.src >= nv : d.slot == d.src && d.src < nv);
    if (d.kind == kCfgInsert)
        ok = ok && n < kDMembers && d.dst >= 1 && d.dst <= n && d.order == n &&
             (d.slot == kCfgNoSlot ? d.dst == n : d.slot == d.dst && d.dst <= nv && nv < HQ_MAX_VOTERS) &&
             (d.new_mem == kCfgNoMove
                  ? (uint64_t)g.mem + n + 1 <= k.n_state_members
                  : ((uint64_t)d.new_mem + n + 1 <= k.n_state_members &&
               ((uint64_t)d.new_mem >= (uint64_t)g.mem + n || (uint64_t)d.new_mem + n + 1 <= g.mem)));
    if (d.kind == kCfgPromote)
        ok = ok && d.src >= nv && d.src < n && d.dst >= 1 && d.dst <= nv && d.slot == d.dst &&
             nv < HQ_MAX_VOTERS;
    if (!ok) {
        atomicOr(k.error, kCfgErrState);
        k.status[i] = HQ_CC_SUSPENDED;
        k.committed[i] = 0;
        return;
    }
    uint32_t status = HQ_CC_NOOP;
    uint64_t commit = 0;
    hq_dread *rd = k.reads + (uint64_t)d.group * kDReads;
    hq_dmember *m = k.members + g.mem;
    if (g.flags & kDSuspended) {
        status = HQ_CC_SUSPENDED;
    } else if (d.kind == kCfgFallback) {
        status = HQ_CC_FALLBACK;
    } else if (d.kind == kCfgRemove && d.slot != kCfgNoSlot) {
        // a recorded vote or ReadIndex acknowledgement of the leaving voter: the reference keeps
        // it by node id and goes on counting it, a slot bitmap cannot
        uint32_t bits = g.granted | g.rejected;
        for (uint32_t r = 0; r < kDReads; ++r)
            if (r < g.n_reads) bits |= rd[r].confirmed;
        if ((bits >> d.slot) & 1) status = HQ_CC_FALLBACK;
    }
    if (status == HQ_CC_FALLBACK) {
        g.flags |= kDSuspended;
        store_grp(k.groups + d.group, g);
    } else if (status != HQ_CC_SUSPENDED && d.kind != kCfgNoop) {
        if (d.kind == kCfgRemove) {
            // the records behind src move down, ascending; the list positions close the gap
            for (uint32_t j = 0; j < kDMembers; ++j) {
                if (j + 1 >= n) break;
                Rec r = load_rec(m + (j < d.src ? j : j + 1));
                const uint32_t o = (uint32_t)(r.tail >> 16) & 0xFFu;
                r.tail = (r.tail & ~uint64_t(0xFF0000)) | (uint64_t)cfg_order_after_remove(o, d.order) << 16;
                store_rec(m + j, r);
            }
            g.n_members = (n - 1);
            if (d.slot != kCfgNoSlot) g.n_voting = (nv - 1);
            status = HQ_CC_APPLIED;
        } else if (d.kind == kCfgInsert) {
            const Rec fresh{d.node_id, 0, (uint64_t)d.role | (uint64_t)d.order << 16};
            if (d.new_mem != kCfgNoMove) {
                // the range is full: the group moves to the pool's end, the new record in its place
                hq_dmember *nm = k.members + d.new_mem;
                for (uint32_t j = 0; j < kDMembers; ++j) {
                    if (j >= n) break;
                    store_rec(nm + cfg_pos_after_insert(j, d.dst), load_rec(m + j));
                }
                store_rec(nm + d.dst, fresh);
                g.mem = d.new_mem;
                m = nm;
            } else {
                // in place: the records from dst on move up, descending
                for (uint32_t t = 0; t < kDMembers; ++t) {
                    if (t >= n - d.dst) break;
                    const uint32_t j = n - 1 - t;
                    store_rec(m + j + 1, load_rec(m + j));
                }
                store_rec(m + d.dst, fresh);
            }
            g.n_members = (n + 1);
            if (d.slot != kCfgNoSlot) g.n_voting = (nv + 1);
            status = HQ_CC_APPLIED;
        } else if (d.kind == kCfgPromote) {
            // the observer's record, carried past the records between dst and src (descending),
            // lands behind the remotes as a remote with its match and active flag
            Rec carry = load_rec(m + d.src);
            for (uint32_t t = 0; t < kDMembers; ++t) {
                if (t >= (uint32_t)d.src - d.dst) break;
                const uint32_t j = d.src - 1 - t;
                store_rec(m + j + 1, load_rec(m + j));
            }
            carry.tail = (carry.tail & ~uint64_t(0xFF)) | HQ_ROLE_REMOTE;
            store_rec(m + d.dst, carry);
            g.n_voting = (nv + 1);
            status = HQ_CC_APPLIED;
        }
        // the slot bitmaps follow the voting slots
        if (status == HQ_CC_APPLIED && d.slot != kCfgNoSlot) {
            const bool rm = d.kind == kCfgRemove;
            g.granted = 0xFFu & (rm ? cfg_remove_bit(g.granted, d.slot) : cfg_insert_bit(g.granted, d.slot));
            g.rejected = 0xFFu & (rm ? cfg_remove_bit(g.rejected, d.slot) : cfg_insert_bit(g.rejected, d.slot));
            for (uint32_t r = 0; r < kDReads; ++r) {
                if (r >= g.n_reads) break;
                const uint32_t c = rd[r].confirmed;
                rd[r].confirmed = (uint8_t)(rm ? cfg_remove_bit(c, d.slot) : cfg_insert_bit(c, d.slot));
            }
        }
        // removeNode's tryCommit (raft.go:1194-1198), a non-member's removal included
        if ((d.kind == kCfgRemove || d.kind == kCfgCommitOnly) && g.state == HQ_STATE_LEADER) {
            commit = try_commit(g, m);
            if (commit) g.committed = commit;        // commitTo (logentry.go:323-332)
        }
        if (status == HQ_CC_APPLIED || commit) store_grp(k.groups + d.group, g);
    }
    k.status[i] = status;
    k.committed[i] = commit;
}

}  // namespace

struct hq_cfg_dev : hq::Sidecar {      // (totals: the error word as the host reads it)
    hq::DevBuf<hq_cfg_desc> desc;      // device
    hq::PinBuf<hq_cfg_desc> desc_host; // pinned staging of the descriptors
    hq::PinBuf<uint32_t> status;       // pinned host columns
    hq::PinBuf<uint64_t> committed;
};

int hq_cfg_dev_open(hq_ctx *ctx, hq_cfg_dev **out) { return hq::sidecar_open(ctx, out, "hq_config error word"); }

void hq_cfg_dev_close(hq_cfg_dev *c) { hq::sidecar_close(c); }

int hq_cfg_dev_run(hq_cfg_dev *c, const hq_dstate_mut *st, uint64_t n_member_records, uint64_t n,
                   const hq_cfg_desc *desc, const uint32_t **status, const uint64_t **committed,
                   uint64_t *gpu_ns, uint32_t *error) {
    hq_ctx *ctx = c->ctx;
    hipStream_t s = ctx->stream;
    *error = 0;
    *gpu_ns = 0;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc) rc = c->desc.grow(ctx, n, "hq_config descriptors");
    if (!rc) rc = c->desc_host.grow(ctx, n, "hq_config descriptors");
    if (!rc) rc = c->status.grow(ctx, n, "hq_config status");
    if (!rc) rc = c->committed.grow(ctx, n, "hq_config commits");
    if (rc) return rc;
    std::copy(desc, desc + n, c->desc_host.get());

    CfgK k{};
    k.groups = st->groups;
    k.reads = st->reads;
    k.members = st->members;
    k.n_state_groups = st->n_groups;
    k.n_state_members = n_member_records;
    k.desc = c->desc;
    k.n = n;
    k.status = c->status;
    k.committed = c->committed;
    k.error = c->error();

    // (from here on every return is finish's: the staging is rewritten by the next call)
    rc = hq::check_hip(ctx, hipEventRecord(c->ev0, s), "event");
    if (!rc) rc = hq::check_hip(ctx, hipMemsetAsync(c->error(), 0, 16, s), "memset");
    if (!rc)
        rc = hq::check_hip(ctx, hipMemcpyAsync(c->desc, c->desc_host, n * sizeof(hq_cfg_desc),
                                               hipMemcpyHostToDevice, s), "hq_config descriptors");
    if (!rc) {
        const uint32_t grid = (uint32_t)((n + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(k_cfg_apply, dim3(grid), dim3(kBlock), 0, s, k);
        rc = hq::check_hip(ctx, hipGetLastError(), "k_cfg_apply");
    }
    if (!rc)
        rc = hq::check_hip(ctx, hipMemcpyAsync(c->totals, c->error(), 4, hipMemcpyDeviceToHost, s),
                           "hq_config error word");
    if (!rc) rc = hq::check_hip(ctx, hipEventRecord(c->ev1, s), "event");
    rc = hq::finish(ctx, rc, "hq_worker_config_changes");
    if (rc) return rc;
    if ((uint32_t)c->totals[0]) {
        *error = (uint32_t)c->totals[0];
        return HQ_E_INVAL;
    }
    *status = c->status;
    *committed = c->committed;
    *gpu_ns = hq::elapsed_ns(c->ev0, c->ev1);
    return HQ_OK;
}
