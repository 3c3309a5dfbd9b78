// hq_worker.cpp — the step worker's group store (hq_worker_k.h): what a group must satisfy, how
// it is loaded into the flat records, and the C entries that open and close a worker and add,
// find, read and replace single groups.
#include <new>

#include "hq_worker_k.h"

using namespace hq::wk;

// ------------------------------------------------------------------------------ state ------
// What a group must satisfy to be loaded (nothing is changed); the node's place in the list and
// the voting members' count on the way.
int hq_worker::check_group(const hq_worker_group *src, const hq_member *m, int *self_out, int *n_voting_out) {
    const uint32_t n = src->n_members;
    if (n < 1 || !m) return fail(HQ_E_INVAL, "group has no members");
    if (n > 64) return fail(HQ_E_INVAL, "more than 64 members");
    if (src->state > HQ_STATE_LEADER) return fail(HQ_E_INVAL, "state must be follower, candidate or leader");
    int self = -1, n_voting = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (m[i].role > HQ_ROLE_WITNESS) return fail(HQ_E_INVAL, "unknown member role");
        for (uint32_t j = 0; j < i; ++j)
            if (m[j].node_id == m[i].node_id) return fail(HQ_E_INVAL, "duplicate member");
        if (m[i].role == HQ_ROLE_REMOTE && m[i].node_id == src->node_id) self = (int)i;
        n_voting += m[i].role != HQ_ROLE_OBSERVER;
    }
    if (self < 0) return fail(HQ_E_INVAL, "the node is not one of the group's remotes");
    if (n_voting > (int)n_max) return fail(HQ_E_INVAL, "more voting members than n_max");
    if (dstep && n > kDMembers)
        return fail(HQ_E_INVAL, "more than 16 members on the device path (HQ_WORKER_ON_DEVICE)");
    *self_out = self;
    *n_voting_out = n_voting;
    return HQ_OK;
}

// Validates and loads a group; `fresh` groups get a new member range, others reuse theirs when
// it is large enough.
int hq_worker::load_group(Group &g, const hq_worker_group *src, const hq_member *m, bool fresh) {
    int self = -1, n_voting = 0;
    if (int rc = check_group(src, m, &self, &n_voting)) return rc;
    const uint32_t n = src->n_members;
    if (fresh || g.mem_cap < n) {
        g.mem = (uint32_t)pool.size();
        g.mem_cap = (uint8_t)n;
        pool.resize(pool.size() + n);
    }
    // pool order: the node itself, the other remotes, the witnesses (the voting slots of
    // hq_pack_commit), then the observers
    Member *dst = pool.data() + g.mem;
    int k = 0;
    auto put = [&](uint32_t i) {
        dst[k] = Member{m[i].node_id, m[i].match, (uint8_t)m[i].role, (uint8_t)(m[i].active != 0),
                        (uint8_t)i, {0, 0, 0, 0, 0}};
        ++k;
    };
    put((uint32_t)self);
    for (uint32_t role : {HQ_ROLE_REMOTE, HQ_ROLE_WITNESS, HQ_ROLE_OBSERVER})
        for (uint32_t i = 0; i < n; ++i)
            if (m[i].role == role && (int)i != self) put(i);
    g.cluster_id = src->cluster_id;
    g.node_id = src->node_id;
    g.term = src->term;
    g.committed = src->committed;
    g.last = src->last_index;
    g.term_start = src->term_start;
    g.state = (uint8_t)src->state;
    g.n_members = (uint8_t)n;
    g.n_voting = (uint8_t)n_voting;
    g.ord = 0;
    g.flags = 0;
    rq_release(g);
    // a candidate holds its own vote (campaign, raft.go:1093)
    g.granted = g.state == HQ_STATE_CANDIDATE ? 1 : 0;
    g.rejected = 0;
    return HQ_OK;
}

int hq_worker::add_group(const hq_worker_group *g, const hq_member *members, uint32_t *handle) {
    if (!g) return fail(HQ_E_INVAL, "hq_worker_add_group: group is NULL");
    if (index.count(g->cluster_id)) return fail(HQ_E_INVAL, "hq_worker_add_group: cluster exists");
    if (host_stale) {                               // new pool entries append to a fresh mirror
        int rc = sync_from_device();
        if (rc) return rc;
    }
    if (groups.size() >= UINT32_MAX) return fail(HQ_E_NOMEM, "hq_worker_add_group: too many groups");
    Group n{};
    n.rq = kNone;
    const size_t pool0 = pool.size();
    int rc = load_group(n, g, members, true);
    if (rc) {
        pool.resize(pool0);
        return rc;
    }
    const uint32_t h = (uint32_t)groups.size();
    try {
        groups.push_back(n);
        index.emplace(g->cluster_id, h);
    } catch (...) {                                 // (the group is there whole or not at all)
        groups.resize(h);
        pool.resize(pool0);
        throw;
    }
    if (handle) *handle = h;
    return HQ_OK;
}

// One handle of a batched call's list: a handle there is (a vacant one included: a tombstone record
// without members), in the 16 members the calls' records hold.
int hq_worker::check_listed(const char *entry, uint64_t h) {
    if (h >= groups.size()) return fail(HQ_E_INVAL, std::string(entry) + ": unknown group handle");
    if (groups[h].n_members > kDMembers)
        return fail(HQ_E_INVAL, std::string(entry) + ": a group of more than 16 members");
    return HQ_OK;
}

// ------------------------------------------------------------------------------ C-ABI ------
// (hq_worker_open* answer through hq_last_error(NULL), hq_worker_close and hq_worker_last_error
// return no code: none of the four allocates beyond the nothrow new)
extern "C" {

int hq_worker_open(int device, uint32_t n_max, hq_worker **out) {
    return hq_worker_open_ex(device, n_max, 0, out);
}

int hq_worker_open_ex(int device, uint32_t n_max, uint32_t flags, hq_worker **out) {
    if (!out) return HQ_E_INVAL;
    if (flags & ~(HQ_WORKER_ON_DEVICE | HQ_WORKER_COMMIT_COLUMN | HQ_WORKER_COMMIT_ADVANCE |
                  HQ_WORKER_READY_COMPACT | HQ_WORKER_READY_SLOTS))
        return HQ_E_INVAL;
    if ((flags & (HQ_WORKER_READY_COMPACT | HQ_WORKER_READY_SLOTS)) && !(flags & HQ_WORKER_ON_DEVICE))
        return HQ_E_INVAL;            // (the compact records are the device step's form)
    if ((flags & HQ_WORKER_READY_SLOTS) && !(flags & HQ_WORKER_COMMIT_ADVANCE))
        return HQ_E_INVAL;            // (the slots follow the advance column in the region)
    *out = nullptr;
    if (n_max < 1 || n_max > HQ_MAX_VOTERS) return HQ_E_INVAL;
    hq_worker *w = new (std::nothrow) hq_worker();
    if (!w) return HQ_E_NOMEM;
    int rc = hq_open(device, 0, &w->ctx);
    if (rc) {
        delete w;
        return rc;   // message: hq_last_error(NULL)
    }
    w->n_max = n_max;
    w->device = device;
    if (flags & HQ_WORKER_ON_DEVICE) {
        rc = hq_dstep_open(w->ctx, &w->dstep,
                           ((flags & HQ_WORKER_COMMIT_COLUMN) ? 1u : 0u) |
                               ((flags & HQ_WORKER_COMMIT_ADVANCE) ? 2u : 0u) |
                               ((flags & HQ_WORKER_READY_COMPACT) ? 4u : 0u) |
                               ((flags & HQ_WORKER_READY_SLOTS) ? 8u : 0u));
        if (rc) {
            hq_close(w->ctx);
            delete w;
            return rc;
        }
    }
    *out = w;
    return HQ_OK;
}

void hq_worker_close(hq_worker *w) {
    if (!w) return;
    if (w->hb) hq_hb_dev_close(w->hb);
    if (w->hbw) hq_hbw_dev_close(w->hbw);
    if (w->cfg) hq_cfg_dev_close(w->cfg);
    if (w->grp) hq_groups_dev_close(w->grp);
    if (w->poolc) hq_pool_dev_close(w->poolc);
    if (w->tickd) hq_tick_dev_close(w->tickd);
    if (w->hbr) hq_hbr_dev_close(w->hbr);
    if (w->dstep) hq_dstep_close(w->dstep);
    if (w->ctx) {
        hq_sync(w->ctx);
        if (w->host) hq_free_pinned(w->ctx, w->host);
        if (w->dev) hq_free_dev(w->ctx, w->dev);
        hq_close(w->ctx);
    }
    delete w;
}

const char *hq_worker_last_error(const hq_worker *w) {
    return w ? w->err.c_str() : hq_last_error(nullptr);
}

int hq_worker_add_group(hq_worker *w, const hq_worker_group *g, const hq_member *members,
                        uint32_t *handle) {
    return guarded(w, "hq_worker_add_group", [&] { return w->add_group(g, members, handle); });
}

int hq_worker_add_groups(hq_worker *w, const hq_worker_group *groups, uint64_t count,
                         const hq_member *members) {
    return guarded(w, "hq_worker_add_groups", [&] {
        if (count && (!groups || !members))
            return w->fail(HQ_E_INVAL, "hq_worker_add_groups: NULL argument");
        w->groups.reserve(w->groups.size() + count);
        w->index.reserve(w->groups.size() + count);
        uint64_t off = 0, nm = 0;
        for (uint64_t i = 0; i < count; ++i) nm += groups[i].n_members;
        w->pool.reserve(w->pool.size() + nm);
        for (uint64_t i = 0; i < count; ++i) {
            int rc = w->add_group(groups + i, members + off, nullptr);
            if (rc) return rc;
            off += groups[i].n_members;
        }
        return HQ_OK;
    });
}

int hq_worker_group_count(hq_worker *w, uint64_t *n) {
    return guarded(w, "hq_worker_group_count", [&] {
        if (!n) return HQ_E_INVAL;
        *n = w->groups.size();
        return HQ_OK;
    });
}

int hq_worker_find(hq_worker *w, uint64_t cluster_id, uint32_t *handle) {
    return guarded(w, "hq_worker_find", [&] {
        auto it = w->index.find(cluster_id);
        if (it == w->index.end()) return w->fail(HQ_E_INVAL, "hq_worker_find: unknown cluster");
        if (handle) *handle = it->second;
        return HQ_OK;
    });
}

int hq_worker_set_group(hq_worker *w, const hq_worker_group *g, const hq_member *members) {
    return guarded(w, "hq_worker_set_group", [&] {
        if (!g) return w->fail(HQ_E_INVAL, "hq_worker_set_group: group is NULL");
        auto it = w->index.find(g->cluster_id);
        if (it == w->index.end()) return w->fail(HQ_E_INVAL, "hq_worker_set_group: unknown cluster");
        int rc = w->sync_from_device();
        if (rc) return rc;
        hq::wk::Group n = w->groups[it->second];
        rc = w->load_group(n, g, members, false);
        if (rc) return rc;
        w->groups[it->second] = n;
        w->tick_touch(it->second);                  // (its timer comes back reset)
        if (w->dstep && it->second < w->dev_groups) w->dirty.push_back(it->second);
        return HQ_OK;
    });
}

int hq_worker_get_group(hq_worker *w, uint64_t cluster_id, hq_worker_group *out,
                        hq_member *members, uint32_t cap, hq_read_status *reads,
                        uint32_t reads_cap) {
    return guarded(w, "hq_worker_get_group", [&] {
        auto it = w->index.find(cluster_id);
        if (it == w->index.end()) return w->fail(HQ_E_INVAL, "hq_worker_get_group: unknown cluster");
        int rc = w->sync_from_device();
        if (rc) return rc;
        const Group &g = w->groups[it->second];
        const ReadQueue *q = w->reads(g);
        if (out) {
            out->cluster_id = g.cluster_id;
            out->node_id = g.node_id;
            out->term = g.term;
            out->committed = g.committed;
            out->last_index = g.last;
            out->term_start = g.term_start;
            out->state = g.state;
            out->n_members = g.n_members;
            out->n_pending_reads = q ? q->n : 0;
            out->suspended = g.has(kSuspended);
        }
        if (members) {                              // back in the caller's order
            const Member *m = w->pool.data() + g.mem;
            for (uint32_t i = 0; i < g.n_members; ++i)
                if (m[i].order < cap)
                    members[m[i].order] = hq_member{m[i].node_id, m[i].match, m[i].role, m[i].active};
        }
        if (reads && q)
            for (uint32_t i = 0; i < reads_cap && i < q->n; ++i) {
                const ReadStatus &r = q->r[i];
                uint32_t n = 0;
                for (uint32_t s = 0; s < HQ_MAX_VOTERS; ++s)
                    n += ((r.confirmed >> s) & 1) || r.ord[s] != kNoAck;
                reads[i] = {r.index, r.from, r.low, r.high, n, 0};
            }
        return HQ_OK;
    });
}

int hq_worker_set_wait(hq_worker *w, uint32_t mode, uint32_t poll_us, uint32_t sleep_us) {
    return guarded(w, "hq_worker_set_wait", [&] {
        if (!w->dstep) return w->fail(HQ_E_INVAL, "hq_worker_set_wait: not a device worker");
        const int rc = hq_dstep_set_wait(w->dstep, mode, poll_us, sleep_us);
        if (rc == HQ_E_INVAL) return w->fail(rc, "hq_worker_set_wait: unknown mode (or sleep_us 0)");
        return w->hq(rc, "hq_worker_set_wait");
    });
}

int hq_worker_readback_count(hq_worker *w, uint64_t *n) {
    return guarded(w, "hq_worker_readback_count", [&] {
        if (!n) return HQ_E_INVAL;
        *n = w->readbacks;
        return HQ_OK;
    });
}

}  // extern "C"

// the wire's device mode (hq_wire_dev.hip; declared in hq_dstep.h)
int hq_worker_cluster_ids(hq_worker *w, uint64_t h0, uint64_t n, uint64_t *out) {
    if (!w || h0 > w->groups.size() || n > w->groups.size() - h0 || (n && !out)) return HQ_E_INVAL;
    for (uint64_t i = 0; i < n; ++i) out[i] = w->groups[h0 + i].cluster_id;
    return HQ_OK;
}
