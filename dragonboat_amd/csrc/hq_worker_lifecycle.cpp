// hq_worker_lifecycle.cpp — groups started and stopped on a running worker and the member pool's
// compaction (hq_worker_k.h; include/hipquorum.h "group lifecycle"), host and device arms. None of
// the calls reads the device state back or touches host_stale: the structure of the mirror (handles,
// member ranges, the index) is the host's own even while its values are stale, and what a device
// worker writes are whole records made from the call's arguments.
#include "hq_worker_k.h"

using namespace hq::wk;

// A handle's row of the heartbeat route column back to "no route" (a group that starts in a reused
// handle must not inherit its predecessor's destinations).
void hq_worker::reset_route_row(uint32_t h) {
    if (routes.size() < ((size_t)h + 1) * kDMembers) return;   // (rows are made HQ_ROUTE_NONE)
    std::fill_n(routes.begin() + (size_t)h * kDMembers, kDMembers, (uint16_t)HQ_ROUTE_NONE);
    if (routes_lo == routes_hi) {
        routes_lo = h;
        routes_hi = (uint64_t)h + 1;
    } else {
        routes_lo = std::min<uint64_t>(routes_lo, h);
        routes_hi = std::max<uint64_t>(routes_hi, (uint64_t)h + 1);
    }
}

// A device worker: the host records of handles hs[0 .. n) (distinct) written to their places in the
// resident state with the listed groups' scatter kernel (hq_groups.hip), as hq_worker_set_groups
// writes its groups. The device arrays already hold every handle and member range.
int hq_worker::scatter_records(const char *entry, uint64_t n, const uint32_t *hs, uint64_t *gpu_ns) {
    hq_grp_record *recs = nullptr;
    uint32_t *hh = nullptr;
    int rc = hq(hq_groups_dev_stage(grp, n, &recs, &hh), entry);
    if (rc) return rc;
    for (uint64_t i = 0; i < n; ++i) {
        hq_dgroup dg;
        hq_dread dr[kDReads];
        hq_dmember dm[kDMembers];
        to_device_record(groups[hs[i]], dg, dr, dm);
        grp_pack(recs[i], dg, dr, dm);
        hh[i] = hs[i];
    }
    hq_dstate_mut st;
    hq_dstep_view_mut(dstep, &st);
    uint32_t e = 0;
    uint64_t ns = 0;
    rc = hq_groups_dev_scatter(grp, &st, dev_members, n, &ns, &e);
    if (rc == HQ_E_INVAL && e)
        return fail(HQ_E_STATE, std::string(entry) + ": a packed group record does not fit the state's "
                                                     "sizes (internal)");
    if ((rc = hq(rc, entry))) return rc;
    if (gpu_ns) *gpu_ns = ns;
    return HQ_OK;
}

int hq_worker::start_groups(uint64_t n, const hq_worker_group *gs, const hq_member *ms, uint32_t *handles,
                            uint64_t *gpu_ns) {
    const char *const entry = "hq_worker_start_groups";
    // every group is checked before any is added
    uint64_t nm = 0;
    uint32_t most = 0;
    std::vector<uint64_t> ids(n);
    for (uint64_t i = 0; i < n; ++i) {
        if (index.count(gs[i].cluster_id)) return fail(HQ_E_INVAL, "hq_worker_start_groups: cluster exists");
        int self = 0, nv = 0;
        if (int bad = check_group(gs + i, ms + nm, &self, &nv)) return bad;
        ids[i] = gs[i].cluster_id;
        nm += gs[i].n_members;
        most = std::max<uint32_t>(most, gs[i].n_members);
    }
    std::sort(ids.begin(), ids.end());
    if (std::adjacent_find(ids.begin(), ids.end()) != ids.end())
        return fail(HQ_E_INVAL, "hq_worker_start_groups: a cluster is listed twice");
    const uint64_t fresh = n > vacant.size() ? n - vacant.size() : 0;
    if (groups.size() + fresh > UINT32_MAX) return fail(HQ_E_NOMEM, "hq_worker_start_groups: too many groups");
    if (pool.size() + nm > UINT32_MAX) return fail(HQ_E_NOMEM, "hq_worker_start_groups: member pool full");

    // everything that can run out of memory before anything changes
    std::vector<uint32_t> hs(n);
    // (vector::reserve allocates exactly what it is asked for: grown by halves here, or every call
    // on a large worker would copy the whole pool)
    auto room = [](auto &v, size_t need) {
        if (need > v.capacity()) v.reserve(std::max(need, v.capacity() + v.capacity() / 2));
    };
    room(groups, groups.size() + fresh);
    room(pool, pool.size() + nm);
    // (only when the buckets run short: reserve() on a table that has room re-buckets all of it)
    if ((double)(index.size() + n) > (double)index.bucket_count() * index.max_load_factor())
        index.reserve(index.size() + n);
    if (dstep) {
        int rc = sync_to_device();                  // pending add / set_group first, as a step does
        if (rc) return rc;
        if (!grp && (rc = hq(hq_groups_dev_open(ctx, &grp), entry))) return rc;
        hq_grp_record *recs = nullptr;
        uint32_t *hh = nullptr;
        if ((rc = hq(hq_groups_dev_stage(grp, n, &recs, &hh), entry))) return rc;
        // the device arrays stay index-identical with the host's: the new handles' records and the
        // new member ranges exist there before the kernel writes them and are never uploaded from
        // the mirror (the groups last: a failure before them leaves the handle space as it was)
        if ((rc = hq(hq_dstep_reserve_members(dstep, dev_members, pool.size() + nm), entry))) return rc;
        if ((rc = hq(hq_dstep_reserve_groups(dstep, groups.size() + fresh), entry))) return rc;
    }
    // load_group sets every field to_device_record reads: a stale mirror does not matter
    uint64_t off = 0;
    for (uint64_t i = 0; i < n; ++i) {
        Group g{};
        g.rq = kNone;
        if (int rc = load_group(g, gs + i, ms + off, true)) return rc;   // (checked above: cannot fail)
        off += gs[i].n_members;
        uint32_t h;
        if (vacant.empty()) {
            h = (uint32_t)groups.size();
            groups.push_back(g);
        } else {
            h = vacant.back();                      // the most recently vacated first
            vacant.pop_back();
            groups[h] = g;
        }
        index.emplace(g.cluster_id, h);
        reset_route_row(h);
        tick_touch(h);                              // (a reused handle's timer comes back reset)
        hs[i] = h;
    }
    ++epoch;
    if (handles) std::copy(hs.begin(), hs.end(), handles);
    if (!dstep) return HQ_OK;
    dev_groups = groups.size();
    dev_members = pool.size();
    hq_dstep_raise_max_members(dstep, most);        // the step's 8-slot kernels must not see 9 members
    return scatter_records(entry, n, hs.data(), gpu_ns);
}

int hq_worker::stop_groups(uint64_t n, const uint32_t *handles, uint64_t *gpu_ns) {
    const char *const entry = "hq_worker_stop_groups";
    int rc = check_distinct(
        n, "hq_worker_stop_groups: a group is listed twice",
        [&](uint64_t i, uint32_t &h) {
            h = handles[i];
            return live(h) ? HQ_OK : fail(HQ_E_INVAL, "hq_worker_stop_groups: unknown group handle");
        },
        [](uint64_t, uint32_t) { return HQ_OK; });
    if (rc) return rc;
    vacant.reserve(vacant.size() + n);
    if (dstep) {
        rc = sync_to_device();                      // pending add / set_group first, as a step does
        if (rc) return rc;
        if (!grp && (rc = hq(hq_groups_dev_open(ctx, &grp), entry))) return rc;
        hq_grp_record *recs = nullptr;
        uint32_t *hh = nullptr;
        if ((rc = hq(hq_groups_dev_stage(grp, n, &recs, &hh), entry))) return rc;
    }
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t h = handles[i];
        Group &g = groups[h];
        index.erase(g.cluster_id);
        rq_release(g);
        // the tombstone: a suspended follower without members or voting slots; its member range
        // stays in the pool as a gap until hq_worker_compact
        Group t{};
        t.rq = kNone;
        t.state = HQ_STATE_FOLLOWER;
        t.flags = kSuspended | kVacant;
        g = t;
        vacant.push_back(h);
        reset_route_row(h);
    }
    ++epoch;
    if (!dstep) return HQ_OK;
    return scatter_records(entry, n, handles, gpu_ns);
}

uint64_t hq_worker::live_member_records() const {
    uint64_t total = 0;
    for (const Group &g : groups) total += g.n_members;   // (a tombstone has none)
    return total;
}

// The member ranges packed in handle order, mem_cap = n_members. A device worker's kernel moves the
// resident records by the same column of new bases the mirror's records move by here (stale values
// move along), so the two pools stay index-identical.
int hq_worker::compact(uint64_t *gpu_ns) {
    const char *const entry = "hq_worker_compact";
    const uint64_t total = live_member_records();
    if (total == pool.size()) return HQ_OK;         // dense: every record is a live group's
    const uint64_t G = groups.size();
    std::vector<uint32_t> own;
    uint32_t *col = nullptr;
    hq_dmember *spare = nullptr;
    if (dstep) {
        int rc = sync_to_device();                  // pending add / set_group first, as a step does
        if (rc) return rc;
        if (!poolc && (rc = hq(hq_pool_dev_open(ctx, &poolc), entry))) return rc;
        if ((rc = hq(hq_pool_dev_stage(poolc, G, &col), entry))) return rc;
    } else {
        own.resize(G);
        col = own.data();
    }
    uint64_t next = 0;
    for (uint64_t h = 0; h < G; ++h) {
        col[h] = groups[h].n_members ? (uint32_t)next : 0;
        next += groups[h].n_members;
    }
    std::vector<Member> packed(total);
    if (dstep) {
        uint64_t capacity = 0;
        int rc = hq(hq_dstep_members_spare(dstep, &spare, &capacity), entry);
        if (rc) return rc;
        if (!spare || total > capacity) {
            hq_dstep_members_drop(dstep, spare);
            return fail(HQ_E_STATE, "hq_worker_compact: the resident member pool is smaller than the host's (internal)");
        }
        hq_dstate_mut st;
        hq_dstep_view_mut(dstep, &st);
        uint32_t e = 0;
        uint64_t ns = 0;
        rc = hq_pool_dev_compact(poolc, &st, dev_members, spare, total, &ns, &e);
        if (rc) {
            hq_dstep_members_drop(dstep, spare);
            if (rc == HQ_E_INVAL && e)
                return fail(HQ_E_STATE, "hq_worker_compact: a resident group record does not match the "
                                        "host's (internal)");
            return hq(rc, entry);
        }
        hq_dstep_members_install(dstep, spare);     // (the kernel has been waited for)
        if (gpu_ns) *gpu_ns = ns;
    }
    for (uint64_t h = 0; h < G; ++h) {
        Group &g = groups[h];
        std::copy_n(pool.begin() + g.mem, g.n_members, packed.begin() + col[h]);
        g.mem = col[h];
        g.mem_cap = g.n_members;
    }
    pool.swap(packed);
    if (dstep) dev_members = pool.size();
    return HQ_OK;
}

// ------------------------------------------------------------------------------ C-ABI ------
extern "C" {

int hq_worker_start_groups(hq_worker *w, uint64_t n, const hq_worker_group *groups,
                           const hq_member *members, uint32_t *handles, uint64_t *gpu_ns) {
    return guarded(w, "hq_worker_start_groups", [&] {
        if (gpu_ns) *gpu_ns = 0;
        if (n && (!groups || !members)) return w->fail(HQ_E_INVAL, "hq_worker_start_groups: NULL argument");
        if (n > UINT32_MAX) return w->fail(HQ_E_INVAL, "hq_worker_start_groups: too many groups listed");
        if (n == 0) return HQ_OK;
        return w->start_groups(n, groups, members, handles, gpu_ns);
    });
}

int hq_worker_stop_groups(hq_worker *w, uint64_t n, const uint32_t *handles, uint64_t *gpu_ns) {
    return guarded(w, "hq_worker_stop_groups", [&] {
        if (gpu_ns) *gpu_ns = 0;
        if (n && !handles) return w->fail(HQ_E_INVAL, "hq_worker_stop_groups: NULL argument");
        if (n > UINT32_MAX) return w->fail(HQ_E_INVAL, "hq_worker_stop_groups: a group is listed twice");
        if (n == 0) return HQ_OK;
        return w->stop_groups(n, handles, gpu_ns);
    });
}

int hq_worker_pool_info(hq_worker *w, hq_pool_info *out) {
    return guarded(w, "hq_worker_pool_info", [&] {
        if (!out) return w->fail(HQ_E_INVAL, "hq_worker_pool_info: NULL argument");
        out->handles = w->groups.size();
        out->vacant_handles = w->vacant.size();
        out->live_groups = w->groups.size() - w->vacant.size();
        out->member_records = w->pool.size();
        out->live_member_records = w->live_member_records();
        out->epoch = w->epoch;
        return HQ_OK;
    });
}

int hq_worker_compact(hq_worker *w, uint64_t *gpu_ns) {
    return guarded(w, "hq_worker_compact", [&] {
        if (gpu_ns) *gpu_ns = 0;
        return w->compact(gpu_ns);
    });
}

}  // extern "C"

// both attached wire modes (hq_wire.cpp, hq_wire_dev.hip; declared in hq_dstep.h)
uint64_t hq_worker_epoch(hq_worker *w) { return w ? w->epoch : 0; }

int hq_worker_live_handles(hq_worker *w, uint64_t h0, uint64_t n, uint8_t *out) {
    if (!w || h0 > w->groups.size() || n > w->groups.size() - h0 || (n && !out)) return HQ_E_INVAL;
    for (uint64_t i = 0; i < n; ++i) out[i] = w->live(h0 + i) ? 1 : 0;
    return HQ_OK;
}
