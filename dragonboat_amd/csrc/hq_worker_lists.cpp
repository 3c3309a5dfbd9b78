// hq_worker_lists.cpp — the step worker's batched calls over listed groups that change or move
// group state (hq_worker_k.h): membership changes (hq_worker_config_changes) and the listed
// groups' fetch / resume (hq_worker_get_groups / hq_worker_set_groups), host and device arms.
#include "hq_worker_k.h"

using namespace hq::wk;

// ------------------------------------------------------------------------------ membership ---
// handleNodeConfigChange (raft.go:1540-1559) for the listed groups. The structure of a group —
// member ids, roles, positions — is the host's own even while a device worker's mirror is stale,
// so every change becomes a descriptor here (hq_config.h); a device worker's are applied where
// the state lives (hq_config.hip), a host worker's below, and the same structural edit then goes
// into the host records of both.

// One change as a descriptor, from the group's structure alone. HQ_E_INVAL for what the reference
// panics on.
int hq_worker::config_desc(const Group &g, const hq_config_change &c, uint32_t limit, hq_cfg_desc &d) {
    d = hq_cfg_desc{};
    d.node_id = c.node_id;
    d.group = c.group;
    d.new_mem = kCfgNoMove;
    d.kind = kCfgNoop;
    d.slot = kCfgNoSlot;
    d.n_members = g.n_members;
    d.n_voting = g.n_voting;
    const Member *m = pool.data() + g.mem;
    hq_cfg_layout l{0, g.n_voting, g.n_members};
    while (l.n_remotes < g.n_voting && m[l.n_remotes].role == HQ_ROLE_REMOTE) ++l.n_remotes;
    const int mi = member_of(g, c.node_id);
    const uint32_t role = mi >= 0 ? m[mi].role : 0xFFu;
    uint32_t new_role = HQ_ROLE_REMOTE;
    switch (c.type) {
    case HQ_CC_REMOVE_NODE:
        if (mi < 0) {
            d.kind = kCfgCommitOnly;                // removeNode's tryCommit runs all the same
        } else if (mi == 0) {
            d.kind = kCfgFallback;                  // the node itself: dragonboat stops it
        } else {
            d.kind = kCfgRemove;
            d.src = (uint8_t)mi;
            d.slot = (uint8_t)cfg_remove_slot((uint32_t)mi, l);
            d.order = m[mi].order;
        }
        return HQ_OK;
    case HQ_CC_ADD_NODE:
        if (role == HQ_ROLE_REMOTE) return HQ_OK;   // already a voting member (raft.go:1141-1144)
        if (role == HQ_ROLE_WITNESS)
            return fail(HQ_E_INVAL, "hq_worker_config_changes: ADD_NODE of a witness (the reference "
                                    "panics: could not promote witness to a full member)");
        if (role == HQ_ROLE_OBSERVER) {             // promoted with its progress (raft.go:1145-1148)
            if (g.n_voting + 1u > n_max) {
                d.kind = kCfgFallback;
                return HQ_OK;
            }
            d.kind = kCfgPromote;
            d.src = (uint8_t)mi;
            d.dst = d.slot = (uint8_t)cfg_promote_pos(l);
            return HQ_OK;
        }
        break;
    case HQ_CC_ADD_OBSERVER:
    case HQ_CC_ADD_WITNESS:
        new_role = c.type == HQ_CC_ADD_OBSERVER ? HQ_ROLE_OBSERVER : HQ_ROLE_WITNESS;
        if (role == new_role) return HQ_OK;
        if (mi >= 0)
            return fail(HQ_E_INVAL, "hq_worker_config_changes: ADD_OBSERVER / ADD_WITNESS of a member "
                                    "in another role");
        break;
    default:
        return fail(HQ_E_INVAL, "hq_worker_config_changes: unknown change type");
    }
    // a new member, match 0 and inactive (setRemote / setObserver / setWitness(nodeID, 0, ...))
    if (g.n_members + 1u > limit || (new_role != HQ_ROLE_OBSERVER && g.n_voting + 1u > n_max)) {
        d.kind = kCfgFallback;
        return HQ_OK;
    }
    d.kind = kCfgInsert;
    d.dst = (uint8_t)cfg_insert_pos(c.type, l);
    d.slot = (uint8_t)cfg_insert_slot(c.type, l);
    d.role = (uint8_t)new_role;
    d.order = g.n_members;
    return HQ_OK;
}

// The structural edit of an applied change in the host records (a host worker's state; a device
// worker's mirror, index-identical with the device pool), and the group's row of the route column.
void hq_worker::config_edit(Group &g, uint32_t h, const hq_cfg_desc &d, uint8_t new_cap) {
    Member *m = members(g);
    const uint32_t n = g.n_members;
    const bool rm = d.kind == kCfgRemove;
    if (rm) {
        for (uint32_t j = d.src; j + 1 < n; ++j) m[j] = m[j + 1];
        for (uint32_t j = 0; j + 1 < n; ++j)
            m[j].order = (uint8_t)cfg_order_after_remove(m[j].order, d.order);
        g.n_members = (uint8_t)(n - 1);
    } else if (d.kind == kCfgInsert) {
        const Member fresh{d.node_id, 0, d.role, 0, d.order, {0, 0, 0, 0, 0}};
        if (d.new_mem != kCfgNoMove) {
            Member *nm = pool.data() + d.new_mem;
            for (uint32_t j = 0; j < n; ++j) nm[cfg_pos_after_insert(j, d.dst)] = m[j];
            nm[d.dst] = fresh;
            g.mem = d.new_mem;
            g.mem_cap = new_cap;
        } else {
            for (uint32_t j = n; j > d.dst; --j) m[j] = m[j - 1];
            m[d.dst] = fresh;
        }
        g.n_members = (uint8_t)(n + 1);
    } else {                                        // kCfgPromote
        Member carry = m[d.src];
        for (uint32_t j = d.src; j > d.dst; --j) m[j] = m[j - 1];
        carry.role = HQ_ROLE_REMOTE;
        m[d.dst] = carry;
    }
    if (d.slot != kCfgNoSlot) {                     // the slot bitmaps follow the voting slots
        const uint32_t s = d.slot;
        auto remap = [&](uint8_t b) {
            return (uint8_t)(rm ? cfg_remove_bit(b, s) : cfg_insert_bit(b, s));
        };
        g.granted = remap(g.granted);
        g.rejected = remap(g.rejected);
        if (ReadQueue *q = reads(g))
            for (uint32_t k = 0; k < q->n; ++k) {
                ReadStatus &r = q->r[k];
                r.confirmed = remap(r.confirmed);
                if (rm) {
                    for (uint32_t v = s; v + 1 < HQ_MAX_VOTERS; ++v) r.ord[v] = r.ord[v + 1];
                    r.ord[HQ_MAX_VOTERS - 1] = kNoAck;
                } else {
                    for (uint32_t v = HQ_MAX_VOTERS - 1; v > s; --v) r.ord[v] = r.ord[v - 1];
                    r.ord[s] = kNoAck;
                }
            }
        g.n_voting = (uint8_t)(rm ? g.n_voting - 1 : g.n_voting + 1);
    }
    // the route column's row moves with the member list
    if (d.kind == kCfgPromote || routes.size() < ((size_t)h + 1) * kDMembers) return;
    uint16_t *row = routes.data() + (size_t)h * kDMembers;
    if (rm) {
        const uint32_t end = std::min<uint32_t>(n, kDMembers);
        for (uint32_t j = d.order; j + 1 < end; ++j) row[j] = row[j + 1];
        if (d.order < end) row[end - 1] = (uint16_t)HQ_ROUTE_NONE;
    } else if (d.order < kDMembers) {
        row[d.order] = (uint16_t)HQ_ROUTE_NONE;
    }
    if (routes_lo == routes_hi) {
        routes_lo = h;
        routes_hi = (uint64_t)h + 1;
    } else {
        routes_lo = std::min<uint64_t>(routes_lo, h);
        routes_hi = std::max<uint64_t>(routes_hi, (uint64_t)h + 1);
    }
}

int hq_worker::config_changes(uint64_t n, const hq_config_change *ch, hq_config_output *out) {
    const uint32_t limit = dstep ? kDMembers : 64;
    // every check first: a refused list changes nothing
    cc_desc.resize(n);
    int rc = check_distinct(
        n, "hq_worker_config_changes: a group is listed twice",
        [&](uint64_t i, uint32_t &h) {
            h = ch[i].group;
            return live(h) ? HQ_OK : fail(HQ_E_INVAL, "hq_worker_config_changes: unknown group handle");
        },
        [&](uint64_t i, uint32_t h) {
            const hq_config_change &c = ch[i];
            if (c.type > HQ_CC_ADD_WITNESS) return fail(HQ_E_INVAL, "hq_worker_config_changes: unknown change type");
            if (c.node_id == 0) return fail(HQ_E_INVAL, "hq_worker_config_changes: node_id 0");
            return config_desc(groups[h], c, limit, cc_desc[i]);
        });
    if (rc) return rc;

    cc_cap.assign(n, 0);
    cc_commits.clear();
    // a full member range moves to the pool's end (with room for one more change)
    auto move_out = [&](uint64_t i) {
        hq_cfg_desc &d = cc_desc[i];
        const Group &g = groups[d.group];
        if (d.kind != kCfgInsert || g.mem_cap > g.n_members) return;
        cc_cap[i] = (uint8_t)std::min<uint32_t>(limit, g.n_members + 2u);
        d.new_mem = (uint32_t)pool.size();
        pool.resize(pool.size() + cc_cap[i]);
    };
    const uint32_t *status = nullptr;
    const uint64_t *committed = nullptr;
    uint64_t gpu_ns = 0;
    if (dstep) {
        rc = sync_to_device();                      // pending add / set_group first, as a step does
        if (rc) return rc;
        uint32_t most = 0;
        for (uint64_t i = 0; i < n; ++i) {
            if (pool.size() + limit > UINT32_MAX) return fail(HQ_E_NOMEM, "hq_worker_config_changes: member pool full");
            move_out(i);
            if (cc_desc[i].kind == kCfgInsert) most = std::max<uint32_t>(most, cc_desc[i].n_members + 1u);
        }
        // the device pool stays index-identical with the host's: the reserved records exist there
        // before the kernel writes them and are never uploaded from the mirror
        rc = hq(hq_dstep_reserve_members(dstep, dev_members, pool.size()), "hq_worker_config_changes");
        if (rc) {
            pool.resize(dev_members);
            return rc;
        }
        dev_members = pool.size();
        hq_dstep_raise_max_members(dstep, most);    // the step's 8-slot kernels must not see 9 members
        if (!cfg && (rc = hq(hq_cfg_dev_open(ctx, &cfg), "hq_worker_config_changes"))) return rc;
        hq_dstate_mut st;
        hq_dstep_view_mut(dstep, &st);
        uint32_t e = 0;
        rc = hq_cfg_dev_run(cfg, &st, dev_members, n, cc_desc.data(), &status, &committed, &gpu_ns, &e);
        if (rc == HQ_E_INVAL && e)
            return fail(HQ_E_STATE, "hq_worker_config_changes: a resident group record does not match "
                                    "the host's (internal)");
        if ((rc = hq(rc, "hq_worker_config_changes"))) return rc;
    } else {
        // a host worker decides from its own records what the kernel decides from the resident ones
        cc_status.resize(n);
        for (uint64_t i = 0; i < n; ++i) {
            const hq_cfg_desc &d = cc_desc[i];
            const Group &g = groups[d.group];
            uint32_t s = HQ_CC_NOOP;
            if (g.has(kSuspended)) {
                s = HQ_CC_SUSPENDED;
            } else if (d.kind == kCfgFallback) {
                s = HQ_CC_FALLBACK;
            } else if (d.kind >= kCfgRemove) {
                s = HQ_CC_APPLIED;
                if (d.kind == kCfgRemove && d.slot != kCfgNoSlot) {
                    uint32_t bits = g.granted | g.rejected;
                    if (const ReadQueue *q = reads(g))
                        for (uint32_t k = 0; k < q->n; ++k) {
                            bits |= q->r[k].confirmed;
                            for (uint32_t v = 0; v < HQ_MAX_VOTERS; ++v)
                                if (q->r[k].ord[v] != kNoAck) bits |= 1u << v;
                        }
                    if ((bits >> d.slot) & 1) s = HQ_CC_FALLBACK;
                }
            }
            cc_status[i] = s;
            if (s == HQ_CC_APPLIED) {
                if (pool.size() + limit > UINT32_MAX) return fail(HQ_E_NOMEM, "hq_worker_config_changes: member pool full");
                move_out(i);
            }
        }
        status = cc_status.data();
    }

    // the same edit in the host records; a host worker's tryCommit through its commit pass
    l_commit.clear();
    l_ri.clear();
    l_vote.clear();
    l_cq.clear();
    uint64_t counts[4] = {0, 0, 0, 0};
    for (uint64_t i = 0; i < n; ++i) {
        const hq_cfg_desc &d = cc_desc[i];
        Group &g = groups[d.group];
        const uint32_t s = status[i] <= HQ_CC_SUSPENDED ? status[i] : HQ_CC_SUSPENDED;
        ++counts[s];
        if (s == HQ_CC_FALLBACK) g.set(kSuspended);
        if (s == HQ_CC_APPLIED) config_edit(g, d.group, d, cc_cap[i]);
        const bool removal = d.kind == kCfgRemove || d.kind == kCfgCommitOnly;
        if (dstep) {
            if (committed[i]) {
                g.committed = committed[i];
                cc_commits.push_back({g.cluster_id, committed[i]});
            }
        } else if (removal && s <= HQ_CC_NOOP && g.state == HQ_STATE_LEADER) {
            g.committed0 = g.committed;             // removeNode's tryCommit (raft.go:1194-1198)
            g.set(kCommitDue);
            l_commit.push_back(d.group);
        }
    }
    if (!l_commit.empty()) {
        rc = run_pass();
        for (uint32_t gi : l_commit) groups[gi].clear(kCommitDue);
        if (rc) return rc;
        for (uint32_t gi : l_commit) {
            const Group &g = groups[gi];
            if (g.committed != g.committed0) cc_commits.push_back({g.cluster_id, g.committed});
        }
    }
    out->status = status;
    out->commits = cc_commits.data();
    out->n_commits = cc_commits.size();
    out->n_applied = counts[HQ_CC_APPLIED];
    out->n_noop = counts[HQ_CC_NOOP];
    out->n_fallback = counts[HQ_CC_FALLBACK];
    out->n_suspended = counts[HQ_CC_SUSPENDED];
    out->gpu_ns = gpu_ns;
    return HQ_OK;
}

// ------------------------------------------------------------------------------ listed groups --
// hq_worker_get_groups / hq_worker_set_groups (include/hipquorum.h "listed groups"): a device
// worker moves one packed record per listed group between the resident state and pinned host
// memory (hq_groups.hip); a host worker packs the same records from its own. Neither call reads
// the device state back or touches host_stale.

// One group of a get_groups output from its device-form records (members in pool order): the
// group as get_group fills it, members in the caller's order, masks in the caller's terms.
bool hq_worker::emit_group(const hq_dgroup &d, const hq_dread *r, const hq_dmember *m) {
    gg_groups.push_back(hq_worker_group{d.cluster_id, d.node_id, d.term, d.committed, d.last, d.term_start,
                                        d.state, d.n_members, d.n_reads,
                                        (d.flags & kDSuspended) ? 1u : 0u});
    const size_t m0 = gg_members.size();
    gg_members.resize(m0 + d.n_members);
    for (uint32_t i = 0; i < d.n_members; ++i) {
        if (m[i].order >= d.n_members) return false;
        gg_members[m0 + m[i].order] = hq_member{m[i].node_id, m[i].match, m[i].role, m[i].active};
    }
    gg_moff.push_back(gg_members.size());
    for (uint32_t k = 0; k < d.n_reads; ++k) {
        uint32_t c = 0;
        for (uint32_t s = 0; s < HQ_MAX_VOTERS; ++s) c += (r[k].confirmed >> s) & 1u;
        gg_reads.push_back(hq_read_status{r[k].index, r[k].from, r[k].low, r[k].high, c, 0});
        gg_rconf.push_back(grp_slots_to_list(r[k].confirmed, d.n_voting, m));
    }
    gg_roff.push_back(gg_reads.size());
    gg_granted.push_back(grp_slots_to_list(d.granted, d.n_voting, m));
    gg_rejected.push_back(grp_slots_to_list(d.rejected, d.n_voting, m));
    return true;
}

int hq_worker::get_groups(uint64_t n, const uint32_t *handles, hq_groups_output *out) {
    // every check the host can make first: nothing is queued for a refused list
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t h = handles ? handles[i] : i;
        if (int rc = check_listed("hq_worker_get_groups", h)) return rc;
        if (!live(h)) return fail(HQ_E_INVAL, "hq_worker_get_groups: unknown group handle");
    }
    for (auto *v : {&gg_granted, &gg_rejected, &gg_rconf}) v->clear();
    gg_groups.clear();
    gg_members.clear();
    gg_reads.clear();
    gg_moff.assign(1, 0);
    gg_roff.assign(1, 0);
    gg_groups.reserve(n);
    gg_moff.reserve(n + 1);
    gg_roff.reserve(n + 1);
    gg_granted.reserve(n);
    gg_rejected.reserve(n);
    uint64_t gpu_ns = 0;
    hq_dgroup dg;
    hq_dread dr[kDReads];
    hq_dmember dm[kDMembers];
    if (dstep) {
        int rc = sync_to_device();                  // pending add / set_group first, as a step does
        if (rc) return rc;
        if (!grp && (rc = hq(hq_groups_dev_open(ctx, &grp), "hq_worker_get_groups"))) return rc;
        hq_grp_record *recs = nullptr;
        uint32_t *hh = nullptr;
        if ((rc = hq(hq_groups_dev_stage(grp, n, &recs, &hh), "hq_worker_get_groups"))) return rc;
        if (handles) std::copy(handles, handles + n, hh);
        hq_dstate_view st;
        hq_dstep_view(dstep, &st);
        uint32_t e = 0;
        rc = hq_groups_dev_gather(grp, &st, dev_members, n, !handles, &gpu_ns, &e);
        if (rc == HQ_E_INVAL && e)
            return fail(HQ_E_STATE, "hq_worker_get_groups: a resident group record does not fit the "
                                    "state's sizes (internal)");
        if ((rc = hq(rc, "hq_worker_get_groups"))) return rc;
        for (uint64_t i = 0; i < n; ++i) {
            // the mirror's structure is the host's own even while its values are stale
            const Group &g = groups[handles ? handles[i] : i];
            bool same = grp_unpack(recs[i], dg, dr, dm) && dg.cluster_id == g.cluster_id &&
                        dg.n_members == g.n_members && dg.n_voting == g.n_voting && dg.mem == g.mem;
            for (uint32_t j = 0; same && j < g.n_members; ++j) same = dm[j].node_id == pool[g.mem + j].node_id;
            if (!same || !emit_group(dg, dr, dm))
                return fail(HQ_E_STATE, "hq_worker_get_groups: a resident group record does not match "
                                        "the host's (internal)");
        }
    } else {
        for (uint64_t i = 0; i < n; ++i) {
            const Group &g = groups[handles ? handles[i] : i];
            to_device_record(g, dg, dr, dm);
            if (!emit_group(dg, dr, dm)) return fail(HQ_E_STATE, "hq_worker_get_groups: member order (internal)");
        }
    }
    out->groups = gg_groups.data();
    out->members = gg_members.data();
    out->member_offsets = gg_moff.data();
    out->reads = gg_reads.data();
    out->read_offsets = gg_roff.data();
    out->granted = gg_granted.data();
    out->rejected = gg_rejected.data();
    out->read_confirmed = gg_rconf.data();
    out->n_groups = n;
    out->gpu_ns = gpu_ns;
    return HQ_OK;
}

int hq_worker::set_groups(uint64_t n, const hq_worker_group *gs, const hq_member *ms, uint64_t *gpu_ns) {
    // every group is checked before any is changed
    uint64_t off = 0, extra = 0;
    uint32_t most = 0;
    int rc = check_distinct(
        n, "hq_worker_set_groups: a cluster is listed twice",
        [&](uint64_t i, uint32_t &h) {
            auto it = index.find(gs[i].cluster_id);
            if (it == index.end()) return fail(HQ_E_INVAL, "hq_worker_set_groups: unknown cluster");
            h = it->second;
            return HQ_OK;
        },
        [&](uint64_t i, uint32_t h) {
            const hq_worker_group &g = gs[i];
            int self = 0, nv = 0;
            if (int bad = check_group(&g, ms + off, &self, &nv)) return bad;
            if (groups[h].mem_cap < g.n_members) extra += g.n_members;   // it moves to the pool's end
            most = std::max<uint32_t>(most, g.n_members);
            off += g.n_members;
            return HQ_OK;
        });
    if (rc) return rc;
    if (pool.size() + extra > UINT32_MAX) return fail(HQ_E_NOMEM, "hq_worker_set_groups: member pool full");

    hq_grp_record *recs = nullptr;
    uint32_t *hh = nullptr;
    if (dstep) {
        rc = sync_to_device();                      // pending add / set_group first, as a step does
        if (rc) return rc;
        if (!grp && (rc = hq(hq_groups_dev_open(ctx, &grp), "hq_worker_set_groups"))) return rc;
        if ((rc = hq(hq_groups_dev_stage(grp, n, &recs, &hh), "hq_worker_set_groups"))) return rc;
        // the device pool stays index-identical with the host's: the ranges of the groups that move
        // exist there before the kernel writes them and are never uploaded from the mirror
        rc = hq(hq_dstep_reserve_members(dstep, dev_members, pool.size() + extra), "hq_worker_set_groups");
        if (rc) return rc;
    }
    // load_group sets every field to_device_record reads: a stale mirror does not matter
    off = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t h = index.find(gs[i].cluster_id)->second;
        Group g = groups[h];
        if ((rc = load_group(g, gs + i, ms + off, false))) return rc;   // (checked above: cannot fail)
        groups[h] = g;
        tick_touch(h);                              // (its timer comes back reset)
        off += gs[i].n_members;
        if (!dstep) continue;
        hq_dgroup dg;
        hq_dread dr[kDReads];
        hq_dmember dm[kDMembers];
        to_device_record(g, dg, dr, dm);
        grp_pack(recs[i], dg, dr, dm);
        hh[i] = h;
    }
    if (!dstep) return HQ_OK;
    dev_members = pool.size();
    hq_dstep_raise_max_members(dstep, most);        // the step's 8-slot kernels must not see 9 members
    hq_dstate_mut st;
    hq_dstep_view_mut(dstep, &st);
    uint32_t e = 0;
    uint64_t ns = 0;
    rc = hq_groups_dev_scatter(grp, &st, dev_members, n, &ns, &e);
    if (rc == HQ_E_INVAL && e)
        return fail(HQ_E_STATE, "hq_worker_set_groups: a packed group record does not fit the state's "
                                "sizes (internal)");
    if ((rc = hq(rc, "hq_worker_set_groups"))) return rc;
    if (gpu_ns) *gpu_ns = ns;
    return HQ_OK;
}

// ------------------------------------------------------------------------------ C-ABI ------
extern "C" {

int hq_worker_get_groups(hq_worker *w, uint64_t n, const uint32_t *handles, hq_groups_output *out) {
    return guarded(w, "hq_worker_get_groups", [&] {
        if (!out) return w->fail(HQ_E_INVAL, "hq_worker_get_groups: NULL argument");
        std::memset(out, 0, sizeof *out);
        if (n > UINT32_MAX) return w->fail(HQ_E_INVAL, "hq_worker_get_groups: too many groups listed");
        if (n == 0) return HQ_OK;
        return w->get_groups(n, handles, out);
    });
}

int hq_worker_set_groups(hq_worker *w, uint64_t n, const hq_worker_group *groups,
                         const hq_member *members, uint64_t *gpu_ns) {
    return guarded(w, "hq_worker_set_groups", [&] {
        if (gpu_ns) *gpu_ns = 0;
        if (n && (!groups || !members)) return w->fail(HQ_E_INVAL, "hq_worker_set_groups: NULL argument");
        if (n > UINT32_MAX) return w->fail(HQ_E_INVAL, "hq_worker_set_groups: a cluster is listed twice");
        if (n == 0) return HQ_OK;
        return w->set_groups(n, groups, members, gpu_ns);
    });
}

int hq_worker_config_changes(hq_worker *w, uint64_t n, const hq_config_change *changes,
                             hq_config_output *out) {
    return guarded(w, "hq_worker_config_changes", [&] {
        if (!out || (n && !changes))
            return w->fail(HQ_E_INVAL, "hq_worker_config_changes: NULL argument");
        if (n > UINT32_MAX) return w->fail(HQ_E_INVAL, "hq_worker_config_changes: a group is listed twice");
        std::memset(out, 0, sizeof *out);
        if (n == 0) return HQ_OK;
        return w->config_changes(n, changes, out);
    });
}

}  // extern "C"
