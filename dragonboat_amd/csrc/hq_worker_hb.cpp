// hq_worker_hb.cpp — leader heartbeats of the step worker (hq_worker_k.h): the compact broadcast
// (hq_worker_heartbeats), the same as MessageBatch bytes per destination
// (hq_worker_heartbeat_batches) with its route column, and hq_heartbeats_expand.
#include "hq_worker_k.h"

using namespace hq::wk;

// ------------------------------------------------------------------------------ heartbeats ---
// Whether `g` sends heartbeats (a leader that is not suspended) and, if so, to whom: every other
// voting member, and the observers too when the heartbeat carries no ctx. Pool order is the node,
// the other voting members, the observers.
bool hq_worker::heartbeat_to(const Group &g, HeartbeatTo &to) const {
    if (g.state != HQ_STATE_LEADER || g.has(kSuspended)) return false;
    to = HeartbeatTo{};
    const ReadQueue *q = reads(g);
    if (q && q->n) {
        to.lo = q->r[q->n - 1].low;
        to.hi = q->r[q->n - 1].high;
    }
    const Member *m = pool.data() + g.mem;
    const uint32_t end = (to.lo | to.hi) == 0 ? g.n_members : g.n_voting;
    for (uint32_t s = 1; s < end; ++s) to.by_order[m[s].order] = m + s;
    return true;
}

// broadcastHeartbeatMessage (raft.go:826-848) for the listed groups. A device worker's state is
// read where it lives (hq_heartbeat.hip); a host worker's here, into the same compact output.
int hq_worker::heartbeats(uint64_t n, const uint32_t *list, hq_heartbeat_output *out) {
    if (dstep) {
        int rc = sync_to_device();
        if (rc) return rc;
        std::memset(out, 0, sizeof *out);
        if (n == 0) return HQ_OK;
        if (!hb && (rc = hq(hq_hb_dev_open(ctx, &hb), "hq_worker_heartbeats"))) return rc;
        hq_dstate_view st;
        hq_dstep_view(dstep, &st);
        uint32_t e = 0;
        rc = hq_hb_dev_run(hb, &st, dev_members, n, list, out, &e);
        if (rc == HQ_E_INVAL && e)
            return e & kHbErrHandle
                       ? fail(HQ_E_INVAL, "hq_worker_heartbeats: unknown group handle")
                       : fail(HQ_E_STATE, "hq_worker_heartbeats: a resident group record is out of "
                                          "range (internal)");
        return hq(rc, "hq_worker_heartbeats");
    }
    for (uint64_t i = 0; i < n; ++i)
        if (int rc = check_listed("hq_worker_heartbeats", list ? list[i] : i)) return rc;
    hb_words.assign(n, 0);
    hb_lags.clear();
    hb_ctxs.clear();
    uint64_t msgs = 0;
    HeartbeatTo to;
    for (uint64_t i = 0; i < n; ++i) {
        const Group &g = groups[list ? list[i] : i];
        if (!heartbeat_to(g, to)) continue;
        uint32_t word = 0;
        for (uint32_t o = 0; o < kDMembers; ++o) {
            if (!to.by_order[o]) continue;
            ++msgs;
            word |= 1u << o;
            if (to.by_order[o]->match < g.committed) {
                word |= 1u << (16 + o);
                hb_lags.push_back({(uint32_t)i, o, to.by_order[o]->match});
            }
        }
        hb_words[i] = word;
        if (word && (to.lo | to.hi) != 0) hb_ctxs.push_back({to.lo, to.hi, (uint32_t)i, 0});
    }
    std::memset(out, 0, sizeof *out);
    out->words = hb_words.data();
    out->n_groups = n;
    out->lags = hb_lags.data();
    out->n_lags = hb_lags.size();
    out->ctxs = hb_ctxs.data();
    out->n_ctxs = hb_ctxs.size();
    out->n_messages = msgs;
    return HQ_OK;
}

// The same heartbeats as MessageBatch bytes, one run of batches per destination. A device worker's
// are marshalled where the state lives (hq_heartbeat_wire.hip); a host worker's here, with the same
// marshaller (hq_heartbeat_wire.h), into the same output.
int hq_worker::heartbeat_batches(uint64_t n, const uint32_t *list, const hq_heartbeat_wire_config *cfg,
                                 hq_heartbeat_batches *out) {
    const char *const bad_route = "hq_worker_heartbeat_batches: a route at or above n_dest";
    routes.resize(groups.size() * kDMembers, (uint16_t)HQ_ROUTE_NONE);
    if (dstep) {
        int rc = sync_to_device();
        if (rc) return rc;
        if (!hbw && (rc = hq(hq_hbw_dev_open(ctx, &hbw), "hq_worker_heartbeat_batches"))) return rc;
        if (routes_on_dev < groups.size()) {            // rows of groups added since
            routes_lo = routes_lo == routes_hi ? routes_on_dev : std::min(routes_lo, routes_on_dev);
            routes_hi = groups.size();
        }
        rc = hq(hq_hbw_dev_put_routes(hbw, routes.data(), groups.size(), routes_lo, routes_hi),
                "hq_worker_heartbeat_batches");
        if (rc) return rc;
        routes_lo = routes_hi = 0;
        routes_on_dev = groups.size();
        if (n == 0) {
            std::memset(out, 0, sizeof *out);
            return HQ_OK;
        }
        hq_dstate_view st;
        hq_dstep_view(dstep, &st);
        uint32_t e = 0;
        hq_heartbeat_batches res;
        rc = hq_hbw_dev_run(hbw, &st, dev_members, n, list, cfg, &res, &e);
        if (rc == HQ_E_INVAL && e)
            return e & kHbErrHandle
                       ? fail(HQ_E_INVAL, "hq_worker_heartbeat_batches: unknown group handle")
                       : e & kHbErrState
                             ? fail(HQ_E_STATE, "hq_worker_heartbeat_batches: a resident group record "
                                                "is out of range (internal)")
                             : fail(HQ_E_INVAL, bad_route);
        if (!rc) *out = res;
        return hq(rc, "hq_worker_heartbeat_batches");
    }
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t h = list ? list[i] : i;
        if (int rc = check_listed("hq_worker_heartbeat_batches", h)) return rc;
        for (uint32_t o = 0; o < groups[h].n_members; ++o) {
            const uint16_t r = routes[h * kDMembers + o];
            if (r != HQ_ROUTE_NONE && r >= cfg->n_dest) return fail(HQ_E_INVAL, bad_route);
        }
    }
    // two passes over the list: the destinations' message counts, then the messages at their
    // places (listed order, then member order within a destination)
    uint64_t unrouted = 0, total = 0;
    HeartbeatTo to;
    hbw_first.assign((size_t)cfg->n_dest + 1, 0);
    for (int write = 0; write < 2; ++write) {
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t h = list ? list[i] : i;
            const Group &g = groups[h];
            if (!heartbeat_to(g, to)) continue;
            for (uint32_t o = 0; o < kDMembers; ++o) {
                if (!to.by_order[o]) continue;
                const uint16_t r = routes[h * kDMembers + o];
                if (r == HQ_ROUTE_NONE) {
                    unrouted += !write;
                } else if (!write) {
                    ++hbw_first[r + 1];
                } else {
                    hbw_msgs[hbw_first[r]++] =
                        hb_fields{to.by_order[o]->node_id, g.node_id, g.cluster_id, g.term,
                                  std::min(to.by_order[o]->match, g.committed), to.lo, to.hi};
                }
            }
        }
        if (!write) {
            for (uint32_t d = 0; d < cfg->n_dest; ++d) hbw_first[d + 1] += hbw_first[d];
            total = hbw_first[cfg->n_dest];
            hbw_msgs.resize(total);
        }
    }
    // (hbw_first[d] is now destination d's end)
    const uint64_t bm = cfg->batch_messages ? cfg->batch_messages : UINT64_MAX;
    const uint32_t trailer = hb_trailer_size(cfg->deployment_id, cfg->source_len);
    hbw_batches.clear();
    uint64_t bytes = 0, j = 0;
    for (uint32_t d = 0; d < cfg->n_dest; ++d) {
        for (const uint64_t end = hbw_first[d]; j < end;) {
            const uint64_t cnt = std::min(bm, end - j);
            uint64_t len = trailer;
            for (uint64_t x = j; x < j + cnt; ++x) len += hb_msg_size(hbw_msgs[x]);
            hbw_batches.push_back({bytes, len, d, (uint32_t)cnt});
            bytes += len;
            j += cnt;
        }
    }
    hbw_bytes.resize(bytes);
    j = 0;
    for (const hq_heartbeat_batch &b : hbw_batches) {
        uint8_t *p = hbw_bytes.data() + b.offset;
        for (uint32_t x = 0; x < b.n_messages; ++x) p = hb_msg_put(p, hbw_msgs[j++]);
        hb_trailer_put(p, cfg->deployment_id, cfg->source, cfg->source_len);
    }
    std::memset(out, 0, sizeof *out);
    out->bytes = hbw_bytes.data();
    out->n_bytes = bytes;
    out->batches = hbw_batches.data();
    out->n_batches = hbw_batches.size();
    out->n_messages = total;
    out->n_unrouted = unrouted;
    return HQ_OK;
}

// hq_heartbeats_expand: the messages of a compact heartbeat output
static int heartbeats_expand(const hq_heartbeat_output *hb, const uint64_t *cluster_id,
                             const uint64_t *term, const uint64_t *committed,
                             const uint32_t *n_members, const uint64_t *member_ids,
                             hq_heartbeat_msg *msgs, uint64_t cap, uint64_t *n) {
    if (!hb || !n) return HQ_E_INVAL;
    const uint64_t G = hb->n_groups;
    if (G && (!hb->words || !cluster_id || !term || !committed || !n_members || !member_ids))
        return HQ_E_INVAL;
    if ((hb->n_lags && !hb->lags) || (hb->n_ctxs && !hb->ctxs)) return HQ_E_INVAL;
    // the checks first (nothing is written for an inconsistent input), then the messages
    for (int write = 0; write < 2; ++write) {
        uint64_t li = 0, ci = 0, k = 0;
        for (uint64_t pos = 0; pos < G; ++pos) {
            const uint32_t w = hb->words[pos], to = w & 0xFFFFu, behind = w >> 16;
            if (!write) {
                if (behind & ~to) return HQ_E_INVAL;
                if (n_members[pos] > kDMembers || (to >> n_members[pos])) return HQ_E_INVAL;
            }
            uint64_t lo = 0, hi = 0;
            if (ci < hb->n_ctxs && hb->ctxs[ci].pos == pos) {
                lo = hb->ctxs[ci].ctx_low;
                hi = hb->ctxs[ci].ctx_high;
                if (!write && (!w || (lo | hi) == 0)) return HQ_E_INVAL;
                ++ci;
            }
            for (uint32_t o = 0; o < kDMembers; ++o) {
                if (!((to >> o) & 1)) continue;
                uint64_t commit = committed[pos];
                if ((behind >> o) & 1) {
                    if (li >= hb->n_lags || hb->lags[li].pos != pos || hb->lags[li].member != o)
                        return HQ_E_INVAL;
                    commit = hb->lags[li++].match;
                }
                if (write)
                    msgs[k] = hq_heartbeat_msg{cluster_id[pos], member_ids[pos * kDMembers + o],
                                               term[pos], commit, lo, hi};
                ++k;
            }
        }
        if (!write) {
            // (records left over: out of order, for a position outside the list, or without a bit)
            if (li != hb->n_lags || ci != hb->n_ctxs || k != hb->n_messages) return HQ_E_INVAL;
            *n = k;
            if (k > cap || (k && !msgs)) return HQ_E_STATE;
        }
    }
    return HQ_OK;
}

// ------------------------------------------------------------------------------ C-ABI ------
extern "C" {

int hq_worker_set_heartbeat_routes(hq_worker *w, uint32_t first_handle, uint64_t n_groups,
                                   const uint16_t *routes) {
    return guarded(w, "hq_worker_set_heartbeat_routes", [&] {
        if (n_groups && !routes)
            return w->fail(HQ_E_INVAL, "hq_worker_set_heartbeat_routes: routes is NULL");
        if (first_handle > w->groups.size() || n_groups > w->groups.size() - first_handle)
            return w->fail(HQ_E_INVAL, "hq_worker_set_heartbeat_routes: unknown group handle");
        if (!n_groups) return HQ_OK;
        w->routes.resize(w->groups.size() * kDMembers, (uint16_t)HQ_ROUTE_NONE);
        std::memcpy(w->routes.data() + (size_t)first_handle * kDMembers, routes,
                    n_groups * kDMembers * sizeof(uint16_t));
        const uint64_t lo = first_handle, hi = first_handle + n_groups;
        if (w->routes_lo == w->routes_hi) {
            w->routes_lo = lo;
            w->routes_hi = hi;
        } else {
            w->routes_lo = std::min(w->routes_lo, lo);
            w->routes_hi = std::max(w->routes_hi, hi);
        }
        return HQ_OK;
    });
}

int hq_worker_heartbeat_batches(hq_worker *w, uint64_t n_groups, const uint32_t *groups,
                                const hq_heartbeat_wire_config *cfg, hq_heartbeat_batches *out) {
    return guarded(w, "hq_worker_heartbeat_batches", [&] {
        if (!cfg || !out) return w->fail(HQ_E_INVAL, "hq_worker_heartbeat_batches: cfg or out is NULL");
        if (cfg->n_dest < 1 || cfg->n_dest > 65535)
            return w->fail(HQ_E_INVAL, "hq_worker_heartbeat_batches: n_dest must be 1 .. 65535");
        if (cfg->source_len > kHbSourceMax || (cfg->source_len && !cfg->source))
            return w->fail(HQ_E_INVAL, "hq_worker_heartbeat_batches: a source of more than 256 bytes "
                                       "(or NULL)");
        if (n_groups >= (uint64_t(1) << 28))
            return w->fail(HQ_E_INVAL, "hq_worker_heartbeat_batches: 2^28 or more groups in one call");
        if (!groups && n_groups > w->groups.size())
            return w->fail(HQ_E_INVAL, "hq_worker_heartbeat_batches: unknown group handle");
        return w->heartbeat_batches(n_groups, groups, cfg, out);
    });
}

int hq_worker_heartbeats(hq_worker *w, uint64_t n_groups, const uint32_t *groups,
                         hq_heartbeat_output *out) {
    return guarded(w, "hq_worker_heartbeats", [&] {
        if (!out) return w->fail(HQ_E_INVAL, "hq_worker_heartbeats: out is NULL");
        if (n_groups >= (uint64_t(1) << 28))
            return w->fail(HQ_E_INVAL, "hq_worker_heartbeats: 2^28 or more groups in one call");
        if (!groups && n_groups > w->groups.size())
            return w->fail(HQ_E_INVAL, "hq_worker_heartbeats: unknown group handle");
        return w->heartbeats(n_groups, groups, out);
    });
}

int hq_heartbeats_expand(const hq_heartbeat_output *hb, const uint64_t *cluster_id,
                         const uint64_t *term, const uint64_t *committed, const uint32_t *n_members,
                         const uint64_t *member_ids, hq_heartbeat_msg *msgs, uint64_t cap,
                         uint64_t *n) {
    // (no worker: nowhere to keep a message)
    return hq::guard("hq_heartbeats_expand", [&] {
        return heartbeats_expand(hb, cluster_id, term, committed, n_members, member_ids, msgs, cap, n);
    });
}

}  // extern "C"
