// hq_worker_tick.cpp — the Raft timers of the step worker (hq_worker_k.h; include/hipquorum.h "raft
// timers"): the tick config, one tick of every group with its three due lists, and the listed
// timers' get / set, host and device arms. The transition is hq_tick.h's for both: a host worker
// applies it to its own records here, a device worker's kernels (hq_tick.hip) to the resident ones.
// None of the calls reads the device state back or touches host_stale: which handles are live is
// the mirror's own structure, and (term, state) are read where they live. The contacts that
// hq_worker_heartbeats_received marked since the last tick (hq_worker_hbrecv.cpp; a device worker's
// in hq_hb_received.hip's device bitmap) are a second contact set of the tick, consumed by it.
#include "hq_worker_k.h"

using namespace hq::wk;

// The hook of the calls that start or re-sync a handle (hq_worker_set_group(s),
// hq_worker_start_groups): its timer comes back reset at the next tick, get or set. A host
// worker's timer is marked at once; a device worker's handle is remembered until tick_flush.
void hq_worker::tick_touch(uint32_t h) {
    if (!tick_on) return;                           // (a config resets every timer anyway)
    if (!dstep) {
        if (h < timers.size()) timers[h] = tick_unseen();
        return;
    }
    if (tick_reset_all) return;
    if (tick_resets.size() > groups.size() + 1024) {   // (a caller that never ticks: one entry per handle)
        std::sort(tick_resets.begin(), tick_resets.end());
        tick_resets.erase(std::unique(tick_resets.begin(), tick_resets.end()), tick_resets.end());
    }
    tick_resets.push_back(h);
}

// A timer for every handle, and the remembered resets applied: before anything reads the timers.
int hq_worker::tick_flush(const char *entry) {
    if (!dstep) {
        timers.resize(groups.size(), tick_unseen());
        return HQ_OK;
    }
    int rc = HQ_OK;
    if (!tickd && (rc = hq(hq_tick_dev_open(ctx, &tickd), entry))) return rc;
    rc = hq(hq_tick_dev_invalidate(tickd, groups.size(), tick_reset_all, tick_reset_all ? 0 : tick_resets.size(),
                                   tick_resets.data()), entry);
    if (rc) return rc;
    tick_reset_all = false;
    tick_resets.clear();
    return HQ_OK;
}

int hq_worker::set_tick_config(const hq_tick_config *cfg) {
    if (cfg->election_rtt < 1 || cfg->election_rtt > 32767)
        return fail(HQ_E_INVAL, "hq_worker_set_tick_config: election_rtt must be 1 .. 32767");
    if (cfg->heartbeat_rtt < 1 || cfg->heartbeat_rtt > 65535)
        return fail(HQ_E_INVAL, "hq_worker_set_tick_config: heartbeat_rtt must be 1 .. 65535");
    if (cfg->check_quorum > 1 || cfg->reserved)
        return fail(HQ_E_INVAL, "hq_worker_set_tick_config: check_quorum must be 0 or 1, reserved 0");
    tick_p = hq_tick_params{cfg->election_rtt, cfg->heartbeat_rtt, cfg->check_quorum, cfg->seed};
    tick_on = true;
    if (int rc = clear_pending_contacts()) return rc;   // (of received heartbeats)
    // every timer reset
    if (dstep) {
        tick_reset_all = true;
        tick_resets.clear();
    } else {
        timers.assign(groups.size(), tick_unseen());
    }
    return HQ_OK;
}

int hq_worker::tick(uint64_t n_contact, const uint32_t *contact, hq_tick_output *out) {
    const char *const entry = "hq_worker_tick";
    if (!tick_on) return fail(HQ_E_STATE, "hq_worker_tick: no tick config (hq_worker_set_tick_config)");
    // the whole contact list is checked before anything is ticked
    for (uint64_t i = 0; i < n_contact; ++i)
        if (!live(contact[i])) return fail(HQ_E_INVAL, "hq_worker_tick: unknown group handle in the contact list");
    const uint64_t G = groups.size();
    if (dstep) {
        int rc = sync_to_device();                  // pending add / set_group first, as a step does
        if (rc) return rc;
        if ((rc = tick_flush(entry))) return rc;
        uint32_t *bitmap = nullptr;
        if (n_contact) {
            if ((rc = hq(hq_tick_dev_contact(tickd, G, &bitmap), entry))) return rc;
            for (uint64_t i = 0; i < n_contact; ++i) bitmap[contact[i] >> 5] |= 1u << (contact[i] & 31u);
        }
        hq_dstate_view st;
        hq_dstep_view(dstep, &st);
        if (st.n_groups != G) return fail(HQ_E_STATE, "hq_worker_tick: the resident state is not the host's size (internal)");
        // the contacts hq_worker_heartbeats_received marked on the device since the last tick
        uint32_t *pending = nullptr;
        if (hbr && (rc = hq(hq_hbr_dev_pending(hbr, G, &pending), entry))) return rc;
        rc = hq(hq_tick_dev_run(tickd, &st, &tick_p, n_contact != 0, pending, out), entry);
        if (!rc && pending) hq_hbr_dev_consumed(hbr);
        return rc;
    }
    tick_flush(entry);
    tk_contact.assign((G + 31) / 32, 0);
    if (hr_marked) {                                // the received heartbeats' contacts, consumed
        for (size_t i = 0; i < std::min(tk_contact.size(), hr_pending.size()); ++i) tk_contact[i] = hr_pending[i];
        clear_pending_contacts();
    }
    for (uint64_t i = 0; i < n_contact; ++i) tk_contact[contact[i] >> 5] |= 1u << (contact[i] & 31u);
    for (auto &l : tk_lists) l.clear();
    uint64_t ticked = 0;
    for (uint64_t h = 0; h < G; ++h) {
        const Group &g = groups[h];
        const bool listed = (tk_contact[h >> 5] >> (h & 31u)) & 1u;
        const uint32_t bits = tick_step(timers[h], tick_p, g.cluster_id, g.term, g.state, g.has(kSuspended), listed);
        for (uint32_t c = 0; c < kTickLists; ++c)
            if ((bits >> c) & 1u) tk_lists[c].push_back((uint32_t)h);
        ticked += (bits & kTickTicked) != 0;
    }
    out->check_quorum = tk_lists[0].data();
    out->n_check_quorum = tk_lists[0].size();
    out->heartbeat = tk_lists[1].data();
    out->n_heartbeat = tk_lists[1].size();
    out->election = tk_lists[2].data();
    out->n_election = tk_lists[2].size();
    out->n_ticked = ticked;
    return HQ_OK;
}

int hq_worker::get_timers(uint64_t n, const uint32_t *handles, hq_timer *out) {
    const char *const entry = "hq_worker_get_timers";
    const uint64_t G = groups.size();
    if (!tick_on) return fail(HQ_E_STATE, "hq_worker_get_timers: no tick config (hq_worker_set_tick_config)");
    for (uint64_t i = 0; i < n; ++i)
        if (!live(handles ? handles[i] : i)) return fail(HQ_E_INVAL, "hq_worker_get_timers: unknown group handle");
    if (dstep) {
        int rc = sync_to_device();                  // pending add / set_group first, as a step does
        if (rc) return rc;
        if ((rc = tick_flush(entry))) return rc;
        hq_dstate_view st;
        hq_dstep_view(dstep, &st);
        uint32_t e = 0;
        uint32_t *pending = nullptr;
        if (hbr && (rc = hq(hq_hbr_dev_pending(hbr, G, &pending), entry))) return rc;
        rc = hq_tick_dev_get(tickd, &st, &tick_p, n, handles, out, pending, &e);
        if (rc == HQ_E_INVAL && e)
            return fail(HQ_E_STATE, "hq_worker_get_timers: a live handle beyond the resident state (internal)");
        return hq(rc, entry);
    }
    tick_flush(entry);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t h = handles ? handles[i] : i;
        const Group &g = groups[h];
        out[i] = tick_public(timers[h], tick_p, g.cluster_id, g.term, g.state);
        if (contact_pending(h) && g.state != HQ_STATE_LEADER) out[i].election_tick = 0;
    }
    return HQ_OK;
}

int hq_worker::set_timers(uint64_t n, const uint32_t *handles, const hq_timer *ts) {
    const char *const entry = "hq_worker_set_timers";
    const uint64_t G = groups.size();
    if (!tick_on) return fail(HQ_E_STATE, "hq_worker_set_timers: no tick config (hq_worker_set_tick_config)");
    // every entry is checked before any is applied
    int rc = check_distinct(
        n, "hq_worker_set_timers: a group is listed twice",
        [&](uint64_t i, uint32_t &h) {
            const uint64_t at = handles ? handles[i] : i;
            if (!live(at)) return fail(HQ_E_INVAL, "hq_worker_set_timers: unknown group handle");
            h = (uint32_t)at;
            return HQ_OK;
        },
        [&](uint64_t i, uint32_t) {
            return tick_settable(ts[i], tick_p)
                       ? HQ_OK
                       : fail(HQ_E_INVAL, "hq_worker_set_timers: a counter beyond its limit, or a "
                                          "randomized_timeout outside [election_rtt, 2 election_rtt)");
        });
    if (rc) return rc;
    if (dstep) {
        if ((rc = sync_to_device())) return rc;     // pending add / set_group first, as a step does
        if ((rc = tick_flush(entry))) return rc;
        hq_dstate_view st;
        hq_dstep_view(dstep, &st);
        uint32_t e = 0;
        uint32_t *pending = nullptr;
        if (hbr && (rc = hq(hq_hbr_dev_pending(hbr, G, &pending), entry))) return rc;
        rc = hq_tick_dev_set(tickd, &st, &tick_p, n, handles, ts, pending, &e);
        if (rc == HQ_E_INVAL && e)
            return fail(HQ_E_STATE, "hq_worker_set_timers: a live handle beyond the resident state (internal)");
        return hq(rc, entry);
    }
    tick_flush(entry);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t h = handles ? handles[i] : i;
        const Group &g = groups[h];
        timers[h] = tick_from_public(ts[i], tick_p, g.cluster_id, g.term, g.state);
        if (contact_pending(h)) hr_pending[h >> 5] &= ~(1u << (h & 31u));
    }
    return HQ_OK;
}

// ------------------------------------------------------------------------------ C-ABI ------
extern "C" {

int hq_worker_set_tick_config(hq_worker *w, const hq_tick_config *cfg) {
    return guarded(w, "hq_worker_set_tick_config", [&] {
        if (!cfg) return w->fail(HQ_E_INVAL, "hq_worker_set_tick_config: NULL argument");
        return w->set_tick_config(cfg);
    });
}

int hq_worker_tick(hq_worker *w, uint64_t n_contact, const uint32_t *contact, hq_tick_output *out) {
    return guarded(w, "hq_worker_tick", [&] {
        if (!out || (n_contact && !contact)) return w->fail(HQ_E_INVAL, "hq_worker_tick: NULL argument");
        std::memset(out, 0, sizeof *out);
        return w->tick(n_contact, contact, out);
    });
}

int hq_tick_timeout(uint64_t seed, uint64_t cluster_id, uint64_t term, uint32_t state,
                    uint32_t election_rtt) {
    if (election_rtt < 1 || election_rtt > 32767) return 0;
    return (int)tick_draw(seed, cluster_id, term, state, election_rtt);
}

int hq_worker_get_timers(hq_worker *w, uint64_t n, const uint32_t *handles, hq_timer *out) {
    return guarded(w, "hq_worker_get_timers", [&] {
        if (n && !out) return w->fail(HQ_E_INVAL, "hq_worker_get_timers: NULL argument");
        if (n > UINT32_MAX) return w->fail(HQ_E_INVAL, "hq_worker_get_timers: too many groups listed");
        if (n == 0) return HQ_OK;
        return w->get_timers(n, handles, out);
    });
}

int hq_worker_set_timers(hq_worker *w, uint64_t n, const uint32_t *handles, const hq_timer *timers) {
    return guarded(w, "hq_worker_set_timers", [&] {
        if (n && !timers) return w->fail(HQ_E_INVAL, "hq_worker_set_timers: NULL argument");
        if (n > UINT32_MAX) return w->fail(HQ_E_INVAL, "hq_worker_set_timers: a group is listed twice");
        if (n == 0) return HQ_OK;
        return w->set_timers(n, handles, timers);
    });
}

}  // extern "C"
