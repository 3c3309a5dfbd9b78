// hq_worker_hbrecv.cpp — the follower side of heartbeats on the step worker (hq_worker_k.h;
// include/hipquorum.h "heartbeats received"): a step interval's received Heartbeats handled where
// the state lives, host and device arms, and the replies expanded to wire messages. The
// per-message transition is hq_hb_received.h's for both: a host worker applies it to its own
// records here, a device worker's kernel (hq_hb_received.hip) to the resident ones. The contacts
// are kept per handle for the next hq_worker_tick (hq_worker_tick.cpp), on the device for a device
// worker: they never pass through the host. Nothing reads the device state back.
#include "hq_worker_k.h"

using namespace hq::wk;

int hq_worker::clear_pending_contacts() {
    if (dstep) return hbr ? hq(hq_hbr_dev_clear(hbr), "hq_worker_heartbeats_received contacts") : HQ_OK;
    if (hr_marked) std::fill(hr_pending.begin(), hr_pending.end(), 0u);
    hr_marked = false;
    return HQ_OK;
}

int hq_worker::heartbeats_received(const hq_hb_received_input *in, hq_hb_received_output *out) {
    const char *const entry = "hq_worker_heartbeats_received";
    const uint64_t n = in->n_groups, G = groups.size();
    // everything is checked before anything is handled
    if (in->check_quorum > 1 || in->reserved)
        return fail(HQ_E_INVAL, "hq_worker_heartbeats_received: check_quorum must be 0 or 1, reserved 0");
    if (n >= (1ull << 28)) return fail(HQ_E_INVAL, "hq_worker_heartbeats_received: too many groups listed");
    if (n == 0) {
        std::memset(out, 0, sizeof *out);
        return HQ_OK;
    }
    if (!in->groups || !in->offsets) return fail(HQ_E_INVAL, "hq_worker_heartbeats_received: NULL groups/offsets");
    if (in->offsets[0] != 0) return fail(HQ_E_INVAL, "hq_worker_heartbeats_received: offsets do not start at 0");
    for (uint64_t i = 0; i < n; ++i)
        if (in->offsets[i + 1] < in->offsets[i])
            return fail(HQ_E_INVAL, "hq_worker_heartbeats_received: offsets decrease");
    const uint64_t n_msgs = in->offsets[n];
    if (n_msgs >= (1ull << 31)) return fail(HQ_E_INVAL, "hq_worker_heartbeats_received: too many messages");
    if (n_msgs && !in->msgs) return fail(HQ_E_INVAL, "hq_worker_heartbeats_received: NULL msgs");
    // The handles against the mirror's structure (its size: a vacant handle is a suspended group
    // here, not an unknown one: its tombstone answers), and each at most once. Seen handles are
    // marked in a bitmap of G bits, not in the group records: 128 KiB at 2^20 handles stay in
    // cache where a pass over the records misses once per handle.
    hr_seen.assign((G + 31) / 32, 0u);
    int rc = HQ_OK;
    for (uint64_t i = 0; i < n && !rc; ++i) {
        const uint32_t h = in->groups[i], bit = 1u << (h & 31u);
        if (h >= G) rc = fail(HQ_E_INVAL, "hq_worker_heartbeats_received: unknown group handle");
        else if (hr_seen[h >> 5] & bit) rc = fail(HQ_E_INVAL, "hq_worker_heartbeats_received: a group is listed twice");
        else hr_seen[h >> 5] |= bit;
    }
    if (rc) return rc;

    if (dstep) {
        if ((rc = sync_to_device())) return rc;     // pending add / set_group first, as a step does
        if (!hbr && (rc = hq(hq_hbr_dev_open(ctx, &hbr), entry))) return rc;
        hq_dstate_mut st;
        hq_dstep_view_mut(dstep, &st);
        if (st.n_groups != G)
            return fail(HQ_E_STATE, "hq_worker_heartbeats_received: the resident state is not the host's size (internal)");
        host_stale = true;                          // the device copy is the authoritative one, as after a step
        hq_hb_received_output res{};
        if ((rc = hq(hq_hbr_dev_run(hbr, &st, dev_members, in, &res), entry))) return rc;
        *out = res;
        return HQ_OK;
    }

    hr_replies.assign(n_msgs, hq_hb_reply{0, 0, 0});
    hr_results.resize(n);
    if (hr_pending.size() < (G + 31) / 32) hr_pending.resize((G + 31) / 32, 0u);
    hq_hb_received_output res{};
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t h = in->groups[i];
        Group &gr = groups[h];
        hq_hbr_group g{gr.term, gr.committed, gr.last, gr.state, false};
        hq_hbr_acc a{0, 0, 0, 0};
        if (gr.has(kSuspended)) {
            a.flags = HQ_HBR_SUSPENDED;
        } else {
            for (uint64_t m = in->offsets[i]; m < in->offsets[i + 1]; ++m) {
                const uint32_t type = hbr_message(g, a, in->msgs[m], in->check_quorum);
                hr_replies[m] = hq_hb_reply{type ? g.term : 0, type, 0};
                res.n_resp += type == HQ_MSG_HEARTBEAT_RESP;
                res.n_noop += type == HQ_MSG_NOOP;
            }
            // becomeFollower's bookkeeping is the step's (reset), without a step's outputs; a
            // group's resets collapse into one: the last term, the same cleared fields
            if (g.reset) {
                gr.state = HQ_STATE_FOLLOWER;
                reset(gr, g.term);
            }
            gr.committed = g.committed;
            if (a.flags & HQ_HBR_CONTACT) {
                hr_pending[h >> 5] |= 1u << (h & 31u);
                hr_marked = true;
            }
        }
        hr_results[i] = hq_hb_group_result{g.term, a.commit, a.leader, g.state, (uint16_t)a.flags, (uint16_t)a.n_resets};
        res.n_contact += (a.flags & HQ_HBR_CONTACT) != 0;
        res.n_committed += (a.flags & HQ_HBR_COMMITTED) != 0;
        res.n_state_changed += a.n_resets != 0;
        res.n_suspended += (a.flags & HQ_HBR_SUSPENDED) != 0;
    }
    res.replies = hr_replies.data();
    res.n_msgs = n_msgs;
    res.results = hr_results.data();
    res.n_groups = n;
    *out = res;
    return HQ_OK;
}

// ------------------------------------------------------------------------------ C-ABI ------
extern "C" {

int hq_worker_heartbeats_received(hq_worker *w, const hq_hb_received_input *in, hq_hb_received_output *out) {
    return guarded(w, "hq_worker_heartbeats_received", [&] {
        if (!in || !out) return w->fail(HQ_E_INVAL, "hq_worker_heartbeats_received: NULL argument");
        return w->heartbeats_received(in, out);
    });
}

int hq_heartbeat_replies_expand(const hq_hb_received_input *in, const hq_hb_received_output *out,
                                const uint64_t *cluster_id, const uint64_t *node_id, hq_wire_message *msgs,
                                uint64_t cap, uint64_t *n) {
    if (n) *n = 0;
    return hq::guard("hq_heartbeat_replies_expand", [&]() -> int {
        if (!in || !out || !n) return HQ_E_INVAL;
        const uint64_t G = in->n_groups;
        if (G != out->n_groups || G >= (1ull << 28)) return HQ_E_INVAL;
        if (G == 0) return HQ_OK;
        if (!in->offsets || in->offsets[0] != 0 || in->offsets[G] != out->n_msgs || out->n_msgs >= (1ull << 31))
            return HQ_E_INVAL;
        for (uint64_t i = 0; i < G; ++i)
            if (in->offsets[i + 1] < in->offsets[i]) return HQ_E_INVAL;
        if (out->n_msgs && (!in->msgs || !out->replies || !cluster_id || !node_id)) return HQ_E_INVAL;
        uint64_t count = 0;
        for (uint64_t m = 0; m < out->n_msgs; ++m) {
            const uint32_t t = out->replies[m].type;
            if (t != 0 && t != HQ_MSG_HEARTBEAT_RESP && t != HQ_MSG_NOOP) return HQ_E_INVAL;
            count += t != 0;
        }
        *n = count;
        if (count > cap) return HQ_E_STATE;
        if (count && !msgs) return HQ_E_INVAL;
        uint64_t at = 0;
        for (uint64_t i = 0; i < G; ++i)
            for (uint64_t m = in->offsets[i]; m < in->offsets[i + 1]; ++m) {
                const hq_hb_reply &r = out->replies[m];
                if (!r.type) continue;
                hq_wire_message w{};
                w.ev.kind = HQ_EV_MESSAGE;
                w.ev.type = r.type;
                w.ev.from = node_id[i];
                w.ev.term = r.term;
                if (r.type == HQ_MSG_HEARTBEAT_RESP) {
                    w.ev.hint = in->msgs[m].hint;
                    w.ev.hint_high = in->msgs[m].hint_high;
                }
                w.cluster_id = cluster_id[i];
                w.to = in->msgs[m].from;
                msgs[at++] = w;
            }
        return HQ_OK;
    });
}

}  // extern "C"
