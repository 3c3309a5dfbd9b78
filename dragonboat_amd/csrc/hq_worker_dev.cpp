// hq_worker_dev.cpp — the device worker (hq_worker_k.h; HQ_WORKER_ON_DEVICE): the host records as
// a mirror of the state resident on the GPU (hq_dstep*.hip), a step as one launch sequence there,
// and the step entry points of both workers.
#include "hq_worker_k.h"

using namespace hq::wk;

// ------------------------------------------------------------------------------ device mode ---
// A group's device form: its record, its kDReads reads and, with `m`, its members in pool order.
void hq_worker::to_device_record(const Group &g, hq_dgroup &d, hq_dread *r, hq_dmember *m) const {
    for (uint32_t i = 0; m && i < g.n_members; ++i) m[i] = to_device_member(pool[g.mem + i]);
    d = hq_dgroup{};
    d.cluster_id = g.cluster_id;
    d.node_id = g.node_id;
    d.term = g.term;
    d.committed = g.committed;
    d.last = g.last;
    d.term_start = g.term_start;
    d.mem = g.mem;
    d.n_members = g.n_members;
    d.n_voting = g.n_voting;
    d.state = g.state;
    d.granted = g.granted;
    d.rejected = g.rejected;
    d.flags = g.has(kSuspended) ? kDSuspended : 0;
    const ReadQueue *q = reads(g);
    d.n_reads = q ? (uint8_t)q->n : 0;
    for (uint32_t k = 0; k < kDReads; ++k) {
        r[k] = hq_dread{};
        if (q && k < q->n) {
            const ReadStatus &s = q->r[k];
            r[k].index = s.index;
            r[k].from = s.from;
            r[k].low = s.low;
            r[k].high = s.high;
            uint8_t c = s.confirmed;
            for (uint32_t v = 0; v < HQ_MAX_VOTERS; ++v)
                if (s.ord[v] != kNoAck) c |= (uint8_t)(1u << v);
            r[k].confirmed = c;
        }
    }
}

// new groups (and their members) in one upload; groups changed by set_group one by one
int hq_worker::sync_to_device() {
    const uint64_t G = groups.size();
    if (dev_groups < G || dev_members < pool.size()) {
        const uint64_t ng = G - dev_groups, nm = pool.size() - dev_members;
        std::vector<hq_dgroup> dg(ng);
        std::vector<hq_dread> dr(ng * kDReads);
        for (uint64_t i = 0; i < ng; ++i)
            to_device_record(groups[dev_groups + i], dg[i], dr.data() + i * kDReads);
        std::vector<hq_dmember> dm(nm);
        for (uint64_t i = 0; i < nm; ++i) dm[i] = to_device_member(pool[dev_members + i]);
        int rc = hq(hq_dstep_put(dstep, dev_groups, ng, dg.data(), dr.data(), dev_members, nm,
                                 dm.data()), "hq_dstep_put");
        if (rc) return rc;
        dev_groups = G;
        dev_members = pool.size();
    }
    for (uint32_t h : dirty) {
        const Group &g = groups[h];
        hq_dgroup dg;
        hq_dread dr[kDReads];
        hq_dmember dm[kDMembers];                   // (check_group: no more on a device worker)
        to_device_record(g, dg, dr, dm);
        int rc = hq(hq_dstep_put(dstep, h, 1, &dg, dr, g.mem, g.n_members, dm), "hq_dstep_put");
        if (rc) return rc;
    }
    dirty.clear();
    return HQ_OK;
}

// the whole device state back into the host records
int hq_worker::sync_from_device() {
    if (!host_stale) return HQ_OK;
    ++readbacks;
    const uint64_t G = dev_groups, M = dev_members;
    std::vector<hq_dgroup> dg(G);
    std::vector<hq_dread> dr(G * kDReads);
    std::vector<hq_dmember> dm(M);
    int rc = hq(hq_dstep_get(dstep, G, dg.data(), dr.data(), M, dm.data()), "hq_dstep_get");
    if (rc) return rc;
    for (uint64_t h = 0; h < G; ++h) {
        Group &g = groups[h];
        const hq_dgroup &d = dg[h];
        g.term = d.term;
        g.committed = d.committed;
        g.last = d.last;
        g.term_start = d.term_start;
        g.state = d.state;
        g.granted = d.granted;
        g.rejected = d.rejected;
        if (d.flags & kDSuspended) g.set(kSuspended);
        else g.clear(kSuspended);
        if (d.n_reads == 0) {
            rq_release(g);
        } else {
            if (g.rq == kNone) g.rq = rq_alloc();
            ReadQueue &q = rqs[g.rq];
            q.n = d.n_reads;
            for (uint32_t k = 0; k < q.n; ++k) {
                const hq_dread &r = dr[h * kDReads + k];
                ReadStatus &s = q.r[k];
                s.index = r.index;
                s.from = r.from;
                s.low = r.low;
                s.high = r.high;
                s.confirmed = r.confirmed;
                std::fill(std::begin(s.ord), std::end(s.ord), kNoAck);
            }
        }
    }
    for (uint64_t i = 0; i < M; ++i) {
        pool[i].match = dm[i].match;
        pool[i].active = dm[i].active;
    }
    host_stale = false;
    return HQ_OK;
}

int hq_worker::step_on_device(const hq_dstep_in &inp, hq_step_output *out) {
    const uint64_t t0 = now_ns();
    // the per-group input checks (handles, offsets, a group listed twice) run in the engine's
    // first kernel, which writes each group's new state in place; a failed step takes that state
    // back (k_step_restore). The device copy is the authoritative one from here on, whatever the
    // outcome: the host copy is reloaded from it before the host reads a group.
    int rc = sync_to_device();
    if (rc) return rc;
    const uint64_t t1 = now_ns();
    host_stale = true;
    rc = hq_dstep_run(dstep, &inp, &dout);
    return device_step_done(rc, inp, out, t0, t1);
}

// the outputs of a device step (hq_dstep_run or hq_dstep_run_jobs) in the worker's terms
int hq_worker::device_step_done(int rc, const hq_dstep_in &inp, hq_step_output *out, uint64_t t0,
                                uint64_t t1) {
    if (rc == HQ_E_INVAL && dout.input_error) {
        const uint32_t e = dout.input_error;
        if (e & (16 | 32))        // (hq_dstep_k.h kErrScan / kErrTicket: not the input's fault)
            return fail(HQ_E_STATE, "hq_worker_step: the device step's scan of the ReadyToRead "
                                    "places or its launch order failed (internal); no group "
                                    "state was written");
        return fail(HQ_E_INVAL, e & 1 ? "hq_worker_step: unknown group handle"
                                : e & 8 ? "hq_worker_step: a group is listed twice"
                                : e & 2 ? "hq_worker_step: offsets decrease"
                                        : "hq_worker_step_stream: boffsets decrease or out of range, sizes "
                                          "not summing to the totals, or a group's bytes not used up by its "
                                          "events (malformed event stream)");
    }
    rc = hq(rc, "hq_dstep_run");
    if (rc) return rc;
    const uint64_t t2 = now_ns();
    out->commits = dout.commits;
    out->n_commits = dout.n_commits;
    out->committed_column = dout.commit_col;
    out->committed_advance = dout.commit_adv;
    out->ready = dout.ready;
    out->ready_compact = dout.ready_compact;
    out->n_ready = dout.n_ready;
    out->read_resps = dout.resps;
    out->n_read_resps = dout.n_resps;
    out->state_changes = dout.states;
    out->n_state_changes = dout.n_states;
    out->dropped_reads = dout.dropped;
    out->n_dropped_reads = dout.n_dropped;
    out->deferred = dout.deferred;
    out->n_deferred = dout.n_deferred;
    out->fallback_groups = dout.fallback;
    out->n_fallback_groups = dout.n_fallback;
    out->gpu_passes = inp.n ? 1 : 0;
    out->decisions = dout.decisions;
    out->ready_slots = dout.ready_slots;
    out->ready_slot_counts = dout.slot_counts;
    out->n_ready_tiles = dout.n_tiles;
    out->n_ready_slotted = dout.n_slotted;
    // (device path: pack = the host's submit, device = the thread's wait for the device, apply =
    // the outputs mapped after the wait, gpu = the GPU's time between the step's events)
    out->pass_ns = t2 - t1;
    out->pack_ns = dout.submit_ns;
    out->device_ns = dout.wait.t_end_ns > dout.wait.t_begin_ns
                         ? dout.wait.t_end_ns - dout.wait.t_begin_ns : 0;
    out->apply_ns = dout.d2h_ns;
    out->handle_ns = t1 - t0;
    out->gpu_ns = dout.gpu_ns;
    out->gpu_jobs = dout.gpu_jobs;
    out->wait_sleeps = (uint32_t)dout.wait.sleeps;
    out->wait_poll_ns = dout.wait.poll_ns;
    out->wait_sleep_ns = dout.wait.sleep_ns;
    out->wait_end_ns = dout.wait.t_end_ns;
    out->device_end_ticks = dout.wait.device_end_ticks;
    out->device_start_ticks = dout.wait.device_start_ticks;
    return HQ_OK;
}

namespace {

const uint8_t kNoBytes = 0;               // an empty stream's bytes: never NULL for the engine

// a sized event stream as the device engine takes it
hq_dstep_in sized_dstep_in(const hq_step_stream &in) {
    hq_dstep_in d{in.n_groups, in.groups, nullptr, nullptr, nullptr, in.bytes ? in.bytes : &kNoBytes};
    d.sizes = in.sizes16 ? nullptr : in.sizes;
    d.sizes16 = in.sizes16;
    d.n_events = in.n_events;
    d.n_bytes = in.n_bytes;
    return d;
}

}  // namespace

// hq_worker_step_stream: both forms of the stream, on either worker
int hq_worker::step_stream(const hq_step_stream *in, hq_step_output *out) {
    if (!in || !out) return fail(HQ_E_INVAL, "hq_worker_step_stream: NULL argument");
    if (in->sizes || in->sizes16 || (in->n_groups && !in->offsets && !in->boffsets)) {
        // the sized form: the device engine scans the sizes; a host worker (or a check) makes
        // the prefix arrays here
        if (in->n_groups && !in->sizes && !in->sizes16)
            return fail(HQ_E_INVAL, "hq_worker_step_stream: NULL sizes");
        if (in->n_bytes && !in->bytes) return fail(HQ_E_INVAL, "hq_worker_step_stream: NULL bytes");
        std::memset(out, 0, sizeof *out);
        if (dstep) return step_on_device(sized_dstep_in(*in), out);
        const uint32_t *list = in->groups;
        if (!list) {                      // the step lists handles 0 .. n_groups - 1
            sized_groups.resize(in->n_groups);
            for (uint64_t i = 0; i < in->n_groups; ++i) sized_groups[i] = (uint32_t)i;
            list = sized_groups.data();
        }
        sized_off.resize(in->n_groups + 1);
        sized_boff.resize(in->n_groups + 1);
        sized_off[0] = sized_boff[0] = 0;
        if (in->sizes16) {        // bytes only: the events counted from the bytes
            for (uint64_t i = 0; i < in->n_groups; ++i)
                sized_boff[i + 1] = sized_boff[i] + in->sizes16[i];
            if (sized_boff[in->n_groups] != in->n_bytes)
                return fail(HQ_E_INVAL, "hq_worker_step_stream: sizes do not sum to the totals");
            if (hq_events_count(in->n_groups, sized_boff.data(), in->bytes ? in->bytes : &kNoBytes,
                                sized_off.data()) != HQ_OK)
                return fail(HQ_E_INVAL, "hq_worker_step_stream: malformed event stream");
        } else {
            for (uint64_t i = 0; i < in->n_groups; ++i) {
                sized_off[i + 1] = sized_off[i] + (in->sizes[i] & 0xFFFFu);
                sized_boff[i + 1] = sized_boff[i] + (in->sizes[i] >> 16);
            }
        }
        if (sized_off[in->n_groups] != in->n_events || sized_boff[in->n_groups] != in->n_bytes)
            return fail(HQ_E_INVAL, "hq_worker_step_stream: sizes do not sum to the totals");
        const hq_step_stream full{in->n_groups, list, sized_off.data(), sized_boff.data(),
                                  in->bytes ? in->bytes : &kNoBytes, nullptr, 0, 0, nullptr};
        return step_stream(&full, out);
    }
    if (in->n_groups && (!in->groups || !in->offsets || !in->boffsets))
        return fail(HQ_E_INVAL, "hq_worker_step_stream: NULL groups/offsets/boffsets");
    if (in->n_groups && in->boffsets[in->n_groups] > in->boffsets[0] && !in->bytes)
        return fail(HQ_E_INVAL, "hq_worker_step_stream: NULL bytes");
    std::memset(out, 0, sizeof *out);
    if (dstep)
        return step_on_device(hq_dstep_in{in->n_groups, in->groups, in->offsets, nullptr,
                                          in->boffsets, in->bytes ? in->bytes : &kNoBytes}, out);
    for (uint64_t i = 0; i < in->n_groups; ++i)
        if (in->offsets[i + 1] < in->offsets[i])
            return fail(HQ_E_INVAL, "hq_worker_step: offsets decrease");
    const uint64_t ne = in->n_groups ? in->offsets[in->n_groups] : 0;
    decoded.resize(ne);
    if (in->n_groups && hq_events_decode(in->n_groups, in->offsets, in->boffsets, in->bytes,
                                         decoded.data()) != HQ_OK)
        return fail(HQ_E_INVAL, "hq_worker_step_stream: malformed event stream");
    const hq_step_input rows{in->n_groups, in->groups, in->offsets, decoded.data()};
    return step(&rows, out);
}

// ------------------------------------------------------------------------------ C-ABI ------
extern "C" {

int hq_worker_step(hq_worker *w, const hq_step_input *in, hq_step_output *out) {
    return guarded(w, "hq_worker_step", [&] {
        if (!in || !out) return w->fail(HQ_E_INVAL, "hq_worker_step: NULL argument");
        if (in->n_groups && (!in->groups || !in->offsets))
            return w->fail(HQ_E_INVAL, "hq_worker_step: NULL groups/offsets");
        if (in->n_groups && in->offsets[in->n_groups] > in->offsets[0] && !in->events)
            return w->fail(HQ_E_INVAL, "hq_worker_step: NULL events");
        std::memset(out, 0, sizeof *out);
        if (w->dstep)
            return w->step_on_device(hq_dstep_in{in->n_groups, in->groups, in->offsets, in->events,
                                                 nullptr, nullptr}, out);
        return w->step(in, out);
    });
}

int hq_worker_step_stream(hq_worker *w, const hq_step_stream *in, hq_step_output *out) {
    return guarded(w, "hq_worker_step_stream", [&] { return w->step_stream(in, out); });
}

}  // extern "C"

// the wire's device mode (hq_wire_dev.hip; declared in hq_dstep.h)
hq_ctx *hq_worker_device_ctx(hq_worker *w) { return w && w->dstep ? w->ctx : nullptr; }

int hq_worker_step_device_rows(hq_worker *w, uint64_t n, const uint32_t *groups,
                               const uint64_t *offsets, const hq_event *events, uint64_t n_events,
                               hq_step_output *out) {
    return guarded(w, "hq_worker_step", [&] {
        if (!out) return (int)HQ_E_INVAL;
        if (!w->dstep) return w->fail(HQ_E_INVAL, "hq_worker_step: not a device worker");
        if (n && !offsets) return w->fail(HQ_E_INVAL, "hq_worker_step: NULL offsets");
        std::memset(out, 0, sizeof *out);
        hq_dstep_in in{n, groups, offsets, events, nullptr, nullptr};
        in.n_events = n_events;
        in.on_device = true;
        return w->step_on_device(in, out);
    });
}

// hq_worker_step_jobs (hq_jobs.cpp): jobs that are all sized event streams for distinct device
// workers on one GPU are stepped through shared launches (hq_dstep_run_jobs: one pass A per
// input chunk, one layout, one k_step_lite and one pass B for all of them, one wait) instead of
// one launch sequence per worker on its own thread. Returns kJobsNotFused, having done nothing,
// for any other set of jobs; else the first job's failure (each job's in its rc).
int hq_worker_step_jobs_fused(hq_step_job *jobs, uint32_t count) {
    if (count < 2 || count > kDStepMaxJobs) return kJobsNotFused;
    int device = -1;
    for (uint32_t j = 0; j < count; ++j) {
        const hq_step_job &b = jobs[j];
        const hq_step_stream *in = b.stream;
        if (!b.worker || !b.worker->dstep || !b.out || b.rows || !in || !(in->sizes || in->sizes16) ||
            (in->n_bytes && !in->bytes) || in->n_groups == 0)
            return kJobsNotFused;
        if (device >= 0 && b.worker->device != device) return kJobsNotFused;
        device = b.worker->device;
    }
    hq_dstep *ds[kDStepMaxJobs];
    hq_dstep_in ins[kDStepMaxJobs];
    hq_dstep_out outs[kDStepMaxJobs];
    int rcs[kDStepMaxJobs];
    uint32_t idx[kDStepMaxJobs], nl = 0;
    const uint64_t t0 = now_ns();
    for (uint32_t j = 0; j < count; ++j) {
        hq_worker *w = jobs[j].worker;
        std::memset(jobs[j].out, 0, sizeof *jobs[j].out);
        jobs[j].rc = w->sync_to_device();
        if (jobs[j].rc) continue;
        w->host_stale = true;
        ds[nl] = w->dstep;
        ins[nl] = sized_dstep_in(*jobs[j].stream);
        idx[nl++] = j;
    }
    const uint64_t t1 = now_ns();
    if (nl) (void)hq_dstep_run_jobs(ds, ins, outs, rcs, nl);
    int first = HQ_OK;
    for (uint32_t x = 0; x < nl; ++x) {
        hq_step_job &b = jobs[idx[x]];
        b.worker->dout = outs[x];
        b.rc = b.worker->device_step_done(rcs[x], ins[x], b.out, t0, t1);
    }
    for (uint32_t j = 0; j < count; ++j)
        if (jobs[j].rc && !first) first = jobs[j].rc;
    return first;
}
