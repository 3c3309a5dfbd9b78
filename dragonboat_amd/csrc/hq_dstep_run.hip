// hq_dstep_run.hip — the order in which the device step engine queues a step: one worker's
// (hq_dstep_run) and several workers' through shared launches (hq_dstep_run_jobs). The copies,
// events, waits, memsets and launches stand here in the order the device takes them; the kernels
// are behind the launchers of hq_dstep_k.h, the buffers in struct hq_dstep.
#include <algorithm>
#include <cstdio>

#include "hq_dstep_k.h"
#include "hq_sidecar.h"

namespace {

using hq::elapsed_ns;
using hq::grow;
using hq::now_ns;
using hq::wait_stream;

// One worker's step from its preparation to its outputs (hq_dstep_run; hq_dstep_run_jobs runs
// several of them through shared launches)
struct Run {
    hq_dstep *d = nullptr;
    const hq_dstep_in *in = nullptr;
    hq_dstep_out *out = nullptr;
    StepK k{};
    uint64_t n = 0, ne = 0, nb = 0, nw = 0;
    size_t ws = 0, tmp = 0, tmp2 = 0;
    size_t o_off = 0, o_boff = 0, o_ev = 0;
    int chunks = 1;
    bool stream = false, sized = false, small = false, small_scan = false;
    bool stepped = false, first = true;
    bool timing = false;          // ev_t0 recorded: pass B records ev_t1 before its wait
    uint64_t t0 = 0, t1 = 0, t_sub = 0, gpu_ns = 0;
    int rc = HQ_OK;
};

// A pinned output region of `want` bytes in place of d's (whose contents go), for d and the step's
// k. The new one is had first: if it cannot be (fail_for_test: HQ_TEST_FAIL_REGROW), the old stays
int new_host_out(hq_dstep *d, StepK &k, size_t want, bool fail_for_test = false) {
    hq_ctx *ctx = d->ctx;
    void *grown = nullptr;
    int rc = hq::check_hip(ctx, hipHostMalloc(&grown, want, hipHostMallocDefault),
                           "hq_dstep pinned output");
    if (fail_for_test) {          // tests: the allocation failure path
        if (grown) (void)hipHostFree(grown);
        grown = nullptr;
        rc = hq::fail(ctx, HQ_E_NOMEM, "hq_dstep pinned output: injected failure");
    }
    if (rc) return rc;
    if (d->host_out) (void)hipHostFree(d->host_out);
    d->host_out = grown;
    d->host_out_cap = want;
    k.out = static_cast<char *>(grown);
    k.out_cap = want;
    return HQ_OK;
}

// one copy queued on s, unless rc is set already or there is nothing to copy
void queue_copy(hq_ctx *ctx, int &rc, void *dst, const void *src, size_t bytes, hipStream_t s,
                hipMemcpyKind kind = hipMemcpyHostToDevice) {
    if (!rc && bytes)
        rc = hq::check_hip(ctx, hipMemcpyAsync(dst, src, bytes, kind, s),
                           kind == hipMemcpyHostToDevice ? "hq_dstep H2D" : "hq_dstep D2D");
}

// The step's buffers (grown as needed) and its StepK, with the memsets it needs queued on s; no
// launch. in->n > 0.
int prepare(Run &r, hipStream_t s, bool jobs = false) {
    hq_dstep *d = r.d;
    hq_ctx *ctx = d->ctx;
    const hq_dstep_in *in = r.in;
    const uint64_t n = r.n = in->n;
    r.stream = in->bytes != nullptr;
    r.sized = r.stream && (in->sizes != nullptr || in->sizes16 != nullptr);   // scanned here
    const bool stream = r.stream, sized = r.sized;
    const bool s16 = sized && in->sizes16 != nullptr;   // 2-byte words: bytes only
    const bool on_dev = in->on_device && !stream;   // rows on the device: nothing read here
    const uint64_t ne = r.ne = sized || on_dev ? in->n_events : in->offsets[n];
    const uint64_t nb = r.nb = !stream ? 0 : sized ? in->n_bytes : in->boffsets[n];
    if (sized && (ne >> 32 || nb >> 32))     // the scanned prefixes pack both totals in 64 bits
        return hq::fail(ctx, HQ_E_INVAL, "hq_dstep: a sized step holds < 2^32 events and bytes");
    r.t0 = now_ns();
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    // chunks of groups (at least 64 Ki each): chunk c's input copy overlaps pass A of chunk c - 1
    while (!on_dev && r.chunks * 2 <= kMaxChunks && n >= (uint64_t)r.chunks * 2 * kChunkGroups)
        r.chunks *= 2;
    // the step's input in one device region: handles, offsets, [boffsets,] events or bytes, each
    // at the offsets it has on the host; a sized stream: handles, sizes (+ a zero), their scan,
    // bytes
    auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
    r.o_off = up(n * 4);
    r.o_boff = r.o_off + up((n + 1) * 8);
    r.o_ev = r.o_boff + (stream ? up((n + 1) * 8) : 0);   // (sized: prefix at o_boff)
    // + 8: slack for ByteReader's aligned word past the last byte
    const size_t in_bytes = r.o_ev + (stream ? nb : ne * sizeof(hq_event)) + 8;
    if (!rc) rc = grow(ctx, &d->in, &d->in_cap, in_bytes, false, "hq_dstep input");
    char *din = static_cast<char *>(d->in);
    // counts [kLists][n] and the prefixes pass B reads, [kLists][n]; the scan buffer holds the
    // per-wave sums [kLists][nw] + 1 (a zero: the scan's last element is the grand total) and
    // their scan (one size covers both)
    const uint64_t nw = r.nw = (n + 63) / 64;
    const size_t ws = r.ws = (size_t)kLists * nw + 1;
    r.small_scan = ws <= kScanSmall;
    const size_t cn = (size_t)2 * kLists * n + 2 * ws;
    size_t cc = d->cnt_cap * 4, sc = d->cnt_cap * 4, bc = d->cnt_cap ? 256 : 0;
    if (!rc && cn > d->cnt_cap) {
        rc = grow(ctx, &d->counts, &cc, cn * 4, false, "hq_dstep counts");
        if (!rc) rc = grow(ctx, &d->scan, &sc, cn * 4, false, "hq_dstep scan");
        if (!rc && !d->bases) {
            rc = grow(ctx, &d->bases, &bc, 256, false, "hq_dstep error");
            if (!rc) rc = hq::check_hip(ctx, hipMemsetAsync(d->bases, 0, 256, s), "memset");
        }
        if (!rc) d->cnt_cap = std::min(cc, sc) / 4;
    }
    // pass A's chained-scan words: zeroed when allocated (their tags then never match a step)
    const size_t tiles_bytes = ((n + 255) / 256 + 1) * 8;
    if (!rc && tiles_bytes > d->tiles_cap) {
        rc = grow(ctx, &d->tiles, &d->tiles_cap, tiles_bytes, false, "hq_dstep tiles");
        if (!rc) rc = hq::check_hip(ctx, hipMemsetAsync(d->tiles, 0, d->tiles_cap, s), "memset");
    }
    if (!rc && ws * 4 > d->wsum_cap) {
        rc = grow(ctx, &d->wsum, &d->wsum_cap, ws * 4, false, "hq_dstep wave sums");
        d->wsum_dirty = true;
    }
    if (!rc && n > d->rcap) {
        size_t fc = d->rcap, lc = d->rcap * 4;
        rc = grow(ctx, &d->rerun, &fc, n, false, "hq_dstep rerun");
        if (!rc) rc = grow(ctx, &d->rerun_list, &lc, n * 4, false, "hq_dstep rerun list");
        size_t sc = d->rcap * sizeof(hq_ready_to_read);
        if (!rc)
            rc = grow(ctx, &d->ready_slot, &sc, n * sizeof(hq_ready_to_read), false,
                      "hq_dstep ready slots");
        if (!rc) d->rcap = std::min({fc, lc / 4, sc / sizeof(hq_ready_to_read)});
    }
    // the host region the lists go to: last step's size with room to spare (a step that needs
    // more runs pass B again after growing it)
    if (!rc && !d->host_out) rc = new_host_out(d, r.k, std::max<size_t>(n * 64, 1 << 16));
    uint64_t *prefix = reinterpret_cast<uint64_t *>(din + r.o_boff);
    // (the jobs path scans with its own kernels: no hipcub temporary, whose size query costs
    // microseconds of host time per job before the first launch)
    if (!rc && !jobs) rc = hq::scan_wave_sums(ctx, s, nullptr, &r.tmp, d->wsum, d->scan, ws);
    if (!rc && sized && !jobs)
        rc = hq::scan_sizes(ctx, s, nullptr, &r.tmp2, din + r.o_off, s16, n, prefix);
    // (the jobs path's per-1024-group size totals live there too)
    const size_t bsum_bytes = sized ? (n + 1 + kSizeTile - 1) / kSizeTile * 8 : 0;
    if (!rc) rc = grow(ctx, &d->scan_tmp, &d->scan_tmp_cap, std::max({r.tmp, r.tmp2, bsum_bytes}),
                       false, "hq_dstep scan tmp");
    if (rc) return rc;
    StepK &k = r.k;
    k = StepK{};
    k.groups = d->groups;
    k.members = d->members;
    k.reads = d->reads;
    k.n = n;
    k.i_end = n;                  // (i_begin, own_lo and chunk start at 0)
    k.own_hi = UINT64_MAX;
    k.handles = (sized || on_dev) && !in->groups ? nullptr : reinterpret_cast<const uint32_t *>(din);
    k.offsets = reinterpret_cast<const uint64_t *>(din + r.o_off);
    if (sized) {
        k.prefix = prefix;
        k.bytes = reinterpret_cast<const uint8_t *>(din + r.o_ev);
        k.sizes = reinterpret_cast<const uint32_t *>(din + r.o_off);
        k.sizes16 = reinterpret_cast<const uint16_t *>(din + r.o_off);   // (one of the two)
        k.bytes_only = s16;
        k.bsum = static_cast<uint64_t *>(d->scan_tmp);
    } else if (stream) {
        k.boffsets = reinterpret_cast<const uint64_t *>(din + r.o_boff);
        k.bytes = reinterpret_cast<const uint8_t *>(din + r.o_ev);
    } else {
        k.events = reinterpret_cast<const hq_event *>(din + r.o_ev);
    }
    k.counts = d->counts;
    k.pre = d->counts + (size_t)kLists * n;
    k.wsum = d->wsum;
    k.ws = ws;
    k.scan = d->scan;
    k.nw = nw;
    k.n_handles = d->n_groups;
    k.n_events = ne;
    k.n_bytes = nb;
    k.stamp = d->stamp;
    if (++d->step_no == 0) {      // stamps wrap: forget them, and the chained-scan words
        rc = hq::check_hip(ctx, hipMemsetAsync(d->stamp, 0, d->gcap * 4, s), "memset");   // (tagged
        if (!rc && d->tiles)                                                               // with it)
            rc = hq::check_hip(ctx, hipMemsetAsync(d->tiles, 0, d->tiles_cap, s), "memset");
        d->step_no = 1;
        if (rc) return rc;
    }
    k.step_no = d->step_no;
    // pass A adds each wave's counts into d->wsum, which k_step_lite leaves zero; a step that
    // stopped before it (or a new buffer) leaves it to clear here
    if (d->wsum_dirty) {
        rc = hq::check_hip(ctx, hipMemsetAsync(d->wsum, 0, d->wsum_cap, s), "memset");
        if (rc) return rc;
    }
    d->wsum_dirty = true;
    k.error = d->bases;           // zero here: reset by the previous step's k_layout
    k.wide = d->commit_column & kColumn32 ? d->bases + 1 : nullptr;   // likewise
    k.out = static_cast<char *>(d->host_out);
    k.layout = d->layout;
    k.groups_old = d->groups_old;
    k.match_old = d->match_old;
    // pass A's advance words need the column allowed and the region to hold n of them (its
    // offset 0 is the commits list's in every layout)
    k.spec_col = (d->commit_column & kColumn32) && n * 4 <= d->host_out_cap;
    k.spec_valid = k.spec_col;
    // pass A writes the single ReadyToReads at their places too (ready_tail): stream input, the
    // column speculated, the counts within a tile word
    // (not the jobs path: there pass A reads the streams over the link in place, and these
    // writes beside its reads slowed it by more than k_step_lite's copy takes, 981 vs 693 + 158
    // us for the 16-worker step5, profiles/r05e)
    // (nor with compact ReadyToReads, whose record size the layout picks after pass A)
    k.spec_ready = !jobs && stream && k.spec_col && ne < kTileVal &&
                   !(d->commit_column & kReadyCompact);
    k.ready_wide = (d->commit_column & kReadyCompact) ? d->bases + 2 : nullptr;   // (zero: k_layout)
    k.ready_off = (n * 4 + 255) & ~uint64_t(255);   // layout_from's offset of the list after the column
    k.tiles = d->tiles;
    k.tickets = d->tickets;
    k.reads_old = d->reads_old;
    k.rerun = d->rerun;
    k.rerun_list = d->rerun_list;
    k.ready_slot = d->ready_slot;
    k.out_cap = d->host_out_cap;
    k.test_scan_fail = d->test_scan_fail;
    k.allow_column = d->commit_column & ~kReadySlots;
    k.host_layout = d->host_layout;
    r.small = d->max_members <= 8;   // member slots in registers: 8 or kDMembers
    // HQ_WORKER_READY_SLOTS: a stream step of the jobs path (pass A's tiles are whole 256-group
    // blocks of one launch there) with the advance column allowed writes the slots; the host region
    // is grown ahead of pass A to hold the column, the slots and room for the lists
    if (jobs && stream && (d->commit_column & kReadySlots) && (d->commit_column & kColumn32)) {
        const uint64_t reserve = slot_layout(n, &k.slot_off, &k.cnt_off);
        const size_t want = reserve + std::max<size_t>(n * 16, 1 << 16);
        if (d->host_out_cap < want) {
            rc = new_host_out(d, k, want);
            if (rc) return rc;
            k.spec_col = n * 4 <= want;
            k.spec_valid = k.spec_col;
        }
        k.slots = 1;
        k.allow_column |= kReadySlots;
    }
    return HQ_OK;
}

// one pass over groups [i0, i1) of the step on its worker's stream
void launch_pass(Run &r, bool write, uint64_t i0, uint64_t i1) {
    r.k.i_begin = i0;
    r.k.i_end = i1;
    if (!r.rc && i1 != i0) r.rc = hq::launch_step(r.d->ctx, write, r.stream, r.small, r.k);
}

// layout, pass B (straight into the pinned region), the layout back: one wait per step. The
// first layout of a small step scans the wave sums in one workgroup; a re-run after an overflow
// (or a step whose sums hipcub scanned) takes k_layout: k_step_lite has cleared the sums
void pass_b(Run &r) {
    hq_dstep *d = r.d;
    hq_ctx *ctx = d->ctx;
    if (!r.rc && r.small_scan && r.first) r.rc = hq::launch_scan_layout(ctx, ctx->stream, r.k);
    else if (!r.rc) r.rc = hq::launch_layout(ctx, ctx->stream, r.k);
    r.first = false;
    if (!r.rc) {
        r.rc = hq::launch_step_lite(ctx, ctx->stream, r.k);
        if (!r.rc) d->wsum_dirty = d->tickets_dirty = false;
    }
    launch_pass(r, true, 0, r.n);
    if (!r.rc && r.timing) {
        r.rc = hq::check_hip(ctx, hipEventRecord(d->ev_t1, ctx->stream), "event");
        r.t_sub = now_ns();
    }
    if (!r.rc) r.rc = wait_stream(d, ctx->stream, "hq_dstep sync");
    if (!r.rc && r.timing) r.gpu_ns = elapsed_ns(d->ev_t0, d->ev_t1);
    r.timing = false;             // (a second pass B, after the output region grew: untimed)
}

// Pass A has written every listed group's new state in place (the state it found is saved).
// From there on a step that fails returns with that state taken back (k_step_restore), so a
// failed step leaves the groups as they were, whatever failed: an input error found by the
// kernels, a HIP error, the output region that could not grow, a second layout failure. (A
// pass A launch that itself fails leaves rc set before that point; the context is then
// unusable and the caller reloads the groups from the device, hq_worker.cpp.)
int restore(Run &r, int code) {
    if (!r.stepped) return code;
    hq_ctx *ctx = r.d->ctx;
    int r2 = hq::launch_step_restore(ctx, ctx->stream, r.k);
    if (!r2) r2 = wait_stream(r.d, ctx->stream, "hq_dstep restore");
    return code ? code : r2;
}

// hq::device_view of a step input, which is host memory: pinned memory only (anything else is
// copied instead)
template <class T>
const T *pinned_on_device(const T *p) {
    bool pinned;
    const void *d = hq::device_view(p, &pinned);
    return pinned ? static_cast<const T *>(d) : nullptr;
}

// after the first pass B and its wait: input errors, an output region too small, the outputs
int finish(Run &r) {
    hq_dstep *d = r.d;
    hq_ctx *ctx = d->ctx;
    hq_dstep_out *out = r.out;
    if (r.rc) return restore(r, r.rc);
    const Layout &lay = *d->host_layout;
    if (lay.error == kErrScan) {
        // pass A's chained scan of the ReadyToRead places gave up on a stalled predecessor
        // (only the copy-out is affected, not a group's step): the layout again, and k_step_lite
        // writes every single ReadyToRead, as when pass A does not (spec_ready off). The layout
        // kept pass A's flags for this; its error word is cleared here
        r.k.spec_ready = 0;
        int rc = hq::check_hip(ctx, hipMemsetAsync(r.k.error, 0, 4, ctx->stream), "memset");
        if (rc) return restore(r, rc);
        pass_b(r);
        if (r.rc) return restore(r, r.rc);
    }
    if (lay.error) {              // no group state is written: pass A's is taken back
        const int rc = restore(r, HQ_OK);
        if (rc) return rc;
        out->input_error = lay.error;
        return HQ_E_INVAL;
    }
    if (lay.overflow) {           // grow the region and write the lists again
        // the new region first: if it cannot be had, the old one stays and the step is undone
        const int rc = new_host_out(d, r.k, lay.total + lay.total / 2, d->test_fail_regrow);
        if (rc) return restore(r, rc);
        r.k.spec_valid = 0;       // pass A's advance words went with the old region
        pass_b(r);
        if (r.rc) return restore(r, r.rc);
        if (lay.overflow || lay.error)
            return restore(r, hq::fail(ctx, HQ_E_STATE, "hq_dstep: output layout"));
    }
    const char *ho = static_cast<const char *>(d->host_out);
    if (lay.reserve) {            // the slot form (pass A's, or k_step_lite's after a regrow)
        out->ready_slots = reinterpret_cast<const hq_ready_compact *>(ho + r.k.slot_off);
        out->slot_counts = reinterpret_cast<const uint32_t *>(ho + r.k.cnt_off);
        out->n_tiles = (r.n + kSlotTile - 1) / kSlotTile;
        out->n_slotted = lay.len[kSlotted];
    }
    out->wait = d->last_wait;
    out->commits = lay.commit_column ? nullptr
                                     : reinterpret_cast<const hq_commit_event *>(ho + lay.off[kCommits]);
    out->commit_col = lay.commit_column == kColumn64
                          ? reinterpret_cast<const uint64_t *>(ho + lay.off[kCommits]) : nullptr;
    out->commit_adv = lay.commit_column == kColumn32
                          ? reinterpret_cast<const uint32_t *>(ho + lay.off[kCommits]) : nullptr;
    out->ready = lay.ready_compact ? nullptr
                                   : reinterpret_cast<const hq_ready_to_read *>(ho + lay.off[kReady]);
    out->ready_compact = lay.ready_compact
                             ? reinterpret_cast<const hq_ready_compact *>(ho + lay.off[kReady])
                             : nullptr;
    out->resps = reinterpret_cast<const hq_read_index_resp *>(ho + lay.off[kResps]);
    out->states = reinterpret_cast<const hq_state_change *>(ho + lay.off[kStates]);
    out->dropped = reinterpret_cast<const hq_dropped_read *>(ho + lay.off[kDropped]);
    out->deferred = reinterpret_cast<const uint64_t *>(ho + lay.off[kDeferred]);
    out->fallback = reinterpret_cast<const uint64_t *>(ho + lay.off[kFallback]);
    out->n_commits = lay.len[kCommits];
    out->n_ready = lay.len[kReady];
    out->n_resps = lay.len[kResps];
    out->n_states = lay.len[kStates];
    out->n_dropped = lay.len[kDropped];
    out->n_deferred = lay.len[kDeferred];
    out->n_fallback = lay.len[kFallback];
    out->decisions = lay.len[kDecisions];
    out->kernel_ns = r.t1 - r.t0;
    out->d2h_ns = now_ns() - r.t1;
    out->submit_ns = r.t_sub > r.t0 ? r.t_sub - r.t0 : 0;
    out->gpu_ns = r.gpu_ns;
    out->gpu_jobs = 1;
    return HQ_OK;
}

}  // namespace

int hq_dstep_run(hq_dstep *d, const hq_dstep_in *in, hq_dstep_out *out) {
    *out = hq_dstep_out{};
    if (in->n == 0) return HQ_OK;
    // A sized stream in pinned memory takes the jobs path as one job: pass A reads it in place in
    // one launch (the stream staged through LDS), where this path's chunked copies put the
    // first chunk's copy ahead of pass A and the last chunk's pass A behind the copies
    if ((in->sizes || in->sizes16) && in->bytes && pinned_on_device(in->bytes)) {
        int rc1 = HQ_OK;
        const int rc = hq_dstep_run_jobs(&d, in, out, &rc1, 1);
        return rc1 ? rc1 : rc;
    }
    Run r{d, in, out};
    hq_ctx *ctx = d->ctx;
    r.rc = prepare(r, ctx->stream);
    if (r.rc) return r.rc;
    r.rc = hq::check_hip(ctx, hipEventRecord(d->ev_t0, ctx->stream), "event");
    if (!r.rc && d->tickets_dirty)
        r.rc = hq::check_hip(ctx, hipMemsetAsync(d->tickets, 0, kTickets * 4, ctx->stream), "memset");
    if (r.rc) return r.rc;
    d->tickets_dirty = true;
    r.timing = true;
    const uint64_t n = r.n, ne = r.ne, nb = r.nb;
    const bool stream = r.stream, sized = r.sized;
    const int chunks = r.chunks;
    uint64_t bound[kMaxChunks + 1];
    // (multiples of 256 inside: pass A's waves are the scan's, its tiles ready_tail's)
    for (int c = 0; c <= chunks; ++c)
        bound[c] = c == chunks ? n : (n * c / chunks) & ~uint64_t(255);
    if (chunks > 1 && !d->copy)       // the copy stream of the first chunked step
        r.rc = hq::check_hip(ctx, hipStreamCreateWithFlags(&d->copy, hipStreamNonBlocking),
                           "hq_dstep copy stream");
    // one chunk: every copy on the compute stream (nothing to overlap, no cross-stream waits)
    hipStream_t cs = chunks > 1 ? d->copy : ctx->stream;
    char *din = static_cast<char *>(d->in);
    if (sized) {
        // handles and sizes, their scan (PackSize adds the totals as element n); then
        // the bytes in equal byte chunks, each followed by pass A over the groups whose bytes end
        // inside what has landed
        // every copy is queued before the first launch, event c behind chunk c's bytes; the
        // handles and sizes go on the compute stream ahead of their scan, the bytes on the copy
        // stream beside them (behind the sizes on one stream the first bytes copy started
        // 50-65 us after the sizes' copy ended)
        // (groups NULL: handles 0 .. n - 1)
        if (in->groups) queue_copy(ctx, r.rc, din, in->groups, n * 4, ctx->stream);
        if (in->sizes16) queue_copy(ctx, r.rc, din + r.o_off, in->sizes16, n * 2, ctx->stream);
        else queue_copy(ctx, r.rc, din + r.o_off, in->sizes, n * 4, ctx->stream);
        for (int c = 0; c < chunks && !r.rc; ++c) {
            const uint64_t lo = nb * c / chunks, hi = nb * (c + 1) / chunks;
            queue_copy(ctx, r.rc, din + r.o_ev + lo, in->bytes + lo, hi - lo, cs);
            if (chunks > 1 && !r.rc) r.rc = hq::check_hip(ctx, hipEventRecord(d->ev_in[c], cs), "event");
        }
        if (!r.rc)
            r.rc = hq::scan_sizes(ctx, ctx->stream, d->scan_tmp, &r.tmp2, din + r.o_off,
                                in->sizes16 != nullptr, n, const_cast<uint64_t *>(r.k.prefix));
        for (int c = 0; c < chunks && !r.rc; ++c) {
            const uint64_t lo = nb * c / chunks, hi = nb * (c + 1) / chunks;
            if (chunks > 1)
                r.rc = hq::check_hip(ctx, hipStreamWaitEvent(ctx->stream, d->ev_in[c], 0), "wait");
            r.k.own_lo = c == 0 ? 0 : lo + 1;
            r.k.own_hi = c + 1 == chunks ? UINT64_MAX : hi + 1;
            r.k.chunk = (uint32_t)c;
            launch_pass(r, false, 0, n);
        }
    }
    // rows on the device: the three arrays into the input region as they are (one chunk)
    const bool on_dev = in->on_device && !stream;
    if (on_dev) {
        const hipMemcpyKind d2d = hipMemcpyDeviceToDevice;
        if (in->groups) queue_copy(ctx, r.rc, din, in->groups, n * 4, ctx->stream, d2d);
        queue_copy(ctx, r.rc, din + r.o_off, in->offsets, (n + 1) * 8, ctx->stream, d2d);
        queue_copy(ctx, r.rc, din + r.o_ev, in->events, ne * sizeof(hq_event), ctx->stream, d2d);
        launch_pass(r, false, 0, n);
    }
    // inputs chunk by chunk, pass A of each chunk once it has landed
    for (int c = 0; c < chunks && !r.rc && !sized && !on_dev; ++c) {
        const uint64_t i0 = bound[c], i1 = bound[c + 1];
        queue_copy(ctx, r.rc, din + i0 * 4, in->groups + i0, (i1 - i0) * 4, cs);
        queue_copy(ctx, r.rc, din + r.o_off + i0 * 8, in->offsets + i0, (i1 - i0 + 1) * 8, cs);
        if (stream) {
            queue_copy(ctx, r.rc, din + r.o_boff + i0 * 8, in->boffsets + i0, (i1 - i0 + 1) * 8, cs);
            // the chunk's bytes (garbage offsets are the kernel's to reject: clamp the copy)
            const uint64_t lo = std::min(in->boffsets[i0], nb);
            const uint64_t hi = std::min(std::max(in->boffsets[i1], lo), nb);
            queue_copy(ctx, r.rc, din + r.o_ev + lo, in->bytes + lo, hi - lo, cs);
        } else {
            const uint64_t lo = std::min(in->offsets[i0], ne);
            const uint64_t hi = std::min(std::max(in->offsets[i1], lo), ne);
            queue_copy(ctx, r.rc, din + r.o_ev + lo * sizeof(hq_event), in->events + lo,
                       (hi - lo) * sizeof(hq_event), cs);
        }
        if (chunks > 1) {
            if (!r.rc) r.rc = hq::check_hip(ctx, hipEventRecord(d->ev_in[c], cs), "event");
            if (!r.rc) r.rc = hq::check_hip(ctx, hipStreamWaitEvent(ctx->stream, d->ev_in[c], 0), "wait");
        }
        r.k.chunk = (uint32_t)c;
        launch_pass(r, false, i0, i1);
    }
    r.k.own_lo = 0;
    r.k.own_hi = UINT64_MAX;
    r.k.chunk = 0;
    // the wave sums' scan (hipcub for a large step; a small one's is the layout's workgroup)
    if (!r.rc && !r.small_scan)
        r.rc = hq::scan_wave_sums(ctx, ctx->stream, d->scan_tmp, &r.tmp, d->wsum, d->scan, r.ws);
    r.stepped = !r.rc;
    pass_b(r);
    r.t1 = now_ns();
    return finish(r);
}

int hq_dstep_run_jobs(hq_dstep *const *ds, const hq_dstep_in *ins, hq_dstep_out *outs, int *rcs,
                      uint32_t count) {
    if (count == 0) return HQ_OK;
    if (count > kMaxJobs) return HQ_E_INVAL;
    hq_dstep *d0 = ds[0];
    hq_ctx *ctx = d0->ctx;
    hipStream_t s = ctx->stream;
    // HQ_STEP_JOBS_TRACE=1: the host phases of each call to stderr (where a step's time goes)
    static const bool trace = hq::env_flag("HQ_STEP_JOBS_TRACE");
    uint64_t tp[6] = {now_ns(), 0, 0, 0, 0, 0};
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    Run runs[kMaxJobs];
    uint32_t live[kMaxJobs], nl = 0;
    for (uint32_t j = 0; j < count; ++j) {
        outs[j] = hq_dstep_out{};
        rcs[j] = HQ_OK;
        if (ds[j]->ctx->device != ctx->device || !(ins[j].sizes || ins[j].sizes16) || !ins[j].bytes) {
            rcs[j] = hq::fail(ds[j]->ctx, HQ_E_INVAL, "hq_dstep_run_jobs: a sized stream step "
                                                      "on the first job's device");
            continue;
        }
        if (rc || ins[j].n == 0) {
            rcs[j] = rc;
            continue;
        }
        Run &r = runs[j];
        r.d = ds[j];
        r.in = &ins[j];
        r.out = &outs[j];
        rcs[j] = prepare(r, s, true);
        if (!rcs[j]) live[nl++] = j;
    }
    if (!nl) return rc;
    tp[1] = now_ns();
    if (!rc && d0->wait_clock) rc = hq::stamp_clock(d0, s, 1);   // the clock ahead of the step
    if (!rc) rc = hq::check_hip(ctx, hipEventRecord(d0->ev_t0, s), "event");
    if (!rc && d0->tickets_dirty)
        rc = hq::check_hip(ctx, hipMemsetAsync(d0->tickets, 0, kTickets * 4, s), "memset");
    d0->tickets_dirty = true;
    // the jobs' StepK, pinned and copied to the device ahead of the launches
    if (!rc && nl > d0->jobs_cap) {
        if (d0->jobs_host) (void)hipHostFree(d0->jobs_host);
        if (d0->jobs_dev) (void)hipFree(d0->jobs_dev);
        d0->jobs_host = d0->jobs_dev = nullptr;
        d0->jobs_host_dev = nullptr;
        d0->jobs_cap = 0;
        rc = hq::check_hip(ctx, hipHostMalloc(&d0->jobs_host, kMaxJobs * sizeof(StepK),
                                              hipHostMallocDefault), "hq_dstep jobs");
        if (!rc) rc = hq::check_hip(ctx, hipMalloc(&d0->jobs_dev, kMaxJobs * sizeof(StepK)),
                                    "hq_dstep jobs");
        if (!rc) {
            d0->jobs_cap = kMaxJobs;
            d0->jobs_host_dev = pinned_on_device(d0->jobs_host);
        }
    }
    bool small = true;
    uint64_t total_bytes = 0;
    // (a stream read in place: ByteReader's aligned 8-byte words and the staging's aligned 16-byte
    // blocks never cross a page, so no read leaves the caller's pages; a kernel launch acquires
    // at system scope, so the host's writes before the call are seen)
    // (the streams' pointers are checked after the sizes' scan is queued: the checks cost the
    // host ~1 us each, and the scan does not read the streams)
    for (uint32_t x = 0; x < nl && !rc; ++x) {
        Run &r = runs[live[x]];
        // sizes in pinned host memory are read by k_size_sums over the link: no copy per job
        // (16 workers' 256 KB size copies took 340 us one after another, with their gaps)
        if (r.in->sizes16) r.k.sizes16_src = pinned_on_device(r.in->sizes16);
        else r.k.sizes_src = pinned_on_device(r.in->sizes);
        d0->jobs_host[x] = r.k;
        small = small && r.small;
        total_bytes += r.nb;
    }
    // (k_size_sums reads the table from the pinned copy and writes it to the device: no copy is
    // queued ahead of the first launch, ~25 us of host time for a one-worker step)
    const bool table_first = !d0->jobs_host_dev;
    if (!rc && table_first)
        rc = hq::check_hip(ctx, hipMemcpyAsync(d0->jobs_dev, d0->jobs_host, nl * sizeof(StepK),
                                               hipMemcpyHostToDevice, s), "hq_dstep jobs");
    tp[2] = now_ns();
    // maps of jobs [x0, x1) onto workgroups of `per` groups (+ extra elements per job)
    auto map = [&](uint32_t x0, uint32_t x1, uint64_t per, uint64_t extra) {
        JobMap m{};
        m.ks = d0->jobs_dev;
        m.job0 = x0;
        m.count = x1 - x0;
        m.tickets = d0->tickets;
        m.blk0[0] = 0;
        for (uint32_t x = x0; x < x1; ++x)
            m.blk0[x - x0 + 1] = m.blk0[x - x0] + (uint32_t)((runs[live[x]].n + extra + per - 1) / per);
        return m;
    };
    // The jobs' bytes in up to kMaxJobChunks chunks of whole jobs, copied on two copy streams
    // (jobs alternating: one copy's start-up gap overlaps the other's transfer), event c behind
    // chunk c on each. Queued in the order the device needs them, since each call takes the host
    // microseconds: the sizes' scan first (it reads pinned sizes over the link), the copies of
    // chunks 0 and 1, then pass A of chunk c (once its bytes have landed) before the copies of
    // chunk c + 2.
    for (hipStream_t *cs : {&d0->copy, &d0->copy2})
        if (!rc && !*cs)
            rc = hq::check_hip(ctx, hipStreamCreateWithFlags(cs, hipStreamNonBlocking),
                               "hq_dstep copy stream");
    uint32_t cend[kMaxJobChunks + 1] = {0};
    int nchunks = 0;
    bool zero_copy = false;
    // the sizes' first pass before anything else the device can start on
    for (uint32_t x = 0; x < nl; ++x) {
        const Run &r = runs[live[x]];
        char *din = static_cast<char *>(r.d->in);
        if (r.in->groups) queue_copy(ctx, rc, din, r.in->groups, r.n * 4, s);
        if (r.in->sizes16) {
            if (!r.k.sizes16_src) queue_copy(ctx, rc, din + r.o_off, r.in->sizes16, r.n * 2, s);
        } else if (!r.k.sizes_src) {
            queue_copy(ctx, rc, din + r.o_off, r.in->sizes, r.n * 4, s);
        }
    }
    if (!rc) {
        // every job's stream in pinned host memory: pass A (and pass B) read it in place, in one
        // launch for all jobs, with no copy (a pageable stream among them: all are copied in
        // chunks). The streams' device addresses go into the table before the first launch, which
        // carries it to the device
        zero_copy = true;
        const uint8_t *zbytes[kMaxJobs] = {};
        for (uint32_t x = 0; x < nl && zero_copy; ++x) {
            zbytes[x] = pinned_on_device(runs[live[x]].in->bytes);
            zero_copy = zbytes[x] != nullptr || runs[live[x]].nb == 0;
        }
        if (zero_copy) {
            for (uint32_t x = 0; x < nl; ++x) {
                Run &r = runs[live[x]];
                if (zbytes[x]) r.k.bytes = zbytes[x];
                d0->jobs_host[x].bytes = r.k.bytes;
            }
        }
        if (zero_copy && table_first)   // (no device alias of the pinned table: copied again)
            rc = hq::check_hip(ctx, hipMemcpyAsync(d0->jobs_dev, d0->jobs_host, nl * sizeof(StepK),
                                                   hipMemcpyHostToDevice, s), "hq_dstep jobs");
    }
    JobMap sm = map(0, nl, kSizeTile, 1);
    for (uint32_t x = 0; x < nl; ++x)   // (a large job: its size tiles' totals get their own scan)
        if ((runs[live[x]].n + kSizeTile) / kSizeTile > kSizeApplyDirect) sm.bsum_scanned = 1;
    if (!rc) {
        // k_size_sums reads the table from its pinned copy and writes it to the device for the
        // launches behind it: no copy of its own (a blit launch and ~10 us of host time)
        JobMap pm = sm;
        if (!table_first) {
            pm.ks = d0->jobs_host_dev;
            pm.table_out = d0->jobs_dev;
        }
        rc = hq::launch_size_sums(ctx, s, pm);
    }
    if (zero_copy) {              // one chunk of all jobs, nothing to copy
        cend[nchunks = 1] = nl;
    } else {
        uint64_t acc = 0;
        uint32_t x = 0;
        while (nchunks < kMaxJobChunks && x < nl) {
            const uint64_t want = total_bytes * (uint64_t)(nchunks + 1) / kMaxJobChunks;
            do acc += runs[live[x++]].nb;
            while (x < nl && (nchunks + 1 == kMaxJobChunks || acc < want));
            cend[++nchunks] = x;
        }
    }
    auto copies = [&](int c) {
        if (c >= nchunks || zero_copy) return;
        for (uint32_t x = cend[c]; x < cend[c + 1]; ++x) {
            const Run &r = runs[live[x]];
            queue_copy(ctx, rc, static_cast<char *>(r.d->in) + r.o_ev, r.in->bytes, r.nb,
                       x % 2 ? d0->copy2 : d0->copy);
        }
        if (!rc) rc = hq::check_hip(ctx, hipEventRecord(d0->ev_in[c], d0->copy), "event");
        if (!rc) rc = hq::check_hip(ctx, hipEventRecord(d0->ev_in2[c], d0->copy2), "event");
    };
    copies(0);
    if (!rc && sm.bsum_scanned) rc = hq::launch_bsum_scan_jobs(ctx, s, sm);
    if (!rc) rc = hq::launch_size_apply(ctx, s, sm);
    copies(1);
    for (int c = 0; c < nchunks && !rc; ++c) {
        const uint32_t x0 = cend[c], x1 = cend[c + 1];
        if (!zero_copy) {
            rc = hq::check_hip(ctx, hipStreamWaitEvent(s, d0->ev_in[c], 0), "wait");
            if (!rc) rc = hq::check_hip(ctx, hipStreamWaitEvent(s, d0->ev_in2[c], 0), "wait");
        }
        JobMap m = map(x0, x1, 256, 0);
        m.chunk = (uint32_t)c;
        if (!rc) {
            rc = hq::launch_step_jobs(ctx, false, small, m);
            for (uint32_t x = x0; x < x1 && !rc; ++x) runs[live[x]].stepped = true;
        }
        copies(c + 2);
    }
    // every job's layout (one workgroup each), k_step_lite and pass B over all jobs, one wait;
    // one large job (a single worker's step) scans its wave sums with hipcub, whose two launches
    // take ~14 us where the one workgroup took 117 for 1 M groups (147 Ki sums, profiles/r05e)
    const JobMap am = map(0, nl, 256, 0);
    Run &r0 = runs[live[0]];
    hq_dstep *dj = r0.d;          // (the one job's engine: not d0 when job 0 listed no group)
    if (!rc && nl == 1 && !r0.small_scan) {
        size_t tmp = 0;
        rc = hq::scan_wave_sums(ctx, s, nullptr, &tmp, dj->wsum, dj->scan, r0.ws);
        // (scan_tmp holds the sizes' block totals, done with once pass A has its prefixes)
        if (!rc) rc = grow(ctx, &dj->scan_tmp, &dj->scan_tmp_cap, tmp, false, "hq_dstep scan tmp");
        if (!rc) rc = hq::scan_wave_sums(ctx, s, dj->scan_tmp, &tmp, dj->wsum, dj->scan, r0.ws);
        if (!rc) rc = hq::launch_layout(ctx, s, r0.k);
    } else if (!rc) {
        rc = hq::launch_scan_layout_jobs(ctx, s, am);
    }
    if (!rc) {
        rc = hq::launch_step_lite_jobs(ctx, s, am);
        for (uint32_t x = 0; x < nl && !rc; ++x) runs[live[x]].d->wsum_dirty = false;
        if (!rc) d0->tickets_dirty = false;
    }
    if (!rc) rc = hq::launch_step_jobs(ctx, true, small, am);
    if (!rc) rc = hq::check_hip(ctx, hipEventRecord(d0->ev_t1, s), "event");
    tp[3] = now_ns();
    uint64_t gpu_ns = 0;
    if (!rc) {
        rc = wait_stream(d0, s, "hq_dstep jobs sync");
        if (!rc) gpu_ns = elapsed_ns(d0->ev_t0, d0->ev_t1);
    } else {                      // (a failed launch sequence leaves no copy behind either)
        (void)hipStreamSynchronize(s);
        for (hipStream_t cs : {d0->copy, d0->copy2})
            if (cs) (void)hipStreamSynchronize(cs);
    }
    const uint64_t t1 = now_ns();
    const hq_wait_clock w = d0->last_wait;   // (the one wait, before any job's own re-run)
    int first_rc = HQ_OK;
    for (uint32_t x = 0; x < nl; ++x) {
        Run &r = runs[live[x]];
        r.rc = rc;                // (restore: only the jobs whose pass A was launched)
        r.first = false;
        r.t1 = t1;
        r.t_sub = tp[3];
        r.gpu_ns = gpu_ns;
        rcs[live[x]] = finish(r);
        outs[live[x]].wait = w;
        outs[live[x]].gpu_jobs = nl;
        if (rcs[live[x]] && !first_rc) first_rc = rcs[live[x]];
    }
    if (trace) {
        tp[4] = t1;
        tp[5] = now_ns();
        std::fprintf(stderr, "hq_dstep_run_jobs %u jobs: prepare %.1f us, pointers + table %.1f, "
                             "submit %.1f, wait %.1f, outputs %.1f\n", nl,
                     (tp[1] - tp[0]) / 1e3, (tp[2] - tp[1]) / 1e3, (tp[3] - tp[2]) / 1e3,
                     (tp[4] - tp[3]) / 1e3, (tp[5] - tp[4]) / 1e3);
    }
    return first_rc;
}
