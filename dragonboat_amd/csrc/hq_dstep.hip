// hq_dstep.hip — the resident state of the step worker's device engine (hq_worker_open_ex,
// HQ_WORKER_ON_DEVICE): one worker's groups, members and pending reads in HBM with the staging a
// step needs (struct hq_dstep, hq_dstep_k.h), how they get there and back, the buffers' growth
// and the step thread's wait. (hq_dstep_step.hip, _layout.hip: the kernels; _run.hip: a step.)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <thread>

#include "hq_dstep_k.h"

namespace {

using hq::grow;

// With HQ_WAIT_CLOCK a one-thread kernel behind the step writes the device's constant clock into
// pinned memory: the step's end on the device's clock, against which the host's wake-up is read
__global__ void k_clock_stamp(uint64_t *dst) {
    if (threadIdx.x == 0) *dst = wall_clock64();
}

// The groups' state moves between the worker's own (pageable) vectors and the device through a
// pinned bounce buffer, in halves of kBounce bytes: for a large pageable copy the HIP runtime pins
// the caller's pages in place, and when those pages' mappings later change (the allocator handing
// them back) the driver evicts and restores the process's queues — a device step queued meanwhile
// started 5-24 ms late (profiles/r06l/)
constexpr size_t kBounce = size_t(8) << 20;

int bounce_ready(hq_dstep *d) {
    if (d->bounce) return HQ_OK;
    hq_ctx *ctx = d->ctx;
    int rc = hq::check_hip(ctx, hipHostMalloc(reinterpret_cast<void **>(&d->bounce), 2 * kBounce,
                                              hipHostMallocDefault), "hq_dstep bounce");
    for (hipEvent_t &e : d->bounce_ev)
        if (!rc) rc = hq::check_hip(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming), "event");
    return rc;
}

int put_staged(hq_dstep *d, void *dst, const void *src, size_t bytes, uint64_t *half) {
    hq_ctx *ctx = d->ctx;
    int rc = bounce_ready(d);
    for (size_t off = 0; !rc && off < bytes; off += kBounce, ++*half) {
        const size_t n = std::min(kBounce, bytes - off);
        const int h = (int)(*half & 1);
        char *b = d->bounce + h * kBounce;
        // (the half's previous copy must have read it: its event, recorded behind that copy)
        if (*half >= 2) rc = hq::check_hip(ctx, hipEventSynchronize(d->bounce_ev[h]), "hq_dstep_put");
        if (rc) break;
        std::memcpy(b, static_cast<const char *>(src) + off, n);
        rc = hq::check_hip(ctx, hipMemcpyAsync(static_cast<char *>(dst) + off, b, n,
                                               hipMemcpyHostToDevice, ctx->stream), "hq_dstep_put");
        if (!rc) rc = hq::check_hip(ctx, hipEventRecord(d->bounce_ev[h], ctx->stream), "hq_dstep_put");
    }
    return rc;
}

int get_staged(hq_dstep *d, void *dst, const void *src, size_t bytes) {
    hq_ctx *ctx = d->ctx;
    int rc = bounce_ready(d);
    for (size_t off = 0; !rc && off < bytes; off += kBounce) {
        const size_t n = std::min(kBounce, bytes - off);
        rc = hq::check_hip(ctx, hipMemcpyAsync(d->bounce, static_cast<const char *>(src) + off, n,
                                               hipMemcpyDeviceToHost, ctx->stream), "hq_dstep_get");
        if (!rc) rc = hq::check_hip(ctx, hipStreamSynchronize(ctx->stream), "hq_dstep_get");
        if (!rc) std::memcpy(static_cast<char *>(dst) + off, d->bounce, n);
    }
    return rc;
}

}  // namespace

namespace hq {

int grow(hq_ctx *ctx, void **p, size_t *cap, size_t need, bool keep, const char *what) {
    if (need <= *cap) return HQ_OK;
    size_t want = need + need / 2;
    // HQ_GROW_TRACE=1: each device regrowth on stderr (a hipMalloc + hipFree in a step's
    // submission: the device synchronizes for the free)
    static const bool trace = env_flag("HQ_GROW_TRACE");
    if (trace)
        std::fprintf(stderr, "[hq grow] %s %zu -> %zu bytes at %.3f ms\n", what, *cap, want,
                     now_ns() / 1e6);
    void *n = nullptr;
    int rc = hq::check_hip(ctx, hipMalloc(&n, want), what);
    if (rc) return rc;
    if (*p && keep) rc = hq::check_hip(ctx, hipMemcpyAsync(n, *p, *cap, hipMemcpyDeviceToDevice,
                                                           ctx->stream), what);
    if (!rc) rc = hq::check_hip(ctx, hipStreamSynchronize(ctx->stream), what);
    if (*p) (void)hipFree(*p);
    *p = n;
    *cap = want;
    return rc;
}

int stamp_clock(hq_dstep *d, hipStream_t s, int slot) {
    d->clock_host[slot] = 0;
    hipLaunchKernelGGL(k_clock_stamp, dim3(1), dim3(64), 0, s, d->clock_host + slot);
    return check_hip(d->ctx, hipGetLastError(), "k_clock_stamp");
}

// Wait for a stream on the step's thread, as d's policy says (hq_dstep_set_wait), its clock in
// d->last_wait:
//   HQ_WAIT_BLOCK  poll for poll_us, then sleep on a blocking-sync event (the runtime's interrupt
//                  wait): 16 workers waiting at once do not spin 16 host cores (a spinning wait
//                  under a CPU quota stalls every thread of the process for the rest of the
//                  period)
//   HQ_WAIT_SLEEP  poll for poll_us, then query the event every sleep_us, asleep in between (a
//                  timer wake-up: its lateness is bounded by the timer's slack, not by the
//                  runtime's interrupt path)
//   HQ_WAIT_SPIN   poll with yields until done (a core held for the step)
//   HQ_WAIT_ADAPT  one timed sleep until max(poll_us, 100) before the end the last step's wait
//                  predicts (its length from the wait's start to the step seen done), then poll
//                  with yields: a spinning wait's lateness for ~100 us of a core per step; past
//                  twice the prediction (+ 1 ms) it sleeps on the blocking-sync event
int wait_stream(hq_dstep *d, hipStream_t s, const char *what) {
    hq_ctx *ctx = d->ctx;
    hq_wait_clock &wc = d->last_wait;
    wc = hq_wait_clock{};
    int rc = HQ_OK;
    if (d->wait_clock) rc = stamp_clock(d, s, 0);
    if (!rc) rc = hq::check_hip(ctx, hipEventRecord(d->ev_sync, s), what);
    if (rc) return rc;
    const uint32_t mode = d->wait_mode;
    const uint32_t poll_us = d->wait_poll_us;
    const uint64_t t0 = now_ns();
    wc.t_begin_ns = t0;
    auto done = [&](int r) {
        wc.t_end_ns = now_ns();
        if (d->wait_clock && !r) {
            wc.device_end_ticks = d->clock_host[0];
            wc.device_start_ticks = d->clock_host[1];
        }
        return r;
    };
    if (mode == HQ_WAIT_ADAPT && d->wait_pred_ns) {
        const uint64_t pred = d->wait_pred_ns;
        const uint64_t margin = (uint64_t)std::max<uint32_t>(poll_us, 100) * 1000;
        if (pred > margin) {
            std::this_thread::sleep_for(std::chrono::nanoseconds(pred - margin));
            wc.sleeps = 1;
            wc.sleep_ns = now_ns() - t0;
        }
        const uint64_t t1 = now_ns();
        for (uint32_t k = 0;; ++k) {
            const hipError_t q = hipEventQuery(d->ev_sync);
            if (q == hipSuccess) {
                wc.poll_ns = now_ns() - t1;
                d->wait_pred_ns = now_ns() - t0;
                return done(HQ_OK);
            }
            if (q != hipErrorNotReady) return done(hq::check_hip(ctx, q, what));
            if (now_ns() - t0 > 2 * pred + 1000000) break;    // far past the prediction
            if ((k & 15) == 15) std::this_thread::yield();
        }
        const uint64_t t2 = now_ns();
        wc.poll_ns = t2 - t1;
        ++wc.sleeps;
        rc = hq::check_hip(ctx, hipEventSynchronize(d->ev_sync), what);
        wc.sleep_ns += now_ns() - t2;
        if (!rc) d->wait_pred_ns = now_ns() - t0;
        return done(rc);
    }
    for (uint32_t k = 0;; ++k) {
        const hipError_t q = hipEventQuery(d->ev_sync);
        if (q == hipSuccess) {
            wc.poll_ns = now_ns() - t0;
            return done(HQ_OK);
        }
        if (q != hipErrorNotReady) return done(hq::check_hip(ctx, q, what));
        if (mode != HQ_WAIT_SPIN && now_ns() - t0 > (uint64_t)poll_us * 1000) break;
        if ((mode == HQ_WAIT_SPIN || poll_us > 50) && (k & 15) == 15) std::this_thread::yield();
    }
    const uint64_t t1 = now_ns();
    wc.poll_ns = t1 - t0;
    if (mode == HQ_WAIT_SLEEP) {
        for (;;) {
            std::this_thread::sleep_for(std::chrono::microseconds(d->wait_sleep_us));
            ++wc.sleeps;
            const hipError_t q = hipEventQuery(d->ev_sync);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) return done(hq::check_hip(ctx, q, what));
        }
        wc.sleep_ns = now_ns() - t1;
        return done(HQ_OK);
    }
    wc.sleeps = 1;
    rc = hq::check_hip(ctx, hipEventSynchronize(d->ev_sync), what);
    wc.sleep_ns = now_ns() - t1;
    if (!rc) d->wait_pred_ns = now_ns() - t0;   // (HQ_WAIT_ADAPT's first step)
    return done(rc);
}

}  // namespace hq

namespace {

// The per-group arrays grown to hold `need` records: groups, reads and stamps with their contents,
// the saved-state buffers (they only live within a step) without.
int grow_groups(hq_dstep *d, uint64_t need) {
    if (need <= d->gcap) return HQ_OK;
    hq_ctx *ctx = d->ctx;
    size_t gc = d->gcap * sizeof(hq_dgroup), rcap = d->gcap * kDReads * sizeof(hq_dread);
    int rc = grow(ctx, &d->groups, &gc, need * sizeof(hq_dgroup), true, "hq_dstep groups");
    if (!rc) rc = grow(ctx, &d->reads, &rcap, need * kDReads * sizeof(hq_dread), true, "hq_dstep reads");
    size_t sc = d->gcap * 4;
    if (!rc) rc = grow(ctx, &d->stamp, &sc, need * 4, true, "hq_dstep stamps");
    size_t gn = d->gcap * sizeof(hq_dgroup), rn = d->gcap * kDReads * sizeof(hq_dread);
    if (!rc) rc = grow(ctx, &d->groups_old, &gn, need * sizeof(hq_dgroup), false, "hq_dstep saved groups");
    if (!rc)
        rc = grow(ctx, &d->reads_old, &rn, need * kDReads * sizeof(hq_dread), false, "hq_dstep saved reads");
    if (!rc) d->gcap = std::min({gc / sizeof(hq_dgroup), rcap / (kDReads * sizeof(hq_dread)),
                                 sc / 4, gn / sizeof(hq_dgroup),
                                 rn / (kDReads * sizeof(hq_dread))});
    return rc;
}

}  // namespace

int hq_dstep_set_wait(hq_dstep *d, uint32_t mode, uint32_t poll_us, uint32_t sleep_us) {
    const uint32_t m = mode & ~HQ_WAIT_CLOCK;
    if (m != HQ_WAIT_BLOCK && m != HQ_WAIT_SLEEP && m != HQ_WAIT_SPIN && m != HQ_WAIT_ADAPT)
        return HQ_E_INVAL;
    if (m == HQ_WAIT_SLEEP && sleep_us == 0) return HQ_E_INVAL;
    if ((mode & HQ_WAIT_CLOCK) && !d->clock_host) {
        int rc = hq::check_hip(d->ctx, hipHostMalloc(&d->clock_host, 64, hipHostMallocDefault),
                               "hq_dstep clock");
        if (rc) return rc;
    }
    d->wait_mode = m;
    d->wait_poll_us = poll_us;
    d->wait_sleep_us = sleep_us;
    d->wait_clock = (mode & HQ_WAIT_CLOCK) != 0;
    return HQ_OK;
}

int hq_dstep_open(hq_ctx *ctx, hq_dstep **out, uint32_t commit_column) {
    *out = new (std::nothrow) hq_dstep();
    if (!*out) return HQ_E_NOMEM;
    hq_dstep *d = *out;
    d->ctx = ctx;
    d->commit_column = commit_column;
    d->test_fail_regrow = hq::env_flag("HQ_TEST_FAIL_REGROW");
    d->test_scan_fail = hq::env_flag("HQ_TEST_SCAN_FAIL");
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc)
        rc = hq::check_hip(ctx, hipEventCreateWithFlags(&d->ev_sync, hipEventDisableTiming |
                                                                          hipEventBlockingSync),
                           "event");
    for (hipEvent_t *e : {&d->ev_t0, &d->ev_t1})
        if (!rc) rc = hq::check_hip(ctx, hipEventCreate(e), "event");
    for (int c = 0; c < kMaxJobChunks && !rc; ++c) {
        rc = hq::check_hip(ctx, hipEventCreateWithFlags(&d->ev_in[c], hipEventDisableTiming), "event");
        if (!rc)
            rc = hq::check_hip(ctx, hipEventCreateWithFlags(&d->ev_in2[c], hipEventDisableTiming),
                               "event");
    }
    if (!rc) rc = hq::check_hip(ctx, hipMalloc(&d->layout, sizeof(Layout)), "hq_dstep layout");
    if (!rc) rc = hq::check_hip(ctx, hipMalloc(&d->tickets, kTickets * 4), "hq_dstep tickets");
    if (!rc) rc = hq::check_hip(ctx, hipMemset(d->tickets, 0, kTickets * 4), "hq_dstep tickets");
    if (!rc)
        rc = hq::check_hip(ctx, hipHostMalloc(&d->host_layout, sizeof(Layout), hipHostMallocDefault),
                           "hq_dstep layout");
    if (rc) {
        hq_dstep_close(d);
        *out = nullptr;
    }
    return rc;
}

void hq_dstep_close(hq_dstep *d) {
    if (!d) return;
    (void)hipSetDevice(d->ctx->device);
    (void)hipStreamSynchronize(d->ctx->stream);
    for (void *p : {(void *)d->groups, (void *)d->reads, (void *)d->members, (void *)d->stamp, d->in,
                    (void *)d->counts, (void *)d->scan, (void *)d->bases, d->scan_tmp,
                    (void *)d->layout, (void *)d->groups_old, (void *)d->reads_old,
                    (void *)d->match_old, (void *)d->rerun, (void *)d->ready_slot,
                    (void *)d->rerun_list, (void *)d->wsum, (void *)d->jobs_dev,
                    (void *)d->tickets, (void *)d->tiles})
        if (p) (void)hipFree(p);
    if (d->host_out) (void)hipHostFree(d->host_out);
    if (d->jobs_host) (void)hipHostFree(d->jobs_host);
    if (d->host_layout) (void)hipHostFree(d->host_layout);
    if (d->clock_host) (void)hipHostFree(d->clock_host);
    if (d->bounce) (void)hipHostFree(d->bounce);
    for (hipEvent_t e : d->bounce_ev)
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t cs : {d->copy, d->copy2}) {
        if (cs) {
            (void)hipStreamSynchronize(cs);
            (void)hipStreamDestroy(cs);
        }
    }
    for (hipEvent_t e : {d->ev_sync, d->ev_t0, d->ev_t1})
        if (e) (void)hipEventDestroy(e);
    for (int c = 0; c < kMaxJobChunks; ++c) {
        if (d->ev_in[c]) (void)hipEventDestroy(d->ev_in[c]);
        if (d->ev_in2[c]) (void)hipEventDestroy(d->ev_in2[c]);
    }
    delete d;
}

int hq_dstep_put(hq_dstep *d, uint64_t g0, uint64_t ng, const hq_dgroup *g, const hq_dread *r,
                 uint64_t m0, uint64_t nm, const hq_dmember *m) {
    hq_ctx *ctx = d->ctx;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    size_t mc = d->mcap * sizeof(hq_dmember);
    if (!rc) rc = grow_groups(d, g0 + ng);
    for (uint64_t i = 0; i < ng; ++i)
        if (g[i].n_members > d->max_members) d->max_members = g[i].n_members;
    if (!rc && ng) {              // new stamps start at 0 (no step has listed them)
        rc = hq::check_hip(ctx, hipMemsetAsync(d->stamp + g0, 0, ng * 4, ctx->stream), "memset");
        if (!rc && g0 + ng > d->n_groups) d->n_groups = g0 + ng;
    }
    if (!rc && (m0 + nm) > d->mcap) {
        size_t xn = d->mcap * 8;
        rc = grow(ctx, &d->members, &mc, (m0 + nm) * sizeof(hq_dmember), true, "hq_dstep members");
        if (!rc) rc = grow(ctx, &d->match_old, &xn, (m0 + nm) * 8, false, "hq_dstep saved matches");
        if (!rc) d->mcap = std::min(mc / sizeof(hq_dmember), xn / 8);
    }
    uint64_t half = 0;
    if (!rc && ng) rc = put_staged(d, d->groups + g0, g, ng * sizeof(hq_dgroup), &half);
    if (!rc && ng) rc = put_staged(d, d->reads + g0 * kDReads, r, ng * kDReads * sizeof(hq_dread), &half);
    if (!rc && nm) rc = put_staged(d, d->members + m0, m, nm * sizeof(hq_dmember), &half);
    if (!rc) rc = hq::check_hip(ctx, hipStreamSynchronize(ctx->stream), "hq_dstep_put");
    return rc;
}

int hq_dstep_get(hq_dstep *d, uint64_t ng, hq_dgroup *g, hq_dread *r, uint64_t nm, hq_dmember *m) {
    hq_ctx *ctx = d->ctx;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc && ng) rc = get_staged(d, g, d->groups, ng * sizeof(hq_dgroup));
    if (!rc && ng) rc = get_staged(d, r, d->reads, ng * kDReads * sizeof(hq_dread));
    if (!rc && nm) rc = get_staged(d, m, d->members, nm * sizeof(hq_dmember));
    return rc;
}

void hq_dstep_view(hq_dstep *d, hq_dstate_view *out) {
    *out = hq_dstate_view{d->ctx, d->groups, d->reads, d->members, d->n_groups};
}

void hq_dstep_view_mut(hq_dstep *d, hq_dstate_mut *out) {
    *out = hq_dstate_mut{d->ctx, d->groups, d->reads, d->members, d->n_groups};
}

int hq_dstep_reserve_members(hq_dstep *d, uint64_t m0, uint64_t total) {
    hq_ctx *ctx = d->ctx;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc && total > d->mcap) {
        size_t mc = d->mcap * sizeof(hq_dmember), xn = d->mcap * 8;
        rc = grow(ctx, &d->members, &mc, total * sizeof(hq_dmember), true, "hq_dstep members");
        if (!rc) rc = grow(ctx, &d->match_old, &xn, total * 8, false, "hq_dstep saved matches");
        if (!rc) d->mcap = std::min(mc / sizeof(hq_dmember), xn / 8);
    }
    if (!rc && total > m0)
        rc = hq::check_hip(ctx, hipMemsetAsync(d->members + m0, 0, (total - m0) * sizeof(hq_dmember),
                                               ctx->stream), "hq_dstep members");
    return rc;
}

int hq_dstep_reserve_groups(hq_dstep *d, uint64_t total) {
    hq_ctx *ctx = d->ctx;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc || total <= d->n_groups) return rc;
    rc = grow_groups(d, total);
    if (!rc)                      // new stamps start at 0 (no step has listed them)
        rc = hq::check_hip(ctx, hipMemsetAsync(d->stamp + d->n_groups, 0, (total - d->n_groups) * 4,
                                               ctx->stream), "memset");
    if (!rc) d->n_groups = total;
    return rc;
}

int hq_dstep_members_spare(hq_dstep *d, hq_dmember **spare, uint64_t *capacity) {
    hq_ctx *ctx = d->ctx;
    *spare = nullptr;
    *capacity = d->mcap;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc || d->mcap == 0) return rc;
    return hq::check_hip(ctx, hipMalloc(reinterpret_cast<void **>(spare), d->mcap * sizeof(hq_dmember)),
                         "hq_dstep members (compaction)");
}

void hq_dstep_members_install(hq_dstep *d, hq_dmember *spare) {
    if (!spare) return;
    (void)hipSetDevice(d->ctx->device);
    if (d->members) (void)hipFree(d->members);
    d->members = spare;
}

void hq_dstep_members_drop(hq_dstep *d, hq_dmember *spare) {
    (void)hipSetDevice(d->ctx->device);
    if (spare) (void)hipFree(spare);
}

void hq_dstep_raise_max_members(hq_dstep *d, uint32_t n) {
    if (n > d->max_members) d->max_members = n;
}
