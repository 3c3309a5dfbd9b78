// hq_stream16.cpp — the event stream from 16-byte compact records (hq_event16): the encoder a
// producer holding records calls, on one thread or on the task pool's, and the pool's clocks.
// No exception leaves an entry: hq_events16_encode_sized and _multi run in hq::guard and answer
// with the code alone (they have no handle to keep a message in); hq_encode_stats_read allocates
// nothing and stays bare.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/hipquorum.h"
#include "hq_guard.h"
#include "hq_stream_k.h"
#include "hq_task_pool.h"

namespace {

using namespace hqs;

// The event a compact record stands for. rc: records taken (1, or 5 for an escape), 0 when a
// record is malformed (an escape without its 4 records). ctx: the group's latest READ ctx.
inline int from16(const hq_event16 *r, uint64_t left, uint64_t ctx[2], hq_event &e) {
    if (r->kind & HQ_EV16_FULL) {
        if (left < 5) return 0;
        std::memcpy(&e, r + 1, sizeof e);
        if (e.kind == HQ_EV_READ) {
            ctx[0] = e.hint;
            ctx[1] = e.hint_high;
        }
        return 5;
    }
    e = hq_event{};
    e.kind = r->kind & 7;
    e.reject = (r->kind >> 3) & 1;
    if (e.kind == HQ_EV_READ) {
        e.hint = ctx[0] = r->value;
        e.hint_high = ctx[1] = r->term;
    } else if (e.kind == HQ_EV_PROPOSE) {
        e.log_index = r->value;
    } else if (e.kind == HQ_EV_MESSAGE) {
        e.type = r->type;
        e.from = r->from;
        e.term = r->term;
        if (e.type == HQ_MSG_HEARTBEAT_RESP || e.type == HQ_MSG_READ_INDEX) {
            if (r->kind & HQ_EV16_READ_CTX) {
                e.hint = ctx[0];
                e.hint_high = ctx[1];
            } else {
                e.hint = r->value;
            }
        } else {
            e.log_index = r->value;
        }
    }
    return 1;
}

// type_code of the types below 32
constexpr uint8_t kCode16[32] = {7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 0, 7, 1,
                                 7, 7, 2, 3, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7};
static_assert(HQ_MSG_REPLICATE_RESP == 13 && HQ_MSG_REQUEST_VOTE_RESP == 15 &&
                  HQ_MSG_HEARTBEAT_RESP == 18 && HQ_MSG_READ_INDEX == 19,
              "kCode16 follows the message type numbers");

// one compact record (not an escape) straight into bytes: encode() of the event from16() makes
// of it, without the row
__attribute__((always_inline)) inline uint8_t *encode16(uint8_t *p, const hq_event16 &r, Prev &pv,
                                                       uint64_t ctx[2]) {
    const uint32_t k = r.kind & 7;
    if (k != HQ_EV_MESSAGE) {
        const uint32_t kind = k >= 1 && k <= 5 ? k : 0;
        *p++ = (uint8_t)kind;
        if (kind == HQ_EV_READ) {
            ctx[0] = r.value;
            ctx[1] = r.term;
            p = put(p, r.value);
            p = put_fast(p, r.term);
        } else if (kind == HQ_EV_PROPOSE) {
            p = put_fast(p, r.value);
        }
        return p;
    }
    uint32_t code = r.type < 32 ? kCode16[r.type] : 7u;
    uint64_t hint = 0, high = 0;
    if (code == 0) {
        if (pv.have_index && r.value == pv.index) code = 4;
        pv.index = r.value;
        pv.have_index = true;
    } else if (code == 2 || code == 3) {
        if (r.kind & HQ_EV16_READ_CTX) {
            hint = ctx[0];
            high = ctx[1];
        } else {
            hint = r.value;
        }
        if (code == 2) {
            if (hint == pv.hint && high == pv.high) code = 5;
            pv.hint = hint;
            pv.high = high;
        }
    }
    const bool same = r.term == pv.term;
    pv.last = last_of(code);
    pv.last_reject = (r.kind & 8) ? 1 : 0;
    const uint32_t hdr =
        HQ_EV_MESSAGE | code << 3 | ((r.kind & 8) ? 0x40u : 0u) | (same ? 0x80u : 0u);
    if (code != 7 && r.from < 0x80) {   // header and a 1-byte sender in one store
        const uint16_t w = (uint16_t)(hdr | (uint32_t)r.from << 8);
        std::memcpy(p, &w, 2);
        p += 2;
    } else {
        *p++ = (uint8_t)hdr;
        if (code == 7) p = put(p, r.type);
        p = put_fast(p, r.from);
    }
    if (!same) p = put(p, r.term);
    pv.term = r.term;
    if (code == 0 || code == 7) p = put_fast(p, r.value);
    if (code == 2 || code == 3 || code == 7) {
        p = put(p, hint);
        p = put_fast(p, high);
    }
    return p;
}

// does record r (not an escape) repeat the group's previous message? (repeats() of the event
// from16 makes of it, without the row)
__attribute__((always_inline)) inline bool repeats16(const hq_event16 &r, const Prev &pv,
                                                    const uint64_t ctx[2]) {
    if (!pv.last || (r.kind & 7) != HQ_EV_MESSAGE || ((r.kind >> 3) & 1) != pv.last_reject ||
        r.term != pv.term)
        return false;
    if (pv.last == 1) return r.type == HQ_MSG_REPLICATE_RESP && r.value == pv.index;
    if (r.type != HQ_MSG_HEARTBEAT_RESP) return false;
    return (r.kind & HQ_EV16_READ_CTX) ? ctx[0] == pv.hint && ctx[1] == pv.high
                                       : r.value == pv.hint && pv.high == 0;
}

// the records recs[k .. r1) that open with a run: its length (0 below kRunMin), the senders in
// from[] and the records it takes in *used (an escaped event is 5 records)
inline uint32_t run16(const hq_event16 *recs, uint64_t k, uint64_t r1, const Prev &pv,
                      const uint64_t ctx[2], uint64_t from[kRunMax], uint64_t *used) {
    uint32_t m = 0;
    uint64_t q = k;
    while (m < kRunMax && q < r1) {
        const hq_event16 &r = recs[q];
        if (r.kind & HQ_EV16_FULL) {      // an escaped event: its row
            if (r1 - q < 5) break;
            hq_event e;
            std::memcpy(&e, &r + 1, sizeof e);
            if (!repeats(e, pv)) break;
            from[m++] = e.from;
            q += 5;
            continue;
        }
        if (!repeats16(r, pv, ctx)) break;
        from[m++] = r.from;
        ++q;
    }
    *used = q - k;
    return m >= kRunMin ? m : 0;
}

// groups [g0, g1) encoded at out (cap bytes), or into a growing scratch (grow != nullptr) from
// its byte pos0 on (a thread's later pieces follow its earlier ones there); the range's event
// count and byte count out, its last event's start relative to the range's first byte (locals
// until the end: threads encoding neighbouring ranges share no written cache line but their ends
// of `sizes`)
int enc16_range(const uint64_t *off, const hq_event16 *recs, uint32_t *sizes, uint64_t g0,
                uint64_t g1, std::vector<uint8_t> *grow, uint8_t *out, uint64_t cap,
                uint64_t *n_events, uint64_t *n_bytes, uint64_t *last_start = nullptr,
                uint64_t pos0 = 0, uint16_t *sizes16 = nullptr) {
    uint64_t pos = pos0, events = 0, ls = ~0ull;
    uint8_t *base = grow ? grow->data() : out;
    for (uint64_t i = g0; i < g1; ++i) {
        const uint64_t r0 = off[i], r1 = off[i + 1];
        if (r1 < r0) return HQ_E_INVAL;
        // room for the group's records at HQ_EVENT_STREAM_MAX each: no check per event
        const uint64_t need = (r1 - r0) * HQ_EVENT_STREAM_MAX;
        if (grow && grow->size() < pos + need) {
            grow->resize(std::max<size_t>(2 * grow->size(), pos + need + (1 << 20)));
            base = grow->data();
        }
        const bool roomy = grow || (cap >= pos && cap - pos >= need);
        const uint64_t p0 = pos;
        uint64_t ne = 0, ctx[2] = {0, 0};
        Prev pv;
        uint8_t *p = base + pos;
        uint8_t *lp = nullptr;
        for (uint64_t k = r0; k < r1; ++ne) {
            if (!roomy && (cap < (uint64_t)(p - base) || cap - (uint64_t)(p - base) <
                                                             HQ_EVENT_STREAM_MAX))
                return HQ_E_STATE;
            lp = p;
            if (pv.last) {                  // the next events repeat the previous message: a run
                uint64_t from[kRunMax], used = 0;
                const uint32_t m = run16(recs, k, r1, pv, ctx, from, &used);
                if (m) {
                    p = put_run(p, m, [&](uint32_t j) { return from[j]; });
                    k += used;
                    ne += m - 1;
                    continue;
                }
            }
            if (!(recs[k].kind & HQ_EV16_FULL)) {
                p = encode16(p, recs[k], pv, ctx);
                ++k;
                continue;
            }
            hq_event e;
            const int used = from16(recs + k, r1 - k, ctx, e);
            if (!used) return HQ_E_INVAL;
            k += used;
            p = encode(p, e, pv);
        }
        pos = (uint64_t)(p - base);
        if (lp) ls = (uint64_t)(lp - base) - pos0;
        if (ne > 0xFFFF || pos - p0 > 0xFFFF) return HQ_E_INVAL;
        if (sizes16) sizes16[i] = (uint16_t)(pos - p0);   // (2-byte words: bytes only)
        else sizes[i] = (uint32_t)ne | (uint32_t)(pos - p0) << 16;
        events += ne;
    }
    *n_events = events;
    *n_bytes = pos - pos0;
    if (last_start) *last_start = ls;
    return HQ_OK;
}

// a pool thread's encode scratch is kept for its next call (first touched on its memory node),
// unless a call grew it past kKeepScratch: then it is released
constexpr size_t kKeepScratch = size_t(256) << 20;
// hq_events16_encode_sized_multi: chunks per encode thread, taken from a shared counter (against
// one range per thread, the static split: profiles/r06v)
constexpr uint64_t kChunksPerThread = 8;

// the call failed as a whole (an exception on one of its threads, or before them): every live
// job answers with the code and nothing encoded
void fail_live(hq_encode16_job *jobs, uint32_t count, int code) {
    for (uint32_t j = 0; j < count; ++j) {
        hq_encode16_job &b = jobs[j];
        if (b.rc || !b.n_groups) continue;
        b.rc = code;
        b.n_events = b.n_bytes = 0;
    }
}

int encode_multi(hq_encode16_job *jobs, uint32_t count, uint32_t threads) {
    // each job checked as its own call would; the records of the valid ones laid end to end
    std::vector<uint64_t> rec0(count + 1, 0);
    std::vector<uint32_t> live;
    live.reserve(count);
    int first = HQ_OK;
    for (uint32_t j = 0; j < count; ++j) {
        hq_encode16_job &b = jobs[j];
        const uint64_t n = b.n_groups;
        if (!b.offsets16 || (n && !b.sizes && !b.sizes16) ||
            (n && b.offsets16[n] > b.offsets16[0] && !b.recs))
            b.rc = HQ_E_INVAL;
        else if (n && b.offsets16[n] > b.offsets16[0] && !b.out)
            b.rc = HQ_E_STATE;
        else if (n && b.offsets16[n] < b.offsets16[0])
            b.rc = HQ_E_INVAL;
        rec0[j + 1] = rec0[j] + (b.rc || !n ? 0 : b.offsets16[n] - b.offsets16[0]);
        if (!b.rc && n) live.push_back(j);
        if (b.rc && !first) first = b.rc;
    }
    const uint64_t R = rec0[count];
    const uint32_t T = (uint32_t)std::min<uint64_t>(
        {std::max(threads, 1u), std::max<uint64_t>(1, R / 4096), TaskPool::kMaxThreads + 1});
    if (live.empty()) return first;
    const uint64_t c0 = now_ns();
    // C chunks of about equal records, taken by the T threads from a shared counter: a thread
    // slowed by its core (a busy SMT sibling or a crowded host) takes fewer chunks instead of
    // holding the call back by a whole 1/T share
    const uint32_t C = (uint32_t)std::min<uint64_t>((uint64_t)T * kChunksPerThread,
                                                    std::max<uint64_t>(T, R / 4096));
    // job j's groups split at the global record cuts R c / C (group boundaries): chunk c of the
    // job is groups [gc[j][c], gc[j][c + 1]), empty unless the job's records meet chunk c
    std::vector<std::vector<uint64_t>> gc(count);
    for (uint32_t j : live) {
        const hq_encode16_job &b = jobs[j];
        std::vector<uint64_t> &c = gc[j];
        c.assign(C + 1, 0);
        c[C] = b.n_groups;
        for (uint32_t t = 1; t < C; ++t) {
            const uint64_t cut = R * t / C;
            const uint64_t rel = cut <= rec0[j] ? 0 : std::min(cut - rec0[j], rec0[j + 1] - rec0[j]);
            const uint64_t want = b.offsets16[0] + rel;
            const uint64_t g = (uint64_t)(std::lower_bound(b.offsets16, b.offsets16 + b.n_groups, want) -
                                          b.offsets16);
            c[t] = std::min<uint64_t>(std::max<uint64_t>(c[t - 1], g), b.n_groups);
        }
    }
    struct Piece {
        uint32_t job, thread;                          // thread: whose scratch holds it
        uint64_t at, events, bytes, last_start, dst;   // at: offset in that scratch; dst: in out
        int rc;
    };
    // Everything the threads and the barrier's last arriver write is allocated here, before the
    // pool is entered: per chunk room for one piece per live job, per job its total and its
    // last event's start. Past this line only a thread's scratch can grow.
    std::vector<std::vector<Piece>> pieces(C);
    for (auto &ps : pieces) ps.reserve(live.size());
    std::vector<uint64_t> total(count, 0), last(count, ~0ull);
    std::vector<uint8_t> fits(count, 1);
    std::atomic<uint32_t> next{0};
    std::atomic<int> failed{HQ_OK};                    // the call's: the first thread's exception
    std::mutex bm;
    std::condition_variable bcv;
    uint32_t arrived = 0;
    uint64_t c1 = 0;
    const int prc = task_pool().parallel_for(T, [&](uint32_t t) {
        thread_local std::vector<uint8_t> scratch;
        // the encode phase catches: whatever happens, the thread arrives at the barrier
        const int erc = hq::guard("hq_events16_encode_sized_multi", [&] {
            uint64_t pos = 0;
            for (;;) {
                const uint32_t c = next.fetch_add(1, std::memory_order_relaxed);
                if (c >= C) break;
                std::vector<Piece> &ps = pieces[c];
                for (uint32_t j : live) {
                    const uint64_t g0 = gc[j][c], g1 = gc[j][c + 1];
                    if (g0 >= g1) continue;
                    const hq_encode16_job &b = jobs[j];
                    Piece pc{j, t, pos, 0, 0, ~0ull, 0, HQ_OK};
                    // (the piece follows the thread's earlier pieces in its scratch)
                    pc.rc = enc16_range(b.offsets16, b.recs, b.sizes, g0, g1, &scratch, nullptr, 0,
                                        &pc.events, &pc.bytes, &pc.last_start, pos, b.sizes16);
                    if (pc.rc) pc.bytes = 0;
                    pos += pc.bytes;
                    ps.push_back(pc);
                }
            }
            return HQ_OK;
        });
        if (erc) {
            int none = HQ_OK;
            failed.compare_exchange_strong(none, erc);
        }
        {
            std::unique_lock<std::mutex> lk(bm);
            if (++arrived == T) {
                // every piece in: each job's totals, its capacity rule and its pieces' places
                c1 = now_ns();
                for (uint32_t u = 0; u < C && !failed; ++u) {   // (chunk order: each job's byte order)
                    for (Piece &pc : pieces[u]) {
                        hq_encode16_job &b = jobs[pc.job];
                        if (pc.rc && !b.rc) b.rc = pc.rc;
                        if (pc.last_start != ~0ull) last[pc.job] = total[pc.job] + pc.last_start;
                        pc.dst = total[pc.job];
                        total[pc.job] += pc.bytes;
                        b.n_events += pc.events;
                    }
                }
                for (uint32_t j : live) {
                    hq_encode16_job &b = jobs[j];
                    fits[j] = last[j] == ~0ull ||
                              (b.cap >= last[j] && b.cap - last[j] >= HQ_EVENT_STREAM_MAX);
                    if (!b.rc && !fits[j]) b.rc = HQ_E_STATE;
                    b.n_bytes = b.rc ? 0 : total[j];
                    if (b.rc) b.n_events = 0;
                }
                bcv.notify_all();
            } else {
                bcv.wait(lk, [&] { return arrived == T; });
            }
        }
        if (failed) {                                   // nobody copies; the scratch goes
            std::vector<uint8_t>().swap(scratch);
            return;
        }
        for (uint32_t c = 0; c < C; ++c)                // the pieces this thread encoded
            for (const Piece &pc : pieces[c]) {
                const hq_encode16_job &b = jobs[pc.job];
                if (pc.thread == t && !b.rc && pc.bytes)
                    std::memcpy(b.out + pc.dst, scratch.data() + pc.at, pc.bytes);
            }
        if (scratch.capacity() > kKeepScratch) std::vector<uint8_t>().swap(scratch);
    }, true);
    if (const int rc = prc ? prc : failed.load()) {     // (nothing encoded)
        fail_live(jobs, count, rc);
        return rc;
    }
    first = HQ_OK;
    for (uint32_t j = 0; j < count && !first; ++j) first = jobs[j].rc;
    const uint64_t c2 = now_ns();
    g_clk.calls++;
    g_clk.encode_ns += c1 - c0;
    g_clk.copy_ns += c2 - c1;
    g_clk.wall_ns += c2 - c0;
    return first;
}

}  // namespace

extern "C" {

int hq_events16_encode_sized(uint64_t n_groups, const uint64_t *offsets16, const hq_event16 *recs,
                             uint8_t *out, uint64_t cap, uint32_t *sizes, uint64_t *n_events,
                             uint64_t *n_bytes, uint32_t threads) {
    if (!offsets16 || !n_events || !n_bytes || (n_groups && !sizes) ||
        (n_groups && offsets16[n_groups] > offsets16[0] && !recs))
        return HQ_E_INVAL;
    *n_events = *n_bytes = 0;
    return hq::guard("hq_events16_encode_sized", [&] {
        if (n_groups && offsets16[n_groups] > offsets16[0] && !out) return HQ_E_STATE;
        const uint64_t nrec = n_groups ? offsets16[n_groups] - offsets16[0] : 0;
        const uint32_t T = (uint32_t)std::min<uint64_t>(
            {std::max(threads, 1u), std::max<uint64_t>(1, nrec / 4096), TaskPool::kMaxThreads + 1});
        // one thread encodes straight into out (through a scratch of its own it was slower: 59
        // against 38 ms for the step5 producer on one fresh thread, profiles/r05b/enc_probe.log)
        if (T <= 1)
            return enc16_range(offsets16, recs, sizes, 0, n_groups, nullptr, out, cap, n_events,
                               n_bytes);
        // the threads take chunks of the records as hq_events16_encode_sized_multi does (one job):
        // each chunk encoded into the taking thread's own scratch (first touched, so held on its
        // memory node, and reused by later calls), then copied into place once every chunk's byte
        // count is known (scratch handed from thread to thread ran the encode 2.5 x slower per record
        // on a 256-CPU host, profiles/r05b/enc_probe.log)
        hq_encode16_job job{};
        job.n_groups = n_groups;
        job.offsets16 = offsets16;
        job.recs = recs;
        job.out = out;
        job.cap = cap;
        job.sizes = sizes;
        const int rc = hq_events16_encode_sized_multi(&job, 1, T);
        if (rc) return rc;
        *n_events = job.n_events;
        *n_bytes = job.n_bytes;
        return HQ_OK;
    });
}

// After an exception (HQ_E_NOMEM: a thread's scratch, the call's own tables or a pool thread
// could not be had; by hq_guard.h's table) every live job's rc is that code with n_events and
// n_bytes 0; `out` and `sizes` may hold parts of an encode and mean nothing. The pool and the
// other callers' calls are untouched and the next call starts clean.
int hq_events16_encode_sized_multi(hq_encode16_job *jobs, uint32_t count, uint32_t threads) {
    if (count && !jobs) return HQ_E_INVAL;
    for (uint32_t j = 0; j < count; ++j) {
        jobs[j].n_events = jobs[j].n_bytes = 0;
        jobs[j].rc = HQ_OK;
    }
    bool returned = false;
    const int rc = hq::guard("hq_events16_encode_sized_multi", [&] {
        const int first = encode_multi(jobs, count, threads);
        returned = true;
        return first;
    });
    if (!returned) fail_live(jobs, count, rc);
    return rc;
}

int hq_encode_stats_read(hq_encode_stats *out, int reset) {
    if (!out) return HQ_E_INVAL;
    auto take = [&](std::atomic<uint64_t> &a) { return reset ? a.exchange(0) : a.load(); };
    out->calls = take(g_clk.calls);
    out->tasks = take(g_clk.tasks);
    out->helped = take(g_clk.helped);
    out->wall_ns = take(g_clk.wall_ns);
    out->encode_ns = take(g_clk.encode_ns);
    out->copy_ns = take(g_clk.copy_ns);
    out->lag_ns = take(g_clk.lag_ns);
    out->max_lag_ns = take(g_clk.max_lag_ns);
    out->run_ns = take(g_clk.run_ns);
    return HQ_OK;
}

}  // extern "C"
