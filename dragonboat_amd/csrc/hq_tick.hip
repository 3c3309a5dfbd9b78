// hq_tick.hip — the Raft timers of a device worker (hq_worker_tick, hq_worker_get_timers /
// _set_timers; include/hipquorum.h "raft timers"): one tick of every group from the (term, state)
// the step keeps resident, and the three due lists compacted in ascending handle order.
//
// The timers are a device array of this module, 16 bytes per handle (hq_tick.h), beside the group
// records. A tick is three kernels on the context's stream behind the last step:
//   k_tick       one lane per handle, 256 handles (a tile) per workgroup: the second and fourth 16
//                bytes of the group record (term | state, flags; a wave's loads are 64-byte
//                strided, two quads of every 64-byte record), the cluster id only of a group whose
//                timer is reset, the timer as one 16-byte load, the contact bit from two bitmaps
//                (the call's staged list, and the contacts hq_hb_received.hip marked on the
//                device since the last tick), the transition of hq_tick.h, the timer back as one 16-byte store. What the tick did
//                goes out as four wave ballots (check-quorum, heartbeat, election, ticked: 32 bytes
//                per 64 handles) and four counts per tile
//   k_tick_scan  one workgroup: the exclusive scan of the tiles' counts, the totals to pinned memory
//   k_tick_emit  one lane per handle again, reading only the ballots and the tile's bases: a listed
//                handle's place is its tile's base + the set bits of the tile's earlier waves + the
//                set bits below its lane; the handle goes straight into the pinned list
// Two passes with per-tile counts instead of one pass with a chained look-back: no workgroup ever
// waits for another (nothing spins), the order is the handle order by construction, and the second
// pass re-reads 32 bytes per wave, not the state. No atomics but the error word's atomicOr in the
// gather / scatter of listed timers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "hq_sidecar.h"
#include "hq_tick.h"

namespace {

constexpr uint32_t kBlock = kTickTile;               // 256: four waves
constexpr uint32_t kWaves = kBlock / 64;
constexpr uint32_t kBits = 4;                        // ballots and counts per wave / tile
static_assert(kBlock == 256 && kWaves == 4, "a tile is four waves");

using Word = ulonglong2;                             // a timer as one 16-byte access
static_assert(sizeof(Word) == sizeof(hq_tick_timer), "16-byte timers");

__device__ __forceinline__ hq_tick_timer unpack(const Word &w) {
    return hq_tick_timer{(uint16_t)w.x, (uint16_t)(w.x >> 16), (uint16_t)(w.x >> 32), (uint8_t)(w.x >> 48),
                         (uint8_t)(w.x >> 56), w.y};
}
__device__ __forceinline__ Word pack(const hq_tick_timer &t) {
    Word w;
    w.x = (uint64_t)t.election_tick | (uint64_t)t.heartbeat_tick << 16 | (uint64_t)t.randomized_timeout << 32 |
          (uint64_t)t.seen_state << 48 | (uint64_t)t.pad << 56;
    w.y = t.seen_term;
    return w;
}

// what the timers read of a group record (hq_dgroup_load, hq_dstep.h)
struct GroupRef {
    uint64_t term;
    uint32_t state;
    bool suspended;
};
__device__ __forceinline__ GroupRef load_group(const hq_dgroup *g) {
    const hq_dgroup_fields f = hq_dgroup_load(g);
    return GroupRef{f.term, f.state, (f.flags & kDSuspended) != 0};
}
__device__ __forceinline__ uint64_t load_cluster_id(const hq_dgroup *g) {
    return *reinterpret_cast<const uint64_t *>(g);
}

struct TickK {
    const hq_dgroup *groups;
    uint64_t n;                    // handles: group records and timers
    Word *timers;
    const uint32_t *contact;       // device bitmap, bit h of word h / 32; NULL: nobody
    const uint32_t *pending;       // the same, of hq_hb_received.hip's pending contacts; NULL: nobody
    hq_tick_params p;
    uint64_t *ballots;             // [n_tiles x kWaves x kBits]
    uint32_t *counts, *bases;      // [n_tiles x kBits]
    uint64_t n_tiles;
    uint32_t *lists[kTickLists];   // pinned host [list_cap] each
    uint64_t list_cap;
    uint64_t *totals;              // pinned host [kBits]
};

__global__ void __launch_bounds__(kBlock) k_tick(TickK k) {
    __shared__ uint32_t s_count[kWaves][kBits];
    const uint64_t h = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t bits = 0;
    if (h < k.n) {
        const hq_dgroup *g = k.groups + h;
        const GroupRef r = load_group(g);
        hq_tick_timer t = unpack(k.timers[h]);
        const bool contact = (k.contact && ((k.contact[h >> 5] >> (h & 31u)) & 1u)) ||
                             (k.pending && ((k.pending[h >> 5] >> (h & 31u)) & 1u));
        const uint64_t cid = !r.suspended && tick_stale(t, r.term, r.state) ? load_cluster_id(g) : 0;
        bits = tick_step(t, k.p, cid, r.term, r.state, r.suspended, contact);
        k.timers[h] = pack(t);
    }
    uint64_t b[kBits];
    for (uint32_t c = 0; c < kBits; ++c) b[c] = __ballot((bits >> c) & 1u);
    if (lane < kBits) {
        const uint64_t mine = lane == 0 ? b[0] : lane == 1 ? b[1] : lane == 2 ? b[2] : b[3];
        k.ballots[((uint64_t)blockIdx.x * kWaves + wave) * kBits + lane] = mine;
        s_count[wave][lane] = (uint32_t)__popcll(mine);
    }
    __syncthreads();
    if (threadIdx.x < kBits) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < kWaves; ++w) sum += s_count[w][threadIdx.x];
        k.counts[(uint64_t)blockIdx.x * kBits + threadIdx.x] = sum;
    }
}

// one workgroup: bases[t] = the counts of the tiles before t, per component; the totals
__global__ void __launch_bounds__(kBlock) k_tick_scan(TickK k) {
    __shared__ uint32_t s_wave[kWaves][kBits];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint4 *counts = reinterpret_cast<const uint4 *>(k.counts);
    uint4 *bases = reinterpret_cast<uint4 *>(k.bases);
    uint32_t carry[kBits] = {0, 0, 0, 0};
    for (uint64_t t0 = 0; t0 < k.n_tiles; t0 += kBlock) {
        const uint64_t t = t0 + threadIdx.x;
        const uint4 v4 = t < k.n_tiles ? counts[t] : make_uint4(0, 0, 0, 0);
        const uint32_t v[kBits] = {v4.x, v4.y, v4.z, v4.w};
        uint32_t incl[kBits];
        for (uint32_t c = 0; c < kBits; ++c) {
            uint32_t x = v[c];
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint32_t y = __shfl_up(x, d, 64);
                if (lane >= d) x += y;
            }
            incl[c] = x;
            if (lane == 63) s_wave[wave][c] = x;
        }
        __syncthreads();
        uint32_t out[kBits];
        for (uint32_t c = 0; c < kBits; ++c) {
            uint32_t before = 0, all = 0;
            for (uint32_t w = 0; w < kWaves; ++w) {
                if (w < wave) before += s_wave[w][c];
                all += s_wave[w][c];
            }
            out[c] = carry[c] + before + incl[c] - v[c];
            carry[c] += all;
        }
        if (t < k.n_tiles) bases[t] = make_uint4(out[0], out[1], out[2], out[3]);
        __syncthreads();                             // (s_wave is written again)
    }
    if (threadIdx.x < kBits) k.totals[threadIdx.x] = carry[threadIdx.x];
}

__global__ void __launch_bounds__(kBlock) k_tick_emit(TickK k) {
    const uint64_t h = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (h >= k.n) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t *tile = k.ballots + (uint64_t)blockIdx.x * kWaves * kBits;
    const uint64_t below = (uint64_t(1) << lane) - 1;
    for (uint32_t c = 0; c < kTickLists; ++c) {
        const uint64_t b = tile[wave * kBits + c];
        if (!((b >> lane) & 1u)) continue;
        uint64_t at = k.bases[(uint64_t)blockIdx.x * kBits + c];
        for (uint32_t w = 0; w < wave; ++w) at += (uint32_t)__popcll(tile[w * kBits + c]);
        at += (uint32_t)__popcll(b & below);
        if (at < k.list_cap) k.lists[c][at] = (uint32_t)h;
    }
}

struct ListedK {
    const hq_dgroup *groups;
    uint64_t n_state_groups;
    Word *timers;
    hq_tick_params p;
    const uint32_t *handles;       // device [n]; NULL: handle i
    uint64_t n;
    hq_timer *pub;                 // device [n]
    uint32_t *error;               // device
    uint32_t *pending;             // hq_hb_received.hip's pending contacts (n_state_groups bits); NULL: none
};

__global__ void __launch_bounds__(kBlock) k_tick_invalidate(ListedK k) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= k.n) return;
    const uint64_t h = k.handles[i];
    if (h < k.n_state_groups) k.timers[h] = pack(tick_unseen());   // (a handle twice: the same value)
}

__global__ void __launch_bounds__(kBlock) k_tick_get(ListedK k) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= k.n) return;
    const uint64_t h = k.handles ? (uint64_t)k.handles[i] : i;
    if (h >= k.n_state_groups) {
        atomicOr(k.error, kTickErrHandle);
        return;
    }
    const hq_dgroup *g = k.groups + h;
    const GroupRef r = load_group(g);
    hq_timer pub = tick_public(unpack(k.timers[h]), k.p, load_cluster_id(g), r.term, r.state);
    // (a pending contact is the next tick's leaderIsAvailable)
    if (k.pending && ((k.pending[h >> 5] >> (h & 31u)) & 1u) && r.state != HQ_STATE_LEADER) pub.election_tick = 0;
    k.pub[i] = pub;
}

__global__ void __launch_bounds__(kBlock) k_tick_set(ListedK k) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= k.n) return;
    const uint64_t h = k.handles ? (uint64_t)k.handles[i] : i;
    if (h >= k.n_state_groups) {
        atomicOr(k.error, kTickErrHandle);
        return;
    }
    const hq_dgroup *g = k.groups + h;
    const GroupRef r = load_group(g);
    k.timers[h] = pack(tick_from_public(k.pub[i], k.p, load_cluster_id(g), r.term, r.state));
    if (k.pending) atomicAnd(k.pending + (h >> 5), ~(1u << (h & 31u)));
}

}  // namespace

struct hq_tick_dev : hq::Sidecar {     // (totals: the four totals, then the listed calls' error word)
    hq::DevBuf<Word> timers;           // device; the first n_timers are in use
    size_t n_timers = 0;
    hq::DevBuf<uint32_t> contact;      // device bitmap
    hq::DevBuf<uint64_t> ballots;
    hq::DevBuf<uint32_t> counts, bases;
    hq::DevBuf<uint32_t> handles;      // device: a call's listed handles
    hq::DevBuf<hq_timer> pub;          // device: a call's public timers
    hq::PinBuf<uint32_t> contact_host; // pinned bitmap, zero between calls
    hq::PinBuf<uint32_t> lists[kTickLists];   // pinned
};

int hq_tick_dev_open(hq_ctx *ctx, hq_tick_dev **out) { return hq::sidecar_open(ctx, out, "hq_tick"); }

void hq_tick_dev_close(hq_tick_dev *t) { hq::sidecar_close(t); }

int hq_tick_dev_contact(hq_tick_dev *t, uint64_t n_groups, uint32_t **bitmap) {
    hq_ctx *ctx = t->ctx;
    const size_t words = hq::words32(n_groups);
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc && words > t->contact_host.cap()) {
        rc = t->contact_host.grow(ctx, words, "hq_tick contact bitmap");
        if (!rc) std::memset(t->contact_host, 0, t->contact_host.cap() * sizeof(uint32_t));
    }
    if (rc) return rc;
    *bitmap = t->contact_host;
    return HQ_OK;
}


int hq_tick_dev_invalidate(hq_tick_dev *t, uint64_t n_groups, bool all, uint64_t n, const uint32_t *handles) {
    hq_ctx *ctx = t->ctx;
    hipStream_t s = ctx->stream;
    if (n > 0xFFFFFFFFull || (n && !handles)) return HQ_E_INVAL;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (rc) return rc;
    // a larger array is all unseen, with the old timers copied in
    rc = t->timers.grow_keep(ctx, n_groups, t->n_timers, 0xFF, "hq_tick timers");
    if (rc) return rc;
    // (the records between n_timers and the capacity are unseen since the array was made)
    t->n_timers = std::max<size_t>(t->n_timers, n_groups);
    if (all) {
        if (t->n_timers)
            rc = hq::check_hip(ctx, hipMemsetAsync(t->timers, 0xFF, t->n_timers * sizeof(Word), s), "hq_tick timers");
        return rc ? hq::finish(ctx, rc, "hq_tick timers") : HQ_OK;
    }
    if (n == 0) return HQ_OK;
    rc = t->handles.grow(ctx, n, "hq_tick handles");
    if (rc) return rc;
    rc = hq::check_hip(ctx, hipMemcpyAsync(t->handles, handles, n * 4, hipMemcpyHostToDevice, s), "hq_tick handles");
    if (!rc) {
        ListedK k{};
        k.n_state_groups = t->n_timers;
        k.timers = t->timers;
        k.handles = t->handles;
        k.n = n;
        hipLaunchKernelGGL(k_tick_invalidate, dim3((uint32_t)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, k);
        rc = hq::check_hip(ctx, hipGetLastError(), "k_tick_invalidate");
    }
    return rc ? hq::finish(ctx, rc, "hq_tick timers") : HQ_OK;
}

int hq_tick_dev_run(hq_tick_dev *t, const hq_dstate_view *st, const hq_tick_params *p, bool with_contact,
                    uint32_t *pending, hq_tick_output *out) {
    hq_ctx *ctx = t->ctx;
    hipStream_t s = ctx->stream;
    const uint64_t n = st->n_groups;
    std::memset(out, 0, sizeof *out);
    if (n > t->n_timers || n > 0xFFFFFFFFull) return hq::fail(ctx, HQ_E_STATE, "hq_tick: fewer timers than groups (internal)");
    const size_t cwords = hq::words32(n);
    if (with_contact && cwords > t->contact_host.cap())
        return hq::fail(ctx, HQ_E_STATE, "hq_tick: the contact bitmap was not staged (internal)");
    if (n == 0) return HQ_OK;
    const uint64_t n_tiles = (n + kBlock - 1) / kBlock;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc) rc = t->ballots.grow(ctx, n_tiles * kWaves * kBits, "hq_tick ballots");
    if (!rc) rc = t->counts.grow(ctx, n_tiles * kBits, "hq_tick counts");
    if (!rc) rc = t->bases.grow(ctx, n_tiles * kBits, "hq_tick bases");
    if (!rc && with_contact) rc = t->contact.grow(ctx, cwords, "hq_tick contact bitmap");
    // (every handle may be due: a list holds them all)
    for (uint32_t c = 0; c < kTickLists && !rc; ++c)
        rc = t->lists[c].grow(ctx, n, "hq_tick lists");

    TickK k{};
    k.groups = st->groups;
    k.n = n;
    k.timers = t->timers;
    k.contact = with_contact ? t->contact.get() : nullptr;
    k.pending = pending;
    k.p = *p;
    k.ballots = t->ballots;
    k.counts = t->counts;
    k.bases = t->bases;
    k.n_tiles = n_tiles;
    k.list_cap = t->lists[0].cap();
    for (uint32_t c = 0; c < kTickLists; ++c) {
        k.lists[c] = t->lists[c];
        k.list_cap = std::min<uint64_t>(k.list_cap, t->lists[c].cap());
    }
    k.totals = t->totals;

    bool queued = false;
    if (!rc) {
        queued = true;
        rc = hq::check_hip(ctx, hipEventRecord(t->ev0, s), "event");
        if (!rc && with_contact)
            rc = hq::check_hip(ctx, hipMemcpyAsync(t->contact, t->contact_host, cwords * 4, hipMemcpyHostToDevice, s),
                               "hq_tick contact bitmap");
        if (!rc) {
            hipLaunchKernelGGL(k_tick, dim3((uint32_t)n_tiles), dim3(kBlock), 0, s, k);
            rc = hq::check_hip(ctx, hipGetLastError(), "k_tick");
        }
        if (!rc) {
            hipLaunchKernelGGL(k_tick_scan, dim3(1), dim3(kBlock), 0, s, k);
            rc = hq::check_hip(ctx, hipGetLastError(), "k_tick_scan");
        }
        if (!rc) {
            hipLaunchKernelGGL(k_tick_emit, dim3((uint32_t)n_tiles), dim3(kBlock), 0, s, k);
            rc = hq::check_hip(ctx, hipGetLastError(), "k_tick_emit");
        }
        // (the pending contacts are consumed)
        if (!rc && pending) rc = hq::check_hip(ctx, hipMemsetAsync(pending, 0, cwords * 4, s), "hq_tick contacts");
        if (!rc) rc = hq::check_hip(ctx, hipEventRecord(t->ev1, s), "event");
    }
    if (queued) rc = hq::finish(ctx, rc, "hq_worker_tick");
    if (with_contact) std::memset(t->contact_host, 0, cwords * 4);   // (consumed, or the call failed)
    if (rc) return rc;
    out->check_quorum = t->lists[0];
    out->n_check_quorum = t->totals[0];
    out->heartbeat = t->lists[1];
    out->n_heartbeat = t->totals[1];
    out->election = t->lists[2];
    out->n_election = t->totals[2];
    out->n_ticked = t->totals[3];
    out->gpu_ns = hq::elapsed_ns(t->ev0, t->ev1);
    return HQ_OK;
}

namespace {

constexpr int kGet = 0, kSet = 1;

int listed(hq_tick_dev *t, int direction, const hq_dstate_view *st, const hq_tick_params *p, uint64_t n,
           const uint32_t *handles, hq_timer *host, uint32_t *pending, uint32_t *error) {
    hq_ctx *ctx = t->ctx;
    hipStream_t s = ctx->stream;
    const char *const what = direction == kGet ? "hq_worker_get_timers" : "hq_worker_set_timers";
    *error = 0;
    if (n == 0 || n > 0xFFFFFFFFull || !host) return HQ_E_INVAL;
    if (st->n_groups > t->n_timers) return hq::fail(ctx, HQ_E_STATE, "hq_tick: fewer timers than groups (internal)");
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc && handles) rc = t->handles.grow(ctx, n, "hq_tick handles");
    if (!rc) rc = t->pub.grow(ctx, n, "hq_tick timers");
    if (rc) return rc;

    ListedK k{};
    k.groups = st->groups;
    k.n_state_groups = st->n_groups;
    k.timers = t->timers;
    k.p = *p;
    k.handles = handles ? t->handles.get() : nullptr;
    k.n = n;
    k.pub = t->pub;
    k.error = t->error();
    k.pending = pending;

    rc = hq::check_hip(ctx, hipMemsetAsync(t->error(), 0, 16, s), "memset");
    if (!rc && handles)
        rc = hq::check_hip(ctx, hipMemcpyAsync(t->handles, handles, n * 4, hipMemcpyHostToDevice, s), what);
    if (!rc && direction == kSet)
        rc = hq::check_hip(ctx, hipMemcpyAsync(t->pub, host, n * sizeof(hq_timer), hipMemcpyHostToDevice, s), what);
    if (!rc) {
        const dim3 grid((uint32_t)((n + kBlock - 1) / kBlock));
        if (direction == kGet) hipLaunchKernelGGL(k_tick_get, grid, dim3(kBlock), 0, s, k);
        else hipLaunchKernelGGL(k_tick_set, grid, dim3(kBlock), 0, s, k);
        rc = hq::check_hip(ctx, hipGetLastError(), direction == kGet ? "k_tick_get" : "k_tick_set");
    }
    // (the error word through the totals' pinned block: its fifth word)
    if (!rc)
        rc = hq::check_hip(ctx, hipMemcpyAsync(t->totals + kBits, t->error(), 4, hipMemcpyDeviceToHost, s), what);
    rc = hq::finish(ctx, rc, what);
    if (rc) return rc;
    if ((uint32_t)t->totals[kBits]) {
        *error = (uint32_t)t->totals[kBits];
        return HQ_E_INVAL;
    }
    if (direction == kGet) {
        rc = hq::check_hip(ctx, hipMemcpyAsync(host, t->pub, n * sizeof(hq_timer), hipMemcpyDeviceToHost, s), what);
        rc = hq::finish(ctx, rc, what);
    }
    return rc;
}

}  // namespace

int hq_tick_dev_get(hq_tick_dev *t, const hq_dstate_view *st, const hq_tick_params *p, uint64_t n,
                    const uint32_t *handles, hq_timer *out, uint32_t *pending, uint32_t *error) {
    return listed(t, kGet, st, p, n, handles, out, pending, error);
}

int hq_tick_dev_set(hq_tick_dev *t, const hq_dstate_view *st, const hq_tick_params *p, uint64_t n,
                    const uint32_t *handles, const hq_timer *timers, uint32_t *pending, uint32_t *error) {
    return listed(t, kSet, st, p, n, handles, const_cast<hq_timer *>(timers), pending, error);
}
