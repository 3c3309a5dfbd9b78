// hq_tick.h — the Raft timers of a step worker (hq_worker_tick and its companions,
// include/hipquorum.h "raft timers"): raft.tick / leaderTick / nonLeaderTick (raft.go:525-636) with
// raft.reset's counter part (raft.go:991-1023) and leaderIsAvailable (raft.go:1859-1861). Shared
// between hq_worker_tick.cpp (plain C++: the C entries, the checks, the host worker's own form) and
// hq_tick.hip (the kernels over a device worker's resident records): the timer record, the draw of
// the randomized timeout and the one-tick transition below are the one source both compile.
// Internal to libhipquorum.so.
#pragma once

#include <cstdint>

#include "../../include/hipquorum.h"
#include "hq_dstep.h"

#if defined(__HIPCC__)
#define HQ_TICK_HD __host__ __device__
#else
#define HQ_TICK_HD
#endif

// ---- the timer: one 16-byte record per group handle, beside the group records (hq_dgroup stays
// as it is). The counters fit 16 bits: election_rtt <= 32767 keeps randomized_timeout and
// election_tick below 65534, heartbeat_rtt <= 65535 keeps heartbeat_tick below it.
// (seen_term, seen_state) is the group's (term, state) the counters belong to; a timer whose pair
// differs from the group's is reset before anything else is done with it. seen_state == kTickUnseen
// matches no state: the form of a timer that must come back reset (a fresh or re-synced handle, a
// suspended group, a new config).
struct hq_tick_timer {
    uint16_t election_tick, heartbeat_tick, randomized_timeout;
    uint8_t seen_state, pad;
    uint64_t seen_term;
};
static_assert(sizeof(hq_tick_timer) == 16 && alignof(hq_tick_timer) == 8, "16-byte timers");
constexpr uint8_t kTickUnseen = 0xFF;      // (a memset of 0xFF makes unseen timers)

struct hq_tick_params {                    // a checked hq_tick_config
    uint32_t election_rtt, heartbeat_rtt, check_quorum;
    uint64_t seed;
};

// what a tick did with a group
constexpr uint32_t kTickCheckQuorum = 1, kTickHeartbeat = 2, kTickElection = 4, kTickTicked = 8;
constexpr uint32_t kTickLists = 3;         // the three due lists, in the bits' order

// hq_tick_timeout: uniform in [E, 2E) from a splitmix64 finalizer over the group's identity and the
// (term, state) the timer is drawn for; all arithmetic modulo 2^64
HQ_TICK_HD inline uint32_t tick_draw(uint64_t seed, uint64_t cluster_id, uint64_t term, uint32_t state,
                                     uint32_t election_rtt) {
    const uint64_t x = seed ^ (cluster_id * 0x9E3779B97F4A7C15ull) ^ (term * 0xBF58476D1CE4E5B9ull) ^
                       (uint64_t)state;
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return election_rtt + (uint32_t)(z % election_rtt);
}

// the timer's counters are another (term, state)'s, or nobody's
HQ_TICK_HD inline bool tick_stale(const hq_tick_timer &t, uint64_t term, uint32_t state) {
    return t.seen_state != state || t.seen_term != term;
}

HQ_TICK_HD inline hq_tick_timer tick_fresh(const hq_tick_params &p, uint64_t cluster_id, uint64_t term,
                                           uint32_t state) {
    return hq_tick_timer{0, 0, (uint16_t)tick_draw(p.seed, cluster_id, term, state, p.election_rtt),
                         (uint8_t)state, 0, term};
}

HQ_TICK_HD inline hq_tick_timer tick_unseen() {
    return hq_tick_timer{0xFFFF, 0xFFFF, 0xFFFF, kTickUnseen, 0xFF, ~uint64_t(0)};
}

// One tick of one group. `suspended`: the record's suspended flag (a vacant handle's tombstone has
// it too): the group is not ticked and its timer comes back reset. `contact`: the caller listed the
// group as having heard from its leader. Returns the kTick* bits.
HQ_TICK_HD inline uint32_t tick_step(hq_tick_timer &t, const hq_tick_params &p, uint64_t cluster_id,
                                     uint64_t term, uint32_t state, bool suspended, bool contact) {
    if (suspended) {
        t = tick_unseen();
        return 0;
    }
    if (tick_stale(t, term, state)) t = tick_fresh(p, cluster_id, term, state);   // 1. reset
    uint32_t election = t.election_tick, bits = kTickTicked;
    if (state == HQ_STATE_LEADER) {                                               // 3. leaderTick
        uint32_t heartbeat = t.heartbeat_tick;
        if (++election >= p.election_rtt) {
            election = 0;
            if (p.check_quorum) bits |= kTickCheckQuorum;
        }
        if (++heartbeat >= p.heartbeat_rtt) {
            heartbeat = 0;
            bits |= kTickHeartbeat;
        }
        t.heartbeat_tick = (uint16_t)heartbeat;
    } else {
        if (contact) election = 0;                                                // 2. contact
        if (++election >= t.randomized_timeout) {                                 // 4. nonLeaderTick
            election = 0;
            bits |= kTickElection;
        }
    }
    t.election_tick = (uint16_t)election;
    return bits;
}

// hq_worker_get_timers' view of a timer: one with a pending reset is returned as reset
HQ_TICK_HD inline hq_timer tick_public(const hq_tick_timer &t, const hq_tick_params &p, uint64_t cluster_id,
                                       uint64_t term, uint32_t state) {
    const hq_tick_timer v = tick_stale(t, term, state) ? tick_fresh(p, cluster_id, term, state) : t;
    return hq_timer{v.election_tick, v.heartbeat_tick, v.randomized_timeout, 0};
}

// hq_worker_set_timers' limits (the group's state is the device's to know: one rule for all states)
HQ_TICK_HD inline bool tick_settable(const hq_timer &s, const hq_tick_params &p) {
    return s.election_tick < 2 * p.election_rtt && s.heartbeat_tick < p.heartbeat_rtt && s.reserved == 0 &&
           (s.randomized_timeout == 0 ||
            (s.randomized_timeout >= p.election_rtt && s.randomized_timeout < 2 * p.election_rtt));
}

// the checked counters of `s` as the timer of a group at (term, state); 0: drawn by the formula
HQ_TICK_HD inline hq_tick_timer tick_from_public(const hq_timer &s, const hq_tick_params &p, uint64_t cluster_id,
                                                 uint64_t term, uint32_t state) {
    hq_tick_timer t = tick_fresh(p, cluster_id, term, state);
    t.election_tick = (uint16_t)s.election_tick;
    t.heartbeat_tick = (uint16_t)s.heartbeat_tick;
    if (s.randomized_timeout) t.randomized_timeout = (uint16_t)s.randomized_timeout;
    return t;
}

// ---- the device path (hq_tick.hip) ----
constexpr uint32_t kTickTile = 256;        // groups per workgroup of the tick: the scan's tile

struct hq_tick_dev;                        // a device worker's timers and its calls' buffers

// hq_tick_dev_*'s *error
constexpr uint32_t kTickErrHandle = 1;     // a listed handle at or beyond the state's group count

int hq_tick_dev_open(hq_ctx *ctx, hq_tick_dev **out);
void hq_tick_dev_close(hq_tick_dev *t);
// The pinned contact bitmap of a tick, n_groups bits (bit h of word h / 32): zero when handed out,
// valid until the next call that asks for a larger one; hq_tick_dev_run clears what it consumed.
int hq_tick_dev_contact(hq_tick_dev *t, uint64_t n_groups, uint32_t **bitmap);
// The timer array grown to n_groups records (new ones unseen) and, queued on the context's stream,
// every timer (`all`) or those of handles[0 .. n) (host memory; repeats allowed) made unseen. On
// success the next run, get or set is queued behind it; a failure has waited for the stream.
int hq_tick_dev_invalidate(hq_tick_dev *t, uint64_t n_groups, bool all, uint64_t n, const uint32_t *handles);
// One tick of every group of `st` (the timers were grown to st->n_groups); with_contact: the
// bitmap handed out by hq_tick_dev_contact. `pending` (or NULL): a device bitmap of at least
// st->n_groups bits whose set bits are contacts too (hq_hb_received.hip's); its first
// ceil(n_groups / 32) words are zeroed behind the kernels. *out's lists are t's pinned buffers, valid until its
// next run. Waits for the kernels, also when something failed.
int hq_tick_dev_run(hq_tick_dev *t, const hq_dstate_view *st, const hq_tick_params *p, bool with_contact,
                    uint32_t *pending, hq_tick_output *out);
// out[i] <- the timer of handles[i] (host memory; NULL: of handle i), as tick_public gives it; the
// timer of handles[i] (distinct) <- timers[i], as tick_from_public makes it. 0 < n < 2^32.
// `pending` as for the run: get returns a non-leader whose bit is set with election_tick 0, set
// clears the bits of its handles. HQ_E_INVAL with *error set when the kernel refused a handle. Both
// wait for their kernel.
int hq_tick_dev_get(hq_tick_dev *t, const hq_dstate_view *st, const hq_tick_params *p, uint64_t n,
                    const uint32_t *handles, hq_timer *out, uint32_t *pending, uint32_t *error);
int hq_tick_dev_set(hq_tick_dev *t, const hq_dstate_view *st, const hq_tick_params *p, uint64_t n,
                    const uint32_t *handles, const hq_timer *timers, uint32_t *pending, uint32_t *error);
