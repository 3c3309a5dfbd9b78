// hq_config.h — membership changes on the worker's quorum state (hq_worker_config_changes,
// include/hipquorum.h "membership changes"), shared between hq_worker_lists.cpp (plain C++: validation,
// the descriptors, the host worker's own edit and the mirror's), hq_config.hip (k_cfg_apply over a
// device worker's resident records) and the stand-alone check of tests/test_config_ref.py. The
// bitmap remaps and the position arithmetic below are the one source all three use.
// Internal to libhipquorum.so.
#pragma once

#include <cstdint>

#include "../../include/hipquorum.h"
#include "hq_dstep.h"

#if defined(__HIPCC__)
#define HQ_CFG_HD __host__ __device__
#else
#define HQ_CFG_HD
#endif

// What a change does to a group's member records (pool order: the node itself, the other remotes,
// the witnesses — the voting slots, a member's slot is its position — then the observers).
constexpr uint8_t kCfgNoop = 0;        // an add of a member already in that role
constexpr uint8_t kCfgCommitOnly = 1;  // REMOVE_NODE of a non-member: removeNode's tryCommit alone
constexpr uint8_t kCfgRemove = 2;      // delete the record at src
constexpr uint8_t kCfgInsert = 3;      // a new record at dst
constexpr uint8_t kCfgPromote = 4;     // the observer at src becomes the remote at dst
constexpr uint8_t kCfgFallback = 5;    // the slot model cannot hold the result: suspend the group
constexpr uint8_t kCfgNoSlot = 0xFF;
constexpr uint32_t kCfgNoMove = 0xFFFFFFFFu;

struct hq_cfg_desc {                   // one change, computed by the host from its mirror's structure
    uint64_t node_id;                  // kCfgInsert: the new member
    uint32_t group;                    // handle
    uint32_t new_mem;                  // kCfgInsert: the group's new member base (its range is
                                       // full: it moves to the pool's end), else kCfgNoMove
    uint8_t kind;
    uint8_t src, dst;                  // pool positions
    uint8_t slot;                      // the voting slot removed / inserted, or kCfgNoSlot
    uint8_t role;                      // kCfgInsert: the new member's role
    uint8_t order;                     // list position: the removed member's / the new member's
    uint8_t n_members, n_voting;       // as the mirror holds them (the kernel checks the record's)
};
static_assert(sizeof(hq_cfg_desc) == 24, "24-byte change descriptors");

// k_cfg_apply's error word
constexpr uint32_t kCfgErrHandle = 1;  // a handle at or beyond the state's group count
constexpr uint32_t kCfgErrState = 2;   // a descriptor the resident record does not match (internal)

// ---- slot bitmaps (granted, rejected, a pending read's confirmed: bit s = voting slot s) ----
HQ_CFG_HD inline uint32_t cfg_low(uint32_t s) { return (1u << s) - 1u; }
// slot s leaves: the slots above it move down by one
HQ_CFG_HD inline uint32_t cfg_remove_bit(uint32_t b, uint32_t s) {
    return (b & cfg_low(s)) | ((b >> 1) & ~cfg_low(s));
}
// a new (clear) slot p: the slots at and above it move up by one
HQ_CFG_HD inline uint32_t cfg_insert_bit(uint32_t b, uint32_t p) {
    return (b & cfg_low(p)) | ((b & ~cfg_low(p)) << 1);
}

// ---- positions ----
struct hq_cfg_layout {                 // a group's pool: [0, n_remotes) remotes (the node first),
    uint32_t n_remotes, n_voting;      // [n_remotes, n_voting) witnesses, [n_voting, n_members)
    uint32_t n_members;                // observers
};
// where a new member of `type` (HQ_CC_ADD_*) goes: behind the members of its role
HQ_CFG_HD inline uint32_t cfg_insert_pos(uint32_t type, const hq_cfg_layout &l) {
    return type == HQ_CC_ADD_NODE ? l.n_remotes : type == HQ_CC_ADD_WITNESS ? l.n_voting : l.n_members;
}
// its voting slot (its position), none for an observer
HQ_CFG_HD inline uint32_t cfg_insert_slot(uint32_t type, const hq_cfg_layout &l) {
    return type == HQ_CC_ADD_OBSERVER ? kCfgNoSlot : cfg_insert_pos(type, l);
}
// a promoted observer goes behind the remotes
HQ_CFG_HD inline uint32_t cfg_promote_pos(const hq_cfg_layout &l) { return l.n_remotes; }
// the voting slot a removal at src frees, none for an observer
HQ_CFG_HD inline uint32_t cfg_remove_slot(uint32_t src, const hq_cfg_layout &l) {
    return src < l.n_voting ? src : kCfgNoSlot;
}
// where the record at old position j stands afterwards
HQ_CFG_HD inline uint32_t cfg_pos_after_remove(uint32_t j, uint32_t src) { return j < src ? j : j - 1; }
HQ_CFG_HD inline uint32_t cfg_pos_after_insert(uint32_t j, uint32_t dst) { return j < dst ? j : j + 1; }
HQ_CFG_HD inline uint32_t cfg_pos_after_promote(uint32_t j, uint32_t src, uint32_t dst) {
    return j == src ? dst : (j >= dst && j < src) ? j + 1 : j;
}
// list positions (hq_dmember::order): a removal closes the gap
HQ_CFG_HD inline uint32_t cfg_order_after_remove(uint32_t o, uint32_t removed) {
    return o > removed ? o - 1 : o;
}

// ---- the device path (hq_config.hip) ----
struct hq_cfg_dev;                     // the buffers of one device worker's calls

int hq_cfg_dev_open(hq_ctx *ctx, hq_cfg_dev **out);
void hq_cfg_dev_close(hq_cfg_dev *c);
// desc[0 .. n) (host memory, distinct groups, n > 0) applied to the resident state `st` of
// n_member_records member records. *status (HQ_CC_* per change) and *committed (the new committed
// index of a removal's tryCommit that advanced, else 0) are c's pinned columns, valid until its
// next run. HQ_E_INVAL with *error set when the kernel refused a descriptor (nothing written for
// that change).
int hq_cfg_dev_run(hq_cfg_dev *c, const hq_dstate_mut *st, uint64_t n_member_records, uint64_t n,
                   const hq_cfg_desc *desc, const uint32_t **status, const uint64_t **committed,
                   uint64_t *gpu_ns, uint32_t *error);
