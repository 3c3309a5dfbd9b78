// hq_groups.h — the state of listed groups fetched from and written to a worker's quorum state
// (hq_worker_get_groups / hq_worker_set_groups, include/hipquorum.h "listed groups"), shared
// between hq_worker_lists.cpp (plain C++: both calls' host side), hq_groups.hip (k_groups_gather /
// k_groups_scatter over a device worker's resident records) and the stand-alone check of
// tests/test_groups_ref.py. The packed record's layout, pack / unpack and the mapping of a slot
// bitmap to list positions below are the one source all three use.
// Internal to libhipquorum.so.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/hipquorum.h"
#include "hq_dstep.h"

#if defined(__HIPCC__)
#define HQ_GRP_HD __host__ __device__
#else
#define HQ_GRP_HD
#endif

// ---- the packed record: what crosses the link per listed group, 48 words of 16 bytes ----
//   words  0 ..  3   the hq_dgroup
//   words  4 .. 23   its kDReads hq_dread
//   words 24 .. 47   its member records, kDMembers x 24 bytes in pool order, zero beyond n_members
struct hq_grp_record {
    hq_dgroup g;
    hq_dread r[kDReads];
    hq_dmember m[kDMembers];
};
constexpr uint32_t kGrpWordBytes = 16;
constexpr uint32_t kGrpGroupWords = sizeof(hq_dgroup) / kGrpWordBytes;                 // 4
constexpr uint32_t kGrpReadWords = kDReads * sizeof(hq_dread) / kGrpWordBytes;         // 20
constexpr uint32_t kGrpMemberWords = kDMembers * sizeof(hq_dmember) / kGrpWordBytes;   // 24
constexpr uint32_t kGrpRecordWords = kGrpGroupWords + kGrpReadWords + kGrpMemberWords; // 48
constexpr uint32_t kGrpRecordBytes = kGrpRecordWords * kGrpWordBytes;                  // 768
constexpr uint32_t kGrpMemberUnits = sizeof(hq_dmember) / 8;   // a member record as 8-byte units
static_assert(sizeof(hq_grp_record) == kGrpRecordBytes && kGrpRecordBytes == 768, "768-byte records");
static_assert(offsetof(hq_grp_record, r) == kGrpGroupWords * kGrpWordBytes, "reads at word 4");
static_assert(offsetof(hq_grp_record, m) == (kGrpGroupWords + kGrpReadWords) * kGrpWordBytes,
              "members at word 24");
static_assert(sizeof(hq_dgroup) % kGrpWordBytes == 0 && (kDReads * sizeof(hq_dread)) % kGrpWordBytes == 0 &&
                  (kDMembers * sizeof(hq_dmember)) % kGrpWordBytes == 0 && sizeof(hq_dmember) % 8 == 0,
              "whole words");
static_assert(kGrpRecordWords == 3 * 16, "three words per lane of a 16-lane team");

// the kernels' error word
constexpr uint32_t kGrpErrHandle = 1;  // a handle at or beyond the state's group count
constexpr uint32_t kGrpErrState = 2;   // a record whose counts or member range do not fit (internal)

// what the kernels check before they index with a record's fields
HQ_GRP_HD inline bool grp_fits(uint32_t mem, uint32_t n_members, uint32_t n_reads, uint64_t n_state_members) {
    return n_members <= kDMembers && n_reads <= kDReads && (uint64_t)mem + n_members <= n_state_members;
}

// (g, reads[0 .. g.n_reads), members[0 .. g.n_members)) -> record; everything else of it zero
HQ_GRP_HD inline void grp_pack(hq_grp_record &rec, const hq_dgroup &g, const hq_dread *reads,
                               const hq_dmember *members) {
    rec.g = g;
    for (uint32_t k = 0; k < kDReads; ++k) rec.r[k] = k < g.n_reads ? reads[k] : hq_dread{};
    for (uint32_t i = 0; i < kDMembers; ++i) rec.m[i] = i < g.n_members ? members[i] : hq_dmember{};
}
// record -> (g, reads[0 .. g.n_reads), members[0 .. g.n_members)); false (nothing but g written)
// for counts beyond the record's arrays
HQ_GRP_HD inline bool grp_unpack(const hq_grp_record &rec, hq_dgroup &g, hq_dread *reads,
                                 hq_dmember *members) {
    g = rec.g;
    if (g.n_members > kDMembers || g.n_reads > kDReads) return false;
    for (uint32_t k = 0; k < g.n_reads; ++k) reads[k] = rec.r[k];
    for (uint32_t i = 0; i < g.n_members; ++i) members[i] = rec.m[i];
    return true;
}

// A slot bitmap (granted, rejected, a read's confirmed: bit s = voting slot s = pool position s)
// in the caller's terms: bit i = member i of the caller's list. `members` is the group's records
// in pool order (their `order` byte is the list position); bits at or above n_voting are no
// member's and are dropped, as are list positions a 16-bit mask cannot hold.
HQ_GRP_HD inline uint16_t grp_slots_to_list(uint32_t bits, uint32_t n_voting, const hq_dmember *members) {
    uint32_t out = 0;
    for (uint32_t s = 0; s < HQ_MAX_VOTERS && s < n_voting; ++s)
        if (((bits >> s) & 1u) && members[s].order < 16) out |= 1u << members[s].order;
    return (uint16_t)out;
}

// ---- the device path (hq_groups.hip) ----
struct hq_groups_dev;                  // the buffers of one device worker's calls; they keep their
                                       // size from call to call
int hq_groups_dev_open(hq_ctx *ctx, hq_groups_dev **out);
void hq_groups_dev_close(hq_groups_dev *c);
// pinned staging for n records and n handles (valid until the next stage call that grows them)
int hq_groups_dev_stage(hq_groups_dev *c, uint64_t n, hq_grp_record **records, uint32_t **handles);
// One kernel over the staged handles on the context's stream, behind whatever was queued there,
// and a wait for it. gather: record i <- the resident state of handle handles[i] (identity: of
// handle i; repeats allowed); scatter: the resident state of handle handles[i] <- record i
// (distinct handles). n_member_records: the member pool's size. HQ_E_INVAL with *error set
// (kGrpErr*) when a kernel refused a group (nothing moved for that group).
int hq_groups_dev_gather(hq_groups_dev *c, const hq_dstate_view *st, uint64_t n_member_records, uint64_t n,
                         bool identity, uint64_t *gpu_ns, uint32_t *error);
int hq_groups_dev_scatter(hq_groups_dev *c, const hq_dstate_mut *st, uint64_t n_member_records, uint64_t n,
                          uint64_t *gpu_ns, uint32_t *error);
