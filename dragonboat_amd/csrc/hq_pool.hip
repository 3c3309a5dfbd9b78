// hq_pool.hip — the member pool of a device worker compacted where it lives (hq_worker_compact,
// include/hipquorum.h "group lifecycle").
//
// One copy kernel on the context's stream behind the last step, 16 lanes per handle (4 handles per
// wave, 16 per workgroup) as in hq_groups.hip. The host has computed every handle's new member
// base from its mirror's structure (an exclusive sum of the live groups' n_members in handle
// order); k_pool_compact reads a group's `mem` and `n_members` from its resident record, moves its
// n_members x 24 bytes as 3 x n_members words of 8 bytes (a member range is only 8-byte aligned)
// from the current pool into a second one — lane l of the team moving words l, l + 16 and l + 32 —
// and writes the new base into the record. The ranges of neighbouring handles are neighbours in
// the new pool, and in the old one wherever the groups were added in order, so a wave's loads and
// stores are contiguous runs. Not in place: old and new ranges overlap. A handle without members
// (a vacant one) copies nothing. Before anything is indexed the team checks the record's member
// count and old range against the old pool's size and the new range against the new pool's; a
// violation sets the error word (the only atomic) and nothing moves for that group. All of a
// lane's loads are issued before its first store. No spinning, no LDS, no loops.
#include <hip/hip_runtime.h>

#include "hq_pool.h"
#include "hq_sidecar.h"

namespace {

constexpr uint32_t kTeam = 16;                        // lanes per handle
constexpr uint32_t kBlock = 256;
constexpr uint32_t kGroupsPerBlock = kBlock / kTeam;  // 16
constexpr uint32_t kMemberUnits = sizeof(hq_dmember) / 8;   // a member record as 8-byte words
static_assert(sizeof(hq_dmember) % 8 == 0 && kDMembers * kMemberUnits == 3 * kTeam,
              "three words per lane of a 16-lane team");
static_assert(sizeof(hq_dgroup) == 64 && offsetof(hq_dgroup, mem) == 48 &&
                  offsetof(hq_dgroup, n_members) == 52,
              "mem and n_members in the record's last 16 bytes");

struct PoolK {
    hq_dgroup *groups;             // the resident records: `mem` is rewritten
    const hq_dmember *src;         // the current pool
    hq_dmember *dst;               // the second pool
    const uint32_t *new_mem;       // device [n_groups]
    uint64_t n_groups, n_old, n_new;
    uint32_t *error;               // device
};

__global__ void __launch_bounds__(kBlock) k_pool_compact(PoolK k) {
    const uint64_t h = (uint64_t)blockIdx.x * kGroupsPerBlock + threadIdx.x / kTeam;
    const uint32_t l = threadIdx.x % kTeam;
    if (h >= k.n_groups) return;
    // the record's last 16 bytes: mem, n_members, ...
    const ulonglong2 tail = reinterpret_cast<const ulonglong2 *>(k.groups + h)[3];
    const uint32_t mem = (uint32_t)tail.x, n = (uint32_t)(tail.x >> 32) & 0xFFu;
    const uint32_t to = k.new_mem[h];
    if (n > kDMembers || (uint64_t)mem + n > k.n_old) {
        if (l == 0) atomicOr(k.error, kPoolErrState);
        return;
    }
    if ((uint64_t)to + n > k.n_new) {
        if (l == 0) atomicOr(k.error, kPoolErrRange);
        return;
    }
    const uint64_t *s = reinterpret_cast<const uint64_t *>(k.src + mem);
    uint64_t *d = reinterpret_cast<uint64_t *>(k.dst + to);
    const uint32_t units = n * kMemberUnits;          // <= 48
    const bool m0 = l < units, m1 = l + kTeam < units, m2 = l + 2 * kTeam < units;
    const uint64_t w0 = m0 ? s[l] : 0;
    const uint64_t w1 = m1 ? s[l + kTeam] : 0;
    const uint64_t w2 = m2 ? s[l + 2 * kTeam] : 0;
    if (m0) d[l] = w0;
    if (m1) d[l + kTeam] = w1;
    if (m2) d[l + 2 * kTeam] = w2;
    if (l == 0) k.groups[h].mem = to;
}

}  // namespace

struct hq_pool_dev : hq::Sidecar {     // (totals: the error word as the host reads it)
    hq::PinBuf<uint32_t> new_mem_host; // pinned staging of the column
    hq::DevBuf<uint32_t> new_mem;      // device, of new_mem_host's capacity
};

int hq_pool_dev_open(hq_ctx *ctx, hq_pool_dev **out) { return hq::sidecar_open(ctx, out, "hq_pool error word"); }

void hq_pool_dev_close(hq_pool_dev *c) { hq::sidecar_close(c); }

int hq_pool_dev_stage(hq_pool_dev *c, uint64_t n_groups, uint32_t **new_mem) {
    hq_ctx *ctx = c->ctx;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc) rc = c->new_mem_host.grow(ctx, n_groups, "hq_pool column", hq::Headroom::kHalf64);
    if (rc) return rc;
    *new_mem = c->new_mem_host;
    return HQ_OK;
}

int hq_pool_dev_compact(hq_pool_dev *c, const hq_dstate_mut *st, uint64_t n_old, hq_dmember *dst,
                        uint64_t n_new, uint64_t *gpu_ns, uint32_t *error) {
    hq_ctx *ctx = c->ctx;
    hipStream_t s = ctx->stream;
    const uint64_t G = st->n_groups;
    *error = 0;
    *gpu_ns = 0;
    if (G == 0 || G > c->new_mem_host.cap() || !dst || !st->groups || !st->members) return HQ_E_INVAL;
    if ((G + kGroupsPerBlock - 1) / kGroupsPerBlock > 0x7FFFFFFFull) return HQ_E_INVAL;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc && G > c->new_mem.cap()) rc = c->new_mem.reserve(ctx, c->new_mem_host.cap(), "hq_pool column");
    if (rc) return rc;

    PoolK k{};
    k.groups = st->groups;
    k.src = st->members;
    k.dst = dst;
    k.new_mem = c->new_mem;
    k.n_groups = G;
    k.n_old = n_old;
    k.n_new = n_new;
    k.error = c->error();

    // (from here on every return is finish's: the staging is rewritten by the next call)
    rc = hq::check_hip(ctx, hipEventRecord(c->ev0, s), "event");
    if (!rc) rc = hq::check_hip(ctx, hipMemsetAsync(c->error(), 0, 16, s), "memset");
    if (!rc)
        rc = hq::check_hip(ctx, hipMemcpyAsync(c->new_mem, c->new_mem_host, G * 4, hipMemcpyHostToDevice, s),
                           "hq_pool column");
    if (!rc) {
        const uint32_t grid = (uint32_t)((G + kGroupsPerBlock - 1) / kGroupsPerBlock);
        hipLaunchKernelGGL(k_pool_compact, dim3(grid), dim3(kBlock), 0, s, k);
        rc = hq::check_hip(ctx, hipGetLastError(), "k_pool_compact");
    }
    if (!rc)
        rc = hq::check_hip(ctx, hipMemcpyAsync(c->totals, c->error(), 4, hipMemcpyDeviceToHost, s),
                           "hq_pool error word");
    if (!rc) rc = hq::check_hip(ctx, hipEventRecord(c->ev1, s), "event");
    rc = hq::finish(ctx, rc, "hq_pool");
    if (rc) return rc;
    if ((uint32_t)c->totals[0]) {
        *error = (uint32_t)c->totals[0];
        return HQ_E_INVAL;
    }
    *gpu_ns = hq::elapsed_ns(c->ev0, c->ev1);
    return HQ_OK;
}
