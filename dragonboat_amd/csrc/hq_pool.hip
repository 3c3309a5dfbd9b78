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

#include <new>

#include "hq_internal.h"
#include "hq_pool.h"

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

template <class T>
int grow_pinned(hq_ctx *ctx, T **p, size_t *cap, size_t need, const char *what) {
    if (need <= *cap) return HQ_OK;
    const size_t want = (need + need / 2 + 63) / 64 * 64;
    T *n = nullptr;
    int rc = hq::check_hip(ctx, hipHostMalloc(reinterpret_cast<void **>(&n), want * sizeof(T),
                                              hipHostMallocDefault), what);
    if (rc) return rc;
    if (*p) (void)hipHostFree(*p);
    *p = n;
    *cap = want;
    return HQ_OK;
}

}  // namespace

struct hq_pool_dev {
    hq_ctx *ctx = nullptr;
    uint32_t *new_mem_host = nullptr;  // pinned staging of the column
    uint32_t *new_mem = nullptr;       // device
    uint32_t *error = nullptr;         // device
    uint32_t *error_host = nullptr;    // pinned
    size_t host_cap = 0, dev_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

int hq_pool_dev_open(hq_ctx *ctx, hq_pool_dev **out) {
    *out = new (std::nothrow) hq_pool_dev();
    if (!*out) return HQ_E_NOMEM;
    hq_pool_dev *c = *out;
    c->ctx = ctx;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    for (hipEvent_t *e : {&c->ev0, &c->ev1})
        if (!rc) rc = hq::check_hip(ctx, hipEventCreate(e), "event");
    if (!rc) rc = hq::check_hip(ctx, hipMalloc(reinterpret_cast<void **>(&c->error), 16),
                                "hq_pool error word");
    if (!rc)
        rc = hq::check_hip(ctx, hipHostMalloc(reinterpret_cast<void **>(&c->error_host), 64,
                                              hipHostMallocDefault), "hq_pool error word");
    if (rc) {
        hq_pool_dev_close(c);
        *out = nullptr;
    }
    return rc;
}

void hq_pool_dev_close(hq_pool_dev *c) {
    if (!c) return;
    (void)hipSetDevice(c->ctx->device);
    (void)hipStreamSynchronize(c->ctx->stream);
    for (void *p : {(void *)c->new_mem, (void *)c->error})
        if (p) (void)hipFree(p);
    for (void *p : {(void *)c->new_mem_host, (void *)c->error_host})
        if (p) (void)hipHostFree(p);
    for (hipEvent_t e : {c->ev0, c->ev1})
        if (e) (void)hipEventDestroy(e);
    delete c;
}

int hq_pool_dev_stage(hq_pool_dev *c, uint64_t n_groups, uint32_t **new_mem) {
    hq_ctx *ctx = c->ctx;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc) rc = grow_pinned(ctx, &c->new_mem_host, &c->host_cap, n_groups, "hq_pool column");
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
    if (G == 0 || G > c->host_cap || !dst || !st->groups || !st->members) return HQ_E_INVAL;
    if ((G + kGroupsPerBlock - 1) / kGroupsPerBlock > 0x7FFFFFFFull) return HQ_E_INVAL;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc && G > c->dev_cap) {
        uint32_t *p = nullptr;
        rc = hq::check_hip(ctx, hipMalloc(reinterpret_cast<void **>(&p), c->host_cap * 4), "hq_pool column");
        if (!rc) {
            if (c->new_mem) (void)hipFree(c->new_mem);
            c->new_mem = p;
            c->dev_cap = c->host_cap;
        }
    }
    if (rc) return rc;

    PoolK k{};
    k.groups = st->groups;
    k.src = st->members;
    k.dst = dst;
    k.new_mem = c->new_mem;
    k.n_groups = G;
    k.n_old = n_old;
    k.n_new = n_new;
    k.error = c->error;

    rc = hq::check_hip(ctx, hipEventRecord(c->ev0, s), "event");
    if (!rc) rc = hq::check_hip(ctx, hipMemsetAsync(c->error, 0, 16, s), "memset");
    if (!rc)
        rc = hq::check_hip(ctx, hipMemcpyAsync(c->new_mem, c->new_mem_host, G * 4, hipMemcpyHostToDevice, s),
                           "hq_pool column");
    if (rc) return rc;
    const uint32_t grid = (uint32_t)((G + kGroupsPerBlock - 1) / kGroupsPerBlock);
    hipLaunchKernelGGL(k_pool_compact, dim3(grid), dim3(kBlock), 0, s, k);
    rc = hq::check_hip(ctx, hipGetLastError(), "k_pool_compact");
    if (!rc)
        rc = hq::check_hip(ctx, hipMemcpyAsync(c->error_host, c->error, 4, hipMemcpyDeviceToHost, s),
                           "hq_pool error word");
    if (!rc) rc = hq::check_hip(ctx, hipEventRecord(c->ev1, s), "event");
    if (!rc) rc = hq::check_hip(ctx, hipStreamSynchronize(s), "hq_pool");
    if (rc) return rc;
    if (*c->error_host) {
        *error = *c->error_host;
        return HQ_E_INVAL;
    }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) {
        (void)hipGetLastError();
        ms = 0.f;
    }
    *gpu_ns = (uint64_t)((double)ms * 1e6);
    return HQ_OK;
}
