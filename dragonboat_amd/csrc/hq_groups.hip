// hq_groups.hip — the state of listed groups of a device worker, fetched and written where it
// lives (hq_worker_get_groups / hq_worker_set_groups, include/hipquorum.h "listed groups").
//
// Two copy kernels on the context's stream behind the last step, 16 lanes per listed group (4
// groups per wave, 16 per workgroup), over the packed 768-byte record of hq_groups.h: 48 words of
// 16 bytes, lane l of a group's team moving words l, l + 16 and l + 32. k_groups_gather reads a
// group's record, its reads and its member range from the resident arrays and stores the record
// into pinned host memory (a wave's output is 3 KiB contiguous); k_groups_scatter reads records
// from pinned host memory and stores them to their places. Group and read words move as 16-byte
// accesses (64 and 320 bytes per handle keep them aligned); a member range starts at mem x 24
// bytes, which is only 8-byte aligned, so member words move as pairs of 8-byte accesses, and none
// of them touches a record at or beyond mem + n_members: a neighbour's range starts there. All of a
// lane's loads are issued before its first store. Before anything is indexed the team re-checks
// the handle against the group count and the record's counts and member range against the state's
// sizes; a violation sets the error word (the only atomic), and nothing moves for that group. No
// spinning, no LDS, no loops.
#include <hip/hip_runtime.h>

#include "hq_groups.h"
#include "hq_sidecar.h"

namespace {

constexpr uint32_t kTeam = 16;                        // lanes per listed group
constexpr uint32_t kBlock = 256;
constexpr uint32_t kGroupsPerBlock = kBlock / kTeam;  // 16
static_assert(kGrpRecordWords == 3 * kTeam, "three words per lane");

using Word = ulonglong2;                              // 16 bytes
static_assert(sizeof(Word) == kGrpWordBytes && alignof(Word) == kGrpWordBytes, "16-byte words");

struct GrpK {
    hq_dgroup *groups;             // the resident state (the gather only reads it)
    hq_dread *reads;
    hq_dmember *members;
    uint64_t n_state_groups, n_state_members;
    const uint32_t *handles;       // device [n]; NULL: handle i
    uint64_t n;
    hq_grp_record *records;        // pinned host [n]
    uint32_t *error;               // device
};

// what a team needs of a group record's last word (bytes 48 .. 63: mem, n_members, n_voting,
// state, granted; rejected, flags, n_reads, padding) before it indexes anything
struct Tail {
    uint32_t mem, n_members, n_reads;
};
__device__ __forceinline__ Tail tail_of(const Word &w) {
    return Tail{(uint32_t)w.x, (uint32_t)(w.x >> 32) & 0xFFu, (uint32_t)(w.y >> 16) & 0xFFu};
}

// Word w of a member range (8-byte units 2w and 2w + 1 of n_units): zero beyond the range.
__device__ __forceinline__ Word load_member_word(const uint64_t *mu, uint32_t w, uint32_t n_units) {
    const uint32_t u = 2 * w;
    Word r;
    r.x = u < n_units ? mu[u] : 0;
    r.y = u + 1 < n_units ? mu[u + 1] : 0;
    return r;
}
__device__ __forceinline__ void store_member_word(uint64_t *mu, uint32_t w, uint32_t n_units, const Word &v) {
    const uint32_t u = 2 * w;
    if (u < n_units) mu[u] = v.x;
    if (u + 1 < n_units) mu[u + 1] = v.y;
}

__global__ void __launch_bounds__(kBlock) k_groups_gather(GrpK k) {
    const uint64_t i = (uint64_t)blockIdx.x * kGroupsPerBlock + threadIdx.x / kTeam;
    const uint32_t l = threadIdx.x % kTeam;
    if (i >= k.n) return;
    const uint64_t h = k.handles ? (uint64_t)k.handles[i] : i;
    if (h >= k.n_state_groups) {
        if (l == 0) atomicOr(k.error, kGrpErrHandle);
        return;
    }
    const Word *gw = reinterpret_cast<const Word *>(k.groups + h);
    const Word *rw = reinterpret_cast<const Word *>(k.reads + h * kDReads);
    const Tail t = tail_of(gw[kGrpGroupWords - 1]);
    if (!grp_fits(t.mem, t.n_members, t.n_reads, k.n_state_members)) {
        if (l == 0) atomicOr(k.error, kGrpErrState);
        return;
    }
    const uint64_t *mu = reinterpret_cast<const uint64_t *>(k.members + t.mem);
    const uint32_t n_units = t.n_members * kGrpMemberUnits;
    // record words l (group | reads), 16 + l (reads | members) and 32 + l (members)
    const Word w0 = l < kGrpGroupWords ? gw[l] : rw[l - kGrpGroupWords];
    const uint32_t first_member = kGrpGroupWords + kGrpReadWords - kTeam;   // lane of member word 0
    const Word w1 = l < first_member ? rw[kTeam - kGrpGroupWords + l]
                                     : load_member_word(mu, l - first_member, n_units);
    const Word w2 = load_member_word(mu, kTeam - first_member + l, n_units);
    Word *out = reinterpret_cast<Word *>(k.records + i);
    out[l] = w0;
    out[kTeam + l] = w1;
    out[2 * kTeam + l] = w2;
}

__global__ void __launch_bounds__(kBlock) k_groups_scatter(GrpK k) {
    const uint64_t i = (uint64_t)blockIdx.x * kGroupsPerBlock + threadIdx.x / kTeam;
    const uint32_t l = threadIdx.x % kTeam;
    if (i >= k.n) return;
    const uint64_t h = k.handles[i];
    if (h >= k.n_state_groups) {
        if (l == 0) atomicOr(k.error, kGrpErrHandle);
        return;
    }
    const Word *in = reinterpret_cast<const Word *>(k.records + i);
    const Tail t = tail_of(in[kGrpGroupWords - 1]);
    if (!grp_fits(t.mem, t.n_members, t.n_reads, k.n_state_members)) {
        if (l == 0) atomicOr(k.error, kGrpErrState);
        return;
    }
    const Word w0 = in[l], w1 = in[kTeam + l], w2 = in[2 * kTeam + l];
    Word *gw = reinterpret_cast<Word *>(k.groups + h);
    Word *rw = reinterpret_cast<Word *>(k.reads + h * kDReads);
    uint64_t *mu = reinterpret_cast<uint64_t *>(k.members + t.mem);
    const uint32_t n_units = t.n_members * kGrpMemberUnits;
    const uint32_t first_member = kGrpGroupWords + kGrpReadWords - kTeam;
    if (l < kGrpGroupWords) gw[l] = w0;
    else rw[l - kGrpGroupWords] = w0;
    if (l < first_member) rw[kTeam - kGrpGroupWords + l] = w1;
    else store_member_word(mu, l - first_member, n_units, w1);
    store_member_word(mu, kTeam - first_member + l, n_units, w2);
}

}  // namespace

struct hq_groups_dev : hq::Sidecar {   // (totals: the error word as the host reads it)
    hq::PinBuf<hq_grp_record> records; // pinned: the gather's output, the scatter's input
    hq::PinBuf<uint32_t> handles_host; // pinned staging of the handles
    hq::DevBuf<uint32_t> handles;      // device, of handles_host's capacity
};

int hq_groups_dev_open(hq_ctx *ctx, hq_groups_dev **out) { return hq::sidecar_open(ctx, out, "hq_groups error word"); }

void hq_groups_dev_close(hq_groups_dev *c) { hq::sidecar_close(c); }

int hq_groups_dev_stage(hq_groups_dev *c, uint64_t n, hq_grp_record **records, uint32_t **handles) {
    hq_ctx *ctx = c->ctx;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc) rc = c->records.grow(ctx, n, "hq_groups records", hq::Headroom::kExact64);
    if (!rc) rc = c->handles_host.grow(ctx, n, "hq_groups handles", hq::Headroom::kExact64);
    if (rc) return rc;
    *records = c->records;
    *handles = c->handles_host;
    return HQ_OK;
}

namespace {

constexpr int kGrpGather = 0, kGrpScatter = 1;

int run(hq_groups_dev *c, int direction, const hq_dstate_mut *st, uint64_t n_member_records, uint64_t n,
        bool identity, uint64_t *gpu_ns, uint32_t *error) {
    hq_ctx *ctx = c->ctx;
    hipStream_t s = ctx->stream;
    *error = 0;
    *gpu_ns = 0;
    if (n == 0 || n > c->records.cap() || n > c->handles_host.cap() || (identity && direction != kGrpGather))
        return HQ_E_INVAL;
    if ((n + kGroupsPerBlock - 1) / kGroupsPerBlock > 0x7FFFFFFFull) return HQ_E_INVAL;
    int rc = hq::check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (!rc && !identity && n > c->handles.cap())
        rc = c->handles.reserve(ctx, c->handles_host.cap(), "hq_groups handles");
    if (rc) return rc;

    GrpK k{};
    k.groups = st->groups;
    k.reads = st->reads;
    k.members = st->members;
    k.n_state_groups = st->n_groups;
    k.n_state_members = n_member_records;
    k.handles = identity ? nullptr : c->handles.get();
    k.n = n;
    k.records = c->records;
    k.error = c->error();

    // (from here on every return is finish's: the staging is rewritten by the next call)
    rc = hq::check_hip(ctx, hipEventRecord(c->ev0, s), "event");
    if (!rc) rc = hq::check_hip(ctx, hipMemsetAsync(c->error(), 0, 16, s), "memset");
    if (!rc && !identity)
        rc = hq::check_hip(ctx, hipMemcpyAsync(c->handles, c->handles_host, n * 4, hipMemcpyHostToDevice, s),
                           "hq_groups handles");
    if (!rc) {
        const uint32_t grid = (uint32_t)((n + kGroupsPerBlock - 1) / kGroupsPerBlock);
        if (direction == kGrpGather) hipLaunchKernelGGL(k_groups_gather, dim3(grid), dim3(kBlock), 0, s, k);
        else hipLaunchKernelGGL(k_groups_scatter, dim3(grid), dim3(kBlock), 0, s, k);
        rc = hq::check_hip(ctx, hipGetLastError(), direction == kGrpGather ? "k_groups_gather" : "k_groups_scatter");
    }
    if (!rc)
        rc = hq::check_hip(ctx, hipMemcpyAsync(c->totals, c->error(), 4, hipMemcpyDeviceToHost, s),
                           "hq_groups error word");
    if (!rc) rc = hq::check_hip(ctx, hipEventRecord(c->ev1, s), "event");
    rc = hq::finish(ctx, rc, "hq_groups");
    if (rc) return rc;
    if ((uint32_t)c->totals[0]) {
        *error = (uint32_t)c->totals[0];
        return HQ_E_INVAL;
    }
    *gpu_ns = hq::elapsed_ns(c->ev0, c->ev1);
    return HQ_OK;
}

}  // namespace

int hq_groups_dev_gather(hq_groups_dev *c, const hq_dstate_view *st, uint64_t n_member_records, uint64_t n,
                         bool identity, uint64_t *gpu_ns, uint32_t *error) {
    // (the gather kernel only reads through these)
    const hq_dstate_mut m{st->ctx, const_cast<hq_dgroup *>(st->groups), const_cast<hq_dread *>(st->reads),
                          const_cast<hq_dmember *>(st->members), st->n_groups};
    return run(c, kGrpGather, &m, n_member_records, n, identity, gpu_ns, error);
}

int hq_groups_dev_scatter(hq_groups_dev *c, const hq_dstate_mut *st, uint64_t n_member_records, uint64_t n,
                          uint64_t *gpu_ns, uint32_t *error) {
    return run(c, kGrpScatter, st, n_member_records, n, false, gpu_ns, error);
}
