// hq_synth.hip — the synthetic input generators (hq_synth_commit_dev, hq_synth_commit_lag_dev,
// hq_synth_bitmaps_dev): benchmark and parity inputs written on the device, one thread per group,
// from a per-group splitmix64 stream (recipe: DESIGN.md "Synthetic inputs"; CPU twin
// oracle/qgen.c). Not a hot path: plain stores, no vector accesses.
#include "hq_commit_body.h"   // CommitCols
#include "hq_launch.h"

namespace {

__device__ __forceinline__ uint64_t splitmix64(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ int synth_n(const hq_synth_spec &s, uint64_t cid) {
    const uint32_t r = (uint32_t)(cid % 3);
    return s.mixed_n ? (r == 0 ? 3 : r == 1 ? 5 : 7) : (int)s.n_max;
}

// lag-layout outputs of the generator (hq_synth_commit_lag_dev); all NULL for the u64 layout
struct LagOut {
    int32_t *lag;
    uint64_t stride;
    int32_t *cin, *ts;
    uint16_t *mask;
    uint64_t *last;
};

__device__ __forceinline__ int32_t lag_of(uint64_t last, uint64_t x) {  // clamp(last - x)
    if (x <= last) {
        const uint64_t d = last - x;
        return d >= (uint64_t)INT32_MAX ? INT32_MAX : (int32_t)d;
    }
    const uint64_t d = x - last;
    return d >= (uint64_t)INT32_MAX + 1 ? INT32_MIN : -(int32_t)d;
}

__global__ __launch_bounds__(kBlock) void k_synth_commit(const hq_synth_spec s, CommitCols o,
                                                         LagOut lo) {
    const uint64_t R = s.ring_len;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < s.G;
         j += (uint64_t)gridDim.x * kBlock) {
        const uint64_t cid = s.cid_base + j * s.cid_stride;
        uint64_t st = s.seed ^ cid;
        const int n = synth_n(s, cid);
        const uint64_t term = 2 + splitmix64(st) % ((1ull << 20) - 2);
        const uint64_t last = (1ull << 20) + splitmix64(st) % (1ull << 40);
        uint64_t committed = last - splitmix64(st) % R;
        const uint64_t term_start = last - splitmix64(st) % R + 1;
        if (s.parity_extras) {
            const uint64_t x = splitmix64(st);
            if (x % 100 == 0) committed = last;
        }
        for (int k = 0; k < (int)s.n_max; ++k) {
            uint64_t m;
            if (k >= n) {
                m = 0;
            } else if (k == 0) {
                m = last;
            } else {
                const uint64_t x = splitmix64(st);
                const uint64_t y = splitmix64(st);
                m = committed - x % 4 + y % (last - committed + 4);
                if (m > last) m = last;
                if (s.parity_extras) {
                    const uint64_t c = splitmix64(st);
                    if (c % 100 == 0) m = last + 1 + (c / 100) % 3;
                }
            }
            if (o.match) const_cast<uint64_t *>(o.match)[(uint64_t)k * o.stride + j] = m;
            if (lo.lag) lo.lag[(uint64_t)k * lo.stride + j] = k < n ? lag_of(last, m) : 0;
        }
        if (lo.cin) lo.cin[j] = lag_of(last, committed);
        if (lo.ts) lo.ts[j] = lag_of(last, term_start);
        if (lo.last) lo.last[j] = last;
        if (o.nv) const_cast<uint8_t *>(o.nv)[j] = (uint8_t)n;
        if (o.cin) const_cast<uint64_t *>(o.cin)[j] = committed;
        if (o.last) const_cast<uint64_t *>(o.last)[j] = last;
        if (o.tstart) const_cast<uint64_t *>(o.tstart)[j] = term_start;
        if (o.term) const_cast<uint64_t *>(o.term)[j] = term;
        if (o.ring || o.mask || o.ring32 || lo.mask) {
            uint64_t cur = term;
            uint32_t mask = 0, lmask = 0;
            for (uint64_t k = 0; k < R; ++k) {
                const uint64_t i = last - k;
                uint64_t t;
                if (i >= term_start) {
                    t = term;
                } else {
                    const uint64_t x = splitmix64(st);
                    const uint64_t dec = (i + 1 == term_start) ? 1 + (x & 1) : (x & 1);
                    cur = cur > dec ? cur - dec : 1;
                    t = cur;
                }
                if (o.ring) const_cast<uint64_t *>(o.ring)[j * R + (i & (R - 1))] = t;
                if (o.ring32)
                    const_cast<uint32_t *>(o.ring32)[j * R + (i & (R - 1))] =
                        t < 0xFFFFFFFFull ? (uint32_t)t : 0xFFFFFFFFu;
                mask |= (uint32_t)(t == term) << (i & (R - 1));
                lmask |= (uint32_t)(t == term) << k;   // indexed by lag k = last - i
            }
            if (o.mask) const_cast<uint16_t *>(o.mask)[j] = (uint16_t)mask;
            if (lo.mask) lo.mask[j] = (uint16_t)lmask;
        }
    }
}

struct Bern {
    uint64_t st, buf;
    int avail;
    __device__ __forceinline__ bool operator()(uint32_t thr16) {
        if (avail == 0) {
            buf = splitmix64(st);
            avail = 4;
        }
        const uint32_t v = (uint32_t)(buf & 0xFFFF);
        buf >>= 16;
        --avail;
        return v < thr16;
    }
};

__global__ __launch_bounds__(kBlock) void k_synth_bits(const hq_synth_spec s, uint8_t *ack,
                                                       uint8_t *granted, uint8_t *rejected,
                                                       uint8_t *nv) {
    constexpr uint32_t P60 = 39322u, P30 = 19661u;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < s.G;
         j += (uint64_t)gridDim.x * kBlock) {
        const uint64_t cid = s.cid_base + j * s.cid_stride;
        Bern b{s.seed ^ cid, 0, 0};
        const int n = synth_n(s, cid);
        uint32_t a = 0, g = 1, r = 0;
        for (int k = 1; k < n; ++k)
            if (b(P60)) a |= 1u << k;
        for (int k = 1; k < n; ++k)
            if (b(P60)) g |= 1u << k;
        for (int k = 1; k < n; ++k)
            if (!((g >> k) & 1) && b(P30)) r |= 1u << k;
        if (s.parity_extras) {
            const uint64_t x = splitmix64(b.st);
            if (x % 50 == 0) r |= g & ~1u;
            if (x % 50 == 1) a |= 1u;
            if (x % 50 == 2) a |= 0xFFu & ~((1u << n) - 1);
        }
        if (ack) ack[j] = (uint8_t)a;
        if (granted) granted[j] = (uint8_t)g;
        if (rejected) rejected[j] = (uint8_t)r;
        if (nv) nv[j] = (uint8_t)n;
    }
}

}  // namespace

extern "C" int hq_synth_commit_dev(hq_ctx *ctx, const hq_synth_spec *s,
                                   const hq_commit_args *a) {
    if (!ctx) return HQ_E_INVAL;
    if (!s || !a) return hq::fail(ctx, HQ_E_INVAL, "hq_synth_commit: NULL argument");
    if (s->ring_len < 1 || (s->ring_len & (s->ring_len - 1)) || s->n_max < 1 || s->n_max > 8 ||
        s->cid_stride < 1 || (s->mixed_n && s->n_max < 7) || (a->match && a->match_stride < s->G))
        return hq::fail(ctx, HQ_E_INVAL, "hq_synth_commit: bad spec");
    if (s->G == 0) return HQ_OK;
    CommitCols o{};
    o.G = s->G;
    o.stride = a->match_stride;
    o.match = a->match;
    o.nv = a->n_voting;
    o.cin = a->committed_in;
    o.last = a->last_index;
    o.tstart = a->term_start;
    o.term = a->term;
    o.ring = a->ring;
    o.mask = a->term_mask;
    o.ring32 = a->ring32;
    if (o.mask && s->ring_len > 16)
        return hq::fail(ctx, HQ_E_INVAL, "hq_synth_commit: term_mask needs ring_len <= 16");
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(k_synth_commit, dim3(grid_for(ctx, s->G)), dim3(kBlock), 0, ctx->stream, *s, o,
                       LagOut{});
    return hq::post_launch(ctx, "k_synth_commit");
}

extern "C" int hq_synth_commit_lag_dev(hq_ctx *ctx, const hq_synth_spec *s,
                                       const hq_commit_lag_args *a, uint64_t *last_index) {
    if (!ctx) return HQ_E_INVAL;
    if (!s || !a) return hq::fail(ctx, HQ_E_INVAL, "hq_synth_commit_lag: NULL argument");
    if (s->ring_len < 1 || (s->ring_len & (s->ring_len - 1)) || s->n_max < 1 || s->n_max > 8 ||
        s->cid_stride < 1 || (s->mixed_n && s->n_max < 7) || (a->lag && a->lag_stride < s->G) ||
        (a->lag_mask && s->ring_len > 16))
        return hq::fail(ctx, HQ_E_INVAL, "hq_synth_commit_lag: bad spec");
    if (a->flags)   // the generator writes every slot's row; view rows 1.. with lag + lag_stride
        return hq::fail(ctx, HQ_E_INVAL, "hq_synth_commit_lag: generate with flags = 0");
    if (s->G == 0) return HQ_OK;
    CommitCols o{};
    o.G = s->G;
    o.nv = a->n_voting;
    LagOut lo{const_cast<int32_t *>(a->lag), a->lag_stride, const_cast<int32_t *>(a->cin_lag),
              const_cast<int32_t *>(a->ts_lag), const_cast<uint16_t *>(a->lag_mask), last_index};
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(k_synth_commit, dim3(grid_for(ctx, s->G)), dim3(kBlock), 0, ctx->stream, *s, o,
                       lo);
    return hq::post_launch(ctx, "k_synth_commit");
}

extern "C" int hq_synth_bitmaps_dev(hq_ctx *ctx, const hq_synth_spec *s, uint8_t *ack,
                                    uint8_t *granted, uint8_t *rejected, uint8_t *n_voting) {
    if (!ctx) return HQ_E_INVAL;
    if (!s || s->n_max < 1 || s->n_max > 8 || s->cid_stride < 1 || (s->mixed_n && s->n_max < 7))
        return hq::fail(ctx, HQ_E_INVAL, "hq_synth_bitmaps: bad spec");
    if (s->G == 0) return HQ_OK;
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(k_synth_bits, dim3(grid_for(ctx, s->G)), dim3(kBlock), 0, ctx->stream, *s, ack,
                       granted, rejected, n_voting);
    return hq::post_launch(ctx, "k_synth_bits");
}
