// hq_commit_lag.hip — commit over lags (hq_commit_lag_dev, hq_commit_lag_fused_dev): the match
// columns as int32 distances below lastIndex, half the bytes of the u64 columns.
//
// An HBM stream over int32 columns: four groups per lane, every column read with 16-byte loads
// of four int32 (consecutive lanes -> consecutive groups; one group per lane where a column is
// not aligned for that). The quorum-th largest match is the quorum-th SMALLEST lag, selected by an
// int32 min/max network in registers; the bitmaps come from wave-wide __ballot. No LDS.
#include "hq_launch.h"

namespace {

template <int N, bool PERN>
constexpr int lag_blk() {
    return !PERN && N <= 4 ? kCommitBlockBig : kCommitBlock;
}

constexpr int kMaxFused = 8;        // lag batches per fused launch
// k_commit_lag_fused's scan of first[] is unrolled as far as k_commit_fused's
// (hq_commit_tiles.hip); k < count <= kMaxFused keeps it inside the array
constexpr int kFusedScan = 32;

struct LagK {
    uint64_t G, stride, nwords;
    uint32_t n_max, R;
    const int32_t *lag;
    const uint8_t *nv;
    const int32_t *cin;
    int32_t *cout;
    const int32_t *ts;
    const uint16_t *mask;
    uint64_t *changed, *fallback;
};

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

constexpr int kLagVec = 4;   // groups per lane of the aligned lag kernels (16-byte loads)

__device__ __forceinline__ void ce_i32(int32_t &a, int32_t &b) {
    const int32_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

// the (n/2+1)-th smallest of v[0..n); slots >= n are padded with INT32_MAX (the maximum), so
// with a runtime n the (n/2+1)-th smallest of the padded N values is the same element
template <int N, bool PERN>
__device__ __forceinline__ int32_t lag_select(int32_t (&v)[N], int n) {
    if constexpr (!PERN && N == 1) {
        return v[0];
    } else if constexpr (!PERN && N == 2) {
        return v[0] > v[1] ? v[0] : v[1];   // quorum 2 of 2: the larger lag
    } else if constexpr (!PERN && N == 3) {  // median of 3
        ce_i32(v[0], v[1]);
        ce_i32(v[1], v[2]);
        return v[0] > v[1] ? v[0] : v[1];
    } else {
#pragma unroll
        for (int r = 0; r < N; ++r) {
#pragma unroll
            for (int i = r & 1; i + 1 < N; i += 2) ce_i32(v[i], v[i + 1]);
        }
        if constexpr (!PERN) return v[N / 2];   // index quorum - 1 = N/2
        const int idx = n / 2;
        int32_t r = 0;
#pragma unroll
        for (int k = 0; k < N; ++k) r = (k == idx) ? v[k] : r;
        return r;
    }
}

template <int N, int FORM, bool PERN>
__device__ __forceinline__ void decide_lag(const LagK &a, int32_t (&l)[N], int n, int32_t c,
                                           int32_t aux, int32_t &co, bool &chg, bool &fb) {
    co = c;
    chg = false;
    if constexpr (PERN) {
        fb = n < 1 || n > N;
#pragma unroll
        for (int s = 0; s < N; ++s) l[s] = (s < n) ? l[s] : INT32_MAX;
    } else {
        fb = false;
    }
    if constexpr (FORM == HQ_FORM_TERM_START) {
        fb |= c == INT32_MAX || c == INT32_MIN;   // committed not representable as a lag
    } else {
        fb |= c < 0 || c > (int32_t)a.R;
    }
    const int32_t d = lag_select<N, PERN>(l, n);
    if constexpr (FORM == HQ_FORM_TERM_START) {
        // q > committed, q <= last, q >= term_start (aux = ts_lag)
        chg = !fb & (d < c) & (d >= 0) & (d <= aux);
    } else {
        // bit d of the lag-indexed mask: term(last - d) == term (d < c <= R <= 16)
        chg = !fb & (d < c) & (d >= 0) && ((aux >> (d & 31)) & 1);
    }
    co = chg ? d : c;
}

// bit i of x (16 bits) -> bit 4i
__device__ __forceinline__ uint64_t spread16x4(uint32_t x) {
    uint64_t v = x & 0xFFFFu;
    v = (v | (v << 24)) & 0x000000FF000000FFull;
    v = (v | (v << 12)) & 0x000F000F000F000Full;
    v = (v | (v << 6)) & 0x0303030303030303ull;
    v = (v | (v << 3)) & 0x1111111111111111ull;
    return v;
}

template <int V> struct LagVec;   // VEC int32 lanes of one load
template <> struct LagVec<4> { typedef i32x4 T; typedef uint64_t M; typedef uint32_t NV; };

// bit i of the V ballots' 64/V-bit slice -> bit V*i + j of a bitmap word
template <int V>
__device__ __forceinline__ uint64_t spread_v(uint32_t x) {
    if constexpr (V == 4) return spread16x4(x);
    else return x;
}

// VEC = 4: lane owns groups g0..g0+3 (16-byte loads of every column); VEC = 1: one group,
// 4-byte loads. The body of workgroup `blk` of `nblk` on batch `a`.
// LEAD = 1 (HQ_LAG_LEADER_IMPLICIT): lag row s - 1 holds slot s, slot 0's lag is 0 (the
// leader's own match is lastIndex, raft.go:918, 1031): 4 bytes less per group.
template <int N, int FORM, int VEC, bool PERN, int BLK, int LEAD = 0>
__device__ __forceinline__ void lag_blocks(const LagK &a, uint64_t blk, uint64_t nblk) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = blk * (BLK / 64) + (threadIdx.x >> 6);
    const uint64_t step = nblk * BLK * VEC;
    for (uint64_t wbase = wave * 64 * VEC; wbase < a.G; wbase += step) {
        const uint64_t g0 = wbase + (uint64_t)lane * VEC;
        bool chg[VEC], fb[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) chg[j] = fb[j] = false;
        bool done = false;
        if constexpr (VEC > 1) {
            if (g0 + VEC <= a.G) {
                done = true;
                typedef typename LagVec<VEC>::T VT;
                int32_t l[VEC][N];
#pragma unroll
                for (int s = LEAD; s < N; ++s) {
                    const VT v = __builtin_nontemporal_load(
                        reinterpret_cast<const VT *>(a.lag + (s - LEAD) * a.stride + g0));
#pragma unroll
                    for (int j = 0; j < VEC; ++j) l[j][s] = v[j];
                }
                if constexpr (LEAD) {
#pragma unroll
                    for (int j = 0; j < VEC; ++j) l[j][0] = 0;
                }
                const VT ci = __builtin_nontemporal_load(reinterpret_cast<const VT *>(a.cin + g0));
                int32_t av[VEC];
                if constexpr (FORM == HQ_FORM_TERM_START) {
                    const VT t = __builtin_nontemporal_load(reinterpret_cast<const VT *>(a.ts + g0));
#pragma unroll
                    for (int j = 0; j < VEC; ++j) av[j] = t[j];
                } else {
                    // the lane's VEC u16 masks in one aligned load
                    typedef typename LagVec<VEC>::M MT;
                    const MT m = __builtin_nontemporal_load(reinterpret_cast<const MT *>(a.mask + g0));
#pragma unroll
                    for (int j = 0; j < VEC; ++j) av[j] = (int32_t)((m >> (16 * j)) & 0xFFFF);
                }
                int nn[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) nn[j] = N;
                if constexpr (PERN) {
                    typedef typename LagVec<VEC>::NV NT;
                    const NT x = *reinterpret_cast<const NT *>(a.nv + g0);
#pragma unroll
                    for (int j = 0; j < VEC; ++j) nn[j] = (x >> (8 * j)) & 0xFF;
                }
                VT co;
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    int32_t c;
                    decide_lag<N, FORM, PERN>(a, l[j], nn[j], ci[j], av[j], c, chg[j], fb[j]);
                    co[j] = c;
                }
                *reinterpret_cast<VT *>(a.cout + g0) = co;
            }
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const uint64_t g = g0 + j;
            if (!done && g < a.G) {
                int32_t l[N];
#pragma unroll
                for (int s = LEAD; s < N; ++s) l[s] = a.lag[(s - LEAD) * a.stride + g];
                if constexpr (LEAD) l[0] = 0;
                const int n = PERN ? (int)a.nv[g] : N;
                const int32_t aux = FORM == HQ_FORM_TERM_START ? a.ts[g] : (int32_t)a.mask[g];
                int32_t co;
                decide_lag<N, FORM, PERN>(a, l, n, a.cin[g], aux, co, chg[j], fb[j]);
                a.cout[g] = co;
            }
        }
        {
        // lane l owns groups VEC*l .. VEC*l+VEC-1 of the wave's 64*VEC: bitmap word k covers
        // lanes (64/VEC)*k .. (64/VEC)*(k+1)-1
        uint64_t bc[VEC], bf[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            bc[j] = __ballot(chg[j]);
            bf[j] = __ballot(fb[j]);
        }
        if (lane < VEC) {
            const int sh = (64 / VEC) * lane;
            const uint64_t w = (wbase >> 6) + lane;
            uint64_t wc = 0, wf = 0;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                wc |= spread_v<VEC>((uint32_t)(bc[j] >> sh)) << j;
                wf |= spread_v<VEC>((uint32_t)(bf[j] >> sh)) << j;
            }
            if (VEC == 1) {
                wc = bc[0];
                wf = bf[0];
            }
            if (w < a.nwords) {
                if (a.changed) a.changed[w] = wc;
                if (a.fallback) a.fallback[w] = wf;
            }
        }
    }
    }
}

template <int N, int FORM, int VEC, bool PERN, int LEAD>
__global__ __launch_bounds__(kCommitBlock) void k_commit_lag(const LagK a) {
    lag_blocks<N, FORM, VEC, PERN, kCommitBlock, LEAD>(a, blockIdx.x, gridDim.x);
}
template <int N, int FORM, int VEC, bool PERN, int LEAD>
__global__ __launch_bounds__(kCommitBlockBig, 8) void k_commit_lag_big(const LagK a) {
    lag_blocks<N, FORM, VEC, PERN, kCommitBlockBig, LEAD>(a, blockIdx.x, gridDim.x);
}

// the lag twin of k_commit_fused: uniform-n lag batches of one step in one launch
struct FusedLagK {
    LagK b[kMaxFused];
    uint32_t first[kMaxFused + 1];
    uint32_t n[kMaxFused];   // dwords: a scalar load (a byte array is read with a vector load + wait)
    uint32_t count;
};

template <int FORM, int BLK, int LEAD>
__global__ __launch_bounds__(BLK, BLK > kCommitBlock ? 8 : 1) void k_commit_lag_fused(const FusedLagK f) {
    const uint32_t blk = blockIdx.x;
    uint32_t i = 0;
#pragma unroll
    for (int k = 1; k < kFusedScan; ++k) i += (k < (int)f.count && blk >= f.first[k]) ? 1u : 0u;
    const uint64_t b = blk - f.first[i], nb = f.first[i + 1] - f.first[i];
    switch (f.n[i]) {
    case 1: lag_blocks<1, FORM, kLagVec, false, BLK, LEAD>(f.b[i], b, nb); break;
    case 2: lag_blocks<2, FORM, kLagVec, false, BLK, LEAD>(f.b[i], b, nb); break;
    case 3: lag_blocks<3, FORM, kLagVec, false, BLK, LEAD>(f.b[i], b, nb); break;
    case 4: lag_blocks<4, FORM, kLagVec, false, BLK, LEAD>(f.b[i], b, nb); break;
    case 5: lag_blocks<5, FORM, kLagVec, false, BLK, LEAD>(f.b[i], b, nb); break;
    case 6: lag_blocks<6, FORM, kLagVec, false, BLK, LEAD>(f.b[i], b, nb); break;
    case 7: lag_blocks<7, FORM, kLagVec, false, BLK, LEAD>(f.b[i], b, nb); break;
    default: lag_blocks<8, FORM, kLagVec, false, BLK, LEAD>(f.b[i], b, nb); break;
    }
}

template <int N, int FORM, int VEC, bool PERN, int LEAD>
int launch_lag_t(hq_ctx *ctx, const LagK &k) {
    constexpr int B = lag_blk<N, PERN>();
    const unsigned grid = grid_for_commit(ctx, (k.G + VEC - 1) / VEC, B);
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    if constexpr (B == kCommitBlock)
        hipLaunchKernelGGL((k_commit_lag<N, FORM, VEC, PERN, LEAD>), dim3(grid), dim3(B), 0,
                           ctx->stream, k);
    else
        hipLaunchKernelGGL((k_commit_lag_big<N, FORM, VEC, PERN, LEAD>), dim3(grid), dim3(B), 0,
                           ctx->stream, k);
    return hq::post_launch(ctx, "k_commit_lag");
}

int validate_lag(hq_ctx *ctx, const hq_commit_lag_args *a) {
    if (!ctx) return HQ_E_INVAL;
    if (!a) return hq::fail(ctx, HQ_E_INVAL, "hq_commit_lag: args is NULL");
    if (a->n_max < 1 || a->n_max > HQ_MAX_VOTERS)
        return hq::fail(ctx, HQ_E_INVAL, "hq_commit_lag: n_max must be 1..8");
    if (a->G == 0) return HQ_OK;
    if (!a->lag || !a->cin_lag || !a->cout_lag)
        return hq::fail(ctx, HQ_E_INVAL, "hq_commit_lag: NULL lag/cin_lag/cout_lag");
    if (a->lag_stride < a->G) return hq::fail(ctx, HQ_E_INVAL, "hq_commit_lag: lag_stride < G");
    if (a->flags & ~(uint32_t)HQ_LAG_LEADER_IMPLICIT)
        return hq::fail(ctx, HQ_E_INVAL, "hq_commit_lag: unknown flags");
    if (a->form == HQ_FORM_TERM_START) {
        if (!a->ts_lag) return hq::fail(ctx, HQ_E_INVAL, "hq_commit_lag: ts_lag is NULL");
    } else if (a->form == HQ_FORM_TERM_MASK) {
        if (!a->lag_mask) return hq::fail(ctx, HQ_E_INVAL, "hq_commit_lag: lag_mask is NULL");
        if (a->ring_len < 1 || a->ring_len > 16 || (a->ring_len & (a->ring_len - 1)))
            return hq::fail(ctx, HQ_E_INVAL, "hq_commit_lag: mask form needs ring_len <= 16 (power of two)");
    } else {
        return hq::fail(ctx, HQ_E_INVAL, "hq_commit_lag: form must be TERM_START or TERM_MASK");
    }
    return HQ_OK;
}

LagK lag_k(const hq_commit_lag_args *a) {
    LagK k;
    k.G = a->G;
    k.stride = a->lag_stride;
    k.nwords = hq::words64(a->G);
    k.n_max = a->n_max;
    k.R = a->ring_len;
    k.lag = a->lag;
    k.nv = a->n_voting;
    k.cin = a->cin_lag;
    k.cout = a->cout_lag;
    k.ts = a->ts_lag;
    k.mask = a->lag_mask;
    k.changed = a->changed;
    k.fallback = a->fallback;
    return k;
}

// every column can be read kLagVec groups per lane with aligned vector loads
bool lag_vec(const hq_commit_lag_args *a) {
    const uintptr_t al = 4 * kLagVec;   // bytes of one lane's int32 load
    auto ok = [&](const void *p, uintptr_t b) { return (reinterpret_cast<uintptr_t>(p) % b) == 0; };
    const bool aux_ok = a->form == HQ_FORM_TERM_START ? ok(a->ts_lag, al) : ok(a->lag_mask, al / 2);
    return ok(a->lag, al) && (a->lag_stride % kLagVec == 0) && ok(a->cin_lag, al) &&
           ok(a->cout_lag, al) && aux_ok && (!a->n_voting || ok(a->n_voting, al / 4));
}

}  // namespace

extern "C" int hq_commit_lag_dev(hq_ctx *ctx, const hq_commit_lag_args *a) {
    int rc = validate_lag(ctx, a);
    if (rc || a->G == 0) return rc;
    const LagK k = lag_k(a);
    const bool vec4 = lag_vec(a);
    const bool pern = a->n_voting != nullptr;
    const bool lead = (a->flags & HQ_LAG_LEADER_IMPLICIT) != 0;
    return dispatch_n(a->n_max, [&](auto n) {
        return dispatch<HQ_FORM_TERM_START, HQ_FORM_TERM_MASK>(a->form, [&](auto form) {
            return dispatch<kLagVec, 1>(vec4 ? kLagVec : 1, [&](auto vec) {
                return dispatch_bool(pern, [&](auto pn) {
                    return dispatch<1, 0>((int)lead, [&](auto ld) {
                        return launch_lag_t<decltype(n)::value, decltype(form)::value,
                                            decltype(vec)::value, decltype(pn)::value,
                                            decltype(ld)::value>(ctx, k);
                    });
                });
            });
        });
    });
}

extern "C" int hq_commit_lag_fused_dev(hq_ctx *ctx, const hq_commit_lag_args *args,
                                       uint32_t count) {
    if (!ctx) return HQ_E_INVAL;
    if (count && !args) return hq::fail(ctx, HQ_E_INVAL, "hq_commit_lag_fused_dev: args is NULL");
    for (uint32_t i = 0; i < count; ++i) {
        int rc = validate_lag(ctx, args + i);
        if (rc) return rc;
    }
    bool fusable = count >= 2 && count <= (uint32_t)kMaxFused;
    for (uint32_t i = 0; fusable && i < count; ++i)
        fusable = args[i].G > 0 && !args[i].n_voting && lag_vec(args + i) &&
                  args[i].form == args[0].form && args[i].flags == args[0].flags;
    if (!fusable) {
        for (uint32_t i = 0; i < count; ++i) {
            int rc = hq_commit_lag_dev(ctx, args + i);
            if (rc) return rc;
        }
        return HQ_OK;
    }
    FusedLagK f{};
    f.count = count;
    bool big = true;
    for (uint32_t i = 0; i < count; ++i) big &= args[i].n_max <= 4;
    const int B = big ? kCommitBlockBig : kCommitBlock;
    uint64_t blocks = 0;
    uint32_t order[kMaxFused];
    for (uint32_t i = 0; i < count; ++i) order[i] = i;
    for (uint32_t i = 1; i < count; ++i)   // the widest batches first, as in hq_commit_fused_dev
        for (uint32_t j = i; j > 0 && args[order[j]].n_max > args[order[j - 1]].n_max; --j) {
            const uint32_t t = order[j];
            order[j] = order[j - 1];
            order[j - 1] = t;
        }
    for (uint32_t i = 0; i < count; ++i) {
        const hq_commit_lag_args *b = args + order[i];
        f.b[i] = lag_k(b);
        f.n[i] = b->n_max;
        f.first[i] = (uint32_t)blocks;
        blocks += grid_for_commit(ctx, (b->G + kLagVec - 1) / kLagVec, B);
    }
    for (uint32_t i = count; i <= (uint32_t)kMaxFused; ++i) f.first[i] = (uint32_t)blocks;
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    const bool lead = (args[0].flags & HQ_LAG_LEADER_IMPLICIT) != 0;
    dispatch<HQ_FORM_TERM_START, HQ_FORM_TERM_MASK>(args[0].form, [&](auto form) {
        dispatch<1, 0>((int)lead, [&](auto ld) {
            dispatch<kCommitBlockBig, kCommitBlock>(B, [&](auto blk) {
                hipLaunchKernelGGL((k_commit_lag_fused<decltype(form)::value, decltype(blk)::value,
                                                       decltype(ld)::value>),
                                   dim3(blocks), dim3(B), 0, ctx->stream, f);
            });
        });
    });
    return hq::post_launch(ctx, "k_commit_lag_fused");
}
