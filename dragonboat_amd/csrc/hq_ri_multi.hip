// hq_ri_multi.hip — general multi-ctx ReadIndex: up to 8 pending ReadIndex
// contexts per group, released in queue order once a quorum has acked them. Columns
// (hq_readindex_multi_dev) and voter-major 128-group tiles (hq_readindex_multi_tiles_dev,
// packed by hq_tile_ri_multi_dev).
//
// One or two groups per lane; the reach time of a ctx is a rank of its voters' first-ack
// ordinals, selected by an 8-key sorting network in registers (packed u16 min / max for the
// two-group kernels); fallback bitmaps by wave-wide __ballot. No LDS.
#include <cstring>

#include "hq_launch.h"

namespace {

struct RiMultiK {
    uint64_t G;
    uint32_t K_max, n_max, n_uniform;
    const uint8_t *tiles;         // tiled layout (hq_readindex_multi_tiles_dev), else columns
    uint64_t tile_bytes;
    const uint16_t *ord;
    const uint64_t *idx;
    const uint8_t *np, *nv;
    uint64_t *rel;
    uint8_t *cnt;
    uint8_t *bend;
    uint64_t *fallback;
};

__device__ __forceinline__ void ce32(uint32_t &a, uint32_t &b) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

// Batcher's odd-even merge sort of 8 keys: 19 compare-exchanges in 6 layers (the transposition
// sort it replaced took 28); only the selected rank is read, so the compiler keeps just the
// min / max halves on its path
constexpr int kNet8[19][2] = {{0, 1}, {2, 3}, {4, 5}, {6, 7}, {0, 2}, {1, 3}, {4, 6},
                              {5, 7}, {1, 2}, {5, 6}, {0, 4}, {1, 5}, {2, 6}, {3, 7},
                              {2, 4}, {3, 5}, {1, 2}, {3, 4}, {5, 6}};

template <typename CE>
__device__ __forceinline__ void sort8(uint32_t (&v)[8], CE ce) {
#pragma unroll
    for (int c = 0; c < 19; ++c) ce(v[kNet8[c][0]], v[kNet8[c][1]]);
}

__device__ __forceinline__ void sort_net_u32(uint32_t (&v)[8]) {
    sort8(v, [](uint32_t &a, uint32_t &b) { ce32(a, b); });
}

template <bool PERK, bool PERN>
__global__ __launch_bounds__(kBlock) void k_ri_multi(const RiMultiK a) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t wbase = wave * 64; wbase < a.G; wbase += step) {
        const uint64_t g = wbase + lane;
        bool fb = false;
        if (g < a.G) {
            const uint32_t K = PERK ? a.np[g] : a.K_max;
            const uint32_t n = PERN ? a.nv[g] : a.n_uniform;
            fb = n < 1 || n > a.n_max || K > a.K_max;
            uint64_t idx[8];
            uint32_t t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                idx[k] = 0;
                t[k] = 0xFFFFu;
                if (!fb && k < (int)K) {
                    idx[k] = a.idx[(uint64_t)k * a.G + g];
                    fb |= k > 0 && idx[k] < idx[k - 1];   // addRequest: index moved backward
                    // reach time: the max(q-1, 1)-th smallest first-ack ordinal (readindex.go:84)
                    uint32_t v[8];
#pragma unroll
                    for (int s = 0; s < 8; ++s)
                        v[s] = (s < (int)n) ? a.ord[((uint64_t)k * a.n_max + s) * a.G + g] : 0xFFFFu;
                    sort_net_u32(v);
                    const int r = (int)(n / 2 + 1) - 1 > 1 ? (int)(n / 2 + 1) - 1 : 1;
                    uint32_t tk = 0xFFFFu;
#pragma unroll
                    for (int s = 0; s < 8; ++s) tk = (s == r - 1) ? v[s] : tk;
                    t[k] = tk;
                }
            }
            // suffix-min scan: entry i goes with the first ctx k >= i to reach quorum
            // (ties at equal reach times go to the earlier ctx: the replay's queue order)
            uint32_t best_t = 0xFFFFu;
            uint64_t best_idx = 0;
            uint32_t released = 0, bend = 0;
#pragma unroll
            for (int k = 7; k >= 0; --k) {
                bool own = false;
                if (!fb && k < (int)K && t[k] != 0xFFFFu && t[k] <= best_t) {
                    best_t = t[k];
                    best_idx = idx[k];
                    own = true;
                }
                const bool rel = !fb && k < (int)K && best_t != 0xFFFFu;
                released += rel;
                // entry k closes its release batch: it is the ctx whose confirm() released
                // the batch (readindex.go:96), whose ctx the ReadIndexResp hints carry
                bend |= (uint32_t)(rel && own) << k;
                if (a.rel && k < (int)a.K_max) a.rel[(uint64_t)k * a.G + g] = rel ? best_idx : ~0ull;
            }
            a.cnt[g] = (uint8_t)released;
            if (a.bend) a.bend[g] = (uint8_t)bend;
        }
        const uint64_t fw = __ballot(fb);
        if (a.fallback && lane == 0) a.fallback[wbase >> 6] = fw;
    }
}


// Two adjacent groups per lane (even G, aligned columns): the u16 first-ack ordinals of both
// groups travel packed in one 32-bit register, so one 4-byte load reads a (ctx, voter) pair and
// the sorting network runs on both groups at once with packed u16 min / max (v_pk_min_u16 /
// v_pk_max_u16); the ctx indexes and released indexes move as 16-byte pairs. Same decisions as
// k_ri_multi (the suffix-min release of readindex.go:77-116).
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void ce_pk(uint32_t &a, uint32_t &b) {
    const u16x2 x = __builtin_bit_cast(u16x2, a), y = __builtin_bit_cast(u16x2, b);
    a = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(x, y));
    b = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(x, y));
}

// KM >= K_max ctx slots in registers: every (ctx, voter) load of the lane is issued before the
// first sorting network (K_max and n_max are uniform, so the guards are scalar branches; with the
// loads inside the per-ctx branches each ctx waited for its own round trip). The lane's two
// groups' loads (ri_load) and their decision (ri_decide) are written apart; a software-pipelined
// form that issued the next tile's loads before deciding the current one (2, 4 or 8 tiles per
// wave at 3 waves per SIMD) was no faster: 50.6-53.3 vs 50.3-51.5 us, profiles/r04b/ab_rimt.log.
template <bool PERK, bool PERN, int KM>
struct RiIn {
    u64x2 idx[KM];
    uint32_t ov[KM][8];
    uint32_t kk, nn;              // PERK / PERN: the two groups' K / n bytes
};

// TILED: the voter-major tile (include/hipquorum.h): voter s's block of K_max * 256 bytes holds,
// for lane l, the K_max ctx ordinal dwords of groups 2 l, 2 l + 1 back to back; EXACT (K_max ==
// KM) reads them as vectors (one 16-byte load per voter at K_max = 4), otherwise dword by dword.
template <bool PERK, bool PERN, int KM, bool TILED, bool EXACT = false>
__device__ __forceinline__ void ri_load(const RiMultiK &a, uint64_t wbase, int lane,
                                        RiIn<PERK, PERN, KM> &in) {
    const uint64_t g = wbase + 2 * (uint64_t)lane;
    // TILED: the wave's 128 groups are one tile (wbase is a multiple of 128)
    const uint8_t *tb = TILED ? a.tiles + (wbase >> 7) * a.tile_bytes : nullptr;
    const uint64_t ord_bytes = (uint64_t)a.K_max * a.n_max * 256;
    in.kk = in.nn = 0;
    if (g >= a.G) return;         // columns: G is even, g + 1 < G too; tiles: padded rows
    if constexpr (PERK)
        in.kk = TILED ? *reinterpret_cast<const uint16_t *>(tb + ord_bytes + a.K_max * 1024ull +
                                                           2 * lane)
                      : *reinterpret_cast<const uint16_t *>(a.np + g);
    if constexpr (PERN)
        in.nn = TILED ? *reinterpret_cast<const uint16_t *>(tb + ord_bytes + a.K_max * 1024ull +
                                                           (PERK ? 128 : 0) + 2 * lane)
                      : *reinterpret_cast<const uint16_t *>(a.nv + g);
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        in.idx[k] = (u64x2){0, 0};
        if (k < (int)a.K_max)
            in.idx[k] = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(
                TILED ? tb + ord_bytes + k * 1024ull + 16 * lane
                      : reinterpret_cast<const uint8_t *>(a.idx + (uint64_t)k * a.G + g)));
    }
#pragma unroll
    for (int sl = 0; sl < 8; ++sl) {
#pragma unroll
        for (int k = 0; k < KM; ++k) in.ov[k][sl] = 0xFFFFFFFFu;
        if (sl >= (int)a.n_max) continue;
        if constexpr (TILED) {
            const uint8_t *p = tb + (uint64_t)sl * a.K_max * 256 + (uint64_t)lane * 4 * a.K_max;
            if constexpr (EXACT && KM == 2) {
                const u32x2 w = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(p));
                in.ov[0][sl] = w.x;
                in.ov[1][sl] = w.y;
            } else if constexpr (EXACT) {
#pragma unroll
                for (int q = 0; q < KM / 4; ++q) {
                    const u32x4 w = __builtin_nontemporal_load(
                        reinterpret_cast<const u32x4 *>(p + 16 * q));
                    in.ov[4 * q + 0][sl] = w.x;
                    in.ov[4 * q + 1][sl] = w.y;
                    in.ov[4 * q + 2][sl] = w.z;
                    in.ov[4 * q + 3][sl] = w.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < KM; ++k)
                    if (k < (int)a.K_max)
                        in.ov[k][sl] = __builtin_nontemporal_load(
                            reinterpret_cast<const uint32_t *>(p + 4 * k));
            }
        } else {
#pragma unroll
            for (int k = 0; k < KM; ++k)
                if (k < (int)a.K_max)
                    in.ov[k][sl] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(
                        a.ord + ((uint64_t)k * a.n_max + sl) * a.G + g));
        }
    }
}

template <bool PERK, bool PERN, int KM, bool TILED>
__device__ __forceinline__ void ri_decide(const RiMultiK &a, uint64_t wbase, int lane,
                                          const RiIn<PERK, PERN, KM> &in) {
    const uint64_t g = wbase + 2 * (uint64_t)lane;
    bool fb0 = false, fb1 = false;
    if (g < a.G) {
        uint32_t K0 = a.K_max, K1 = a.K_max, n0 = a.n_uniform, n1 = a.n_uniform;
        if constexpr (PERK) {
            K0 = in.kk & 0xFF;
            K1 = in.kk >> 8;
        }
        if constexpr (PERN) {
            n0 = in.nn & 0xFF;
            n1 = in.nn >> 8;
        }
        fb0 = n0 < 1 || n0 > a.n_max || K0 > a.K_max;
        fb1 = n1 < 1 || n1 > a.n_max || K1 > a.K_max;
        // padding of the voters >= n, per half (0xFFFF = never acked)
        const int r0 = n0 / 2 > 1 ? (int)(n0 / 2) : 1, r1 = n1 / 2 > 1 ? (int)(n1 / 2) : 1;
        const uint32_t kmax = K0 > K1 ? K0 : K1;
        uint32_t t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            t[k] = 0xFFFFFFFFu;
            if (k < KM && k < (int)kmax && k < (int)a.K_max) {
                uint32_t v[8];
#pragma unroll
                for (int sl = 0; sl < 8; ++sl)
                    v[sl] = in.ov[k < KM ? k : 0][sl] | (sl < (int)n0 ? 0u : 0xFFFFu) |
                            (sl < (int)n1 ? 0u : 0xFFFF0000u);
                sort8(v, [](uint32_t &x, uint32_t &y) { ce_pk(x, y); });
                // reach time: the max(q-1, 1)-th smallest first-ack ordinal (readindex.go:84)
                uint32_t tk = 0;
#pragma unroll
                for (int sl = 0; sl < 8; ++sl) {
                    const uint32_t m = (sl == r0 - 1 ? 0xFFFFu : 0u) |
                                       (sl == r1 - 1 ? 0xFFFF0000u : 0u);
                    tk |= v[sl] & m;
                }
                t[k] = tk;
            }
        }
        u64x2 idx[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) idx[k] = k < KM ? in.idx[k < KM ? k : 0] : (u64x2){0, 0};
#pragma unroll
        for (int k = 1; k < 8; ++k) {   // addRequest: index moved backward
            if (k < KM && k < (int)kmax && k < (int)a.K_max) {
                fb0 |= k < (int)K0 && idx[k].x < idx[k - 1].x;
                fb1 |= k < (int)K1 && idx[k].y < idx[k - 1].y;
            }
        }
        // suffix-min scan per group (ties go to the earlier ctx, as in k_ri_multi)
        uint32_t bt0 = 0xFFFFu, bt1 = 0xFFFFu, rel0 = 0, rel1 = 0, be0 = 0, be1 = 0;
        uint64_t bi0 = 0, bi1 = 0;
#pragma unroll
        for (int k = 7; k >= 0; --k) {
            const uint32_t t0 = t[k] & 0xFFFFu, t1 = t[k] >> 16;
            const bool in0 = !fb0 && k < (int)K0, in1 = !fb1 && k < (int)K1;
            bool own0 = false, own1 = false;
            if (in0 && t0 != 0xFFFFu && t0 <= bt0) { bt0 = t0; bi0 = idx[k].x; own0 = true; }
            if (in1 && t1 != 0xFFFFu && t1 <= bt1) { bt1 = t1; bi1 = idx[k].y; own1 = true; }
            const bool rl0 = in0 && bt0 != 0xFFFFu, rl1 = in1 && bt1 != 0xFFFFu;
            rel0 += rl0;
            rel1 += rl1;
            be0 |= (uint32_t)(rl0 && own0) << k;
            be1 |= (uint32_t)(rl1 && own1) << k;
            if (a.rel && k < (int)a.K_max) {
                uint64_t *r = a.rel + (uint64_t)k * a.G + g;
                if (!TILED || g + 1 < a.G) {
                    *reinterpret_cast<u64x2 *>(r) = (u64x2){rl0 ? bi0 : ~0ull, rl1 ? bi1 : ~0ull};
                } else {
                    r[0] = rl0 ? bi0 : ~0ull;   // odd G: the tile's padding group has no slot
                }
            }
        }
        if (!TILED || g + 1 < a.G) {
            *reinterpret_cast<uint16_t *>(a.cnt + g) = (uint16_t)(rel0 | (rel1 << 8));
            if (a.bend) *reinterpret_cast<uint16_t *>(a.bend + g) = (uint16_t)(be0 | (be1 << 8));
        } else {
            a.cnt[g] = (uint8_t)rel0;
            if (a.bend) a.bend[g] = (uint8_t)be0;
            fb1 = false;
        }
    }
    const uint64_t f0 = __ballot(fb0), f1 = __ballot(fb1);
    if (a.fallback && lane < 2) {
        const uint32_t sh = 32 * lane;
        const uint64_t w = (wbase >> 6) + lane;
        if (w < (a.G + 63) >> 6)
            a.fallback[w] = spread32((uint32_t)(f0 >> sh)) | (spread32((uint32_t)(f1 >> sh)) << 1);
    }
}

template <bool PERK, bool PERN, int KM, bool TILED = false, bool EXACT = false>
__global__ __launch_bounds__(kBlock) void k_ri_multi2(const RiMultiK a) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const uint64_t step = (uint64_t)gridDim.x * kBlock * 2;
    for (uint64_t wbase = wave * 128; wbase < a.G; wbase += step) {
        RiIn<PERK, PERN, KM> in;
        ri_load<PERK, PERN, KM, TILED, EXACT>(a, wbase, lane, in);
        ri_decide<PERK, PERN, KM, TILED>(a, wbase, lane, in);
    }
}

// Uniform wide tiles (K_max == KM ctx slots and n_uniform == n_max == N voters in every group,
// the voter-major ordinal layout): every bound is a constant, so the loads are N 16-byte reads
// (KM = 4) plus KM ctx-index reads with no guards, the rank max(q - 1, 1) = max(N / 2, 1) is a
// constant that prunes the network to the comparators that reach it, and no per-half masks or
// SGPR-held exec masks remain. Same decisions as ri_decide (readindex.go:77-116).
template <int KM, int N>
__global__ __launch_bounds__(kBlock) void k_ri_tiles_u(const RiMultiK a) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const uint64_t step = (uint64_t)gridDim.x * kBlock * 2;
    constexpr int R = N / 2 > 1 ? N / 2 : 1;
    for (uint64_t wbase = wave * 128; wbase < a.G; wbase += step) {
        const uint64_t g = wbase + 2 * (uint64_t)lane;   // G even: g < G implies g + 1 < G
        bool fb0 = false, fb1 = false;
        if (g < a.G) {
            const uint8_t *tb = a.tiles + (wbase >> 7) * a.tile_bytes;
            uint32_t ov[KM][N];
#pragma unroll
            for (int sl = 0; sl < N; ++sl) {
                const uint8_t *p = tb + sl * KM * 256 + lane * 4 * KM;
                if constexpr (KM == 2) {
                    const u32x2 w = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(p));
                    ov[0][sl] = w.x;
                    ov[1][sl] = w.y;
                } else {
#pragma unroll
                    for (int q = 0; q < KM / 4; ++q) {
                        const u32x4 w = __builtin_nontemporal_load(
                            reinterpret_cast<const u32x4 *>(p + 16 * q));
                        ov[4 * q + 0][sl] = w.x;
                        ov[4 * q + 1][sl] = w.y;
                        ov[4 * q + 2][sl] = w.z;
                        ov[4 * q + 3][sl] = w.w;
                    }
                }
            }
            u64x2 idx[KM];
#pragma unroll
            for (int k = 0; k < KM; ++k)
                idx[k] = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(
                    tb + N * KM * 256 + k * 1024 + 16 * lane));
            uint32_t t[KM];
#pragma unroll
            for (int k = 0; k < KM; ++k) {
                uint32_t v[8];
#pragma unroll
                for (int sl = 0; sl < 8; ++sl) v[sl] = sl < N ? ov[k][sl < N ? sl : 0] : 0xFFFFFFFFu;
                sort8(v, [](uint32_t &x, uint32_t &y) { ce_pk(x, y); });
                t[k] = v[R - 1];       // the R-th smallest first-ack ordinal of both groups
            }
#pragma unroll
            for (int k = 1; k < KM; ++k) {   // addRequest: index moved backward
                fb0 |= idx[k].x < idx[k - 1].x;
                fb1 |= idx[k].y < idx[k - 1].y;
            }
            uint32_t bt0 = 0xFFFFu, bt1 = 0xFFFFu, rel0 = 0, rel1 = 0, be0 = 0, be1 = 0;
            uint64_t bi0 = 0, bi1 = 0;
#pragma unroll
            for (int k = KM - 1; k >= 0; --k) {
                const uint32_t t0 = t[k] & 0xFFFFu, t1 = t[k] >> 16;
                bool own0 = false, own1 = false;
                if (t0 != 0xFFFFu && t0 <= bt0) { bt0 = t0; bi0 = idx[k].x; own0 = true; }
                if (t1 != 0xFFFFu && t1 <= bt1) { bt1 = t1; bi1 = idx[k].y; own1 = true; }
                const bool rl0 = !fb0 && bt0 != 0xFFFFu, rl1 = !fb1 && bt1 != 0xFFFFu;
                rel0 += rl0;
                rel1 += rl1;
                be0 |= (uint32_t)(rl0 && own0) << k;
                be1 |= (uint32_t)(rl1 && own1) << k;
                if (a.rel)
                    *reinterpret_cast<u64x2 *>(a.rel + (uint64_t)k * a.G + g) =
                        (u64x2){rl0 ? bi0 : ~0ull, rl1 ? bi1 : ~0ull};
            }
            *reinterpret_cast<uint16_t *>(a.cnt + g) = (uint16_t)(rel0 | (rel1 << 8));
            if (a.bend) *reinterpret_cast<uint16_t *>(a.bend + g) = (uint16_t)(be0 | (be1 << 8));
        }
        const uint64_t f0 = __ballot(fb0), f1 = __ballot(fb1);
        if (a.fallback && lane < 2) {
            const uint32_t sh = 32 * lane;
            const uint64_t w = (wbase >> 6) + lane;
            if (w < (a.G + 63) >> 6)
                a.fallback[w] = spread32((uint32_t)(f0 >> sh)) | (spread32((uint32_t)(f1 >> sh)) << 1);
        }
    }
}

}  // namespace

extern "C" int hq_readindex_multi_dev(hq_ctx *ctx, uint64_t G, uint32_t K_max, uint32_t n_max,
                                      const uint16_t *ack_ordinal, const uint64_t *ctx_index,
                                      const uint8_t *n_pending, const uint8_t *n_voting,
                                      uint32_t n_uniform, uint64_t *released_index,
                                      uint8_t *released_count, uint8_t *batch_end,
                                      uint64_t *fallback) {
    if (!ctx) return HQ_E_INVAL;
    if (G == 0) return HQ_OK;
    // released_index may be NULL when batch_end is given (the caller derives it from ctx_index)
    if (!ack_ordinal || !ctx_index || (!released_index && !batch_end) || !released_count ||
        K_max < 1 || K_max > 8 || n_max < 1 || n_max > 8 ||
        (!n_voting && (n_uniform < 1 || n_uniform > 8)))
        return hq::fail(ctx, HQ_E_INVAL, "hq_readindex_multi_dev: bad arguments");
    RiMultiK k{G, K_max, n_max, n_uniform, nullptr, 0, ack_ordinal, ctx_index, n_pending,
               n_voting, released_index, released_count, batch_end, fallback};
    auto al = [](const void *p, uintptr_t m) { return ((uintptr_t)p & (m - 1)) == 0; };
    const bool pairs = ctx->ri_pairs && G % 2 == 0 && al(ack_ordinal, 4) && al(ctx_index, 16) &&
                       al(released_index, 16) && al(released_count, 2) && al(batch_end, 2) &&
                       al(n_pending, 2) && al(n_voting, 2);
    const unsigned grid = pairs ? grid_for(ctx, G / 2) : grid_for(ctx, G);
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    const int km = K_max <= 2 ? 2 : K_max <= 4 ? 4 : 8;   // ctx slots the pair kernel holds
    dispatch_bool(n_pending != nullptr, [&](auto perk) {
        dispatch_bool(n_voting != nullptr, [&](auto pern) {
            constexpr bool PK = decltype(perk)::value, PN = decltype(pern)::value;
            if (pairs)
                dispatch<2, 4, 8>(km, [&](auto kmv) {
                    hipLaunchKernelGGL((k_ri_multi2<PK, PN, decltype(kmv)::value>), dim3(grid),
                                       dim3(kBlock), 0, ctx->stream, k);
                });
            else
                hipLaunchKernelGGL((k_ri_multi<PK, PN>), dim3(grid), dim3(kBlock), 0,
                                   ctx->stream, k);
        });
    });
    return hq::post_launch(ctx, pairs ? "k_ri_multi2" : "k_ri_multi");
}

namespace {

// columns -> multi-ctx ReadIndex tiles: one thread per (tile, row, 16-byte chunk)
__global__ __launch_bounds__(kBlock) void k_tile_ri_multi(uint64_t G, uint32_t K_max,
                                                          uint32_t n_max, const uint16_t *ord,
                                                          const uint64_t *idx, const uint8_t *np,
                                                          const uint8_t *nv, uint8_t *tiles,
                                                          uint64_t tile_bytes) {
    const uint64_t ntiles = (G + HQ_RI_TILE_GROUPS - 1) / HQ_RI_TILE_GROUPS;
    const uint64_t chunks = tile_bytes / 16;
    const uint64_t ord_rows = (uint64_t)K_max * n_max, ord_bytes = ord_rows * 256;
    for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < ntiles * chunks;
         q += (uint64_t)gridDim.x * kBlock) {
        const uint64_t t = q / chunks, off = (q % chunks) * 16;
        const uint64_t g0 = t * HQ_RI_TILE_GROUPS;
        uint8_t v[16];
        if (off < ord_bytes) {                           // 8 u16 ordinal entries
            for (int e = 0; e < 8; ++e) {
                // voter sl's block of K_max * 256 bytes: pair l's K_max dwords (groups 2 l and
                // 2 l + 1 of ctx k at dword k)
                const uint64_t b = off + 2 * e;
                const uint64_t sl = b / (K_max * 256ull), r = b % (K_max * 256ull);
                const uint64_t l = r / (4ull * K_max), w = r % (4ull * K_max);
                const uint64_t row = (w / 4) * n_max + sl, j = 2 * l + (w % 4) / 2;
                const uint64_t g = g0 + j;
                const uint16_t x = g < G ? ord[row * G + g] : 0xFFFFu;
                v[2 * e] = (uint8_t)x;
                v[2 * e + 1] = (uint8_t)(x >> 8);
            }
        } else if (off < ord_bytes + K_max * 1024ull) {  // 2 u64 entries of ctx row
            const uint64_t o = off - ord_bytes, k = o / 1024, j = (o % 1024) / 8;
            for (int e = 0; e < 2; ++e) {
                const uint64_t g = g0 + j + e;
                const uint64_t x = g < G ? idx[k * G + g] : 0;
                for (int b = 0; b < 8; ++b) v[8 * e + b] = (uint8_t)(x >> (8 * b));
            }
        } else {                                         // the u8 rows: n_pending, n_voting
            const uint64_t o = off - ord_bytes - K_max * 1024ull;
            const uint8_t *src = (np && o < 128) ? np : nv;
            const uint64_t j = o % 128;
            for (int e = 0; e < 16; ++e) {
                const uint64_t g = g0 + j + e;
                v[e] = g < G && src ? src[g] : 0;
            }
        }
        uint4 w;
        memcpy(&w, v, 16);
        *reinterpret_cast<uint4 *>(tiles + t * tile_bytes + off) = w;
    }
}

}  // namespace

extern "C" int hq_readindex_multi_tiles_dev(hq_ctx *ctx, uint64_t G, uint32_t K_max,
                                            uint32_t n_max, const uint8_t *tiles, uint32_t flags,
                                            uint32_t n_uniform, uint64_t *released_index,
                                            uint8_t *released_count, uint8_t *batch_end,
                                            uint64_t *fallback) {
    if (!ctx) return HQ_E_INVAL;
    if (G == 0) return HQ_OK;
    const bool perk = flags & HQ_RI_TILE_PER_K, pern = flags & HQ_RI_TILE_PER_N;
    if (!tiles || (!released_index && !batch_end) || !released_count || K_max < 1 || K_max > 8 ||
        n_max < 1 || n_max > 8 || (flags & ~(HQ_RI_TILE_PER_K | HQ_RI_TILE_PER_N)) ||
        (!pern && (n_uniform < 1 || n_uniform > 8)) || !hq::aligned16(tiles) ||
        (reinterpret_cast<uintptr_t>(released_index) & 15) ||
        (reinterpret_cast<uintptr_t>(released_count) & 1) ||
        (batch_end && (reinterpret_cast<uintptr_t>(batch_end) & 1)))
        return hq::fail(ctx, HQ_E_INVAL, "hq_readindex_multi_tiles_dev: bad arguments");
    RiMultiK k{G, K_max, n_max, n_uniform, tiles, hq_ri_tile_bytes(K_max, n_max, flags),
               nullptr, nullptr, nullptr, nullptr, released_index, released_count, batch_end,
               fallback};
    // the pair kernel's column stores need 16-byte rows: G even keeps k * G + g aligned
    if (G % 2)
        return hq::fail(ctx, HQ_E_INVAL, "hq_readindex_multi_tiles_dev: G must be even");
    const unsigned grid = grid_for(ctx, G / 2);
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    const int km = K_max <= 2 ? 2 : K_max <= 4 ? 4 : 8;
    const bool exact = (uint32_t)km == K_max;
    if (exact && ctx->ri_uniform && !perk && !pern && n_uniform == n_max) {
        dispatch<2, 4, 8>(km, [&](auto kmv) {
            dispatch_n(n_max, [&](auto n) {
                hipLaunchKernelGGL((k_ri_tiles_u<decltype(kmv)::value, decltype(n)::value>),
                                   dim3(grid), dim3(kBlock), 0, ctx->stream, k);
            });
        });
        return hq::post_launch(ctx, "k_ri_tiles_u");
    }
    dispatch_bool(perk, [&](auto pk) {
        dispatch_bool(pern, [&](auto pn) {
            dispatch<2, 4, 8>(km, [&](auto kmv) {
                dispatch_bool(exact, [&](auto ex) {
                    hipLaunchKernelGGL(
                        (k_ri_multi2<decltype(pk)::value, decltype(pn)::value,
                                     decltype(kmv)::value, true, decltype(ex)::value>),
                        dim3(grid), dim3(kBlock), 0, ctx->stream, k);
                });
            });
        });
    });
    return hq::post_launch(ctx, "k_ri_multi2<tiles>");
}

extern "C" int hq_tile_ri_multi_dev(hq_ctx *ctx, uint64_t G, uint32_t K_max, uint32_t n_max,
                                    const uint16_t *ack_ordinal, const uint64_t *ctx_index,
                                    const uint8_t *n_pending, const uint8_t *n_voting,
                                    uint8_t *tiles) {
    if (!ctx) return HQ_E_INVAL;
    if (G == 0) return HQ_OK;
    if (!ack_ordinal || !ctx_index || !tiles || K_max < 1 || K_max > 8 || n_max < 1 ||
        n_max > 8 || !hq::aligned16(tiles))
        return hq::fail(ctx, HQ_E_INVAL, "hq_tile_ri_multi_dev: bad arguments");
    const uint32_t flags = (n_pending ? HQ_RI_TILE_PER_K : 0) | (n_voting ? HQ_RI_TILE_PER_N : 0);
    const uint64_t tb = hq_ri_tile_bytes(K_max, n_max, flags);
    const uint64_t ntiles = (G + HQ_RI_TILE_GROUPS - 1) / HQ_RI_TILE_GROUPS;
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tile_ri_multi, dim3(grid_for(ctx, ntiles * (tb / 16))), dim3(kBlock), 0,
                       ctx->stream, G, K_max, n_max, ack_ordinal, ctx_index, n_pending, n_voting,
                       tiles, tb);
    return hq::post_launch(ctx, "k_tile_ri_multi");
}
