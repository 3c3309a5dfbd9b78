// hq_commit.h — what hq_commit.hip (columns) and hq_commit_tiles.hip (tiles, fused launch) share:
// the k_commit / k_commit_big kernels with the column body, their launcher, and the validation
// and argument packing of a hq_commit_args batch. Each of the two files instantiates the kernels
// of its own layouts only; the tile body (tile_blocks) is defined in hq_commit_tiles.hip.
#pragma once

#include "hq_commit_body.h"
#include "hq_launch.h"

namespace hq {
// hq_commit_dev's tile arm (hq_commit_tiles.hip): a validated batch in a tile layout
int launch_commit_tiles(hq_ctx *ctx, const hq_commit_args *a);
}  // namespace hq

namespace {

template <int N, int FORM, bool PERN>
constexpr int commit_blk() {
    return !PERN && N <= 5 ? kCommitBlockBig : kCommitBlock;
}

// VEC = groups per lane (2: 16-byte loads of every SoA column; 1: 8-byte loads). The body of
// one workgroup `blk` of `nblk` working on batch `a` (k_commit: the grid; k_commit_fused: the
// workgroups one batch of the launch owns). TILED (HQ_LAYOUT_TILES, VEC = 2 only): a wave's 128
// groups are one tile, so its loads walk one contiguous 128·(n+3)·8-byte block instead of n + 3
// column streams. TILED = 2 (HQ_LAYOUT_TILES_LEADER): the same tiles without the leader's match
// row; slot 0 is last_index (the leader's own match, raft.go:918, 1031).
template <int N, int FORM, bool PERN, int BLK, int LEAD, bool INPLACE = false>
__device__ __forceinline__ void tile_blocks(const CommitK &a, uint64_t blk, uint64_t nblk);

template <int N, int FORM, int VEC, bool PERN, int BLK>
__device__ __forceinline__ void column_blocks(const CommitK &a, uint64_t blk, uint64_t nblk) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = blk * (BLK / 64) + (threadIdx.x >> 6);
    const uint64_t step = nblk * BLK * VEC;
    for (uint64_t wbase = wave * 64 * VEC; wbase < a.G; wbase += step) {
        const uint64_t g0 = wbase + (uint64_t)lane * VEC;
        // every input field as a base + this lane's element offset: slot s of match at
        // bm[s * ms + off], then committed_in, last_index and aux (term_start / term as u64, or
        // the u16 mask)
        const uint64_t *bm = a.match, *bcin = a.cin, *blast = a.last;
        const uint64_t *baux = static_cast<const uint64_t *>(a.aux);
        const uint16_t *bmask = static_cast<const uint16_t *>(a.aux);
        const uint64_t ms = a.stride, off = g0;
        auto aux1 = [&]() -> uint64_t {
            if constexpr (FORM == HQ_FORM_TERM_MASK) return bmask[off];
            return baux[off];
        };
        bool chg[VEC], fb[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) chg[j] = fb[j] = false;
        if constexpr (VEC == 2) {
            // both groups of the lane: 16-byte loads of every field
            auto pair = [&]() {
                uint64_t m0[N], m1[N];
#pragma unroll
                for (int s = 0; s < N; ++s) {
                    const u64x2 v = ld_stream2(bm + s * ms + off);
                    m0[s] = v.x;
                    m1[s] = v.y;
                }
                const u64x2 ci = ld_stream2(bcin + off);
                const u64x2 la = ld_stream2(blast + off);
                u64x2 ax;
                if constexpr (FORM == HQ_FORM_TERM_MASK) {
                    const uint32_t mm = __builtin_nontemporal_load(
                        reinterpret_cast<const uint32_t *>(bmask + off));
                    ax = (u64x2){mm & 0xFFFFu, mm >> 16};
                } else {
                    ax = ld_stream2(baux + off);
                }
                int n0 = N, n1 = N;
                if constexpr (PERN) {
                    const uint16_t nn = *reinterpret_cast<const uint16_t *>(a.nv + g0);
                    n0 = nn & 0xFF;
                    n1 = nn >> 8;
                }
                uint64_t co0, co1;
                decide<N, FORM, PERN>(a, g0, m0, n0, ci.x, la.x, ax.x, co0, chg[0], fb[0]);
                decide<N, FORM, PERN>(a, g0 + 1, m1, n1, ci.y, la.y, ax.y, co1, chg[1], fb[1]);
                st_stream2(a.cout + g0, (u64x2){co0, co1});
            };
            // one group (the other of the lane's pair is outside the batch)
            auto single = [&](int j) {
                uint64_t m0[N];
#pragma unroll
                for (int s = 0; s < N; ++s) m0[s] = bm[s * ms + off + j];
                const int n0 = PERN ? (int)a.nv[g0 + j] : N;
                const uint64_t ax = FORM == HQ_FORM_TERM_MASK ? (uint64_t)bmask[off + j]
                                                              : baux[off + j];
                uint64_t co;
                decide<N, FORM, PERN>(a, g0 + j, m0, n0, bcin[off + j], blast[off + j], ax, co,
                                      chg[j], fb[j]);
                a.cout[g0 + j] = co;
            };
            if (g0 + 1 < a.G) pair();
            else if (g0 < a.G) single(0);
            // the wave's 128 groups are two bitmap words: lane k < 2 writes word k (lane i's
            // groups are bits 2i, 2i+1: the two ballots interleaved)
            const uint64_t b0 = __ballot(chg[0]), b1 = __ballot(chg[1]);
            const uint64_t f0 = __ballot(fb[0]), f1 = __ballot(fb[1]);
            const uint64_t w = (wbase >> 6) + lane;
            if (lane < 2 && w < ((a.G + 63) >> 6)) {
                const int sh = 32 * lane;
                if (a.changed)
                    a.changed[w] = spread32((uint32_t)(b0 >> sh)) |
                                   (spread32((uint32_t)(b1 >> sh)) << 1);
                if (a.fallback)
                    a.fallback[w] = spread32((uint32_t)(f0 >> sh)) |
                                    (spread32((uint32_t)(f1 >> sh)) << 1);
            }
        } else {
            auto one = [&]() {
                uint64_t m0[N];
#pragma unroll
                for (int s = 0; s < N; ++s) m0[s] = bm[s * ms + off];
                const int n0 = PERN ? (int)a.nv[g0] : N;
                uint64_t co;
                decide<N, FORM, PERN>(a, g0, m0, n0, bcin[off], blast[off], aux1(), co, chg[0],
                                      fb[0]);
                a.cout[g0] = co;
            };
            if (g0 < a.G) one();
            const uint64_t b0 = __ballot(chg[0]);
            const uint64_t f0 = __ballot(fb[0]);
            if (lane == 0) {
                if (a.changed) a.changed[wbase >> 6] = b0;
                if (a.fallback) a.fallback[wbase >> 6] = f0;
            }
        }
    }
}

// HQ_LAYOUT_TILES: one wave per 128-group tile. Row position 2i holds group i of the tile and
// position 2i + 1 group i + 64, so lane i's 16-byte load of a row brings groups i and i + 64:
// every field of the wave is ONE contiguous block of (n + 3) KiB, and the two ballots are the
// tile's two bitmap words as they are (no bit interleave). The full-tile test is scalar (the
// wave index is read into an SGPR), so full tiles carry no per-lane guard.
// TILED = 3: HQ_LAYOUT_TILES_LEADER | HQ_LAYOUT_IN_PLACE, the device-resident table decided in
// place (committed' written into the tile's committed row)
template <int N, int FORM, int VEC, bool PERN, int BLK, int TILED = 0>
__device__ __forceinline__ void commit_blocks(const CommitK &a, uint64_t blk, uint64_t nblk) {
    static_assert(!TILED || VEC == 2, "tiles are read two groups per lane");
    if constexpr (TILED) tile_blocks<N, FORM, PERN, BLK, TILED >= 2 ? 1 : 0, TILED == 3>(a, blk, nblk);
    else column_blocks<N, FORM, VEC, PERN, BLK>(a, blk, nblk);
}

template <int N, int FORM, int VEC, bool PERN, int TILED>
__global__ __launch_bounds__(kCommitBlock) void k_commit(const CommitK a) {
    commit_blocks<N, FORM, VEC, PERN, kCommitBlock, TILED>(a, blockIdx.x, gridDim.x);
}
// the 1024-thread twin: two blocks per CU need occupancy 8 (<= 64 VGPRs), so it is asked for
template <int N, int FORM, int VEC, bool PERN, int TILED>
__global__ __launch_bounds__(kCommitBlockBig, 8) void k_commit_big(const CommitK a) {
    commit_blocks<N, FORM, VEC, PERN, kCommitBlockBig, TILED>(a, blockIdx.x, gridDim.x);
}

template <int N, int FORM, int VEC, bool PERN, int TILED = 0>
int launch_commit_t(hq_ctx *ctx, const CommitK &k) {
    constexpr int B = commit_blk<N, FORM, PERN>();
    const unsigned grid = grid_for_commit(ctx, (k.G + VEC - 1) / VEC, B);
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    if constexpr (B == kCommitBlock)
        hipLaunchKernelGGL((k_commit<N, FORM, VEC, PERN, TILED>), dim3(grid), dim3(B), 0,
                           ctx->stream, k);
    else
        hipLaunchKernelGGL((k_commit_big<N, FORM, VEC, PERN, TILED>), dim3(grid), dim3(B), 0,
                           ctx->stream, k);
    return hq::post_launch(ctx, "k_commit");
}

inline int validate_commit(hq_ctx *ctx, const hq_commit_args *a) {
    if (!ctx) return HQ_E_INVAL;
    if (!a) return hq::fail(ctx, HQ_E_INVAL, "hq_commit: args is NULL");
    if (a->n_max < 1 || a->n_max > HQ_MAX_VOTERS)
        return hq::fail(ctx, HQ_E_INVAL, "hq_commit: n_max must be 1..8");
    const bool in_place = a->layout == (HQ_LAYOUT_TILES_LEADER | HQ_LAYOUT_IN_PLACE);
    if (a->layout != HQ_LAYOUT_COLUMNS && a->layout != HQ_LAYOUT_TILES &&
        a->layout != HQ_LAYOUT_TILES_LEADER && !in_place)
        return hq::fail(ctx, HQ_E_INVAL, "hq_commit: unknown layout");
    if (in_place && a->form != HQ_FORM_TERM_START && a->form != HQ_FORM_TERM_MASK)
        return hq::fail(ctx, HQ_E_INVAL,
                        "hq_commit: an in-place table holds the term-start or term-mask form");
    if (a->G == 0) return HQ_OK;
    const bool tiles = a->layout != HQ_LAYOUT_COLUMNS;
    if (tiles) {
        if (!a->match || (!a->committed_out && !in_place))
            return hq::fail(ctx, HQ_E_INVAL, "hq_commit: NULL tiles (match) / committed_out");
        if (!hq::aligned16(a->match) || (!in_place && !hq::aligned16(a->committed_out)) ||
            (a->n_voting && (reinterpret_cast<uintptr_t>(a->n_voting) & 1)))
            return hq::fail(ctx, HQ_E_INVAL,
                            "hq_commit: tiles and committed_out must be 16-byte aligned, "
                            "n_voting 2-byte aligned");
    } else {
        if (!a->match || !a->committed_in || !a->committed_out || !a->last_index)
            return hq::fail(ctx, HQ_E_INVAL, "hq_commit: NULL match/committed/last_index");
        if (a->match_stride < a->G)
            return hq::fail(ctx, HQ_E_INVAL, "hq_commit: match_stride < G");
    }
    if (a->form == HQ_FORM_TERM_START) {
        if (!tiles && !a->term_start)
            return hq::fail(ctx, HQ_E_INVAL, "hq_commit: term_start is NULL");
    } else if (a->form == HQ_FORM_TERM_RING || a->form == HQ_FORM_TERM_RING32) {
        if ((!tiles && !a->term) || (a->form == HQ_FORM_TERM_RING ? !a->ring : !a->ring32))
            return hq::fail(ctx, HQ_E_INVAL, "hq_commit: term/ring NULL");
        if (a->ring_len < 1 || a->ring_len > 1024 || (a->ring_len & (a->ring_len - 1)))
            return hq::fail(ctx, HQ_E_INVAL, "hq_commit: ring_len must be a power of two <= 1024");
    } else if (a->form == HQ_FORM_TERM_MASK) {
        if (!tiles && !a->term_mask)
            return hq::fail(ctx, HQ_E_INVAL, "hq_commit: term_mask is NULL");
        if (a->ring_len < 1 || a->ring_len > 16 || (a->ring_len & (a->ring_len - 1)))
            return hq::fail(ctx, HQ_E_INVAL, "hq_commit: mask form needs ring_len <= 16 (power of two)");
    } else {
        return hq::fail(ctx, HQ_E_INVAL, "hq_commit: unknown form");
    }
    return HQ_OK;
}

inline CommitK commit_k(const hq_commit_args *a) {
    CommitK k{};
    const bool tiles = a->layout != HQ_LAYOUT_COLUMNS;
    k.G = a->G;
    k.stride = tiles ? hq_commit_tile_words_for(a->n_max, a->form, a->layout) : a->match_stride;
    k.R = a->ring_len;
    k.match = a->match;
    k.nv = a->n_voting;
    k.cin = a->committed_in;
    k.cout = a->committed_out;
    k.last = a->last_index;
    k.aux = a->form == HQ_FORM_TERM_START ? static_cast<const void *>(a->term_start)
          : a->form == HQ_FORM_TERM_MASK  ? static_cast<const void *>(a->term_mask)
                                          : static_cast<const void *>(a->term);
    k.ring = a->form == HQ_FORM_TERM_RING32 ? static_cast<const void *>(a->ring32)
                                            : static_cast<const void *>(a->ring);
    k.changed = a->changed;
    k.fallback = a->fallback;
    return k;
}

// every column of the batch can be read two groups per lane with 16-byte loads
inline bool commit_vec2(const hq_commit_args *a) {
    if (a->layout != HQ_LAYOUT_COLUMNS) return true;   // alignment checked by validate_commit
    const bool aux_ok = a->form == HQ_FORM_TERM_START ? hq::aligned16(a->term_start)
                      : a->form == HQ_FORM_TERM_MASK
                          ? (reinterpret_cast<uintptr_t>(a->term_mask) & 3) == 0
                          : hq::aligned16(a->term);
    return hq::aligned16(a->match) && (a->match_stride % 2 == 0) &&
           hq::aligned16(a->committed_in) && hq::aligned16(a->committed_out) &&
           hq::aligned16(a->last_index) && aux_ok &&
           (!a->n_voting || (reinterpret_cast<uintptr_t>(a->n_voting) & 1) == 0);
}

}  // namespace
