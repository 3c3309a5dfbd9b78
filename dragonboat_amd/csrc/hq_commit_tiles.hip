// hq_commit_tiles.hip — the commit kernels over 128-group tiles (k_commit / k_commit_big with
// TILED = 1, 2, 3: tiles, tiles without the leader's row, the same decided in place), the fused
// launch of several batches (k_commit_fused, columns or tiles), the column -> tile packer, and
// hq_commit_fused_dev / hq_tile_commit*_dev.
//
// A wave decides one tile: its loads walk one contiguous block of (n + 3) KiB, 16 bytes per lane
// and row, every row load issued before the first compare; the decision is the min/max network of
// hq_commit_body.h in registers and the two ballots are the tile's two bitmap words. No LDS and
// no MFMA: nothing is reused or a contraction (DESIGN.md "Kernels").
#include "hq_commit.h"

namespace {

// LEAD = 1: rows start at slot 1 (row s - 1 holds slot s) and m[0] = last_index, so the wave's
// block is (n + 2) KiB: 8 bytes less per group.
template <int N, int FORM, bool PERN, int BLK, int LEAD, bool INPLACE>
__device__ __forceinline__ void tile_blocks(const CommitK &a, uint64_t blk, uint64_t nblk) {
    constexpr uint64_t T = HQ_TILE_GROUPS;
    const uint64_t lane = threadIdx.x & 63;
    const uint64_t wave = blk * (BLK / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t step = nblk * BLK * 2;
    for (uint64_t wbase = wave * T; wbase < a.G; wbase += step)
        commit_tile<N, FORM, PERN, LEAD, INPLACE>(a, wbase, lane);
}

// Several uniform-n batches of one step in ONE launch (a step worker's voter-count buckets):
// batch i owns workgroups [first[i], first[i+1]); the batch index and its n are uniform per
// workgroup, so the switch costs no divergence. Saves the dependent-launch boundary and the
// grid fill / drain between buckets (MI355X_MICROARCH.md "boundary": 1.7-1.9 us each).
// commit batches per fused launch: a step worker's voter-count buckets, or the independent
// batches of several steps / step workers posted together (32 x 1M-group batches in one launch:
// no boundary, fill or drain between them; 3.3 KB of kernel arguments)
constexpr int kMaxFusedCommit = 32;
struct FusedK {
    CommitK b[kMaxFusedCommit];
    uint32_t first[kMaxFusedCommit + 1];
    uint32_t n[kMaxFusedCommit];   // dwords: a scalar load (a byte array is read with a vector load + wait)
    uint32_t count;
};

template <int FORM, int BLK, int TILED>
__global__ __launch_bounds__(BLK, BLK > kCommitBlock ? 8 : 1) void k_commit_fused(const FusedK f) {
    const uint32_t blk = blockIdx.x;
    uint32_t i = 0;
#pragma unroll
    for (int k = 1; k < kMaxFusedCommit; ++k) i += (k < (int)f.count && blk >= f.first[k]) ? 1u : 0u;
    const uint64_t b = blk - f.first[i], nb = f.first[i + 1] - f.first[i];
    switch (f.n[i]) {
    case 1: commit_blocks<1, FORM, 2, false, BLK, TILED>(f.b[i], b, nb); break;
    case 2: commit_blocks<2, FORM, 2, false, BLK, TILED>(f.b[i], b, nb); break;
    case 3: commit_blocks<3, FORM, 2, false, BLK, TILED>(f.b[i], b, nb); break;
    case 4: commit_blocks<4, FORM, 2, false, BLK, TILED>(f.b[i], b, nb); break;
    case 5: commit_blocks<5, FORM, 2, false, BLK, TILED>(f.b[i], b, nb); break;
    case 6: commit_blocks<6, FORM, 2, false, BLK, TILED>(f.b[i], b, nb); break;
    case 7: commit_blocks<7, FORM, 2, false, BLK, TILED>(f.b[i], b, nb); break;
    default: commit_blocks<8, FORM, 2, false, BLK, TILED>(f.b[i], b, nb); break;
    }
}

// every field of a column batch (generator, tile packer)
CommitCols commit_cols(const hq_commit_args *a) {
    CommitCols k{};
    k.G = a->G;
    k.stride = a->match_stride;
    k.nwords = hq::words64(a->G);
    k.n_max = a->n_max;
    k.R = a->ring_len;
    k.match = a->match;
    k.nv = a->n_voting;
    k.cin = a->committed_in;
    k.cout = a->committed_out;
    k.last = a->last_index;
    k.tstart = a->term_start;
    k.term = a->term;
    k.ring = a->ring;
    k.changed = a->changed;
    k.fallback = a->fallback;
    k.mask = a->term_mask;
    k.ring32 = a->ring32;
    k.tile_words = hq_commit_tile_words(a->n_max, a->form);
    return k;
}

// the fused launch runs the big block only where every batch's body fits it
constexpr uint32_t kFusedBigNmax = 5;

}  // namespace

int hq::launch_commit_tiles(hq_ctx *ctx, const hq_commit_args *a) {
    const CommitK k = commit_k(a);
    // 1 HQ_LAYOUT_TILES, 2 HQ_LAYOUT_TILES_LEADER, 3 the leader tiles in place
    const int tiled = a->layout == (HQ_LAYOUT_TILES_LEADER | HQ_LAYOUT_IN_PLACE) ? 3
                    : a->layout == HQ_LAYOUT_TILES_LEADER                       ? 2
                                                                                : 1;
    // tiles are always read two groups per lane (the validation requires a 16-byte aligned base)
    return dispatch_n(a->n_max, [&](auto n) {
        return dispatch<HQ_FORM_TERM_START, HQ_FORM_TERM_MASK, HQ_FORM_TERM_RING32,
                        HQ_FORM_TERM_RING>(a->form, [&](auto form) {
            return dispatch_bool(a->n_voting != nullptr, [&](auto pern) {
                return dispatch<3, 2, 1>(tiled, [&](auto t) {
                    return launch_commit_t<decltype(n)::value, decltype(form)::value, 2,
                                           decltype(pern)::value, decltype(t)::value>(ctx, k);
                });
            });
        });
    });
}

extern "C" int hq_commit_fused_dev(hq_ctx *ctx, const hq_commit_args *args, uint32_t count) {
    if (!ctx) return HQ_E_INVAL;
    if (count && !args) return hq::fail(ctx, HQ_E_INVAL, "hq_commit_fused_dev: args is NULL");
    for (uint32_t i = 0; i < count; ++i) {
        int rc = validate_commit(ctx, args + i);
        if (rc) return rc;
    }
    // batches that can share the launch: uniform n, 16-byte aligned columns, one form
    bool fusable = count >= 2 && count <= (uint32_t)kMaxFusedCommit;
    for (uint32_t i = 0; fusable && i < count; ++i)
        fusable = args[i].G > 0 && !args[i].n_voting && commit_vec2(args + i) &&
                  args[i].form == args[0].form && args[i].layout == args[0].layout &&
                  !(args[i].layout & HQ_LAYOUT_IN_PLACE);
    if (!fusable) return hq_commit_many_dev(ctx, args, count);
    FusedK f{};
    f.count = count;
    // one block size for the launch: the big one only if every batch's kernel body fits it
    bool big = true;
    // (the fused kernel's bodies fit 64 VGPRs without spilling for these two forms only)
    for (uint32_t i = 0; i < count; ++i)
        big &= args[i].n_max <= kFusedBigNmax &&
               (args[i].form == HQ_FORM_TERM_START || args[i].form == HQ_FORM_TERM_MASK);
    const int B = big ? kCommitBlockBig : kCommitBlock;
    uint64_t blocks = 0;
    // workgroup ranges in launch order, the widest batches first (their waves are dispatched
    // first, so the tail is made of the light ones: c5t 96-97 -> 93-94 us,
    // profiles/r01f/ab_heavy_first.log)
    uint32_t order[kMaxFusedCommit];
    for (uint32_t i = 0; i < count; ++i) order[i] = i;
    for (uint32_t i = 1; i < count; ++i)
        for (uint32_t j = i; j > 0 && args[order[j]].n_max > args[order[j - 1]].n_max; --j) {
            const uint32_t t = order[j];
            order[j] = order[j - 1];
            order[j - 1] = t;
        }
    for (uint32_t k = 0; k < count; ++k) {
        const uint32_t i = k;
        f.b[i] = commit_k(args + order[k]);
        f.n[i] = args[order[k]].n_max;
        f.first[i] = (uint32_t)blocks;
        // the same lanes per batch as its own launch would get (grid-stride beyond that)
        blocks += grid_for_commit(ctx, (args[order[k]].G + 1) / 2, B);
    }
    for (uint32_t i = count; i <= (uint32_t)kMaxFusedCommit; ++i) f.first[i] = (uint32_t)blocks;
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    // TILED as in k_commit: 2 HQ_LAYOUT_TILES_LEADER, 1 HQ_LAYOUT_TILES, 0 columns
    const int tiled = args[0].layout == HQ_LAYOUT_TILES_LEADER ? 2
                    : args[0].layout == HQ_LAYOUT_TILES        ? 1
                                                               : 0;
    dispatch<HQ_FORM_TERM_START, HQ_FORM_TERM_MASK, HQ_FORM_TERM_RING32, HQ_FORM_TERM_RING>(
        args[0].form, [&](auto form) {
            dispatch<2, 1, 0>(tiled, [&](auto t) {
                constexpr int F = decltype(form)::value, T = decltype(t)::value;
                // the ring forms have no big-block instance (`big` is false for them)
                if constexpr (F == HQ_FORM_TERM_START || F == HQ_FORM_TERM_MASK) {
                    if (big) {
                        hipLaunchKernelGGL((k_commit_fused<F, kCommitBlockBig, T>), dim3(blocks),
                                           dim3(kCommitBlockBig), 0, ctx->stream, f);
                        return;
                    }
                }
                hipLaunchKernelGGL((k_commit_fused<F, kCommitBlock, T>), dim3(blocks),
                                   dim3(kCommitBlock), 0, ctx->stream, f);
            });
        });
    return hq::post_launch(ctx, "k_commit_fused");
}

// Columns -> HQ_LAYOUT_TILES(_LEADER) tiles, one thread per tile word (include/hipquorum.h).
// Builds tiled inputs from column batches on the device (benchmark inputs, device-side packers).
// lead = 1 drops slot 0's row: tile row r < n holds match slot r + 1.
__global__ __launch_bounds__(kBlock) void k_tile_commit(const CommitCols c, uint64_t *tiles,
                                                        uint64_t ntiles, uint32_t n, int form,
                                                        int lead) {
    const uint64_t tw = c.tile_words, total = ntiles * tw;
    for (uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x; w < total;
         w += (uint64_t)gridDim.x * kBlock) {
        const uint64_t t = w / tw, r = w % tw, row = r / HQ_TILE_GROUPS;
        uint64_t v = 0;
        // row position p holds group (p >> 1) + 64 * (p & 1) of the tile (include/hipquorum.h)
        auto group = [&](uint64_t p) { return t * HQ_TILE_GROUPS + (p >> 1) + (HQ_TILE_GROUPS / 2) * (p & 1); };
        if (form == HQ_FORM_TERM_MASK && row >= n + 2) {   // 4 u16 masks per word
            const uint64_t p0 = 4 * (r - (uint64_t)(n + 2) * HQ_TILE_GROUPS);
            for (int k = 3; k >= 0; --k) {
                const uint64_t g = group(p0 + k);
                v = (v << 16) | (g < c.G ? c.mask[g] : 0);
            }
        } else {
            const uint64_t g = group(r % HQ_TILE_GROUPS);
            if (g < c.G) {
                v = row < n       ? c.match[(row + lead) * c.stride + g]
                  : row == n      ? c.cin[g]
                  : row == n + 1  ? c.last[g]
                  : form == HQ_FORM_TERM_START ? c.tstart[g] : c.term[g];
            }
        }
        tiles[w] = v;
    }
}

extern "C" int hq_tile_commit_dev(hq_ctx *ctx, const hq_commit_args *a, uint64_t *tiles) {
    return hq_tile_commit_as_dev(ctx, a, tiles, HQ_LAYOUT_TILES);
}

extern "C" int hq_tile_commit_as_dev(hq_ctx *ctx, const hq_commit_args *a, uint64_t *tiles,
                                     uint32_t layout) {
    if (!ctx) return HQ_E_INVAL;
    if (!a || !tiles) return hq::fail(ctx, HQ_E_INVAL, "hq_tile_commit: NULL argument");
    if (a->layout != HQ_LAYOUT_COLUMNS)
        return hq::fail(ctx, HQ_E_INVAL, "hq_tile_commit: input must be the column layout");
    if (layout != HQ_LAYOUT_TILES && layout != HQ_LAYOUT_TILES_LEADER)
        return hq::fail(ctx, HQ_E_INVAL, "hq_tile_commit: target must be a tile layout");
    hq_commit_args chk = *a;
    chk.committed_out = chk.committed_out ? chk.committed_out : tiles;  // not written here
    int rc = validate_commit(ctx, &chk);
    if (rc || a->G == 0) return rc;
    const int lead = layout == HQ_LAYOUT_TILES_LEADER ? 1 : 0;
    CommitCols k = commit_cols(a);
    k.tile_words = hq_commit_tile_words_for(a->n_max, a->form, layout);
    const uint64_t ntiles = hq_commit_tiles(a->G);
    rc = hq::pre_launch(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tile_commit, dim3(grid_for(ctx, ntiles * k.tile_words)), dim3(kBlock), 0,
                       ctx->stream, k, tiles, ntiles, a->n_max - lead, (int)a->form, lead);
    return hq::post_launch(ctx, "k_tile_commit");
}
