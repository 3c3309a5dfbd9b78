// hq_launch.h — what the kernel families' launchers share: the block sizes, the grid cap with
// its grid-stride sizing, the helper that picks a template instance from run-time values, and the
// 16-byte vector types with the two-groups-per-lane bit interleave.
#pragma once

#include <type_traits>
#include <utility>

#include "hq_internal.h"

namespace {

constexpr int kBlock = 256;           // 4 waves of 64
// The commit streams (u64 and lag) run 512-thread blocks: ~5 % shorter than 256 on the 1M x 3
// launch under rocprofv3 (11.7 vs 12.4 us, tools/kexp2.hip, git history); 4 groups per lane was
// slower.
constexpr int kCommitBlock = 512;
// Kernels that fit 64 VGPRs (occupancy 8) run 1024-thread blocks: 10.57 vs 11.1 us per 1M x 3
// launch (tools/kexp3.hip, git history: fewer workgroups to dispatch for the same waves); the
// others keep 512 so that two or more blocks still fit a CU.
constexpr int kCommitBlockBig = 1024;
// Grid cap in 256-thread units (64 per CU), grid-stride beyond. An 8M-group x 5 launch then runs
// one tile per wave: 92-94 vs 96-98 us with the earlier cap of 16 per CU, neutral at 1M groups
// (profiles/r01e/ab_maxblocks.log).
constexpr int kMaxBlocks = 256 * 64;

static_assert(hq::kDefaultMaxBlocks == kMaxBlocks, "hq_ctx::max_blocks starts at the grid cap");

// The cap is the context's (hq_ctx::max_blocks: kMaxBlocks unless HQ_MAX_BLOCKS lowered it at
// hq_open, so that a test's small batch makes several grid-stride passes).
inline unsigned grid_capped(uint64_t lanes_needed, int block, uint64_t max_blocks) {
    uint64_t b = (lanes_needed + block - 1) / block;
    if (b < 1) b = 1;
    if (b > max_blocks) b = max_blocks;
    return (unsigned)b;
}
inline unsigned grid_for(const hq_ctx *ctx, uint64_t lanes_needed, int block = kBlock) {
    return grid_capped(lanes_needed, block, ctx->max_blocks);
}
// the commit streams: the same threads under the cap whatever the block size B
inline unsigned grid_for_commit(const hq_ctx *ctx, uint64_t lanes_needed, int B) {
    return grid_capped(lanes_needed, B, (uint64_t)ctx->max_blocks * 256 / B);
}

// A run-time value from the fixed list Vs as a compile-time constant: calls f with the
// std::integral_constant of the entry equal to v; the last entry is the default. Nested calls
// pick a template instance, `if constexpr` in f keeps out the combinations that do not exist:
//     dispatch_n(n_max, [&](auto n) { launch<decltype(n)::value>(...); });
template <auto V, auto... Rest, class T, class F>
auto dispatch(T v, F &&f) {
    if constexpr (sizeof...(Rest) == 0) {
        return f(std::integral_constant<decltype(V), V>{});
    } else {
        if (v == static_cast<T>(V)) return f(std::integral_constant<decltype(V), V>{});
        return dispatch<Rest...>(v, std::forward<F>(f));
    }
}
template <class T, class F>
auto dispatch_n(T n, F &&f) {   // a voter / ctx count in 1..8
    return dispatch<1, 2, 3, 4, 5, 6, 7, 8>(n, std::forward<F>(f));
}
template <class F>
auto dispatch_bool(bool b, F &&f) {
    return dispatch<true, false>(b, std::forward<F>(f));
}

// 16-byte vector accesses, and the bit interleave of the kernels that own two groups per lane
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint64_t spread32(uint32_t x) {  // bit i -> bit 2i
    uint64_t v = x;
    v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
    v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
    v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    v = (v | (v << 1)) & 0x5555555555555555ull;
    return v;
}

}  // namespace
