// hq_dstep_layout.hip — around the device step's two passes (hq_dstep_step.hip): where a step's
// lists go in the host output region, from the scan of pass A's per-wave sums, and ahead of pass A
// the scan of a sized stream's sizes into the groups' prefixes. Both hipcub scans are here:
// <hipcub/hipcub.hpp> and its rocprim instances are compiled by this file alone.
#include <hipcub/hipcub.hpp>

#include "hq_dstep_k.h"

namespace {

struct PackSize {                 // group i's size word -> events << 32 | bytes; i = n: 0 (the
    const uint32_t *sizes;        // scan's last element is the totals; no memset on the copy
    uint64_t n;                   // stream between the sizes' copy and the bytes')
    const uint16_t *sizes16 = nullptr;   // 2-byte words: bytes only
    __host__ __device__ uint64_t operator()(uint64_t i) const {
        if (sizes16) return i < n ? sizes16[i] : 0;
        const uint32_t s = i < n ? sizes[i] : 0;
        return (uint64_t)(s & 0xFFFFu) << 32 | (s >> 16);
    }
};

// the lists' place in the host output region (of cap bytes) from the scanned per-wave sums, and
// the input errors of pass A (reset for the next step)
// bnd[l] = the scan at l * nw (list l's first record), l = 0 .. kLists; want_events: the step's
// event total when pass A counted the events (2-byte size words), else ~0
__device__ void layout_from(const uint32_t *bnd, uint64_t n, uint32_t *error, uint64_t cap,
                            uint32_t allow_column, uint64_t want_events, Layout *lay,
                            Layout *host_lay) {
    uint32_t *wide = error + 1;   // pass A: an advance of 2^32 or more
    uint32_t *ready_wide = error + 2;   // pass A: a ReadyToRead delta beyond 32 bits
    if (want_events != ~uint64_t(0) && (uint64_t)(bnd[kEvents + 1] - bnd[kEvents]) != want_events)
        *error |= kErrBoffsets;   // (the events decoded are not the totals the caller gave)
    lay->ready_compact = (allow_column & kReadyCompact) && !*ready_wide;
    const uint64_t rec[kLists] = {sizeof(hq_commit_event),
                                  lay->ready_compact ? sizeof(hq_ready_compact) : sizeof(hq_ready_to_read),
                                  sizeof(hq_read_index_resp), sizeof(hq_state_change),
                                  sizeof(hq_dropped_read), 8, 8, 0, 0, 0, 0};
    const uint32_t commits = bnd[1] - bnd[0];
    // the commits as a column when that moves fewer bytes (16 per commit in the list against 8
    // per listed group, or 4 when every advance fits)
    // (allow_column: bit kColumn64 HQ_WORKER_COMMIT_COLUMN, bit kColumn32 _ADVANCE)
    lay->commit_column = (allow_column & kColumn32) && !*wide && 4 * (uint64_t)commits > n
                             ? kColumn32
                         : (allow_column & kColumn64) && 2 * (uint64_t)commits > n ? kColumn64 : 0;
    // the slot form: the column and the slots pass A wrote come first, the lists after them
    const bool slots = (allow_column & kReadySlots) != 0;
    const uint64_t reserve = slots ? slot_layout(n, nullptr, nullptr) : 0;
    uint64_t total = reserve;
    for (int l = 0; l < kLists; ++l) {
        const uint32_t len = bnd[l + 1] - bnd[l];
        lay->len[l] = len;
        if (l == kCommits && slots && lay->commit_column == kColumn32) {
            lay->off[l] = 0;      // (where pass A wrote the advance words)
            continue;
        }
        lay->off[l] = total;
        const uint64_t bytes = l == kCommits && lay->commit_column
                                   ? n * (lay->commit_column == kColumn32 ? 4 : 8)
                                   : len * rec[l];
        total += (bytes + 255) & ~uint64_t(255);
    }
    lay->total = total;
    lay->reserve = reserve;
    lay->error = *error;
    lay->overflow = total > cap;
    // pass A's flags are reset for the next step, except when the host will run this layout again
    // for the same step and the re-run must see the same flags (or it could choose the 4-byte
    // advance column for a 2^32 advance): an overflow without an input error (the region grows),
    // or kErrScan alone (the copy-out runs again without pass A's records; the host clears it)
    if (!((lay->overflow && !*error) || *error == kErrScan)) {
        *error = 0;
        *wide = 0;
        *ready_wide = 0;
    }
    *host_lay = *lay;             // the host's copy, written into pinned memory (no copy launch)
}

__global__ void k_layout(const uint32_t *scan, uint64_t n, uint64_t nw, uint32_t *error,
                         uint64_t cap, uint32_t allow_column, uint64_t want_events, Layout *lay,
                         Layout *host_lay) {
    if (threadIdx.x != 0) return;
    uint32_t bnd[kLists + 1];
    for (int l = 0; l <= kLists; ++l) bnd[l] = scan[(uint64_t)l * nw];
    layout_from(bnd, n, error, cap, allow_column, want_events, lay, host_lay);
}

// A small step's scan of the per-wave sums and its layout in one workgroup (hipcub's scan is two
// launches, then k_layout a third: 16 workers pay 48 such launches per step): tiles of 11 Ki sums,
// each thread scanning 11 consecutive ones from LDS (an odd stride: no bank conflicts), the
// threads' totals scanned across the waves, with the carry of the tiles before
__device__ __forceinline__ void scan_layout(const uint32_t *wsum, uint32_t *scan, uint64_t ws,
                                            uint64_t n, uint64_t nw, uint32_t *error, uint64_t cap,
                                            uint32_t allow_column, uint64_t want_events, Layout *lay,
                                            Layout *host_lay) {
    __shared__ uint32_t tile[kScanT * kScanE];
    __shared__ uint32_t wtot[kScanT / 64];
    __shared__ uint32_t bnd[kLists + 1];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    uint32_t carry = 0;
    for (uint64_t base = 0; base < ws; base += (uint64_t)kScanT * kScanE) {
        for (int k = 0; k < kScanE; ++k) {
            const uint64_t j = base + (uint64_t)k * kScanT + t;
            tile[k * kScanT + t] = j < ws ? wsum[j] : 0u;
        }
        __syncthreads();
        uint32_t v[kScanE], sum = 0;
        for (int k = 0; k < kScanE; ++k) {
            v[k] = tile[t * kScanE + k];
            sum += v[k];
        }
        uint32_t x = sum;         // inclusive scan of the threads' totals over the wave
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d, 64);
            x += lane >= d ? y : 0u;
        }
        if (lane == 63) wtot[wv] = x;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int w = 0; w < kScanT / 64; ++w) {
            const uint32_t z = wtot[w];
            before += w < wv ? z : 0u;
            all += z;
        }
        uint32_t run = carry + before + x - sum;
        for (int k = 0; k < kScanE; ++k) {
            tile[t * kScanE + k] = run;
            run += v[k];
        }
        __syncthreads();
        for (int k = 0; k < kScanE; ++k) {
            const uint64_t j = base + (uint64_t)k * kScanT + t;
            if (j < ws) {
                const uint32_t e = tile[k * kScanT + t];
                scan[j] = e;
                if (j % nw == 0 && j / nw <= kLists) bnd[j / nw] = e;
            }
        }
        carry += all;
        __syncthreads();          // (the next tile overwrites tile and wtot)
    }
    if (t == 0) layout_from(bnd, n, error, cap, allow_column, want_events, lay, host_lay);
}

__global__ __launch_bounds__(kScanT) void k_scan_layout(const uint32_t *wsum, uint32_t *scan,
                                                        uint64_t ws, uint64_t n, uint64_t nw,
                                                        uint32_t *error, uint64_t cap,
                                                        uint32_t allow_column, uint64_t want_events,
                                                        Layout *lay, Layout *host_lay) {
    scan_layout(wsum, scan, ws, n, nw, error, cap, allow_column, want_events, lay, host_lay);
}

__host__ __device__ inline uint64_t want_events_of(const StepK &a) {
    return a.bytes_only ? a.n_events : ~uint64_t(0);
}

// the jobs path: one workgroup per job (grid = the jobs)
__global__ __launch_bounds__(kScanT) void k_scan_layout_jobs(const StepK *ks) {
    const StepK &a = ks[blockIdx.x];
    scan_layout(a.wsum, const_cast<uint32_t *>(a.scan), a.ws, a.n, a.nw, a.error, a.out_cap,
                a.allow_column, want_events_of(a), const_cast<Layout *>(a.layout), a.host_layout);
}

// The jobs path's scan of a sized stream's sizes (the single path: hipcub over PackSize), in
// two launches for all jobs: each 1024 groups' packed total (k_size_sums), then each 1024 groups
// scanned in a workgroup from the sum of the totals before it (k_size_apply); prefix[i] = events
// before group i << 32 | bytes before it, prefix[n] the totals (n + 1 elements, as the single
// path's scan)
__device__ __forceinline__ uint64_t packed_size(const StepK &a, uint64_t i) {
    if (i >= a.n) return 0;
    if (a.bytes_only) return a.sizes16[i];
    const uint32_t s = a.sizes[i];
    return (uint64_t)(s & 0xFFFFu) << 32 | (s >> 16);
}

__device__ __forceinline__ uint64_t block_excl_scan(uint64_t v, uint64_t *total) {
    __shared__ uint64_t wt[1024 / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint64_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(x, d, 64);
        x += lane >= d ? y : 0ull;
    }
    if (lane == 63) wt[wv] = x;
    __syncthreads();
    uint64_t before = 0, all = 0;
    for (int w = 0; w < (int)(blockDim.x / 64); ++w) {
        before += w < wv ? wt[w] : 0ull;
        all += wt[w];
    }
    __syncthreads();              // (wt is reused by the next call)
    *total = all;
    return before + x - v;
}

__global__ __launch_bounds__(256) void k_size_sums(const JobMap m) {
    if (m.table_out && blockIdx.x == 0) {   // the table for the launches behind this one
        const uint64_t *src = reinterpret_cast<const uint64_t *>(m.ks + m.job0);
        uint64_t *dst = reinterpret_cast<uint64_t *>(m.table_out + m.job0);
        for (uint32_t q = threadIdx.x; q < m.count * (uint32_t)(sizeof(StepK) / 8); q += 256)
            dst[q] = src[q];
    }
    const uint32_t j = job_of(m, blockIdx.x);
    const StepK &a = m.ks[m.job0 + j];
    const uint64_t b = blockIdx.x - m.blk0[j], i0 = b * kSizeTile + threadIdx.x * 4;
    uint64_t v = 0;
    if (a.bytes_only && a.sizes16_src) {
        // 2-byte words straight from pinned host memory (one 8-byte load of a thread's 4 where
        // aligned and whole), kept on device for k_size_apply
        uint16_t *dst = const_cast<uint16_t *>(a.sizes16);
        uint16_t z[4];
        if (i0 + 4 <= a.n && !(reinterpret_cast<uintptr_t>(a.sizes16_src) & 7)) {
            const uint64_t w = *reinterpret_cast<const uint64_t *>(a.sizes16_src + i0);
#pragma unroll
            for (int k = 0; k < 4; ++k) z[k] = (uint16_t)(w >> (16 * k));
            *reinterpret_cast<uint64_t *>(dst + i0) = w;   // (dst: a 256-byte aligned region)
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint64_t i = i0 + k;
                z[k] = i < a.n ? a.sizes16_src[i] : 0;
                if (i < a.n) dst[i] = z[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) v += z[k];
    } else if (!a.bytes_only && a.sizes_src) {   // the sizes straight from pinned host memory
        uint32_t *dst = const_cast<uint32_t *>(a.sizes);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t i = i0 + k;
            const uint32_t z = i < a.n ? a.sizes_src[i] : 0;
            if (i < a.n) dst[i] = z;
            v += (uint64_t)(z & 0xFFFFu) << 32 | (z >> 16);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v += packed_size(a, i0 + k);
    }
    uint64_t tot;
    (void)block_excl_scan(v, &tot);
    if (threadIdx.x == 0) a.bsum[b] = tot;
}

// the size tiles' totals of every job scanned in place (exclusive), one workgroup per job: the
// large steps' form (k_size_apply then reads its tile's prefix)
__global__ __launch_bounds__(1024) void k_bsum_scan_jobs(const JobMap m) {
    const StepK &a = m.ks[m.job0 + blockIdx.x];
    const uint64_t nb = (a.n + 1 + kSizeTile - 1) / kSizeTile;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < nb; base += 1024) {
        const uint64_t k = base + threadIdx.x;
        const uint64_t v = k < nb ? a.bsum[k] : 0;
        uint64_t tot;
        const uint64_t ex = block_excl_scan(v, &tot);
        if (k < nb) a.bsum[k] = carry + ex;
        carry += tot;
    }
}

// (a small job's workgroups each sum the totals of the tiles before their own: at most a few
// thousand words from L2, in place of a scan launch between the two passes)
__global__ __launch_bounds__(256) void k_size_apply(const JobMap m) {
    const uint32_t j = job_of(m, blockIdx.x);
    const StepK &a = m.ks[m.job0 + j];
    const uint64_t b = blockIdx.x - m.blk0[j], i0 = b * kSizeTile + threadIdx.x * 4;
    uint64_t base;
    if (m.bsum_scanned) {
        base = a.bsum[b];
    } else {
        uint64_t before = 0;
        for (uint64_t k = threadIdx.x; k < b; k += 256) before += a.bsum[k];
        (void)block_excl_scan(before, &base);
    }
    uint64_t v[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = packed_size(a, i0 + k);
        sum += v[k];
    }
    uint64_t tot;
    uint64_t run = base + block_excl_scan(sum, &tot);
    uint64_t *prefix = const_cast<uint64_t *>(a.prefix);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (i0 + k <= a.n) prefix[i0 + k] = run;
        run += v[k];
    }
}

}  // namespace

namespace hq {

int launch_layout(hq_ctx *ctx, hipStream_t s, const StepArgs &ka) {
    const StepK &k = static_cast<const StepK &>(ka);
    return launch(ctx, s, "k_layout", k_layout, 1, 64, k.scan, k.n, k.nw, k.error, k.out_cap,
                  k.allow_column, want_events_of(k), const_cast<Layout *>(k.layout), k.host_layout);
}
int launch_scan_layout(hq_ctx *ctx, hipStream_t s, const StepArgs &ka) {
    const StepK &k = static_cast<const StepK &>(ka);
    return launch(ctx, s, "k_scan_layout", k_scan_layout, 1, kScanT, k.wsum,
                  const_cast<uint32_t *>(k.scan), k.ws, k.n, k.nw, k.error, k.out_cap,
                  k.allow_column, want_events_of(k), const_cast<Layout *>(k.layout), k.host_layout);
}
int launch_scan_layout_jobs(hq_ctx *ctx, hipStream_t s, const JobArgs &ma) {
    const JobMap &m = static_cast<const JobMap &>(ma);   // (one workgroup per job of the table)
    return launch(ctx, s, "k_scan_layout_jobs", k_scan_layout_jobs, m.count, kScanT, m.ks);
}
int launch_size_sums(hq_ctx *ctx, hipStream_t s, const JobArgs &ma) {
    const JobMap &m = static_cast<const JobMap &>(ma);
    return launch(ctx, s, "k_size_sums", k_size_sums, m.blk0[m.count], 256, m);
}
int launch_bsum_scan_jobs(hq_ctx *ctx, hipStream_t s, const JobArgs &ma) {
    const JobMap &m = static_cast<const JobMap &>(ma);
    return launch(ctx, s, "k_bsum_scan_jobs", k_bsum_scan_jobs, m.count, 1024, m);
}
int launch_size_apply(hq_ctx *ctx, hipStream_t s, const JobArgs &ma) {
    const JobMap &m = static_cast<const JobMap &>(ma);
    return launch(ctx, s, "k_size_apply", k_size_apply, m.blk0[m.count], 256, m);
}

int scan_wave_sums(hq_ctx *ctx, hipStream_t s, void *tmp, size_t *tmp_bytes, uint32_t *wsum,
                   uint32_t *scan, size_t ws) {
    return check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, *tmp_bytes, wsum, scan, ws, s),
                     tmp ? "hipcub scan" : "hipcub scan size");
}
int scan_sizes(hq_ctx *ctx, hipStream_t s, void *tmp, size_t *tmp_bytes, const void *sizes,
               bool s16, uint64_t n, uint64_t *prefix) {
    const hipcub::TransformInputIterator<uint64_t, PackSize, hipcub::CountingInputIterator<uint64_t>>
        packed_sizes(hipcub::CountingInputIterator<uint64_t>(0),
                     PackSize{static_cast<const uint32_t *>(sizes), n,
                              s16 ? static_cast<const uint16_t *>(sizes) : nullptr});
    return check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, *tmp_bytes, packed_sizes, prefix,
                                                           n + 1, s),
                     tmp ? "hipcub scan" : "hipcub scan size");
}

}  // namespace hq
