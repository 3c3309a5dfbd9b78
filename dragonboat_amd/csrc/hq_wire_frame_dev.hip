// hq_wire_frame_dev.hip — hq_wire_frame_batch's work on the device (include/hipquorum.h "wire
// framing on the device"): MessageBatch bytes cut into segments, one wave walking each with
// hq_wire_codec.h's segment walker (the code the host runs under sanitizers), a chain over every
// batch's segment records that takes only the segments walked from their true entries, and a
// compaction of their spans into the dense list hq_wire_decode_dev / k_wire_decode take.
//
// Order comes from kernel boundaries and three scans (segments, messages and spans per batch):
// no kernel waits on another workgroup, none spins or looks back, and there is no atomic. The
// bytes are not trusted: every loop is bounded by a segment's or a batch's length, and nothing
// outside a batch is read.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "hq_internal.h"
#include "hq_wire_codec.h"
#include "hq_wire_dev.h"

namespace {

using hqw::kNoEntry;
using hqw::Segment;
using hqw::SegmentPlace;

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;   // a wave per segment
constexpr uint32_t kWindow = 4096;                           // bytes of a batch a wave keeps in LDS

struct FrameK {
    const uint8_t *bytes;
    uint64_t len;
    const hq_wire_batch_ref *batches;
    uint64_t n_batches;
    uint32_t S, region;                   // segment bytes; spans a segment's region holds
    uint64_t seg_cap;                     // segment records and regions there are
    uint64_t *nseg, *seg0;                // [n_batches + 1]: segments per batch, and their scan
    Segment *segs;                        // [seg_cap]
    SegmentPlace *place;                  // [seg_cap]
    hq_wire_span *regions;                // [seg_cap * region]
    uint64_t *cnt_msgs, *cnt_spans;       // [n_batches + 1]: of the batches in the dense list
    uint64_t *msg0, *span0;               //   and their scans
    uint32_t *dense;                      // [n_batches]: the batch's spans go to the dense list
    uint32_t *voids;                      // [n_batches] or NULL
    hq_wire_frame_result *results;
    hq_wire_span *spans;
    uint64_t span_cap;
    uint32_t *span_batch;
    uint64_t *totals;
    uint32_t check, bin_ver;              // check: only batches of this deployment and binary
    uint64_t deployment_id;               //   version go to the dense list (the wire's step)
};

__device__ __forceinline__ bool within(const hq_wire_batch_ref &r, uint64_t len) {
    return r.offset <= len && r.len <= len - r.offset;
}

__global__ void __launch_bounds__(256) k_wire_segments(const FrameK a) {
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b > a.n_batches) return;
    uint64_t n = 0;
    if (b < a.n_batches) {
        const hq_wire_batch_ref r = a.batches[b];
        if (within(r, a.len)) n = hqw::segment_count(a.S, r.len);
    }
    a.nseg[b] = n;
}

// the batch of segment s: the last b with seg0[b] <= s (s < seg0[n_batches]; a batch without
// segments shares its seg0 with the next)
__device__ __forceinline__ uint64_t batch_of(const uint64_t *seg0, uint64_t n_batches, uint64_t s) {
    uint64_t lo = 0, hi = n_batches;                  // seg0[lo] <= s < seg0[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (seg0[mid] <= s) lo = mid;
        else hi = mid;
    }
    return lo;
}

// this wave's LDS stores have landed and its lanes read them (waves do not wait for each other:
// each has its own segment and its own number of windows)
__device__ __forceinline__ void wave_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// n bytes at g into the wave's stage behind the low 4 bits of g (k_wire_decode's staging): the
// whole 16-byte words of memory inside [g, g + n) as such, the ragged edges byte by byte; nothing
// outside is read. Returns where the first byte lies.
__device__ __forceinline__ const uint8_t *stage(uint4 *words, const uint8_t *g, uint32_t n,
                                                uint32_t lane) {
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(g) & 15u);
    uint8_t *const sb = reinterpret_cast<uint8_t *>(words);
    const uint4 *const g16 = reinterpret_cast<const uint4 *>(g - sh);
    const uint32_t n_words = (sh + n + 15) / 16;      // (n <= kWindow: at most kWindow / 16 + 1)
    for (uint32_t c = lane; c < n_words; c += 64) {
        const uint32_t b0 = c * 16;
        if (b0 >= sh && b0 + 16 <= sh + n) {
            words[c] = g16[c];
        } else {
            for (uint32_t j = 0; j < 16; ++j)
                if (b0 + j >= sh && b0 + j < sh + n) sb[b0 + j] = g[b0 + j - sh];
        }
    }
    return sb + sh;
}

__global__ void __launch_bounds__(kThreads) k_wire_frame(const FrameK a) {
    __shared__ uint4 stage_words[kWaves][kWindow / 16 + 1];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t s = (uint64_t)blockIdx.x * kWaves + wave;
    const uint64_t total = a.seg0[a.n_batches];
    if (s >= total || s >= a.seg_cap) return;         // (no workgroup barrier below)
    const uint64_t b = batch_of(a.seg0, a.n_batches, s), k = s - a.seg0[b];
    const hq_wire_batch_ref ref = a.batches[b];
    const uint8_t *const g = a.bytes + ref.offset;
    const uint64_t len = ref.len, S = a.S;
    const uint64_t lo = k * S, end = hqw::segment_end(k, S, len);
    uint4 *const words = stage_words[wave];

    // the window [at, at + wn) of the batch in LDS at win
    uint64_t at = lo, entry = k ? kNoEntry : 0;
    uint32_t wn = (uint32_t)std::min<uint64_t>(kWindow, len - at);
    const uint8_t *win = stage(words, g + at, wn, lane);
    wave_sync();
    if (k) {
        // the guess, a candidate per lane; its reads behind the window go to memory
        for (;;) {                                    // (at most (end - lo) / kWindow + 1 windows)
            const uint64_t cand_end = std::min<uint64_t>(at + kWindow, end);
            const hqw::WindowOver over{hqw::Window{win, at, at + wn}, g};
            for (uint64_t q0 = at; q0 < cand_end; q0 += 64) {
                const uint64_t q = q0 + lane;
                const uint64_t hit = __ballot(q < cand_end && hqw::guess_at(over, q, len));
                if (hit) {
                    entry = q0 + (uint64_t)(__ffsll((long long)hit) - 1);
                    break;
                }
            }
            if (entry != kNoEntry || cand_end >= end) break;
            wave_sync();
            at = cand_end;
            wn = (uint32_t)std::min<uint64_t>(kWindow, len - at);
            win = stage(words, g + at, wn, lane);
            wave_sync();
        }
    }

    // the walk, by lane 0 over the window; a field that needs bytes behind it moves the window
    hqw::SegmentWalk w;
    hqw::segment_begin(w, entry);
    hq_wire_span *const region = a.regions + s * a.region;
    const uint64_t region_cap = a.region;
    auto put = [&](uint64_t i, const hq_wire_span &sp) {
        if (i < region_cap) region[i] = sp;
    };
    if (entry != kNoEntry) {
        for (uint64_t turn = 0; turn <= end - lo; ++turn) {   // (every window takes a field)
            int done = 0;
            if (lane == 0)
                done = hqw::walk_segment(hqw::Window{win, at, at + wn}, at + wn, len, end, w, put);
            if (__shfl(done, 0)) break;
            wave_sync();
            at = __shfl((unsigned long long)w.pos, 0);
            wn = (uint32_t)std::min<uint64_t>(kWindow, len - at);
            win = stage(words, g + at, wn, lane);
            wave_sync();
        }
    }
    if (lane == 0) a.segs[s] = w.s;
}

__global__ void __launch_bounds__(256) k_wire_chain(const FrameK a) {
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b > a.n_batches) return;
    if (b == a.n_batches) {
        a.cnt_msgs[b] = a.cnt_spans[b] = 0;
        return;
    }
    const hq_wire_batch_ref ref = a.batches[b];
    const uint64_t s0 = a.seg0[b], n = a.seg0[b + 1] - s0;
    hq_wire_frame_result r{};
    uint32_t voids = 0;
    if (!within(ref, a.len)) r.status = hqw::kMalformed;
    else if (s0 + n > a.seg_cap) r.status = hqw::kUnconfirmed;
    else hqw::chain_batch(a.segs + s0, n, a.S, ref.len, a.region, a.place + s0, r, voids);
    const bool dense = r.status == hqw::kFramed &&
                       !(a.check && (r.deployment_id != a.deployment_id || r.bin_ver != a.bin_ver));
    a.cnt_msgs[b] = dense ? r.n_messages : 0;
    a.cnt_spans[b] = dense ? r.n_spans : 0;
    a.dense[b] = dense;
    if (a.voids) a.voids[b] = voids;
    a.results[b] = r;
}

// the taken segments' spans into the dense list: `offset` from the buffer, `first` from the
// list's first message
__global__ void __launch_bounds__(kThreads) k_wire_spans(const FrameK a) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t s = (uint64_t)blockIdx.x * kWaves + wave;
    if (s == 0 && lane == 0) {
        a.totals[0] = a.msg0[a.n_batches];
        a.totals[1] = a.span0[a.n_batches];
    }
    if (s >= a.seg0[a.n_batches] || s >= a.seg_cap) return;
    const uint64_t b = batch_of(a.seg0, a.n_batches, s);
    if (!a.dense[b]) return;
    const uint64_t span0 = a.span0[b];
    if (s == a.seg0[b] && lane == 0 && span0 + a.cnt_spans[b] > a.span_cap)
        a.results[b].status = hqw::kSpansDidNotFit;
    const SegmentPlace pl = a.place[s];
    if (pl.first_span == kNoEntry) return;
    const uint64_t n = a.segs[s].n_spans, offset = a.batches[b].offset;
    const uint64_t first = a.msg0[b] + pl.first_message;
    const hq_wire_span *const region = a.regions + s * a.region;
    for (uint64_t i = lane; i < n && i < a.region; i += 64) {
        const uint64_t j = span0 + pl.first_span + i;
        if (j >= a.span_cap) break;
        hq_wire_span sp = region[i];
        sp.offset += offset;
        sp.first += (uint32_t)first;
        a.spans[j] = sp;
        if (a.span_batch) a.span_batch[j] = (uint32_t)b;
    }
}

template <class T>
T *take(uint8_t *&p, uint64_t n) {
    T *const out = reinterpret_cast<T *>(p);
    p += (n * sizeof(T) + 255) & ~uint64_t(255);
    return out;
}

}  // namespace

int hq_wire_frame_launch(hq_ctx *ctx, const uint8_t *bytes, uint64_t len,
                         const hq_wire_batch_ref *batches, uint64_t n_batches, uint32_t segment_bytes,
                         uint64_t seg_cap, hq_wire_span *spans, uint64_t span_cap, uint32_t *span_batch,
                         hq_wire_frame_result *results, uint64_t *totals, uint32_t *voids,
                         const uint64_t *deployment_id) {
    const char *const what = "hq_wire_frame_dev";
    const uint32_t S = segment_bytes ? segment_bytes : HQ_WIRE_FRAME_SEGMENT;
    if (S < 64) return hq::fail(ctx, HQ_E_INVAL, "hq_wire_frame_dev: segment_bytes below 64");
    if (n_batches >= 0x7FFFFFFFull || (seg_cap + kWaves - 1) / kWaves > 0x7FFFFFFFull)
        return hq::fail(ctx, HQ_E_INVAL, "hq_wire_frame_dev: 2^31 batches, or 2^33 segments");
    FrameK k{};
    k.bytes = bytes;
    k.len = len;
    k.batches = batches;
    k.n_batches = n_batches;
    k.S = S;
    k.region = S / 128 + 8;
    k.seg_cap = seg_cap;
    const uint64_t nb1 = n_batches + 1;
    size_t tmp = 0;
    int rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, k.nseg, k.seg0, (int)nb1,
                                                                ctx->stream), "hipcub scan size");
    if (rc) return rc;
    const auto pad = [](uint64_t v) { return (v + 255) & ~uint64_t(255); };
    const uint64_t need = 6 * pad(nb1 * 8) + pad(n_batches * 4) + pad(seg_cap * sizeof(Segment)) +
                          pad(seg_cap * sizeof(SegmentPlace)) +
                          pad(seg_cap * k.region * sizeof(hq_wire_span)) + pad(tmp) + 256;
    rc = hq::ensure_workspace(ctx, need);
    if (rc) return rc;
    uint8_t *p = static_cast<uint8_t *>(ctx->ws);
    k.nseg = take<uint64_t>(p, nb1);
    k.seg0 = take<uint64_t>(p, nb1);
    k.cnt_msgs = take<uint64_t>(p, nb1);
    k.cnt_spans = take<uint64_t>(p, nb1);
    k.msg0 = take<uint64_t>(p, nb1);
    k.span0 = take<uint64_t>(p, nb1);
    k.dense = take<uint32_t>(p, n_batches);
    k.segs = take<Segment>(p, seg_cap);
    k.place = take<SegmentPlace>(p, seg_cap);
    k.regions = take<hq_wire_span>(p, seg_cap * k.region);
    void *const d_tmp = take<uint8_t>(p, tmp);
    k.voids = voids;
    k.results = results;
    k.spans = spans;
    k.span_cap = span_cap;
    k.span_batch = span_batch;
    k.totals = totals;
    if (deployment_id) {
        k.check = 1;
        k.bin_ver = HQ_RPC_BIN_VERSION;
        k.deployment_id = *deployment_id;
    }
    const dim3 per_batch((uint32_t)((nb1 + 255) / 256)), per_segment((uint32_t)std::max<uint64_t>(
                                                              1, (seg_cap + kWaves - 1) / kWaves));
    hipStream_t st = ctx->stream;
    rc = hq::pre_launch(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(k_wire_segments, per_batch, dim3(256), 0, st, k);
    rc = hq::post_launch(ctx, what);
    if (!rc)
        rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp, k.nseg, k.seg0, (int)nb1, st),
                           "hipcub scan");
    if (!rc && seg_cap) {
        hipLaunchKernelGGL(k_wire_frame, per_segment, dim3(kThreads), 0, st, k);
        rc = hq::post_launch(ctx, what);
    }
    if (!rc) {
        hipLaunchKernelGGL(k_wire_chain, per_batch, dim3(256), 0, st, k);
        rc = hq::post_launch(ctx, what);
    }
    if (!rc)
        rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp, k.cnt_msgs, k.msg0, (int)nb1, st),
                           "hipcub scan");
    if (!rc)
        rc = hq::check_hip(ctx, hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp, k.cnt_spans, k.span0, (int)nb1, st),
                           "hipcub scan");
    if (!rc) {
        hipLaunchKernelGGL(k_wire_spans, per_segment, dim3(kThreads), 0, st, k);
        rc = hq::post_launch(ctx, what);
    }
    return rc;
}

extern "C" int hq_wire_frame_dev(hq_ctx *ctx, const uint8_t *bytes, uint64_t len,
                                 const hq_wire_batch_ref *batches, uint64_t n_batches,
                                 uint32_t segment_bytes, hq_wire_span *spans, uint64_t span_cap,
                                 uint32_t *span_batch, hq_wire_frame_result *results,
                                 uint64_t totals[2]) {
    if (!ctx) return HQ_E_INVAL;
    if (!totals || (n_batches && (!batches || !results)) || (span_cap && !spans) || (!bytes && len))
        return hq::fail(ctx, HQ_E_INVAL, "hq_wire_frame_dev: NULL argument");
    const uint32_t S = segment_bytes ? segment_bytes : HQ_WIRE_FRAME_SEGMENT;
    if (S < 64) return hq::fail(ctx, HQ_E_INVAL, "hq_wire_frame_dev: segment_bytes below 64");
    // batches that do not overlap have at most this many segments
    const uint64_t seg_cap = len / S + n_batches;
    return hq_wire_frame_launch(ctx, bytes, len, batches, n_batches, S, seg_cap, spans, span_cap,
                                span_batch, results, totals, nullptr, nullptr);
}
