// hq_dstep_k.h — what the device step engine's files share (the rest of the library sees
// hq_dstep.h only): the kernels' argument blocks, Layout, the constants, the launchers through
// which hq_dstep_run.hip launches every kernel, and one worker's state (struct hq_dstep).
#pragma once

#include <chrono>
#include <cstdlib>

#include "hq_dstep.h"
#include "hq_internal.h"

namespace hq {
// StepK and JobMap live in each file's unnamed namespace, as the kernels do: a launcher takes one
// across files as its empty base
struct StepArgs {};
struct JobArgs {};
}  // namespace hq

namespace {

// kRerun: 1 for a group with records other than its commit; kEvents: the group's events (pass A
// counts them as it decodes: with 2-byte size words the event prefix pass B needs is their scan);
// kSlotted: 1 for a group whose single ReadyToRead went to its tile's slot (HQ_WORKER_READY_SLOTS)
enum List { kCommits, kReady, kResps, kStates, kDropped, kDeferred, kFallback, kDecisions,
            kRerun, kEvents, kSlotted, kLists };
// the worker's input checks, taken by pass A (which writes no group state) before pass B runs;
// kErrScan: pass A's chained scan of the ReadyToRead places gave up on a tile's word (a stalled
// predecessor: the step re-runs the copy-out through k_step_lite, finish()); kErrTicket: a pass A
// launch found its ticket word not zeroed (an internal fault: nothing of that launch stepped)
enum InputError : uint32_t { kErrHandle = 1, kErrOffsets = 2, kErrBoffsets = 4, kErrTwice = 8,
                             kErrScan = 16, kErrTicket = 32 };
constexpr uint32_t kTickets = 8;  // pass A launches per step (chunks) with their own ticket word

struct StepK : hq::StepArgs {
    hq_dgroup *groups;
    hq_dmember *members;
    hq_dread *reads;
    uint64_t n;                   // groups listed in this step
    uint64_t i_begin, i_end;      // the chunk of them this launch takes
    uint64_t n_handles;           // groups on the device (valid handles)
    uint64_t n_events, n_bytes;   // input sizes (rows or stream bytes)
    uint32_t *stamp;              // per handle: the last step that listed it
    uint32_t step_no;
    uint32_t *error;              // pass A: input errors (kErr* bits)
    uint32_t *wide;               // pass A: a committed index advanced by 2^32 or more (or NULL)
    const uint32_t *handles;
    const uint64_t *offsets;
    const hq_event *events;       // rows, or
    const uint64_t *boffsets;     // an event stream (include/hipquorum.h "event streams")
    const uint8_t *bytes;
    // sized streams: prefix[i] = events before group i << 32 | bytes before it (the scan of the
    // sizes); pass A of byte chunk c takes the groups whose bytes end in [own_lo, own_hi)
    const uint64_t *prefix;
    uint64_t own_lo, own_hi;
    uint32_t *counts;             // [kLists][n]: pass A output (the group's records per list)
    uint32_t *wsum;               // [kLists][nw] + 1 zero: pass A adds each wave's counts (zero
    uint64_t ws;                  //   between steps: k_step_lite clears the ws it used, after the scan)
    const uint32_t *scan;         // exclusive scan of wsum: a wave's first record per list
    uint64_t nw;
    uint32_t *pre;                // [kLists][n] k_step_lite: the counts of the lanes before in the
                                  //   wave, for the groups pass B replays (with scan: their places)
    char *out;                    // pass B: the lists, written straight into pinned host memory
    const struct Layout *layout;  //   at layout->off[list]
    // pass A writes each group's new state in place and its state before the step here (same
    // indexing as groups / members / reads): pass B replays the step from it, and a step with an
    // input error puts it back (k_step_restore)
    hq_dgroup *groups_old;        // (pad1 holds the members' active flags, bit s = member s)
    uint64_t *match_old;
    hq_dread *reads_old;
    // pass A also writes every group's 4-byte advance where the advance column goes (offset 0
    // of the host region) when spec_col is set: those PCIe writes then overlap the later chunks'
    // input copies, and k_step_lite skips them when the layout picks that column (spec_valid)
    uint32_t spec_col, spec_valid;
    uint8_t *rerun;               // [n] pass A: bit 0 the group has records other than its
                                  //   commit (and not just one ReadyToRead), bit 1 pass A stepped
                                  //   it (0: an input error), bit 2 its only record besides the
                                  //   commit is one ReadyToRead, kept in ready_slot
    hq_ready_to_read *ready_slot; // [n] pass A: a group's first ReadyToRead of the step
    uint32_t *rerun_list;         // [n] k_step_lite: the positions of those groups, in order
    // the jobs path (hq_dstep_run_jobs: several workers' steps in shared launches): the layout's
    // arguments, the sizes of a sized stream and the per-1024-group sums of their scan
    uint64_t out_cap;
    uint32_t allow_column, pad_j;
    struct Layout *host_layout;
    const uint32_t *sizes;
    const uint32_t *sizes_src;    // the caller's sizes when in pinned host memory (read over the
                                  //   link by k_size_sums, which writes `sizes`), else NULL
    uint64_t *bsum;
    // pass A over a stream with the advance column speculated (spec_ready): the ReadyToRead
    // records of the groups pass B does not replay go straight to their places in the host region
    // (ready_off: the list's offset when the commits are the 4-byte column), each tile of 256
    // groups finding its first place by a chained scan over `tiles` in start order (`tickets`,
    // one word per pass A launch `chunk`; k_step_lite zeroes them)
    uint32_t spec_ready, chunk;
    uint64_t ready_off;
    // HQ_WORKER_READY_COMPACT: pass A flags a ReadyToRead whose index - the group's committed
    // index before the step does not fit 32 bits (the step then keeps the 32-byte records)
    uint32_t *ready_wide;
    uint64_t *tiles;              // per tile: step_no << 32 | chunk << 29 | inclusive << 28 | count
    uint32_t *tickets;            // [kTickets]
    // 2-byte size words (hq_step_stream.sizes16: a group's byte count only): the prefixes hold
    // bytes alone, pass A counts each group's events as it decodes them (kEvents) and a group's
    // bytes that do not decode are an input error (kErrBoffsets); sizes16_src as sizes_src
    const uint16_t *sizes16;
    const uint16_t *sizes16_src;
    uint32_t bytes_only;
    // HQ_WORKER_READY_SLOTS: pass A writes the single ReadyToRead of every group that has no other
    // record (and whose index - committed fits 32 bits) as an hq_ready_compact into its tile's slot
    // in the host region — tile t (256 groups) at out + slot_off + 6144 t, in group order, its
    // count at out + cnt_off + 4 t — in the link's write direction while pass A reads the stream;
    // those groups leave the list (kSlotted instead of kReady)
    uint32_t slots;
    uint64_t slot_off, cnt_off;
    uint32_t test_scan_fail, pad_t;   // HQ_TEST_SCAN_FAIL at open: every look-back gives up (tests)
};

constexpr uint32_t kSlotTile = 256;   // groups per slot tile (pass A's workgroup)
constexpr uint64_t kSlotTileBytes = kSlotTile * sizeof(hq_ready_compact);
static_assert(kSlotTileBytes % 256 == 0, "slot tiles keep the region's 256-byte alignment");

// where the lists go in the host output region (k_layout, from the scanned counts); a step with
// an input error or a region too small has pass B write nothing, not even state
struct Layout {
    uint64_t off[kLists];
    uint32_t len[kLists];
    uint64_t total;
    uint32_t error, overflow;
    uint32_t commit_column;       // the commits list is a column: one word per listed group
                                  // (kColumn64: the committed index, kColumn32: its advance)
    uint32_t ready_compact;       // the ReadyToReads are hq_ready_compact records
    uint32_t pad;
    uint64_t reserve;             // bytes ahead of the lists (the slot form's column + slots)
};
constexpr uint32_t kColumn64 = 1, kColumn32 = 2;
constexpr uint32_t kReadyCompact = 4;   // allow_column bit: HQ_WORKER_READY_COMPACT
constexpr uint32_t kReadySlots = 8;     // allow_column bit: this step writes slots (ready slots)

// pass A's chained scan of the ReadyToRead places (StepK::tiles): a tile publishes its count
// (aggregate) and then its inclusive prefix, tagged with the step and the launch's chunk so that
// words of earlier launches and steps are never taken for this one's
constexpr uint32_t kTileVal = (1u << 28) - 1;

// The jobs path: one launch over several workers' steps, each job's groups in consecutive
// workgroups (blk0[j] .. blk0[j + 1]) and its StepK in device memory
constexpr uint32_t kMaxJobs = kDStepMaxJobs;
struct JobMap : hq::JobArgs {
    const StepK *ks;              // the jobs' StepK, job0 .. job0 + count - 1 in this launch
    uint32_t job0, count;
    uint32_t blk0[kMaxJobs + 1];  // relative to job0
    uint32_t *tickets;            // pass A: the launch's ticket word is tickets[chunk]; k_step_lite_jobs
    uint32_t chunk;               //   zeroes them
    StepK *table_out;             // k_size_sums (reading `ks` from its pinned copy): workgroup 0
                                  //   writes the jobs' StepK there for the later launches
    uint32_t bsum_scanned, pad;   // k_size_apply: the tiles' totals were scanned (k_bsum_scan_jobs)
};
static_assert(sizeof(StepK) % 8 == 0, "k_size_sums copies the table in 8-byte words");

__device__ __forceinline__ uint32_t job_of(const JobMap &m, uint32_t b) {
    uint32_t j = 0;               // (uniform: kernel arguments and blockIdx)
    while (j + 1 < m.count && b >= m.blk0[j + 1]) ++j;
    return j;
}

// input chunks of a large step (at least kChunkGroups groups each): chunk c's copy overlaps pass A
// of chunk c - 1, and the last chunk's pass A is the step's tail (8 chunks: no faster, profiles/r03e/ab_step_chunks.log)
constexpr int kMaxChunks = 4;
constexpr int kMaxJobChunks = 8;   // the jobs path's chunks of whole jobs (events per copy stream)
static_assert(kMaxChunks <= kMaxJobChunks, "the chunk events serve both paths");
static_assert(kMaxJobChunks <= kTickets, "a ticket word per pass A launch");
constexpr uint64_t kChunkGroups = 65536;
// the slot form's part of the host region ahead of the lists: the 4-byte column at 0, tile t's
// slots at slot_off + 6144 t, the tiles' counts at cnt_off; returns its size (the lists' start)
__host__ __device__ inline uint64_t slot_layout(uint64_t n, uint64_t *slot_off, uint64_t *cnt_off) {
    const uint64_t tiles = (n + kSlotTile - 1) / kSlotTile;
    const uint64_t so = (n * 4 + 255) & ~uint64_t(255);
    const uint64_t co = so + tiles * kSlotTileBytes;
    if (slot_off) *slot_off = so;
    if (cnt_off) *cnt_off = co;
    return co + ((tiles * 4 + 255) & ~uint64_t(255));
}

constexpr int kScanT = 1024, kScanE = 11;
constexpr uint64_t kScanSmall = 2 * kScanT * kScanE;   // sums k_scan_layout takes (2 tiles)

constexpr uint32_t kSizeTile = 1024;   // groups per workgroup of 256 threads (4 each)
// a job of more size tiles than this has its tiles' totals scanned by a launch of their own
// (k_bsum_scan_jobs) instead of each k_size_apply workgroup summing the totals before it (the
// sum's work grows with the square of the tiles: ~134 M L2 loads at 16 M groups)
constexpr uint64_t kSizeApplyDirect = 2048;

// kernel k over `grid` workgroups of `block` threads on s: the launch's status under `what`
template <class K, class... A>
int launch(hq_ctx *ctx, hipStream_t s, const char *what, K k, uint64_t grid, unsigned block,
           const A &...a) {
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(block), 0, s, a...);
    return hq::check_hip(ctx, hipGetLastError(), what);
}

}  // namespace

namespace hq {
// One launcher per kernel, over k's groups or m's jobs (launch_step: groups [k.i_begin, k.i_end),
// write: pass B). hq_dstep_step.hip:
int launch_step(hq_ctx *ctx, bool write, bool stream, bool small, const StepArgs &k);
int launch_step_jobs(hq_ctx *ctx, bool write, bool small, const JobArgs &m);
int launch_step_lite(hq_ctx *ctx, hipStream_t s, const StepArgs &k);
int launch_step_lite_jobs(hq_ctx *ctx, hipStream_t s, const JobArgs &m);
int launch_step_restore(hq_ctx *ctx, hipStream_t s, const StepArgs &k);
// hq_dstep_layout.hip:
int launch_layout(hq_ctx *ctx, hipStream_t s, const StepArgs &k);
int launch_scan_layout(hq_ctx *ctx, hipStream_t s, const StepArgs &k);
int launch_scan_layout_jobs(hq_ctx *ctx, hipStream_t s, const JobArgs &m);
int launch_size_sums(hq_ctx *ctx, hipStream_t s, const JobArgs &m);
int launch_bsum_scan_jobs(hq_ctx *ctx, hipStream_t s, const JobArgs &m);
int launch_size_apply(hq_ctx *ctx, hipStream_t s, const JobArgs &m);
// the hipcub scans (tmp NULL: only *tmp_bytes, the temporary's size)
int scan_wave_sums(hq_ctx *ctx, hipStream_t s, void *tmp, size_t *tmp_bytes, uint32_t *wsum,
                   uint32_t *scan, size_t ws);
int scan_sizes(hq_ctx *ctx, hipStream_t s, void *tmp, size_t *tmp_bytes, const void *sizes,
               bool s16, uint64_t n, uint64_t *prefix);
inline uint64_t now_ns() {
    using namespace std::chrono;
    return (uint64_t)duration_cast<nanoseconds>(steady_clock::now().time_since_epoch()).count();
}
inline bool env_flag(const char *name) {   // NAME=<non-zero> in the environment
    const char *v = std::getenv(name);
    return v && std::atoi(v) != 0;
}
// hq_dstep.hip: a device buffer of at least `need` bytes (keep: with its contents), the device's
// clock into d->clock_host[slot] (HQ_WAIT_CLOCK), the step thread's wait for s by d's policy
int grow(hq_ctx *ctx, void **p, size_t *cap, size_t need, bool keep, const char *what);
template <class T>
int grow(hq_ctx *ctx, T **p, size_t *cap, size_t need, bool keep, const char *what) {
    return grow(ctx, reinterpret_cast<void **>(p), cap, need, keep, what);
}
int stamp_clock(hq_dstep *d, hipStream_t s, int slot);
int wait_stream(hq_dstep *d, hipStream_t s, const char *what);
}  // namespace hq

// (StepK and Layout are unnamed-namespace types: every file that sees this struct must take them
// from this header alone, so that the struct is the same text and layout in each)
struct hq_dstep {
    hq_ctx *ctx = nullptr;
    // HQ_TEST_FAIL_REGROW=1 in the environment at open: the output region's regrow fails (the
    // failure path's test, tests/test_gpu_worker.py)
    bool test_fail_regrow = false;
    bool test_scan_fail = false;  // HQ_TEST_SCAN_FAIL=1 at open: pass A's look-backs give up
    hq_dgroup *groups = nullptr;
    hq_dread *reads = nullptr;
    hq_dmember *members = nullptr;
    // the state pass A saved (StepK::groups_old ...), as large as the state
    hq_dgroup *groups_old = nullptr;
    hq_dread *reads_old = nullptr;
    uint64_t *match_old = nullptr;
    uint8_t *rerun = nullptr;     // [rcap] per listed group
    uint32_t *rerun_list = nullptr;
    hq_ready_to_read *ready_slot = nullptr;
    size_t rcap = 0;
    uint32_t *stamp = nullptr;    // [gcap] step stamps (duplicate handles)
    uint64_t gcap = 0, mcap = 0;
    uint64_t n_groups = 0;        // group records uploaded (valid handles)
    uint32_t max_members = 0;     // the most members of any uploaded group
    uint32_t step_no = 0;
    uint32_t commit_column = 0;   // bits: kColumn64 HQ_WORKER_COMMIT_COLUMN, kColumn32 _ADVANCE
    // step staging
    void *in = nullptr;
    size_t in_cap = 0;
    uint32_t *counts = nullptr, *scan = nullptr, *bases = nullptr;
    size_t cnt_cap = 0;
    uint32_t *wsum = nullptr;     // pass A's per-wave sums (StepK::wsum), zero between steps
    size_t wsum_cap = 0;          //   (bytes)
    bool wsum_dirty = true;
    void *scan_tmp = nullptr;
    size_t scan_tmp_cap = 0;
    void *host_out = nullptr;     // pinned host region pass B writes the lists into
    size_t host_out_cap = 0;
    Layout *layout = nullptr;     // device: the lists' places (k_layout)
    Layout *host_layout = nullptr;  // pinned mirror, copied back at the end of the step
    // a large step runs in chunks of groups: chunk c's input copy (copy stream) overlaps pass A
    // of chunk c - 1, and its result copy overlaps pass B of chunk c + 1 (compute stream); the
    // copy stream is created by the first such step
    hipStream_t copy = nullptr;
    hipEvent_t ev_in[kMaxJobChunks] = {};
    // the jobs path's second copy stream (jobs' byte copies alternate between the two, so that
    // one copy's start-up gap overlaps the other's transfer) and its events
    hipStream_t copy2 = nullptr;
    hipEvent_t ev_in2[kMaxJobChunks] = {};
    // the pinned bounce buffer of hq_dstep_put / _get (two halves) and each half's last copy
    char *bounce = nullptr;
    hipEvent_t bounce_ev[2] = {nullptr, nullptr};
    hipEvent_t ev_sync = nullptr;  // blocking-sync event: a waiting worker thread sleeps
    // timing events around a step's device work (hq_dstep_out::gpu_ns): the host's wait for a
    // step, less the GPU's time, is its wake-up and queueing delay
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;
    // the jobs path (hq_dstep_run_jobs, this engine first): the jobs' StepK, pinned and on device
    StepK *jobs_host = nullptr, *jobs_dev = nullptr;
    const StepK *jobs_host_dev = nullptr;   // jobs_host's device address (k_size_sums reads it)
    uint32_t jobs_cap = 0;
    // pass A's ticket words (StepK::tickets), zeroed by k_step_lite; a step that stopped before
    // it leaves them to clear (dirty), and pass A's chained-scan words per tile of 256 groups
    uint32_t *tickets = nullptr;
    bool tickets_dirty = false;
    uint64_t *tiles = nullptr;
    size_t tiles_cap = 0;         // (bytes)
    // how the step's thread waits for the device (hq_dstep_set_wait; HQ_WAIT_*) and the clock of
    // the last wait: the device's 100-MHz stamp after the step's last kernel (HQ_WAIT_CLOCK), in
    // pinned memory
    uint32_t wait_mode = HQ_WAIT_BLOCK, wait_poll_us = 50, wait_sleep_us = 20;
    uint64_t wait_pred_ns = 0;    // HQ_WAIT_ADAPT: the last step's wait, start to seen done
    bool wait_clock = false;
    uint64_t *clock_host = nullptr;
    hq_wait_clock last_wait{};
};
