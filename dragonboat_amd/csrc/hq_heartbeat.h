// hq_heartbeat.h — the leader heartbeat broadcast of a device worker (hq_worker_heartbeats),
// shared between hq_worker.cpp (plain C++: the flush, the checks, the host worker's own form) and
// hq_heartbeat.hip (the kernels and their buffers). Internal to libhipquorum.so.
#pragma once

#include <cstdint>

#include "../../include/hipquorum.h"
#include "hq_dstep.h"

struct hq_hb_dev;     // the buffers of one device worker's heartbeat calls

// hq_hb_dev_run's *error
constexpr uint32_t kHbErrHandle = 1;   // a listed handle at or beyond the state's group count
constexpr uint32_t kHbErrState = 2;    // a group record the kernels cannot take (internal)

int hq_hb_dev_open(hq_ctx *ctx, hq_hb_dev **out);
void hq_hb_dev_close(hq_hb_dev *h);
// The heartbeats of groups[0 .. n) (host memory; NULL: handles 0 .. n - 1; 0 < n < 2^28) over the
// resident state `st` of n_member_records members. HQ_E_INVAL with *error set when a kernel
// refused its input (then *out is not written); *out's arrays are h's pinned buffers, valid until
// its next run.
int hq_hb_dev_run(hq_hb_dev *h, const hq_dstate_view *st, uint64_t n_member_records, uint64_t n,
                  const uint32_t *groups, hq_heartbeat_output *out, uint32_t *error);
