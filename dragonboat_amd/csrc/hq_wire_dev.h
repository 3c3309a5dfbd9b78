// hq_wire_dev.h — the wire's device mode (hq_wire_attach_device), shared between hq_wire.cpp (plain
// C++: framing, the batch checks, the local events, the stats) and hq_wire_dev.hip (the kernels and
// the device buffers). Internal to libhipquorum.so.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/hipquorum.h"
#include "hq_stream.h"

struct hq_wire_dev;   // the device side of one attached wire

// worker: a device worker (HQ_E_INVAL otherwise)
int hq_wire_dev_open(hq_worker *worker, hq_wire_dev **out);
void hq_wire_dev_close(hq_wire_dev *d);
const char *hq_wire_dev_error(const hq_wire_dev *d);
// forget the queued batches
void hq_wire_dev_reset(hq_wire_dev *d);
// Queue one framed batch (spans with offsets from 0, as hq_wire_frame_batch gives them with base
// 0; n_messages > 0): bytes the device can read in place are referenced, any other memory is
// copied into the wire's pinned staging. `index` names the batch in hq_wire_dev_step's rejected
// list.
int hq_wire_dev_add_batch(hq_wire_dev *d, const uint8_t *bytes, size_t len, const hq_wire_span *spans,
                          uint64_t n_spans, uint64_t n_messages, uint32_t index);
// The framing on the device (hq_wire_set_device_framing): from now on batches are queued unframed
// by hq_wire_dev_queue and framed by hq_wire_dev_step, which keeps of them those of deployment_id
// and HQ_RPC_BIN_VERSION. Nothing may be queued.
void hq_wire_dev_set_framing(hq_wire_dev *d, bool on, uint64_t deployment_id);
bool hq_wire_dev_framing(const hq_wire_dev *d);
// Queue one batch as it came (any bytes), placed as hq_wire_dev_add_batch places it.
int hq_wire_dev_queue(hq_wire_dev *d, const uint8_t *bytes, size_t len, uint32_t index);
// of the last step: segments, void segments, batches with status 2 or 3; steps framed on the host
// since the open
void hq_wire_dev_frame_stats(const hq_wire_dev *d, uint64_t out[4]);
// hq_wire_frame_dev (hq_wire_frame_dev.hip) with the segment records sized by the caller
// (seg_cap; batches whose segments lie beyond it come back unconfirmed), the void segments per
// batch in voids (device memory, or NULL), and, with deployment_id, only the batches of that
// deployment and HQ_RPC_BIN_VERSION in the dense list. The temporaries are ctx's workspace.
int hq_wire_frame_launch(hq_ctx *ctx, const uint8_t *bytes, uint64_t len,
                         const hq_wire_batch_ref *batches, uint64_t n_batches, uint32_t segment_bytes,
                         uint64_t seg_cap, hq_wire_span *spans, uint64_t span_cap, uint32_t *span_batch,
                         hq_wire_frame_result *results, uint64_t *totals, uint32_t *voids,
                         const uint64_t *deployment_id);
// Decode the queued batches, key and sort their records with the local ones (locals[i].key the
// worker's handle), and step the worker over the rows. counters: messages, entries,
// snapshot_received, dropped_no_cluster of the batches that decoded; rejected / n_rejected: the
// `index` of every batch that held a malformed message (owned by d until its next step), their
// count of bytes in *rejected_bytes and their number in *n_bad_message. With the framing on the
// device the batches are framed first: *add is then the host's share of the stats for them
// (batches, bytes, dropped_batches, dropped_messages; zero otherwise), and a batch with a framing
// error is in the rejected list as well (counted neither in *add nor in *n_bad_message).
int hq_wire_dev_step(hq_wire_dev *d, const hqs::WireEvent *locals, uint64_t n_locals,
                     hq_step_output *out, uint64_t counters[4], const uint32_t **rejected,
                     uint64_t *n_rejected, uint64_t *rejected_bytes, uint64_t *n_bad_message,
                     hq_wire_stats *add);
