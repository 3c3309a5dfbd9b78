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
// Decode the queued batches, key and sort their records with the local ones (locals[i].key the
// worker's handle), and step the worker over the rows. counters: messages, entries,
// snapshot_received, dropped_no_cluster of the batches that decoded; rejected / n_rejected: the
// `index` of every batch that held a malformed message (owned by d until its next step), their
// count of bytes in *rejected_bytes.
int hq_wire_dev_step(hq_wire_dev *d, const hqs::WireEvent *locals, uint64_t n_locals,
                     hq_step_output *out, uint64_t counters[4], const uint32_t **rejected,
                     uint64_t *n_rejected, uint64_t *rejected_bytes);
