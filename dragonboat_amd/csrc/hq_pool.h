// hq_pool.h — the member pool's compaction on a device worker (hq_worker_compact,
// include/hipquorum.h "group lifecycle"), shared between hq_worker_lifecycle.cpp (plain C++: the
// new member bases from the mirror's structure) and hq_pool.hip (k_pool_compact over the resident
// records). Internal to libhipquorum.so.
#pragma once

#include <cstdint>

#include "../../include/hipquorum.h"
#include "hq_dstep.h"

// k_pool_compact's error word
constexpr uint32_t kPoolErrState = 1;  // a record whose member count or old range does not fit (internal)
constexpr uint32_t kPoolErrRange = 2;  // a new range past the new pool's records (internal)

struct hq_pool_dev;                    // the buffers of one device worker's calls; they keep their
                                       // size from call to call
int hq_pool_dev_open(hq_ctx *ctx, hq_pool_dev **out);
void hq_pool_dev_close(hq_pool_dev *c);
// pinned staging for the new member base of every handle (valid until the next stage call that
// grows it)
int hq_pool_dev_stage(hq_pool_dev *c, uint64_t n_groups, uint32_t **new_mem);
// One kernel over every handle of `st` on the context's stream, behind whatever was queued there,
// and a wait for it: group h's member records move from st->members (n_old records) to
// dst[new_mem[h] ..] (n_new records), and its record's `mem` becomes new_mem[h]. A group without
// members (a vacant handle) copies nothing. HQ_E_INVAL with *error set (kPoolErr*) when the kernel
// refused a group (nothing moved for that group, its `mem` unchanged): dst is then to be dropped.
int hq_pool_dev_compact(hq_pool_dev *c, const hq_dstate_mut *st, uint64_t n_old, hq_dmember *dst,
                        uint64_t n_new, uint64_t *gpu_ns, uint32_t *error);
