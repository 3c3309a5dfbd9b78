#!/usr/bin/env python3
"""Groups started and stopped on a running device worker (hq_worker_start_groups /
hq_worker_stop_groups), the wire's table refresh that follows, and the member pool's compaction
(hq_worker_compact), against the only other way to add to a running worker: hq_worker_add_groups
on a stale mirror, which copies the whole device state back first. One process, one GPU.

The state is step5's, as tools/heartbeat_probe.py builds it: G leader groups of 7 members after
--steps steps. Measured, after --warmup calls, over --reps calls each (median; min and max beside
it), wall time and the GPU time between the call's HIP events (gpu_ns):
  stop / start   hq_worker_stop_groups of --batch handles spread over the handle space, then
                 hq_worker_start_groups of as many new clusters (they take the vacated handles)
  wire           hq_wire_step_device of one ReplicateResp right after such a stop + start (the
                 device table is rebuilt from the live handles and uploaded) and once more with the
                 epoch standing (the table is kept): the refresh is the difference
  compact        hq_worker_compact after G / 8 groups were stopped (each rep stops them, compacts,
                 and starts as many again)
  add_groups     a step that lists one group without events (the mirror is stale again), then
                 hq_worker_add_groups of --batch new clusters; its readback_count delta is stated
hq_worker_readback_count must not move in the new calls. Output: one JSON line, and --out FILE.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dragonboat_amd import hipquorum as hq  # noqa: E402
from heartbeat_probe import LAST0, RREP, TERM, groups_and_members, stats, step_rows  # noqa: E402
import wire_encode as we  # noqa: E402

DEPLOYMENT = 0x5EED


def new_groups(n, cid0):
    g, m = groups_and_members(n)
    g["cluster_id"] = np.arange(cid0, cid0 + n, dtype=np.uint64)
    return g, m


def timed(fn):
    t0 = time.perf_counter_ns()
    r = fn()
    return time.perf_counter_ns() - t0, r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--readback-reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    G, B = a.groups, a.batch
    assert G % 16 == 0 and G >= 8 * B

    w = hq.Worker(0, 8, on_device=True)
    w.add_groups(*groups_and_members(G))
    for s in range(a.steps):
        res = w.step(*step_rows(G, s, False), copy=False)
        assert len(res["fallback_groups"]) == 0
    del res
    next_cid = [G + 1]

    def fresh(n):
        g, m = new_groups(n, next_cid[0])
        next_cid[0] += n
        return g, m

    # stop / start of a batch spread over the handle space
    some = (np.arange(B, dtype=np.uint64) * np.uint64(G // B)).astype(np.uint32)
    t = {k: [] for k in ("stop_wall", "stop_gpu", "start_wall", "start_gpu", "wire_refresh", "wire_kept",
                         "compact_wall", "compact_gpu", "add_wall")}
    wire = hq.Wire(DEPLOYMENT)
    wire.attach_device(w)

    def wire_step(cid):
        wire.reset()
        wire.add_batch(we.batch([we.message(type=RREP, to=1, frm=2, cluster_id=cid, term=TERM,
                                            log_index=LAST0)], deployment_id=DEPLOYMENT,
                                source_address=b"n2:1"))
        dt, (res, st) = timed(lambda: wire.step_device(copy=False))
        assert st.messages == 1 and st.dropped_no_cluster == 0
        return dt

    for i in range(a.warmup + a.reps):
        dt0, ns0 = timed(lambda: w.stop_groups(some))
        g, m = fresh(B)
        dt1, got = timed(lambda: w.start_groups(g, m))
        assert sorted(got.tolist()) == sorted(some.tolist())
        dr, dk = wire_step(int(g["cluster_id"][0])), wire_step(int(g["cluster_id"][1]))
        if i >= a.warmup:
            for k, v in (("stop_wall", dt0), ("stop_gpu", ns0), ("start_wall", dt1),
                         ("start_gpu", w.last_gpu_ns), ("wire_refresh", dr), ("wire_kept", dk)):
                t[k].append(v)
    assert w.readback_count() == 0

    # compaction after an eighth of the groups was stopped
    eighth = (np.arange(G // 8, dtype=np.uint64) * np.uint64(8) + np.uint64(3)).astype(np.uint32)
    info = None
    for i in range(a.warmup + a.reps):
        w.stop_groups(eighth)
        before = w.pool_info()
        dt, ns = timed(w.compact)
        info = w.pool_info()
        assert before["member_records"] > before["live_member_records"] == info["member_records"]
        w.start_groups(*fresh(G // 8))
        if i >= a.warmup:
            t["compact_wall"].append(dt)
            t["compact_gpu"].append(ns)
    assert w.readback_count() == 0
    # the state still steps (step 0's rows: acknowledgements every group's log holds, the restarted
    # groups' included)
    res = w.step(*step_rows(G, 0, False), copy=False)
    assert len(res["fallback_groups"]) == 0 and len(res["deferred"]) == 0
    del res

    # the comparison: add_groups on a stale mirror
    none = (np.zeros(1, np.uint32), np.zeros(2, np.uint64), np.zeros(0, hq.EVENT_DTYPE))
    rb0 = w.readback_count()
    for i in range(a.readback_reps + 1):
        w.step(*none, copy=False)
        g, m = fresh(B)
        dt, _ = timed(lambda: w.add_groups(g, m))
        if i:                                        # (the first one warms the bounce buffer up)
            t["add_wall"].append(dt)
    readbacks = w.readback_count() - rb0
    wire.close()
    w.close()

    out = {"probe": "lifecycle", "groups": G, "steps": a.steps, "batch": B, "members": 7}
    out.update({k: stats(v) for k, v in t.items()})
    out["wire_refresh_minus_kept_us"] = out["wire_refresh"]["median_us"] - out["wire_kept"]["median_us"]
    out["compact_member_records"] = info["member_records"]
    out["compact_bytes_moved"] = info["member_records"] * 24 * 2
    out["compact_GBps_over_gpu_time"] = out["compact_bytes_moved"] / (out["compact_gpu"]["median_us"] * 1e3)
    out["readback_count_new_calls"] = 0
    out["add_groups_readbacks"] = readbacks
    out["add_groups_calls"] = a.readback_reps + 1
    out["add_over_start_wall"] = out["add_wall"]["median_us"] / out["start_wall"]["median_us"]
    out["note"] = "measured once, one box"
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
