#!/usr/bin/env python3
"""The leader heartbeat broadcast of a device worker (hq_worker_heartbeats) against the only other
way a host can learn the same thing: the full-state readback hq_worker_get_group triggers on a
stale mirror. One process, one GPU.

The state is step5's (bench.py's membership, built here): G leader groups of 7 members (4 full
members with the leader, a witness, 2 observers) after --steps steps in which every other member
acknowledges the leader's last entry and answers its heartbeat, every fourth group serves a local
ReadIndex and every group proposes one entry. So that the broadcast has something to say, in the
last step member 2 of every 8th group acknowledges one entry less (it is behind the commit that
the other four reach) and every 16th group's ReadIndex stays unconfirmed (its ctx rides on the
next heartbeats).

Measured, after --warmup calls, over --reps calls each (median; min and max beside it):
  heartbeats  hq_worker_heartbeats over every handle: its wall time, the GPU time between the HIP
              events around its kernels (gpu_ns), the bytes it writes to the host
  readback    a step that lists one group without events (the mirror is stale again), then
              hq_worker_get_group of one group: its wall time, the state bytes it copies back
The outputs are checked against each other: the heartbeat words, lags and ctxs against a numpy
restatement over the state the pattern above leaves. Output: one JSON line, and --out FILE.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dragonboat_amd import hipquorum as hq  # noqa: E402

RREP, HBRESP = 13, 18
REMOTE, OBSERVER, WITNESS = 0, 1, 2
ROLES = (REMOTE,) * 4 + (WITNESS,) + (OBSERVER,) * 2      # node ids 1 .. 7; node 1 is the leader
TERM, LAST0 = 5, 1000
GROUP_BYTES, READ_BYTES, MEMBER_BYTES = 64, 40, 24         # the resident records (hq_dstep.h)


def groups_and_members(G):
    g = np.zeros(G, hq.WORKER_GROUP_DTYPE)
    g["cluster_id"] = np.arange(1, G + 1, dtype=np.uint64)
    g["node_id"], g["term"], g["state"] = 1, TERM, hq.STATE_LEADER
    g["committed"] = g["last_index"] = LAST0
    g["term_start"] = LAST0 - 10
    g["n_members"] = len(ROLES)
    m = np.zeros(G * len(ROLES), hq.MEMBER_DTYPE)
    m["node_id"] = np.tile(np.arange(1, len(ROLES) + 1, dtype=np.uint64), G)
    m["match"] = LAST0
    m["role"] = np.tile(np.array(ROLES, np.uint32), G)
    return g, m


def step_rows(G, s, last_step):
    """Step s as hq_step_input rows, every group in handle order: [read], 6 ReplicateResps,
    6 HeartbeatResps, a proposal."""
    idx = np.arange(G)
    has_read = idx % 4 == 0
    unconfirmed = has_read & (idx % 16 == 0) & last_step
    lagging = (idx % 8 == 0) & last_step
    k = len(ROLES) - 1
    per = 2 * k + 1 + has_read.astype(np.int64)
    offsets = np.zeros(G + 1, np.uint64)
    offsets[1:] = np.cumsum(per)
    ev = np.zeros(int(offsets[-1]), hq.EVENT_DTYPE)
    base = offsets[:-1].astype(np.int64)
    ctx_low = (np.uint64(s + 1) << np.uint64(32)) | idx.astype(np.uint64)
    rd = np.nonzero(has_read)[0]
    r = ev[base[rd]]
    r["kind"], r["hint"], r["hint_high"] = hq.EV_READ, ctx_low[rd], s + 1
    ev[base[rd]] = r
    first = base + has_read
    last_s = np.uint64(LAST0 + s)
    for j in range(k):
        frm = j + 2
        b = ev[first + j]
        b["kind"], b["type"], b["from"], b["term"] = hq.EV_MESSAGE, RREP, frm, TERM
        b["log_index"] = np.where(lagging & (frm == 2), last_s - np.uint64(1), last_s)
        ev[first + j] = b
        b = ev[first + k + j]
        b["kind"], b["type"], b["from"], b["term"] = hq.EV_MESSAGE, HBRESP, frm, TERM
        if ROLES[j + 1] != OBSERVER:
            b["hint"] = np.where(has_read & ~unconfirmed, ctx_low, 0)
            b["hint_high"] = np.where(has_read & ~unconfirmed, s + 1, 0)
        ev[first + k + j] = b
    p = ev[first + 2 * k]
    p["kind"], p["log_index"] = hq.EV_PROPOSE, 1
    ev[first + 2 * k] = p
    return np.arange(G, dtype=np.uint32), offsets, ev


def expected(G, steps):
    """The compact output the pattern leaves: committed = LAST0 + steps - 1 everywhere; member 2
    (list position 1) of every 8th group one behind; every 16th group's ctx pending, so its
    heartbeats go to the 4 other voting members only."""
    idx = np.arange(G)
    pending, lag = idx % 16 == 0, idx % 8 == 0
    words = np.where(pending, 0x1E, 0x7E).astype(np.uint32) | np.where(lag, 1 << 17, 0).astype(np.uint32)
    lags = np.zeros(int(lag.sum()), hq.HEARTBEAT_LAG_DTYPE)
    lags["pos"], lags["member"], lags["match"] = idx[lag], 1, LAST0 + steps - 2
    ctxs = np.zeros(int(pending.sum()), hq.HEARTBEAT_CTX_DTYPE)
    ctxs["pos"], ctxs["ctx_high"] = idx[pending], steps
    ctxs["ctx_low"] = (np.uint64(steps) << np.uint64(32)) | idx[pending].astype(np.uint64)
    return words, lags, ctxs


def stats(ns):
    a = np.sort(np.asarray(ns, np.float64))
    return {"median_us": float(np.median(a)) / 1e3, "min_us": float(a[0]) / 1e3,
            "max_us": float(a[-1]) / 1e3, "n": len(a)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--readback-reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    G = a.groups
    assert G % 16 == 0 and a.steps >= 2

    w = hq.Worker(0, 8, on_device=True)
    g, m = groups_and_members(G)
    w.add_groups(g, m)
    for s in range(a.steps):
        res = w.step(*step_rows(G, s, s == a.steps - 1), copy=False)
        assert len(res["fallback_groups"]) == 0
    del res

    # the heartbeats: warm up (the buffers reach their sizes), then the timed calls
    for _ in range(a.warmup):
        hb = w.heartbeats(copy=False)
    want = expected(G, a.steps)
    np.testing.assert_array_equal(hb["words"], want[0])
    for got, exp in ((hb["lags"], want[1]), (hb["ctxs"], want[2])):
        assert len(got) == len(exp)
        for f in exp.dtype.names:
            np.testing.assert_array_equal(got[f], exp[f], err_msg=f)
    wall, gpu = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter_ns()
        hb = w.heartbeats(copy=False)
        wall.append(time.perf_counter_ns() - t0)
        gpu.append(hb["gpu_ns"])
    host_bytes = 4 * G + 16 * len(hb["lags"]) + 24 * len(hb["ctxs"]) + 32
    # what the kernels read of the state: every listed group's record, the records of the members
    # its broadcast visits, the tail read of a group with one pending; the groups with a record
    # once more by the second kernel
    visited = np.where(np.arange(G) % 16 == 0, 4, 6)
    rec = (hb["words"] >> 16 != 0) | (np.arange(G) % 16 == 0)
    state_read = int(GROUP_BYTES * G + MEMBER_BYTES * visited.sum() + READ_BYTES * (G // 16) +
                     (GROUP_BYTES + MEMBER_BYTES * 6) * rec.sum() + READ_BYTES * (G // 16))
    n_messages = int(hb["n_messages"])

    # the readback: a step makes the mirror stale, get_group pulls the whole state back
    none = (np.zeros(1, np.uint32), np.zeros(2, np.uint64), np.zeros(0, hq.EVENT_DTYPE))
    back = []
    for i in range(a.readback_reps + 1):
        w.step(*none, copy=False)
        t0 = time.perf_counter_ns()
        grp, mem, _ = w.get_group(int(g["cluster_id"][8]))
        dt = time.perf_counter_ns() - t0
        if i:                                        # (the first one warms the bounce buffer up)
            back.append(dt)
    assert int(mem["match"][1]) == LAST0 + a.steps - 2 and int(grp["committed"]) == LAST0 + a.steps - 1
    state_bytes = G * (GROUP_BYTES + 8 * READ_BYTES) + G * len(ROLES) * MEMBER_BYTES
    w.close()

    hb_wall, hb_gpu, rb = stats(wall), stats(gpu), stats(back)
    out = {
        "probe": "heartbeat", "groups": G, "steps": a.steps, "members": len(ROLES),
        "n_messages": n_messages, "n_lags": len(want[1]), "n_ctxs": len(want[2]),
        "heartbeats_wall": hb_wall, "heartbeats_gpu": hb_gpu, "host_bytes_written": host_bytes,
        "state_bytes_read": state_read,
        "state_read_GBps_over_gpu_time": state_read / (hb_gpu["median_us"] * 1e3),
        "readback_wall": rb, "readback_state_bytes": state_bytes,
        "readback_GBps": state_bytes / (rb["median_us"] * 1e3),
        "readback_over_heartbeats_wall": rb["median_us"] / hb_wall["median_us"],
        "note": "measured once, one box",
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
