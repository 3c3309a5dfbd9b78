#!/usr/bin/env python3
"""A step interval's received Heartbeats on a device worker (hq_worker_heartbeats_received), and the
tick that follows it with the contacts arriving on the device, beside the same tick fed the same
handles through its `contact` list. One process, one GPU.

The state is G follower groups of heartbeat_probe.py's membership (step5's shape: 7 members), node 1
following, committed 40 below last_index. Every call carries one Heartbeat per group at the group's
term. Two kinds of call are timed apart: `advance` (Commit one above the resident committed index:
every group's record is written back) and `steady` (Commit at the resident one: nothing but the
contact bit is written on the device). Every group is in contact after either.

The input arrays (handles, offsets, messages) lie in pinned host memory, as a caller's rows do
(INTEGRATION §4); --pageable takes them from ordinary memory instead, where the runtime stages the
copies. What the host's checks cost (the offsets, and every handle marked in a bitmap so that a
handle listed twice is seen) is timed by a call that is refused at its last handle, which is
listed twice: it runs every check and nothing else.

Per call, one JSON line: gpu_ns (the HIP events around the call's kernel), the wall time
of the call, the wall time and gpu_ns of the hq_worker_tick that follows with no contact list (the
contacts are the device bitmap's), and the bytes moved per group. Then the same number of ticks
with no received call before them and all G handles in the tick's `contact` list, and
hq_worker_heartbeats over the same groups (the kernel's yardstick: it reads the same records).
A summary line with the medians goes to --out.

Bytes per group of one call (one message per group): in over the host link 4 (handle) + 8 (offset)
+ 40 (message) = 52; on the device 48 read of the group record (three quads) + 52 of the staged
input, 16 written back when the commit advances, 4 of contact bitmap per 32 groups (an atomic
each); out over the host link 16 (reply) + 32 (result) = 48 of kernel stores into pinned memory.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dragonboat_amd import hipquorum as hq  # noqa: E402
from heartbeat_probe import LAST0, TERM, groups_and_members, stats  # noqa: E402

E_RTT, H_RTT, SEED = 10, 1, 0x4B3C
LINK_IN, DEV_READ, DEV_WRITE, LINK_OUT = 52, 48 + 52, 16, 48


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pageable", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    G = a.groups
    assert a.reps >= 20 and a.reps + a.warmup <= 40

    g, m = groups_and_members(G)
    g["state"] = hq.STATE_FOLLOWER
    g["committed"] = LAST0 - 40
    m["match"] = np.where(m["node_id"] == 1, LAST0, 0)
    w = hq.Worker(0, 8, on_device=True)
    w.add_groups(g, m)
    w.set_tick_config(E_RTT, H_RTT, True, SEED)
    pin = None if a.pageable else hq.Context(0)
    alloc = (lambda n, dt: np.zeros(n, dt)) if a.pageable else pin.pinned
    everyone, offsets, msgs = alloc(G, np.uint32), alloc(G + 1, np.uint64), alloc(G, hq.HB_RECEIVED_DTYPE)
    everyone[:] = np.arange(G, dtype=np.uint32)
    offsets[:] = np.arange(G + 1, dtype=np.uint64)
    msgs[:] = np.zeros(G, hq.HB_RECEIVED_DTYPE)
    msgs["from"], msgs["term"] = 2, TERM
    committed = LAST0 - 40

    rows = []
    for kind in ("advance", "steady"):
        for i in range(a.warmup + a.reps):
            if kind == "advance":
                committed += 1
            msgs["commit"] = committed
            t0 = time.perf_counter_ns()
            r = w.heartbeats_received(everyone, offsets, msgs, True, copy=False)
            t1 = time.perf_counter_ns()
            tk = w.tick(None, copy=False)
            t2 = time.perf_counter_ns()
            assert (r["n_resp"], r["n_contact"], r["n_committed"]) == (G, G, G if kind == "advance" else 0)
            assert len(tk["election"]) == 0 and tk["n_ticked"] == G
            row = {"kind": kind, "call": i, "warmup": i < a.warmup, "gpu_ns": r["gpu_ns"], "wall_ns": t1 - t0,
                   "tick_wall_ns": t2 - t1, "tick_gpu_ns": tk["gpu_ns"]}
            print(json.dumps(row))
            rows.append(row)
    # every follower was in contact at every tick: nobody's election timer moved past 1
    t = w.get_timers(np.array([0, G // 2, G - 1], np.uint32))
    assert t["election_tick"].tolist() == [1, 1, 1]
    got = w.get_groups(np.array([0, G - 1], np.uint32))["groups"]
    assert got["committed"].tolist() == [committed] * 2 and got["state"].tolist() == [hq.STATE_FOLLOWER] * 2

    # the host's checks alone: the last handle is listed twice
    twice = everyone.copy()
    twice[-1] = twice[-2]
    checks = []
    for i in range(a.warmup + 5):
        t0 = time.perf_counter_ns()
        try:
            w.heartbeats_received(twice, offsets, msgs, True, copy=False)
            raise AssertionError("a handle listed twice was accepted")
        except hq.HQError as e:
            assert e.code == hq.HQ_E_INVAL
        if i >= a.warmup:
            checks.append(time.perf_counter_ns() - t0)

    listed = []
    for i in range(a.warmup + a.reps):
        t0 = time.perf_counter_ns()
        tk = w.tick(everyone, copy=False)
        t1 = time.perf_counter_ns()
        assert len(tk["election"]) == 0 and tk["n_ticked"] == G
        if i >= a.warmup:
            listed.append({"wall_ns": t1 - t0, "gpu_ns": tk["gpu_ns"]})
    bare = []
    for i in range(a.warmup + 5):                    # (no contact at all: what a tick costs here)
        t0 = time.perf_counter_ns()
        tk = w.tick(None, copy=False)
        t1 = time.perf_counter_ns()
        if i >= a.warmup:
            bare.append({"wall_ns": t1 - t0, "gpu_ns": tk["gpu_ns"]})
    hb_wall, hb_gpu = [], []
    for i in range(a.warmup + a.reps):
        t0 = time.perf_counter_ns()
        hb = w.heartbeats(copy=False)
        if i >= a.warmup:
            hb_wall.append(time.perf_counter_ns() - t0)
            hb_gpu.append(hb["gpu_ns"])
    assert hb["n_messages"] == 0 and w.readback_count() == 0
    w.close()
    if pin:
        pin.close()

    def med(kind, key):
        return stats([r[key] for r in rows if r["kind"] == kind and not r["warmup"]])

    out = {"probe": "hb_received", "groups": G, "reps": a.reps, "warmup": a.warmup,
           "input": "pageable" if a.pageable else "pinned", "host_checks_wall": stats(checks),
           "bytes_per_group": {"link_in": LINK_IN, "device_read": DEV_READ, "device_write_advance": DEV_WRITE,
                               "link_out": LINK_OUT}}
    for kind in ("advance", "steady"):
        out[kind] = {"gpu": med(kind, "gpu_ns"), "wall": med(kind, "wall_ns"),
                     "next_tick_wall": med(kind, "tick_wall_ns"), "next_tick_gpu": med(kind, "tick_gpu_ns")}
    out["tick_with_contact_list"] = {"wall": stats([r["wall_ns"] for r in listed]),
                                     "gpu": stats([r["gpu_ns"] for r in listed])}
    out["tick_without_contact"] = {"wall": stats([r["wall_ns"] for r in bare]),
                                   "gpu": stats([r["gpu_ns"] for r in bare])}
    out["heartbeats_gpu"], out["heartbeats_wall"] = stats(hb_gpu), stats(hb_wall)
    out["device_contact_tick_over_listed_tick_wall"] = \
        out["steady"]["next_tick_wall"]["median_us"] / out["tick_with_contact_list"]["wall"]["median_us"]
    out["link_out_GBps_over_gpu_time"] = LINK_OUT * G / (out["steady"]["gpu"]["median_us"] * 1e3)
    out["note"] = "measured once, one box"
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
