#!/usr/bin/env python3
"""Membership changes applied on a device worker's resident state (hq_worker_config_changes)
against the only other way to follow one: hq_worker_get_group on a stale mirror (the full-state
readback), hq_worker_set_group, and the next step's flush. One process, one GPU.

The state is tools/heartbeat_probe.py's (step5's membership: G leader groups of 7 members) after
--steps steps. Measured, after --warmup calls, over --reps calls each (median; min and max):
  remove      one REMOVE_NODE of member 4 (a full member) in every --every-th group, a different
              set of groups per call: wall time and gpu_ns (the HIP events around the descriptor
              upload, the kernel and the error word's copy)
  replaced    the same change the old way, for the same number of groups: a step without events
              makes the mirror stale (not timed), then get_group of each group (the first one reads
              the whole state back), set_group without the member, and a step without events that
              uploads the queued groups
  add         one ADD_OBSERVER in EVERY group (--add-warmup + --add-reps calls: a group holds at
              most 16 members): every other call finds the member ranges full and moves every
              group to the pool's end
Every status is checked. Output: one JSON line, and --out FILE.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import heartbeat_probe as hp  # noqa: E402
from dragonboat_amd import hipquorum as hq  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--every", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--replaced-reps", type=int, default=3)
    ap.add_argument("--add-warmup", type=int, default=1)
    ap.add_argument("--add-reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    G, every = a.groups, a.every
    calls = a.warmup + a.reps + a.replaced_reps + 1
    assert G % 16 == 0 and G % every == 0 and calls <= every and a.add_warmup + a.add_reps <= 9

    w = hq.Worker(0, 8, on_device=True)
    g, m = hp.groups_and_members(G)
    w.add_groups(g, m)
    for s in range(a.steps):
        res = w.step(*hp.step_rows(G, s, s == a.steps - 1), copy=False)
        assert len(res["fallback_groups"]) == 0
    del res
    none = (np.zeros(1, np.uint32), np.zeros(2, np.uint64), np.zeros(0, hq.EVENT_DTYPE))
    n_changes = G // every
    base = np.arange(0, G, every, dtype=np.uint32)

    def changes(handles, ctype, node):
        c = np.zeros(len(handles), hq.CONFIG_CHANGE_DTYPE)
        c["group"], c["type"], c["node_id"] = handles, ctype, node
        return c

    # (i) REMOVE_NODE in every `every`-th group, a fresh set of groups per call
    wall, gpu = [], []
    r0 = w.readback_count()
    for k in range(a.warmup + a.reps):
        c = changes(base + k, hq.HQ_CC_REMOVE_NODE, 4)
        t0 = time.perf_counter_ns()
        out = w.config_changes(c, copy=False)
        dt = time.perf_counter_ns() - t0
        assert out["n_applied"] == n_changes, out
        if k >= a.warmup:
            wall.append(dt)
            gpu.append(out["gpu_ns"])
    assert w.readback_count() == r0 == 0

    # the path it replaces, for as many groups
    replaced, readback_part = [], []
    mem4 = None
    for k in range(a.replaced_reps + 1):
        hs = base + (a.warmup + a.reps + k)
        w.step(*none, copy=False)                        # the mirror is stale again
        t0 = time.perf_counter_ns()
        first = None
        for h in hs.tolist():
            grp, mem, _ = w.get_group(h + 1)             # cluster id = handle + 1
            if first is None:
                first = time.perf_counter_ns() - t0
            keep = mem[mem["node_id"] != 4]
            w.set_group(h + 1, int(grp["node_id"]), int(grp["term"]), int(grp["state"]),
                        int(grp["committed"]), int(grp["last_index"]), int(grp["term_start"]), keep)
            mem4 = len(keep)
        w.step(*none, copy=False)                        # the flush
        dt = time.perf_counter_ns() - t0
        if k:                                            # (the first warms the bounce buffer up)
            replaced.append(dt)
            readback_part.append(first)
    assert mem4 == len(hp.ROLES) - 1

    # (ii) ADD_OBSERVER in every group
    awall, agpu = [], []
    everyone = np.arange(G, dtype=np.uint32)
    for k in range(a.add_warmup + a.add_reps):
        c = changes(everyone, hq.HQ_CC_ADD_OBSERVER, 100 + k)
        t0 = time.perf_counter_ns()
        out = w.config_changes(c, copy=False)
        dt = time.perf_counter_ns() - t0
        assert out["n_applied"] == G, out
        if k >= a.add_warmup:
            awall.append(dt)
            agpu.append(out["gpu_ns"])
    grp, mem, _ = w.get_group(1)
    assert len(mem) == len(hp.ROLES) - 1 + a.add_warmup + a.add_reps
    w.close()

    rm_wall, rp = hp.stats(wall), hp.stats(replaced)
    out = {
        "probe": "config_change", "groups": G, "steps": a.steps, "members": len(hp.ROLES),
        "remove_changes_per_call": n_changes, "remove_wall": rm_wall, "remove_gpu": hp.stats(gpu),
        "replaced_wall": rp, "replaced_first_get_group_wall": hp.stats(readback_part),
        "replaced_over_remove_wall": rp["median_us"] / rm_wall["median_us"],
        "add_changes_per_call": G, "add_wall": hp.stats(awall), "add_gpu": hp.stats(agpu),
        "add_calls_us": [x / 1e3 for x in awall],
        "readbacks_during_config_changes": 0,
        "note": "measured once, one box; gpu_ns spans the descriptor upload, the kernel and the "
                "error word's copy (not split); wall adds the host's validation, descriptors, "
                "mirror edit and the wait; the replaced path includes ~2 Python calls per group",
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
