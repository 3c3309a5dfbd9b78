#!/usr/bin/env python3
"""Listed groups fetched from and resumed on a device worker's resident state
(hq_worker_get_groups / hq_worker_set_groups) against the only other way to do either:
hq_worker_get_group on a stale mirror (the full-state readback), hq_worker_set_group per group,
and the next step's flush. One process, one GPU.

The state is tools/heartbeat_probe.py's (step5's membership: G leader groups of 7 members) after
--steps steps. Measured, after --warmup calls, over --reps calls each (median; min and max):
  fetch       get_groups of every --every-th group: wall time and gpu_ns (the HIP events around
              the handle upload, the gather kernel and the error word's copy)
  resume      set_groups of the same groups with what was fetched: wall time and gpu_ns (the
              handle upload, the scatter kernel, the error word's copy)
  fetch_all   get_groups of every group (--all-reps calls after one warm-up)
  replaced    the old way for the same listed groups: a step without events makes the mirror stale
              (not timed), then get_group of each group (the first one reads the whole state
              back), set_group of each with what it returned, and a step without events that
              uploads the queued groups
The readback counter is checked to stay 0 until the replaced path runs. Output: one JSON line, and
--out FILE.
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

RECORD_BYTES = 768


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--every", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--all-reps", type=int, default=3)
    ap.add_argument("--replaced-reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    G, every = a.groups, a.every
    assert G % 16 == 0 and G % every == 0

    w = hq.Worker(0, 8, on_device=True)
    g, m = hp.groups_and_members(G)
    w.add_groups(g, m)
    for s in range(a.steps):
        res = w.step(*hp.step_rows(G, s, s == a.steps - 1), copy=False)
        assert len(res["fallback_groups"]) == 0
    del res
    none = (np.zeros(1, np.uint32), np.zeros(2, np.uint64), np.zeros(0, hq.EVENT_DTYPE))
    listed = np.arange(0, G, every, dtype=np.uint32)
    n_listed = len(listed)

    def timed(fn, warmup, reps):
        wall, gpu = [], []
        for k in range(warmup + reps):
            t0 = time.perf_counter_ns()
            ns = fn()
            dt = time.perf_counter_ns() - t0
            if k >= warmup:
                wall.append(dt)
                gpu.append(ns)
        return hp.stats(wall), hp.stats(gpu)

    # fetch: the listed groups, views of the worker's buffers
    got = {}

    def fetch():
        got["r"] = w.get_groups(listed, copy=False)
        return got["r"]["gpu_ns"]

    fetch_wall, fetch_gpu = timed(fetch, a.warmup, a.reps)
    r = got["r"]
    assert len(r["groups"]) == n_listed and int(r["member_offsets"][-1]) == n_listed * len(hp.ROLES)
    assert (r["groups"]["cluster_id"] == listed.astype(np.uint64) + 1).all()
    groups, members = r["groups"].copy(), r["members"].copy()
    pending = int(r["read_offsets"][-1])

    # resume: the same groups with what was fetched
    resume_wall, resume_gpu = timed(lambda: w.set_groups(groups, members), a.warmup, a.reps)
    back = w.get_groups(listed, copy=False)
    assert back["members"].tobytes() == members.tobytes() and int(back["read_offsets"][-1]) == 0

    # fetch of every group
    def fetch_all():
        out = w.get_groups(None, copy=False)
        assert len(out["groups"]) == G
        return out["gpu_ns"]

    all_wall, all_gpu = timed(fetch_all, 1, a.all_reps)
    assert w.readback_count() == 0

    # the path the two calls replace, for the same listed groups
    replaced, readback_part, set_part, flush_part = [], [], [], []
    for k in range(a.replaced_reps + 1):
        w.step(*none, copy=False)                        # the mirror is stale again
        t0 = time.perf_counter_ns()
        fetched = []
        first = None
        for h in listed.tolist():
            grp, mem, _ = w.get_group(h + 1)             # cluster id = handle + 1
            if first is None:
                first = time.perf_counter_ns() - t0
            fetched.append((grp, mem))
        t1 = time.perf_counter_ns()
        for grp, mem in fetched:
            w.set_group(int(grp["cluster_id"]), int(grp["node_id"]), int(grp["term"]), int(grp["state"]),
                        int(grp["committed"]), int(grp["last_index"]), int(grp["term_start"]), mem)
        t2 = time.perf_counter_ns()
        w.step(*none, copy=False)                        # the flush
        t3 = time.perf_counter_ns()
        if k:                                            # (the first warms the bounce buffer up)
            replaced.append(t3 - t0)
            readback_part.append(first)
            set_part.append(t2 - t1)
            flush_part.append(t3 - t2)
    readbacks = w.readback_count()
    w.close()

    rp = hp.stats(replaced)
    out = {
        "probe": "groups", "groups": G, "steps": a.steps, "members": len(hp.ROLES),
        "listed_per_call": n_listed, "record_bytes": RECORD_BYTES,
        "listed_bytes_per_call": n_listed * RECORD_BYTES, "pending_reads_in_listed": pending,
        "fetch_wall": fetch_wall, "fetch_gpu": fetch_gpu,
        "resume_wall": resume_wall, "resume_gpu": resume_gpu,
        "fetch_all_wall": all_wall, "fetch_all_gpu": all_gpu, "fetch_all_bytes": G * RECORD_BYTES,
        "readbacks_during_listed_calls": 0,
        "replaced_wall": rp, "replaced_first_get_group_wall": hp.stats(readback_part),
        "replaced_set_group_wall": hp.stats(set_part), "replaced_flush_wall": hp.stats(flush_part),
        "replaced_readbacks": readbacks,
        "replaced_over_fetch_plus_resume_wall":
            rp["median_us"] / (fetch_wall["median_us"] + resume_wall["median_us"]),
        "note": "measured once, one box; gpu_ns spans the handle upload, the kernel (its stores or "
                "loads cross the link to pinned host memory) and the error word's copy (not split); "
                "wall adds the host's validation, the flush check, pack / unpack and the wait; the "
                "replaced path includes 2 Python calls per group and its get_group of every listed "
                "group after the first reads the fresh mirror",
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
