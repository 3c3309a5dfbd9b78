#!/usr/bin/env python3
"""The wire's device mode against the host wire path, at step size, in one process on one GPU.

The workload is step5's steady-state mix built here (not bench.py's generator): G leader groups of
7 members (4 full members with the leader, a witness, 2 observers); per group and step a
ReplicateResp and a HeartbeatResp from each of the 6 other members (12 messages), a proposal, and
for every fourth group a local ReadIndex whose ctx the voting members' HeartbeatResps confirm. The
messages arrive as one MessageBatch per (message type, sender), or with --batch-messages N cut
into batches of N messages (2048 is the reference's SendQueueLength, which processMessages drains
into one batch, transport.go:460-475), marshalled by hq_wire_encode_batch into pinned memory
outside the timed region.

Per step, over --steps steps after --warmup:
  host1   hq_wire_add_batch + add_locals + step_sized + hq_worker_step_stream, one thread
  host16  the same on 16 step workers (G / 16 groups each), each wire on its own thread, then
          hq_worker_step_jobs
  device  hq_wire_attach_device: add_batch frames, hq_wire_step_device decodes, keys, sorts and
          steps on the GPU; the batches are read in place
  device_framed  the same with hq_wire_set_device_framing: add_batch only queues, the step frames
          on the GPU as well
The device paths' host time is reported split into add_batch and add_locals.

Every path must commit and release the same numbers of groups and ReadIndexes per step. The link
yardstick is tools/link_probe's read rate on the same box. Output: one JSON line, and --out FILE.
"""
import argparse
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dragonboat_amd import hipquorum as hq  # noqa: E402

RREP, HBRESP = 13, 18
REMOTE, OBSERVER, WITNESS = 0, 1, 2
ROLES = (REMOTE,) * 4 + (WITNESS,) + (OBSERVER,) * 2      # node ids 1 .. 7; node 1 is the leader
DEP, TERM, LAST0 = 0x5EED, 5, 100


def groups_and_members(G):
    g = np.zeros(G, hq.WORKER_GROUP_DTYPE)
    g["cluster_id"] = np.arange(1, G + 1, dtype=np.uint64) * np.uint64(3)
    g["node_id"], g["term"], g["state"] = 1, TERM, hq.STATE_LEADER
    g["committed"] = g["last_index"] = g["term_start"] = LAST0
    g["n_members"] = len(ROLES)
    m = np.zeros(G * len(ROLES), hq.MEMBER_DTYPE)
    m["node_id"] = np.tile(np.arange(1, len(ROLES) + 1, dtype=np.uint64), G)
    m["match"] = LAST0
    m["role"] = np.tile(np.array(ROLES, np.uint32), G)
    m["active"] = 1
    return g, m


class Arrivals:
    """Step s's batches for groups [lo, hi) in pinned buffers (rewritten per step), and its local
    events."""

    def __init__(self, pin, cids, batch_messages=0):
        self.cids = cids
        n = len(cids)
        self.chunk = batch_messages or max(1, n)
        chunks = -(-n // self.chunk)
        self.bufs = [pin.pinned(n * 72 + 64 * (chunks + 1), np.uint8)
                     for _ in range(2 * (len(ROLES) - 1))]
        self.batches = []                 # (address, length) of every batch, in arrival order
        self.msg = np.zeros(n, hq.WIRE_MESSAGE_DTYPE)
        self.msg["ev"]["kind"] = hq.EV_MESSAGE
        self.msg["ev"]["term"] = TERM
        self.msg["cluster_id"] = cids
        self.msg["to"] = 1
        self.reads = np.nonzero(cids % np.uint64(4) == 0)[0]
        # local events: [ReadIndex] then a proposal, per group
        per = np.ones(n, np.uint64)
        per[self.reads] += np.uint64(1)
        self.loff = np.zeros(n + 1, np.uint64)
        self.loff[1:] = np.cumsum(per)
        self.lev = np.zeros(int(self.loff[-1]), hq.EVENT_DTYPE)
        self.lev["kind"] = hq.EV_PROPOSE
        self.lev["log_index"] = 1
        self.read_rows = self.loff[self.reads].astype(np.int64)
        self.lev["kind"][self.read_rows] = hq.EV_READ
        self.lev["log_index"][self.read_rows] = 0
        self.lev["hint_high"][self.read_rows] = cids[self.reads]

    def set(self, s):
        m, k, batches = self.msg, 0, []
        self.lev["hint"][self.read_rows] = s + 1
        for typ in (RREP, HBRESP):
            for node in range(2, len(ROLES) + 1):
                m["ev"]["type"], m["ev"]["from"] = typ, node
                m["ev"]["log_index"] = LAST0 + s if typ == RREP else 0
                m["ev"]["hint"] = m["ev"]["hint_high"] = 0
                if typ == HBRESP and ROLES[node - 1] != OBSERVER:   # (an observer's ack of a ctx
                    m["ev"]["hint"][self.reads] = s + 1             # is the worker's fallback)
                    m["ev"]["hint_high"][self.reads] = self.cids[self.reads]
                at = 0
                for lo in range(0, len(m), self.chunk):
                    out = hq.encode_wire_batch(m[lo:lo + self.chunk], deployment_id=DEP,
                                               source_address=b"n%d:63000" % node,
                                               out=self.bufs[k][at:])
                    batches.append((self.bufs[k].ctypes.data + at, len(out)))
                    at += len(out)
                k += 1
        self.batches = batches

    def add_batches_to(self, wire):
        for addr, n in self.batches:
            wire.add_batch_at(addr, n)

    def add_to(self, wire):
        self.add_batches_to(wire)
        wire.add_locals(self.cids, self.loff, self.lev)

    @property
    def n_messages(self):
        return len(self.cids) * len(self.bufs)

    @property
    def n_bytes(self):
        return sum(n for _, n in self.batches)


def counts(res):
    n_commits = res.get("n_commits", len(res["commits"]))
    n_ready = len(res["ready"]) + len(res.get("ready_compact", ())) + len(res.get("ready_slots", ()))
    return int(n_commits), int(n_ready), len(res["fallback_groups"])


def link_read_gbps(device):
    exe = os.path.join(ROOT, "tools", "link_probe")
    if not os.path.exists(exe):
        return None
    r = subprocess.run([exe, "256", str(device), "--json"], capture_output=True, text=True)
    try:
        return json.loads(r.stdout.strip().splitlines()[-1])["read_GBps"]
    except (ValueError, IndexError, KeyError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--batch-messages", type=int, default=0,
                    help="cut each sender's traffic into batches of N messages (0: one batch)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    G, W = a.groups, a.threads
    nv = sum(r != OBSERVER for r in ROLES)
    g, m = groups_and_members(G)
    cids = g["cluster_id"].copy()
    nm = len(ROLES)
    pin = hq.Context(a.device)
    bounds = [G * i // W for i in range(W + 1)]

    def worker(lo, hi):
        w = hq.Worker(a.device, nv, on_device=True)
        w.add_groups(g[lo:hi], m[nm * lo:nm * hi])
        return w

    arr = Arrivals(pin, cids, a.batch_messages)
    parts = [Arrivals(pin, cids[bounds[i]:bounds[i + 1]], a.batch_messages) for i in range(W)]
    # host, one thread
    w1, wire1 = worker(0, G), hq.Wire(DEP)
    wire1.attach(w1)
    data1 = pin.pinned(arr.n_messages * 6 + len(arr.lev) * 24 + 4096, np.uint8)
    sizes1 = pin.pinned(G, np.uint16)
    # host, W threads
    wk = [worker(bounds[i], bounds[i + 1]) for i in range(W)]
    wires = [hq.Wire(DEP) for _ in range(W)]
    for x, y in zip(wires, wk):
        x.attach(y)
    bufs = [(pin.pinned(p.n_messages * 6 + len(p.lev) * 24 + 4096, np.uint8),
             pin.pinned(len(p.cids), np.uint16)) for p in parts]
    pool = ThreadPoolExecutor(W)
    # device mode
    wd, wired = worker(0, G), hq.Wire(DEP)
    wired.attach_device(wd)
    wf, wiref = worker(0, G), hq.Wire(DEP)
    wiref.attach_device(wf)
    wiref.set_device_framing(True)

    t = {"host1": [], "host1_decode": [], "host16": [], "host16_decode": [], "device": [],
         "device_frame": [], "device_add_batch": [], "device_add_locals": [], "device_step": [],
         "device_step_gpu": [], "device_framed": [], "device_framed_add_batch": [],
         "device_framed_add_locals": [], "device_framed_step": [], "device_framed_step_gpu": []}
    frame_stats = None
    same = True
    for s in range(a.warmup + a.steps):
        arr.set(s)
        for p in parts:
            p.set(s)
        t0 = time.perf_counter()
        wire1.reset()
        arr.add_to(wire1)
        ss, st1 = wire1.step_sized(data1, sizes1)
        t1 = time.perf_counter()
        r1 = w1.step_sized(*ss, copy=False)
        t2 = time.perf_counter()
        c1 = counts(r1)

        def decode(i):
            wires[i].reset()
            parts[i].add_to(wires[i])
            return wires[i].step_sized(*bufs[i])[0]

        t3 = time.perf_counter()
        streams = list(pool.map(decode, range(W)))
        t4 = time.perf_counter()
        jobs = hq.StepJobs(list(zip(wk, streams)))
        jobs.execute()
        t5 = time.perf_counter()
        c16 = tuple(map(sum, zip(*(counts(r) for r in jobs.results(copy=False)))))

        t6 = time.perf_counter()
        wired.reset()
        arr.add_batches_to(wired)
        t6b = time.perf_counter()
        wired.add_locals(arr.cids, arr.loff, arr.lev)
        t7 = time.perf_counter()
        rd, std = wired.step_device(copy=False)
        t8 = time.perf_counter()
        cd = counts(rd)
        gpu_d = rd["gpu_ns"] * 1e-9

        t9 = time.perf_counter()
        wiref.reset()
        arr.add_batches_to(wiref)
        t9b = time.perf_counter()
        wiref.add_locals(arr.cids, arr.loff, arr.lev)
        t10 = time.perf_counter()
        rf, stf = wiref.step_device(copy=False)
        t11 = time.perf_counter()
        cf = counts(rf)
        frame_stats = wiref.device_frame_stats()
        same = same and c1 == c16 == cd == cf and c1[2] == 0 and \
            all(getattr(st1, k) == getattr(std, k) == getattr(stf, k)
                for k, _ in hq.WireStats._fields_)
        if s >= a.warmup:
            t["host1"].append(t2 - t0)
            t["host1_decode"].append(t1 - t0)
            t["host16"].append(t5 - t3)
            t["host16_decode"].append(t4 - t3)
            t["device"].append(t8 - t6)
            t["device_frame"].append(t7 - t6)
            t["device_add_batch"].append(t6b - t6)
            t["device_add_locals"].append(t7 - t6b)
            t["device_step"].append(t8 - t7)
            t["device_step_gpu"].append(gpu_d)
            t["device_framed"].append(t11 - t9)
            t["device_framed_add_batch"].append(t9b - t9)
            t["device_framed_add_locals"].append(t10 - t9b)
            t["device_framed_step"].append(t11 - t10)
            t["device_framed_step_gpu"].append(rf["gpu_ns"] * 1e-9)
    n_spans = -(-arr.n_messages // 64)            # (an estimate from below: spans also end at 4 KiB)
    ms = lambda v: {"median": float(np.median(v)) * 1e3, "worst": float(np.max(v)) * 1e3}
    link = link_read_gbps(a.device)
    rec = {"tool": "wire_dev_probe", "groups": G, "steps": a.steps, "warmup": a.warmup,
           "messages_per_step": arr.n_messages, "local_events_per_step": len(arr.lev),
           "message_bytes_per_step": arr.n_bytes, "batch_messages": a.batch_messages,
           "batches_per_step": len(arr.batches),
           "frame_stats_last_step": dict(zip(("segments", "void_segments", "open_batches",
                                              "steps_framed_on_host"), frame_stats or ())),
           "bytes_per_message": arr.n_bytes / arr.n_messages,
           "span_index_bytes_per_step_min": n_spans * hq.WIRE_SPAN_DTYPE.itemsize,
           "commits_ready_fallback_last_step": c1, "paths_agree": bool(same),
           "ms_per_step": {k: ms(v) for k, v in t.items()},
           "link_read_GBps": link,
           "link_bound_ms": arr.n_bytes / (link * 1e9) * 1e3 if link else None}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    pool.shutdown()
    for x in [wire1, wired, wiref] + wires + [w1, wd, wf] + wk:
        x.close()
    pin.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
