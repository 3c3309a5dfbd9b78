#!/usr/bin/env python3
"""The leader heartbeats of a device worker marshalled on the device (hq_worker_heartbeat_batches)
against the host chain they replace, in one process on one GPU.

The state is tools/heartbeat_probe.py's: G leader groups of 7 members after --steps steps, member 2
of every 8th group behind, every 16th group's ReadIndex ctx pending. Routes: member index mod
--dests. For each --batch-messages value, after --warmup calls:
  device      --reps calls of hq_worker_heartbeat_batches over every handle: wall time, the GPU
              time between the HIP events around its kernels (gpu_ns), n_bytes, n_messages
  host chain  --host-reps runs, on this one thread, of hq_worker_heartbeats, hq_heartbeats_expand
              (the caller's columns built once, outside the timing), the split per destination
              (a stable sort of the messages by route), and hq_wire_encode_batch per batch into one
              preallocated buffer
The two must give the same bytes; the probe fails otherwise. The link yardstick is n_bytes over
--link-gbps (what tools/link_probe reads on the box for device-to-host writes; not measured here).
Output: one JSON line per batch_messages value, and --out FILE.
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

from dragonboat_amd import hipquorum as hq  # noqa: E402
import heartbeat_probe as hp  # noqa: E402

DEPLOYMENT, SOURCE = 0x5EED, b"10.0.0.1:63001"


def host_chain(w, cols, routes, frm, n_dest, bm, out):
    """hq_worker_heartbeats -> expand -> split -> encode; returns (bytes view of out, batches)."""
    hb = w.heartbeats(copy=False)
    msgs = hq.heartbeats_expand(hb, *cols)
    bits = ((hb["words"][:, None] >> np.arange(16, dtype=np.uint32)) & 1).astype(bool)
    dest = routes[bits]                                   # group order, then member order
    keep = dest != hq.HQ_ROUTE_NONE
    order = np.argsort(dest[keep], kind="stable")
    rows = hq.heartbeat_wire_messages(msgs[keep][order], frm)
    ends = np.searchsorted(dest[keep][order], np.arange(n_dest), side="right")
    at, first, table = 0, 0, []
    for d in range(n_dest):
        end = int(ends[d])
        while first < end:
            cnt = min(bm or end - first, end - first)
            b = hq.encode_wire_batch(rows[first:first + cnt], DEPLOYMENT, SOURCE, out=out[at:])
            table.append((at, len(b), d, cnt))
            at += len(b)
            first += cnt
    return out[:at], np.array(table, hq.HEARTBEAT_BATCH_DTYPE)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--dests", type=int, default=7)
    ap.add_argument("--batch-messages", type=int, nargs="+", default=[0, 4096])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--link-gbps", type=float, default=57.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    G = a.groups
    assert G % 16 == 0 and a.steps >= 2

    w = hq.Worker(0, 8, on_device=True)
    g, m = hp.groups_and_members(G)
    w.add_groups(g, m)
    for s in range(a.steps):
        res = w.step(*hp.step_rows(G, s, s == a.steps - 1), copy=False)
        assert len(res["fallback_groups"]) == 0
    del res
    routes = np.tile(np.arange(16, dtype=np.uint16) % a.dests, (G, 1))
    routes[:, len(hp.ROLES):] = hq.HQ_ROUTE_NONE
    w.set_heartbeat_routes(0, routes)
    # what the caller of the host chain holds: ids, terms, the committed indices its commits told it
    ids = np.zeros((G, 16), np.uint64)
    ids[:, :len(hp.ROLES)] = np.arange(1, len(hp.ROLES) + 1, dtype=np.uint64)
    cols = (g["cluster_id"].copy(), np.full(G, hp.TERM, np.uint64),
            np.full(G, hp.LAST0 + a.steps - 1, np.uint64), np.full(G, len(hp.ROLES), np.uint32), ids)

    lines = []
    out = None
    for bm in a.batch_messages:
        for _ in range(a.warmup):
            got = w.heartbeat_batches(None, DEPLOYMENT, SOURCE, a.dests, bm, copy=False)
        wall, gpu = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter_ns()
            got = w.heartbeat_batches(None, DEPLOYMENT, SOURCE, a.dests, bm, copy=False)
            wall.append(time.perf_counter_ns() - t0)
            gpu.append(got["gpu_ns"])
        n_bytes, n_messages = len(got["bytes"]), int(got["n_messages"])
        if out is None:
            out = np.empty(n_bytes + (1 << 20), np.uint8)
        chain = []
        for i in range(a.host_reps + 1):
            t0 = time.perf_counter_ns()
            data, table = host_chain(w, cols, routes, 1, a.dests, bm, out)
            if i:                                        # (the first one warms the buffers up)
                chain.append(time.perf_counter_ns() - t0)
        np.testing.assert_array_equal(table, got["batches"])
        assert len(data) == n_bytes and np.array_equal(data, got["bytes"]), "device and host bytes differ"
        dev_wall, dev_gpu, host = hp.stats(wall), hp.stats(gpu), hp.stats(chain)
        link_us = n_bytes / (a.link_gbps * 1e3)
        lines.append({
            "probe": "heartbeat_wire", "groups": G, "steps": a.steps, "dests": a.dests,
            "batch_messages": bm, "n_messages": n_messages, "n_unrouted": int(got["n_unrouted"]),
            "n_bytes": n_bytes, "n_batches": len(got["batches"]),
            "device_wall": dev_wall, "device_gpu": dev_gpu, "host_chain_one_thread": host,
            "link_gbps_assumed": a.link_gbps, "link_yardstick_us": link_us,
            "gpu_over_link": dev_gpu["median_us"] / link_us,
            "host_chain_over_device_wall": host["median_us"] / dev_wall["median_us"],
            "bytes_equal": True, "note": "measured once, one box",
        })
        print(json.dumps(lines[-1]), flush=True)
    w.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
