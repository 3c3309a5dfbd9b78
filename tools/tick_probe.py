#!/usr/bin/env python3
"""One tick of every group of a device worker (hq_worker_tick) beside the leader heartbeat
broadcast over the same groups (hq_worker_heartbeats), whose kernel reads the same group records
plus members and reads and is the yardstick. One process, one GPU.

The state is heartbeat_probe.py's (step5's membership): G leader groups of 7 members after --steps
steps. The tick config is election_rtt 10, heartbeat_rtt 1, check_quorum on, so every tick lists
every group in `heartbeat`, the tenth tick lists every group in `check_quorum` too, and `election`
stays empty (no follower); --contact N adds a contact list of N handles (all leaders here: the
bitmap is built, uploaded and read, and changes nothing).

Printed per tick, one JSON line: gpu_ns (the HIP events around the call's kernels), the wall time
of the call, the three list sizes, and the bytes the kernels must move: per group the two 16-byte
quads of the group record that hold term | state, flags (the cluster id's quad too in a tick that
resets the timer: the first), the 16-byte timer read and written; per wave of 64 groups 32 bytes
of ballots written and read again; per tile of 256 groups 16 bytes of counts and 16 of bases,
written and read; the contact bitmap; and 4 bytes per listed handle written to pinned host memory.
Then --reps heartbeats calls over all groups on the same state, and a summary line with the
medians and the tick's fraction of the 8 TB/s HBM peak. Output: JSON lines, the summary to --out.
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
from heartbeat_probe import groups_and_members, stats, step_rows  # noqa: E402

E_RTT, H_RTT, SEED = 10, 1, 0x71C4
HBM_PEAK = 8e12
TILE = 256


def tick_bytes(G, reset, n_contact, sizes):
    """(device bytes, host bytes) one tick must move."""
    waves, tiles = -(-G // 64), -(-G // TILE)
    dev = G * (32 + (16 if reset else 0) + 16 + 16) + waves * 32 * 2 + tiles * 16 * 4
    dev += 2 * 4 * (-(-G // 32)) if n_contact else 0       # the bitmap copied in, then read
    return dev, 4 * sum(sizes) + 32


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=24)
    ap.add_argument("--contact", type=int, default=0)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out")
    a = ap.parse_args()
    G = a.groups
    assert G % 16 == 0 and a.steps >= 2 and a.ticks > E_RTT

    w = hq.Worker(0, 8, on_device=True)
    w.add_groups(*groups_and_members(G))
    for s in range(a.steps):
        res = w.step(*step_rows(G, s, s == a.steps - 1), copy=False)
        assert len(res["fallback_groups"]) == 0
    del res
    w.set_tick_config(E_RTT, H_RTT, True, SEED)
    contact = np.arange(0, G, max(1, G // a.contact), dtype=np.uint32)[:a.contact] if a.contact else None
    everyone = np.arange(G, dtype=np.uint32)

    ticks = []
    for k in range(1, a.ticks + 1):
        t0 = time.perf_counter_ns()
        r = w.tick(contact, copy=False)
        wall = time.perf_counter_ns() - t0
        sizes = [len(r["check_quorum"]), len(r["heartbeat"]), len(r["election"])]
        assert sizes == [G if k % E_RTT == 0 else 0, G, 0] and r["n_ticked"] == G, (k, sizes)
        np.testing.assert_array_equal(r["heartbeat"], everyone)
        if k % E_RTT == 0:
            np.testing.assert_array_equal(r["check_quorum"], everyone)
        dev, host = tick_bytes(G, k == 1, a.contact, sizes)
        row = {"tick": k, "gpu_ns": int(r["gpu_ns"]), "wall_ns": wall, "n_check_quorum": sizes[0],
               "n_heartbeat": sizes[1], "n_election": sizes[2], "device_bytes": dev, "host_bytes": host}
        print(json.dumps(row))
        ticks.append(row)
    t = w.get_timers(np.array([0, G - 1], np.uint32))
    assert t["election_tick"].tolist() == [a.ticks % E_RTT] * 2 and t["heartbeat_tick"].tolist() == [0, 0]

    wall, gpu = [], []
    for i in range(a.reps + 3):
        t0 = time.perf_counter_ns()
        hb = w.heartbeats(copy=False)
        if i >= 3:                                       # (the first calls size the buffers)
            wall.append(time.perf_counter_ns() - t0)
            gpu.append(hb["gpu_ns"])
    assert w.readback_count() == 0
    w.close()

    # the first ticks size the buffers and reset every timer: the steady ticks are those after
    # them, with (every tenth) and without the CheckQuorum list
    steady = [r for r in ticks if r["tick"] > 2]
    plain = [r for r in steady if not r["n_check_quorum"]]
    both = [r for r in steady if r["n_check_quorum"]]
    tick_gpu = stats([r["gpu_ns"] for r in plain])
    out = {
        "probe": "tick", "groups": G, "steps": a.steps, "ticks": a.ticks, "contact": a.contact,
        "election_rtt": E_RTT, "heartbeat_rtt": H_RTT,
        "tick_gpu": tick_gpu, "tick_wall": stats([r["wall_ns"] for r in plain]),
        "tick_gpu_with_check_quorum": stats([r["gpu_ns"] for r in both]),
        "tick_wall_with_check_quorum": stats([r["wall_ns"] for r in both]),
        "first_tick_gpu_us": ticks[0]["gpu_ns"] / 1e3,
        "device_bytes": plain[0]["device_bytes"], "host_bytes": plain[0]["host_bytes"],
        "host_bytes_with_check_quorum": both[0]["host_bytes"],
        "device_GBps_over_gpu_time": plain[0]["device_bytes"] / (tick_gpu["median_us"] * 1e3),
        "fraction_of_hbm_peak": plain[0]["device_bytes"] / (tick_gpu["median_us"] * 1e-6) / HBM_PEAK,
        "host_GBps_over_gpu_time": plain[0]["host_bytes"] / (tick_gpu["median_us"] * 1e3),
        "heartbeats_gpu": stats(gpu), "heartbeats_wall": stats(wall),
        "tick_over_heartbeats_gpu": tick_gpu["median_us"] / stats(gpu)["median_us"],
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
