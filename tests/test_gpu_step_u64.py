"""Whole step worlds at large values: the worlds of tests/step_shift.py (the small random and
consecutive-run worlds of tests/step_random.py translated to 2^16, 2^31 / 2^32, 2^63 and the top of
the u64 range) through the step worker, against the oracle's results on the same shifted groups and
events (step_shift.reference, computed once per world and held to the small world's results by
tests/test_step_shift.py). Everything is bit-exact: every stepped group's lists, no fallback, every
group's state after every step."""
import numpy as np
import pytest

import step_scenarios as sc
import step_shift as ss
from step_harness import WorkerBackend, same_step

pytestmark = pytest.mark.gpu

# (on_device, stream) of WorkerBackend
RANDOM_FEEDS = [(True, False), (True, True), (True, "sized16-slots"), (False, "sized16")]
RANDOM_IDS = ["device", "device-stream", "device-sized16-slots", "host-sized16"]
RUNS_FEEDS = [(True, True), (True, "sized16"), (True, "sized16-slots"), (False, True)]
RUNS_IDS = ["device-stream", "device-sized16", "device-sized16-slots", "host-stream"]


def run_world(w, ref, after_step=None):
    """ref's groups and steps through backend w; returns the output counts (from w's results)."""
    for g in ref.groups:
        w.add_group(*g)
    seen = dict(ready=0, resps=0, states=0, dropped=0, deferred=0, commit=0)
    for s, (per, want, states) in enumerate(ref.steps):
        got = w.step(per)
        assert got["_fallback"] == [], s
        for cid in per:
            same_step(want, got, cid)
            ss.count_seen(seen, got[cid])
        for cid, st in states.items():
            assert w.state(cid) == st, (s, cid)
        if after_step:
            after_step(s, per, want)
    return seen


@pytest.mark.parametrize("feed", RANDOM_FEEDS, ids=RANDOM_IDS)
@pytest.mark.parametrize("world", ss.SHIFTED)
def test_random_world(hq, world, feed):
    """test_random_differential's world (witnesses, observers, non-members, stale / zero / higher
    terms, several ReadIndex ctxs, campaigns, CheckQuorum, proposals) shifted: device rows, device
    stream, the slot feed and the host worker on 2-byte size words; every output kind seen, with
    the counts the small world gives."""
    ref = ss.reference("random", world)
    w = WorkerBackend(hq, n_max=8, seed=1, on_device=feed[0], stream=feed[1])
    try:
        seen = run_world(w, ref)
        print(f"random {world} {feed}: {ref.n_events} events, seen {seen}")
        assert (ref.n_events, seen) == (ss.RANDOM_EVENTS, ss.RANDOM_SEEN)
    finally:
        w.close()


def _wire_backends():
    from test_gpu_wire_dev import DeviceWireBackend
    from test_gpu_wire_frame_dev import FramedWireBackend

    return {"device-wire": DeviceWireBackend, "framed-wire": FramedWireBackend}


@pytest.mark.parametrize("backend", ["device-wire", "framed-wire"])
@pytest.mark.parametrize("world", ["u63", "top"])
def test_random_world_from_wire_bytes(hq, world, backend):
    """The same world as raftpb.MessageBatch bytes decoded (and framed) on the device: cluster ids
    at the top of the range through the device hash table and the key sort, 10-byte varints
    through the device decoder; the backends' own stats assertions hold."""
    ref = ss.reference("random", world)
    w = _wire_backends()[backend](hq, n_max=8, seed=1)

    def stats(s, per, want):
        st = w.last_stats
        assert st.dropped_batches == 1 and st.batches >= 2, s

    try:
        seen = run_world(w, ref, stats)
        print(f"random {world} {backend}: seen {seen}")
        assert seen == ss.RANDOM_SEEN
        assert w.in_place == len(ref.steps) and w.staged >= 2 * len(ref.steps)
    finally:
        w.close()


def _count_run_headers(hq, w, totals):
    """Wraps w.build_inputs: totals += (consecutive-form, listed) run headers of each step's
    stream, found by walking its events."""
    build = w.build_inputs

    def counting(per):
        arrs, refs = build(per)
        if isinstance(arrs, hq.SizedStream):
            sizes, data = arrs[1], arrs[3]
            nb = sizes if sizes.dtype == np.uint16 else sizes >> np.uint32(16)
            boff = np.concatenate([[0], np.cumsum(nb.astype(np.uint64))]).astype(np.uint64)
        else:
            boff, data = arrs[2], arrs[3]
        seq, listed = ss.run_headers(np.asarray(data)[:int(boff[-1])], boff)
        totals[0] += seq
        totals[1] += listed
        return arrs, refs

    w.build_inputs = counting


@pytest.mark.parametrize("feed", RUNS_FEEDS, ids=RUNS_IDS)
@pytest.mark.parametrize("world", ss.SHIFTED)
def test_runs_world(hq, world, feed):
    """Runs of acks from consecutive node ids that cross 2^16 / 2^32 / 2^63 or end at node
    2^64 - 1. The consecutive form (the device's take_run) holds 32-bit senders only: the u16
    world's streams carry it, and the top world's for the small senders past the members; in the
    u32 and u63 worlds every run of three ends at or above 2^32 - 1, so their runs list their
    senders and the form must not appear at all."""
    ref = ss.reference("runs", world)
    w = WorkerBackend(hq, n_max=8, seed=31, on_device=feed[0], stream=feed[1])
    headers = [0, 0]
    _count_run_headers(hq, w, headers)
    try:
        seen = run_world(w, ref)
        print(f"runs {world} {feed}: {ref.n_events} events, seen {seen}, run headers "
              f"(consecutive, listed) {headers}")
        assert all(v > 0 for k, v in seen.items() if k != "resps"), seen
        assert ref.n_events > 20000 and headers[1] > 0
        assert headers[0] > 0 if world in ("u16", "top") else headers[0] == 0, headers
    finally:
        w.close()


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_wrapped_run_header_on_the_worker(hq, on_device):
    """step_shift.wrapped_run_stream (a consecutive-form header whose first sender + count wraps
    to 0 in 64 bits) as group 1's stream: the host worker rejects the step as malformed; the
    device worker suspends the group at the header's first event, the ReplicateResp before it
    taken and the other group unaffected."""
    w = hq.Worker(0, 4, on_device=on_device)
    try:
        for cid in (1, 2):
            w.add_group(cid, 1, 2, sc.LEADER, 5, 6, 5, [(1, 6, 0, 0), (2, 5, 0, 0), (3, 5, 0, 0)])
        one = np.array([(hq.EV_MESSAGE, sc.RREP, 2, 2, 6, 0, 0, 0, 0)], hq.EVENT_DTYPE)
        tail, _ = hq.encode_events(np.array([0, 1], np.uint64), one)
        bad = ss.wrapped_run_stream()
        data = np.concatenate([bad, tail])
        off = np.array([0, 4, 5], np.uint64)
        boff = np.array([0, len(bad), len(data)], np.uint64)
        grp = np.array([w.find(1), w.find(2)], np.uint32)
        if not on_device:
            with pytest.raises(hq.HQError, match="malformed"):
                w.step_stream(grp, off, boff, data)
            assert w.get_group(1)[0]["committed"] == 5 and w.get_group(2)[0]["committed"] == 5
            return
        res = w.step_stream(grp, off, boff, data)
        assert list(res["fallback_groups"]) == [1] and list(res["deferred"]) == [1, 2, 3]
        assert w.get_group(2)[0]["committed"] == 6       # the other group is unaffected
        g1, m1, _ = w.get_group(1)                        # its first ack was taken
        assert g1["committed"] == 6 and g1["suspended"] == 1
        assert sorted((int(m["node_id"]), int(m["match"])) for m in m1) == [(1, 6), (2, 6), (3, 5)]
    finally:
        w.close()


def test_narrow_columns_straddle_2_32(hq):
    """The u32 runs world on the slot feed (commits as 4-byte advances, ReadyToReads compact: an
    int32 delta from the committed index before the step): committed indexes and ReadyToRead
    indexes lie on both sides of 2^32, some advances cross it, and the steps counted here did
    return the narrow forms, so those are what the comparison with the oracle tested. (The runs
    world: a step returns the advance column only when more than a quarter of its listed groups
    commit, which no step of the random world does and the runs world's first step does.)"""
    ref = ss.reference("runs", "u32")
    w = WorkerBackend(hq, n_max=8, seed=31, on_device=True, stream="sized16-slots")
    lim = 2**32
    before = {g[0]: g[4] for g in ref.groups}
    tally = dict(advance_steps=0, compact_steps=0, narrow_steps=0, crossing=0, commit_below=0,
                 commit_above=0, ready_below=0, ready_above=0)

    def columns(s, per, want):
        res = w.last_raw
        narrow = "committed_advance" in res and "ready_compact" in res
        tally["narrow_steps"] += narrow
        tally["advance_steps"] += "committed_advance" in res
        tally["compact_steps"] += "ready_compact" in res
        for cid in per:
            o = want[cid]
            if narrow and o["commit_changed"]:
                tally["crossing"] += before[cid] < lim <= o["committed"]
                tally["commit_below"] += o["committed"] < lim
                tally["commit_above"] += o["committed"] >= lim
            if narrow:
                tally["ready_below"] += sum(i < lim for i, _, _ in o["ready"])
                tally["ready_above"] += sum(i >= lim for i, _, _ in o["ready"])
            before[cid] = o["committed"]

    try:
        run_world(w, ref, columns)
        print(f"u32 narrow columns: {tally}")
        assert all(v > 0 for v in tally.values()), tally
    finally:
        w.close()
