"""The device modules' buffers regrown on a live worker (dragonboat_amd/csrc/hq_sidecar.h).

Two arrays keep contents across calls and must carry them into a larger block: the timers of
hq_tick.hip and the pending-contact bitmap of hq_hb_received.hip. Their headroom is 1.5x, so the
lifecycle tests (10 groups, one added) never leave it. Here 40 started groups give a timer
capacity of 60 and a bitmap of 2 words with capacity 3 (96 handles); 200 handles need 7 words and
200 timers, 1000 handles 32 words (over the 10 that 7 grew to) and 1000 timers (over 300). Timers
are set and contacts marked before each growth, with no tick in between, and must be found after
it: by get_timers, and by the next tick's lists against tick_model and the host-worker twin.

The other buffers hold one call's data: they are grown by the same calls at 40 and then 1000 listed
groups, every result compared with the host-worker twin's."""
import numpy as np
import pytest

import config_ref as ref
import heartbeat_wire_ref as hwr
import lifecycle_model as lm
import step_scenarios as sc
from test_gpu_hb_received import E, Sim, spec

pytestmark = pytest.mark.gpu
KINDS = ["device", "host"]
STATES = [sc.FOLLOWER, sc.LEADER, sc.FOLLOWER, sc.CANDIDATE]      # of handle h: STATES[h % 4]
assert E == 4       # (the timers below are written for it: timeouts 4 .. 7, counters below 8)


def specs_of(h0, h1):
    return [spec(3000 + h, STATES[h % 4]) for h in range(h0, h1)]


def start_more(hq, sim, total):
    """start_groups up to `total` handles on every worker; the table follows."""
    h0 = len(sim.table)
    new = specs_of(h0, total)
    g, m = lm.group_arrays(hq, new)
    for w in sim.workers.values():
        assert w.start_groups(g, m).tolist() == list(range(h0, total))
    sim.table += [sim.entry(s) for s in new]


def set_timers(hq, sim, timers):
    """{handle: (election_tick, heartbeat_tick, randomized_timeout)} on every worker and the model."""
    hs = np.array(sorted(timers), np.uint32)
    ts = np.array([timers[int(h)] + (0,) for h in hs], hq.TIMER_DTYPE)
    groups = sim.tick_groups()
    for w in sim.workers.values():
        w.set_timers(hs, ts)
    for h, t in timers.items():
        sim.model.set(h, groups[h], *t)
        sim.pending.discard(h)


def mark(sim, heard, unheard):
    """Received heartbeats: `heard` followers get their leader's (term 3: a contact), `unheard`
    ones a deposed leader's (term 2: none)."""
    hs = list(heard) + list(unheard)
    sim.received(hs, [[(2, 3, 12, 0, 0)]] * len(heard) + [[(2, 2, 12, 0, 0)]] * len(unheard))
    assert sim.pending >= set(heard) and not sim.pending & set(unheard)


@pytest.mark.parametrize("kind", KINDS)
def test_timers_and_contacts_survive_two_regrows(hq, kind):
    sim = Sim(hq, kind, specs_of(0, 40), start=True)
    try:
        # followers one tick before their timeout, in both bitmap words: 2 and 34 will be in
        # contact, 6 and 36 not; a leader one tick before both limits; counters a reset would lose
        set_timers(hq, sim, {2: (6, 0, 7), 6: (6, 0, 7), 34: (5, 0, 6), 36: (5, 0, 6), 1: (3, 1, 0),
                             37: (2, 0, 0), 39: (1, 0, 5)})
        mark(sim, heard=[0, 2, 34, 38], unheard=[4, 36])
        start_more(hq, sim, 200)                      # (no tick in between)
        sim.check_timers()                            # the old ones as set, the new ones fresh
        for w in sim.workers.values():
            got = w.get_timers(np.array([6, 36, 1, 37, 39, 2], np.uint32))
            assert got["election_tick"].tolist() == [6, 5, 3, 2, 1, 0]     # (2: a pending contact)
            assert got["randomized_timeout"].tolist()[:2] == [7, 6]
        cq, hb, el, ticked = sim.tick()
        assert ticked == 200 and {6, 36} <= set(el) and not {0, 2, 34, 38} & set(el)
        assert 1 in cq and 1 in hb and 37 not in cq
        # honoured once: the contacts are consumed, the followers count on from 1
        sim.tick()
        groups = sim.tick_groups()
        assert [sim.model.get(h, groups[h])[0] for h in (0, 2, 34, 38)] == [2, 2, 2, 2]

        # again, over handles of the first growth too
        set_timers(hq, sim, {150: (6, 0, 7), 154: (6, 0, 7), 198: (5, 0, 6), 2: (6, 0, 7), 41: (3, 1, 0)})
        mark(sim, heard=[150, 198, 2, 64, 96], unheard=[154, 100])
        start_more(hq, sim, 1000)
        sim.check_timers()
        cq, hb, el, ticked = sim.tick()
        assert ticked == 1000 and 154 in el and not {150, 198, 2, 64, 96} & set(el)
        assert 41 in cq and 41 in hb
        sim.tick()
        groups = sim.tick_groups()
        assert [sim.model.get(h, groups[h])[0] for h in (150, 198, 2)] == [2, 2, 2]
        sim.check_state()
    finally:
        sim.close()


def test_per_call_buffers_grow_with_the_listed_groups(hq):
    """heartbeats, heartbeat_batches, get_groups and config_changes of one device worker at 40 and
    then at 1000 listed groups, each against the host-worker twin."""
    sim = Sim(hq, "device", specs_of(0, 40), start=True)
    dev, twin = sim.workers["device"], sim.workers["twin"]
    rng = np.random.default_rng(40)
    try:
        for total, node in ((40, 500), (1000, 501)):
            if total > len(sim.table):
                start_more(hq, sim, total)
            routes = hwr.random_routes(rng, total, 5)
            for w in (dev, twin):
                w.set_heartbeat_routes(0, routes)
            a, b = dev.heartbeats(), twin.heartbeats()
            for k in ("words", "lags", "ctxs"):
                assert a[k].tobytes() == b[k].tobytes(), (total, k)
            assert a["n_messages"] == b["n_messages"] > 0
            a, b = (w.heartbeat_batches(None, 7, b"node-1:9", 5, 16) for w in (dev, twin))
            for k in ("bytes", "batches"):
                assert a[k].tobytes() == b[k].tobytes(), (total, k)
            assert (a["n_messages"], a["n_unrouted"]) == (b["n_messages"], b["n_unrouted"])
            everyone = list(range(total))
            assert lm.snapshot(dev, everyone) == lm.snapshot(twin, everyone), total
            changes = [(h, ref.ADD_NODE, node) for h in everyone]
            a, b = dev.config_changes(changes), twin.config_changes(changes)
            for k in ("status", "commits"):
                assert a[k].tobytes() == b[k].tobytes(), (total, k)
            assert a["n_applied"] == b["n_applied"] == total
            assert lm.snapshot(dev, everyone) == lm.snapshot(twin, everyone), total
        assert dev.readback_count() == 0
    finally:
        sim.close()
