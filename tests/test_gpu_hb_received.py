"""The follower side of heartbeats on the step worker (hq_worker_heartbeats_received:
hq_worker_hbrecv.cpp, hq_hb_received.hip; the contacts' way into hq_worker_tick: hq_tick.hip).
Expected values come from hb_received_model (and tick_model for the timers) over a table the test
keeps itself, or over the CPU oracle's state in the random worlds; device workers are additionally
held byte-equal to a host-worker twin. No device worker may read its state back. The seeds are
shown to reach every branch on the models alone in test_hb_received_api.py."""
import ctypes

import numpy as np
import pytest

import hb_received_model as hm
import hb_received_world as hw
import lifecycle_model as lm
import step_scenarios as sc
import tick_model as tm
from step_harness import event_record

pytestmark = pytest.mark.gpu
KINDS = ["device", "host"]
SEED = 0xBEA7
E, H = 4, 2
U64 = (1 << 64) - 1


def make_workers(hq, kind):
    if kind == "device":
        return {"device": hq.Worker(0, 8, on_device=True), "twin": hq.Worker(0, 8)}
    return {"host": hq.Worker(0, 8)}


def spec(cid, state, term=3, last=20, committed=10, n=3, node=1):
    """A group of n remotes (ids 1 .. n) in `state`; a leader's followers are at `committed`."""
    mem = [(i, last if i == node else (committed if state == sc.LEADER else 0), sc.REMOTE, 1)
           for i in range(1, n + 1)]
    return (cid, node, term, state, committed, last, committed, mem, None)


class Sim:
    """The workers of one kind, the test's own table of their groups (by handle) and a TickModel."""

    def __init__(self, hq, kind, specs, cq=True, config=True, start=False):
        self.hq, self.cq = hq, cq
        self.workers = make_workers(hq, kind)
        self.table = []
        self.model = tm.TickModel(E, H, cq, SEED)
        self.pending = set()
        self.seen = hm.Seen()
        g, m = lm.group_arrays(hq, specs)
        for w in self.workers.values():
            if start:
                assert w.start_groups(g, m).tolist() == list(range(len(specs)))
            else:
                w.add_groups(g, m)
            if config:
                w.set_tick_config(E, H, cq, SEED)
        for s in specs:
            self.table.append(self.entry(s))

    @staticmethod
    def entry(s):
        return {"cid": s[0], "node": s[1], "term": s[2], "state": s[3], "committed": s[4], "last": s[5],
                "suspended": False, "members": {m[0]: [m[1], m[2], m[3]] for m in s[7]}, "votes": None,
                "reads": 0}

    def close(self):
        for w in self.workers.values():
            w.close()

    def tick_groups(self):
        return [None if t is None else (t["cid"], t["term"], t["state"], t["suspended"]) for t in self.table]

    def received(self, handles, rows, cq=None):
        """One call on the model and every worker. Returns the workers' results by name."""
        cq = self.cq if cq is None else cq
        want_replies, want_results = [], []
        for h, msgs in zip(handles, rows):
            t = self.table[h]
            g = t if t is not None else {"term": 0, "state": 0, "committed": 0, "last": 0, "suspended": True}
            replies, res, after = hm.handle(g, msgs, cq)
            self.seen.add(g, replies, res)
            want_replies += replies
            want_results.append(res)
            if t is None:
                continue
            t.update(term=after["term"], state=after["state"], committed=after["committed"])
            if after["reset"]:
                for i, m in t["members"].items():
                    m[0], m[2] = (t["last"] if i == t["node"] else 0), 0
                t["votes"], t["reads"] = (0, 0), 0
            if res["flags"] & hm.CONTACT:
                self.pending.add(h)
        groups = np.array(handles, np.uint32)
        offsets = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
        msgs = np.array([m for r in rows for m in r], self.hq.HB_RECEIVED_DTYPE)
        got = {}
        for name, w in self.workers.items():
            got[name] = w.heartbeats_received(groups, offsets, msgs, cq)
            hw.check_output(got[name], want_replies, want_results, name)
            assert (got[name]["gpu_ns"] > 0) == (name == "device") or not len(groups), name
        if "twin" in got:
            for k in ("replies", "results"):
                assert got["device"][k].tobytes() == got["twin"][k].tobytes(), k
        return got

    def tick(self, contact=()):
        want = self.model.tick(self.tick_groups(), list(contact) + sorted(self.pending))
        self.pending.clear()
        got = {}
        for name, w in self.workers.items():
            got[name] = w.tick(np.array(contact, np.uint32) if len(contact) else None)
            tm.check_tick(got[name], want)
        self.check_timers()
        if "twin" in got:
            for k in ("check_quorum", "heartbeat", "election"):
                assert got["device"][k].tobytes() == got["twin"][k].tobytes(), k
        return want

    def want_timer(self, h):
        t = self.model.get(h, self.tick_groups()[h])
        # (a pending contact is the next tick's leaderIsAvailable: election_tick 0 for a non-leader)
        return (0,) + t[1:] if h in self.pending and self.table[h]["state"] != sc.LEADER else t

    def check_timers(self):
        live = [h for h, t in enumerate(self.table) if t is not None]
        for name, w in self.workers.items():
            got = w.get_timers(np.array(live, np.uint32))
            have = list(zip(got["election_tick"].tolist(), got["heartbeat_tick"].tolist(),
                            got["randomized_timeout"].tolist()))
            assert have == [self.want_timer(h) for h in live], name

    def check_state(self):
        """hq_worker_get_groups of every live handle against the table; device against twin."""
        live = [h for h, t in enumerate(self.table) if t is not None]
        for name, w in self.workers.items():
            r = w.get_groups(np.array(live, np.uint32))
            for i, h in enumerate(live):
                t, g = self.table[h], r["groups"][i]
                assert (int(g["cluster_id"]), int(g["term"]), int(g["state"]), int(g["committed"]),
                        int(g["last_index"]), bool(g["suspended"]), int(g["n_pending_reads"])) == \
                    (t["cid"], t["term"], t["state"], t["committed"], t["last"], t["suspended"], t["reads"]), \
                    (name, h)
                mo = r["member_offsets"]
                mem = {int(m["node_id"]): [int(m["match"]), int(m["role"]), int(m["active"])]
                       for m in r["members"][int(mo[i]):int(mo[i + 1])]}
                assert mem == t["members"], (name, h)
                if t["votes"] is not None:
                    assert (int(r["granted"][i]), int(r["rejected"][i])) == t["votes"], (name, h)
            assert w.readback_count() == 0, name
        if "twin" in self.workers:
            assert lm.snapshot(self.workers["device"], live) == lm.snapshot(self.workers["twin"], live)


# ------------------------------------------------------------------ the edges ------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("G", hw.EDGE_SIZES)
def test_listed_group_edges(hq, G, kind):
    """G listed groups at the contact words' and the waves' edges, some without messages, the
    handles in descending order and then scattered (every third, the rest reversed)."""
    specs, rows = hw.edge_rows(G)
    sim = Sim(hq, kind, specs)
    try:
        order = list(range(G - 1, -1, -1))
        sim.received(order, [rows[h] for h in order])
        sim.check_state()
        sim.check_timers()
        sim.tick()
        rng = np.random.default_rng(G)
        scattered = list(range(0, G, 3)) + [h for h in range(G - 1, -1, -1) if h % 3]
        again = [hm.random_messages(rng, sim.table[h], members=list(sim.table[h]["members"]))
                 for h in scattered]
        sim.received(scattered, again)
        sim.check_state()
        sim.tick(contact=[h for h in range(G) if sim.table[h]["state"] != sc.LEADER][:5])
        sim.tick()
    finally:
        sim.close()


@pytest.mark.parametrize("kind", KINDS)
def test_all_in_contact_or_none(hq, kind):
    """65 followers: every one in contact at once (no election for E ticks more, all timers at 0),
    then none (lower-term heartbeats: a NoOP each with check_quorum, nothing without)."""
    G = 65
    sim = Sim(hq, kind, [spec(500 + j, sc.FOLLOWER) for j in range(G)])
    try:
        for _ in range(E - 1):
            sim.tick()
        everyone = list(range(G))
        got = sim.received(everyone, [[(2, 3, 12, 7, 9)]] * G)
        for r in got.values():
            assert (r["n_contact"], r["n_resp"], r["n_committed"], r["n_noop"]) == (G, G, G, 0)
        assert all(sim.want_timer(h)[0] == 0 for h in everyone)
        sim.check_timers()
        assert sim.tick()[2] == []                    # (everyone counts from 0 again)
        sim.check_state()
        for cq, noops in ((True, G), (False, 0)):
            got = sim.received(everyone, [[(2, 2, 15, 0, 0)]] * G, cq=cq)
            for r in got.values():
                assert (r["n_contact"], r["n_resp"], r["n_noop"], r["n_committed"]) == (0, 0, noops, 0)
        assert not sim.pending
        sim.check_state()
        due = []
        for _ in range(2 * E):
            due += sim.tick()[2]
        assert sorted(set(due)) == everyone
    finally:
        sim.close()


# ------------------------------------------------------------------ random worlds --------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cq", [1, 0])
@pytest.mark.parametrize("G", [17, 300])
def test_random_worlds(hq, G, cq, kind):
    """30 rounds of received heartbeats, a tick with a caller contact list for some other
    followers, a step with the tick's events, and heartbeats, on groups with witnesses and
    observers among their members; the whole state and the timers compared after every round. The
    election lists must differ from the same world's without the received call: the contacts
    reached the tick."""
    workers = make_workers(hq, kind)
    seen, elections = hw.run(hq, workers, {n: False for n in workers}, G, cq)   # (run closes the workers)
    seen.check(noop=bool(cq))
    _, without = hw.run(hq, {}, {}, G, cq, received=False)
    assert elections != without


# ------------------------------------------------------------------ the closed loop ------------
@pytest.mark.parametrize("follower_kind", KINDS)
def test_closed_loop_over_the_wire(hq, follower_kind):
    """A device leader worker's heartbeat batches, carrying a pending ReadIndex ctx, decoded and
    fed as rows to follower workers holding the same clusters on node ids 2 and 3; their replies
    expanded, encoded and added to a wire attached to the leader worker, whose step then releases
    the ReadyToRead of that ctx; the followers' committed = min(match, committed) as sent."""
    G, last, committed = 40, 30, 25
    cids = [700 + j for j in range(G)]
    match = {2: [committed - j % 4 for j in range(G)], 3: [last] * G}
    leader = hq.Worker(0, 8, on_device=True)
    followers = {n: make_workers(hq, follower_kind) for n in (2, 3)}
    wire = hq.Wire(0x5EED)
    try:
        specs = [(c, 1, 4, sc.LEADER, committed, last, committed,
                  [(1, last, sc.REMOTE, 1), (2, match[2][j], sc.REMOTE, 1), (3, match[3][j], sc.REMOTE, 1)], None)
                 for j, c in enumerate(cids)]
        leader.add_groups(*lm.group_arrays(hq, specs))
        for n, ws in followers.items():
            fs = [(c, n, 4, sc.FOLLOWER, 5, match[n][j], 5,
                   [(1, 0, sc.REMOTE, 0), (2, 0, sc.REMOTE, 0), (3, 0, sc.REMOTE, 0)], None)
                  for j, c in enumerate(cids)]
            for w in ws.values():
                w.add_groups(*lm.group_arrays(hq, fs))
        # a local ReadIndex per group: pending until a quorum of HeartbeatResps echoes its ctx
        ev = np.array([event_record(hq, ("read", 9000 + j, 77)) for j in range(G)], hq.EVENT_DTYPE)
        res = leader.step(np.arange(G, dtype=np.uint32), np.arange(G + 1, dtype=np.uint64), ev)
        assert len(res["ready"]) == 0
        leader.set_heartbeat_routes(0, np.tile(np.array([0xFFFF, 0, 1] + [0xFFFF] * 13, np.uint16), (G, 1)))
        hb = leader.heartbeat_batches(None, deployment_id=0x5EED, source=b"n1:1", n_dest=2)
        assert len(hb["batches"]) == 2
        wire.attach(leader)
        for b in hb["batches"]:
            data = hb["bytes"][int(b["offset"]):int(b["offset"]) + int(b["len"])].tobytes()
            msgs, _ = hq.decode_batch(data)
            n = int(msgs["to"][0])
            assert n in (2, 3) and len(msgs) == G and (msgs["ev"]["type"] == hq.HQ_MSG_HEARTBEAT).all()
            assert (msgs["ev"]["hint"] >= 9000).all() and (msgs["ev"]["hint_high"] == 77).all()
            order = np.argsort(msgs["cluster_id"], kind="stable")
            msgs = msgs[order]
            assert msgs["cluster_id"].tolist() == cids
            rows = np.zeros(G, hq.HB_RECEIVED_DTYPE)
            rows["from"], rows["term"], rows["commit"] = msgs["ev"]["from"], msgs["ev"]["term"], msgs["commit"]
            rows["hint"], rows["hint_high"] = msgs["ev"]["hint"], msgs["ev"]["hint_high"]
            assert rows["commit"].tolist() == [min(m, committed) for m in match[n]]
            groups, offsets = np.arange(G, dtype=np.uint32), np.arange(G + 1, dtype=np.uint64)
            outs = {name: w.heartbeats_received(groups, offsets, rows) for name, w in followers[n].items()}
            for name, w in followers[n].items():
                out = outs[name]
                assert out["n_resp"] == G and out["n_contact"] == G and out["n_committed"] == G
                got = w.get_groups(groups)["groups"]
                assert got["committed"].tolist() == [min(m, committed) for m in match[n]], (n, name)
                assert w.readback_count() == 0
            first = next(iter(outs.values()))
            replies = hq.heartbeat_replies_expand(groups, offsets, rows, first, cids, [n] * G)
            assert len(replies) == G
            wire.add_batch(hq.encode_wire_batch(replies, deployment_id=0x5EED, source_address=b"n%d:1" % n)
                           .tobytes())
        data, sizes = np.zeros(2 * G * hq.HQ_EVENT_STREAM_MAX + 64, np.uint8), np.zeros(G, np.uint16)
        stream, stats = wire.step_sized(data, sizes)
        assert stats.messages == 2 * G and stream[2] == 2 * G
        res = leader.step_sized(*stream)
        ready = sorted((int(r["cluster_id"]), int(r["index"]), int(r["ctx_low"]), int(r["ctx_high"]))
                       for r in res["ready"])
        assert ready == [(c, committed, 9000 + j, 77) for j, c in enumerate(cids)]
        assert leader.readback_count() == 0
    finally:
        wire.close()
        leader.close()
        for ws in followers.values():
            for w in ws.values():
                w.close()


# ------------------------------------------------------------------ lifecycle ------------------
@pytest.mark.parametrize("kind", KINDS)
def test_lifecycle(hq, kind):
    states = [sc.FOLLOWER, sc.LEADER, sc.FOLLOWER, sc.CANDIDATE, sc.FOLLOWER, sc.LEADER]
    sim = Sim(hq, kind, [spec(800 + h, s) for h, s in enumerate(states)], start=True)
    try:
        sim.tick()
        # a leader with a pending ReadIndex, then demoted by a higher-term heartbeat: its pending
        # reads and its members' matches are gone, and the next heartbeats send nothing for it
        for w in sim.workers.values():
            ev = np.array([event_record(hq, ("read", 41, 42))], hq.EVENT_DTYPE)
            res = w.step(np.array([1], np.uint32), np.array([0, 1], np.uint64), ev)
            assert len(res["ready"]) == 0 and len(res["fallback_groups"]) == 0
            assert w.heartbeats(np.array([1], np.uint32))["n_messages"] == 2
        sim.table[1]["reads"] = 1
        sim.check_state()
        got = sim.received([1, 5], [[(2, 9, 0, 0, 0)], [(2, 3, 0, 0, 0)]])
        for r in got.values():
            assert r["results"]["n_resets"].tolist() == [1, 0] and r["n_state_changed"] == 1
        assert sim.table[1]["state"] == sc.FOLLOWER and sim.table[1]["reads"] == 0
        sim.check_state()
        for w in sim.workers.values():
            assert w.heartbeats(np.array([1, 5], np.uint32))["words"].tolist()[0] == 0
        sim.tick()

        # a group suspended by a fallback, and a stopped handle: SUSPENDED, nothing changes
        for w in sim.workers.values():
            ev = np.array([event_record(hq, sc.msg(99, 2, 3))], hq.EVENT_DTYPE)
            res = w.step(np.array([2], np.uint32), np.array([0, 1], np.uint64), ev)
            assert [int(x) for x in res["fallback_groups"]] == [802]
            w.stop_groups(np.array([4], np.uint32))
        sim.table[2]["suspended"] = True
        sim.table[4] = None
        got = sim.received([4, 2, 0], [[(2, 9, 15, 0, 0)], [(2, 9, 15, 1, 2), (3, 3, 15, 0, 0)], [(2, 3, 15, 0, 0)]])
        for r in got.values():
            assert r["results"]["flags"].tolist() == [hm.SUSPENDED, hm.SUSPENDED, hm.CONTACT | hm.COMMITTED]
            assert r["n_suspended"] == 2
        assert sim.pending == {0}
        sim.check_state()

        # get_timers / set_timers around a pending contact: handle 0 reads as election_tick 0;
        # set_timers clears its contact, so the set counter counts on
        sim.check_timers()
        for w in sim.workers.values():
            w.set_timers(np.array([0], np.uint32), np.array([(2, 0, 0, 0)], hq.TIMER_DTYPE))
        sim.model.set(0, sim.tick_groups()[0], 2, 0, 0)
        sim.pending.discard(0)
        sim.check_timers()
        sim.tick()
        assert sim.model.get(0, sim.tick_groups()[0])[0] in (3, 0)

        # a contact pending on a handle that is stopped and restarted as another cluster is not
        # inherited; a new tick config clears the pending contacts
        sim.received([0, 3], [[(2, 3, 0, 0, 0)], [(2, 3, 0, 0, 0)]])
        assert sim.pending == {0, 3} and sim.table[3]["state"] == sc.FOLLOWER
        for w in sim.workers.values():
            w.stop_groups(np.array([3], np.uint32))
            new = spec(900, sc.FOLLOWER, term=3)
            assert w.start_groups(*lm.group_arrays(hq, [new])).tolist() == [3]
        sim.table[3] = sim.entry(spec(900, sc.FOLLOWER, term=3))
        sim.model.reset(3)
        sim.pending.discard(3)
        sim.check_timers()
        sim.tick()
        sim.received([0], [[(2, 3, 0, 0, 0)]])
        for w in sim.workers.values():
            w.set_tick_config(E, H, sim.cq, SEED)
        sim.model = tm.TickModel(E, H, sim.cq, SEED)
        sim.pending.clear()
        sim.check_timers()
        sim.tick()
        sim.check_state()
    finally:
        sim.close()


@pytest.mark.parametrize("kind", KINDS)
def test_before_a_tick_config(hq, kind):
    """The call works before a tick config is set; the config then clears what it marked."""
    sim = Sim(hq, kind, [spec(600, sc.FOLLOWER), spec(601, sc.CANDIDATE)], config=False)
    try:
        got = sim.received([1, 0], [[(2, 3, 11, 0, 0)], [(3, 4, 12, 0, 0)]])
        for r in got.values():
            assert r["results"]["n_resets"].tolist() == [1, 1] and r["n_contact"] == 2
        sim.check_state()
        for w in sim.workers.values():
            w.set_tick_config(E, H, True, SEED)
        sim.pending.clear()
        sim.check_timers()
        sim.tick()
    finally:
        sim.close()


# ------------------------------------------------------------------ u64 edges ------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("base", [1 << 32, 1 << 63, U64])
def test_u64_edges(hq, base, kind):
    """Terms and indexes at 2^32, 2^63 and 2^64 - 1: heartbeats at, below and above them."""
    specs = [spec(1000 + j, s, term=base - 2, last=base - 1, committed=base - 4)
             for j, s in enumerate([sc.FOLLOWER, sc.CANDIDATE, sc.LEADER, sc.FOLLOWER])]
    specs.append(spec(1004, sc.FOLLOWER, term=base, last=base, committed=base - 1))
    sim = Sim(hq, kind, specs)
    try:
        rows = [[(2, base - 2, base - 3, U64, base), (2, base - 1, base - 1, 1, 2), (3, base, base, 0, 0)],
                [(2, base - 2, base - 2, 0, 0), (2, base, base - 1, 0, 0)],
                [(2, base - 3, 0, 0, 0), (2, base, base - 1, base, base)],
                [(3, base - 3, base, 0, 0), (3, 0, base - 1, 0, 0)],
                [(2, base, base, 5, 6), (2, base - 1, base, 0, 0)]]
        got = sim.received([4, 3, 2, 1, 0], rows[::-1])
        for r in got.values():
            assert r["results"]["term"].tolist() == [base, base - 2, base, base, base]
            assert r["results"]["commit"].tolist() == [base, base - 1, base - 1, base - 1, base]
        assert sim.table[0]["committed"] == base - 1 and sim.table[4]["committed"] == base
        sim.check_state()
        sim.tick()
        sim.check_state()
    finally:
        sim.close()


# ------------------------------------------------------------------ refusals -------------------
@pytest.mark.parametrize("kind", KINDS)
def test_refusals_change_nothing(hq, kind):
    sim = Sim(hq, kind, [spec(1100 + j, s) for j, s in enumerate([sc.FOLLOWER, sc.CANDIDATE, sc.LEADER])])
    lib, inval = hq.lib, hq.HQ_E_INVAL
    try:
        sim.tick()
        sim.received([0], [[(2, 3, 12, 0, 0)]])
        assert sim.pending == {0}
        good = (np.array([1, 2], np.uint32), np.array([0, 1, 2], np.uint64),
                np.array([(2, 9, 15, 0, 0), (2, 9, 15, 0, 0)], hq.HB_RECEIVED_DTYPE))
        for name, w in sim.workers.items():
            prev = w.heartbeats_received(np.array([2], np.uint32), np.array([0, 1], np.uint64),
                                         np.array([(2, 3, 0, 0, 0)], hq.HB_RECEIVED_DTYPE), copy=False)
            prev_bytes = (prev["replies"].tobytes(), prev["results"].tobytes())
            state = lm.snapshot(w, [0, 1, 2])
            timers = w.get_timers().tobytes()

            def refused(groups, offsets, msgs, cq=1, reserved=0, n=None, null=()):
                inp, keep = hq.hb_received_input(groups, offsets, msgs, cq)
                inp.reserved = reserved
                if n is not None:
                    inp.n_groups = n
                for f in null:
                    setattr(inp, f, None)
                out = hq.HbReceivedOutput()
                out.n_resp = 77
                assert lib.hq_worker_heartbeats_received(w.h, ctypes.byref(inp), ctypes.byref(out)) == inval, name
                assert lib.hq_worker_last_error(w.h).decode() != ""
                assert out.n_resp == 77 and out.replies is None
                assert lm.snapshot(w, [0, 1, 2]) == state and w.get_timers().tobytes() == timers, name
                assert (prev["replies"].tobytes(), prev["results"].tobytes()) == prev_bytes, name

            g, o, m = good
            refused(g, o, m, cq=2)
            refused(g, o, m, reserved=1)
            refused(g, o, m, n=1 << 28)
            refused(g, np.array([0, 1, 1 << 31], np.uint64), m)
            refused(g, o, m, null=("groups",))
            refused(g, o, m, null=("offsets",))
            refused(g, o, m, null=("msgs",))
            refused(g, np.array([0, 2, 1], np.uint64), m)
            refused(g, np.array([1, 1, 2], np.uint64), m)
            refused(np.array([1, 3], np.uint32), o, m)
            refused(np.array([1, 1], np.uint32), o, m)
            out = hq.HbReceivedOutput()
            inp, keep = hq.hb_received_input(g, o, m)
            assert lib.hq_worker_heartbeats_received(w.h, None, ctypes.byref(out)) == inval
            assert lib.hq_worker_heartbeats_received(w.h, ctypes.byref(inp), None) == inval
            # no groups: HQ_OK with empty outputs
            r = w.heartbeats_received(np.zeros(0, np.uint32), np.zeros(1, np.uint64),
                                      np.zeros(0, hq.HB_RECEIVED_DTYPE))
            assert len(r["replies"]) == 0 and len(r["results"]) == 0 and r["n_resp"] == 0
            assert lm.snapshot(w, [0, 1, 2]) == state and w.get_timers().tobytes() == timers
        # the pending contact of handle 0 survived all of it
        sim.check_timers()
        sim.tick()
        sim.check_state()
    finally:
        sim.close()
