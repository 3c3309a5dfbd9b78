"""Groups started and stopped on a running worker, and the member pool's compaction
(hq_worker_start_groups / _stop_groups / _pool_info / _compact: hq_worker_lifecycle.cpp,
hq_pool.hip, the wire's handle tables). Expected values come from the CPU oracle
(step_harness.OracleBackend: its world is a dict by cluster id, so a start adds an entry and a stop
deletes one) and from the handle model of lifecycle_model.py; device workers are additionally held
equal to a host-worker twin. No device worker may read its state back."""
import ctypes

import numpy as np
import pytest

import config_ref as ref
import lifecycle_model as lm
import step_random as sr
import step_scenarios as sc
import wire_encode as we
from step_harness import event_record

pytestmark = pytest.mark.gpu
KINDS = ["device", "host"]
U64 = (1 << 64) - 1


def make_world(hq, kind, form="rows"):
    """kind 'device': a device worker and its host twin; 'host': a host worker alone. form 'rows'
    or 'sized16' (a device worker then with HQ_WORKER_READY_SLOTS, fed from pinned memory)."""
    if kind == "device":
        slots = form == "sized16"
        workers = {"device": hq.Worker(0, 8, on_device=True, commit_advance=slots, ready_compact=slots,
                                       ready_slots=slots), "twin": hq.Worker(0, 8)}
        streams = {"device": "sized16-slots" if slots else False, "twin": False}
    else:
        workers = {"host": hq.Worker(0, 8)}
        streams = {"host": "sized16" if form == "sized16" else False}
    return lm.World(hq, workers, streams)


def under_test(wd):
    return wd.workers.get("device") or wd.workers["host"]


def expect_inval(hq, fn):
    with pytest.raises(hq.HQError) as e:
        fn()
    assert e.value.code == hq.HQ_E_INVAL


def wide_group(rng, cid):
    """16 members: 8 voting (one of them a witness) and 8 observers, a leader."""
    g = list(sr.random_groups(rng, 1, cid0=cid)[0])
    last, committed = g[5], g[4]
    ids = rng.choice(np.arange(1, 64), 16, replace=False).tolist()
    roles = [sc.REMOTE] * 7 + [sc.WITNESS] + [sc.OBSERVER] * 8
    mem = [(int(i), last if k == 0 else int(rng.integers(max(0, committed - 3), last + 1)), r, 0)
           for k, (i, r) in enumerate(zip(ids, roles))]
    g[1], g[3] = int(ids[0]), sc.LEADER
    g[7] = [mem[k] for k in rng.permutation(16)]
    g[8] = sr.random_log(rng, g[2], g[3], committed, g[6])
    return tuple(g)


def single_group(rng, cid):
    g = list(sr.random_groups(rng, 1, cid0=cid)[0])
    g[3] = sc.LEADER
    g[7] = [(g[1], g[5], sc.REMOTE, 1)]
    g[8] = sr.random_log(rng, g[2], g[3], g[4], g[6])
    return tuple(g)


def random_step(wd, rng, step_no, ctx_seq, share=0.85):
    per = {c: sr.random_events(rng, wd.oracle.state(c), step_no, ctx_seq)
           for c in wd.model.live_cids() if rng.random() < share}
    if per:
        wd.step(per)


# ------------------------------------------------------------------ random lifecycles ---------
@pytest.mark.parametrize("form", ["rows", "sized16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("G0", [1, 17, 300])
def test_random_lifecycles(hq, G0, kind, form):
    rng = np.random.default_rng(7700 + G0)
    wd = make_world(hq, kind, form)
    try:
        wd.start(sr.random_groups(rng, G0), via_add=True)
        next_cid, stopped, ctx_seq = 10_000, [], [0]
        for rnd in range(12):
            random_step(wd, rng, rnd + 1, ctx_seq)
            if "twin" in wd.workers:
                a, b = wd.workers["device"].heartbeats(), wd.workers["twin"].heartbeats()
                for k in ("words", "lags", "ctxs"):
                    assert a[k].tobytes() == b[k].tobytes(), (rnd, k)
                assert a["n_messages"] == b["n_messages"]
            live = wd.model.live()
            k = min(int(rng.choice([0, 1, 15, 16, 17])), len(live))
            if k:
                stopped += wd.stop([int(h) for h in rng.choice(live, k, replace=False)])
            # new clusters: random ones, a 1-member group, a 16-member group, and restarts of
            # stopped cluster ids in another state and term
            specs = sr.random_groups(rng, int(rng.integers(0, 20)), cid0=next_cid)
            next_cid += len(specs)
            specs += [single_group(rng, next_cid), wide_group(rng, next_cid + 1)]
            next_cid += 2
            rng.shuffle(stopped)
            back, stopped = stopped[:len(stopped) // 2], stopped[len(stopped) // 2:]
            specs += [sr.random_groups(rng, 1, cid0=c)[0] for c in back]
            order = rng.permutation(len(specs))
            wd.start([specs[i] for i in order])
            if rnd % 3 == 1:
                config_round(wd, rng, 900 + rnd)
            wd.no_readback()
        random_step(wd, rng, 13, ctx_seq, share=1.0)
        live = wd.model.live()
        w = under_test(wd)
        info = w.pool_info()
        assert (info["handles"], info["live_groups"], info["vacant_handles"]) == \
            (wd.model.handles, len(live), len(wd.model.vacant))
        assert w.group_count() == wd.model.handles
        if "twin" in wd.workers:
            lm.same_output(w.get_groups(np.array(live, np.uint32)),
                           wd.workers["twin"].get_groups(np.array(live, np.uint32)))
            assert info == wd.workers["twin"].pool_info()
        wd.no_readback()
    finally:
        wd.close()


def config_round(wd, rng, node_id):
    """ADD_OBSERVER of a new node to a few groups without pending reads or votes; the oracle's
    group is rebuilt with the observer (match 0, inactive: addObserver, raft.go:1152-1160)."""
    picks = []
    for c in wd.model.live_cids():
        st = wd.oracle.state(c)
        if st[1] != sc.CANDIDATE and not st[6] and len(st[5]) < 16 and rng.random() < 0.2:
            picks.append(c)
    picks = picks[:5]
    if not picks:
        return
    ch = [(wd.model.find(c), ref.ADD_OBSERVER, node_id) for c in picks]
    for name, b in wd.backs.items():
        assert b.w.config_changes(ch)["status"].tolist() == [ref.APPLIED] * len(ch), name
    for c in picks:
        term, state, committed, last, ts, mem, _ = wd.oracle.state(c)
        log = wd.oracle.groups[c].log_terms()
        wd.oracle.add_group(c, wd.node_of[c], term, state, committed, last, ts,
                            mem + [(node_id, 0, sc.OBSERVER, 0)], log)


# ------------------------------------------------------------------ a vacant handle -----------
@pytest.mark.parametrize("kind", KINDS)
def test_vacant_handle(hq, kind):
    wd = make_world(hq, kind)
    try:
        wd.start([lm.leader(c, 3, 10, 5) for c in (11, 12, 13)], via_add=True)
        wd.step({c: [sc.msg(sc.RREP, 2, 2, 7)] for c in (11, 12, 13)})
        wd.stop([1])
        for name, w in wd.workers.items():
            ev = np.array([event_record(hq, e) for e in
                           [sc.msg(sc.RREP, 2, 2, 8), sc.msg(sc.RREP, 3, 2, 9), ("propose", 1),
                            sc.msg(sc.RREP, 2, 2, 8)]], hq.EVENT_DTYPE)
            res = w.step(np.array([1, 2], np.uint32), np.array([0, 3, 4], np.uint64), ev)
            assert sorted(res["deferred"].tolist()) == [0, 1, 2], name      # the vacant handle's
            assert res["commits"]["cluster_id"].tolist() == [13]
            assert len(res["fallback_groups"]) == 0 and len(res["state_changes"]) == 0
            assert len(res["ready"]) == 0 and len(res["read_resps"]) == 0
            assert w.heartbeats(np.array([1], np.uint32))["words"].tolist() == [0]
            assert w.heartbeats()["words"][1] == 0
            hb = w.heartbeat_batches(np.array([1], np.uint32))
            assert hb["n_messages"] == 0 and len(hb["bytes"]) == 0
            before = lm.snapshot(w, [0, 2])
            expect_inval(hq, lambda: w.config_changes([(1, ref.ADD_OBSERVER, 77)]))
            expect_inval(hq, lambda: w.config_changes([(0, ref.ADD_OBSERVER, 77), (1, ref.ADD_OBSERVER, 77)]))
            expect_inval(hq, lambda: w.get_groups(np.array([0, 1], np.uint32)))
            expect_inval(hq, lambda: w.get_groups())
            expect_inval(hq, lambda: w.find(12))
            assert lm.snapshot(w, [0, 2]) == before
            assert w.group_count() == 3
            assert w.pool_info() == {"handles": 3, "live_groups": 2, "vacant_handles": 1,
                                     "member_records": 9, "live_member_records": 6, "epoch": 1}
        wd.oracle.step({13: [sc.msg(sc.RREP, 2, 2, 8)]})            # (the step above, on the oracle)
        # a route row written while the handle is vacant is reset by the next start
        for w in wd.workers.values():
            w.set_heartbeat_routes(1, np.zeros((1, 16), np.uint16))
        assert wd.start([lm.leader(14, 3, 20, 15)]) == [1]
        for w in wd.workers.values():
            hb = w.heartbeat_batches(np.array([1], np.uint32))
            assert hb["n_messages"] == 0 and hb["n_unrouted"] == 2
        wd.step({c: [sc.msg(sc.RREP, 2, 2, 9)] for c in (11, 13)} | {14: [sc.msg(sc.RREP, 2, 2, 17)]})
        wd.no_readback()
    finally:
        wd.close()


# ------------------------------------------------------------------ errors change nothing -----
@pytest.mark.parametrize("kind", KINDS)
def test_errors_change_nothing(hq, kind):
    rng = np.random.default_rng(31)
    wd = make_world(hq, kind)
    try:
        wd.start(sr.random_groups(rng, 6), via_add=True)
        random_step(wd, rng, 1, [0], share=1.0)
        wd.stop([2])
        w, live = under_test(wd), wd.model.live()
        before, info = lm.snapshot(w, live), w.pool_info()
        ok = lm.leader(50, 3, 10, 5)
        nine = (52, 1, 2, sc.LEADER, 5, 10, 5, [(i, 5, sc.REMOTE, 0) for i in range(1, 10)])
        seventeen = (53, 1, 2, sc.LEADER, 5, 10, 5,
                     [(1, 10, sc.REMOTE, 0)] + [(i, 5, sc.OBSERVER, 0) for i in range(2, 18)])
        bad_starts = [[ok, lm.leader(1, 3, 10, 5)],                     # an existing cluster
                      [ok, lm.leader(51, 3, 10, 5), lm.leader(51, 5, 10, 5)],   # a cluster twice
                      [ok, lm.leader(51, 3, 10, 5, node=9)],            # the node is no remote
                      [ok, nine]]                                       # 9 voting members
        if kind == "device":
            bad_starts.append([ok, seventeen])                          # 17 members on the device
        for specs in bad_starts:
            expect_inval(hq, lambda: w.start_groups(*lm.group_arrays(hq, specs)))
            assert (lm.snapshot(w, live), w.pool_info()) == (before, info), specs[-1][0]
            expect_inval(hq, lambda: w.find(50))
        for handles in ([0, 6], [0, 2], [0, 1, 0]):                     # unknown, vacant, duplicate
            expect_inval(hq, lambda: w.stop_groups(np.array(handles, np.uint32)))
            assert (lm.snapshot(w, live), w.pool_info()) == (before, info), handles
        lib, inval = hq.lib, hq.HQ_E_INVAL
        g, m = lm.group_arrays(hq, [ok])
        gp, mp = g.ctypes.data_as(ctypes.c_void_p), m.ctypes.data_as(ctypes.c_void_p)
        one = np.zeros(1, np.uint32)
        assert lib.hq_worker_start_groups(w.h, 1, None, mp, None, None) == inval
        assert lib.hq_worker_start_groups(w.h, 1, gp, None, None, None) == inval
        assert lib.hq_worker_stop_groups(w.h, 1, None, None) == inval
        assert lib.hq_worker_pool_info(w.h, None) == inval
        assert lib.hq_worker_start_groups(None, 1, gp, mp, None, None) == inval
        assert lib.hq_worker_stop_groups(None, 1, one.ctypes.data_as(ctypes.c_void_p), None) == inval
        assert lib.hq_worker_compact(None, None) == inval
        assert lib.hq_worker_start_groups(w.h, 0, None, None, None, None) == hq.HQ_OK
        assert lib.hq_worker_stop_groups(w.h, 0, None, None) == hq.HQ_OK
        assert (lm.snapshot(w, live), w.pool_info()) == (before, info)
        random_step(wd, rng, 2, [100], share=1.0)
        wd.no_readback()
    finally:
        wd.close()


# ------------------------------------------------------------------ growth --------------------
def test_growth_keeps_resident_state(hq):
    """The device arrays regrow under a start while the mirror is stale: the first groups' state,
    which only the device holds, must survive."""
    rng = np.random.default_rng(41)
    wd = make_world(hq, "device")
    try:
        wd.start([lm.leader(c, 3, 10, 5) for c in (1, 2, 3)], via_add=True)
        wd.step({c: [("read", 70 + c, 1), sc.msg(sc.RREP, 2, 2, 6 + c), ("propose", 2)] for c in (1, 2, 3)})
        dev = wd.workers["device"]
        before = lm.snapshot(dev, [0, 1, 2])
        r = dev.get_groups(np.array([0, 1, 2], np.uint32))
        assert r["groups"]["n_pending_reads"].tolist() == [1, 1, 1]
        assert r["groups"]["committed"].tolist() == [7, 8, 9]
        new = wd.start(sr.random_groups(rng, 5000, cid0=100))
        assert new == list(range(3, 5003))
        assert lm.snapshot(dev, [0, 1, 2]) == before
        lm.same_output(dev.get_groups(np.array([0, 1, 2, 3, 2500, 5002], np.uint32)),
                       wd.workers["twin"].get_groups(np.array([0, 1, 2, 3, 2500, 5002], np.uint32)))
        per = {c: [sc.msg(sc.HBRESP, 2, 2, hint=70 + c, high=1), sc.msg(sc.RREP, 3, 2, 12)] for c in (1, 2, 3)}
        for c in (100, 2600, 5099):
            per[c] = sr.random_events(rng, wd.oracle.state(c), 2, [500])
        want = wd.step(per)
        # (the reads pending since the first step, at the index committed when they came)
        assert [want[c]["ready"] for c in (1, 2, 3)] == [[(5, 70 + c, 1)] for c in (1, 2, 3)]
        wd.no_readback()
    finally:
        wd.close()


# ------------------------------------------------------------------ compaction ----------------
@pytest.mark.parametrize("kind", KINDS)
def test_compaction(hq, kind):
    rng = np.random.default_rng(51)
    wd = make_world(hq, kind)
    try:
        specs = []
        for j in range(12):      # 3-member groups with 16-member and 1-member neighbours
            specs += [lm.leader(100 + 3 * j, 3, 10, 5), wide_group(rng, 101 + 3 * j),
                      single_group(rng, 102 + 3 * j)]
        wd.start(specs[:18], via_add=True)
        wd.start(specs[18:])
        others = [s[0] for s in specs if s[0] % 3 != 1]          # (the 3-member groups: 100 + 3j)
        wd.step({c: sr.random_events(rng, wd.oracle.state(c), 1, [0]) for c in others})
        # a full range (3 members + 1) moves to the pool's end and leaves a gap behind; the mirror
        # is stale by now
        three = [wd.model.find(100 + 3 * j) for j in range(12)]
        for name, b in wd.backs.items():
            st = b.w.config_changes([(h, ref.ADD_OBSERVER, 200) for h in three])["status"]
            assert st.tolist() == [ref.APPLIED] * 12, name
        for j in range(12):
            c = 100 + 3 * j
            term, state, committed, last, ts, mem, reads = wd.oracle.state(c)
            assert not reads
            wd.oracle.add_group(c, 1, term, state, committed, last, ts, mem + [(200, 0, sc.OBSERVER, 0)],
                                wd.oracle.groups[c].log_terms())
        random_step(wd, rng, 2, [100], share=1.0)
        wd.stop([h + k for h in (0, 9, 18, 27) for k in range(3)])      # a third of the groups
        live = wd.model.live()
        w = under_test(wd)
        info = w.pool_info()
        assert info["live_member_records"] == sum(len(wd.oracle.state(c)[5]) for c in wd.model.live_cids())
        assert info["member_records"] > info["live_member_records"]
        before = {n: lm.snapshot(x, live) for n, x in wd.workers.items()}
        for n, x in wd.workers.items():
            ns = x.compact()
            assert (ns > 0) == (n == "device"), n
            after = x.pool_info()
            assert after["member_records"] == after["live_member_records"] == info["live_member_records"]
            assert {k: v for k, v in after.items() if k != "member_records"} == \
                {k: v for k, v in info.items() if k != "member_records"}
            assert lm.snapshot(x, live) == before[n], n
        for s in range(3):
            random_step(wd, rng, 3 + s, [1000 * (s + 1)], share=1.0)
        if "twin" in wd.workers:
            lm.same_output(w.get_groups(np.array(live, np.uint32)),
                           wd.workers["twin"].get_groups(np.array(live, np.uint32)))
        # a later relocation and start land behind the packed pool
        c = next(c for c in wd.model.live_cids() if c % 3 == 0 and c < 200 and not wd.oracle.state(c)[6])
        h = wd.model.find(c)                                            # (a 1-member group)
        for b in wd.backs.values():
            assert b.w.config_changes([(h, ref.ADD_OBSERVER, 201)])["status"].tolist() == [ref.APPLIED]
        term, state, committed, last, ts, mem, reads = wd.oracle.state(c)
        wd.oracle.add_group(c, wd.node_of[c], term, state, committed, last, ts,
                            mem + [(201, 0, sc.OBSERVER, 0)], wd.oracle.groups[c].log_terms())
        wd.start([lm.leader(900, 5, 30, 20)])
        random_step(wd, rng, 9, [9000], share=1.0)
        for x in wd.workers.values():
            assert x.compact() >= 0 and x.compact() == 0                # dense: nothing to do
            assert x.pool_info()["member_records"] == x.pool_info()["live_member_records"]
        random_step(wd, rng, 10, [10000], share=1.0)
        wd.stop(wd.model.live())
        for x in wd.workers.values():                                   # an all-vacant worker
            x.compact()
            info = x.pool_info()
            assert (info["member_records"], info["live_groups"]) == (0, 0)
            x.compact()
        assert wd.start([lm.leader(901, 3, 10, 5)]) == [wd.model.find(901)]
        wd.step({901: [sc.msg(sc.RREP, 2, 2, 8)]})
        wd.no_readback()
    finally:
        wd.close()


# ------------------------------------------------------------------ slots with vacancies ------
def with_acks(state, node, ev):
    """A leader's events with every other voting member's ack of its last index ahead of the other
    messages: it commits in this step (the advance column needs a quarter of the groups to)."""
    term, st, committed, last, ts, mem, reads = state
    if st != sc.LEADER:
        return ev
    k = sum(1 for e in ev if e[0] == "read")
    return ev[:k] + [sc.msg(sc.RREP, m[0], term, last) for m in mem
                     if m[2] != sc.OBSERVER and m[0] != node] + ev[k:]


def test_slots_with_vacancies(hq):
    """An implicit-list sized16 step over a handle space with vacancies at a tile's edges (handles
    0, 255, 256, 257 and the last): the merged ReadyToReads and the advance column."""
    rng = np.random.default_rng(61)
    G = 600
    wd = make_world(hq, "device", "sized16")
    try:
        wd.start(sr.random_groups(rng, G), via_add=True)
        ctx_seq = [0]
        for s in range(2):
            random_step(wd, rng, s + 1, ctx_seq)
        wd.stop([0, 255, 256, 257, 599])
        cids = [c if c is not None else 0 for c in wd.model.cluster]
        per = {c: with_acks(wd.oracle.state(c), wd.node_of[c],
                            sr.random_events(rng, wd.oracle.state(c), 3, ctx_seq))
               for c in wd.model.live_cids()}
        committed = np.array([wd.oracle.state(c)[2] if c else 0 for c in cids], np.uint64)
        want = wd.oracle.step(per)
        recs, off = [], [0]
        for c in cids:
            recs += [event_record(hq, e) for e in per.get(c, ())]
            off.append(len(recs))
        ev = np.array(recs, hq.EVENT_DTYPE)
        data, sizes = hq.encode_events_sized(np.array(off, np.uint64), ev)
        b = wd.backs["device"]
        res = wd.workers["device"].step_sized(None, b._pinned("sizes", hq.sizes16_of(sizes)), len(ev),
                                              b._pinned("data", data))
        assert len(res["ready_slots"]) > 0
        got = hq.merge_ready(res, np.array(cids, np.uint64), committed)
        exp = [(c, *r) for c in cids if c for r in want[c]["ready"]]
        assert [(int(r["cluster_id"]), int(r["index"]), int(r["ctx_low"]), int(r["ctx_high"]))
                for r in got] == exp and len(exp) > 20
        # the advance column (a step in which more than a quarter of the groups commit)
        exp_adv = [want[c]["committed"] - int(committed[h]) if c else 0 for h, c in enumerate(cids)]
        assert sum(1 for a in exp_adv if a) > G // 4
        assert res["committed_advance"].tolist() == exp_adv
        assert len(res["fallback_groups"]) == 0
        wd.no_readback()
    finally:
        wd.close()


# ------------------------------------------------------------------ the wire follows ----------
DEPLOYMENT = 0x5EED


def wire_step(hq, wire, w, mode, pin, msgs, locals_=()):
    """One step through the attached wire: returns ({cluster: committed}, WireStats)."""
    wire.reset()
    for cid, events in locals_:
        wire.add_local(cid, np.array([event_record(hq, e) for e in events], hq.EVENT_DTYPE))
    wire.add_batch(we.batch([we.message(type=sc.RREP, to=1, frm=2, cluster_id=c, term=2, log_index=i)
                             for c, i in msgs], deployment_id=DEPLOYMENT, source_address=b"n2:1"))
    if mode == "device":
        res, st = wire.step_device()
    else:
        data, sizes = pin.pinned(4096, np.uint8), pin.pinned(w.group_count(), np.uint16)
        ss, st = wire.step_sized(data, sizes)
        res = w.step_sized(*ss)
    assert len(res["fallback_groups"]) == 0 and len(res["deferred"]) == 0
    return {int(r["cluster_id"]): int(r["committed"]) for r in res["commits"]}, st


@pytest.mark.parametrize("mode", ["host-attached", "device"])
def test_wire_follows(hq, mode):
    A, B, C = 5, U64, 9
    w = hq.Worker(0, 8, on_device=mode == "device")
    wire, pin = hq.Wire(DEPLOYMENT), hq.Context(0)
    try:
        g, m = lm.group_arrays(hq, [lm.leader(c, 3, 10, 5) for c in (A, B, C)])
        assert w.start_groups(g, m).tolist() == [0, 1, 2]
        wire.attach_device(w) if mode == "device" else wire.attach(w)
        got, st = wire_step(hq, wire, w, mode, pin, [(A, 7), (B, 7), (C, 7)])
        assert got == {A: 7, B: 7, C: 7} and st.dropped_no_cluster == 0
        w.stop_groups(np.array([0, 1], np.uint32))
        got, st = wire_step(hq, wire, w, mode, pin, [(A, 8), (B, 8), (C, 8), (B, 9)],
                            locals_=[(A, [("propose", 1)]), (B, [("propose", 2), ("propose", 1)])])
        assert got == {C: 8} and st.dropped_no_cluster == 3 + 3
        for c in (A, B):
            expect_inval(hq, lambda: w.find(c))
        # restarted in swapped order: each takes the other's old handle
        g, m = lm.group_arrays(hq, [lm.leader(A, 3, 20, 11), lm.leader(B, 3, 30, 21)])
        assert w.start_groups(g, m).tolist() == [1, 0]
        got, st = wire_step(hq, wire, w, mode, pin, [(A, 15), (B, 25), (C, 9)],
                            locals_=[(B, [("propose", 1)])])
        assert got == {A: 15, B: 25, C: 9} and st.dropped_no_cluster == 0
        r = w.get_groups(np.array([0, 1, 2], np.uint32))["groups"]
        assert r["cluster_id"].tolist() == [B, A, C] and r["last_index"].tolist() == [31, 20, 10]
        assert w.readback_count() == 0
    finally:
        wire.close()
        w.close()
        pin.close()


# ------------------------------------------------------------------ the u64 edge --------------
@pytest.mark.parametrize("kind", KINDS)
def test_restart_at_u64_edge(hq, kind):
    wd = make_world(hq, kind)
    try:
        wd.start([lm.leader(c, 3, 10, 5) for c in (1, 2)], via_add=True)
        wd.step({1: [sc.msg(sc.RREP, 2, 2, 7)]})
        wd.stop([0])
        top = U64 - 2
        assert wd.start([lm.leader(1, 3, top, top - 3, term=U64 - 1)]) == [0]
        want = wd.step({1: [("read", U64, U64), sc.msg(sc.RREP, 2, U64 - 1, top - 1),
                            sc.msg(sc.HBRESP, 3, U64 - 1, hint=U64, high=U64), ("propose", 1)],
                        2: [sc.msg(sc.RREP, 3, 2, 9)]})
        assert want[1]["committed"] == top - 1 and want[1]["ready"] == [(top - 3, U64, U64)]
        want = wd.step({1: [sc.msg(sc.RREP, 3, U64 - 1, top + 1)]})
        assert want[1]["committed"] == top + 1
        wd.no_readback()
    finally:
        wd.close()
