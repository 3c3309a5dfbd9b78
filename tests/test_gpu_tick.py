"""Raft timers on the step worker (hq_worker_set_tick_config / _tick / _get_timers / _set_timers:
hq_worker_tick.cpp, hq_tick.hip). Expected values come from tick_model.TickModel over the state of
the CPU oracle (or over a table the test keeps itself where no group changes state); device workers
are additionally held byte-equal to a host-worker twin. No device worker may read its state back."""
import ctypes

import numpy as np
import pytest

import lifecycle_model as lm
import step_scenarios as sc
import tick_model as tm
import tick_world as tw
from step_harness import event_record

pytestmark = pytest.mark.gpu
KINDS = ["device", "host"]
TILE = 256          # kTickTile (hq_tick.h): handles per workgroup of the tick, the scan's tile
SEED = 0xD1CE


def make_workers(hq, kind):
    if kind == "device":
        return {"device": hq.Worker(0, 8, on_device=True), "twin": hq.Worker(0, 8)}
    return {"host": hq.Worker(0, 8)}


def close_all(workers):
    for w in workers.values():
        w.close()


def spec(cid, state, term=2, last=10, committed=5):
    """A group of three remotes (the node is 1) in `state`."""
    mem = [(i, last if i == 1 and state == sc.LEADER else (committed if state == sc.LEADER else 0),
            sc.REMOTE, 0) for i in (1, 2, 3)]
    return (cid, 1, term, state, committed, last, committed, mem, None)


def tick_all(workers, model, groups, contact=()):
    """One tick on the model and on every worker; lists, n_ticked and all live timers must match,
    and a device worker's lists are byte-equal to its twin's. Returns the model's tick."""
    want = model.tick(groups, contact)
    got = {}
    for name, w in workers.items():
        got[name] = w.tick(np.array(contact, np.uint32) if len(contact) else None)
        tm.check_tick(got[name], want)
        tm.check_timers(w, model, groups)
        assert (got[name]["gpu_ns"] > 0) == (name == "device") or not len(groups), name
    if "twin" in got:
        for k in ("check_quorum", "heartbeat", "election"):
            assert got["device"][k].tobytes() == got["twin"][k].tobytes(), k
    return want


# ------------------------------------------------------------------ the compaction's edges -----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("G", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_compaction_boundaries(hq, G, H, kind):
    """All leaders, E = 3: every handle is due at once or none is, at every wave and tile edge."""
    workers = make_workers(hq, kind)
    try:
        g, m = lm.group_arrays(hq, [spec(100 + j, sc.LEADER) for j in range(G)])
        groups = [(100 + j, 2, sc.LEADER, False) for j in range(G)]
        model = tm.TickModel(3, H, True, SEED)
        for w in workers.values():
            w.add_groups(g, m)
            w.set_tick_config(3, H, True, SEED)
        everyone = nobody = 0
        for _ in range(7):
            want = tick_all(workers, model, groups)
            assert want[2] == [] and want[3] == G
            everyone += sum(len(l) == G for l in want[:2])
            nobody += sum(len(l) == 0 for l in want[:2])
        # CheckQuorum at ticks 3 and 6; heartbeats at every tick (H = 1) or at ticks 2, 4, 6
        assert (everyone, nobody) == ((9, 5) if H == 1 else (5, 9))
        for w in workers.values():
            assert w.readback_count() == 0
    finally:
        close_all(workers)


# ------------------------------------------------------------------ random worlds with steps ---
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cq", [1, 0])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("E", [2, 5])
@pytest.mark.parametrize("G", [17, 300])
def test_random_worlds_with_steps(hq, G, E, H, cq, kind):
    """40 rounds of tick (with a contact list of followers, some leaders and repeats), a step whose
    events include the tick's CheckQuorum / Election, and heartbeats over the tick's list. The
    same seeds are checked on the CPU to show every list and every kind of reset
    (test_tick_api.py)."""
    workers = make_workers(hq, kind)
    streams = {n: False for n in workers}
    tw.check_seen(tw.run(hq, workers, streams, G, E, H, cq), cq)      # (run closes the workers)


# ------------------------------------------------------------------ lifecycle and re-sync ------
def raw_step(hq, w, handle, events):
    ev = np.array([event_record(hq, e) for e in events], hq.EVENT_DTYPE)
    return w.step(np.array([handle], np.uint32), np.array([0, len(ev)], np.uint64), ev)


@pytest.mark.parametrize("kind", KINDS)
def test_lifecycle_and_resync(hq, kind):
    E, H = 4, 3
    workers = make_workers(hq, kind)
    try:
        states = [sc.LEADER, sc.FOLLOWER, sc.LEADER, sc.FOLLOWER, sc.LEADER, sc.CANDIDATE, sc.FOLLOWER,
                  sc.LEADER, sc.FOLLOWER, sc.LEADER]
        specs = [spec(200 + h, s, term=3 + h % 2) for h, s in enumerate(states)]
        groups = [(s[0], s[2], s[3], False) for s in specs]
        model = tm.TickModel(E, H, True, SEED)
        g, m = lm.group_arrays(hq, specs)
        for w in workers.values():
            assert w.start_groups(g, m).tolist() == list(range(10))
            w.set_tick_config(E, H, True, SEED)
        for _ in range(2):
            tick_all(workers, model, groups, contact=[1])
        assert model.get(4, groups[4])[:2] == (2, 2)            # (counters a reset would lose)

        # stopped: vacant handles are in no list and not ticked
        for w in workers.values():
            w.stop_groups(np.array([3, 4], np.uint32))
        groups[3] = groups[4] = None
        want = tick_all(workers, model, groups)
        assert want[3] == 8 and not {3, 4} & set(want[0] + want[1] + want[2])

        # restarted: handle 4 (vacated last) reused by another cluster with the same term and
        # state; its timer is a reset one drawn for the new cluster id
        old = specs[4]
        new = spec(900, old[3], term=old[2])
        g1, m1 = lm.group_arrays(hq, [new])
        for w in workers.values():
            assert w.start_groups(g1, m1).tolist() == [4]
        groups[4] = (900, new[2], new[3], False)
        model.reset(4)
        fresh = (0, 0, tm.timeout(SEED, 900, new[2], new[3], E))
        assert tm.timeout(SEED, 900, new[2], new[3], E) != tm.timeout(SEED, 204, new[2], new[3], E)
        for w in workers.values():
            t = w.get_timers(np.array([4], np.uint32))[0]
            assert (int(t["election_tick"]), int(t["heartbeat_tick"]), int(t["randomized_timeout"])) == fresh
        tick_all(workers, model, groups)

        # suspended by a fallback (a message type no worker takes), ticked while suspended, then
        # handed back with set_groups: not ticked, in no list, and back with a reset timer
        for w in workers.values():
            res = raw_step(hq, w, 0, [sc.msg(99, 1, groups[0][1])])
            assert [int(x) for x in res["fallback_groups"]] == [200]
        groups[0] = (200, groups[0][1], groups[0][2], True)
        for _ in range(2):
            want = tick_all(workers, model, groups, contact=[0, 1])
            assert want[3] == 8 and 0 not in want[0] + want[1] + want[2]
        for w in workers.values():
            got = w.get_groups(np.array([0], np.uint32))
            assert got["groups"]["suspended"].tolist() == [1]
            w.set_groups(got["groups"].copy(), got["members"])
        groups[0] = (200, groups[0][1], groups[0][2], False)
        model.reset(0)
        want = tick_all(workers, model, groups)
        assert want[3] == 9 and model.get(0, groups[0])[:2] == (1, 1)

        # a group re-synced while it counts (not suspended) comes back reset too
        tick_all(workers, model, groups)
        for w in workers.values():
            got = w.get_groups(np.array([7], np.uint32))
            w.set_groups(got["groups"].copy(), got["members"])
        model.reset(7)
        tick_all(workers, model, groups)
        assert model.get(7, groups[7])[:2] == (1, 1)

        # after hq_worker_compact (the stopped groups left gaps in the member pool)
        for name, w in workers.items():
            assert w.pool_info()["member_records"] > w.pool_info()["live_member_records"], name
            w.compact()
        tick_all(workers, model, groups)

        # set_timers of arbitrary valid counters: a leader one tick before both of its limits, a
        # follower one tick before a timeout of its own, a candidate with a drawn timeout
        sets = {2: (E - 1, H - 1, 0), 1: (E + 1, 0, E + 2), 5: (1, 0, 0), 9: (2 * E - 1, 0, 2 * E - 1)}
        hs = np.array(sorted(sets), np.uint32)
        ts = np.array([sets[int(h)] + (0,) for h in hs], hq.TIMER_DTYPE)
        for w in workers.values():
            w.set_timers(hs, ts)
        for h, (et, ht, rt) in sets.items():
            model.set(h, groups[h], et, ht, rt)
        for w in workers.values():
            tm.check_timers(w, model, groups)
        want = tick_all(workers, model, groups)
        assert 2 in want[0] and 2 in want[1] and 1 in want[2] and 9 in want[0]
        for _ in range(3):
            tick_all(workers, model, groups, contact=[6, 6, 8])
        for w in workers.values():
            assert w.readback_count() == 0
    finally:
        close_all(workers)


# ------------------------------------------------------------------ many workgroups ------------
@pytest.mark.parametrize("kind", KINDS)
def test_many_workgroups(hq, kind):
    """G = 65 537 + 3 x 256 = 66 305 handles (260 tiles of 256, the last one a single handle: the
    cross-tile scan makes two rounds of 256 tiles), leaders and followers mixed, E = 2."""
    G = 65_537 + 3 * TILE
    rng = np.random.default_rng(77)
    state = rng.choice([sc.LEADER, sc.LEADER, sc.FOLLOWER, sc.CANDIDATE], G).astype(np.uint32)
    term = rng.integers(1, 6, G).astype(np.uint64)
    g = np.zeros(G, hq.WORKER_GROUP_DTYPE)
    g["cluster_id"] = np.arange(1, G + 1, dtype=np.uint64) * 3
    g["node_id"], g["term"], g["state"], g["n_members"] = 1, term, state, 1
    g["committed"], g["last_index"], g["term_start"] = 5, 10, 5
    m = np.zeros(G, hq.MEMBER_DTYPE)
    m["node_id"], m["match"], m["role"] = 1, 10, sc.REMOTE
    groups = list(zip((g["cluster_id"]).tolist(), term.tolist(), state.tolist(), [False] * G))
    workers = make_workers(hq, kind)
    try:
        model = tm.TickModel(2, 2, True, SEED)
        for w in workers.values():
            w.add_groups(g, m)
            w.set_tick_config(2, 2, True, SEED)
        sizes = []
        for k in range(4):
            contact = np.flatnonzero((state != sc.LEADER) & (rng.random(G) < 0.3)).astype(np.uint32)
            want = model.tick(groups, contact)
            for name, w in workers.items():
                tm.check_tick(w.tick(contact), want)
            sizes.append([len(l) for l in want[:3]])
        for w in workers.values():
            tm.check_timers(w, model, groups, handles=list(range(0, G, 7)) + [G - 1])
            assert w.readback_count() == 0
        assert all(max(col) > 1000 for col in zip(*sizes)), sizes
    finally:
        close_all(workers)


# ------------------------------------------------------------------ refusals -------------------
@pytest.mark.parametrize("kind", KINDS)
def test_refusals_on_a_live_worker(hq, kind):
    E, H = 4, 2
    workers = make_workers(hq, kind)
    try:
        specs = [spec(300 + h, s) for h, s in enumerate([sc.LEADER, sc.FOLLOWER, sc.LEADER, sc.FOLLOWER])]
        g, m = lm.group_arrays(hq, specs)
        groups = [(s[0], s[2], s[3], False) for s in specs]
        for name, w in workers.items():
            w.start_groups(g, m)

            def refused(code, fn):
                with pytest.raises(hq.HQError) as e:
                    fn()
                assert e.value.code == code, name
                assert hq.lib.hq_worker_last_error(w.h).decode() != ""

            # before a config
            refused(hq.HQ_E_STATE, lambda: w.tick())
            refused(hq.HQ_E_STATE, lambda: w.get_timers())
            refused(hq.HQ_E_STATE, lambda: w.set_timers(np.array([0], np.uint32), np.zeros(1, hq.TIMER_DTYPE)))
            for bad in ((0, 1, 1), (32768, 1, 1), (4, 0, 1), (4, 65536, 1), (4, 1, 2)):
                refused(hq.HQ_E_INVAL, lambda: w.set_tick_config(*bad))
            refused(hq.HQ_E_STATE, lambda: w.tick())                  # (a refused config sets none)
            w.set_tick_config(E, H, True, SEED)
        model = tm.TickModel(E, H, True, SEED)
        tick_all(workers, model, groups)
        for w in workers.values():
            w.stop_groups(np.array([2], np.uint32))
        groups[2] = None
        tick_all(workers, model, groups, contact=[1])
        live = np.array([0, 1, 3], np.uint32)
        for name, w in workers.items():
            before = w.get_timers(live).tobytes()

            def refused(code, fn):
                with pytest.raises(hq.HQError) as e:
                    fn()
                assert e.value.code == code, name
                assert hq.lib.hq_worker_last_error(w.h).decode() != ""
                assert w.get_timers(live).tobytes() == before, name

            refused(hq.HQ_E_INVAL, lambda: w.tick(np.array([1, 4], np.uint32)))      # out of range
            refused(hq.HQ_E_INVAL, lambda: w.tick(np.array([1, 2], np.uint32)))      # vacant
            refused(hq.HQ_E_INVAL, lambda: w.get_timers(np.array([0, 2], np.uint32)))
            refused(hq.HQ_E_INVAL, lambda: w.get_timers())                            # 0 .. 3 holds a vacancy
            one = np.array([1], np.uint32)
            for bad in ((2 * E, 0, 0), (0, H, 0), (0, 0, E - 1), (0, 0, 2 * E), (0, 0, 0, 1)):
                t = np.array([bad + (0,) * (4 - len(bad))], hq.TIMER_DTYPE)
                refused(hq.HQ_E_INVAL, lambda: w.set_timers(one, t))
            two = np.zeros(2, hq.TIMER_DTYPE)
            refused(hq.HQ_E_INVAL, lambda: w.set_timers(np.array([0, 2], np.uint32), two))   # vacant
            refused(hq.HQ_E_INVAL, lambda: w.set_timers(np.array([0, 4], np.uint32), two))   # out of range
            refused(hq.HQ_E_INVAL, lambda: w.set_timers(np.array([1, 1], np.uint32), two))   # twice
            # one bad entry refuses the whole list
            mixed = np.array([(1, 1, 0, 0), (0, H, 0, 0)], hq.TIMER_DTYPE)
            refused(hq.HQ_E_INVAL, lambda: w.set_timers(np.array([0, 1], np.uint32), mixed))
            lib, inval = hq.lib, hq.HQ_E_INVAL
            out = hq.TickOutput()
            vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
            assert lib.hq_worker_tick(w.h, 0, None, None) == inval
            assert lib.hq_worker_tick(w.h, 1, None, ctypes.byref(out)) == inval
            assert lib.hq_worker_set_tick_config(w.h, None) == inval
            assert lib.hq_worker_get_timers(w.h, 1, vp(one), None) == inval
            assert lib.hq_worker_set_timers(w.h, 1, vp(one), None) == inval
            assert lib.hq_worker_get_timers(w.h, 0, None, None) == hq.HQ_OK
            assert lib.hq_worker_set_timers(w.h, 0, None, None) == hq.HQ_OK
            assert w.get_timers(live).tobytes() == before, name
        tick_all(workers, model, groups)                              # nothing was ticked or lost
        for w in workers.values():
            assert w.readback_count() == 0
    finally:
        close_all(workers)
