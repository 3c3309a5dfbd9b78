"""hq_worker_config_changes on device and host workers (dragonboat_amd/csrc/hq_config.hip,
hq_worker_lists.cpp): membership changes applied where the quorum state lives. Expected values are the
Python restatement of raft.go:1136-1199, 1540-1559 (tests/config_ref.py) over Worker.get_group,
the reference's tables (tests/golden/config_change_kats.json) and, for the steps after a change,
a fresh oracle (oracle/qref_step.c) built from the restatement's post-change state."""
import ctypes

import numpy as np
import pytest

import config_ref as ref
import heartbeat_ref as hb
import heartbeat_wire_ref as hw
import step_random as sr
import step_scenarios as sc
from step_harness import OracleBackend, WorkerBackend, same_step

pytestmark = pytest.mark.gpu
MODES = [True, False]
MODE_IDS = ["device", "host"]
LIMIT = {True: 16, False: 64}


def snapshot(w, cids):
    return {c: ref.group_of(w, c) for c in cids}


def may_hold(g, node_id):
    """Whether get_group leaves open that a voter holds a recorded vote or ack (fallback (c))."""
    role = {m["node_id"]: m["role"] for m in g["members"]}.get(node_id)
    return role in (ref.REMOTE, ref.WITNESS) and \
        (g["state"] == ref.CANDIDATE or any(r["n_confirmed"] for r in g["reads"]))


def check_call(w, on_device, cids, changes, n_max=8, acked=None, open_acks=False):
    """One call against the model: status, commits, counters, and get_group of EVERY group
    afterwards. acked: handle -> the node ids known to hold a vote or ack; open_acks: where
    get_group cannot tell (random worlds), a removal's FALLBACK is taken as the member holding one.
    Returns (the call's result, the groups afterwards)."""
    before = snapshot(w, cids)
    by_handle = {h: before[c] for h, c in enumerate(cids)}
    assert not ref.invalid(by_handle, changes)
    got = w.config_changes(changes)
    want_groups, want_status, want_commits = dict(before), [], []
    for i, (h, t, nid) in enumerate(changes):
        g = by_handle[h]
        s, g2, c = ref.apply(g, t, nid, n_max, LIMIT[on_device], (acked or {}).get(h, ()))
        if open_acks and s == ref.APPLIED and t == ref.REMOVE_NODE and may_hold(g, nid) and \
                int(got["status"][i]) == ref.FALLBACK:
            s, g2, c = ref.apply(g, t, nid, n_max, LIMIT[on_device], {nid})
        want_status.append(s)
        want_groups[cids[h]] = g2
        if c is not None:
            want_commits.append((cids[h], c))
    assert got["status"].tolist() == want_status
    assert [(int(x["cluster_id"]), int(x["committed"])) for x in got["commits"]] == want_commits
    for k, v in (("n_applied", ref.APPLIED), ("n_noop", ref.NOOP), ("n_fallback", ref.FALLBACK),
                 ("n_suspended", ref.SUSPENDED)):
        assert got[k] == want_status.count(v), k
    assert (got["gpu_ns"] > 0) == bool(on_device and changes)
    after = snapshot(w, cids)
    for c in cids:
        assert after[c] == want_groups[c], c
    return got, after


def same_output(a, b):
    assert a["status"].tolist() == b["status"].tolist()
    assert a["commits"].tolist() == b["commits"].tolist()
    for k in ("n_applied", "n_noop", "n_fallback", "n_suspended"):
        assert a[k] == b[k]


def model_tuple(g):
    """A model group as the backends' state() reports one."""
    return (g["term"], g["state"], g["committed"], g["last_index"], g["term_start"],
            ref.member_tuples(g), [(r["index"], r["from"], r["ctx"], r["n_confirmed"])
                                   for r in g["reads"]])


def oracle_from(groups):
    """A fresh oracle holding the model's groups (add_group carries no reads and no votes)."""
    o = OracleBackend()
    for c, g in groups.items():
        o.add_group(c, g["node_id"], g["term"], g["state"], g["committed"], g["last_index"],
                    g["term_start"], ref.member_tuples(g))
    return o


# ------------------------------------------------------------------ the reference's tables ----
@pytest.mark.parametrize("on_device", MODES, ids=MODE_IDS)
def test_reference_tables(hq, on_device):
    cases = ref.kats()
    with hq.Worker(0, 8, on_device=on_device) as w:
        cids = []
        for c in cases:
            g = c["group"]
            w.add_group(g["cluster_id"], g["node_id"], g["term"], g["state"], g["committed"],
                        g["last_index"], g["term_start"], [tuple(m) for m in g["members"]])
            cids.append(g["cluster_id"])
        for k in range(max(len(c["steps"]) for c in cases)):
            valid = [(h, c["steps"][k]) for h, c in enumerate(cases)
                     if k < len(c["steps"]) and not c["steps"][k].get("inval")]
            got, after = check_call(w, on_device, cids, [(h, s["type"], s["node_id"]) for h, s in valid])
            for i, (h, s) in enumerate(valid):
                assert int(got["status"][i]) == s["status"], cases[h]["name"]
                assert ref.member_tuples(after[cids[h]]) == [tuple(m) for m in s["members"]]
                assert after[cids[h]]["suspended"] == s.get("suspended", 0)
                commits = [int(x["committed"]) for x in got["commits"] if int(x["cluster_id"]) == cids[h]]
                assert commits == ([] if s["commit"] is None else [s["commit"]]), cases[h]["name"]
            for h, c in enumerate(cases):
                if k < len(c["steps"]) and c["steps"][k].get("inval"):
                    s = c["steps"][k]
                    before = snapshot(w, cids)
                    with pytest.raises(hq.HQError) as e:
                        w.config_changes([(h, s["type"], s["node_id"])])
                    assert e.value.code == hq.HQ_E_INVAL
                    assert snapshot(w, cids) == before


# ------------------------------------------------------------------ random worlds ------------
def random_changes(rng, groups_now, cids):
    """One random change in a random subset of the groups, all four types, members, non-members
    and observers as targets, the handles shuffled; never an invalid list."""
    changes = []
    for h in rng.permutation(len(cids)):
        if rng.random() > 0.6 and len(cids) > 1:
            continue
        g = groups_now[cids[int(h)]]
        by_role = {r: [m["node_id"] for m in g["members"] if m["role"] == r] for r in (0, 1, 2)}
        t = int(rng.integers(0, 4))
        fresh = 200 + int(rng.integers(0, 50))
        if t == ref.REMOVE_NODE:
            ids = [m["node_id"] for m in g["members"]]
            nid = fresh if rng.random() < 0.15 else int(rng.choice(ids))
        else:
            same = by_role[{ref.ADD_NODE: 0, ref.ADD_OBSERVER: 1, ref.ADD_WITNESS: 2}[t]]
            pool = [fresh, fresh] + same[:1]
            if t == ref.ADD_NODE:
                pool += by_role[1] * 2                   # promotions
            nid = int(rng.choice(pool))
        changes.append((int(h), t, nid))
    return changes


@pytest.mark.parametrize("G", [1, 63, 64, 65, 2000])
def test_random_worlds_and_continuation(hq, G):
    rng = np.random.default_rng(7000 + G)
    groups = sr.random_groups(rng, G)
    cids = [g[0] for g in groups]
    workers = [hq.Worker(0, 8, on_device=d) for d in MODES]
    try:
        backs = [WorkerBackend(hq, worker=w, seed=5) for w in workers]
        for b in backs:
            for g in groups:
                b.add_group(*g[:8])
        ctx_seq = [0]

        def steps(first, count, oracle=None, only=None):
            for s in range(first, first + count):
                per = {}
                for c in (only if only is not None else cids):
                    if rng.random() < 0.85:
                        per[c] = sr.random_events(rng, backs[0].state(c), s + 1, ctx_seq)
                outs = [b.step(per) for b in backs]
                assert all(o["_fallback"] == [] for o in outs)
                if oracle:
                    want = oracle.step(per)
                    for b, got in zip(backs, outs):
                        for c in per:
                            same_step(want, got, c)
                        for c in only:
                            assert b.state(c) == oracle.state(c), (s, c)

        steps(0, 3)
        # an event no worker can take suspends some of the leaders
        node_of = {g[0]: g[1] for g in groups}
        per = {c: [sc.msg(99, node_of[c], backs[0].state(c)[0])] for c in cids
               if backs[0].state(c)[1] == sc.LEADER and rng.random() < 0.1}
        if per:
            for b in backs:
                assert sorted(b.step(per)["_fallback"]) == sorted(per)
        changes = random_changes(rng, snapshot(workers[0], cids), cids)
        results = [check_call(w, d, cids, changes, open_acks=True) for w, d in zip(workers, MODES)]
        same_output(results[0][0], results[1][0])
        assert results[0][1] == results[1][1]
        after = results[0][1]
        if G >= 2000:        # the world holds every outcome
            st = results[0][0]["status"].tolist()
            assert all(st.count(v) > 0 for v in range(4)), [st.count(v) for v in range(4)]
            assert len(results[0][0]["commits"]) > 0
        # three more steps on the changed workers against a fresh oracle holding the model's state
        # (groups with no pending read and no votes beyond the node's own: add_group carries none)
        cont = [c for c in cids if not after[c]["reads"] and not after[c]["suspended"] and
                after[c]["state"] != ref.CANDIDATE]
        oracle = oracle_from({c: after[c] for c in cont})
        for c in cont:
            assert oracle.state(c) == model_tuple(after[c])
        steps(10, 3, oracle, cont)
    finally:
        for w in workers:
            w.close()


# ------------------------------------------------------------------ reads and votes survive ---
def leader5(w, cid=1, extra=()):
    """A leader (node 1, term 2) of remotes 1..5 with everything committed, plus `extra`."""
    mem = [(i, 9, sc.REMOTE, 0) for i in range(1, 6)] + list(extra)
    w.add_group(cid, 1, 2, sc.LEADER, 9, 9, 9, mem)


@pytest.mark.parametrize("on_device", MODES, ids=MODE_IDS)
def test_pending_read_survives_a_removal(hq, on_device):
    """5 voters, a ctx confirmed by slot 3 (node 4); removing slot 1 (node 2) moves that bit to
    slot 2. With 4 voters the quorum is 3: node 4 again changes nothing, node 5 releases."""
    with hq.Worker(0, 8, on_device=on_device) as w:
        leader5(w)
        b = WorkerBackend(hq, worker=w)
        out = b.step({1: [("read", 5, 6), sc.msg(sc.HBRESP, 4, 2, hint=5, high=6)]})
        assert out[1]["ready"] == [] and b.state(1)[6] == [(9, 0, (5, 6), 1)]
        got, after = check_call(w, on_device, [1], [(0, ref.REMOVE_NODE, 2)], acked={0: {4}})
        assert got["status"].tolist() == [ref.APPLIED] and after[1]["reads"][0]["n_confirmed"] == 1
        out = b.step({1: [sc.msg(sc.HBRESP, 4, 2, hint=5, high=6)]})
        assert out[1]["ready"] == [] and b.state(1)[6] == [(9, 0, (5, 6), 1)]
        out = b.step({1: [sc.msg(sc.HBRESP, 5, 2, hint=5, high=6)]})
        assert out[1]["ready"] == [(9, 5, 6)] and b.state(1)[6] == []


@pytest.mark.parametrize("on_device", MODES, ids=MODE_IDS)
def test_pending_read_survives_an_insertion(hq, on_device):
    """Remotes 1..4 and witness 5 (slot 4), which confirmed a ctx; a new remote takes slot 4 and
    the witness's bit moves to slot 5. With 6 voters the quorum is 4: node 2, then node 5 again
    (no new ack), then node 3 releases."""
    with hq.Worker(0, 8, on_device=on_device) as w:
        mem = [(i, 9, sc.REMOTE, 0) for i in range(1, 5)] + [(5, 9, sc.WITNESS, 0)]
        w.add_group(1, 1, 2, sc.LEADER, 9, 9, 9, mem)
        b = WorkerBackend(hq, worker=w)
        out = b.step({1: [("read", 5, 6), sc.msg(sc.HBRESP, 5, 2, hint=5, high=6)]})
        assert out[1]["ready"] == []
        got, after = check_call(w, on_device, [1], [(0, ref.ADD_NODE, 6)], acked={0: {5}})
        assert got["status"].tolist() == [ref.APPLIED]
        assert ref.member_tuples(after[1])[-1] == (6, 0, sc.REMOTE, 0)
        out = b.step({1: [sc.msg(sc.HBRESP, 2, 2, hint=5, high=6),
                          sc.msg(sc.HBRESP, 5, 2, hint=5, high=6)]})
        assert out[1]["ready"] == [] and b.state(1)[6] == [(9, 0, (5, 6), 2)]
        out = b.step({1: [sc.msg(sc.HBRESP, 3, 2, hint=5, high=6)]})
        assert out[1]["ready"] == [(9, 5, 6)]


@pytest.mark.parametrize("on_device", MODES, ids=MODE_IDS)
def test_votes_survive_a_removal(hq, on_device):
    """A candidate of 5 with a grant from slot 2 (node 3); removing slot 1 (node 2) moves it to
    slot 1. With 4 voters the quorum is 3: node 3 again decides nothing, node 4's grant elects."""
    with hq.Worker(0, 8, on_device=on_device) as w:
        w.add_group(1, 1, 3, sc.CANDIDATE, 9, 9, 5, [(i, 0, sc.REMOTE, 0) for i in range(1, 6)])
        b = WorkerBackend(hq, worker=w)
        assert b.step({1: [sc.msg(sc.VRESP, 3, 3)]})[1]["states"] == []
        got, _ = check_call(w, on_device, [1], [(0, ref.REMOVE_NODE, 2)], acked={0: {1, 3}})
        assert got["status"].tolist() == [ref.APPLIED]
        assert b.step({1: [sc.msg(sc.VRESP, 3, 3)]})[1]["states"] == []
        assert b.step({1: [sc.msg(sc.VRESP, 4, 3)]})[1]["states"] == [(3, sc.LEADER, sc.R_VOTE)]


# ------------------------------------------------------------------ fallbacks ----------------
def expect_fallback(hq, w, on_device, cids, h, change, acked=None, n_max=8):
    """The change is a FALLBACK: the group untouched but suspended, its next step's events
    deferred, and set_group resumes it."""
    cid = cids[h]
    before = ref.group_of(w, cid)
    got, after = check_call(w, on_device, cids, [change], n_max=n_max, acked=acked)
    assert got["status"].tolist() == [ref.FALLBACK] and got["n_fallback"] == 1
    assert after[cid] == dict(before, suspended=1)
    b = WorkerBackend(hq, worker=w)
    out = b.step({cid: [("propose", 1), ("propose", 1)]})
    assert out[cid]["deferred"] == [0, 1]
    assert check_call(w, on_device, cids, [change], n_max=n_max)[0]["status"].tolist() == [ref.SUSPENDED]
    w.set_group(cid, before["node_id"], before["term"], before["state"], before["committed"],
                before["last_index"], before["term_start"], ref.member_tuples(before))
    assert ref.group_of(w, cid)["suspended"] == 0
    out = b.step({cid: [("campaign",)] if before["state"] != ref.LEADER else [("propose", 1)]})
    assert out[cid]["deferred"] == []
    now = ref.group_of(w, cid)
    assert now["last_index"] == before["last_index"] + 1 if before["state"] == ref.LEADER \
        else now["state"] == ref.CANDIDATE


@pytest.mark.parametrize("on_device", MODES, ids=MODE_IDS)
def test_fallback_at_the_voting_limit(hq, on_device):
    with hq.Worker(0, 3, on_device=on_device) as w:
        cids = [1, 2, 3]
        for c in cids:
            w.add_group(c, 1, 2, sc.LEADER, 9, 9, 9, [(1, 9, 0, 0), (2, 9, 0, 0), (3, 9, 2, 0), (4, 9, 1, 0)])
        expect_fallback(hq, w, on_device, cids, 0, (0, ref.ADD_NODE, 7), n_max=3)
        expect_fallback(hq, w, on_device, cids, 1, (1, ref.ADD_WITNESS, 7), n_max=3)
        expect_fallback(hq, w, on_device, cids, 2, (2, ref.ADD_NODE, 4), n_max=3)   # a promotion


@pytest.mark.parametrize("on_device", MODES, ids=MODE_IDS)
def test_fallback_at_the_member_limit(hq, on_device):
    n = LIMIT[on_device]
    with hq.Worker(0, 8, on_device=on_device) as w:
        mem = [(1, 9, 0, 0), (2, 9, 0, 0), (3, 9, 0, 0)] + [(i, 0, 1, 0) for i in range(4, n + 1)]
        w.add_group(1, 1, 2, sc.LEADER, 9, 9, 9, mem[:-1])
        got, after = check_call(w, on_device, [1], [(0, ref.ADD_OBSERVER, n)])   # the last that fits
        assert got["status"].tolist() == [ref.APPLIED] and len(after[1]["members"]) == n
        expect_fallback(hq, w, on_device, [1], 0, (0, ref.ADD_OBSERVER, 100))


@pytest.mark.parametrize("state", [sc.LEADER, sc.FOLLOWER], ids=["leader", "follower"])
@pytest.mark.parametrize("on_device", MODES, ids=MODE_IDS)
def test_fallback_removing_the_node_itself(hq, on_device, state):
    with hq.Worker(0, 8, on_device=on_device) as w:
        w.add_group(1, 1, 2, state, 9, 9, 9, [(2, 9, 0, 0), (1, 9, 0, 0), (3, 9, 0, 0)])
        expect_fallback(hq, w, on_device, [1], 0, (0, ref.REMOVE_NODE, 1))


@pytest.mark.parametrize("kind", ["granted", "rejected", "confirmed"])
@pytest.mark.parametrize("on_device", MODES, ids=MODE_IDS)
def test_fallback_removing_a_voter_with_a_recorded_answer(hq, on_device, kind):
    with hq.Worker(0, 8, on_device=on_device) as w:
        b = WorkerBackend(hq, worker=w)
        if kind == "confirmed":
            leader5(w)
            b.step({1: [("read", 5, 6), sc.msg(sc.HBRESP, 4, 2, hint=5, high=6)]})
            target = 4
        else:
            w.add_group(1, 1, 3, sc.CANDIDATE, 9, 9, 5, [(i, 0, sc.REMOTE, 0) for i in range(1, 6)])
            b.step({1: [sc.msg(sc.VRESP, 3, 3, reject=int(kind == "rejected"))]})
            target = 3
        expect_fallback(hq, w, on_device, [1], 0, (0, ref.REMOVE_NODE, target), acked={0: {target}})


# ------------------------------------------------------------------ 8 -> 9 members ------------
@pytest.mark.parametrize("ctype", [ref.ADD_OBSERVER, ref.ADD_NODE], ids=["observer", "remote"])
def test_ninth_member_is_seen_by_the_next_step(hq, ctype):
    """A device worker whose groups all have 8 members steps with 8 member slots in registers; a
    ninth member must move it to the 16-slot kernels. The step after the change carries events
    from the new member and from the member now last in the pool."""
    with hq.Worker(0, 8, on_device=True) as w:
        mem = [(i, 5, sc.REMOTE, 0) for i in range(1, 6)] + [(i, 0, sc.OBSERVER, 0) for i in (6, 7, 8)]
        mem[0] = (1, 9, sc.REMOTE, 0)
        w.add_group(1, 1, 2, sc.LEADER, 5, 9, 4, mem)
        b = WorkerBackend(hq, worker=w)
        b.step({1: [sc.msg(sc.HBRESP, 2, 2)]})            # the 8-slot kernels have run
        got, after = check_call(w, True, [1], [(0, ctype, 9)])
        assert got["status"].tolist() == [ref.APPLIED] and len(after[1]["members"]) == 9
        o = oracle_from(after)
        for per in ({1: [sc.msg(sc.RREP, 9, 2, 9), sc.msg(sc.RREP, 8, 2, 7), sc.msg(sc.RREP, 2, 2, 8)]},
                    {1: [sc.msg(sc.HBRESP, 9, 2), sc.msg(sc.RREP, 3, 2, 9), ("check_quorum",)]}):
            want, have = o.step(per), b.step(per)
            same_step(want, have, 1)
            assert b.state(1) == o.state(1)


# ------------------------------------------------------------------ relocation ----------------
@pytest.mark.parametrize("on_device", MODES, ids=MODE_IDS)
def test_relocation_leaves_the_neighbours_alone(hq, on_device):
    """Groups added back to back have full member ranges: the first insertion moves the group to
    the pool's end (with room for one more), the second fits in place, the third moves again."""
    with hq.Worker(0, 8, on_device=on_device) as w:
        rng = np.random.default_rng(11)
        groups = sr.random_groups(rng, 9)
        cids = [g[0] for g in groups]
        for g in groups:
            w.add_group(*g[:8])
        b = WorkerBackend(hq, worker=w)
        b.step({c: [("propose", 1)] for c in cids})
        for k, t in enumerate([ref.ADD_OBSERVER, ref.ADD_OBSERVER, ref.ADD_OBSERVER, ref.REMOVE_NODE,
                               ref.ADD_OBSERVER, ref.ADD_OBSERVER]):
            changes = [(h, t, 300 + k if t != ref.REMOVE_NODE else 300) for h in (1, 4, 5, 8)]
            got, _ = check_call(w, on_device, cids, changes)
            assert got["status"].tolist() == [ref.APPLIED] * 4
        o = oracle_from({c: g for c, g in snapshot(w, cids).items()
                         if g["state"] != ref.CANDIDATE and not g["reads"]})
        per = {c: [sc.msg(sc.RREP, 304, o.state(c)[0], o.state(c)[3]), ("propose", 2)] for c in o.groups}
        want, have = o.step(per), b.step(per)
        for c in per:
            same_step(want, have, c)
            assert b.state(c) == o.state(c)


# ------------------------------------------------------------------ routes --------------------
@pytest.mark.parametrize("on_device", MODES, ids=MODE_IDS)
def test_routes_move_with_the_members(hq, on_device):
    with hq.Worker(0, 8, on_device=on_device) as w:
        rng = np.random.default_rng(21)
        groups = [g for g in sr.random_groups(rng, 40) if g[3] == sc.LEADER and len(g[7]) >= 3][:12]
        cids = [g[0] for g in groups]
        for g in groups:
            w.add_group(*g[:8])
        routes = hw.random_routes(rng, len(cids), 5, none=0.0)
        w.set_heartbeat_routes(0, routes)
        hw.run_and_check(hq, hw.World(w, cids), None, routes, 5)      # the column is on the device
        for t in (ref.REMOVE_NODE, ref.ADD_NODE, ref.ADD_OBSERVER):
            changes, before = [], snapshot(w, cids)
            for h, c in enumerate(cids):
                if h % 3 == 2:
                    continue
                others = [m["node_id"] for m in before[c]["members"][:-1] if m["node_id"] != before[c]["node_id"]]
                if t == ref.REMOVE_NODE and not others:
                    continue
                changes.append((h, t, others[len(others) // 2] if t == ref.REMOVE_NODE else 400 + t))
            got, _ = check_call(w, on_device, cids, changes)
            for (h, _, nid), s in zip(changes, got["status"].tolist()):
                routes[h] = ref.routes_after(routes[h].tolist(), before[cids[h]], t, nid, s)
            assert ref.APPLIED in got["status"].tolist()
            world = hw.World(w, cids)
            hw.run_and_check(hq, world, None, routes, 5)
            listed = [hb.worker_group(w, c) for c in cids]
            hb.assert_same(w.heartbeats(), hb.compact(hq, listed)[0])
        # routes set after the changes go by the new list
        routes = hw.random_routes(rng, len(cids), 5)
        w.set_heartbeat_routes(0, routes)
        hw.run_and_check(hq, hw.World(w, cids), None, routes, 5)


# ------------------------------------------------------------------ ordering with other calls -
@pytest.mark.parametrize("on_device", MODES, ids=MODE_IDS)
def test_set_group_is_flushed_first_and_step_output_survives(hq, on_device):
    with hq.Worker(0, 8, on_device=on_device) as w:
        leader5(w, 1)
        leader5(w, 2)
        res = w.step(np.array([0, 1], np.uint32), np.array([0, 1, 2], np.uint64),
                     np.array([(hq.EV_PROPOSE, 0, 0, 0, 1, 0, 0, 0, 0)] * 2, hq.EVENT_DTYPE), copy=False)
        kept = {k: np.array(v) for k, v in res.items() if isinstance(v, np.ndarray)}
        # queued, not yet uploaded: node 7 exists only in the new member list
        w.set_group(1, 1, 2, sc.LEADER, 9, 12, 9, [(1, 12, 0, 0), (2, 9, 0, 0), (7, 12, 0, 1)])
        got = w.config_changes([(0, ref.REMOVE_NODE, 2)])
        assert got["status"].tolist() == [ref.APPLIED]
        assert [(int(x["cluster_id"]), int(x["committed"])) for x in got["commits"]] == [(1, 12)]
        g = ref.group_of(w, 1)
        assert ref.member_tuples(g) == [(1, 12, 0, 0), (7, 12, 0, 1)] and g["committed"] == 12
        for k, v in kept.items():                       # the step's buffers are not the call's
            np.testing.assert_array_equal(res[k], v, err_msg=k)


@pytest.mark.parametrize("on_device", MODES, ids=MODE_IDS)
def test_invalid_lists_change_nothing(hq, on_device):
    with hq.Worker(0, 8, on_device=on_device) as w:
        cids = [1, 2, 3]
        for c in cids:
            leader5(w, c, extra=[(6, 0, sc.WITNESS, 0), (7, 0, sc.OBSERVER, 0)])
        WorkerBackend(hq, worker=w).step({c: [("propose", 1)] for c in cids})
        before = snapshot(w, cids)
        good = (0, ref.REMOVE_NODE, 2)
        bad_lists = [[good, (3, ref.ADD_NODE, 9)],            # an unknown handle
                     [good, (1, ref.ADD_NODE, 9), (0, ref.ADD_NODE, 9)],   # a group listed twice
                     [good, (1, 4, 9)],                       # an unknown type
                     [good, (1, ref.REMOVE_NODE, 0)],         # node_id 0
                     [good, (1, ref.ADD_NODE, 6)],            # a witness cannot be promoted
                     [good, (1, ref.ADD_OBSERVER, 2)],        # a member in another role
                     [good, (1, ref.ADD_WITNESS, 7)],
                     [good, (1, ref.ADD_OBSERVER, 6)]]
        by_handle = {h: before[c] for h, c in enumerate(cids)}
        for bad in bad_lists:
            assert ref.invalid(by_handle, bad)
            with pytest.raises(hq.HQError) as e:
                w.config_changes(bad)
            assert e.value.code == hq.HQ_E_INVAL, bad
            assert snapshot(w, cids) == before, bad
        out = hq.ConfigOutput()
        one = np.array([good], hq.CONFIG_CHANGE_DTYPE)
        assert hq.lib.hq_worker_config_changes(w.h, 1, None, ctypes.byref(out)) == hq.HQ_E_INVAL
        assert hq.lib.hq_worker_config_changes(w.h, 1, one.ctypes.data, None) == hq.HQ_E_INVAL
        assert hq.lib.hq_worker_config_changes(None, 1, one.ctypes.data, ctypes.byref(out)) == hq.HQ_E_INVAL
        assert hq.lib.hq_worker_config_changes(w.h, 0, None, ctypes.byref(out)) == hq.HQ_OK
        assert snapshot(w, cids) == before
        got, _ = check_call(w, on_device, cids, [good, (1, ref.ADD_NODE, 7)])     # still usable
        assert got["status"].tolist() == [ref.APPLIED, ref.APPLIED]


def test_no_readback(hq):
    """A device worker whose mirror is stale applies the changes without copying the state back."""
    with hq.Worker(0, 8, on_device=True) as w:
        rng = np.random.default_rng(31)
        groups = sr.random_groups(rng, 200)
        for g in groups:
            w.add_group(*g[:8])
        handles = np.arange(200, dtype=np.uint32)
        ev = np.array([(hq.EV_PROPOSE, 0, 0, 0, 1, 0, 0, 0, 0)] * 200, hq.EVENT_DTYPE)
        w.step(handles, np.arange(201, dtype=np.uint64), ev)          # the mirror is stale now
        assert w.readback_count() == 0
        for t in (ref.ADD_OBSERVER, ref.REMOVE_NODE, ref.ADD_NODE):
            got = w.config_changes([(h, t, 500) for h in range(0, 200, 3)])
            assert got["n_applied"] + got["n_noop"] > 0
            w.step(handles, np.arange(201, dtype=np.uint64), ev)
            w.heartbeats()
        assert w.readback_count() == 0
        w.get_group(groups[0][0])
        assert w.readback_count() == 1
    with hq.Worker(0, 8) as w:
        leader5(w)
        w.config_changes([(0, ref.ADD_NODE, 9)])
        w.get_group(1)
        assert w.readback_count() == 0
