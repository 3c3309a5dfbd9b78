"""The random world of the received-heartbeat tests: the CPU oracle's groups (lifecycle_model.World),
the received-heartbeat model (hb_received_model), the timer model (tick_model.TickModel) and any
number of workers driven together through rounds of: received heartbeats, a tick with a caller
contact list for some other followers, a step with the tick's events, and leader heartbeats. With
no workers it runs on the CPU alone, which is how the seeds are checked to reach every branch
before a GPU test relies on them (test_hb_received_api.py), and how the same world is run without
the received call to show that the contacts reached the tick."""
import numpy as np

import hb_received_model as hm
import lifecycle_model as lm
import step_random as sr
import step_scenarios as sc
import tick_model as tm
import tick_world as tw

ROUNDS = 30
E, H = 4, 2


EDGE_SIZES = (1, 31, 32, 33, 63, 64, 65, 257, 1025)   # the contact words' and the waves' edges


def spec_group(s):
    """A step_random.random_groups spec as the model's group."""
    return {"term": s[2], "state": s[3], "committed": s[4], "last": s[5], "suspended": False}


def edge_rows(G):
    """G random groups (witnesses and observers among their members) and their received
    heartbeats; every fifth group has none."""
    rng = np.random.default_rng(9000 + G)
    specs = sr.random_groups(rng, G, cid0=100)
    rows = [[] if j % 5 == 3 else hm.random_messages(rng, spec_group(s), members=[m[0] for m in s[7]])
            for j, s in enumerate(specs)]
    return specs, rows


def world_seed(G, cq):
    return 7100 + 31 * G + int(cq)


def apply_to_oracle(oracle, cid, node, after):
    """The oracle's group as the reference leaves it after the received heartbeats: rebuilt from
    its own state with the model's (term, state, committed) and, after a becomeFollower, reset's
    cleared members and reads. Nothing else of a group can change in that path."""
    old = oracle.groups[cid]
    term, state, committed, last, term_start, members, reads = old.state()
    if not after["reset"] and after["committed"] == committed:
        assert (after["term"], after["state"]) == (term, state)
        return
    if after["reset"]:
        members = [(i, last if i == node else 0, role, 0) for i, _m, role, _a in members]
    else:
        assert reads == [] and state == hm.FOLLOWER     # (only a follower's committed moves)
    oracle.groups[cid] = oracle.qref.StepGroup(cid, node, after["term"], after["state"], after["committed"],
                                               last, term_start, members, old.log_terms())


def received_round(hq, wd, rng, cids, cq, seen, share=0.4):
    """One hq_worker_heartbeats_received over a random, shuffled subset of the groups on the model,
    the oracle and every worker. Returns the handles the model marks as in contact."""
    listed = [h for h in range(len(cids)) if rng.random() < share]
    rng.shuffle(listed)
    rows, want_replies, want_results, contact = [], [], [], []
    for h in listed:
        cid = cids[h]
        term, state, committed, last, _ts, members, _reads = wd.oracle.state(cid)
        g = {"term": term, "state": state, "committed": committed, "last": last, "suspended": False}
        msgs = hm.random_messages(rng, g, members=[m[0] for m in members] + [999])
        replies, res, after = hm.handle(g, msgs, cq)
        seen.add(g, replies, res)
        apply_to_oracle(wd.oracle, cid, wd.node_of[cid], after)
        rows.append(msgs)
        want_replies += replies
        want_results.append(res)
        if res["flags"] & hm.CONTACT:
            contact.append(h)
    groups = np.array(listed, np.uint32)
    offsets = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    msgs = np.array([m for r in rows for m in r], hq.HB_RECEIVED_DTYPE)
    got = {}
    for name, w in wd.workers.items():
        got[name] = w.heartbeats_received(groups, offsets, msgs, cq)
        check_output(got[name], want_replies, want_results, name)
        assert (got[name]["gpu_ns"] > 0) == (name == "device") or not len(groups), name
        wd.backs[name].w._cache = None            # (the NoReadback proxy's fetched state is stale)
    if "twin" in got:
        for k in ("replies", "results"):
            assert got["device"][k].tobytes() == got["twin"][k].tobytes(), k
    return contact


def check_output(got, want_replies, want_results, name=""):
    """A Worker.heartbeats_received result against the model's replies and results."""
    rep = got["replies"]
    assert list(zip(rep["type"].tolist(), rep["term"].tolist())) == want_replies, name
    assert not rep["reserved"].any()
    rs = got["results"]
    assert len(rs) == len(want_results), name
    for k in ("term", "commit", "leader", "state", "flags", "n_resets"):
        assert rs[k].tolist() == [r[k] for r in want_results], (name, k)
    for k, v in hm.counts(want_replies, want_results).items():
        assert got[k] == v, (name, k, got[k], v)


def run(hq, workers, streams, G, cq, rounds=ROUNDS, received=True):
    """Returns (seen, elections): what the received calls showed, and the tick's election list of
    every round."""
    seed = world_seed(G, cq)
    rng = np.random.default_rng(seed)
    wd = lm.World(hq, workers, streams)
    seen, elections = hm.Seen(), []
    try:
        specs = sr.random_groups(rng, G)
        cids = [s[0] for s in specs]
        assert wd.start(specs, via_add=True) == list(range(G))
        model = tm.TickModel(E, H, cq, seed)
        for w in workers.values():
            w.set_tick_config(E, H, cq, seed)
        ctx_seq = [0]
        for rnd in range(rounds):
            rx = np.random.default_rng([seed, rnd])          # (the received call's own stream)
            heard = received_round(hq, wd, rx, cids, cq, seen) if received else []
            states = [wd.oracle.state(c) for c in cids]
            groups = [(c, st[0], st[1], False) for c, st in zip(cids, states)]
            others = [h for h, st in enumerate(states) if st[1] != sc.LEADER and h not in set(heard)]
            contact = np.array([h for h in others if rng.random() < 0.25], np.uint32)   # (Replicate's)
            want = model.tick(groups, list(contact) + heard)
            elections.append(want[2])
            got = {}
            for name, w in workers.items():
                got[name] = w.tick(contact)
                tm.check_tick(got[name], want)
                tm.check_timers(w, model, groups)
            if "twin" in got:
                for k in ("check_quorum", "heartbeat", "election"):
                    assert got["device"][k].tobytes() == got["twin"][k].tobytes(), (rnd, k)
            due_cq, due_el = set(want[0]), set(want[2])
            per = {}
            for h, c in enumerate(cids):
                ev = sr.random_events(rng, states[h], rnd + 1, ctx_seq) if rng.random() < 0.4 else []
                ev = tw.with_tick_events(ev, h in due_cq, h in due_el)
                if ev:
                    per[c] = ev
            if per:
                wd.step(per)
            if "twin" in workers:
                hb = np.array(want[1], np.uint32)
                a, b = workers["device"].heartbeats(hb), workers["twin"].heartbeats(hb)
                for k in ("words", "lags", "ctxs"):
                    assert a[k].tobytes() == b[k].tobytes(), (rnd, k)
            # the whole state after the round: every worker against the oracle, device against twin
            for name, b in wd.backs.items():
                b.w._cache = None
                for c in cids:
                    assert b.state(c) == wd.oracle.state(c), (name, rnd, c)
            if "twin" in workers:
                everyone = list(range(G))
                assert lm.snapshot(workers["device"], everyone) == lm.snapshot(workers["twin"], everyone), rnd
        wd.no_readback()
    finally:
        wd.close()
    return seen, elections
