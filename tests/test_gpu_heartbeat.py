"""hq_worker_heartbeats on a device worker (dragonboat_amd/csrc/hq_heartbeat.hip): the leader
heartbeat broadcast read from the resident state. Expected values are the Python restatement of
raft.go:812-848 (tests/heartbeat_ref.py) over Worker.get_group, which reads the state back through
hq_dstep_get and never touches the heartbeat kernels."""
import ctypes

import numpy as np
import pytest

import heartbeat_ref as ref
import step_random as sr
import step_scenarios as sc
from step_harness import WorkerBackend

pytestmark = pytest.mark.gpu
KATS = ref.kats()
SIZES = [1, 63, 64, 65, 255, 257, 5000]     # the wave edge, the workgroup edge, several scan tiles


def wide_group(rng, cid):
    """A leader with 16 members (the device path's most): 6 remotes, 2 witnesses, 8 observers, in a
    random list order, every match around the committed index."""
    roles = [sc.REMOTE] * 6 + [sc.WITNESS] * 2 + [sc.OBSERVER] * 8
    last, committed = 120, 115
    mem = [(i + 1, last if i == 0 else int(rng.integers(committed - 3, last + 1)), r, 0)
           for i, r in enumerate(roles)]
    mem = [mem[k] for k in rng.permutation(16)]
    return (cid, 1, 3, sc.LEADER, committed, last, 110, mem, None)


def random_world(rng, G):
    """G groups: tests/step_random.py's (3/5/7 voters, witnesses, observers; leaders, followers,
    candidates) and a few 16-member leaders."""
    wide = 1 if G == 1 else min(4, G // 8)
    groups = sr.random_groups(rng, G - wide) if G > wide else []
    return groups + [wide_group(rng, 1 + len(groups) + k) for k in range(wide)]


def step_world(hq, rng, workers, groups, steps):
    """The same random steps on every worker (driven by the first one's state), then an event no
    worker can take on some of the leaders, which suspends them."""
    backs = [WorkerBackend(hq, worker=w, seed=3) for w in workers]
    for b in backs:
        b.cids = [g[0] for g in groups]
    ctx_seq = [0]
    for s in range(steps):
        per = {}
        for g in groups:
            if rng.random() < 0.85:
                per[g[0]] = sr.random_events(rng, backs[0].state(g[0]), s + 1, ctx_seq)
        for b in backs:
            assert b.step(per)["_fallback"] == []
    per = {}
    for g in groups:
        st = backs[0].state(g[0])
        if st[1] == sc.LEADER and rng.random() < 0.15:
            per[g[0]] = [sc.msg(99, g[1], st[0])]           # an unknown message type: fallback
    if per:
        for b in backs:
            assert sorted(b.step(per)["_fallback"]) == sorted(per)
    return per


def reference(hq, w, cids):
    """The compact output and the messages wanted for the listed clusters, from get_group."""
    seen = {}
    for c in cids:
        if c not in seen:
            seen[c] = ref.worker_group(w, c)
    listed = [seen[c] for c in cids]
    hb, msgs = ref.compact(hq, listed)
    return listed, hb, msgs


def check_list(hq, w, handles, cids):
    listed, want, want_msgs = reference(hq, w, cids)
    got = w.heartbeats(handles)
    ref.assert_same(got, want)
    msgs = hq.heartbeats_expand(got, *ref.columns(listed, cids))
    assert len(msgs) == len(want_msgs)
    for f in ("to", "commit", "hint", "hint_high"):
        np.testing.assert_array_equal(msgs[f], want_msgs[f], err_msg=f)
    np.testing.assert_array_equal(msgs["cluster_id"], np.repeat(
        np.array(cids, np.uint64), [bin(int(x) & 0xFFFF).count("1") for x in got["words"]]))
    return got, listed


def add_kat(w, case):
    g = case["group"]
    h = w.add_group(g["cluster_id"], g["node_id"], g["term"], sc.LEADER, g["committed"],
                    g["last_index"], g["term_start"], [(i, m, r, 0) for i, m, r in g["members"]])
    return h


def test_reference_tables_on_device(hq):
    """The reference's tables: the groups added to a device worker, the ctx made pending by a local
    ReadIndex."""
    with hq.Worker(0, 8, on_device=True) as w:
        handles = [add_kat(w, c) for c in KATS]
        b = WorkerBackend(hq, worker=w)
        reads = {c["group"]["cluster_id"]: [("read", c["ctx"][0], c["ctx"][1])]
                 for c in KATS if tuple(c["ctx"]) != (0, 0)}
        out = b.step(reads)
        assert all(out[cid]["ready"] == [] and out[cid]["dropped"] == [] for cid in reads)
        cids = [c["group"]["cluster_id"] for c in KATS]
        got, listed = check_list(hq, w, None, cids)
        assert got["n_messages"] == sum(len(c["want"]) for c in KATS)
        msgs = hq.heartbeats_expand(got, *ref.columns(listed, cids))
        want = [(c["group"]["cluster_id"], x["to"], c["group"]["term"], x["commit"], x["hint"],
                 x["hint_high"]) for c in KATS for x in c["want"]]
        assert [tuple(int(m[f]) for f in m.dtype.names) for m in msgs] == want
        assert handles == list(range(len(KATS)))


@pytest.mark.parametrize("G", SIZES)
def test_differential(hq, G):
    rng = np.random.default_rng(1000 + G)
    groups = random_world(rng, G)
    with hq.Worker(0, 8, on_device=True) as w:
        for g in groups:
            w.add_group(*g[:8])
        suspended = step_world(hq, rng, [w], groups, 2 if G > 1000 else 3)
        cids = [g[0] for g in groups]
        got, listed = check_list(hq, w, None, cids)
        if G >= 255:     # the worlds hold every kind of group
            kinds = dict(leader=sum(x[1] == sc.LEADER for x in listed),
                         other=sum(x[1] != sc.LEADER for x in listed),
                         suspended=len(suspended), reads=sum(bool(x[5]) for x in listed),
                         lags=len(got["lags"]), ctxs=len(got["ctxs"]),
                         observers=sum(any(m[2] == sc.OBSERVER for m in x[4]) for x in listed))
            assert all(v > 0 for v in kinds.values()), kinds
            assert any(x[2] and x[1] == sc.LEADER for x in listed)
        # a shuffled subset with repeats
        pick = rng.integers(0, G, max(1, (2 * G) // 3))
        pick = np.concatenate([pick, pick[:max(1, G // 7)]])
        rng.shuffle(pick)
        check_list(hq, w, pick.astype(np.uint32), [cids[int(h)] for h in pick])


def test_boundaries(hq):
    big = (1 << 40) + 5                    # indices above 2^32 stay exact
    rem, obs, wit = sc.REMOTE, sc.OBSERVER, sc.WITNESS
    with hq.Worker(0, 8, on_device=True) as w:
        assert w.heartbeats()["n_messages"] == 0 and len(w.heartbeats()["words"]) == 0
        assert len(w.heartbeats(np.zeros(0, np.uint32))["words"]) == 0
        # 1: match == committed, committed - 1, match > committed; an observer behind whose low 32
        # bits are above the committed index's
        w.add_group(1, 1, 5, sc.LEADER, big, big + 9, big - 2,
                    [(2, big, rem, 0), (1, big + 9, rem, 0), (3, big - 1, rem, 0),
                     (4, big + 1, wit, 0), (5, (1 << 33) + 6, obs, 0)])
        # 2: a ctx of (0, 0) pending; 3: a nonzero ctx pending (witness in, observers out)
        for cid in (2, 3):
            w.add_group(cid, 1, 5, sc.LEADER, 50, 60, 40,
                        [(1, 60, rem, 0), (2, 50, rem, 0), (3, 49, wit, 0), (4, 7, obs, 0),
                         (5, 50, obs, 0)])
        # 4: a single voter with observers; 5: a single voter alone; 6 / 7: not leaders
        w.add_group(4, 9, 2, sc.LEADER, 30, 31, 30, [(8, 29, obs, 0), (9, 31, rem, 0), (7, 31, obs, 0)])
        w.add_group(5, 9, 2, sc.LEADER, 30, 31, 30, [(9, 31, rem, 0)])
        w.add_group(6, 1, 5, sc.FOLLOWER, 50, 60, 40, [(1, 60, rem, 0), (2, 0, rem, 0), (3, 0, rem, 0)])
        w.add_group(7, 1, 5, sc.CANDIDATE, 50, 60, 40, [(1, 60, rem, 0), (2, 0, rem, 0), (3, 0, rem, 0)])
        b = WorkerBackend(hq, worker=w)
        b.step({2: [("read", 0, 0)], 3: [("read", 1 << 63, 0), ("read", 0, (1 << 64) - 1)]})
        assert len(w.get_group(2)[2]) == 1 and len(w.get_group(3)[2]) == 2
        cids = [1, 2, 3, 4, 5, 6, 7]
        got, _ = check_list(hq, w, None, cids)
        assert list(got["words"]) == [
            0x0014001D,                    # to 0, 2, 3, 4; 2 (committed - 1) and the observer behind
            0x000C001E,                    # zero ctx: observers too; 3 (49) and 4 (7) behind
            0x00040006,                    # nonzero ctx: remote and witness only; 3 (49) behind
            0x00010005,                    # the observers of a single voter; 8 (29) behind
            0, 0, 0]
        assert [tuple(int(x) for x in l) for l in got["lags"]] == [
            (0, 2, big - 1), (0, 4, (1 << 33) + 6), (1, 2, 49), (1, 3, 7), (2, 2, 49), (3, 0, 29)]
        # peepCtx: the LAST pending read's ctx
        assert [tuple(int(x) for x in c)[:3] for c in got["ctxs"]] == [(0, (1 << 64) - 1, 2)]
        assert got["n_messages"] == 4 + 4 + 2 + 2 and got["gpu_ns"] > 0


def test_device_and_host_workers_agree(hq):
    rng = np.random.default_rng(77)
    groups = random_world(rng, 300)
    with hq.Worker(0, 8, on_device=True) as d, hq.Worker(0, 8) as h:
        for g in groups:
            d.add_group(*g[:8])
            h.add_group(*g[:8])
        step_world(hq, rng, [d, h], groups, 3)
        pick = rng.integers(0, 300, 500).astype(np.uint32)
        for handles in (None, pick):
            a, b = d.heartbeats(handles), h.heartbeats(handles)
            ref.assert_same(a, b)
            assert len(a["lags"]) > 0 and len(a["ctxs"]) > 0
        assert b["gpu_ns"] == 0


def test_set_group_is_flushed_first(hq):
    with hq.Worker(0, 8, on_device=True) as w:
        mem = [(1, 20, 0, 0), (2, 20, 0, 0), (3, 20, 0, 0)]
        w.add_group(5, 1, 2, sc.FOLLOWER, 20, 20, 18, mem)
        w.add_group(6, 1, 2, sc.LEADER, 20, 20, 18, mem)
        WorkerBackend(hq, worker=w).step({6: [("propose", 1)]})       # the state is on the device
        assert list(w.heartbeats()["words"]) == [0, 0x6]
        w.set_group(5, 1, 3, sc.LEADER, 20, 22, 21, [(1, 22, 0, 0), (2, 19, 0, 0), (3, 20, 0, 0),
                                                     (4, 0, 1, 0)])
        got = w.heartbeats()                                          # no step in between
        assert list(got["words"]) == [0x000A000E, 0x6]
        assert [tuple(int(x) for x in l) for l in got["lags"]] == [(0, 1, 19), (0, 3, 0)]
        check_list(hq, w, None, [5, 6])


def test_step_output_survives(hq):
    rng = np.random.default_rng(5)
    groups = random_world(rng, 200)
    with hq.Worker(0, 8, on_device=True) as w:
        for g in groups:
            w.add_group(*g[:8])
        b = WorkerBackend(hq, worker=w, seed=1)
        ctx_seq = [0]
        per = {g[0]: sr.random_events(rng, b.state(g[0]), 1, ctx_seq) for g in groups}
        (grp, off, ev), _ = b.build_inputs(per)
        views = w.step(grp, off, ev, copy=False)
        lists = [k for k, v in views.items() if isinstance(v, np.ndarray) and len(v)]
        assert len(lists) >= 2, lists
        before = {k: views[k].copy() for k in lists}
        assert w.heartbeats()["n_messages"] > 0
        w.heartbeats(np.arange(200, dtype=np.uint32)[::-1].copy())
        for k in lists:
            np.testing.assert_array_equal(views[k], before[k], err_msg=k)


def test_bad_handle_leaves_the_worker_usable(hq):
    with hq.Worker(0, 8, on_device=True) as w:
        mem = [(1, 20, 0, 0), (2, 19, 0, 0), (3, 20, 0, 0)]
        for cid in (1, 2, 3):
            w.add_group(cid, 1, 2, sc.LEADER, 20, 20, 18, mem)
        good = w.heartbeats()
        for handles in ([0, 3], [7], [1, 2, 0xFFFFFFFF]):
            with pytest.raises(hq.HQError, match="unknown group handle"):
                w.heartbeats(np.array(handles, np.uint32))
        assert hq.lib.hq_worker_heartbeats(w.h, 4, None, ctypes.byref(hq.HeartbeatOutput())) == \
            hq.HQ_E_INVAL                                   # handles 0 .. 3 of 3 groups
        assert hq.lib.hq_worker_heartbeats(w.h, 3, None, None) == hq.HQ_E_INVAL
        assert b"NULL" in hq.lib.hq_worker_last_error(w.h)
        ref.assert_same(w.heartbeats(), good)
        out = WorkerBackend(hq, worker=w).step({2: [sc.msg(sc.RREP, 2, 2, 20)]})
        assert out["_fallback"] == [] and out[2]["committed"] == 20
        check_list(hq, w, np.array([2, 1, 1, 0], np.uint32), [3, 2, 2, 1])


def test_host_worker_member_limit(hq):
    """A host worker may hold a group of more than 16 members, which the word cannot name."""
    with hq.Worker(0, 8) as w:
        w.add_group(1, 1, 2, sc.LEADER, 20, 20, 18,
                    [(1, 20, 0, 0), (2, 19, 0, 0)] + [(10 + i, 5, 1, 0) for i in range(15)])
        w.add_group(2, 1, 2, sc.LEADER, 20, 20, 18, [(1, 20, 0, 0), (2, 19, 0, 0)])
        with pytest.raises(hq.HQError, match="more than 16 members"):
            w.heartbeats()
        got = w.heartbeats(np.array([1], np.uint32))
        assert list(got["words"]) == [0x00020002] and got["n_messages"] == 1
