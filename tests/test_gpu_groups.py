"""hq_worker_get_groups / hq_worker_set_groups on device and host workers
(dragonboat_amd/csrc/hq_groups.hip, hq_worker_lists.cpp): the state of listed groups fetched and resumed
where it lives, without a readback. Expected values never come from the new calls: they are
Worker.get_group (the full readback, taken AFTER the new call ran against a stale mirror),
Worker.set_group one group at a time on a twin worker, what the test itself sent (the masks), and
a fresh oracle (oracle/qref_step.c) for the steps after a resume."""
import ctypes

import numpy as np
import pytest

import config_ref as ref
import step_random as sr
import step_scenarios as sc
from step_harness import OracleBackend, WorkerBackend, same_step

pytestmark = pytest.mark.gpu
MODES = [True, False]
MODE_IDS = ["device", "host"]
PER_WORKGROUP = 16          # listed groups per workgroup of the kernels (16 lanes each, 256 lanes)
ARRAYS = ("groups", "members", "member_offsets", "reads", "read_offsets", "granted", "rejected",
          "read_confirmed")


# ------------------------------------------------------------------ helpers -------------------
def raw_step(back, per):
    """One step without WorkerBackend.step's get_group (a readback): the fallback clusters."""
    arrs, _ = back.build_inputs(per)
    return sorted(int(x) for x in back.w.step(*arrs)["fallback_groups"])


class World:
    """The same random groups on `n_dev` device workers and one host worker, after `steps` random
    steps whose events come from the host worker's state (its get_group copies nothing back)."""

    def __init__(self, hq, seed, G, n_dev=1, steps=3, suspend=0):
        self.rng = rng = np.random.default_rng(seed)
        self.groups = sr.random_groups(rng, G)
        self.cids = [g[0] for g in self.groups]
        self.devs = [hq.Worker(0, 8, on_device=True) for _ in range(n_dev)]
        self.host = hq.Worker(0, 8)
        self.bdevs = [WorkerBackend(hq, worker=w, seed=5) for w in self.devs]
        self.bhost = WorkerBackend(hq, worker=self.host, seed=5)
        for b in self.bdevs + [self.bhost]:
            for g in self.groups:
                b.add_group(*g[:8])
        self.ctx_seq = [0]
        for s in range(steps):
            per = {c: sr.random_events(rng, self.bhost.state(c), s + 1, self.ctx_seq)
                   for c in self.cids if rng.random() < 0.85}
            if per:
                self.step_all(per, [])
        self.suspended = []
        if suspend:      # an event no worker can take suspends every suspend-th group that leads
            node_of = {g[0]: g[1] for g in self.groups}
            per = {c: [sc.msg(99, node_of[c], self.bhost.state(c)[0])] for c in self.cids[::suspend]
                   if self.bhost.state(c)[1] == sc.LEADER}
            if per:
                self.step_all(per, sorted(per))
            self.suspended = sorted(per)

    def step_all(self, per, fallback):
        for b in self.bdevs:
            assert raw_step(b, per) == fallback
        assert sorted(self.bhost.step(per)["_fallback"]) == fallback

    def close(self):
        for w in self.devs + [self.host]:
            w.close()


def entry(res, i):
    """Listed group i of a get_groups result as bytes and masks."""
    mo, ro = res["member_offsets"], res["read_offsets"]
    m0, m1, r0, r1 = int(mo[i]), int(mo[i + 1]), int(ro[i]), int(ro[i + 1])
    return (res["groups"][i].tobytes(), res["members"][m0:m1].tobytes(), res["reads"][r0:r1].tobytes(),
            int(res["granted"][i]), int(res["rejected"][i]), res["read_confirmed"][r0:r1].tolist())


def same_output(a, b):
    for k in ARRAYS:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def check_shape(res, n):
    assert len(res["groups"]) == len(res["granted"]) == len(res["rejected"]) == n
    assert len(res["member_offsets"]) == len(res["read_offsets"]) == n + 1
    assert int(res["member_offsets"][0]) == 0 and int(res["read_offsets"][0]) == 0
    assert int(res["member_offsets"][-1]) == len(res["members"])
    assert int(res["read_offsets"][-1]) == len(res["reads"]) == len(res["read_confirmed"])
    assert res["member_offsets"][1:].tolist() == np.cumsum(res["groups"]["n_members"]).tolist()
    assert res["read_offsets"][1:].tolist() == np.cumsum(res["groups"]["n_pending_reads"]).tolist()


def check_against_get_group(w, cids, handles, res):
    """Every listed group against the old path: group record, members in order, reads; and what
    get_group can say about the masks (their popcounts, voting members only, the own vote)."""
    check_shape(res, len(handles))
    old = {}
    for i, h in enumerate(handles):
        cid = cids[int(h)]
        if cid not in old:
            old[cid] = w.get_group(cid)
        g, m, r = old[cid]
        eg, em, er, granted, rejected, conf = entry(res, i)
        assert eg == g.tobytes(), (i, cid)
        assert em == m.tobytes(), (i, cid)
        assert er == r.tobytes(), (i, cid)
        assert [bin(c).count("1") for c in conf] == r["n_confirmed"].tolist(), (i, cid)
        voters = sum(1 << j for j, x in enumerate(m) if int(x["role"]) != sc.OBSERVER)
        for mask in [granted, rejected] + conf:
            assert mask & ~voters == 0, (i, cid)
        assert granted & rejected == 0
        me = [j for j, x in enumerate(m) if int(x["node_id"]) == int(g["node_id"])][0]
        if int(g["state"]) == sc.CANDIDATE:
            assert granted >> me & 1, (i, cid)            # campaign: the own vote (raft.go:1093)
        if int(g["state"]) == sc.LEADER:
            assert granted == 0 and rejected == 0         # becomeLeader -> reset clears r.votes


# ------------------------------------------------------------------ fetch ---------------------
@pytest.mark.parametrize("G", [1, 17, 2000])
def test_fetch_random_worlds(hq, G):
    wd = World(hq, 9000 + G, G)
    try:
        dev, host, rng = wd.devs[0], wd.host, wd.rng
        lists = [None] + [rng.integers(0, G, n).astype(np.uint32)
                          for n in (1, 3, 4, 5, PER_WORKGROUP - 1, PER_WORKGROUP, PER_WORKGROUP + 1)]
        lists.append(rng.permutation(G).astype(np.uint32))
        assert dev.readback_count() == 0
        got = [dev.get_groups(l) for l in lists]
        assert dev.readback_count() == 0               # the mirror is stale and stays so
        assert all(r["gpu_ns"] > 0 for r in got)
        for l, r in zip(lists, got):                   # only now the old path (the readback)
            check_against_get_group(dev, wd.cids, np.arange(G) if l is None else l, r)
        assert dev.readback_count() == 1
        for l, r in zip(lists, got):
            h = host.get_groups(l)
            assert h["gpu_ns"] == 0
            same_output(r, h)
            same_output(r, dev.get_groups(l, copy=False))   # and again, the mirror fresh
        if G >= 2000:      # the world holds pending reads, candidates' votes and acknowledgements
            assert len(got[0]["reads"]) > 0 and got[0]["read_confirmed"].any()
            assert (got[0]["rejected"] != 0).any() and (got[0]["granted"] != 0).any()
        assert host.readback_count() == 0 and dev.readback_count() == 1
    finally:
        wd.close()


# ------------------------------------------------------------------ masks ---------------------
# the list order differs from the pool order: an observer first, the node itself last
MASK_MEMBERS = [(9, sc.OBSERVER), (3, sc.REMOTE), (5, sc.WITNESS), (2, sc.REMOTE), (4, sc.REMOTE),
                (6, sc.REMOTE), (7, sc.REMOTE), (1, sc.REMOTE)]
POS = {nid: i for i, (nid, _) in enumerate(MASK_MEMBERS)}


def bits(*nodes):
    return sum(1 << POS[n] for n in nodes)


@pytest.mark.parametrize("on_device", MODES, ids=MODE_IDS)
def test_exact_masks(hq, on_device):
    """7 voters (quorum 4). The candidate: its own vote, a grant from node 3, rejections from the
    witness 5 and node 4 (a repeated answer of node 3 does not count twice, raft.go:1071-1073). The
    leader: ctx (5, 6) acknowledged by node 3 and the witness, ctx (7, 8) by node 7."""
    with hq.Worker(0, 8, on_device=on_device) as w:
        w.add_group(1, 1, 3, sc.CANDIDATE, 9, 9, 5, [(i, 0, r, 0) for i, r in MASK_MEMBERS])
        w.add_group(2, 1, 2, sc.LEADER, 9, 9, 9, [(i, 9, r, 0) for i, r in MASK_MEMBERS])
        b = WorkerBackend(hq, worker=w)
        assert raw_step(b, {1: [sc.msg(sc.VRESP, 3, 3), sc.msg(sc.VRESP, 5, 3, reject=1),
                                sc.msg(sc.VRESP, 4, 3, reject=1), sc.msg(sc.VRESP, 3, 3, reject=1)],
                            2: [("read", 5, 6), ("read", 7, 8),
                                sc.msg(sc.HBRESP, 3, 2, hint=5, high=6),
                                sc.msg(sc.HBRESP, 5, 2, hint=5, high=6),
                                sc.msg(sc.HBRESP, 7, 2, hint=7, high=8)]}) == []
        r = w.get_groups()
        assert w.readback_count() == 0
        assert r["granted"].tolist() == [bits(1, 3), 0]
        assert r["rejected"].tolist() == [bits(5, 4), 0]
        assert r["read_offsets"].tolist() == [0, 0, 2]
        assert r["read_confirmed"].tolist() == [bits(3, 5), bits(7)]
        assert [(int(x["ctx_low"]), int(x["ctx_high"]), int(x["n_confirmed"])) for x in r["reads"]] == \
            [(5, 6, 2), (7, 8, 1)]
        assert r["groups"]["state"].tolist() == [sc.CANDIDATE, sc.LEADER]
        check_against_get_group(w, [1, 2], [0, 1], r)
        # a repeated and reordered list carries the same masks
        r2 = w.get_groups(np.array([1, 0, 1], np.uint32))
        assert r2["granted"].tolist() == [0, bits(1, 3), 0]
        assert r2["read_confirmed"].tolist() == [bits(3, 5), bits(7)] * 2


# ------------------------------------------------------------------ shapes at the edges -------
BIG = (1 << 33) + 1000          # indexes above 2^32


def edge_world(hq, w):
    """Pool neighbours of 1, 16 and 1 members; 8 pending reads; a suspended group; a group a
    membership change relocates; a group added after the last step. Returns the cluster ids."""
    lead = lambda ids: [(i, BIG + 9, sc.REMOTE, 0) for i in ids]
    w.add_group(1, 7, 2, sc.LEADER, BIG + 9, BIG + 9, BIG + 9, [(7, BIG + 9, sc.REMOTE, 0)])
    w.add_group(2, 1, 2, sc.LEADER, BIG + 5, BIG + 9, BIG + 4,
                [(20 + i, BIG + i, sc.OBSERVER, i & 1) for i in range(8)] +
                [(1, BIG + 9, sc.REMOTE, 0)] + [(i, BIG + i, sc.REMOTE, 1) for i in range(2, 7)] +
                [(i, BIG + i, sc.WITNESS, 0) for i in (7, 8)])
    w.add_group(3, 8, 4, sc.FOLLOWER, BIG, BIG + 2, BIG, [(8, BIG + 2, sc.REMOTE, 1)])
    w.add_group(4, 1, 2, sc.LEADER, BIG + 9, BIG + 9, BIG + 9, lead(range(1, 6)))
    w.add_group(5, 1, 2, sc.LEADER, BIG + 9, BIG + 9, BIG + 9, lead(range(1, 4)))
    w.add_group(6, 1, 2, sc.LEADER, BIG + 9, BIG + 9, BIG + 9, lead(range(1, 4)))
    w.add_group(7, 2, 2, sc.LEADER, BIG + 9, BIG + 9, BIG + 9, lead(range(1, 4)))
    b = WorkerBackend(hq, worker=w)
    per = {c: [("propose", 1)] for c in (1, 2, 6, 7)}
    per[4] = [("read", 100 + k, BIG + k) for k in range(8)] + \
        [sc.msg(sc.HBRESP, 2, 2, hint=103, high=BIG + 3)]
    per[5] = [sc.msg(99, 1, 2)]
    assert raw_step(b, per) == [5]
    got = w.config_changes([(5, ref.ADD_OBSERVER, 50), (6, ref.ADD_NODE, 51)])
    assert got["status"].tolist() == [ref.APPLIED, ref.APPLIED]      # 3 members: both relocate
    w.add_group(8, 3, 6, sc.CANDIDATE, BIG, BIG + 1, BIG - 5,                      # after the last step
                [(1, 0, sc.REMOTE, 0), (2, 0, sc.REMOTE, 0), (3, BIG + 1, sc.REMOTE, 0)])
    return list(range(1, 9))


def test_edge_shapes(hq):
    with hq.Worker(0, 8, on_device=True) as dev, hq.Worker(0, 8) as host:
        cids = edge_world(hq, dev)
        assert edge_world(hq, host) == cids
        handles = np.arange(len(cids))
        n0 = dev.readback_count()            # (add_group after a step reads back: out of scope here)
        r = dev.get_groups()
        assert dev.readback_count() == n0
        g = r["groups"]
        assert g["n_members"].tolist() == [1, 16, 1, 5, 3, 4, 4, 3]
        assert g["n_pending_reads"].tolist() == [0, 0, 0, 8, 0, 0, 0, 0]
        assert g["suspended"].tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
        assert g["last_index"].tolist() == [BIG + 10, BIG + 10, BIG + 2, BIG + 9, BIG + 9, BIG + 10,
                                            BIG + 10, BIG + 1]
        # the 1-member neighbours hold their own member and nothing of the 16-member group's
        assert r["member_offsets"].tolist() == [0, 1, 17, 18, 23, 26, 30, 34, 37]
        assert (int(r["members"]["node_id"][0]), int(r["members"]["match"][0])) == (7, BIG + 10)
        assert [int(x) for x in r["members"]["node_id"][1:17]] == \
            [20 + i for i in range(8)] + list(range(1, 9))
        assert [int(x) for x in r["members"]["match"][1:9]] == [BIG + i for i in range(8)]
        assert [tuple(int(v) for v in r["members"][17])] == [(8, BIG + 2, sc.REMOTE, 1)]
        assert r["reads"]["ctx_low"].tolist() == [100 + k for k in range(8)]
        assert r["reads"]["ctx_high"].tolist() == [BIG + k for k in range(8)]
        assert r["reads"]["index"].tolist() == [BIG + 9] * 8
        assert r["read_confirmed"].tolist() == [0, 0, 0, 1 << 1, 0, 0, 0, 0]
        assert int(r["granted"][7]) == 1 << 2 and r["granted"][:7].tolist() == [0] * 7
        same_output(r, host.get_groups())
        check_against_get_group(dev, cids, handles, r)
        # the relocated groups and the 16-member group, listed alone and out of order
        some = np.array([6, 1, 5, 1], np.uint32)
        r2 = dev.get_groups(some)
        same_output(r2, host.get_groups(some))
        check_against_get_group(dev, cids, some, r2)


# ------------------------------------------------------------------ resume --------------------
def resumed_spec(g, kind):
    """What a CPU raft hands back for model group g: grown to 9 members, shrunk, or as it was."""
    mem = ref.member_tuples(g)
    if kind == "grow":
        mem = mem + [(100 + j, 0, sc.OBSERVER, j & 1) for j in range(9 - len(mem))]
    elif kind == "shrink":
        keep = [m for m in mem if m[2] != sc.OBSERVER]
        if len(keep) == len(mem) and len(mem) > 1:
            keep = [m for m in mem if m[0] != [x[0] for x in mem if x[0] != g["node_id"]][-1]]
        mem = keep
    return (g["cluster_id"], g["node_id"], g["term"], g["state"], g["committed"], g["last_index"],
            g["term_start"], mem)


def spec_arrays(hq, specs):
    groups = np.zeros(len(specs), hq.WORKER_GROUP_DTYPE)
    members = []
    for i, s in enumerate(specs):
        groups[i] = (s[0], s[1], s[2], s[4], s[5], s[6], s[3], len(s[7]), 0, 0)
        members += s[7]
    return groups, np.array(members, hq.MEMBER_DTYPE)


def oracle_from(groups):
    """A fresh oracle holding the model's groups (add_group carries no reads and no votes)."""
    o = OracleBackend()
    for c, g in groups.items():
        o.add_group(c, g["node_id"], g["term"], g["state"], g["committed"], g["last_index"],
                    g["term_start"], ref.member_tuples(g))
    return o


def model_tuple(g):
    return (g["term"], g["state"], g["committed"], g["last_index"], g["term_start"],
            ref.member_tuples(g), [(r["index"], r["from"], r["ctx"], r["n_confirmed"])
                                   for r in g["reads"]])


@pytest.mark.parametrize("k", [1, 4, 5, 257])
def test_resume_matches_set_group_one_by_one(hq, k):
    G = 2 * k + 38
    wd = World(hq, 9100 + k, G, n_dev=2, suspend=3)
    try:
        A, B, rng, cids = wd.devs[0], wd.devs[1], wd.rng, wd.cids
        model = {c: ref.group_of(wd.host, c) for c in cids}          # (a host worker: no readback)
        # the resumed handles: a 3-member group first (it grows to 9), then every other handle, so
        # each resumed group has neighbours that are not; suspended groups among them
        h3 = [h for h, c in enumerate(cids) if len(model[c]["members"]) == 3][0]
        cand = [h for h in range(h3 % 2, G, 2) if h != h3]
        susp = [h for h in cand if model[cids[h]]["suspended"]][:max(1, k // 3)]
        resumed = [h3] + (susp + [h for h in cand if h not in susp])[:k - 1]
        kinds = ["grow"] + [("shrink", "same", "grow")[i % 3] for i in range(k - 1)]
        specs = [resumed_spec(model[cids[h]], kind) for h, kind in zip(resumed, kinds)]
        if k >= 4:
            assert any(model[cids[h]]["suspended"] for h in resumed)
        if k >= 257:
            assert any(len(s[7]) < len(model[s[0]]["members"]) for s in specs)
        assert len(specs[0][7]) == 9 and len(model[specs[0][0]]["members"]) == 3
        before = B.get_groups()
        for s in specs:                                              # the old path, on A
            A.set_group(*s)
        assert A.readback_count() == 1 and B.readback_count() == 0
        assert B.set_groups(*spec_arrays(hq, specs)) > 0
        assert B.readback_count() == 0
        ra, rb = A.get_groups(), B.get_groups()
        assert B.readback_count() == 0
        same_output(ra, rb)
        for h in range(G):                                           # the others: byte-identical
            if h not in resumed:
                assert entry(rb, h) == entry(before, h), h
        for h, s in zip(resumed, specs):
            assert int(rb["groups"]["suspended"][h]) == 0 and int(rb["groups"]["n_pending_reads"][h]) == 0
            assert int(rb["groups"]["n_members"][h]) == len(s[7])
        # the full readback straight after set_groups reads what the scatter kernel wrote
        after = {c: ref.group_of(B, c) for c in cids}
        assert B.readback_count() == 1
        assert after == {c: ref.group_of(A, c) for c in cids}
        check_against_get_group(B, cids, np.arange(G), rb)
        for h, s in zip(resumed, specs):
            assert ref.member_tuples(after[s[0]]) == s[7] and after[s[0]]["reads"] == []
        # three more steps on B against a fresh oracle holding the post-resume state
        cont = [c for c in cids if not after[c]["reads"] and not after[c]["suspended"] and
                after[c]["state"] != ref.CANDIDATE]
        was_suspended = [cids[h] for h in resumed if model[cids[h]]["suspended"]]
        assert set(was_suspended) <= set(cont)
        oracle = oracle_from({c: after[c] for c in cont})
        for c in cont:
            assert oracle.state(c) == model_tuple(after[c])
        back = wd.bdevs[1]
        stepped = set()
        for s in range(10, 13):
            per = {c: sr.random_events(rng, back.state(c), s + 1, wd.ctx_seq)
                   for c in cont if c in was_suspended or rng.random() < 0.85}
            if not per:
                continue
            want, got = oracle.step(per), back.step(per)
            assert got["_fallback"] == []
            for c in per:
                same_step(want, got, c)
            for c in cont:
                assert back.state(c) == oracle.state(c), (s, c)
            stepped |= set(per)
        assert set(was_suspended) <= stepped
    finally:
        wd.close()


def test_grow_to_nine_members_is_seen_by_the_next_step(hq):
    """A device worker whose groups all have at most 8 members steps with 8 member slots in
    registers; a group resumed with 9 members must move it to the 16-slot kernels."""
    with hq.Worker(0, 8, on_device=True) as w:
        mem = [(1, 9, sc.REMOTE, 0), (2, 5, sc.REMOTE, 0), (3, 5, sc.REMOTE, 0)]
        for c in (1, 2, 3):
            w.add_group(c, 1, 2, sc.LEADER, 5, 9, 4, mem)
        b = WorkerBackend(hq, worker=w)
        assert raw_step(b, {c: [sc.msg(sc.HBRESP, 2, 2)] for c in (1, 2, 3)}) == []
        grown = mem + [(i, 5, sc.REMOTE, 0) for i in (4, 5)] + [(i, 0, sc.OBSERVER, 0) for i in (6, 7, 8, 9)]
        w.set_groups(*spec_arrays(hq, [(2, 1, 2, sc.LEADER, 5, 9, 4, grown)]))
        assert w.readback_count() == 0
        after = {c: ref.group_of(w, c) for c in (1, 2, 3)}
        stepped = [mem[0], (2, 5, sc.REMOTE, 1), mem[2]]                # (the HeartbeatResp: active)
        assert ref.member_tuples(after[2]) == grown and ref.member_tuples(after[1]) == stepped
        o = oracle_from(after)
        for per in ({2: [sc.msg(sc.RREP, 9, 2, 9), sc.msg(sc.RREP, 5, 2, 7), sc.msg(sc.RREP, 2, 2, 8)],
                     1: [sc.msg(sc.RREP, 2, 2, 8)], 3: [sc.msg(sc.RREP, 3, 2, 9)]},
                    {2: [sc.msg(sc.HBRESP, 9, 2), sc.msg(sc.RREP, 4, 2, 9), ("check_quorum",)]}):
            want, have = o.step(per), b.step(per)
            for c in per:
                same_step(want, have, c)
                assert b.state(c) == o.state(c)


# ------------------------------------------------------------------ the round trip ------------
class Listed:
    """A worker whose get_group goes through get_groups: WorkerBackend over it never reads back."""

    def __init__(self, w):
        self._w = w

    def __getattr__(self, name):
        return getattr(self._w, name)

    def get_group(self, cid):
        r = self._w.get_groups(np.array([self._w.find(cid)], np.uint32))
        return r["groups"][0], r["members"], r["reads"]


@pytest.mark.parametrize("on_device", MODES, ids=MODE_IDS)
def test_round_trip_after_a_fallback(hq, on_device):
    """Some groups fall back in a step (an observer acknowledging a ctx; a ReplicateResp above
    lastIndex); the caller fetches them, hands back exactly what it fetched, and they step again."""
    with hq.Worker(0, 8, on_device=on_device) as w:
        G = 40
        mem = [(4, 0, sc.OBSERVER, 0), (2, 7, sc.REMOTE, 1), (1, 9, sc.REMOTE, 0), (3, 6, sc.REMOTE, 0)]
        for c in range(1, G + 1):
            w.add_group(c, 1, 2, sc.LEADER, 6, 9, 5, mem)
        b = WorkerBackend(hq, worker=Listed(w))
        per, fall = {}, []
        for c in range(1, G + 1):
            per[c] = [("read", c, 77), sc.msg(sc.RREP, 2, 2, 8)]
            if c % 5 == 1:
                per[c].append(sc.msg(sc.HBRESP, 4, 2, hint=c, high=77))      # the observer acks
                fall.append(c)
            elif c % 5 == 3:
                per[c].append(sc.msg(sc.RREP, 3, 2, 10))                     # above lastIndex
                fall.append(c)
            per[c].append(sc.msg(sc.RREP, 3, 2, 9))
        out = b.step(per)
        assert sorted(out["_fallback"]) == fall
        handles = np.array([w.find(c) for c in fall], np.uint32)
        got = w.get_groups(handles)
        assert got["groups"]["suspended"].tolist() == [1] * len(fall)
        assert got["groups"]["cluster_id"].tolist() == fall
        assert got["groups"]["committed"].tolist() == [8] * len(fall)       # the events before it took
        assert got["groups"]["n_pending_reads"].tolist() == [1] * len(fall)
        gs = got["groups"].copy()
        w.set_groups(gs, got["members"])
        again = w.get_groups(handles)
        assert again["groups"]["suspended"].tolist() == [0] * len(fall)
        assert again["groups"]["n_pending_reads"].tolist() == [0] * len(fall)
        assert again["members"].tobytes() == got["members"].tobytes()
        for k in ("cluster_id", "node_id", "term", "committed", "last_index", "term_start", "state"):
            assert again["groups"][k].tolist() == got["groups"][k].tolist(), k
        # the resumed groups step again, and the next steps match an oracle holding what was fetched
        o = OracleBackend()
        for i, c in enumerate(fall):
            g = got["groups"][i]
            m0, m1 = int(got["member_offsets"][i]), int(got["member_offsets"][i + 1])
            o.add_group(c, int(g["node_id"]), int(g["term"]), int(g["state"]), int(g["committed"]),
                        int(g["last_index"]), int(g["term_start"]),
                        [tuple(int(v) for v in x) for x in got["members"][m0:m1]])
        for step_no in range(2):
            per = {c: [("read", 1000 + c, step_no + 1), sc.msg(sc.RREP, 3, 2, 9),
                       sc.msg(sc.HBRESP, 2, 2, hint=1000 + c, high=step_no + 1), ("propose", 2)]
                   for c in fall}
            want, have = o.step(per), b.step(per)
            assert have["_fallback"] == []
            for c in fall:
                same_step(want, have, c)
                assert have[c]["deferred"] == [] and b.state(c) == o.state(c)
        assert w.readback_count() == 0
        check_against_get_group(w, list(range(1, G + 1)), np.arange(G), w.get_groups())


# ------------------------------------------------------------------ errors --------------------
@pytest.mark.parametrize("on_device", MODES, ids=MODE_IDS)
def test_errors_change_nothing(hq, on_device):
    with hq.Worker(0, 8, on_device=on_device) as w:
        mem = [(1, 9, sc.REMOTE, 0), (2, 9, sc.REMOTE, 0), (3, 9, sc.REMOTE, 0), (4, 0, sc.OBSERVER, 0)]
        for c in (1, 2, 3):
            w.add_group(c, 1, 2, sc.LEADER, 9, 9, 9, mem)
        b = WorkerBackend(hq, worker=w)
        assert raw_step(b, {c: [("read", 5, c), ("propose", 1)] for c in (1, 2, 3)}) == []
        before = w.get_groups()
        out = hq.GroupsOutput()
        # get_groups: a NULL worker, a NULL output, an unknown handle, n = 0
        assert hq.lib.hq_worker_get_groups(None, 0, None, ctypes.byref(out)) == hq.HQ_E_INVAL
        assert hq.lib.hq_worker_get_groups(w.h, 1, None, None) == hq.HQ_E_INVAL
        for bad in ([3], [0, 1, 3], [0xFFFFFFFF]):
            with pytest.raises(hq.HQError) as e:
                w.get_groups(np.array(bad, np.uint32))
            assert e.value.code == hq.HQ_E_INVAL
        assert hq.lib.hq_worker_get_groups(w.h, 4, None, ctypes.byref(out)) == hq.HQ_E_INVAL
        assert hq.lib.hq_worker_get_groups(w.h, 0, None, ctypes.byref(out)) == hq.HQ_OK
        assert out.n_groups == 0 and out.gpu_ns == 0
        empty = w.get_groups(np.zeros(0, np.uint32))
        assert len(empty["groups"]) == 0 and empty["member_offsets"].tolist() == [0]
        same_output(before, w.get_groups())
        # set_groups: an unknown cluster, a cluster listed twice, one invalid group in the middle
        ok = lambda c, m=[(1, 12, sc.REMOTE, 0)] + mem[1:3]: (c, 1, 3, sc.LEADER, 10, 12, 11, m)
        bad_lists = [[ok(1), ok(9)], [ok(1), ok(2), ok(1)],
                     [ok(1), ok(2, mem[1:]), ok(3)],                            # the node is no member
                     [ok(1), ok(2, mem[:3] + [(2, 0, sc.OBSERVER, 0)]), ok(3)], # a duplicate member
                     [ok(1), ok(2, [(1, 9, 7, 0)]), ok(3)],                     # an unknown role
                     [ok(1), (2, 1, 3, 3, 10, 12, 11, mem), ok(3)],             # an unknown state
                     [ok(1), ok(2, [(i, 9, sc.REMOTE, 0) for i in range(1, 10)]), ok(3)]]   # 9 voters
        for bad in bad_lists:
            with pytest.raises(hq.HQError) as e:
                w.set_groups(*spec_arrays(hq, bad))
            assert e.value.code == hq.HQ_E_INVAL, bad
            same_output(before, w.get_groups())
        groups, members = spec_arrays(hq, [ok(1)])
        ns = ctypes.c_uint64(5)
        assert hq.lib.hq_worker_set_groups(None, 1, groups.ctypes.data, members.ctypes.data, None) == hq.HQ_E_INVAL
        assert hq.lib.hq_worker_set_groups(w.h, 1, None, members.ctypes.data, None) == hq.HQ_E_INVAL
        assert hq.lib.hq_worker_set_groups(w.h, 1, groups.ctypes.data, None, None) == hq.HQ_E_INVAL
        assert hq.lib.hq_worker_set_groups(w.h, 0, None, None, ctypes.byref(ns)) == hq.HQ_OK and ns.value == 0
        same_output(before, w.get_groups())
        assert w.readback_count() == 0
        check_against_get_group(w, [1, 2, 3], np.arange(3), before)
        # still usable
        w.set_groups(*spec_arrays(hq, [ok(3), ok(1)]))
        now = w.get_groups()
        assert now["groups"]["term"].tolist() == [3, 2, 3] and now["groups"]["n_members"].tolist() == [3, 4, 3]
        assert now["groups"]["n_pending_reads"].tolist() == [0, 1, 0]
        assert raw_step(b, {c: [("propose", 1)] for c in (1, 2, 3)}) == []
        assert w.get_groups()["groups"]["last_index"].tolist() == [13, 11, 13]
        check_against_get_group(w, [1, 2, 3], np.arange(3), w.get_groups())
