"""Every refusal the step worker's C entries make (dragonboat_amd/csrc/hq_worker*.cpp,
hq_jobs.cpp), written out: the entry, the bad call, its code and the exact hq_worker_last_error
text on a host worker and on a device worker. All of them are validations that return. After each
refusal the same entry is called with valid arguments on both workers and must give the same
result on both: nothing was left marked, queued or half-written. The world: a host worker and a
device worker over the same 8 leader groups of 3 members (handles 0 .. 7), plus one group of 17
members on the host worker alone (handle 8)."""
import ctypes

import numpy as np
import pytest

import step_scenarios as sc

pytestmark = pytest.mark.gpu

G = 8
CIDS = list(range(101, 101 + G))
BIG = 117                                   # the host worker's group of 17 members, handle 8
MEMBERS = [(1, 6, sc.REMOTE, 0), (2, 5, sc.REMOTE, 0), (3, 5, sc.REMOTE, 0)]
BIG_MEMBERS = MEMBERS + [(n, 0, sc.OBSERVER, 0) for n in range(4, 18)]
LISTS = ("commits", "ready", "read_resps", "state_changes", "dropped_reads", "deferred",
         "fallback_groups")
LONG = ("hq_worker_step_stream: boffsets decrease or out of range, sizes not summing to the totals, "
        "or a group's bytes not used up by its events (malformed event stream)")
UNCHANGED = object()                        # the entry returns its code without a message


class World:
    def __init__(self, hq):
        self.hq = hq
        self.dev, self.host = hq.Worker(0, 8, on_device=True), hq.Worker(0, 8)
        for w in (self.dev, self.host):
            for c in CIDS:
                assert w.add_group(c, 1, 2, sc.LEADER, 5, 6, 5, MEMBERS) == c - 101
        assert self.host.add_group(BIG, 1, 2, sc.LEADER, 5, 6, 5, BIG_MEMBERS) == G
        self.last = 6                       # every small group's lastIndex, moved by valid steps
        self.next_cid = 300
        self.all = np.arange(G, dtype=np.uint32)

    def close(self):
        self.dev.close()
        self.host.close()

    def events(self):
        """A valid step for all 8 groups: one proposal, then node 2's ack of it (a commit each)."""
        self.last += 1
        ev = np.zeros(2 * G, self.hq.EVENT_DTYPE)
        ev["kind"][0::2] = self.hq.EV_PROPOSE
        ev["log_index"][0::2] = 1
        ev["kind"][1::2] = self.hq.EV_MESSAGE
        ev["type"][1::2], ev["from"][1::2], ev["term"][1::2] = sc.RREP, 2, 2
        ev["log_index"][1::2] = self.last
        return np.arange(0, 2 * G + 1, 2, dtype=np.uint64), ev


def last_error(hq, w):
    return hq.lib.hq_worker_last_error(w.h).decode()


def refused(hq, w, call, code, text):
    """`call(w)` is refused with `code`; the worker's message is `text` (UNCHANGED: as before)."""
    before = last_error(hq, w)
    try:
        rc = call(w)
    except hq.HQError as e:
        rc = e.code
    assert rc == code, (rc, last_error(hq, w))
    assert last_error(hq, w) == (before if text is UNCHANGED else text)


def same_lists(a, b):
    for k in LISTS:
        assert sorted(map(tuple, a[k].tolist()) if a[k].dtype.names else a[k].tolist()) == \
            sorted(map(tuple, b[k].tolist()) if b[k].dtype.names else b[k].tolist()), k


def same_arrays(a, b, keys):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def run_table(hq, wd, table, valid):
    """Each row: (what, call, code, host text, device text); a text of None: the row is not for
    that worker. `valid()` calls the entry on both workers and compares."""
    for what, call, code, host_text, dev_text in table:
        for w, text in ((wd.host, host_text), (wd.dev, dev_text)):
            if text is not None:
                refused(hq, w, call, code, text)
        valid()


@pytest.fixture(scope="module")
def world(hq):
    wd = World(hq)
    yield wd
    wd.close()


# ------------------------------------------------------------------ the step entries ----------
def test_step_refusals(hq, world):
    wd, lib, INVAL = world, hq.lib, hq.HQ_E_INVAL
    ev2 = np.zeros(2, hq.EVENT_DTYPE)
    ev2["kind"], ev2["type"], ev2["from"], ev2["term"], ev2["log_index"] = hq.EV_MESSAGE, sc.RREP, 2, 2, 6
    u32, u64 = (lambda x: np.array(x, np.uint32)), (lambda x: np.array(x, np.uint64))
    out = hq.StepOutput()
    inp = hq.StepInput(1, None, None, None)
    g01, o012 = u32([0, 1]), u64([0, 1, 2])
    no_ev = hq.StepInput(2, hq._p(g01), hq._p(o012), None)

    def valid():
        off, ev = wd.events()
        a, b = wd.dev.step(wd.all, off, ev), wd.host.step(wd.all, off, ev)
        same_lists(a, b)
        assert sorted(map(tuple, a["commits"].tolist())) == [(c, wd.last) for c in CIDS]

    P = "hq_worker_step: "
    run_table(hq, wd, [
        ("in NULL", lambda w: lib.hq_worker_step(w.h, None, ctypes.byref(out)), INVAL,
         P + "NULL argument", P + "NULL argument"),
        ("out NULL", lambda w: lib.hq_worker_step(w.h, ctypes.byref(inp), None), INVAL,
         P + "NULL argument", P + "NULL argument"),
        ("groups NULL", lambda w: lib.hq_worker_step(w.h, ctypes.byref(inp), ctypes.byref(out)), INVAL,
         P + "NULL groups/offsets", P + "NULL groups/offsets"),
        ("events NULL", lambda w: lib.hq_worker_step(w.h, ctypes.byref(no_ev), ctypes.byref(out)), INVAL,
         P + "NULL events", P + "NULL events"),
        ("unknown handle", lambda w: w.step(u32([0, 99]), o012, ev2), INVAL,
         P + "unknown group handle", P + "unknown group handle"),
        ("listed twice", lambda w: w.step(u32([1, 1]), o012, ev2), INVAL,
         P + "a group is listed twice", P + "a group is listed twice"),
        ("offsets decrease", lambda w: w.step(g01, u64([0, 2, 1]), ev2), INVAL,
         P + "offsets decrease", P + "offsets decrease"),
    ], valid)
    # no worker at all: the code alone
    assert lib.hq_worker_step(None, ctypes.byref(inp), ctypes.byref(out)) == INVAL


def test_step_stream_refusals(hq, world):
    wd, lib, INVAL = world, hq.lib, hq.HQ_E_INVAL
    ev2 = np.zeros(2, hq.EVENT_DTYPE)
    ev2["kind"], ev2["type"], ev2["from"], ev2["term"], ev2["log_index"] = hq.EV_MESSAGE, sc.RREP, 2, 2, 6
    u32, u64 = (lambda x: np.array(x, np.uint32)), (lambda x: np.array(x, np.uint64))
    o012 = u64([0, 1, 2])
    data, boff = hq.encode_events(o012, ev2)
    sdata, sizes = hq.encode_events_sized(o012, ev2)
    assert list(sizes) == [1 | 4 << 16, 1 | 4 << 16] and len(sdata) == 8 and list(boff) == [0, 4, 8]
    out = hq.StepOutput()
    g01 = u32([0, 1])
    # (n_groups, groups, offsets, boffsets, bytes, sizes, n_events, n_bytes, sizes16)
    no_sizes = hq.StepStream(2, hq._p(g01), None, None, hq._p(sdata), None, 2, 8, None)
    no_bytes = hq.StepStream(2, hq._p(g01), None, None, None, hq._p(sizes), 2, 8, None)
    no_boff = hq.StepStream(2, hq._p(g01), hq._p(o012), None, hq._p(data))
    no_data = hq.StepStream(2, hq._p(g01), hq._p(o012), hq._p(boff), None)
    raw = lambda s: (lambda w: lib.hq_worker_step_stream(w.h, ctypes.byref(s), ctypes.byref(out)))
    cut = np.concatenate([data[:3], data[4:]])          # group 0's event loses its last byte
    form = [0]

    def valid():
        off, ev = wd.events()
        form[0] += 1
        if form[0] % 3 == 0:                            # the three forms of the stream in turn
            d, b = hq.encode_events(off, ev)
            a, c = wd.dev.step_stream(wd.all, off, b, d), wd.host.step_stream(wd.all, off, b, d)
        else:
            d, z = hq.encode_events_sized(off, ev)
            if form[0] % 3 == 1:
                z = hq.sizes16_of(z)
            a = wd.dev.step_sized(wd.all, z, len(ev), d)
            c = wd.host.step_sized(None, z, len(ev), d)
        same_lists(a, c)
        assert sorted(map(tuple, a["commits"].tolist())) == [(c, wd.last) for c in CIDS]

    P, Q = "hq_worker_step_stream: ", "hq_worker_step: "
    run_table(hq, wd, [
        ("in NULL", lambda w: lib.hq_worker_step_stream(w.h, None, ctypes.byref(out)), INVAL,
         P + "NULL argument", P + "NULL argument"),
        ("out NULL", lambda w: lib.hq_worker_step_stream(w.h, ctypes.byref(no_sizes), None), INVAL,
         P + "NULL argument", P + "NULL argument"),
        ("sizes NULL", raw(no_sizes), INVAL, P + "NULL sizes", P + "NULL sizes"),
        ("sized: bytes NULL", raw(no_bytes), INVAL, P + "NULL bytes", P + "NULL bytes"),
        ("boffsets NULL", raw(no_boff), INVAL,
         P + "NULL groups/offsets/boffsets", P + "NULL groups/offsets/boffsets"),
        ("bytes NULL", raw(no_data), INVAL, P + "NULL bytes", P + "NULL bytes"),
        ("sized: events total", lambda w: w.step_sized(g01, sizes, 3, sdata), INVAL,
         P + "sizes do not sum to the totals", LONG),
        ("sized: bytes total", lambda w: w.step_sized(g01, sizes, 2, np.concatenate([sdata, sdata[:1]])),
         INVAL, P + "sizes do not sum to the totals", LONG),
        ("sized: one size", lambda w: w.step_sized(g01, u32([1 | 4 << 16, 1 | 5 << 16]), 2, sdata), INVAL,
         P + "sizes do not sum to the totals", LONG),
        ("sized16: bytes total", lambda w: w.step_sized(g01, np.array([4, 5], np.uint16), 2, sdata), INVAL,
         P + "sizes do not sum to the totals", LONG),
        ("sized: split wrong", lambda w: w.step_sized(g01, u32([1 | 5 << 16, 1 | 3 << 16]), 2, sdata), INVAL,
         P + "malformed event stream", LONG),
        ("sized16: split wrong", lambda w: w.step_sized(g01, np.array([5, 3], np.uint16), 2, sdata), INVAL,
         P + "malformed event stream", LONG),
        ("sized: unknown handle", lambda w: w.step_sized(u32([0, 99]), sizes, 2, sdata), INVAL,
         Q + "unknown group handle", Q + "unknown group handle"),
        ("sized: listed twice", lambda w: w.step_sized(u32([1, 1]), sizes, 2, sdata), INVAL,
         Q + "a group is listed twice", Q + "a group is listed twice"),
        ("sized: more sizes than groups", lambda w: w.step_sized(None, np.zeros(20, np.uint32), 0, sdata[:0]),
         INVAL, Q + "unknown group handle", Q + "unknown group handle"),
        ("unknown handle", lambda w: w.step_stream(u32([0, 99]), o012, boff, data), INVAL,
         Q + "unknown group handle", Q + "unknown group handle"),
        ("listed twice", lambda w: w.step_stream(u32([1, 1]), o012, boff, data), INVAL,
         Q + "a group is listed twice", Q + "a group is listed twice"),
        ("offsets decrease", lambda w: w.step_stream(g01, u64([0, 2, 1]), boff, data), INVAL,
         Q + "offsets decrease", Q + "offsets decrease"),
        # (a device worker takes a group's undecodable event as a fallback of that group, not as a
        # refusal: test_gpu_worker.py test_malformed_stream)
        ("malformed", lambda w: w.step_stream(g01, o012, u64([0, 3, 7]), cut), INVAL,
         P + "malformed event stream", None),
    ], valid)


def test_step_jobs_refusals(hq, world):
    wd, lib, INVAL = world, hq.lib, hq.HQ_E_INVAL
    ev2 = np.zeros(2, hq.EVENT_DTYPE)
    ev2["kind"], ev2["type"], ev2["from"], ev2["term"], ev2["log_index"] = hq.EV_MESSAGE, sc.RREP, 2, 2, 6
    bad = (np.array([1, 1], np.uint32), np.array([0, 1, 2], np.uint64), ev2)

    def valid():
        off, ev = wd.events()
        a, b = hq.step_jobs([(wd.dev, (wd.all, off, ev)), (wd.host, (wd.all, off, ev))])
        same_lists(a, b)
        assert sorted(map(tuple, a["commits"].tolist())) == [(c, wd.last) for c in CIDS]

    assert lib.hq_worker_step_jobs(None, 2) == INVAL
    valid()
    for w in (wd.dev, wd.host):                          # a worker in two jobs: no job's message
        off, ev = wd.events()
        wd.last -= 1
        jobs = hq.StepJobs([(w, (wd.all, off, ev)), (w, (wd.all, off, ev))])
        before = last_error(hq, w)
        assert lib.hq_worker_step_jobs(jobs.arr, 2) == INVAL and last_error(hq, w) == before
        valid()
    # one job refused, the other stepped: the call's code is the refused job's, and so is the text
    off, ev = wd.events()
    jobs = hq.StepJobs([(wd.dev, bad), (wd.host, (wd.all, off, ev))])
    assert lib.hq_worker_step_jobs(jobs.arr, 2) == INVAL
    assert (jobs.arr[0].rc, jobs.arr[1].rc) == (INVAL, hq.HQ_OK)
    assert last_error(hq, wd.dev) == "hq_worker_step: a group is listed twice"
    got = wd.dev.step(wd.all, off, ev)                   # (the device worker catches up)
    same_lists(got, jobs.results()[1])
    valid()


# ------------------------------------------------------------------ heartbeats ----------------
def test_heartbeat_refusals(hq, world):
    wd, lib, INVAL = world, hq.lib, hq.HQ_E_INVAL
    out = hq.HeartbeatOutput()
    P = "hq_worker_heartbeats: "

    def valid():
        a, b = wd.dev.heartbeats(wd.all), wd.host.heartbeats(wd.all)
        same_arrays(a, b, ("words", "lags", "ctxs"))
        assert a["n_messages"] == b["n_messages"] == 2 * G
        assert [int(x) & 0xFFFF for x in a["words"]] == [0b110] * G    # to members 1 and 2

    run_table(hq, wd, [
        ("out NULL", lambda w: lib.hq_worker_heartbeats(w.h, 1, None, None), INVAL,
         P + "out is NULL", P + "out is NULL"),
        ("2^28 groups", lambda w: lib.hq_worker_heartbeats(w.h, 1 << 28, None, ctypes.byref(out)), INVAL,
         P + "2^28 or more groups in one call", P + "2^28 or more groups in one call"),
        ("more than there are", lambda w: lib.hq_worker_heartbeats(w.h, 10, None, ctypes.byref(out)), INVAL,
         P + "unknown group handle", P + "unknown group handle"),
        ("unknown handle", lambda w: w.heartbeats(np.array([0, 99], np.uint32)), INVAL,
         P + "unknown group handle", P + "unknown group handle"),
        ("17 members", lambda w: w.heartbeats(np.array([0, G], np.uint32)), INVAL,
         P + "a group of more than 16 members", None),
        ("17 members, every handle", lambda w: w.heartbeats(), INVAL,
         P + "a group of more than 16 members", None),
    ], valid)


def test_heartbeat_batches_refusals(hq, world):
    wd, lib, INVAL = world, hq.lib, hq.HQ_E_INVAL
    out = hq.HeartbeatBatches()
    src = ctypes.create_string_buffer(b"host", 4)
    cfg = hq.HeartbeatWireConfig(7, ctypes.cast(src, ctypes.c_void_p), 4, 3, 0)
    no_src = hq.HeartbeatWireConfig(7, None, 4, 3, 0)
    P, R = "hq_worker_heartbeat_batches: ", "hq_worker_set_heartbeat_routes: "
    routes = np.full((G, 16), hq.HQ_ROUTE_NONE, np.uint16)
    routes[:, 1], routes[:, 2] = 1, 2                    # member 1 -> destination 1, member 2 -> 2

    def valid_routes():
        for w in (wd.dev, wd.host):
            w.set_heartbeat_routes(0, routes)

    run_table(hq, wd, [
        ("routes NULL", lambda w: lib.hq_worker_set_heartbeat_routes(w.h, 0, 2, None), INVAL,
         R + "routes is NULL", R + "routes is NULL"),
        ("first handle", lambda w: w.set_heartbeat_routes(99, routes[:1]), INVAL,
         R + "unknown group handle", R + "unknown group handle"),
        ("past the end", lambda w: w.set_heartbeat_routes(7, np.concatenate([routes, routes])[:4]), INVAL,
         R + "unknown group handle", R + "unknown group handle"),
    ], valid_routes)

    def valid():
        a = wd.dev.heartbeat_batches(wd.all, 7, b"host", n_dest=3)
        b = wd.host.heartbeat_batches(wd.all, 7, b"host", n_dest=3)
        same_arrays(a, b, ("bytes", "batches"))
        assert a["n_messages"] == b["n_messages"] == 2 * G and a["n_unrouted"] == b["n_unrouted"] == 0
        assert a["batches"]["dest"].tolist() == [1, 2]

    one = np.array([0], np.uint32)
    run_table(hq, wd, [
        ("cfg NULL", lambda w: lib.hq_worker_heartbeat_batches(w.h, 1, None, None, ctypes.byref(out)), INVAL,
         P + "cfg or out is NULL", P + "cfg or out is NULL"),
        ("out NULL", lambda w: lib.hq_worker_heartbeat_batches(w.h, 1, None, ctypes.byref(cfg), None), INVAL,
         P + "cfg or out is NULL", P + "cfg or out is NULL"),
        ("n_dest 0", lambda w: w.heartbeat_batches(one, n_dest=0), INVAL,
         P + "n_dest must be 1 .. 65535", P + "n_dest must be 1 .. 65535"),
        ("n_dest 65536", lambda w: w.heartbeat_batches(one, n_dest=65536), INVAL,
         P + "n_dest must be 1 .. 65535", P + "n_dest must be 1 .. 65535"),
        ("source 257 bytes", lambda w: w.heartbeat_batches(one, source=b"x" * 257, n_dest=3), INVAL,
         P + "a source of more than 256 bytes (or NULL)", P + "a source of more than 256 bytes (or NULL)"),
        ("source NULL", lambda w: lib.hq_worker_heartbeat_batches(w.h, 1, None, ctypes.byref(no_src),
                                                                  ctypes.byref(out)), INVAL,
         P + "a source of more than 256 bytes (or NULL)", P + "a source of more than 256 bytes (or NULL)"),
        ("2^28 groups", lambda w: lib.hq_worker_heartbeat_batches(w.h, 1 << 28, None, ctypes.byref(cfg),
                                                                  ctypes.byref(out)), INVAL,
         P + "2^28 or more groups in one call", P + "2^28 or more groups in one call"),
        ("more than there are", lambda w: lib.hq_worker_heartbeat_batches(w.h, 10, None, ctypes.byref(cfg),
                                                                          ctypes.byref(out)), INVAL,
         P + "unknown group handle", P + "unknown group handle"),
        ("unknown handle", lambda w: w.heartbeat_batches(np.array([0, 99], np.uint32), n_dest=3), INVAL,
         P + "unknown group handle", P + "unknown group handle"),
        ("17 members", lambda w: w.heartbeat_batches(np.array([0, G], np.uint32), n_dest=3), INVAL,
         P + "a group of more than 16 members", None),
        ("route 2 of 2 destinations", lambda w: w.heartbeat_batches(wd.all, n_dest=2), INVAL,
         P + "a route at or above n_dest", P + "a route at or above n_dest"),
    ], valid)


# ------------------------------------------------------------------ membership ----------------
def test_config_change_refusals(hq, world):
    wd, lib, INVAL = world, hq.lib, hq.HQ_E_INVAL
    out = hq.ConfigOutput()
    one = np.array([(0, hq.HQ_CC_REMOVE_NODE, 99)], hq.CONFIG_CHANGE_DTYPE)
    P = "hq_worker_config_changes: "
    turn = [0]

    def valid():
        # in turn: node 9 joins groups 6 and 7 as an observer and leaves again; in between, the
        # removal of a node that is no member (its tryCommit runs all the same)
        turn[0] += 1
        kind = (hq.HQ_CC_REMOVE_NODE, hq.HQ_CC_ADD_OBSERVER, hq.HQ_CC_REMOVE_NODE)[turn[0] % 3]
        node = 50 if turn[0] % 3 == 2 else 9
        ch = [(6, kind, node), (7, kind, node)]
        a, b = wd.dev.config_changes(ch), wd.host.config_changes(ch)
        same_arrays(a, b, ("status", "commits"))
        for k in ("n_applied", "n_noop", "n_fallback", "n_suspended"):
            assert a[k] == b[k], k
        assert a["n_applied"] == (0 if turn[0] % 3 == 2 else 2)
        same_arrays(wd.dev.get_groups([6, 7]), wd.host.get_groups([6, 7]), ("groups", "members"))

    run_table(hq, wd, [
        ("out NULL", lambda w: lib.hq_worker_config_changes(w.h, 1, hq._p(one), None), INVAL,
         P + "NULL argument", P + "NULL argument"),
        ("changes NULL", lambda w: lib.hq_worker_config_changes(w.h, 1, None, ctypes.byref(out)), INVAL,
         P + "NULL argument", P + "NULL argument"),
        ("2^32 changes", lambda w: lib.hq_worker_config_changes(w.h, 1 << 32, hq._p(one), ctypes.byref(out)),
         INVAL, P + "a group is listed twice", P + "a group is listed twice"),
        ("unknown handle", lambda w: w.config_changes([(0, hq.HQ_CC_ADD_OBSERVER, 9), (99, 0, 9)]), INVAL,
         P + "unknown group handle", P + "unknown group handle"),
        ("listed twice", lambda w: w.config_changes([(0, hq.HQ_CC_ADD_OBSERVER, 9), (1, 2, 9), (0, 2, 8)]),
         INVAL, P + "a group is listed twice", P + "a group is listed twice"),
        ("unknown type", lambda w: w.config_changes([(0, hq.HQ_CC_ADD_OBSERVER, 9), (1, 4, 9)]), INVAL,
         P + "unknown change type", P + "unknown change type"),
        ("node_id 0", lambda w: w.config_changes([(0, hq.HQ_CC_ADD_OBSERVER, 9), (1, 0, 0)]), INVAL,
         P + "node_id 0", P + "node_id 0"),
        ("a member in another role", lambda w: w.config_changes([(0, hq.HQ_CC_ADD_OBSERVER, 9),
                                                                  (1, hq.HQ_CC_ADD_WITNESS, 2)]), INVAL,
         P + "ADD_OBSERVER / ADD_WITNESS of a member in another role",
         P + "ADD_OBSERVER / ADD_WITNESS of a member in another role"),
    ], valid)


# ------------------------------------------------------------------ groups --------------------
GG = ("groups", "members", "member_offsets", "reads", "read_offsets", "granted", "rejected",
      "read_confirmed")


def test_get_set_groups_refusals(hq, world):
    wd, lib, INVAL = world, hq.lib, hq.HQ_E_INVAL
    out = hq.GroupsOutput()
    P, S = "hq_worker_get_groups: ", "hq_worker_set_groups: "

    def valid():
        same_arrays(wd.dev.get_groups(wd.all), wd.host.get_groups(wd.all), GG)
        same_arrays(wd.dev.get_groups([3, 3, 0]), wd.host.get_groups([3, 3, 0]), GG)

    run_table(hq, wd, [
        ("out NULL", lambda w: lib.hq_worker_get_groups(w.h, 1, None, None), INVAL,
         P + "NULL argument", P + "NULL argument"),
        ("2^32 groups", lambda w: lib.hq_worker_get_groups(w.h, 1 << 32, None, ctypes.byref(out)), INVAL,
         P + "too many groups listed", P + "too many groups listed"),
        # (every handle up to 9: the host worker meets its handle 8, of 17 members, first)
        ("more than there are", lambda w: lib.hq_worker_get_groups(w.h, 10, None, ctypes.byref(out)), INVAL,
         P + "a group of more than 16 members", P + "unknown group handle"),
        ("unknown handle", lambda w: w.get_groups([0, 99]), INVAL,
         P + "unknown group handle", P + "unknown group handle"),
        ("17 members", lambda w: w.get_groups([0, G]), INVAL, P + "a group of more than 16 members", None),
    ], valid)

    cur = wd.host.get_groups([2, 5])
    g2, m2 = cur["groups"], cur["members"]
    ns = ctypes.c_uint64(0)

    def edited(**kw):
        g = g2.copy()
        for k, v in kw.items():
            g[k] = v
        return g

    dup = m2.copy()
    dup["node_id"][4] = dup["node_id"][3]                # group 5's member 1 twice
    big = np.zeros(1, hq.WORKER_GROUP_DTYPE)
    big[0] = g2[0]
    big["n_members"] = 17
    big_m = np.array(BIG_MEMBERS, hq.MEMBER_DTYPE)

    def valid_set():
        # groups 2 and 5 resumed as follower and candidate of the next term on both workers,
        # then as they were
        g = edited(term=g2["term"] + 1, state=[sc.FOLLOWER, sc.CANDIDATE])
        for w in (wd.dev, wd.host):
            w.set_groups(g, m2)
        same_arrays(wd.dev.get_groups(wd.all), wd.host.get_groups(wd.all), GG)
        for w in (wd.dev, wd.host):
            w.set_groups(g2, m2)
        got = wd.dev.get_groups([2, 5])
        same_arrays(got, wd.host.get_groups([2, 5]), GG)
        same_arrays(got, cur, ("groups", "members"))

    run_table(hq, wd, [
        ("groups NULL", lambda w: lib.hq_worker_set_groups(w.h, 2, None, hq._p(m2), ctypes.byref(ns)), INVAL,
         S + "NULL argument", S + "NULL argument"),
        ("members NULL", lambda w: lib.hq_worker_set_groups(w.h, 2, hq._p(g2), None, ctypes.byref(ns)), INVAL,
         S + "NULL argument", S + "NULL argument"),
        ("2^32 groups", lambda w: lib.hq_worker_set_groups(w.h, 1 << 32, hq._p(g2), hq._p(m2), None), INVAL,
         S + "a cluster is listed twice", S + "a cluster is listed twice"),
        ("unknown cluster", lambda w: w.set_groups(edited(cluster_id=[103, 999]), m2), INVAL,
         S + "unknown cluster", S + "unknown cluster"),
        ("listed twice", lambda w: w.set_groups(edited(cluster_id=[103, 103]), m2), INVAL,
         S + "a cluster is listed twice", S + "a cluster is listed twice"),
        ("second group: a member twice", lambda w: w.set_groups(g2, dup), INVAL,
         "duplicate member", "duplicate member"),
        ("second group: state 3", lambda w: w.set_groups(edited(state=[sc.LEADER, 3]), m2), INVAL,
         "state must be follower, candidate or leader", "state must be follower, candidate or leader"),
        ("second group: not a member itself", lambda w: w.set_groups(edited(node_id=[1, 77]), m2), INVAL,
         "the node is not one of the group's remotes", "the node is not one of the group's remotes"),
        ("17 members", lambda w: w.set_groups(big, big_m), INVAL,
         None, "more than 16 members on the device path (HQ_WORKER_ON_DEVICE)"),
    ], valid_set)


def test_group_store_refusals(hq, world):
    wd, lib, INVAL = world, hq.lib, hq.HQ_E_INVAL
    m = np.array(MEMBERS, hq.MEMBER_DTYPE)
    h = ctypes.c_uint32(0)
    n64 = ctypes.c_uint64(0)

    def same_group(cid):
        (ga, ma, ra), (gb, mb, rb) = wd.dev.get_group(cid), wd.host.get_group(cid)
        assert ga.tobytes() == gb.tobytes() and ma.tobytes() == mb.tobytes() and ra.tobytes() == rb.tobytes()
        return ga

    def valid_add():
        wd.next_cid += 1
        hs = [w.add_group(wd.next_cid, 2, 3, sc.FOLLOWER, 1, 2, 1, MEMBERS) for w in (wd.dev, wd.host)]
        assert hs == [wd.dev.group_count() - 1, wd.host.group_count() - 1]
        assert [wd.dev.find(wd.next_cid), wd.host.find(wd.next_cid)] == hs
        assert int(same_group(wd.next_cid)["term"]) == 3

    A = "hq_worker_add_group: "
    run_table(hq, wd, [
        ("group NULL", lambda w: lib.hq_worker_add_group(w.h, None, hq._p(m), ctypes.byref(h)), INVAL,
         A + "group is NULL", A + "group is NULL"),
        ("cluster exists", lambda w: w.add_group(101, 1, 2, sc.LEADER, 5, 6, 5, MEMBERS), INVAL,
         A + "cluster exists", A + "cluster exists"),
        ("no members", lambda w: w.add_group(400, 1, 2, sc.LEADER, 5, 6, 5, []), INVAL,
         "group has no members", "group has no members"),
        ("65 members", lambda w: w.add_group(400, 1, 2, sc.LEADER, 5, 6, 5,
                                              MEMBERS + [(n, 0, sc.OBSERVER, 0) for n in range(4, 66)]), INVAL,
         "more than 64 members", "more than 64 members"),
        ("role 3", lambda w: w.add_group(400, 1, 2, sc.LEADER, 5, 6, 5, MEMBERS[:2] + [(3, 5, 3, 0)]), INVAL,
         "unknown member role", "unknown member role"),
        ("9 voting members", lambda w: w.add_group(400, 1, 2, sc.LEADER, 5, 6, 5,
                                                    [(n, 0, sc.REMOTE, 0) for n in range(1, 10)]), INVAL,
         "more voting members than n_max", "more voting members than n_max"),
        ("17 members", lambda w: w.add_group(400, 1, 2, sc.LEADER, 5, 6, 5, BIG_MEMBERS), INVAL,
         None, "more than 16 members on the device path (HQ_WORKER_ON_DEVICE)"),
    ], valid_add)

    def valid_add_groups():
        wd.next_cid += 2
        g = np.zeros(2, hq.WORKER_GROUP_DTYPE)
        g["cluster_id"] = [wd.next_cid - 1, wd.next_cid]
        g["node_id"], g["term"], g["n_members"], g["last_index"] = 1, 4, 3, 6
        for w in (wd.dev, wd.host):
            w.add_groups(g, np.concatenate([m, m]))
        assert int(same_group(wd.next_cid)["term"]) == 4

    g1 = np.zeros(1, hq.WORKER_GROUP_DTYPE)
    g1["cluster_id"], g1["node_id"], g1["n_members"] = 101, 1, 3
    B = "hq_worker_add_groups: "
    run_table(hq, wd, [
        ("groups NULL", lambda w: lib.hq_worker_add_groups(w.h, None, 1, hq._p(m)), INVAL,
         B + "NULL argument", B + "NULL argument"),
        ("members NULL", lambda w: lib.hq_worker_add_groups(w.h, hq._p(g1), 1, None), INVAL,
         B + "NULL argument", B + "NULL argument"),
        ("cluster exists", lambda w: w.add_groups(g1, m), INVAL, A + "cluster exists", A + "cluster exists"),
    ], valid_add_groups)

    def valid_find():
        assert [wd.dev.find(104), wd.host.find(104)] == [3, 3]
        assert wd.host.find(BIG) == G

    run_table(hq, wd, [
        ("unknown cluster", lambda w: w.find(999), INVAL,
         "hq_worker_find: unknown cluster", "hq_worker_find: unknown cluster"),
        ("count: n NULL", lambda w: lib.hq_worker_group_count(w.h, None), INVAL, UNCHANGED, UNCHANGED),
        ("readbacks: n NULL", lambda w: lib.hq_worker_readback_count(w.h, None), INVAL, UNCHANGED, UNCHANGED),
    ], valid_find)

    def valid_set_get():
        for w in (wd.dev, wd.host):
            w.set_group(104, 1, 9, sc.FOLLOWER, 5, 6, 5, MEMBERS)
        assert int(same_group(104)["term"]) == 9
        for w in (wd.dev, wd.host):
            w.set_group(104, 1, 2, sc.LEADER, 5, wd.last, 5, [(1, wd.last, 0, 0)] + MEMBERS[1:])
        assert int(same_group(104)["state"]) == sc.LEADER

    gnull = lambda w: lib.hq_worker_set_group(w.h, None, hq._p(m))
    S, T = "hq_worker_set_group: ", "hq_worker_get_group: "
    run_table(hq, wd, [
        ("set: group NULL", gnull, INVAL, S + "group is NULL", S + "group is NULL"),
        ("set: unknown cluster", lambda w: w.set_group(999, 1, 2, sc.LEADER, 5, 6, 5, MEMBERS), INVAL,
         S + "unknown cluster", S + "unknown cluster"),
        ("set: a member twice", lambda w: w.set_group(104, 1, 2, sc.LEADER, 5, 6, 5, MEMBERS + MEMBERS[1:2]),
         INVAL, "duplicate member", "duplicate member"),
        ("set: 17 members", lambda w: w.set_group(104, 1, 2, sc.LEADER, 5, 6, 5, BIG_MEMBERS), INVAL,
         None, "more than 16 members on the device path (HQ_WORKER_ON_DEVICE)"),
        ("get: unknown cluster", lambda w: w.get_group(999), INVAL, T + "unknown cluster", T + "unknown cluster"),
    ], valid_set_get)

    W = "hq_worker_set_wait: "
    run_table(hq, wd, [
        ("a host worker", lambda w: w.set_wait(hq.HQ_WAIT_BLOCK), INVAL, W + "not a device worker", None),
        ("mode 77", lambda w: w.set_wait(77), INVAL, None, W + "unknown mode (or sleep_us 0)"),
        ("sleep_us 0", lambda w: w.set_wait(hq.HQ_WAIT_SLEEP, 50, 0), INVAL,
         None, W + "unknown mode (or sleep_us 0)"),
    ], lambda: wd.dev.set_wait(hq.HQ_WAIT_BLOCK))
    # and the workers still step together
    off, ev = wd.events()
    same_lists(wd.dev.step(wd.all, off, ev), wd.host.step(wd.all, off, ev))
