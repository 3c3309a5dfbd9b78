"""hq_worker_heartbeat_batches on a device worker (dragonboat_amd/csrc/hq_heartbeat_wire.hip): the
leader heartbeats marshalled on the device as MessageBatch bytes per destination. Expected values
come from tests/heartbeat_wire_ref.py (heartbeat_ref.broadcast over Worker.get_group, the routes
looked up in Python, wire_encode.batch for the bytes), which never touches the new kernels; every
batch also goes through hq_wire_decode_batch."""
import numpy as np
import pytest

import heartbeat_ref as ref
import heartbeat_wire_ref as hw
import step_random as sr
import step_scenarios as sc
import test_gpu_heartbeat as hbt
import test_heartbeat_wire_host as host
from step_harness import WorkerBackend

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 257, 5000]     # the wave edge, the workgroup edge, several scan tiles
DESTS, CUTS = (1, 7, 300), (0, 1, 64)


def first_ordinals(batches):
    """Each batch's first message as its ordinal among the call's sorted messages."""
    return np.concatenate([[0], np.cumsum(batches["n_messages"])[:-1]])


def test_reference_tables_on_device(hq):
    with hq.Worker(0, 8, on_device=True) as w:
        host.check_kats(hq, w)


@pytest.mark.parametrize("G", SIZES)
def test_differential(hq, G):
    rng = np.random.default_rng(2000 + G)
    groups = hbt.random_world(rng, G)
    with hq.Worker(0, 8, on_device=True) as w:
        for g in groups:
            w.add_group(*g[:8])
        suspended = hbt.step_world(hq, rng, [w], groups, 2 if G > 1000 else 3)
        world = hw.World(w, [g[0] for g in groups])
        pick = rng.integers(0, G, max(1, (2 * G) // 3))
        pick = np.concatenate([pick, pick[:max(1, G // 7)]]).astype(np.uint32)
        rng.shuffle(pick)
        # every pairing of n_dest and batch_messages; at 5000 groups each value once per list
        pairs = [(d, c) for d in DESTS for c in CUTS]
        if G > 1000:
            pairs = [(1, 0), (7, 64), (300, 1)]
        empty_dest = cut_inside = False
        for k, (n_dest, bm) in enumerate(pairs):
            routes = hw.random_routes(rng, G, n_dest)
            w.set_heartbeat_routes(0, routes)
            got, _ = hw.run_and_check(hq, world, None, routes, n_dest, bm, decode=G <= 1000 or k == 1)
            b = got["batches"]
            empty_dest |= len(set(b["dest"].tolist())) < n_dest
            same_dest = np.concatenate([[False], b["dest"][1:] == b["dest"][:-1]])
            cut_inside |= bool(np.any(same_dest & (first_ordinals(b) % 256 != 0)))
            other = pairs[(k + 1) % len(pairs)][1] if G > 1000 else bm
            hw.run_and_check(hq, world, pick, routes, n_dest, other, 0, b"", decode=G <= 1000)
        if G >= 257:     # the worlds hold every kind
            listed = [ref.worker_group(w, c) for c in world.cids]
            hb = w.heartbeats()
            kinds = dict(leader=sum(x[1] == sc.LEADER for x in listed),
                         other=sum(x[1] != sc.LEADER for x in listed), suspended=len(suspended),
                         lags=len(hb["lags"]), ctxs=len(hb["ctxs"]),
                         observers=sum(any(m[2] == sc.OBSERVER for m in x[4]) for x in listed),
                         unrouted=got["n_unrouted"], empty_dest=empty_dest, cut_inside=cut_inside)
            assert all(v > 0 for v in kinds.values()), kinds


@pytest.fixture(scope="module")
def pairs_worker(hq):
    """513 leaders with one other voter each: a message per group, ids around the one- / two-byte
    varint edge so that the messages differ in length."""
    w = hq.Worker(0, 8, on_device=True)
    cids = list(range(100, 613))
    for c in cids:
        w.add_group(c, 1, 3, sc.LEADER, c, c + 1, c - 1, [(1, c + 1, 0, 0), (c + 20, c - 50, 0, 0)])
    routes = host.rows(*[[hw.NONE, 0]] * len(cids))
    w.set_heartbeat_routes(0, routes)
    yield w, hw.World(w, cids), routes
    w.close()


@pytest.mark.parametrize("bm", [256, 255])
@pytest.mark.parametrize("K", [255, 256, 257, 513])
def test_encode_kernel_edges(hq, pairs_worker, K, bm):
    """Exactly K messages to one destination, cut on a workgroup's edge (256) and next to it."""
    w, world, routes = pairs_worker
    got, _ = hw.run_and_check(hq, world, np.arange(K, dtype=np.uint32), routes, 1, bm)
    assert got["n_messages"] == K and len(got["batches"]) == -(-K // bm)


@pytest.fixture(scope="module")
def world1000(hq):
    rng = np.random.default_rng(31)
    groups = hbt.random_world(rng, 1000)
    w = hq.Worker(0, 8, on_device=True)
    for g in groups:
        w.add_group(*g[:8])
    hbt.step_world(hq, rng, [w], groups, 2)
    routes = hw.random_routes(rng, 1000, 5)
    w.set_heartbeat_routes(0, routes)
    yield w, hw.World(w, [g[0] for g in groups]), routes
    w.close()


def test_both_store_paths(hq, world1000):
    """k_hbw_encode stages a workgroup's range in LDS when it is at most kStageBytes (32768) and
    stores directly otherwise. batch_messages = 1 with a 256-byte source puts a trailer of some 265
    bytes behind every message (256 messages: over 80,000 bytes, the direct path in every full
    workgroup); one batch per destination and an empty source stay under 29,000 (the staged
    path)."""
    w, world, routes = world1000
    src = bytes(range(256))
    direct, _ = hw.run_and_check(hq, world, None, routes, 5, 1, 3, src, decode=False)
    assert direct["n_messages"] > 4 * 256
    assert len(direct["bytes"]) > (direct["n_messages"] // 256) * 32768 * 2
    staged, _ = hw.run_and_check(hq, world, None, routes, 5, 0, 3, b"")
    assert len(staged["bytes"]) < (staged["n_messages"] // 256) * 29000


@pytest.mark.parametrize("n", range(18))
def test_output_alignment(hq, pairs_worker, n):
    """One destination, a batch every 3 messages, source lengths 0 .. 17: batches (and workgroups'
    ranges) end and begin at every offset mod 16."""
    w, world, routes = pairs_worker
    hw.run_and_check(hq, world, None, routes, 1, 3, 1, bytes(range(n)), decode=n == 5)


def test_alignment_covers_every_residue(hq, pairs_worker):
    w, world, routes = pairs_worker
    seen = set()
    for n in range(18):
        b = w.heartbeat_batches(None, 1, bytes(range(n)), 1, 3)["batches"]
        seen |= set((b["offset"] % 16).tolist())
    assert seen == set(range(16))


def test_regrow(hq):
    """A fresh worker: the first call at 5000 groups grows every buffer (and, with a trailer behind
    every message, finds the first guess of the byte buffer short: the encode kernel runs again),
    then a smaller call, then the large one again."""
    G = 5000
    with hq.Worker(0, 8, on_device=True) as w:
        cids = list(range(1, G + 1))
        for c in cids:
            w.add_group(c, 1, 3, sc.LEADER, 40 + c, 50 + c, 30, [(1, 50 + c, 0, 0), (2, 45 + c, 0, 0),
                                                                 (3, 20 + c, 0, 0), (4, c, 1, 0)])
        rng = np.random.default_rng(9)
        routes = hw.random_routes(rng, G, 7)
        w.set_heartbeat_routes(0, routes)
        world = hw.World(w, cids)
        small = np.arange(100, 140, dtype=np.uint32)
        a, _ = hw.run_and_check(hq, world, None, routes, 7, 1, 5, b"x" * 40, decode=False)
        b, _ = hw.run_and_check(hq, world, small, routes, 7, 1, 5, b"x" * 40)
        c, _ = hw.run_and_check(hq, world, None, routes, 7, 1, 5, b"x" * 40, decode=False)
        assert len(a["bytes"]) > a["n_messages"] * 90 and a["n_messages"] > 13000
        np.testing.assert_array_equal(a["bytes"], c["bytes"])
        np.testing.assert_array_equal(a["batches"], c["batches"])
        hw.run_and_check(hq, world, None, routes, 7, 0, 5, b"")


def test_device_and_host_workers_agree(hq):
    rng = np.random.default_rng(78)
    groups = hbt.random_world(rng, 300)
    with hq.Worker(0, 8, on_device=True) as d, hq.Worker(0, 8) as h:
        for g in groups:
            d.add_group(*g[:8])
            h.add_group(*g[:8])
        hbt.step_world(hq, rng, [d, h], groups, 3)
        routes = hw.random_routes(rng, 300, 9)
        for w in (d, h):
            w.set_heartbeat_routes(0, routes)
        pick = rng.integers(0, 300, 500).astype(np.uint32)
        for handles in (None, pick):
            for bm in (0, 1, 7):
                a = d.heartbeat_batches(handles, 11, b"node-1:9", 9, bm)
                b = h.heartbeat_batches(handles, 11, b"node-1:9", 9, bm)
                for k in ("bytes", "batches"):
                    np.testing.assert_array_equal(a[k], b[k], err_msg=k)
                assert (a["n_messages"], a["n_unrouted"]) == (b["n_messages"], b["n_unrouted"])
                assert a["n_messages"] > 0 and a["n_unrouted"] > 0
        assert a["gpu_ns"] > 0 and b["gpu_ns"] == 0


def test_set_group_and_routes_are_flushed_first(hq):
    with hq.Worker(0, 8, on_device=True) as w:
        mem = [(1, 20, 0, 0), (2, 20, 0, 0), (3, 20, 0, 0)]
        w.add_group(5, 1, 2, sc.FOLLOWER, 20, 20, 18, mem)
        w.add_group(6, 1, 2, sc.LEADER, 20, 20, 18, mem)
        WorkerBackend(hq, worker=w).step({6: [("propose", 1)]})       # the state is on the device
        routes = host.rows([0, 1, 2, 1], [0, 1, 1])
        w.set_heartbeat_routes(0, routes)
        got, _ = hw.run_and_check(hq, hw.World(w, [5, 6]), None, routes, 3)
        assert got["n_messages"] == 2 and list(got["batches"]["dest"]) == [1]
        w.set_group(5, 1, 3, sc.LEADER, 20, 22, 21, [(1, 22, 0, 0), (2, 19, 0, 0), (3, 20, 0, 0),
                                                     (4, 0, 1, 0)])
        got, _ = hw.run_and_check(hq, hw.World(w, [5, 6]), None, routes, 3)   # no step in between
        assert got["n_messages"] == 5 and list(got["batches"]["dest"]) == [1, 2]
        routes[1] = [2, 0, hw.NONE] + [hw.NONE] * 13
        w.set_heartbeat_routes(1, routes[1:])                          # a route change alone
        got, _ = hw.run_and_check(hq, hw.World(w, [5, 6]), None, routes, 3)
        assert (got["n_messages"], got["n_unrouted"]) == (4, 1)
        assert list(got["batches"]["dest"]) == [0, 1, 2]
        # a group added after the column is on the device: no route, then routed
        w.add_group(7, 1, 2, sc.LEADER, 20, 20, 18, mem)
        routes = np.concatenate([routes, host.rows([])])
        got, _ = hw.run_and_check(hq, hw.World(w, [5, 6, 7]), None, routes, 3)
        assert (got["n_messages"], got["n_unrouted"]) == (4, 3)
        routes[2, :3] = [1, 1, 1]
        w.set_heartbeat_routes(2, routes[2:])
        got, _ = hw.run_and_check(hq, hw.World(w, [5, 6, 7]), None, routes, 3)
        assert (got["n_messages"], got["n_unrouted"]) == (6, 1)


def test_earlier_outputs_survive(hq):
    rng = np.random.default_rng(6)
    groups = hbt.random_world(rng, 200)
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
        hb = w.heartbeats(copy=False)
        hb_before = {k: hb[k].copy() for k in ("words", "lags", "ctxs")}
        assert hb["n_messages"] > 0 and len(hb["lags"]) > 0
        w.set_heartbeat_routes(0, hw.random_routes(rng, 200, 4))
        first = w.heartbeat_batches(None, 1, b"s", 4, 16, copy=False)
        keep = first["bytes"].copy()
        assert first["n_messages"] > 0
        for k in lists:
            np.testing.assert_array_equal(views[k], before[k], err_msg=k)
        for k in hb_before:
            np.testing.assert_array_equal(hb[k], hb_before[k], err_msg=k)
        w.heartbeats(np.arange(200, dtype=np.uint32)[::-1].copy())
        np.testing.assert_array_equal(first["bytes"], keep)    # valid until the next batches call


def test_errors_leave_the_worker_usable(hq):
    with hq.Worker(0, 8, on_device=True) as w:
        cids = host.follower_worker(w)
        host.check_errors(hq, w, cids)
        out = WorkerBackend(hq, worker=w).step({1: [sc.msg(sc.RREP, 2, 2, 20)]})
        assert out["_fallback"] == []
        hw.run_and_check(hq, hw.World(w, cids), None, host.rows(*[[0, 1, 2]] * 3), 3)


def test_nothing_to_send(hq):
    with hq.Worker(0, 8, on_device=True) as w:
        host.follower_worker(w)
        w.set_heartbeat_routes(0, host.rows([0, 0, 0], [0, 0, 0], [0, 0, 0]))
        for handles in (np.array([1, 2, 2], np.uint32), np.zeros(0, np.uint32)):
            got = w.heartbeat_batches(handles, 1, b"s", 1)
            assert len(got["batches"]) == 0 and len(got["bytes"]) == 0
            assert (got["n_messages"], got["n_unrouted"]) == (0, 0)
        w.set_heartbeat_routes(0, host.rows([], [0, 0, 0], [0, 0, 0]))
        got = w.heartbeat_batches(None, 1, b"s", 1)
        assert len(got["batches"]) == 0 and (got["n_messages"], got["n_unrouted"]) == (0, 2)
