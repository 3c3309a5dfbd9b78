"""hq_worker_heartbeat_batches on a host worker, and the shared marshaller
(dragonboat_amd/csrc/hq_heartbeat_wire.h) under sanitizers in a program of its own. Expected values
come from tests/heartbeat_wire_ref.py: heartbeat_ref.broadcast over Worker.get_group, the routes
looked up in Python, wire_encode.batch for the bytes; every batch also goes through
hq_wire_decode_batch.

A host worker opens a device context like every worker (its decisions run in GPU passes), so the
worker tests carry the gpu mark; the marshaller's sanitizer program needs no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import heartbeat_ref as ref
import heartbeat_wire_ref as hw
import step_scenarios as sc
import test_gpu_heartbeat as hbt
from step_harness import WorkerBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = ref.kats()
needs_device = pytest.mark.gpu      # hq_worker_open needs a HIP device, for a host worker too
EDGES = [127, 128, (1 << 14) - 1, 1 << 14, 1 << 32, 1 << 63, (1 << 64) - 1]


def rows(*routes):
    """Route rows: each argument the routes of a group's first members, HQ_ROUTE_NONE after."""
    out = np.full((len(routes), 16), hw.NONE, np.uint16)
    for k, r in enumerate(routes):
        out[k, :len(r)] = r
    return out


def kat_worker(hq, w):
    """The reference's tables on worker w, the ctx made pending by a local ReadIndex."""
    for c in KATS:
        hbt.add_kat(w, c)
    reads = {c["group"]["cluster_id"]: [("read", c["ctx"][0], c["ctx"][1])]
             for c in KATS if tuple(c["ctx"]) != (0, 0)}
    if reads:
        WorkerBackend(hq, worker=w).step(reads)
    return [c["group"]["cluster_id"] for c in KATS]


def check_kats(hq, w):
    cids = kat_worker(hq, w)
    routes = np.tile(np.arange(16, dtype=np.uint16) % 3, (len(cids), 1))
    w.set_heartbeat_routes(0, routes)
    world = hw.World(w, cids)
    for bm in (0, 1, 2):
        got, want = hw.run_and_check(hq, world, None, routes, 3, bm, 0x1234, b"10.0.0.1:63001")
        sent = [(f["cluster_id"], f["to"], f["term"], f["commit"], f["hint"], f["hint_high"])
                for _, msgs, _ in want for f in msgs]
        table = [(c["group"]["cluster_id"], x["to"], c["group"]["term"], x["commit"], x["hint"],
                  x["hint_high"]) for c in KATS for x in c["want"]]
        assert sorted(sent) == sorted(table) and got["n_unrouted"] == 0


@needs_device
def test_reference_tables(hq):
    with hq.Worker(0, 8) as w:
        check_kats(hq, w)


@pytest.fixture(scope="module")
def world300(hq):
    """300 random groups after random steps, some leaders suspended."""
    rng = np.random.default_rng(4242)
    groups = hbt.random_world(rng, 300)
    w = hq.Worker(0, 8)
    for g in groups:
        w.add_group(*g[:8])
    hbt.step_world(hq, rng, [w], groups, 3)
    yield rng, w, hw.World(w, [g[0] for g in groups])
    w.close()


@needs_device
@pytest.mark.parametrize("bm", [0, 1, 5])
@pytest.mark.parametrize("n_dest", [1, 3, 300])
def test_random_world(hq, world300, n_dest, bm):
    rng, w, world = world300
    G = len(world.cids)
    routes = hw.random_routes(rng, G, n_dest, none=0.1)
    leaders = [h for h in range(G) if world.messages(h)]
    never = leaders[-1]                           # a leader whose routes are never set
    routes[leaders[0]] = routes[never] = hw.NONE  # and one whose members all have no route
    w.set_heartbeat_routes(0, routes[:never])
    w.set_heartbeat_routes(never + 1, routes[never + 1:])
    got, want = hw.run_and_check(hq, world, None, routes, n_dest, bm)
    assert got["n_unrouted"] >= len(world.messages(never)) + len(world.messages(leaders[0]))
    assert got["n_messages"] > 300
    assert got["gpu_ns"] == 0
    pick = rng.integers(0, G, 400).astype(np.uint32)
    hw.run_and_check(hq, world, pick, routes, n_dest, bm, 0, b"")


def edge_group(w, cid, node, term, other, committed, match):
    w.add_group(cid, node, term, sc.LEADER, committed, max(committed, match), min(committed, 1),
                [(node, max(committed, match), sc.REMOTE, 0), (other, match, sc.REMOTE, 0)])


@needs_device
def test_varint_edges(hq):
    """Each field in turn at the varint length edges, the others small; the smallest (50 bytes) and
    the largest (113 bytes) message."""
    with hq.Worker(0, 8) as w:
        cids, reads = [], {}
        for k, v in enumerate(EDGES):
            base = 100 * (k + 1)
            for j, (cid, node, term, other, com, match, ctx) in enumerate([
                    (v, 1, 2, 2, 9, 9, None),                 # cluster id (asserted distinct below)
                    (base + 1, v, 2, 2, 9, 9, None),          # From
                    (base + 2, 1, 2, v, 9, 9, None),          # To
                    (base + 3, 1, v, 2, 9, 9, None),          # Term
                    (base + 4, 1, 2, 2, v, v, None),          # Commit = committed
                    (base + 5, 1, 2, 2, v, v - 1, None),      # Commit = match
                    (base + 6, 1, 2, 2, 9, 9, (v, 0)),        # Hint
                    (base + 7, 1, 2, 2, 9, 9, (0, v)),        # HintHigh
                    (base + 8, 1, 2, 2, 9, 9, (v, v))]):
                if j == 0 and cid in cids:
                    continue
                edge_group(w, cid, node, term, other, com, match)
                cids.append(cid)
                if ctx:
                    reads[cid] = [("read", ctx[0], ctx[1])]
        small, big = 5, (1 << 63) + 5
        edge_group(w, small, 1, 2, 2, 9, 9)
        top = (1 << 64) - 1
        edge_group(w, big, top - 1, 1 << 63, top, top - 2, top - 3)
        reads[big] = [("read", top, 1 << 63)]
        cids += [small, big]
        assert len(set(cids)) == len(cids)
        out = WorkerBackend(hq, worker=w).step(reads)
        assert all(out[c]["dropped"] == [] for c in reads)
        routes = rows(*[[0, 0]] * len(cids))
        w.set_heartbeat_routes(0, routes)
        world = hw.World(w, cids)
        got, want = hw.run_and_check(hq, world, None, routes, 1, 1)
        sizes = [int(t["len"]) - len(we_trailer()) for t in got["batches"]]
        assert len(sizes) == len(cids) and min(sizes) == 50 and max(sizes) == 113
        assert sizes[-2:] == [50, 113]
        fields = [m[0] for _, m, _ in want]
        assert any(f["hint"] == top and f["hint_high"] == 1 << 63 and f["commit"] == top - 3
                   for f in fields)
        hw.run_and_check(hq, world, None, routes, 1, 0)


def we_trailer():
    return hw.we.batch([], 7, b"host-a:1")


@needs_device
@pytest.mark.parametrize("n", [0, 1, 127, 128, 256])
def test_source_lengths(hq, n):
    with hq.Worker(0, 8) as w:
        cids = kat_worker(hq, w)
        routes = rows(*[[0, 1, 0]] * len(cids))
        w.set_heartbeat_routes(0, routes)
        src = bytes((7 * i + n) & 0xFF for i in range(n))
        hw.run_and_check(hq, hw.World(w, cids), None, routes, 2, 1, (1 << 64) - 1, src)
        if n == 256:
            with pytest.raises(hq.HQError, match="256 bytes"):
                w.heartbeat_batches(None, 1, src + b"x", 2)
            hw.run_and_check(hq, hw.World(w, cids), None, routes, 2, 0, 1, src)


def check_errors(hq, w, cids):
    """The refused calls of a worker holding the groups `cids` (three members each at least), and
    that it stays usable."""
    G = len(cids)
    good = rows(*[[0, 1, 2]] * G)
    w.set_heartbeat_routes(0, good)
    world = hw.World(w, cids)
    hw.run_and_check(hq, world, None, good, 3)
    err = lambda: hq.lib.hq_worker_last_error(w.h)
    # a route at n_dest; a member's route is checked whatever the group sends
    for bad_row in range(G):
        bad = good.copy()
        bad[bad_row, 1] = 3
        w.set_heartbeat_routes(bad_row, bad[bad_row:bad_row + 1])
        with pytest.raises(hq.HQError, match="route"):
            w.heartbeat_batches(None, 1, b"s", 3)
        assert b"route" in err()
        w.heartbeat_batches(None, 1, b"s", 4)              # (a destination 3 exists now)
        w.set_heartbeat_routes(bad_row, good[bad_row:bad_row + 1])
        hw.run_and_check(hq, world, None, good, 3)
    for n_dest in (0, 65536, 1 << 31):
        with pytest.raises(hq.HQError, match="n_dest"):
            w.heartbeat_batches(None, 1, b"s", n_dest)
    out = hq.HeartbeatBatches()
    cfg = hq.HeartbeatWireConfig(1, None, 0, 3, 0)
    assert hq.lib.hq_worker_heartbeat_batches(w.h, G, None, None, ctypes.byref(out)) == hq.HQ_E_INVAL
    assert b"NULL" in err()
    assert hq.lib.hq_worker_heartbeat_batches(w.h, G, None, ctypes.byref(cfg), None) == hq.HQ_E_INVAL
    assert hq.lib.hq_worker_heartbeat_batches(w.h, 1 << 28, None, ctypes.byref(cfg),
                                              ctypes.byref(out)) == hq.HQ_E_INVAL
    assert b"2^28" in err()
    for handles in ([0, G], [0xFFFFFFFF]):
        with pytest.raises(hq.HQError, match="unknown group handle"):
            w.heartbeat_batches(np.array(handles, np.uint32), 1, b"s", 3)
    assert hq.lib.hq_worker_heartbeat_batches(w.h, G + 1, None, ctypes.byref(cfg),
                                              ctypes.byref(out)) == hq.HQ_E_INVAL
    with pytest.raises(hq.HQError, match="unknown group handle"):
        w.set_heartbeat_routes(G, good[:1])
    with pytest.raises(hq.HQError, match="unknown group handle"):
        w.set_heartbeat_routes(1, good)
    hw.run_and_check(hq, world, np.array([G - 1, 0, 0], np.uint32), good, 3, 2)


def follower_worker(w):
    mem = [(1, 20, 0, 0), (2, 19, 0, 0), (3, 20, 0, 0)]
    w.add_group(1, 1, 2, sc.LEADER, 20, 20, 18, mem)
    w.add_group(2, 1, 2, sc.FOLLOWER, 20, 20, 18, mem)
    w.add_group(3, 1, 2, sc.CANDIDATE, 20, 20, 18, mem)
    return [1, 2, 3]


@needs_device
def test_errors_leave_the_worker_usable(hq):
    with hq.Worker(0, 8) as w:
        check_errors(hq, w, follower_worker(w))


@needs_device
def test_nothing_to_send(hq):
    with hq.Worker(0, 8) as w:
        follower_worker(w)
        w.set_heartbeat_routes(0, rows([0, 0, 0], [0, 0, 0], [0, 0, 0]))
        for handles in (np.array([1, 2, 2], np.uint32), np.zeros(0, np.uint32)):
            got = w.heartbeat_batches(handles, 1, b"s", 1)
            assert len(got["batches"]) == 0 and len(got["bytes"]) == 0
            assert (got["n_messages"], got["n_unrouted"]) == (0, 0)
        w.set_heartbeat_routes(0, rows([], [0, 0, 0], [0, 0, 0]))      # a leader without routes
        got = w.heartbeat_batches(None, 1, b"s", 1)
        assert len(got["batches"]) == 0 and (got["n_messages"], got["n_unrouted"]) == (0, 2)


@needs_device
def test_earlier_outputs_stay_valid(hq, world300):
    rng, w, world = world300
    G = len(world.cids)
    routes = hw.random_routes(rng, G, 5)
    w.set_heartbeat_routes(0, routes)
    first = w.heartbeat_batches(None, 1, b"s", 5, copy=False)
    keep = {k: first[k].copy() for k in ("bytes", "batches")}
    hb = w.heartbeats(copy=False)
    hb_keep = {k: hb[k].copy() for k in ("words", "lags", "ctxs")}
    assert len(hb_keep["lags"]) > 0
    got = w.heartbeat_batches(None, 1, b"s", 5)
    for k in hb_keep:                      # the compact output survives the call
        np.testing.assert_array_equal(hb[k], hb_keep[k], err_msg=k)
    for k in keep:                         # and the same state gives the same bytes
        np.testing.assert_array_equal(got[k], keep[k], err_msg=k)
    w.heartbeats(np.arange(10, dtype=np.uint32))
    after = w.heartbeat_batches(None, 1, b"s", 5, copy=False)
    np.testing.assert_array_equal(after["bytes"], keep["bytes"])


SANITIZER_MAIN = r"""
// hq_heartbeat_wire.h against a second writer (a plain protobuf writer over a std::vector): some
// 100,000 pseudo-random Heartbeats with every field at the varint length edges, cut into batches
// with sources of 0 .. 256 bytes, each batch marshalled into a heap buffer of exactly its size.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hq_heartbeat_wire.h"

static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t value() {
    const uint64_t r = next();
    const unsigned bits = (unsigned)(r % 65);             // 0 .. 64 significant bits
    uint64_t v = bits == 0 ? 0 : bits == 64 ? next() | (1ull << 63)
                                             : (next() & ((1ull << bits) - 1)) | (1ull << (bits - 1));
    switch ((r >> 8) % 8) {                               // or exactly at a varint length edge
        case 0: v = (1ull << (7 * (1 + (r >> 16) % 9))) - 1; break;
        case 1: v = 1ull << (7 * (1 + (r >> 16) % 9)); break;
        case 2: v = ~0ull; break;
        default: break;
    }
    return v;
}
static void ref_varint(std::vector<uint8_t> &o, uint64_t v) {
    do {
        uint8_t b = v & 0x7F;
        v >>= 7;
        o.push_back(v ? b | 0x80 : b);
    } while (v);
}
static void ref_field(std::vector<uint8_t> &o, unsigned field, uint64_t v) {
    ref_varint(o, field << 3);
    ref_varint(o, v);
}
static void ref_bytes(std::vector<uint8_t> &o, unsigned field, const std::vector<uint8_t> &b) {
    ref_varint(o, field << 3 | 2);
    ref_varint(o, b.size());
    o.insert(o.end(), b.begin(), b.end());
}
static std::vector<uint8_t> ref_message(const hb_fields &f) {
    std::vector<uint8_t> m, snap, membership;
    ref_field(membership, 1, 0);
    ref_bytes(snap, 2, {});
    for (unsigned k : {3u, 4u, 5u}) ref_field(snap, k, 0);
    ref_bytes(snap, 6, membership);
    for (unsigned k : {9u, 10u, 11u, 12u, 13u, 14u}) ref_field(snap, k, 0);
    const uint64_t v[10] = {17, f.to, f.from, f.cluster_id, f.term, 0, 0, f.commit, 0, f.hint};
    for (unsigned k = 0; k < 10; ++k) ref_field(m, k + 1, v[k]);
    ref_bytes(m, 12, snap);
    ref_field(m, 13, f.hint_high);
    return m;
}

// with arguments (to from cluster_id term commit hint hint_high deployment_id source_len): that
// one-message batch in hex, the source bytes 0, 1, 2, ...
static int one_batch(char **a) {
    uint64_t v[9];
    for (int i = 0; i < 9; ++i) v[i] = strtoull(a[i], nullptr, 10);
    const hb_fields f{v[0], v[1], v[2], v[3], v[4], v[5], v[6]};
    const uint32_t source_len = (uint32_t)v[8];
    const uint64_t size = hb_msg_size(f) + hb_trailer_size(v[7], source_len);
    uint8_t *buf = new uint8_t[size], *src = new uint8_t[source_len ? source_len : 1];
    for (uint32_t i = 0; i < source_len; ++i) src[i] = (uint8_t)i;
    uint8_t *p = hb_trailer_put(hb_msg_put(buf, f), v[7], src, source_len);
    if ((uint64_t)(p - buf) != size) return 1;
    for (uint64_t i = 0; i < size; ++i) printf("%02x", buf[i]);
    printf("\n");
    delete[] buf;
    delete[] src;
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 10) return one_batch(argv + 1);
    uint64_t messages = 0, bytes = 0;
    uint32_t smallest = ~0u, largest = 0;
    for (unsigned batch = 0; messages < 100000; ++batch) {
        const unsigned n = (unsigned)(next() % 40);
        const uint32_t source_len = batch < 257 ? batch : (uint32_t)(next() % 257);
        const uint64_t deployment_id = value();
        std::vector<uint8_t> source(source_len);
        for (auto &b : source) b = (uint8_t)next();
        std::vector<hb_fields> fs(n);
        std::vector<uint8_t> want;
        uint64_t size = 0;
        for (auto &f : fs) {
            f = hb_fields{value(), value(), value(), value(), value(), value(), value()};
            if (next() % 16 == 0) f = hb_fields{1, 2, 3, 4, 5, 0, 0};
            if (next() % 16 == 0) f = hb_fields{~0ull, ~1ull, ~2ull, ~3ull, ~4ull, ~5ull, ~6ull};
            ref_bytes(want, 1, ref_message(f));
            const uint32_t one = hb_msg_size(f);
            if (one < kHbMsgMin || one > kHbMsgMax) return printf("size %u\n", one), 1;
            smallest = one < smallest ? one : smallest;
            largest = one > largest ? one : largest;
            size += one;
        }
        ref_field(want, 2, deployment_id);
        ref_bytes(want, 3, source);
        ref_field(want, 4, 210);
        const uint32_t trailer = hb_trailer_size(deployment_id, source_len);
        if (trailer > kHbTrailerMax) return printf("trailer %u\n", trailer), 1;
        size += trailer;
        if (size != want.size()) return printf("batch %u: %llu bytes, want %zu\n", batch,
                                               (unsigned long long)size, want.size()), 1;
        uint8_t *buf = new uint8_t[size], *p = buf;       // exactly sized: a byte too many is caught
        // (an empty source is passed as NULL: nothing of it may be read)
        const uint8_t *src = source_len ? new uint8_t[source_len] : nullptr;
        if (source_len) std::memcpy(const_cast<uint8_t *>(src), source.data(), source_len);
        for (const auto &f : fs) {
            uint8_t *q = hb_msg_put(p, f);
            if (q - p != hb_msg_size(f)) return printf("batch %u: put and size differ\n", batch), 1;
            p = q;
        }
        p = hb_trailer_put(p, deployment_id, src, source_len);
        if ((uint64_t)(p - buf) != size || std::memcmp(buf, want.data(), size))
            return printf("batch %u differs\n", batch), 1;
        delete[] buf;
        delete[] src;
        messages += n;
        bytes += size;
    }
    if (smallest != 50 || largest != 113) return printf("sizes %u .. %u\n", smallest, largest), 1;
    printf("ok %llu %llu\n", (unsigned long long)messages, (unsigned long long)bytes);
    return 0;
}
"""


@pytest.fixture(scope="module")
def sweep_program(tmp_path_factory):
    """The shared marshaller compiled into a program of its own with -fsanitize=address,undefined;
    no Python process loads sanitized code."""
    d = tmp_path_factory.mktemp("heartbeat_wire")
    src, exe = d / "heartbeat_wire_sweep.cpp", d / "heartbeat_wire_sweep"
    src.write_text(SANITIZER_MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "dragonboat_amd", "csrc"), "-o", str(exe), str(src)],
                   check=True)
    return str(exe)


def test_sanitizer_marshaller_stand_alone(sweep_program):
    """Some 100,000 pseudo-random Heartbeats against a second writer in the same program, each
    batch in a heap buffer of exactly its size."""
    r = subprocess.run([sweep_program], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "" and r.stdout.startswith("ok ")
    assert int(r.stdout.split()[1]) >= 100000


def test_marshaller_matches_wire_encode(sweep_program):
    """The same program's one-batch form against tests/wire_encode.py: each field in turn at the
    varint length edges, the smallest and the largest message, source lengths around 128."""
    top = (1 << 64) - 1
    cases = [([1, 2, 3, 4, 5, 0, 0], 0, 0), ([top] * 7, top, 256)]
    for v in EDGES:
        for k in range(7):
            f = [1, 2, 3, 4, 5, 6, 7]
            f[k] = v
            cases.append((f, v, len(cases) % 3))
    cases += [([9] * 7, 300, n) for n in (1, 127, 128, 255)]
    for f, dep, n in cases:
        r = subprocess.run([sweep_program] + [str(x) for x in f + [dep, n]], capture_output=True,
                           text=True)
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
        m = hw.we.message(type=17, to=f[0], frm=f[1], cluster_id=f[2], term=f[3], commit=f[4],
                          hint=f[5], hint_high=f[6])
        assert bytes.fromhex(r.stdout.strip()) == hw.we.batch([m], dep, bytes(range(n))), (f, dep, n)
    assert len(hw.we.message(type=17, to=1, frm=2, cluster_id=3, term=4, commit=5)) == 48
    assert len(hw.we.message(type=17, to=top, frm=top, cluster_id=top, term=top, commit=top, hint=top,
                             hint_high=top)) == 111
