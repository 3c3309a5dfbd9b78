"""The wire framing on the device (dragonboat_amd/csrc/hq_wire_frame_dev.hip) against the host
framer and decoder: hq_wire_frame_dev's verdicts must be hq_wire_frame_batch's, its spans must obey
the span rules and decode (hq_wire_decode_dev) to hq_wire_decode_batch's records, a batch of one
segment must give the host's spans exactly, and the device mode with the framing on the device
(hq_wire_set_device_framing) must give the outputs, stats and rejected list of the host-framed
device mode. Every comparison is exact. The segment walker itself is held to the host framer on
the CPU, under sanitizers, by test_wire_frame_segments.py."""
import ctypes

import numpy as np
import pytest

import step_random as sr
import step_scenarios as sc
import wire_cases
import wire_encode as we
from step_harness import OracleBackend, same_step
from test_gpu_wire_dev import CASES, SIZES, STATS, DeviceWireBackend
from test_wire_frame import message_of_len
from wire_cases import FIX

pytestmark = pytest.mark.gpu

FRAMED, MALFORMED, NO_FIT, UNCONFIRMED = 0, 1, 2, 3


def steady(n, seed=0):
    """n steady-state messages whose bytes hold no 0x0a (no `requests` tag inside a message), so
    that no segment's guess can go wrong before the batch's last fields."""
    rng = np.random.default_rng(seed)
    return [we.message(type=13, to=1, frm=int(rng.integers(1, 8)), cluster_id=int(rng.integers(1, 10)),
                       term=5, log_index=int(rng.integers(0, 10))) for _ in range(n)]


def host_frame(hq, data):
    """(spans, info) of hq_wire_frame_batch, or None where it returns HQ_E_INVAL."""
    try:
        return hq.frame_batch(data)
    except hq.HQError as e:
        assert e.code == hq.HQ_E_INVAL
        return None


def lay_out(batches, aligns):
    buf, refs = bytearray(), []
    for data, a in zip(batches, aligns):
        buf += bytes((a - len(buf)) % 16)
        refs.append((len(buf), len(data)))
        buf += data
    return bytes(buf), refs


def frame_and_check(hq, ctx, batches, aligns, S=0, pinned=False, decode=True):
    """The batches laid out in one buffer, framed by hq_wire_frame_dev with segments of S bytes
    and checked against the host; returns the results."""
    buf, refs = lay_out(batches, aligns)
    src = np.frombuffer(buf, np.uint8)
    if pinned:
        pin = ctx.pinned(max(1, len(buf)), np.uint8)
        pin[:len(buf)] = src
        src = pin[:len(buf)]
        assert hq.pointer_kind(pin) == hq.HQ_PTR_PINNED_HOST
    spans, span_batch, res, totals = hq.frame_dev(ctx, src, refs, S, data_len=len(buf))
    seg = S or hq.HQ_WIRE_FRAME_SEGMENT
    want, first, at = [], 0, 0
    for b, (data, (off, n)) in enumerate(zip(batches, refs)):
        host = host_frame(hq, data)
        status = int(res["status"][b])
        assert status in (FRAMED, MALFORMED, NO_FIT, UNCONFIRMED)
        if len(data) <= seg:
            assert status in (FRAMED, MALFORMED), (b, status)
        if status == MALFORMED:
            assert host is None, b
        if status != FRAMED:
            continue
        assert host is not None, b
        hspans, info = host
        for f in ("n_messages", "deployment_id", "source_address_len", "bin_ver"):
            assert int(res[f][b]) == getattr(info, f), (b, f)
        mine = spans[at:at + int(res["n_spans"][b])]
        assert (span_batch[at:at + len(mine)] == b).all()
        at += len(mine)
        # the span rules, and the messages' headers hopped from each span
        msgs = []
        for sp in mine:
            count, length, o = int(sp["count"]), int(sp["len"]), int(sp["offset"]) - off
            assert 1 <= count <= hq.HQ_WIRE_SPAN_MESSAGES and 0 <= o and o + length <= n
            if sp["flags"]:
                assert sp["flags"] == hq.HQ_WIRE_SPAN_LARGE and count == 1
                assert length > hq.HQ_WIRE_SPAN_BYTES
            else:
                assert length <= hq.HQ_WIRE_SPAN_BYTES
            assert int(sp["first"]) == first + len(msgs)
            p = o
            for _ in range(count):
                assert data[p] == 0x0A
                k, p = we_varint(data, p + 1)
                msgs.append((p, p + k))
                p += k
            assert p == o + length
        hmsgs = []
        for sp in hspans:
            p = int(sp["offset"])
            for _ in range(int(sp["count"])):
                k, p = we_varint(data, p + 1)
                hmsgs.append((p, p + k))
                p += k
        assert msgs == hmsgs, b
        if len(data) <= seg:                          # one segment: the host's spans
            h = hspans.copy()
            h["offset"] += off
            h["first"] += np.uint32(first)
            assert mine.tobytes() == h.tobytes(), b
        first += info.n_messages
        want.append(data)
    assert at == len(spans) == totals[1] and first == totals[0]
    if decode and first:
        got, status = hq.decode_dev(ctx, src, spans, first, data_len=len(buf))
        rows = []
        for data in want:
            # (a batch may hold a message the decoder rejects: compared message by message)
            for lo, hi in batch_messages(data):
                rows.append(data[lo:hi])
        assert len(rows) == first
        for i, body in enumerate(rows):
            one = we.f_bytes(1, body)
            try:
                m, _ = hq.decode_batch(one)
            except hq.HQError:
                assert status[i] == 1, i
                continue
            assert status[i] == 0 and got[i].tobytes() == m[0].tobytes(), i
    return res, spans, totals


def we_varint(b, p):
    v = shift = 0
    while True:
        x = b[p]
        p += 1
        v |= (x & 0x7F) << shift
        shift += 7
        if x < 0x80:
            return v, p


def batch_messages(data):
    """(body start, body end) of every message of a batch the host framer accepts."""
    import test_wire_frame as twf

    return [(f[2], f[3]) for f in twf.ref_walk(data)[0] if f[0] == "m"]


def parity_batches():
    """test_gpu_wire_dev.test_decode_parity's batches and alignments."""
    msgs = wire_cases.parity_messages()
    batches = [bytes.fromhex(fx["hex"]) for fx in FIX["batches"]]
    k = 0
    for a in range(16):
        for n in SIZES:
            batches.append(we.batch([msgs[(k + i) % len(msgs)] for i in range(n)], deployment_id=a,
                                    source_address=b"n:1"))
            k += n
    rng = np.random.default_rng(6)
    batches.append(we.batch([we.message(type=sc.RREP, to=1, frm=int(rng.integers(1, 8)),
                                        cluster_id=int(rng.integers(1, 128)), term=5,
                                        log_index=int(rng.integers(0, 128)))
                             for _ in range(200)], deployment_id=1))
    aligns = [0, 5, 11] + [a for a in range(16) for _ in SIZES] + [7]
    return batches, aligns


def test_parity_one_segment_batches(hq, gpu_ctx):
    batches, aligns = parity_batches()
    msgs = wire_cases.parity_messages()
    for n in (63, 64, 65):
        batches.append(we.batch(steady(n, n), deployment_id=n))
    batches.append(we.batch([msgs[0], message_of_len(4096 - 3), msgs[1], message_of_len(4097 - 3),
                             msgs[2]], deployment_id=2))
    m = [we.f_bytes(1, x) for x in msgs[:6]]
    batches.append(m[0] + m[1] + we.f_varint(2, 5) + m[2] + we.key(9, 5) + b"abcd" + m[3]
                   + we.f_bytes(3, b"a:1") + we.f_varint(4, 210) + m[4] + m[5])
    batches.append(b"")
    batches.append(we.batch([], deployment_id=77, source_address=b"n9:1"))
    aligns += [3, 9, 14, 1, 6, 0, 13]
    res, spans, totals = frame_and_check(hq, gpu_ctx, batches, aligns)
    assert (res["status"] == FRAMED).all()
    big = res[len(batches) - 4]
    assert int(big["n_messages"]) == 5
    # the 4097-byte message is a large span, the 4096-byte one is not
    assert sum(f == hq.HQ_WIRE_SPAN_LARGE for f in spans["flags"]) == 1
    assert int(res["n_messages"][-1]) == 0 and int(res["deployment_id"][-1]) == 77
    assert int(res["deployment_id"][-3]) == 5 and int(res["n_spans"][-3]) == 4


def multi_segment_cases():
    """(name, batch, segment bytes, must be framed): batches of several segments."""
    s = steady(40, 1)
    assert len(s[0]) + 2 == 50
    out = []
    # 3 segments of 256 bytes, a message across either edge (50-byte fields: 256 is no multiple)
    out.append(("three_segments", we.batch(s[:14], deployment_id=4, source_address=b"a-long-source:1"),
                256, True))
    # a message with 3000-byte entries across an edge of 4096
    big = we.message(type=3, cluster_id=4, entries=[we.entry(1, i, b"\x5a" * 3000) for i in range(2)])
    out.append(("entries_across_an_edge", we.batch(s[:60] + [big] + s[:30], deployment_id=4,
                                                   source_address=b"a-long-source:1"), 4096, True))
    # a message that covers a whole segment of 256 bytes (a void segment), then more messages
    out.append(("void_segment", we.batch(s[:3] + [message_of_len(700)] + s[3:20], deployment_id=1,
                                         source_address=b"a-long-source:1"), 256, True))
    # the default segment size: 200 KB of steady-state messages
    out.append(("steady_200k", we.batch(steady(4200, 2), deployment_id=1,
                                        source_address=b"a-long-source:1"), 0, True))
    # parity messages at small segments: wrong guesses may leave it unconfirmed, never wrong
    out.append(("parity_small_segments", we.batch(wire_cases.parity_messages()[:300], deployment_id=9),
                100, False))
    return out


@pytest.mark.parametrize("name,data,S,must", multi_segment_cases(),
                         ids=[c[0] for c in multi_segment_cases()])
def test_parity_batches_of_several_segments(hq, gpu_ctx, name, data, S, must):
    for align, pinned in ((0, False), (5, True)):
        res, spans, totals = frame_and_check(hq, gpu_ctx, [data, data], [align, 11], S, pinned=pinned)
        assert len(data) > 2 * (S or hq.HQ_WIRE_FRAME_SEGMENT)
        if must:
            assert (res["status"] == FRAMED).all(), name
        else:
            assert set(res["status"]) <= {FRAMED, UNCONFIRMED}


def test_rejection_parity(hq, gpu_ctx):
    """Every truncation and a set of single-byte replacements of the fixture batches (and of the
    three in one batch, cut into segments of 64 bytes), each a batch of its own, in one launch:
    status 1 exactly where the host returns HQ_E_INVAL."""
    fixtures = [bytes.fromhex(fx["hex"]) for fx in FIX["batches"]]
    joined = b"".join(fixtures) + we.f_varint(2, 7) + we.f_varint(4, 210)
    for S, raws in ((0, fixtures + [bytes.fromhex(fx["hex"]) for fx in FIX["malformed"]]),
                    (64, [joined])):
        batches = []
        for raw in raws:
            batches += [raw[:n] for n in range(len(raw) + 1)]
            for i, b in enumerate(raw):
                batches += [raw[:i] + bytes([v]) + raw[i + 1:] for v in (0x00, 0x7F, 0x80, 0xFF, b ^ 1,
                                                                         b ^ 0x80)]
        res, _, _ = frame_and_check(hq, gpu_ctx, batches, [i % 16 for i in range(len(batches))], S,
                                    decode=False)
        host = np.array([host_frame(hq, b) is None for b in batches])
        assert host.any() and not host.all()
        if S == 0:
            np.testing.assert_array_equal(res["status"] == MALFORMED, host)
        else:       # several segments: unconfirmed at worst, and mostly not
            np.testing.assert_array_equal((res["status"] == MALFORMED) & host, res["status"] == MALFORMED)
            assert ((res["status"] == FRAMED) <= ~host).all()
            assert (res["status"] == MALFORMED).any() and (res["status"] == FRAMED).any()


def test_arguments(hq, gpu_ctx):
    data = we.batch(steady(10), deployment_id=1)
    with pytest.raises(hq.HQError) as e:
        hq.frame_dev(gpu_ctx, data, [(0, len(data))], 63)
    assert e.value.code == hq.HQ_E_INVAL
    # a batch that does not lie within the bytes; spans that do not fit the list
    spans, sb, res, totals = hq.frame_dev(gpu_ctx, data, [(0, len(data)), (8, len(data))], 0)
    assert list(res["status"]) == [FRAMED, MALFORMED] and totals == (10, 1)
    many = we.batch(steady(130), deployment_id=1)
    spans, sb, res, totals = hq.frame_dev(gpu_ctx, many + many, [(0, len(many)), (len(many), len(many))],
                                          0, span_cap=4)
    assert list(res["status"]) == [FRAMED, NO_FIT] and totals == (260, 6) and len(spans) == 4
    assert list(spans["first"]) == [0, 64, 128, 130] and list(sb) == [0, 0, 0, 1]


# ---- the device mode with the framing on the device ------------------------------------------------

def decoy_batch(S):
    """A large message that holds a run of fake `requests` headers (0a 02 08 00) exactly at a
    segment's start and ends inside that segment: the segment's guess takes the run."""
    head, tail = steady(200, 3), steady(100, 4)
    run = bytes.fromhex("0a020800") * 300
    fill = S - 200 * 50 - 64
    for _ in range(3):
        big = we.message(type=3, cluster_id=2, term=5, entries=[we.entry(1, 1, b"\x5a" * fill + run)])
        data = we.batch(head + [big] + tail, deployment_id=7, source_address=b"n2:1")
        edge = data.find(run[:16])
        if edge == S:
            break
        fill += S - edge
    assert edge == S and S < len(data) < 2 * S
    return data


def _results_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k.endswith("_ns"):                          # (timings)
            continue
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_decoy(hq, gpu_ctx):
    S = hq.HQ_WIRE_FRAME_SEGMENT
    data = decoy_batch(S)
    res, spans, totals = frame_and_check(hq, gpu_ctx, [data], [0])
    assert int(res["status"][0]) in (FRAMED, UNCONFIRMED)
    unconfirmed = int(res["status"][0]) == UNCONFIRMED
    clean = we.batch(steady(4200, 5), deployment_id=7, source_address=b"n2:1")
    mem = [(i, 9, sc.REMOTE, 0) for i in range(1, 4)]
    workers = [hq.Worker(0, 3, on_device=True) for _ in range(2)]
    wires = [hq.Wire(7) for _ in range(2)]
    try:
        for w, wire in zip(workers, wires):
            for cid in range(1, 10):
                w.add_group(cid, 1, 5, sc.LEADER, 9, 9, 9, mem)
            wire.attach_device(w)
        wires[1].set_device_framing(True)
        for step, batches in enumerate(([data], [clean], [clean, data, b"\x0a\x05"])):
            outs = []
            for wire in wires:
                wire.reset()
                rejected_at_once = []
                for i, b in enumerate(batches):
                    try:
                        wire.add_batch(b)
                    except hq.HQError:
                        rejected_at_once.append(i)
                out, st = wire.step_device()
                outs.append((out, st, rejected_at_once + list(wire.device_rejected())))
            _results_equal(outs[0][0], outs[1][0])
            for k in STATS:
                assert getattr(outs[0][1], k) == getattr(outs[1][1], k), k
            assert outs[0][2] == outs[1][2]
            segments, voids, open_batches, reframed = wires[1].device_frame_stats()
            if step == 0:
                assert segments == 2 and outs[1][1].messages == 301
                assert (open_batches, reframed) == ((1, 1) if unconfirmed else (0, 0))
            elif step == 1:                            # framed on the device: nothing left open
                assert segments == 4 and open_batches == 0 and outs[1][1].messages == 4200
                assert reframed == (1 if unconfirmed else 0)
            else:
                assert segments == 7 and outs[1][2] == [2]
                assert reframed == (2 if unconfirmed else 0)
    finally:
        for wire in wires:
            wire.close()
        for w in workers:
            w.close()


class _FramedWire:
    """The backend's wire with the framing on the device. add_batch raises for a batch the host
    framer rejects, as the host-framed mode does at once (so that the arrival stream of
    DeviceWireBackend runs unchanged), and expects that batch in the step's rejected list instead,
    from which device_rejected takes it out again."""

    def __init__(self, hq, wire):
        self._hq, self._wire = hq, wire
        self.calls = 0
        self.framing_errors = []
        self.framing_errors_seen = 0

    def __getattr__(self, name):
        return getattr(self._wire, name)

    def reset(self):
        self.calls = 0
        self.framing_errors = []
        self._wire.reset()

    def _count(self, data):
        index = self.calls
        self.calls += 1
        if host_frame(self._hq, bytes(data)) is None:
            self.framing_errors.append(index)
            raise self._hq.HQError(self._hq.HQ_E_INVAL, "framing error: listed at the step")

    def add_batch(self, data):
        self._wire.add_batch(data)                     # (HQ_OK for any bytes)
        self._count(data)

    def add_batch_at(self, addr, n):
        self._wire.add_batch_at(addr, n)
        self._count(ctypes.string_at(addr, n))

    def device_rejected(self):
        got = list(self._wire.device_rejected())
        assert got == sorted(got) and set(self.framing_errors) <= set(got)
        self.framing_errors_seen += len(self.framing_errors)
        segments, voids, open_batches, reframed = self._wire.device_frame_stats()
        assert segments >= 3 and (open_batches, reframed) == (0, 0)
        return [i for i in got if i not in self.framing_errors]


class FramedWireBackend(DeviceWireBackend):
    """DeviceWireBackend (its arrival stream, its foreign, poisoned and truncated batches, its
    shadow for the stats) with hq_wire_set_device_framing."""

    def __init__(self, hq, n_max=8, seed=0, worker=None):
        super().__init__(hq, n_max, seed, worker)
        self.wire.set_device_framing(True)
        self.wire = _FramedWire(hq, self.wire)

    def build_inputs(self, per_group):
        out = super().build_inputs(per_group)
        with pytest.raises(self.hq.HQError):           # a framing error in every step
            self.wire.add_batch(bytes.fromhex("0a05080d10"))
        return out


@pytest.fixture(scope="module")
def framed_wire_backend(hq):
    b = FramedWireBackend(hq, n_max=8, seed=5)
    yield b
    assert b.in_place > 0 and b.staged > 0 and b.wire.framing_errors_seen > 0
    b.close()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reference_scenario_framed_on_device(framed_wire_backend, case):
    outs, state = sc.run_case(framed_wire_backend, case)
    sc.check_case(case, outs, state)
    want_outs, want_state = sc.run_case(OracleBackend(), case)
    assert state == want_state, case["name"]
    for w, o in zip(outs, want_outs):
        for k in ("committed", "commit_changed", "ready", "resps", "states", "dropped",
                  "deferred"):
            assert w[k] == o[k], (case["name"], k, w[k], o[k])


@pytest.mark.parametrize("seed,G,steps", [(11, 1500, 6), (12, 300, 15)])
def test_random_differential_framed_on_device(hq, seed, G, steps):
    rng = np.random.default_rng(seed)
    groups = sr.random_groups(rng, G)
    late = groups[-20:]
    o, w = OracleBackend(), FramedWireBackend(hq, n_max=8, seed=seed)
    try:
        for g in groups[:-20]:
            o.add_group(*g)
            w.add_group(*g)
        have = groups[:-20]
        ctx_seq = [0]
        for s in range(steps):
            if s == 2:
                for g in late:
                    o.add_group(*g)
                    w.add_group(*g)
                have = groups
            per = {}
            for g in have:
                if rng.random() < 0.85:
                    per[g[0]] = sr.random_events(rng, o.state(g[0]), s + 1, ctx_seq)
            want = o.step(per)
            got = w.step(per)                          # (stats and rejected list: _DeviceStep)
            st = w.last_stats
            assert st.dropped_batches == 1 and st.batches >= 2
            assert got["_fallback"] == []
            for cid in per:
                same_step(want, got, cid)
            for g in have:
                assert w.state(g[0]) == o.state(g[0]), (s, g[0])
        assert w.wire.framing_errors_seen >= steps          # (and the stream's truncated batch)
        assert w.in_place == steps and w.staged >= 2 * steps
    finally:
        w.close()


def test_mode_errors(hq):
    host, dev = hq.Worker(0, 3), hq.Worker(0, 3, on_device=True)
    wire = hq.Wire(7)
    try:
        def code(f, *a):
            with pytest.raises(hq.HQError) as e:
                f(*a)
            return e.value.code

        assert code(wire.set_device_framing, True) == hq.HQ_E_STATE      # not attached
        assert code(wire.device_frame_stats) == hq.HQ_E_STATE
        wire.attach(host)
        assert code(wire.set_device_framing, True) == hq.HQ_E_STATE      # the host mode
        dev.add_group(1, 1, 1, sc.LEADER, 1, 1, 1, [(1, 1, 0, 0)])
        wire.attach_device(dev)
        wire.set_device_framing(True)
        wire.add_batch(bytes.fromhex("0a05080d10"))                      # any bytes: queued
        assert code(wire.set_device_framing, False) == hq.HQ_E_STATE     # a batch queued
        assert code(wire.attach, dev) == hq.HQ_E_STATE
        res, st = wire.step_device()
        assert list(wire.device_rejected()) == [0] and st.batches == 0 and st.bytes == 0
        assert wire.device_frame_stats() == (1, 0, 0, 0)
        wire.reset()
        res, st = wire.step_device()                                     # nothing queued
        assert len(wire.device_rejected()) == 0 and wire.device_frame_stats() == (0, 0, 0, 0)
        wire.add_batch(b"")
        wire.add_batch(we.batch([], deployment_id=8))
        res, st = wire.step_device()
        assert (st.batches, st.dropped_batches, st.messages) == (2, 2, 0)
        wire.reset()
        wire.set_device_framing(False)
        with pytest.raises(hq.HQError):                                  # framed at once again
            wire.add_batch(bytes.fromhex("0a05080d10"))
    finally:
        wire.close()
        host.close()
        dev.close()
