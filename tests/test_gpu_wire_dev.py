"""The wire decode on the device (dragonboat_amd/csrc/hq_wire_dev.hip) against the host decoder
(hq_wire_decode_batch): hq_wire_frame_batch's spans decoded by hq_wire_decode_dev must give the
host decoder's records field for field, and reject exactly the messages it rejects. Every
comparison is exact. Both decoders are hq_wire_codec.h compiled twice, so the messages are
wire_cases.py's, on which test_wire_codec.py holds the host decoder to the referee
(wire_decode_ref.py); the rejections are held to the referee here as well."""
import ctypes

import numpy as np
import pytest

import step_random as sr
import step_scenarios as sc
import wire_cases
import wire_decode_ref as ref
import wire_encode as we
from step_harness import OracleBackend, WireBackend, check_phase_order, event_record, same_step
from wire_cases import FIX, random_fields

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 200)


def host_decode_one(hq, body):
    """(rejected, record) of the host decoder for the one-message batch holding `body`."""
    data = np.frombuffer(we.f_bytes(1, bytes(body)), np.uint8)
    out = np.zeros(1, hq.WIRE_MESSAGE_DTYPE)
    n = ctypes.c_uint64(0)
    rc = hq.lib.hq_wire_decode_batch(hq._p(data), len(data), hq._p(out), 1, ctypes.byref(n), None)
    assert rc in (hq.HQ_OK, hq.HQ_E_INVAL)
    return rc != hq.HQ_OK, out[0]


@pytest.fixture(scope="module")
def parity_messages():
    return wire_cases.parity_messages()


def lay_out(hq, batches, aligns):
    """The batches in one buffer, batch j starting `aligns[j]` past a 16-byte boundary; their
    spans (offsets and first indices in the whole) and the host decoder's records."""
    buf, spans, want = bytearray(), [], []
    for data, a in zip(batches, aligns):
        buf += bytes((a - len(buf)) % 16)
        sp, info = hq.frame_batch(data, base=len(buf), first=len(want))
        msgs, dinfo = hq.decode_batch(data)
        assert info.n_messages == dinfo.n_messages == len(msgs)
        spans.append(sp)
        want.extend(msgs[:dinfo.n_messages])
        buf += data
    return (np.frombuffer(bytes(buf), np.uint8), np.concatenate(spans),
            np.array(want, hq.WIRE_MESSAGE_DTYPE))


def test_decode_parity(hq, gpu_ctx, parity_messages):
    batches = [bytes.fromhex(fx["hex"]) for fx in FIX["batches"]]
    k = 0
    for a in range(16):
        for n in SIZES:
            batches.append(we.batch([parity_messages[(k + i) % len(parity_messages)]
                                     for i in range(n)], deployment_id=a, source_address=b"n:1"))
            k += n
    assert k >= len(parity_messages)                 # every message, both encodings
    # steady-state messages (one-byte varints): whole 64-message spans
    rng = np.random.default_rng(6)
    batches.append(we.batch([we.message(type=sc.RREP, to=1, frm=int(rng.integers(1, 8)),
                                        cluster_id=int(rng.integers(1, 128)), term=5,
                                        log_index=int(rng.integers(0, 128)))
                             for _ in range(200)], deployment_id=1))
    aligns = [0, 5, 11] + [a for a in range(16) for _ in SIZES] + [7]
    data, spans, want = lay_out(hq, batches, aligns)
    assert len(want) == 3 + k + 200 and list(spans["count"][-4:]) == [64, 64, 64, 8]
    got, status = hq.decode_dev(gpu_ctx, data, spans, len(want))
    assert not status.any()
    assert got.tobytes() == want.tobytes()
    for f in ("cluster_id", "to", "log_term", "commit", "n_entries", "has_snapshot"):
        np.testing.assert_array_equal(got[f], want[f])
    for f in hq.EVENT_DTYPE.names:
        np.testing.assert_array_equal(got["ev"][f], want["ev"][f])


def test_decode_parity_unaligned_buffer(hq, gpu_ctx, parity_messages):
    """The byte buffer itself starting 0 .. 15 bytes past a 16-byte boundary."""
    data = we.batch(parity_messages[:65], deployment_id=3)
    spans, info = hq.frame_batch(data)
    want, _ = hq.decode_batch(data)
    dspans = gpu_ctx.upload(spans)
    for off in range(16):
        dev = gpu_ctx.upload(np.frombuffer(bytes(off) + data, np.uint8))
        assert dev.ptr % 16 == 0
        got, status = hq.decode_dev(gpu_ctx, dev.ptr + off, dspans, 65, data_len=len(data))
        gpu_ctx.free(dev)
        assert not status.any() and got.tobytes() == want[:65].tobytes(), off
    gpu_ctx.free(dspans)


def test_large_message_and_pinned_bytes(hq, gpu_ctx):
    """A message over the span budget (one lane, from memory) between staged spans, the bytes in
    pinned host memory read in place."""
    rng = np.random.default_rng(8)
    big = we.message(type=3, cluster_id=9, term=1 << 63,
                     entries=[we.entry(1, i, b"\x5a" * 3000) for i in range(3)], hint_high=5)
    small = [we.message(**random_fields(rng)) for _ in range(70)]
    data = we.batch(small[:33] + [big] + small[33:], deployment_id=1)
    spans, info = hq.frame_batch(data)
    assert [int(f) for f in spans["flags"]] == [0, 1, 0]
    want, _ = hq.decode_batch(data)
    pin = gpu_ctx.pinned(len(data) + 7, np.uint8)
    pin[7:] = np.frombuffer(data, np.uint8)
    spans["offset"] += 7
    got, status = hq.decode_dev(gpu_ctx, pin, spans, 71)
    assert hq.pointer_kind(pin) == hq.HQ_PTR_PINNED_HOST
    assert not status.any() and got.tobytes() == want[:71].tobytes()
    assert int(got["n_entries"][33]) == 3


def test_rejection_parity(hq, gpu_ctx):
    """Every proper prefix and a set of single-byte replacements of every fixture message, each
    in a `requests` framing of its own (so the batch is well framed by construction), in one
    launch: status[i] is whether the host decoder rejects slice i; equal records where it does
    not."""
    slices, owner, n_fixtures = wire_cases.rejection_slices()
    host = [host_decode_one(hq, s) for s in slices]
    rejected = np.array([r for r, _ in host])
    assert list(rejected) == [ref.rejected(s) for s in slices]
    for k in range(0, n_fixtures, 2):    # both outcomes for every fixture's message
        mine = rejected[np.array(owner) == k]
        assert mine.any() and not mine.all(), k
    data = b"".join(we.f_bytes(1, s) for s in slices)
    spans, info = hq.frame_batch(data)
    assert info.n_messages == len(slices)
    got, status = hq.decode_dev(gpu_ctx, data, spans, len(slices))
    np.testing.assert_array_equal(status, rejected.astype(np.uint8))
    ok = ~rejected
    want = np.array([m for _, m in host], hq.WIRE_MESSAGE_DTYPE)
    assert got[ok].tobytes() == want[ok].tobytes()


def test_spans_that_do_not_fit_the_bytes(hq, gpu_ctx):
    """Spans are checked against the bytes: a span whose headers are not where it says, or that
    does not lie within the buffer, gives status 1 for its messages and nothing else."""
    msgs = [we.message(type=13, frm=2, cluster_id=i + 1, term=4) for i in range(10)]
    data = we.batch(msgs)
    spans, _ = hq.frame_batch(data)
    want, _ = hq.decode_batch(data)
    assert len(spans) == 1
    bad = np.repeat(spans, 6)
    bad["first"] = np.arange(6) * 10
    bad["offset"][1] += 1                       # starts inside a header
    bad["len"][2] -= 1                          # ends inside the last message
    bad["offset"][3] = len(data) - 5            # runs past the buffer's end
    bad["offset"][4] = 1 << 62
    bad["count"][5] = 9                         # fewer messages than the bytes hold
    got, status = hq.decode_dev(gpu_ctx, data, bad, 59)
    assert not status[:10].any() and got[:10].tobytes() == want[:10].tobytes()
    assert status[10:].all()


# ---- the device mode end to end: MessageBatch bytes to a device step, against the oracle --------

CASES = list(sc.all_cases())
STATS = ("batches", "bytes", "messages", "entries", "snapshot_received", "dropped_batches",
         "dropped_messages", "dropped_no_cluster")


class _DeviceStep:
    """The backend's worker with `step` replaced by the wire's device step (WorkerBackend.step
    calls self.w.step(*arrs) for rows)."""

    def __init__(self, worker, backend):
        self._worker, self._backend = worker, backend

    def __getattr__(self, name):
        return getattr(self._worker, name)

    def step(self, *_):
        b = self._backend
        res, b.last_stats = b.wire.step_device()
        assert list(b.wire.device_rejected()) == [b.bad_index]
        # the host-attached wire, given the same calls, reports the same counters
        for k in STATS:
            assert getattr(b.last_stats, k) == getattr(b.shadow_stats, k), k
        return res


class DeviceWireBackend(WireBackend):
    """WireBackend in the device mode: attach_device / step_device. The parent's arrival stream
    (shuffled clusters, the queues merged at random, three batches, SnapshotReceived and foreign
    clusters mixed in, a foreign deployment's batch, a truncated batch), plus one well-framed batch
    per step that holds a message with a wrong wire type (nothing of it may reach a group) and
    one batch per step in pinned memory (read in place; the others are staged)."""

    def __init__(self, hq, n_max=8, seed=0, worker=None):
        super().__init__(hq, n_max, seed, worker, on_device=True, stream=False)
        self.wire.attach_device(self.w)
        self.shadow = hq.Wire(self.DEPLOYMENT)    # the host path, for the stats
        self.shadow.attach(self.w)
        self.w = _DeviceStep(self.w, self)
        self.pin_ctx = hq.Context(0)
        self.pin_buf = None
        self.in_place = self.staged = 0
        self.local_kinds = set()

    def close(self):
        self.shadow.close()
        self.wire.close()
        self.w._worker.close()
        self.pin_ctx.close()

    def _add(self, data, pinned=False, bad=False):
        """One add_batch on the device wire and on the shadow; returns the call's index."""
        hq = self.hq
        index = self.calls
        self.calls += 1
        if pinned:
            if self.pin_buf is None or len(self.pin_buf) < len(data) + 3:
                self.pin_buf = self.pin_ctx.pinned(2 * len(data) + 64, np.uint8)
            self.pin_buf[3:3 + len(data)] = np.frombuffer(data, np.uint8)
            assert hq.pointer_kind(self.pin_buf) == hq.HQ_PTR_PINNED_HOST
            self.wire.add_batch_at(self.pin_buf.ctypes.data + 3, len(data))
            self.in_place += 1
        else:
            self.wire.add_batch(data)
            self.staged += 1
        if bad:     # the host path rejects it at once
            with pytest.raises(hq.HQError):
                self.shadow.add_batch(data)
        else:
            self.shadow.add_batch(data)
        return index

    def build_inputs(self, per_group):
        hq, rng, wire = self.hq, self.rng, self.wire
        wire.reset()
        self.shadow.reset()
        self.calls = 0
        cids = list(per_group)
        rng.shuffle(cids)
        queues = {}
        for cid in cids:
            events = per_group[cid]
            check_phase_order(events)
            local = [event_record(hq, e) for e in events if e[0] != "msg"]
            self.local_kinds |= {e[0] for e in events if e[0] != "msg"}
            if local:
                wire.add_local(cid, np.array(local, hq.EVENT_DTYPE))
                self.shadow.add_local(cid, np.array(local, hq.EVENT_DTYPE))
            queues[cid] = [we.message(type=e[1], to=1, frm=e[2], cluster_id=cid, term=e[3],
                                      log_index=e[4], hint=e[5], hint_high=e[6],
                                      reject=bool(e[7]))
                           for e in events if e[0] == "msg"]
        stream, heads = [], {c: 0 for c in cids}
        live = [c for c in cids if queues[c]]
        while live:
            c = live[int(rng.integers(len(live)))]
            stream.append(queues[c][heads[c]])
            heads[c] += 1
            if heads[c] == len(queues[c]):
                live.remove(c)
            r = rng.random()
            if r < 0.02:
                stream.append(we.message(type=22, frm=2, cluster_id=c))
            elif r < 0.04:
                stream.append(we.message(type=13, frm=2, cluster_id=(1 << 62) + c, term=1,
                                         log_index=5))
        cut = sorted(set(int(x) for x in rng.integers(0, len(stream) + 1, 3)))
        parts = [stream[a:b] for a, b in zip([0] + cut, cut + [len(stream)])]
        longest = max(range(len(parts)), key=lambda i: len(parts[i]))
        for i, p in enumerate(parts):
            self._add(we.batch(p, deployment_id=self.DEPLOYMENT, source_address=b"n2:1"),
                      pinned=i == longest)
            if i == 0:
                self._add(we.batch(p, deployment_id=self.DEPLOYMENT + 1))
                # well framed, one message with a wrong wire type (field 1 as bytes) among
                # messages that would depose every leader they reached (a far higher term)
                poison = [we.message(type=sc.RREP, to=1, frm=2, cluster_id=c, term=1 << 40,
                                     log_index=1) for c in cids[:5]]
                bad = poison[:2] + [we.f_varint(2, 1) + we.f_bytes(1, b"\x00")] + poison[2:]
                self.bad_index = self._add(we.batch(bad, deployment_id=self.DEPLOYMENT), bad=True)
                if p:
                    b = we.batch(p, deployment_id=self.DEPLOYMENT, source_address=b"n2:1")
                    tail = len(we.batch([], deployment_id=self.DEPLOYMENT, source_address=b"n2:1"))
                    for w_ in (wire, self.shadow):
                        with pytest.raises(hq.HQError):
                            w_.add_batch(b[:len(b) - tail - 1])
                    self.calls += 1
        self.shadow_stats = self.shadow.step_sized(
            np.zeros(sum(len(v) for v in per_group.values()) * hq.HQ_EVENT_STREAM_MAX + 64, np.uint8),
            np.zeros(len(self.cids), np.uint16))[1]
        # the rows are in handle order (the order the groups were added in)
        refs, k = {}, 0
        for cid in self.cids:
            for pos in range(len(per_group.get(cid, ()))):
                refs[k] = (cid, pos)
                k += 1
        self.last_cids = list(self.cids)
        return (None, None, None), refs


@pytest.fixture(scope="module")
def device_wire_backend(hq):
    b = DeviceWireBackend(hq, n_max=8, seed=5)
    yield b
    assert b.in_place > 0 and b.staged > 0
    b.close()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reference_scenario_from_wire_bytes_on_device(device_wire_backend, case):
    """Every scenario adds its group to the one worker after the earlier scenarios' steps: the
    handle table is extended between steps, and the new group then receives messages."""
    outs, state = sc.run_case(device_wire_backend, case)
    sc.check_case(case, outs, state)
    want_outs, want_state = sc.run_case(OracleBackend(), case)
    assert state == want_state, case["name"]
    for w, o in zip(outs, want_outs):
        for k in ("committed", "commit_changed", "ready", "resps", "states", "dropped",
                  "deferred"):
            assert w[k] == o[k], (case["name"], k, w[k], o[k])


@pytest.mark.parametrize("seed,G,steps", [(11, 1500, 6), (12, 300, 15)])
def test_random_differential_from_wire_bytes_on_device(hq, seed, G, steps):
    rng = np.random.default_rng(seed)
    groups = sr.random_groups(rng, G)
    late = groups[-20:]                 # added between two steps; they then receive messages
    o, w = OracleBackend(), DeviceWireBackend(hq, n_max=8, seed=seed)
    try:
        for g in groups[:-20]:
            o.add_group(*g)
            w.add_group(*g)
        have = groups[:-20]
        ctx_seq = [0]
        dropped = late_messages = 0
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
            late_messages += sum(e[0] == "msg" for g in late for e in per.get(g[0], ()))
            want = o.step(per)
            got = w.step(per)
            st = w.last_stats
            assert st.dropped_batches == 1 and st.batches >= 2
            dropped += st.dropped_no_cluster + st.snapshot_received
            assert got["_fallback"] == []
            for cid in per:
                same_step(want, got, cid)
            for g in have:
                assert w.state(g[0]) == o.state(g[0]), (s, g[0])
        assert dropped > 0 and late_messages > 0
        assert w.local_kinds == {"read", "check_quorum", "campaign", "propose"}
        assert w.in_place == steps and w.staged >= 2 * steps
    finally:
        w.close()


def test_fallback_and_resync_on_device(hq):
    """A group goes through fallback (an observer acknowledging a pending ctx), stays suspended,
    and steps again after set_group: the device mode hands the rows over as the row path does."""
    w = hq.Worker(0, 8, on_device=True)
    mem = [(i, 9, sc.REMOTE, 0) for i in range(1, 6)] + [(6, 0, sc.OBSERVER, 0)]
    w.add_group(7, 1, 2, sc.LEADER, 9, 9, 9, mem)
    w.add_group(8, 1, 2, sc.LEADER, 9, 9, 9, mem)
    b = DeviceWireBackend(hq, worker=w)
    b.cids = [7, 8]
    try:
        out = b.step({7: [("read", 5, 6), sc.msg(sc.HBRESP, 2, 2, hint=5, high=6),
                          sc.msg(sc.HBRESP, 6, 2, hint=5, high=6), sc.msg(sc.RREP, 2, 2, 9),
                          ("propose", 1)]})
        assert out["_fallback"] == [7]
        assert out[7]["deferred"] == [2, 3, 4]
        g, m, r = w.get_group(7)
        assert g["suspended"] == 1 and len(r) == 1 and r[0]["n_confirmed"] == 1
        out = b.step({7: [("propose", 1)]})
        assert out[7]["deferred"] == [0]       # still suspended
        w.set_group(7, 1, 2, sc.LEADER, 9, 10, 9, [(1, 10, 0, 0), (2, 10, 0, 0), (3, 9, 0, 0),
                                                   (4, 9, 0, 0), (5, 9, 0, 0), (6, 0, 1, 0)])
        out = b.step({7: [sc.msg(sc.RREP, 3, 2, 10)], 8: [("propose", 2)]})
        assert out["_fallback"] == [] and out[7]["committed"] == 10
        assert w.get_group(8)[0]["last_index"] == 11
    finally:
        b.close()


def test_mode_errors(hq):
    host, dev = hq.Worker(0, 3), hq.Worker(0, 3, on_device=True)
    wire = hq.Wire(7)
    ev = np.array([(hq.EV_PROPOSE, 0, 0, 0, 1, 0, 0, 0, 0)], hq.EVENT_DTYPE)
    try:
        def code(f, *a):
            with pytest.raises(hq.HQError) as e:
                f(*a)
            return e.value.code

        assert code(wire.step_device) == hq.HQ_E_STATE             # not attached
        assert hq.lib.hq_wire_device_rejected(wire.h, None, None) == hq.HQ_E_INVAL
        assert code(wire.device_rejected) == hq.HQ_E_STATE
        assert code(wire.attach_device, host) == hq.HQ_E_INVAL     # not a device worker
        assert code(wire.attach_device, None) == hq.HQ_E_INVAL
        assert hq.lib.hq_wire_attach_device(None, dev.h) == hq.HQ_E_INVAL
        dev.add_group(1, 1, 1, sc.LEADER, 1, 1, 1, [(1, 1, 0, 0)])
        wire.attach_device(dev)
        res, st = wire.step_device()                               # nothing queued
        for k in ("commits", "ready", "read_resps", "state_changes", "dropped_reads", "deferred",
                  "fallback_groups"):
            assert len(res[k]) == 0, k
        assert all(getattr(st, k) == 0 for k in STATS)
        assert len(wire.device_rejected()) == 0
        assert code(wire.step_input, dev) == hq.HQ_E_STATE
        assert code(wire.step_stream, dev) == hq.HQ_E_STATE
        assert code(wire.step_sized, np.zeros(64, np.uint8), np.zeros(4, np.uint16)) == hq.HQ_E_STATE
        with pytest.raises(hq.HQError) as e:                       # a framing error: at once
            wire.add_batch(bytes.fromhex("0a05080d10"))
        assert e.value.code == hq.HQ_E_INVAL
        wire.add_local(1, ev)
        assert code(wire.attach_device, dev) == hq.HQ_E_STATE      # events queued
        assert code(wire.attach, dev) == hq.HQ_E_STATE
        res, st = wire.step_device()
        assert dev.get_group(1)[0]["last_index"] == 2 and st.batches == 0
        wire.reset()
        wire.add_batch(we.batch([we.message(type=sc.RREP, frm=1, cluster_id=1, term=1)],
                                deployment_id=7))
        assert code(wire.attach, dev) == hq.HQ_E_STATE             # a batch queued
        wire.reset()
        wire.attach(dev)                                           # back to the host mode
        assert code(wire.step_device) == hq.HQ_E_STATE
    finally:
        wire.close()
        host.close()
        dev.close()
