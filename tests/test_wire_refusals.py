"""Every refusal the wire's C entries make (dragonboat_amd/csrc/hq_wire.cpp), written out: the
entry, the bad call, its code and the exact hq_wire_last_error text (UNCHANGED: the entry returns
its code without a message; the handle-less entries and a NULL wire have nowhere to keep one).
All of them are validations that return, and the order of an entry's refusals is part of the
table: where two apply, the row says which one answers. After each group of rows the same wire
takes a valid batch and steps. A worker, host or device, opens only with a GPU, so the rows that
need one carry the gpu mark: 8 leader groups of 3 members, a host worker and a device worker.
One refusal is not in the table: hq_wire_step_sized's "a queued record's handle is past the
worker's groups" cannot be reached through the entries (handles only grow)."""
import ctypes

import numpy as np
import pytest

import step_scenarios as sc

DEPLOYMENT = 7
G = 8
CIDS = list(range(101, 101 + G))
MEMBERS = [(1, 6, sc.REMOTE, 0), (2, 5, sc.REMOTE, 0), (3, 5, sc.REMOTE, 0)]
UNCHANGED = object()
MALFORMED = "hq_wire_add_batch: malformed MessageBatch"


def last_error(hq, w):
    return hq.lib.hq_wire_last_error(w).decode()


def run_table(hq, w, table):
    """Each row: (what, call, code, text); call() returns the entry's code."""
    for what, call, code, text in table:
        before = last_error(hq, w)
        rc = call()
        assert rc == code, (what, rc, last_error(hq, w))
        assert last_error(hq, w) == (before if text is UNCHANGED else text), what
    return len(table)


def acks(hq, cids, index=6):
    """One valid MessageBatch: node 2's ReplicateResp at `index` for every cluster of cids."""
    m = np.zeros(len(cids), hq.WIRE_MESSAGE_DTYPE)
    m["ev"]["kind"], m["ev"]["type"], m["ev"]["from"], m["ev"]["term"] = hq.EV_MESSAGE, sc.RREP, 2, 2
    m["ev"]["log_index"], m["cluster_id"], m["to"] = index, cids, 1
    return hq.encode_wire_batch(m, DEPLOYMENT)


def locals_of(hq, kind, n=1):
    ev = np.zeros(n, hq.EVENT_DTYPE)
    ev["kind"] = kind
    return ev


@pytest.fixture()
def wire(hq):
    w = hq.Wire(DEPLOYMENT)
    yield w
    w.close()


# ------------------------------------------------------------------ no worker needed ----------
def test_handle_less_entries(hq):
    lib, INVAL, STATE = hq.lib, hq.HQ_E_INVAL, hq.HQ_E_STATE
    n, ln = ctypes.c_uint64(0), ctypes.c_uint64(0)
    good = acks(hq, CIDS)
    out1 = np.zeros(1, hq.WIRE_MESSAGE_DTYPE)
    msg = np.zeros(1, hq.WIRE_MESSAGE_DTYPE)
    ent = msg.copy()
    ent["n_entries"] = 1
    buf, src = np.zeros(256, np.uint8), np.zeros(4, np.uint8)
    p = hq._p
    rows = [
        ("decode: NULL bytes with a length", lib.hq_wire_decode_batch(None, 5, None, 0, ctypes.byref(n), None), INVAL),
        ("decode: NULL count", lib.hq_wire_decode_batch(p(good), len(good), None, 0, None, None), INVAL),
        ("decode: malformed", lib.hq_wire_decode_batch(p(good), len(good) - 1, None, 0, ctypes.byref(n), None), INVAL),
        ("decode: more messages than cap", lib.hq_wire_decode_batch(p(good), len(good), p(out1), 1, ctypes.byref(n), None), STATE),
        ("encode: NULL msgs", lib.hq_wire_encode_batch(None, 1, 0, None, 0, p(buf), 256, ctypes.byref(ln)), INVAL),
        ("encode: NULL len", lib.hq_wire_encode_batch(p(msg), 1, 0, None, 0, p(buf), 256, None), INVAL),
        ("encode: NULL source with a length", lib.hq_wire_encode_batch(p(msg), 1, 0, None, 4, p(buf), 256, ctypes.byref(ln)), INVAL),
        ("encode: NULL out with a cap", lib.hq_wire_encode_batch(p(msg), 1, 0, None, 0, None, 256, ctypes.byref(ln)), INVAL),
        ("encode: entries", lib.hq_wire_encode_batch(p(ent), 1, 0, None, 0, p(buf), 256, ctypes.byref(ln)), INVAL),
        ("encode: no room for the message", lib.hq_wire_encode_batch(p(msg), 1, 0, None, 0, p(buf), 8, ctypes.byref(ln)), STATE),
        ("encode: no room for the trailer", lib.hq_wire_encode_batch(p(msg), 1, 0, p(src), 4, p(buf), 60, ctypes.byref(ln)), STATE),
        ("open: NULL out", lib.hq_wire_open(0, None), INVAL),
    ]
    for what, rc, code in rows:
        assert rc == code, what
    assert n.value == G                     # (the count is given with HQ_E_STATE)
    assert lib.hq_wire_last_error(None) == b""
    assert len(rows) == 12


def test_null_wire(hq):
    lib, z = hq.lib, ctypes.c_uint64(0)
    ev, inp, ss, so = locals_of(hq, hq.EV_PROPOSE), hq.StepInput(), hq.StepStream(), hq.StepOutput()
    four, ptr = np.zeros(4, np.uint64), ctypes.c_void_p()
    rows = [
        lib.hq_wire_attach(None, None), lib.hq_wire_attach_device(None, None), lib.hq_wire_reset(None),
        lib.hq_wire_add_local(None, 1, hq._p(ev), 1),
        lib.hq_wire_add_locals(None, 0, None, None, None), lib.hq_wire_add_batch(None, None, 0),
        lib.hq_wire_step_input(None, None, ctypes.byref(inp), None),
        lib.hq_wire_step_stream(None, None, ctypes.byref(ss), None),
        lib.hq_wire_step_sized(None, None, 0, None, 0, ctypes.byref(ss), None),
        lib.hq_wire_step_device(None, ctypes.byref(so), None),
        lib.hq_wire_set_device_framing(None, 1), lib.hq_wire_device_frame_stats(None, hq._p(four)),
        lib.hq_wire_device_rejected(None, ctypes.byref(ptr), ctypes.byref(z)),
    ]
    assert rows == [hq.HQ_E_INVAL] * 13


def test_refusals_without_a_worker(hq, wire):
    lib, w, p = hq.lib, wire.h, hq._p
    INVAL, STATE = hq.HQ_E_INVAL, hq.HQ_E_STATE
    good = acks(hq, CIDS)
    prop, msg = locals_of(hq, hq.EV_PROPOSE, 2), locals_of(hq, hq.EV_MESSAGE, 2)
    mixed = prop.copy()
    mixed["kind"][1] = 0
    c1, o01, o02, o20 = (np.array(x, np.uint64) for x in ([5], [0, 1], [0, 2], [2, 0]))
    c2, o021 = np.array([5, 6], np.uint64), np.array([0, 2, 1], np.uint64)
    inp, ss, so, st = hq.StepInput(), hq.StepStream(), hq.StepOutput(), hq.WireStats()
    four, ptr, z = np.zeros(4, np.uint64), ctypes.c_void_p(), ctypes.c_uint64(0)
    data, s16 = np.zeros(4096, np.uint8), np.zeros(G, np.uint16)
    bad_msg = bytes([0x0a, 0x02, 0x08, 0x80]) + bytes(good[-6:])   # a message's varint cut short
    bad = np.frombuffer(bad_msg, np.uint8)
    nd = ": no device worker attached"
    count = run_table(hq, w, [
        ("add_batch: NULL bytes", lambda: lib.hq_wire_add_batch(w, None, 5), INVAL,
         "hq_wire_add_batch: NULL bytes"),
        ("add_batch: a batch cut short", lambda: lib.hq_wire_add_batch(w, p(good), len(good) - 1), INVAL, MALFORMED),
        ("add_batch: a message's varint cut short", lambda: lib.hq_wire_add_batch(w, p(bad), len(bad)), INVAL,
         MALFORMED + ": Message: unexpected end of data in a varint"),
        ("add_local: NULL events", lambda: lib.hq_wire_add_local(w, 5, None, 2), INVAL, UNCHANGED),
        ("add_local: a message", lambda: lib.hq_wire_add_local(w, 5, p(msg), 2), INVAL,
         "hq_wire_add_local: kind must be a local event"),
        ("add_locals: NULL cluster ids", lambda: lib.hq_wire_add_locals(w, 1, None, p(o01), p(prop)), INVAL, UNCHANGED),
        ("add_locals: NULL offsets", lambda: lib.hq_wire_add_locals(w, 1, p(c1), None, p(prop)), INVAL, UNCHANGED),
        ("add_locals: NULL events", lambda: lib.hq_wire_add_locals(w, 1, p(c1), p(o02), None), INVAL, UNCHANGED),
        ("add_locals: offsets decrease", lambda: lib.hq_wire_add_locals(w, 1, p(c1), p(o20), p(prop)), INVAL,
         "hq_wire_add_locals: offsets decrease"),
        ("add_locals: offsets decrease inside (after the first cluster's kinds)",
         lambda: lib.hq_wire_add_locals(w, 2, p(c2), p(o021), p(prop)), INVAL, "hq_wire_add_locals: offsets decrease"),
        ("add_locals: a kind that is none (it speaks as add_local)",
         lambda: lib.hq_wire_add_locals(w, 1, p(c1), p(o02), p(mixed)), INVAL,
         "hq_wire_add_local: kind must be a local event"),
        ("attach_device: NULL worker", lambda: lib.hq_wire_attach_device(w, None), INVAL,
         "hq_wire_attach_device: NULL worker"),
        ("step_input: NULL worker", lambda: lib.hq_wire_step_input(w, None, ctypes.byref(inp), None), INVAL, UNCHANGED),
        ("step_stream: NULL out", lambda: lib.hq_wire_step_stream(w, None, None, None), INVAL, UNCHANGED),
        ("step_stream: NULL worker", lambda: lib.hq_wire_step_stream(w, None, ctypes.byref(ss), None), INVAL, UNCHANGED),
        ("step_sized: NULL out", lambda: lib.hq_wire_step_sized(w, p(data), 4096, p(s16), G, None, None), INVAL, UNCHANGED),
        ("step_sized: NULL bytes with a cap",
         lambda: lib.hq_wire_step_sized(w, None, 4096, p(s16), G, ctypes.byref(ss), None), INVAL, UNCHANGED),
        ("step_sized: no worker attached",
         lambda: lib.hq_wire_step_sized(w, p(data), 4096, p(s16), G, ctypes.byref(ss), ctypes.byref(st)), STATE,
         "hq_wire_step_sized: no worker attached"),
        ("step_device: NULL out", lambda: lib.hq_wire_step_device(w, None, None), INVAL, UNCHANGED),
        ("step_device: no device worker", lambda: lib.hq_wire_step_device(w, ctypes.byref(so), None), STATE,
         "hq_wire_step_device" + nd),
        ("set_device_framing: no device worker", lambda: lib.hq_wire_set_device_framing(w, 1), STATE,
         "hq_wire_set_device_framing" + nd),
        ("device_frame_stats: NULL out", lambda: lib.hq_wire_device_frame_stats(w, None), INVAL, UNCHANGED),
        ("device_frame_stats: no device worker", lambda: lib.hq_wire_device_frame_stats(w, p(four)), STATE,
         "hq_wire_device_frame_stats" + nd),
        ("device_rejected: NULL batches", lambda: lib.hq_wire_device_rejected(w, None, ctypes.byref(z)), INVAL, UNCHANGED),
        ("device_rejected: NULL n", lambda: lib.hq_wire_device_rejected(w, ctypes.byref(ptr), None), INVAL, UNCHANGED),
        ("device_rejected: no device worker",
         lambda: lib.hq_wire_device_rejected(w, ctypes.byref(ptr), ctypes.byref(z)), STATE,
         "hq_wire_device_rejected" + nd),
    ])
    # nothing was queued by a refused call; a valid batch and local event are, and then the
    # attaches refuse (a NULL worker still comes first)
    wire.add_batch(good.tobytes())
    wire.add_local(CIDS[0], prop[:1])
    count += run_table(hq, w, [
        ("attach: events queued", lambda: lib.hq_wire_attach(w, None), STATE,
         "hq_wire_attach: events queued (reset first)"),
        ("attach_device: NULL worker, events queued", lambda: lib.hq_wire_attach_device(w, None), INVAL,
         "hq_wire_attach_device: NULL worker"),
    ])
    wire.reset()
    wire.attach(None)
    assert count == 28


# ------------------------------------------------------------------ with workers --------------
@pytest.fixture(scope="module")
def workers(hq):
    dev, host = hq.Worker(0, 8, on_device=True), hq.Worker(0, 8)
    for wk in (dev, host):
        for c in CIDS:
            assert wk.add_group(c, 1, 2, sc.LEADER, 5, 6, 5, MEMBERS) == c - 101
    yield host, dev
    dev.close()
    host.close()


@pytest.mark.gpu
def test_refusals_with_a_host_worker(hq, wire, workers):
    lib, w, p = hq.lib, wire.h, hq._p
    INVAL, STATE = hq.HQ_E_INVAL, hq.HQ_E_STATE
    host, _ = workers
    good = acks(hq, CIDS)
    inp, ss, st = hq.StepInput(), hq.StepStream(), hq.WireStats()
    data, s16 = np.zeros(1 << 16, np.uint8), np.zeros(G, np.uint16)
    big = np.zeros(65536 * hq.HQ_EVENT_STREAM_MAX, np.uint8)

    def sized(d, cap, s, n):
        return lib.hq_wire_step_sized(w, p(d) if d is not None else None, cap, p(s) if s is not None else None, n,
                                      ctypes.byref(ss), ctypes.byref(st))

    count = run_table(hq, w, [
        ("attach_device: a host worker", lambda: lib.hq_wire_attach_device(w, host.h), INVAL,
         "hq_wire_attach_device: not a device worker (HQ_WORKER_ON_DEVICE)"),
    ])
    wire.attach(host)
    wire.add_batch(good.tobytes())
    count += run_table(hq, w, [
        ("attach: events queued", lambda: lib.hq_wire_attach(w, host.h), STATE,
         "hq_wire_attach: events queued (reset first)"),
        ("attach_device: events queued (before the worker is looked at)",
         lambda: lib.hq_wire_attach_device(w, host.h), STATE, "hq_wire_attach_device: events queued (reset first)"),
        ("step_input: attached", lambda: lib.hq_wire_step_input(w, host.h, ctypes.byref(inp), None), STATE,
         "hq_wire_step_input: attached (hq_wire_step_sized)"),
        ("step_stream: attached (it speaks as step_input)",
         lambda: lib.hq_wire_step_stream(w, host.h, ctypes.byref(ss), None), STATE,
         "hq_wire_step_input: attached (hq_wire_step_sized)"),
        ("step_sized: fewer words than groups", lambda: sized(data, len(data), s16, G - 1), INVAL,
         "hq_wire_step_sized: sizes16 holds fewer words than the worker's groups"),
        ("step_sized: NULL sizes16", lambda: sized(data, len(data), None, G), INVAL,
         "hq_wire_step_sized: sizes16 holds fewer words than the worker's groups"),
        ("step_sized: no room (HQ_EVENT_STREAM_MAX bytes are asked before each event)",
         lambda: sized(data, hq.HQ_EVENT_STREAM_MAX - 1, s16, G), STATE,
         "hq_wire_step_sized: the stream does not fit cap"),
        ("step_sized: no bytes at all", lambda: sized(None, 0, s16, G), STATE,
         "hq_wire_step_sized: the stream does not fit cap"),
    ])
    # the queue is as it was: the same step now succeeds
    s, stats = wire.step_sized(data, s16)
    assert s[2] == G and stats.messages == G and (s16 > 0).all()     # (s[2]: the stream's events)
    wire.reset()
    wire.add_locals([CIDS[3]], [0, 65536], locals_of(hq, hq.EV_PROPOSE, 65536))
    count += run_table(hq, w, [
        ("step_sized: a group of 2^16 events", lambda: sized(big, len(big), s16, G), INVAL,
         "hq_wire_step_sized: a group of 2^16 events or bytes"),
    ])
    wire.reset()
    wire.attach(None)
    assert count == 10


@pytest.mark.gpu
def test_refusals_in_the_device_mode(hq, wire, workers):
    lib, w, p = hq.lib, wire.h, hq._p
    INVAL, STATE = hq.HQ_E_INVAL, hq.HQ_E_STATE
    _, dev = workers
    good = acks(hq, CIDS)
    ss, st = hq.StepStream(), hq.WireStats()
    data, s16 = np.zeros(1 << 16, np.uint8), np.zeros(G, np.uint16)
    wire.attach_device(dev)
    count = run_table(hq, w, [
        ("add_batch: NULL bytes (before the device arm)", lambda: lib.hq_wire_add_batch(w, None, 5), INVAL,
         "hq_wire_add_batch: NULL bytes"),
        ("add_batch: a batch cut short", lambda: lib.hq_wire_add_batch(w, p(good), len(good) - 1), INVAL, MALFORMED),
        ("step_sized: device mode",
         lambda: lib.hq_wire_step_sized(w, p(data), len(data), p(s16), G, ctypes.byref(ss), ctypes.byref(st)), STATE,
         "hq_wire_step_sized: device mode (hq_wire_step_device)"),
    ])
    wire.add_batch(good.tobytes())
    count += run_table(hq, w, [
        ("set_device_framing: events queued", lambda: lib.hq_wire_set_device_framing(w, 1), STATE,
         "hq_wire_set_device_framing: events queued (reset first)"),
        ("attach: events queued on the device side", lambda: lib.hq_wire_attach(w, None), STATE,
         "hq_wire_attach: events queued (reset first)"),
        ("attach_device: events queued on the device side", lambda: lib.hq_wire_attach_device(w, dev.h), STATE,
         "hq_wire_attach_device: events queued (reset first)"),
    ])
    res, stats = wire.step_device()
    assert stats.messages == G and stats.batches == 1 and len(res["commits"]) <= G
    wire.reset()
    wire.attach(None)                            # back from the device mode
    count += run_table(hq, w, [
        ("step_device: back on the host", lambda: lib.hq_wire_step_device(w, ctypes.byref(hq.StepOutput()), None),
         STATE, "hq_wire_step_device: no device worker attached"),
    ])
    assert count == 7
