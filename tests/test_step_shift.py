"""tests/step_shift.py checked on the CPU before a GPU is involved: the oracle is equivariant under
every world's Shift (the guard on the helper itself: a mistake in it would yield out-of-contract
worlds that pass or fail for the wrong reason), and the host stream codec — the row encoder, the
sized form and the compact-record path — carries every shifted world's rows exactly, runs of
consecutive senders that end at or wrap past 2^64 - 1 included."""
import numpy as np
import pytest

import step_shift as ss
from step_harness import OracleBackend
from test_stream import RREP, HBRESP, carried

FIELDS = ("kind", "type", "from", "term", "log_index", "hint", "hint_high", "reject", "reserved")
WORLDS = ("small",) + ss.SHIFTED
M = ss.M


@pytest.fixture(scope="module", params=["random", "runs"])
def small_world(request):
    """The small world run plainly (no Shift anywhere): groups, steps = [(per, want, states)]."""
    kind = request.param
    G, steps, seed = ss.SIZES[kind]
    rng = np.random.default_rng(seed)
    groups = ss.small_groups(kind, rng, G)
    o = OracleBackend()
    for g in groups:
        o.add_group(*g)
    ctx_seq = [0]
    out = []
    for s in range(steps):
        per = ss.small_events(kind, rng, groups, o.state, s, ctx_seq)
        want = o.step(per)
        out.append((per, want, {g[0]: o.state(g[0]) for g in groups}))
    return kind, groups, out


@pytest.mark.parametrize("world", WORLDS)
def test_oracle_equivariance(small_world, world):
    """The oracle stepped on the shifted world gives exactly the shift of what it gives on the
    small world: every output list and every group's state() after every step; Shift.unstate
    inverts Shift.state; every output kind occurs (the runs world has no ReadIndex responses)."""
    kind, groups, steps = small_world
    ref = ss.reference(kind, world)
    assert len(ref.steps) == len(steps)
    for g, b in zip(groups, ref.groups):
        assert ref.shifts[g[0]].group(g) == b
        assert all(0 <= v <= M for v in b[:3] + b[4:7]), b
        assert all(0 <= i <= M and 0 <= m <= M for i, m, _, _ in b[7]), b
    assert len({b[0] for b in ref.groups}) == len(groups)
    for s, ((per, want, states), (bper, bwant, bstates)) in enumerate(zip(steps, ref.steps)):
        assert len(per) == len(bper)
        for g, b in zip(groups, ref.groups):
            sh, cid, big = ref.shifts[g[0]], g[0], b[0]
            assert (cid in per) == (big in bper)
            if cid in per:
                assert [sh.event(e) for e in per[cid]] == bper[big], (s, cid)
                got = {k: bwant[big][k] for k in sh.out(want[cid])}
                assert sh.out(want[cid]) == got, (s, cid)
            assert sh.state(states[cid]) == bstates[big], (s, cid)
            assert sh.unstate(bstates[big]) == states[cid], (s, cid)
    seen = dict(ready=0, resps=0, states=0, dropped=0, deferred=0, commit=0)
    for per, want, _ in steps:
        for cid in per:
            ss.count_seen(seen, want[cid])
    assert ref.seen == seen
    assert ref.n_events == sum(len(ev) for per, _, _ in steps for ev in per.values())
    need = [k for k in seen if kind == "random" or k != "resps"]
    assert all(seen[k] > 0 for k in need), seen
    if kind == "random":
        assert (ref.n_events, seen) == (ss.RANDOM_EVENTS, ss.RANDOM_SEEN)


def test_shifted_worlds_reach_their_boundaries():
    """What the worlds are chosen for: ids, indexes and ctxs on both sides of 2^16 / 2^31 / 2^32 /
    2^63, the top runs world's groups ending at node 2^64 - 1 with small senders past them."""
    for world, lim_id, lim_idx in (("u16", 2**16, 2**31), ("u32", 2**32, 2**32),
                                   ("u63", 2**63, 2**63)):
        for kind in ("random", "runs"):
            ref = ss.reference(kind, world)
            frm = [e[2] for per, _, _ in ref.steps for ev in per.values() for e in ev
                   if e[0] == "msg"]
            idx = [e[4] for per, _, _ in ref.steps for ev in per.values() for e in ev
                   if e[0] == "msg" and e[4]]
            assert min(frm) < lim_id <= max(frm), (world, kind)
            assert min(idx) < lim_idx <= max(idx), (world, kind)
    top = ss.reference("runs", "top")
    assert all(max(i for i, _, _, _ in g[7]) == M for g in top.groups)
    frm = {e[2] for per, _, _ in top.steps for ev in per.values() for e in ev if e[0] == "msg"}
    assert M in frm and min(frm) < 16


def _same_rows(back, want, what):
    for k in FIELDS:
        np.testing.assert_array_equal(back[k], want[k], err_msg=f"{what} {k}")


def _round_trips(hq, off, ev, what):
    """Rows through the three host encoders and back; returns (bytes, boffsets, which rows took
    an escape in the compact records)."""
    want = carried(hq, ev)
    data, boff = hq.encode_events(off, ev)
    _same_rows(hq.decode_events(off, boff, data), want, f"{what} rows")
    sdata, sizes = hq.encode_events_sized(off, ev)
    np.testing.assert_array_equal(sizes & 0xFFFF, np.diff(off), err_msg=what)
    sboff = np.concatenate([[0], np.cumsum(sizes >> 16)]).astype(np.uint64)
    _same_rows(hq.decode_events(off, sboff, sdata), want, f"{what} sized")
    recs, off16 = hq.events_to16(off, ev)
    cdata, csizes, ne = hq.encode_events16_sized(off16, recs)
    assert ne == len(ev), what
    np.testing.assert_array_equal(csizes & 0xFFFF, np.diff(off), err_msg=what)
    cboff = np.concatenate([[0], np.cumsum(csizes >> 16)]).astype(np.uint64)
    _same_rows(hq.decode_events(off, cboff, cdata), want, f"{what} compact records")
    return data, boff, ss.escaped_rows(hq, recs, off16, off)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("kind", ["random", "runs"])
def test_codec_round_trip_on_shifted_rows(hq, kind, world):
    """Each step's rows of each world through hq_events_encode, hq_events_encode_sized and
    hq_events_to16 -> hq_events16_encode_sized, decoded by hq_events_decode: every carried field
    exact.

    hq_event16's escapes: at small values a row escapes only for a ctx with a high word that is
    not the group's latest READ (a forwarded ReadIndex's ctx, an ack of an older pending ctx) —
    the small worlds do have those, so "no escape" cannot be asked of them; no small row escapes
    for its sender, term or index. The u16 world escapes every message from a sender >= 2^16 and
    more rows than the small world does. The runs world's streams hold consecutive-form headers
    (counted by walking the events) wherever senders stay below 2^32; how many is printed."""
    ref, small = ss.reference(kind, world), ss.reference(kind, "small")
    escaped = small_escaped = wide_senders = seq_headers = 0
    for s, ((per, _, _), (sper, _, _)) in enumerate(zip(ref.steps, small.steps)):
        off, ev = ss.rows(hq, per)
        data, boff, esc = _round_trips(hq, off, ev, f"{kind} {world} step {s}")
        escaped += int(esc.sum())
        seq_headers += ss.run_headers(data, boff)[0]
        soff, sev = ss.rows(hq, sper)
        sesc = ss.escaped_rows(hq, *hq.events_to16(soff, sev), soff)
        small_escaped += int(sesc.sum())
        if world == "small":
            ctx_msg = (ev["kind"] == hq.EV_MESSAGE) & np.isin(ev["type"], [HBRESP, 19]) & \
                (ev["hint_high"] != 0)
            assert not (esc & ~ctx_msg).any()
        if world == "u16":
            wide = (ev["kind"] == hq.EV_MESSAGE) & (ev["from"] >= 2**16)
            wide_senders += int(wide.sum())
            assert esc[wide].all() and esc[sesc].all()
    print(f"{kind} {world}: {escaped} escaped rows (small world {small_escaped}), "
          f"{seq_headers} consecutive-form run headers")
    if world == "u16":
        assert wide_senders > 0 and escaped > small_escaped
    if kind == "runs" and world in ("small", "u16"):
        assert seq_headers > 100, seq_headers


def _run_rows(hq, typ, senders):
    """A previous message (sender 1) followed by its repeats from `senders`."""
    idx, hint = (1000, 0) if typ == RREP else (0, 0)
    rows = [(hq.EV_MESSAGE, typ, f, 41, idx, hint, 0, 0, 0) for f in [1] + list(senders)]
    return np.array([0, len(rows)], np.uint64), np.array(rows, hq.EVENT_DTYPE)


RUN_ENDS = (2**16 - 1, 2**16, 2**32 - 2, 2**32 - 1, 2**32, 2**63, 2**64 - 2, 2**64 - 1)
RUN_CASES = [(f"end-{end:#x}-m{m}", [end - m + 1 + j for j in range(m)])
             for end in RUN_ENDS for m in range(3, 7)]
RUN_CASES += [("wrap-4", [M - 1, M, 0, 1]), ("wrap-3", [M, 0, 1])]


@pytest.mark.parametrize("typ", [RREP, HBRESP], ids=["replicate", "heartbeat"])
@pytest.mark.parametrize("name,senders", RUN_CASES, ids=[c[0] for c in RUN_CASES])
def test_directed_runs(hq, typ, name, senders):
    """A message and m = 3..6 repeats from consecutive senders ending at each width boundary, and
    sender lists that wrap past 2^64 - 1: the round trip is exact through the row encoder and the
    compact-record encoder, which write the same bytes, and the consecutive form (header bit 7)
    is used exactly when the last sender is <= 2^32 - 2 (s0 + m <= 0xFFFFFFFF without wrap)."""
    off, ev = _run_rows(hq, typ, senders)
    data, boff, _ = _round_trips(hq, off, ev, name)
    recs, off16 = hq.events_to16(off, ev)
    cdata, _, _ = hq.encode_events16_sized(off16, recs)
    np.testing.assert_array_equal(cdata, data)
    first = len(hq.encode_events(np.array([0, 1], np.uint64), ev[:1])[0])
    seq = senders == list(range(senders[0], senders[0] + len(senders))) and \
        senders[-1] <= 2**32 - 2
    assert data[first] == (ss.RUN_HEADER | (0x80 if seq else 0)) and data[first + 1] == len(senders)
    assert ss.run_headers(data, boff) == ((1, 0) if seq else (0, 1))
    if seq:
        assert len(data) == first + 2 + len(ss.varint(senders[0]))


def test_wrapped_run_header_is_malformed(hq):
    """The hand-made consecutive-form header whose first sender + count wraps to 0 in 64 bits
    (step_shift.wrapped_run_stream): hq_events_decode rejects it; it must not return senders cut
    to 32 bits. The same header one sender lower (last sender 2^64 - 2, no wrap) is rejected by
    the 2^32 bound, and with a first sender of 2^32 - 5 it decodes."""
    off = np.array([0, 4], np.uint64)
    data = ss.wrapped_run_stream()
    with pytest.raises(hq.HQError):
        hq.decode_events(off, np.array([0, len(data)], np.uint64), data)
    head = bytes(data[:6])
    for f0, ok in ((2**64 - 4, False), (2**32 - 3, False), (2**32 - 4, True)):
        d = np.frombuffer(head + ss.varint(f0), np.uint8)
        boff = np.array([0, len(d)], np.uint64)
        if ok:
            back = hq.decode_events(off, boff, d)
            assert [int(x) for x in back["from"]] == [2, f0, f0 + 1, f0 + 2]
        else:
            with pytest.raises(hq.HQError):
                hq.decode_events(off, boff, d)
