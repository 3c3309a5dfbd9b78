"""hq_heartbeats_expand (host only, stateless): compact heartbeat outputs built by hand reproduce the
reference's own tables (tests/golden/heartbeat_kats.json), the messages survive the wire
(hq_wire_encode_batch -> hq_wire_decode_batch), and inconsistent inputs are refused."""
import numpy as np
import pytest

import heartbeat_ref as ref

KATS = ref.kats()


def kat_group(case):
    """A KAT as heartbeat_ref.compact's group tuple: the leader's state with `ctx` pending."""
    g = case["group"]
    members = [tuple(m) for m in g["members"]]
    reads = [tuple(case["ctx"])] if tuple(case["ctx"]) != (0, 0) else []
    return (g["node_id"], ref.LEADER, 0, g["committed"], members, reads, g["term"])


def hand_built(hq, case):
    """The compact output of one KAT written out bit by bit (no helper in between)."""
    g = case["group"]
    word, lags = 0, []
    for i, (nid, match, role) in enumerate(g["members"]):
        if nid == g["node_id"]:
            continue
        word |= 1 << i
        if match < g["committed"]:
            word |= 1 << (16 + i)
            lags.append((0, i, match))
    low, high = case["ctx"]
    ctxs = [(low, high, 0, 0)] if (low, high) != (0, 0) else []
    return {"words": np.array([word], np.uint32), "lags": np.array(lags, hq.HEARTBEAT_LAG_DTYPE),
            "ctxs": np.array(ctxs, hq.HEARTBEAT_CTX_DTYPE), "n_messages": len(g["members"]) - 1}


def as_tuples(msgs):
    return [tuple(int(m[f]) for f in ("cluster_id", "to", "term", "commit", "hint", "hint_high"))
            for m in msgs]


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_expand_reproduces_the_reference_tables(hq, case):
    g = kat_group(case)
    hb = hand_built(hq, case)
    ref.assert_same(hb, ref.compact(hq, [g])[0])         # the restatement agrees with the table
    msgs = hq.heartbeats_expand(hb, *ref.columns([g], [case["group"]["cluster_id"]]))
    want = [(case["group"]["cluster_id"], w["to"], case["group"]["term"], w["commit"], w["hint"],
             w["hint_high"]) for w in case["want"]]
    assert as_tuples(msgs) == want


def test_expand_all_tables_in_one_output(hq):
    """Several groups in one output, followers and an empty word between them: group order, then
    member order, lags and ctxs consumed in step."""
    groups = [kat_group(c) for c in KATS]
    follower = (1, 0, 0, 50, [(1, 50, 0), (2, 0, 0)], [], 3)
    listed = [groups[0], follower, groups[1], groups[3], follower, groups[2]]
    cids = [11, 12, 13, 14, 15, 16]
    hb, want = ref.compact(hq, listed)
    assert list(hb["words"] == 0) == [False, True, False, False, True, False]
    msgs = hq.heartbeats_expand(hb, *ref.columns(listed, cids))
    assert len(msgs) == hb["n_messages"] == 7
    for f in ("to", "commit", "hint", "hint_high"):
        np.testing.assert_array_equal(msgs[f], want[f])
    assert list(msgs["cluster_id"]) == [11, 11, 13, 14, 14, 16, 16]
    assert list(msgs["term"]) == [2, 2, 1, 1, 1, 1, 1]


def test_values_are_full_u64(hq):
    big = (1 << 63) + 12345
    g = (7, ref.LEADER, 0, big, [(7, big + 5, 0), (1 << 62, big - 1, 0), ((1 << 64) - 1, big, 2)],
         [((1 << 64) - 2, (1 << 33) + 1)], (1 << 40) + 3)
    hb, _ = ref.compact(hq, [g])
    msgs = hq.heartbeats_expand(hb, *ref.columns([g], [(1 << 64) - 9]))
    assert as_tuples(msgs) == [
        ((1 << 64) - 9, 1 << 62, (1 << 40) + 3, big - 1, (1 << 64) - 2, (1 << 33) + 1),
        ((1 << 64) - 9, (1 << 64) - 1, (1 << 40) + 3, big, (1 << 64) - 2, (1 << 33) + 1)]


def test_messages_survive_the_wire(hq):
    """expand -> hq_wire_message rows of type Heartbeat -> hq_wire_encode_batch ->
    hq_wire_decode_batch: to, term, commit, hint and hint_high come back."""
    listed = [kat_group(c) for c in KATS]
    cids = [c["group"]["cluster_id"] for c in KATS]
    hb, _ = ref.compact(hq, listed)
    msgs = hq.heartbeats_expand(hb, *ref.columns(listed, cids))
    rows = hq.heartbeat_wire_messages(msgs, 1)
    data = hq.encode_wire_batch(rows, deployment_id=77, source_address=b"n1:9")
    back, info = hq.decode_batch(data.tobytes())
    assert info.n_messages == len(msgs) == 7 and info.deployment_id == 77
    assert all(int(t) == hq.HQ_MSG_HEARTBEAT == 17 for t in back["ev"]["type"])
    np.testing.assert_array_equal(back["ev"]["from"], np.ones(len(msgs), np.uint64))
    for wire, field in (("to", "to"), ("commit", "commit"), ("cluster_id", "cluster_id")):
        np.testing.assert_array_equal(back[wire], msgs[field])
    for f in ("term", "hint", "hint_high"):
        np.testing.assert_array_equal(back["ev"][f], msgs[f])


def _valid(hq):
    """Two leaders: one with a lagging member and a hint, one without either."""
    listed = [(1, ref.LEADER, 0, 10, [(1, 12, 0), (2, 7, 0), (3, 10, 2), (4, 2, 1)], [(5, 6)], 4),
              (1, ref.LEADER, 0, 10, [(2, 3, 0), (1, 12, 0), (4, 12, 1)], [], 4)]
    hb, _ = ref.compact(hq, listed)
    # group 0: to {1, 2}, member 1 behind, ctx (5, 6); group 1: to {0, 2}, member 0 behind
    assert list(hb["words"]) == [0x00020006, 0x00010005] and hb["n_messages"] == 4
    assert len(hb["lags"]) == 2 and len(hb["ctxs"]) == 1
    return hb, ref.columns(listed, [21, 22])


def _expect(hq, code, hb, cols, **kw):
    with pytest.raises(hq.HQError) as e:
        hq.heartbeats_expand(hb, *cols, **kw)
    assert f"error {code}:" in str(e.value), e.value
    return e.value


def test_inconsistent_inputs_are_invalid(hq):
    hb, cols = _valid(hq)
    assert len(hq.heartbeats_expand(hb, *cols)) == 4

    def broken(**change):
        b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in hb.items()}
        for k, f in change.items():
            b[k] = f(b[k])
        return b

    def setw(i, w):
        def f(words):
            words[i] = w
            return words
        return f

    def setf(i, field, v):
        def f(recs):
            recs[field][i] = v
            return recs
        return f

    bad = {
        "a behind bit outside the to mask": broken(words=setw(1, 0x00030005)),
        "a to bit at or beyond n_members": broken(words=setw(1, 0x0001000D), n_messages=lambda n: 5),
        "lags out of order (groups swapped)": broken(lags=lambda l: l[::-1].copy()),
        "lags out of order (members)": broken(words=setw(0, 0x00060006),
                                              lags=lambda l: np.array(
                                                  [(0, 2, 1), (0, 1, 7), (1, 0, 3)], l.dtype)),
        "a lag whose bit is not set": broken(lags=setf(0, "member", 2)),
        "a lag of a position outside the list": broken(lags=setf(1, "pos", 2)),
        "a lag too many": broken(lags=lambda l: np.concatenate([l, l[-1:]])),
        "a lag missing": broken(lags=lambda l: l[:1].copy()),
        "n_messages not the words' count": broken(n_messages=lambda n: 3),
        "ctxs out of order": broken(ctxs=lambda c: np.array([(5, 6, 1, 0), (7, 8, 0, 0)], c.dtype)),
        "a ctx of a position outside the list": broken(ctxs=setf(0, "pos", 9)),
        "a zero ctx": broken(ctxs=lambda c: np.array([(0, 0, 0, 0)], c.dtype)),
        "a ctx of a group with nothing to send": broken(
            words=setw(0, 0), lags=lambda l: l[1:].copy(), n_messages=lambda n: 2),
    }
    for what, b in bad.items():
        try:
            _expect(hq, hq.HQ_E_INVAL, b, cols)
        except BaseException as e:
            raise AssertionError(what) from e
    # more than 16 members in a group
    c = list(cols)
    c[3] = np.array([17, 3], np.uint32)
    _expect(hq, hq.HQ_E_INVAL, hb, c)


def test_short_cap_is_state_with_the_count(hq):
    hb, cols = _valid(hq)
    for cap in (0, 1, 3):
        e = _expect(hq, hq.HQ_E_STATE, hb, cols, cap=cap)
        assert e.n == 4
    assert len(hq.heartbeats_expand(hb, *cols, cap=4)) == 4
    assert len(hq.heartbeats_expand(hb, *cols, cap=9)) == 4


def test_empty_output(hq):
    hb, _ = ref.compact(hq, [])
    assert len(hq.heartbeats_expand(hb, *ref.columns([], []))) == 0
