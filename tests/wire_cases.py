"""Test infrastructure: the Message encodings the wire decoders are held to the referee
(wire_decode_ref.py) on, shared by the host test (test_wire_codec.py) and the device test
(test_gpu_wire_dev.py): 4000 accepted messages in the marshalled and in a shuffled encoding, and
the prefixes and single-byte replacements of every fixture message."""
import functools
import json
import os

import numpy as np

import wire_encode as we

FIX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "wire_fixtures.json")))
EDGES = [0, 127, 128, (1 << 32) - 1, 1 << 63, (1 << 64) - 1]     # 1- to 10-byte varints


def random_fields(rng):
    v = lambda: EDGES[int(rng.integers(len(EDGES)))] if rng.random() < 0.5 else \
        int(rng.integers(0, 1 << int(rng.integers(1, 64))))
    return dict(type=int(rng.integers(0, 26)), to=v(), frm=v(), cluster_id=v(), term=v(),
                log_term=v(), log_index=v(), commit=v(), reject=bool(rng.random() < 0.5), hint=v(),
                hint_high=v())


def shuffled(rng, f):
    """The same message in another valid encoding: fields in a random order, unknown fields of
    every skippable wire type, an entry, a repeated scalar (the last one counts), the snapshot
    present or not."""
    parts = [we.f_varint(1, f["type"]), we.f_varint(2, f["to"]), we.f_varint(3, f["frm"]),
             we.f_varint(4, f["cluster_id"]), we.f_varint(5, f["term"]),
             we.f_varint(6, f["log_term"]), we.f_varint(7, f["log_index"]),
             we.f_varint(8, f["commit"]), we.f_varint(9, 1 if f["reject"] else 0),
             we.f_varint(10, f["hint"]), we.f_varint(13, f["hint_high"]),
             we.f_bytes(11, we.entry(3, 4, b"cmd")),
             we.f_varint(15, int(rng.integers(0, 1 << 62))), we.key(16, 1) + bytes(range(8)),
             we.key(17, 5) + b"\xaa\xbb\xcc\xdd", we.f_bytes(18, b"\x80" * int(rng.integers(0, 9))),
             we.f_varint((1 << 28) + 3, 7)]
    if rng.random() < 0.5:
        parts.append(we.f_bytes(12, we.snapshot()))
    order = rng.permutation(len(parts))
    body = b"".join(parts[i] for i in order)
    return we.f_varint(5, f["term"] ^ 1) + body        # term repeated: the later value stays


@functools.lru_cache(maxsize=None)
def parity_messages():
    """2000 random messages, each as Message.MarshalTo writes it and shuffled. (Shared: do not
    change the list.)"""
    rng = np.random.default_rng(41)
    out = []
    for _ in range(2000):
        f = random_fields(rng)
        out.append(we.message(**f))
        out.append(shuffled(rng, f))
    return out


@functools.lru_cache(maxsize=None)
def rejection_slices():
    """(slices, owner, n_fixtures): every proper prefix and a set of single-byte replacements of
    every fixture message (even owners) and of every fixture's bytes taken as one message (odd
    owners), then the malformed fixtures' messages (owner -1)."""
    slices, owner = [], []
    fixtures = []
    for fx in FIX["batches"]:
        raw = bytes.fromhex(fx["hex"])
        assert raw[0] == 0x0A and raw[1] < 0x80
        fixtures += [raw[2:2 + raw[1]], raw]   # the message, and the fixture's bytes taken as one
    for k, m in enumerate(fixtures):
        for n in range(len(m)):
            slices.append(m[:n])
            owner.append(k)
        for i, b in enumerate(m):
            for v in (0x00, 0x7F, 0x80, 0xFF, b ^ 1, b ^ 0x80):
                slices.append(m[:i] + bytes([v]) + m[i + 1:])
                owner.append(k)
    for fx in FIX["malformed"]:
        raw = bytes.fromhex(fx["hex"])
        slices.append(raw[2:2 + raw[1]] if raw[0] == 0x0A else raw)
        owner.append(-1)
    assert len(slices) > 1100
    return slices, owner, len(fixtures)
