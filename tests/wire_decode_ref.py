"""Test infrastructure: the referee of the raftpb.Message decode. A Python restatement, written
from raftpb/raft.proto:154-168 and the rules of accepted input that hq_wire_codec.h states (any
field order, a repeated scalar takes its last value, the tag's field number truncated to 32 bits,
unknown fields skipped by wire type, entries counted, the snapshot noted), in the way
test_wire_frame.py carries ref_walk for the batch. The host decoder (test_wire_codec.py) and the
device decoder (test_gpu_wire_dev.py) are both held to it: they are one source compiled twice, so
comparing them with each other proves nothing."""

M64 = (1 << 64) - 1

# field number -> name, for the varint fields of Message (raft.proto:154-168)
VARINT_FIELDS = {1: "type", 2: "to", 3: "from", 4: "cluster_id", 5: "term", 6: "log_term",
                 7: "log_index", 8: "commit", 9: "reject", 10: "hint", 13: "hint_high"}
ENTRIES, SNAPSHOT = 11, 12


class Rejected(Exception):
    pass


def read_varint(b, p):
    """(value mod 2^64, next position) of the varint at b[p:]: at most 10 bytes."""
    v = 0
    for k in range(10):
        if p + k >= len(b):
            raise Rejected("end of data in a varint")
        v |= (b[p + k] & 0x7F) << (7 * k)
        if b[p + k] < 0x80:
            return v & M64, p + k + 1
    raise Rejected("varint longer than 10 bytes")


def read_length(b, p):
    """(body start, body end) of a length-delimited field whose length is at b[p:]."""
    n, p = read_varint(b, p)
    if n > len(b) - p:
        raise Rejected("end of data in a length-delimited field")
    return p, p + n


def decode_message(b):
    """The fields of the Message encoded in b, as a dict with the names of hq_wire_message (the
    event's fields without a prefix), or raises Rejected."""
    m = dict.fromkeys(VARINT_FIELDS.values(), 0)
    m.update(n_entries=0, has_snapshot=0)
    p = 0
    while p < len(b):
        tag, p = read_varint(b, p)
        field, wt = (tag >> 3) & 0xFFFFFFFF, tag & 7
        if field == 0:
            raise Rejected("field number 0")
        if field in VARINT_FIELDS:
            if wt != 0:
                raise Rejected("wrong wire type of a scalar field")
            v, p = read_varint(b, p)
            name = VARINT_FIELDS[field]
            m[name] = v & 0xFFFFFFFF if name == "type" else int(v != 0) if name == "reject" else v
        elif field in (ENTRIES, SNAPSHOT):
            if wt != 2:
                raise Rejected("wrong wire type of a message field")
            _, p = read_length(b, p)
            if field == ENTRIES:
                m["n_entries"] += 1
            else:
                m["has_snapshot"] = 1
        elif wt == 0:
            _, p = read_varint(b, p)
        elif wt == 2:
            _, p = read_length(b, p)
        elif wt in (1, 5):
            n = 8 if wt == 1 else 4
            if n > len(b) - p:
                raise Rejected("end of data in a fixed-width field")
            p += n
        else:
            raise Rejected("group wire type")
    return m


def rejected(b):
    try:
        decode_message(b)
        return False
    except Rejected:
        return True


def as_record(hq, m):
    """A referee's dict as one hq.WIRE_MESSAGE_DTYPE record (what the decoders write)."""
    import numpy as np

    r = np.zeros(1, hq.WIRE_MESSAGE_DTYPE)
    ev = r["ev"]
    ev["kind"] = hq.EV_MESSAGE
    for name in ("type", "from", "term", "log_index", "hint", "hint_high", "reject"):
        ev[name] = m[name]
    for name in ("cluster_id", "to", "log_term", "commit", "n_entries", "has_snapshot"):
        r[name] = m[name]
    return r[0]
