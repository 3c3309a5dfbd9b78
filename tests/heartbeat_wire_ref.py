"""Expected values for hq_worker_heartbeat_batches, independent of the code under test: the
messages are tests/heartbeat_ref.py's broadcast over Worker.get_group, the routes are looked up
here, and every batch is marshalled by tests/wire_encode.py. check() compares a call's output with
them field for field and byte for byte, and feeds every batch to hq_wire_decode_batch."""
import numpy as np

import heartbeat_ref as ref
import wire_encode as we

NONE = 0xFFFF
HEARTBEAT = 17


class World:
    """The groups of a worker as get_group reports them, read once per state, and their
    marshalled messages (which do not depend on the routing)."""

    def __init__(self, w, cids):
        self.w, self.cids = w, list(cids)          # cids[handle]
        self.groups, self.sent = {}, {}

    def messages(self, h):
        """[(member index, message fields, marshalled message)] of handle h."""
        if h not in self.sent:
            cid = self.cids[h]
            node_id, state, susp, committed, members, reads, term = ref.worker_group(self.w, cid)
            out = []
            for i, to, commit, low, high in ref.broadcast(node_id, state, susp, committed, members,
                                                          reads):
                f = dict(type=HEARTBEAT, to=to, frm=node_id, cluster_id=cid, term=term,
                         commit=commit, hint=low, hint_high=high)
                out.append((i, f, we.message(**f)))
            self.sent[h] = out
        return self.sent[h]


def expected(world, handles, routes, n_dest, batch_messages, deployment_id, source):
    """[(dest, [message fields], batch bytes)] by destination, then in sequence, and the unrouted
    count. routes: (groups, 16) by handle."""
    per_dest, unrouted = {}, 0
    for h in handles:
        for i, f, b in world.messages(int(h)):
            r = int(routes[int(h)][i])
            if r == NONE:
                unrouted += 1
                continue
            assert r < n_dest
            per_dest.setdefault(r, []).append((f, b))
    batches = []
    for d in sorted(per_dest):
        msgs = per_dest[d]
        cut = batch_messages or len(msgs)
        for k in range(0, len(msgs), cut):
            chunk = msgs[k:k + cut]
            batches.append((d, [f for f, _ in chunk],
                            we.batch([b for _, b in chunk], deployment_id, source)))
    return batches, unrouted


def check(hq, got, want, unrouted, deployment_id, source, decode=True):
    batches = got["batches"]
    assert len(batches) == len(want)
    assert got["n_unrouted"] == unrouted
    assert got["n_messages"] == sum(len(m) for _, m, _ in want)
    assert len(got["bytes"]) == sum(len(b) for _, _, b in want)
    data = got["bytes"].tobytes()
    at = 0
    for t, (dest, msgs, b) in zip(batches, want):
        assert (int(t["dest"]), int(t["n_messages"]), int(t["len"]), int(t["offset"])) == \
            (dest, len(msgs), len(b), at)
        piece = data[at:at + len(b)]
        assert piece == b, (dest, at)
        at += len(b)
        if decode:
            m, info = hq.decode_batch(piece)
            assert (info.deployment_id, info.source_address_len, info.bin_ver) == \
                (deployment_id, len(source), 210)
            assert len(m) == len(msgs)
            for x, f in zip(m, msgs):
                assert (int(x["ev"]["type"]), int(x["to"]), int(x["ev"]["from"]),
                        int(x["cluster_id"]), int(x["ev"]["term"]), int(x["log_term"]),
                        int(x["ev"]["log_index"]), int(x["commit"]), int(x["ev"]["reject"]),
                        int(x["ev"]["hint"]), int(x["ev"]["hint_high"]), int(x["n_entries"])) == \
                    (HEARTBEAT, f["to"], f["frm"], f["cluster_id"], f["term"], 0, 0, f["commit"], 0,
                     f["hint"], f["hint_high"], 0)


def run_and_check(hq, world, handles, routes, n_dest, batch_messages=0, deployment_id=7,
                  source=b"host-a:1", decode=True):
    """One call over `handles` (None: every handle) against the expected values; returns the
    call's output and the expected batches."""
    hs = range(len(world.cids)) if handles is None else handles
    want, unrouted = expected(world, hs, routes, n_dest, batch_messages, deployment_id, source)
    got = world.w.heartbeat_batches(handles, deployment_id, source, n_dest, batch_messages)
    check(hq, got, want, unrouted, deployment_id, source, decode)
    return got, want


def random_routes(rng, G, n_dest, none=0.05):
    """(G, 16) routes below n_dest, a share of them HQ_ROUTE_NONE; with more than one destination,
    one of them (n_dest // 2) gets nothing."""
    r = rng.integers(0, n_dest, (G, 16)).astype(np.uint16)
    if n_dest > 1:
        r[r == n_dest // 2] = (n_dest // 2 + 1) % n_dest
    r[rng.random((G, 16)) < none] = NONE
    return r
