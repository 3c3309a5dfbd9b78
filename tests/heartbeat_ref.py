"""The leader heartbeat broadcast restated in Python (raft.go:812-848, readindex.go:69-75), for the
heartbeat tests: the messages a group sends on a LeaderHeartbeat from its state as the worker
reports it (Worker.get_group, which never touches the heartbeat kernels), and the compact output
(include/hipquorum.h "leader heartbeat broadcast") those messages correspond to."""
import json
import os

import numpy as np

REMOTE, OBSERVER, WITNESS = 0, 1, 2
LEADER = 2
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heartbeat_kats.json")


def kats():
    return json.load(open(KATS))["cases"]


def broadcast(node_id, state, suspended, committed, members, reads):
    """broadcastHeartbeatMessage for one group. members: (node_id, match, role) in the caller's
    list order; reads: the pending ctxs (low, high), oldest first. Returns [(member index, to,
    commit, hint, hint_high)] in member order; nothing for a group that is not a leader or is
    suspended (its events go to the CPU raft)."""
    if state != LEADER or suspended:
        return []
    low, high = reads[-1] if reads else (0, 0)          # hasPendingRequest / peepCtx
    out = []
    for i, (nid, match, role) in enumerate(members):
        voting = role in (REMOTE, WITNESS)               # votingMembers: remotes and witnesses
        if nid == node_id and voting:
            continue
        if voting or (low, high) == (0, 0):              # observers only with the zero ctx
            out.append((i, nid, min(match, committed), low, high))   # sendHeartbeatMessage
    return out


def worker_group(w, cid):
    """(node_id, state, suspended, committed, members, reads, term) of one group of a worker."""
    g, m, r = w.get_group(cid)
    members = [(int(x["node_id"]), int(x["match"]), int(x["role"])) for x in m]
    reads = [(int(x["ctx_low"]), int(x["ctx_high"])) for x in r]
    return (int(g["node_id"]), int(g["state"]), int(g["suspended"]), int(g["committed"]), members,
            reads, int(g["term"]))


def compact(hq, listed):
    """The compact output of `listed` groups, each (node_id, state, suspended, committed, members,
    reads, ...): a dict as Worker.heartbeats returns it (without gpu_ns), and the messages
    (HEARTBEAT_MSG_DTYPE, cluster_id and term left 0) in group order, then member order."""
    words = np.zeros(len(listed), np.uint32)
    lags, ctxs, msgs = [], [], []
    for pos, g in enumerate(listed):
        node_id, state, suspended, committed, members, reads = g[:6]
        sent = broadcast(node_id, state, suspended, committed, members, reads)
        for i, to, commit, low, high in sent:
            words[pos] |= np.uint32(1 << i)
            if members[i][1] < committed:                # behind: Commit is the member's match
                words[pos] |= np.uint32(1 << (16 + i))
                lags.append((pos, i, members[i][1]))
            msgs.append((0, to, 0, commit, low, high))
        if sent and (sent[0][3], sent[0][4]) != (0, 0):
            ctxs.append((sent[0][3], sent[0][4], pos, 0))
    return ({"words": words, "lags": np.array(lags, hq.HEARTBEAT_LAG_DTYPE),
             "ctxs": np.array(ctxs, hq.HEARTBEAT_CTX_DTYPE), "n_messages": len(msgs)},
            np.array(msgs, hq.HEARTBEAT_MSG_DTYPE))


def columns(listed, cluster_ids):
    """hq_heartbeats_expand's per-group columns for `listed` (as compact takes them, with the term
    as the 7th field) and their cluster ids."""
    G = len(listed)
    ids = np.zeros((G, 16), np.uint64)
    for pos, g in enumerate(listed):
        for i, m in enumerate(g[4]):
            ids[pos, i] = m[0]
    return (np.array(cluster_ids, np.uint64), np.array([g[6] for g in listed], np.uint64),
            np.array([g[3] for g in listed], np.uint64),
            np.array([len(g[4]) for g in listed], np.uint32), ids)


def assert_same(got, want):
    """A heartbeat output against the compact output wanted, field for field."""
    np.testing.assert_array_equal(got["words"], want["words"])
    assert got["n_messages"] == want["n_messages"]
    for k in ("lags", "ctxs"):
        assert len(got[k]) == len(want[k]), k
        for f in want[k].dtype.names:
            if f != "reserved":
                np.testing.assert_array_equal(got[k][f], want[k][f], err_msg=f"{k}.{f}")
