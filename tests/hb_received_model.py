"""The expected values of the received-heartbeat tests (hq_worker_heartbeats_received,
hq_heartbeat_replies_expand): a direct Python restatement of include/hipquorum.h "heartbeats
received" from the reference's lines (raft.go:1416-1452 onMessageTermNotMatched, :1869-1873
handleFollowerHeartbeat, :1963-1966 handleCandidateHeartbeat, :1302-1310 handleHeartbeatMessage,
:1859-1861 leaderIsAvailable, :949-957 becomeFollower, :991-1010 reset). It shares no code with the
library's hq_hb_received.h.

A group is a dict with term, state, committed, last, suspended; a message a tuple
(from, term, commit, hint, hint_high)."""
FOLLOWER, CANDIDATE, LEADER = 0, 1, 2
MSG_NOOP, MSG_HEARTBEAT, MSG_HEARTBEAT_RESP = 4, 17, 18
COMMITTED, COMMIT_ABOVE_LAST, CONTACT, SUSPENDED = 1, 2, 4, 8
EV_MESSAGE = 2


def handle(group, msgs, check_quorum):
    """What the reference does with `msgs`, in order, in `group`'s state. Returns (replies, result,
    after): replies one (type, term) per message; result a dict of hq_hb_group_result's fields;
    after the group's dict after the call, with 'reset' (becomeFollower ran: votes, pending reads,
    matches and active flags are cleared as raft.reset does)."""
    g = dict(group, reset=False)
    res = {"commit": 0, "leader": 0, "flags": 0, "n_resets": 0}
    if g["suspended"]:
        res.update(term=g["term"], state=g["state"], flags=SUSPENDED)
        return [(0, 0)] * len(msgs), res, g

    def become_follower(term):
        g.update(state=FOLLOWER, term=term, reset=True)
        res["n_resets"] += 1

    replies = []
    for frm, term, commit, _hint, _high in msgs:
        if term != 0 and term > g["term"]:                        # raft.go:1425-1438
            become_follower(term)
        elif term != 0 and term < g["term"]:                      # raft.go:1439-1450
            replies.append((MSG_NOOP, g["term"]) if check_quorum else (0, 0))
            continue
        if g["state"] == LEADER:                                  # no handler registered
            replies.append((0, 0))
            continue
        if g["state"] == CANDIDATE:                               # handleCandidateHeartbeat
            become_follower(g["term"])
        res["flags"] |= CONTACT                                   # leaderIsAvailable
        res["leader"] = frm                                       # setLeaderID
        if commit > g["committed"] and commit <= g["last"]:       # commitTo
            g["committed"] = commit
            res["flags"] |= COMMITTED
        if commit > g["last"]:
            res["flags"] |= COMMIT_ABOVE_LAST
        res["commit"] = max(res["commit"], commit)
        replies.append((MSG_HEARTBEAT_RESP, g["term"]))
    res.update(term=g["term"], state=g["state"])
    return replies, res, g


def counts(all_replies, all_results):
    """hq_hb_received_output's six counts of a call's replies and results."""
    return {"n_resp": sum(t == MSG_HEARTBEAT_RESP for t, _ in all_replies),
            "n_noop": sum(t == MSG_NOOP for t, _ in all_replies),
            "n_contact": sum(bool(r["flags"] & CONTACT) for r in all_results),
            "n_committed": sum(bool(r["flags"] & COMMITTED) for r in all_results),
            "n_state_changed": sum(r["n_resets"] > 0 for r in all_results),
            "n_suspended": sum(bool(r["flags"] & SUSPENDED) for r in all_results)}


def expand(rows, replies, cluster_ids, node_ids):
    """hq_heartbeat_replies_expand: rows[i] the messages of listed group i, replies in message
    order. Returns dicts of the wire message's nonzero fields, in input order."""
    out, k = [], 0
    for i, msgs in enumerate(rows):
        for frm, _term, _commit, hint, high in msgs:
            typ, term = replies[k]
            k += 1
            if typ == 0:
                continue
            echo = typ == MSG_HEARTBEAT_RESP
            out.append({"kind": EV_MESSAGE, "type": typ, "from": node_ids[i], "to": frm,
                        "cluster_id": cluster_ids[i], "term": term, "hint": hint if echo else 0,
                        "hint_high": high if echo else 0})
    return out


def random_messages(rng, group, max_msgs=4, members=(2, 3, 4), u64=False):
    """0 .. max_msgs received heartbeats for a group: terms below, at and above its term and 0,
    commits below, at and above committed and last; later messages are drawn against the state the
    earlier ones leave (so candidate -> follower -> higher term occurs within one group)."""
    g = dict(group)
    msgs = []
    for _ in range(int(rng.integers(0, max_msgs + 1))):
        u = rng.random()
        term = g["term"] if u < 0.55 else 0 if u < 0.65 else max(g["term"] - int(rng.integers(1, 3)), 1) \
            if u < 0.82 else g["term"] + int(rng.integers(1, 3))
        v = rng.random()
        commit = (max(g["committed"] - int(rng.integers(0, 3)), 0) if v < 0.3 else
                  g["committed"] + int(rng.integers(0, g["last"] - g["committed"] + 1)) if v < 0.75 and g["last"] >= g["committed"] else
                  g["last"] if v < 0.85 else g["last"] + int(rng.integers(1, 4)))
        if u64:
            term, commit = min(term, (1 << 64) - 1), min(commit, (1 << 64) - 1)
        ctx = (int(rng.integers(1, 1 << 62)), int(rng.integers(0, 1 << 62))) if rng.random() < 0.4 else (0, 0)
        m = (int(rng.choice(members)), term, commit) + ctx
        msgs.append(m)
        _, _, g = handle(dict(g, suspended=False), [m], True)
    return msgs


class Seen:
    """What a run of calls has shown: a test that cannot reach a branch must fail, not pass."""

    def __init__(self):
        self.types, self.flags, self.n_resets, self.demoted = set(), 0, set(), 0
        self.cand_then_higher = 0

    def add(self, before, replies, res):
        self.types |= {t for t, _ in replies}
        self.flags |= res["flags"]
        self.n_resets.add(min(res["n_resets"], 2))
        self.demoted += before["state"] == LEADER and res["n_resets"] > 0
        self.cand_then_higher += before["state"] == CANDIDATE and res["n_resets"] >= 2

    def check(self, suspended=False, noop=True):
        assert self.types >= {0, MSG_HEARTBEAT_RESP} | ({MSG_NOOP} if noop else set()), self.types
        want = COMMITTED | COMMIT_ABOVE_LAST | CONTACT | (SUSPENDED if suspended else 0)
        assert self.flags & want == want, self.flags
        assert self.n_resets == {0, 1, 2}, self.n_resets
        assert self.demoted > 0 and self.cand_then_higher > 0, (self.demoted, self.cand_then_higher)
