"""Membership changes restated in Python for the config-change tests: handleNodeConfigChange
(raft.go:1540-1559) -> addNode / addObserver / addWitness / removeNode (raft.go:1136-1199) with
removeNode's tryCommit (raft.go:888-909, logentry.go:378-393), over a group as Worker.get_group
reports it, plus the worker's own rules of include/hipquorum.h "membership changes": where a
member stands in the list afterwards, and when a change is a fallback. Nothing here touches the
code under test.

A group is a dict: node_id, state, committed, last_index, term_start, suspended, members (list
order: dicts of node_id, match, role, active), reads (dicts of index, from, ctx, n_confirmed).
"""
import copy
import json
import os

REMOTE, OBSERVER, WITNESS = 0, 1, 2
FOLLOWER, CANDIDATE, LEADER = 0, 1, 2
ADD_NODE, REMOVE_NODE, ADD_OBSERVER, ADD_WITNESS = 0, 1, 2, 3
APPLIED, NOOP, FALLBACK, SUSPENDED = 0, 1, 2, 3
ROUTE_NONE = 0xFFFF
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config_change_kats.json")


def kats():
    return json.load(open(KATS))["cases"]


def group_of(w, cid):
    """A worker's group as the model takes it (Worker.get_group: a readback on a device worker)."""
    g, m, r = w.get_group(cid)
    return {"cluster_id": int(g["cluster_id"]), "node_id": int(g["node_id"]), "term": int(g["term"]),
            "state": int(g["state"]), "committed": int(g["committed"]),
            "last_index": int(g["last_index"]), "term_start": int(g["term_start"]),
            "suspended": int(g["suspended"]),
            "members": [{"node_id": int(x["node_id"]), "match": int(x["match"]),
                         "role": int(x["role"]), "active": int(x["active"])} for x in m],
            "reads": [{"index": int(x["index"]), "from": int(x["from"]),
                       "ctx": (int(x["ctx_low"]), int(x["ctx_high"])),
                       "n_confirmed": int(x["n_confirmed"])} for x in r]}


def member_tuples(group):
    return [(m["node_id"], m["match"], m["role"], m["active"]) for m in group["members"]]


def voting(group):
    return [m for m in group["members"] if m["role"] != OBSERVER]


def try_commit(group):
    """raft.tryCommit: the quorum-th largest voting match q; committed iff q > committed and
    term(q) == term, which for a leader is term_start <= q <= last_index. Returns q or None."""
    matched = sorted((m["match"] for m in voting(group)), reverse=True)
    q = matched[len(matched) // 2]                      # the (n / 2 + 1)-th largest
    if q > group["committed"] and group["term_start"] <= q <= group["last_index"]:
        return q
    return None


def invalid(groups, changes):
    """Whether the worker refuses the whole list (HQ_E_INVAL). groups: handle -> group, or None
    for an unknown handle; changes: (handle, type, node_id)."""
    seen = set()
    for h, t, nid in changes:
        g = groups.get(h)
        if g is None or h in seen or t not in (ADD_NODE, REMOVE_NODE, ADD_OBSERVER, ADD_WITNESS):
            return True
        seen.add(h)
        if nid == 0:
            return True
        role = {m["node_id"]: m["role"] for m in g["members"]}.get(nid)
        if t == ADD_NODE and role == WITNESS:           # the reference panics (raft.go:1153-1154)
            return True
        if t == ADD_OBSERVER and role not in (None, OBSERVER):
            return True
        if t == ADD_WITNESS and role not in (None, WITNESS):
            return True
    return False


def apply(group, ctype, node_id, n_max, member_limit, acked=()):
    """One valid change. acked: the node ids that hold a recorded vote (granted or rejected) or an
    acknowledgement of a pending ReadIndex in this group — what get_group does not report; the
    caller knows it from the events it sent. Returns (status, group afterwards, commit): the
    group is a new dict, commit the index removeNode's tryCommit advanced to or None."""
    g = copy.deepcopy(group)
    if g["suspended"]:
        return SUSPENDED, g, None
    by_id = {m["node_id"]: i for i, m in enumerate(g["members"])}
    i = by_id.get(node_id)
    role = g["members"][i]["role"] if i is not None else None
    n_voting = len(voting(g))

    def fallback():
        g["suspended"] = 1
        return FALLBACK, g, None

    if ctype == REMOVE_NODE:
        status = NOOP
        if i is not None:
            if node_id == g["node_id"]:
                return fallback()                        # (b) the worker's own node
            if role != OBSERVER and node_id in acked:
                return fallback()                        # (c) a vote or ack the reference keeps
            del g["members"][i]                          # deleteRemote / Observer / Witness
            status = APPLIED
        commit = None
        if g["state"] == LEADER and voting(g):           # raft.go:1194-1198
            commit = try_commit(g)
            if commit is not None:
                g["committed"] = commit
        return status, g, commit
    want = {ADD_NODE: REMOTE, ADD_OBSERVER: OBSERVER, ADD_WITNESS: WITNESS}[ctype]
    if role == want:
        return NOOP, g, None
    if ctype == ADD_NODE and role == OBSERVER:           # promoted with its progress, in place
        if n_voting + 1 > n_max:
            return fallback()                            # (a)
        g["members"][i]["role"] = REMOTE
        return APPLIED, g, None
    assert role is None, "an invalid change (see invalid())"
    if len(g["members"]) + 1 > member_limit or (want != OBSERVER and n_voting + 1 > n_max):
        return fallback()                                # (a)
    g["members"].append({"node_id": node_id, "match": 0, "role": want, "active": 0})
    return APPLIED, g, None


def routes_after(row, group, ctype, node_id, status):
    """The group's route row (16 words by list position) after a change with `status`."""
    row = list(row)
    if status != APPLIED:
        return row
    ids = [m["node_id"] for m in group["members"]]
    if ctype == REMOVE_NODE:
        i = ids.index(node_id)
        if i < 16:
            del row[i]
            row.insert(min(len(ids), 16) - 1, ROUTE_NONE)
    elif node_id not in ids and len(ids) < 16:
        row[len(ids)] = ROUTE_NONE
    return row
