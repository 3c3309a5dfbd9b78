"""The small worlds of tests/step_random.py translated into corners of the u64 range.

The generators draw node ids 1..63, indexes 91..200, terms 2..10, ReadIndex ctxs that are small
counters and cluster ids 1..G; the step worker's width assumptions (a run's 32-bit first sender,
hq_event16's 16-bit sender and 32-bit term, the 4-byte commit advance, the int32 ReadyToRead delta,
the device hash table's cluster ids, 64-bit match and id values in registers) only show at other
values. A Shift maps a group tuple and an event tuple of those generators to their shifted forms,
and a shifted backend.state() back to small values, so that the generators keep producing events
inside the worker's contract:

  indexes      i -> i + B, a literal 0 (a follower's remote match, a message without an index)
               stays 0: committed, last, term_start, member matches, message log_index, the log's
               first_minus_1 and run starts (run 0's start stays 0); propose counts are not shifted
  terms        t -> t + T, a message term of 0 stays 0: the group term, message terms, log run terms
  node ids     k -> N + k: node, members, message `from` (the non-member 999 included); an id that
               would pass 2^64 - 1 maps to k itself, a small id that is no member because every
               member id is large (which breaks a consecutive run at the top on purpose); 0, the
               `from` of a local read in the outputs, is no node and stays 0
  ctxs         (lo, hi) -> (lo + C, hi + C), (0, 0) (no ctx) stays (0, 0)
  cluster ids  cid -> cid + K

The oracle is equivariant under a Shift (tests/test_step_shift.py holds it to that), which is what
makes the shifted worlds in-contract and their expected results known.
"""
import functools

import numpy as np

import step_random as sr
from step_harness import OracleBackend

M = 2**64 - 1


class Shift:
    def __init__(self, B, T, N, C, K):
        self.B, self.T, self.N, self.C, self.K = B, T, N, C, K

    # ---- values -------------------------------------------------------------------------------
    def index(self, i):
        return i + self.B if i else 0

    def term(self, t):
        return t + self.T if t else 0

    def node(self, k):
        if k == 0:
            return 0
        return self.N + k if self.N + k <= M else k

    def ctx(self, lo, hi):
        return (lo + self.C, hi + self.C) if (lo, hi) != (0, 0) else (0, 0)

    def cluster(self, cid):
        return cid + self.K

    def _unindex(self, v):
        return v - self.B if v else 0

    def _unnode(self, v):
        return v - self.N if v > self.N else v

    def _unctx(self, lo, hi):
        return (lo - self.C, hi - self.C) if (lo, hi) != (0, 0) else (0, 0)

    # ---- generator tuples ---------------------------------------------------------------------
    def group(self, g):
        """(cid, node, term, state, committed, last, term_start, members[, log]) shifted."""
        cid, node, term, state, committed, last, term_start, mem = g[:8]
        out = (self.cluster(cid), self.node(node), self.term(term), state, self.index(committed),
               self.index(last), self.index(term_start),
               [(self.node(i), self.index(m), r, a) for i, m, r, a in mem])
        if len(g) > 8:
            first_minus_1, runs = g[8]
            out += ((self.index(first_minus_1),
                     [(self.index(s), self.term(t)) for s, t in runs]),)
        return out

    def event(self, e):
        if e[0] == "read":
            return ("read",) + self.ctx(e[1], e[2])
        if e[0] == "msg":
            _, typ, frm, term, idx, hint, high, rej = e
            return ("msg", typ, self.node(frm), self.term(term), self.index(idx)) + \
                self.ctx(hint, high) + (rej,)
        return e                                  # check_quorum, campaign, propose (a count)

    # ---- results ------------------------------------------------------------------------------
    def out(self, r):
        """A group's step results (OracleBackend.step / WorkerBackend.step) shifted."""
        return {
            "committed": self.index(r["committed"]), "commit_changed": r["commit_changed"],
            "ready": [(self.index(i),) + self.ctx(lo, hi) for i, lo, hi in r["ready"]],
            "resps": [(self.node(to), self.index(i)) + self.ctx(lo, hi)
                      for to, i, lo, hi in r["resps"]],
            "states": [(self.term(t), st, why) for t, st, why in r["states"]],
            "dropped": [self.ctx(lo, hi) + (self.node(frm), why)
                        for lo, hi, frm, why in r["dropped"]],
            "deferred": list(r["deferred"]),
        }

    def state(self, s):
        """backend.state() of a small group as its shifted group's."""
        term, st, committed, last, term_start, mem, reads = s
        return (self.term(term), st, self.index(committed), self.index(last),
                self.index(term_start), [(self.node(i), self.index(m), r, a) for i, m, r, a in mem],
                [(self.index(i), self.node(frm), self.ctx(*c), n) for i, frm, c, n in reads])

    def unstate(self, s):
        """The inverse of state(): a shifted backend.state() as the generators read it."""
        term, st, committed, last, term_start, mem, reads = s
        return (term - self.T, st, self._unindex(committed), self._unindex(last),
                self._unindex(term_start),
                [(self._unnode(i), self._unindex(m), r, a) for i, m, r, a in mem],
                [(self._unindex(i), self._unnode(frm), self._unctx(*c), n)
                 for i, frm, c, n in reads])


# world -> (B, T, N of the random world, C, K). Each boundary falls inside the world: indexes
# 91..200 + B straddle 2^31 / 2^32 / 2^63, ids 1..63 + N straddle 2^16 / 2^32 / 2^63, terms cross
# theirs as campaigns raise them. u16 drives hq_event16's escapes (senders at and above 2^16, a
# ctx high word at 2^16). top leaves room for a run's proposals and campaigns without wrapping,
# and its K keeps (1 << 62) + cid ("a cluster this host does not run" of the wire backends) below
# 2^64 and distinct from every member cluster.
WORLDS = {
    "small": (0, 0, 0, 0, 0),
    "u16": (2**31 - 120, 2**16 - 5, 2**16 - 32, 2**16 - 3, 2**16 - 100),
    "u32": (2**32 - 120, 2**32 - 5, 2**32 - 32, 2**32 - 3, 2**32 - 100),
    "u63": (2**63 - 120, 2**63 - 5, 2**63 - 32, 2**63 - 3, 2**63 - 100),
    "top": (2**64 - 2**20, 2**64 - 2**16, 2**64 - 64, 2**64 - 2**24, 3 * 2**62 - 2**32),
}
SHIFTED = ("u16", "u32", "u63", "top")
# the runs world (members 1..n, the leader node 1): N is the boundary - 4, so that runs cross it;
# top: N = M - n per group, the group's last member node 2^64 - 1 and the senders "past the
# members" small non-member ids
RUNS_BOUNDARY = {"u16": 2**16, "u32": 2**32, "u63": 2**63}
# (kind) -> (groups, steps, seed)
SIZES = {"random": (400, 8, 1), "runs": (400, 5, 31)}
# the random world's events and outputs over its 8 steps, the same in every world
RANDOM_EVENTS = 20468
RANDOM_SEEN = dict(ready=195, resps=90, states=941, dropped=374, deferred=2224, commit=214)


def shift_of(kind, world, g):
    """The Shift of small group g in `world` (kind "random" or "runs")."""
    B, T, N, C, K = WORLDS[world]
    if kind == "runs" and world != "small":
        N = M - len(g[7]) if world == "top" else RUNS_BOUNDARY[world] - 4
    return Shift(B, T, N, C, K)


def small_groups(kind, rng, G):
    return sr.random_groups(rng, G) if kind == "random" else sr._consecutive_groups(rng, G)


def small_events(kind, rng, groups, state_of, step, ctx_seq):
    """One step of small events, {small cid: events}: the draws of test_random_differential
    (random) and test_consecutive_runs_device_equals_reference (runs) in tests/test_gpu_worker.py.
    state_of(small cid) is the group's small state."""
    per = {}
    for g in groups:
        if kind == "random":
            if rng.random() < 0.85:
                per[g[0]] = sr.random_events(rng, state_of(g[0]), step + 1, ctx_seq)
        elif rng.random() < 0.9:
            per[g[0]] = sr._run_events(rng, state_of(g[0]), ctx_seq)
    return per


KINDS = ("ready", "resps", "states", "dropped", "deferred")


def count_seen(seen, out):
    seen["commit"] += out["commit_changed"]
    for k in KINDS:
        seen[k] += len(out[k])


class Reference:
    """A shifted world run through the oracle: groups (shifted tuples), steps = [(per, want,
    states)] with per {shifted cid: shifted events}, want the oracle's step results and states
    {shifted cid: state()} after the step, seen the output counts and n_events. The events come
    from the generators applied to the shifted oracle's state mapped back (Shift.unstate)."""

    def __init__(self, kind, world):
        G, steps, seed = SIZES[kind]
        rng = np.random.default_rng(seed)
        small = small_groups(kind, rng, G)
        self.shifts = {g[0]: shift_of(kind, world, g) for g in small}
        self.groups = [self.shifts[g[0]].group(g) for g in small]
        big = {g[0]: b[0] for g, b in zip(small, self.groups)}
        o = OracleBackend()
        for b in self.groups:
            o.add_group(*b)
        ctx_seq = [0]
        self.seen = dict(ready=0, resps=0, states=0, dropped=0, deferred=0, commit=0)
        self.n_events = 0
        self.steps = []
        for s in range(steps):
            per = small_events(kind, rng, small,
                               lambda c: self.shifts[c].unstate(o.state(big[c])), s, ctx_seq)
            per = {big[c]: [self.shifts[c].event(e) for e in ev] for c, ev in per.items()}
            want = o.step(per)
            for cid in per:
                count_seen(self.seen, want[cid])
            self.n_events += sum(len(ev) for ev in per.values())
            self.steps.append((per, want, {b[0]: o.state(b[0]) for b in self.groups}))


@functools.lru_cache(maxsize=None)
def reference(kind, world):
    """The Reference of (kind, world), computed once and shared: treat it as read-only."""
    return Reference(kind, world)


def rows(hq, per):
    """A step's events as (offsets, hq_event rows), the groups in per's order."""
    from step_harness import event_record

    off, recs = [0], []
    for events in per.values():
        recs += [event_record(hq, e) for e in events]
        off.append(len(recs))
    return np.array(off, np.uint64), np.array(recs, hq.EVENT_DTYPE)


RUN_HEADER = 2 | 6 << 3                            # HQ_EV_MESSAGE, code 6; | 0x80: consecutive


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def run_headers(data, boff):
    """(consecutive-form, listed) run headers of a stream, found by walking every group's events
    (a byte search would also count varint bytes that look like a header)."""
    data = bytes(data)

    def skip(p):                                   # past one varint
        while data[p] & 0x80:
            p += 1
        return p + 1

    seq = listed = 0
    for b0, b1 in zip(boff[:-1], boff[1:]):
        p, end = int(b0), int(b1)
        while p < end:
            h = data[p]
            p += 1
            kind, code = h & 7, (h >> 3) & 7
            n = 0                                  # varints after the header
            if kind == 1:                          # READ: hint, hint_high
                n = 2
            elif kind == 5:                        # PROPOSE: the count
                n = 1
            elif kind == 2 and code == 6:          # a run: m, then s0 or m senders
                m = data[p]
                assert 1 <= m < 0x80
                seq += h >> 7
                listed += 1 - (h >> 7)
                n = 2 if h & 0x80 else 1 + m
            elif kind == 2:                        # [type], from, [term], [index], [hint, high]
                n = 1 + (code == 7) + (not h & 0x80) + (code in (0, 7)) + 2 * (code in (2, 3, 7))
            for _ in range(n):
                p = skip(p)
        assert p == end
    return seq, listed


def escaped_rows(hq, recs, off16, off):
    """Which rows hq_events_to16 wrote as an escape (5 records), as a bool array over the rows."""
    out = np.zeros(int(off[-1]), bool)
    for g in range(len(off) - 1):
        k, e = int(off16[g]), int(off[g])
        while k < int(off16[g + 1]):
            full = bool(recs["kind"][k] & hq.EV16_FULL)
            out[e] = full
            k += 5 if full else 1
            e += 1
        assert e == int(off[g + 1])
    return out


def wrapped_run_stream():
    """A hand-made group stream of 4 events: a valid ReplicateResp (from 2, term 2, index 6), then
    a consecutive-form run header with m = 3 and the 10-byte first sender 2^64 - 3, whose last
    sender would be 2^64 - 1 and whose s0 + m wraps to 0 in 64 bits. Malformed: the consecutive
    form holds senders below 2^32 only."""
    return np.frombuffer(bytes([2 | 0 << 3, 2, 2, 6, RUN_HEADER | 0x80, 3]) + varint(2**64 - 3),
                         np.uint8)
