"""The expected values of the Raft-timer tests (hq_worker_set_tick_config / _tick / _get_timers /
_set_timers, hq_tick_timeout): a direct Python restatement of include/hipquorum.h "raft timers"
over the groups' (cluster id, term, state) as step_harness.OracleBackend (or a test's own table)
holds them. It shares no code with the library's hq_tick.h.

A group is given to the model per handle as (cluster_id, term, state, suspended), None for a vacant
handle. The model keeps per handle [election_tick, heartbeat_tick, randomized_timeout, term, state],
or nothing for a timer that comes back reset."""
M64 = (1 << 64) - 1
FOLLOWER, CANDIDATE, LEADER = 0, 1, 2


def timeout(seed, cluster_id, term, state, E):
    """hq_tick_timeout's formula, all arithmetic modulo 2^64."""
    x = seed ^ (cluster_id * 0x9E3779B97F4A7C15 & M64) ^ (term * 0xBF58476D1CE4E5B9 & M64) ^ state
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return E + z % E


class TickModel:
    def __init__(self, election_rtt, heartbeat_rtt, check_quorum, seed):
        self.E, self.H, self.cq, self.seed = election_rtt, heartbeat_rtt, bool(check_quorum), seed
        self.timers = {}
        self.resets = 0        # resets of timers that had counted under another (term, state)

    def reset(self, handle):
        """The handle was started, re-synced or un-suspended: its timer comes back reset."""
        self.timers.pop(handle, None)

    def _current(self, handle, group):
        """The handle's timer after step 1 (reset) of a tick, as a new list; not stored."""
        cid, term, state, _ = group
        t = self.timers.get(handle)
        if t is None or (t[3], t[4]) != (term, state):
            return [0, 0, timeout(self.seed, cid, term, state, self.E), term, state], t is not None
        return list(t), False

    def tick(self, groups, contact=()):
        """One tick of groups[h] for every handle h. Returns (check_quorum, heartbeat, election,
        n_ticked): three ascending handle lists and the number of groups advanced."""
        contact = set(int(h) for h in contact)
        cq, hb, el, ticked = [], [], [], 0
        for h, g in enumerate(groups):
            if g is None or g[3]:                   # vacant or suspended: not ticked, back reset
                self.timers.pop(h, None)
                continue
            t, was_reset = self._current(h, g)
            self.resets += was_reset
            ticked += 1
            if g[2] == LEADER:
                t[0] += 1
                if t[0] >= self.E:
                    t[0] = 0
                    if self.cq:
                        cq.append(h)
                t[1] += 1
                if t[1] >= self.H:
                    t[1] = 0
                    hb.append(h)
            else:
                if h in contact:
                    t[0] = 0
                t[0] += 1
                if t[0] >= t[2]:
                    t[0] = 0
                    el.append(h)
            self.timers[h] = t
        return cq, hb, el, ticked

    def get(self, handle, group):
        """hq_worker_get_timers' (election_tick, heartbeat_tick, randomized_timeout)."""
        t, _ = self._current(handle, group)
        return tuple(t[:3])

    def set(self, handle, group, election_tick, heartbeat_tick, randomized_timeout):
        cid, term, state, _ = group
        rt = randomized_timeout or timeout(self.seed, cid, term, state, self.E)
        self.timers[handle] = [election_tick, heartbeat_tick, rt, term, state]


def check_tick(got, want):
    """A Worker.tick result against TickModel.tick's; the lists strictly ascending."""
    for name, exp in zip(("check_quorum", "heartbeat", "election"), want[:3]):
        lst = got[name].tolist()
        assert all(a < b for a, b in zip(lst, lst[1:])), name
        assert lst == exp, (name, lst[:8], exp[:8], len(lst), len(exp))
    assert got["n_ticked"] == want[3]


def check_timers(worker, model, groups, handles=None):
    """get_timers of the live handles (or `handles`) against the model."""
    if handles is None:
        handles = [h for h, g in enumerate(groups) if g is not None]
    if not handles:
        return
    import numpy as np

    got = worker.get_timers(np.array(handles, np.uint32))
    have = list(zip(got["election_tick"].tolist(), got["heartbeat_tick"].tolist(),
                    got["randomized_timeout"].tolist()))
    want = [model.get(h, groups[h]) for h in handles]
    assert have == want, [(h, a, b) for h, a, b in zip(handles, have, want) if a != b][:5]
    assert not got["reserved"].any()
