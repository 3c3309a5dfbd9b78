"""Helpers of the group-lifecycle tests (hq_worker_start_groups / _stop_groups / _pool_info /
_compact): a Python model of the worker's handle space, a worker proxy whose get_group does not
read the device state back, and a world that keeps the CPU oracle, the model and any number of
workers in step. Nothing here touches the code under test beyond calling it.

The handle rule (include/hipquorum.h "group lifecycle"): a stop vacates its handles in list
order; a start takes the most recently vacated handle first (a stack), else the next new handle;
the handle space never shrinks."""
import numpy as np

import step_scenarios as sc
from step_harness import OracleBackend, WorkerBackend, same_step

ARRAYS = ("groups", "members", "member_offsets", "reads", "read_offsets", "granted", "rejected",
          "read_confirmed")


class HandleModel:
    """cluster[h]: the cluster id a handle holds, None while it is vacant."""

    def __init__(self):
        self.cluster = []
        self.vacant = []
        self.epoch = 0

    def start(self, cids):
        assert len(set(cids)) == len(cids) and not set(cids) & set(self.live_cids())
        out = []
        for c in cids:
            if self.vacant:
                h = self.vacant.pop()
                self.cluster[h] = c
            else:
                h = len(self.cluster)
                self.cluster.append(c)
            out.append(h)
        self.epoch += 1 if cids else 0
        return out

    def stop(self, handles):
        assert len(set(handles)) == len(handles)
        for h in handles:
            assert self.cluster[h] is not None
            self.cluster[h] = None
            self.vacant.append(h)
        self.epoch += 1 if handles else 0

    @property
    def handles(self):
        return len(self.cluster)

    def live(self):
        return [h for h, c in enumerate(self.cluster) if c is not None]

    def live_cids(self):
        return [c for c in self.cluster if c is not None]

    def find(self, cid):
        return self.cluster.index(cid)


class NoReadback:
    """A Worker whose get_group(cid) is answered from hq_worker_get_groups (no copy of the device
    state): one fetch of every live handle per step, kept until the state changes again."""

    def __init__(self, w, model):
        self.w, self.model, self._cache = w, model, None

    def __getattr__(self, name):
        attr = getattr(self.w, name)
        if name in ("step", "step_sized", "step_stream", "start_groups", "stop_groups",
                    "config_changes", "set_groups", "compact"):
            def call(*a, **k):
                self._cache = None
                return attr(*a, **k)
            return call
        return attr

    def get_group(self, cid):
        if self._cache is None:
            live = self.model.live()
            r = self.w.get_groups(np.array(live, np.uint32))
            self._cache = (r, {int(c): i for i, c in enumerate(r["groups"]["cluster_id"])})
        r, at = self._cache
        i = at[cid]
        mo, ro = r["member_offsets"], r["read_offsets"]
        return (r["groups"][i], r["members"][int(mo[i]):int(mo[i + 1])],
                r["reads"][int(ro[i]):int(ro[i + 1])])


def group_arrays(hq, specs):
    """(cid, node, term, state, committed, last, term_start, members, ...) tuples as the
    WORKER_GROUP_DTYPE / MEMBER_DTYPE arrays of add_groups / start_groups."""
    g = np.zeros(len(specs), hq.WORKER_GROUP_DTYPE)
    mem = []
    for i, s in enumerate(specs):
        (g["cluster_id"][i], g["node_id"][i], g["term"][i], g["state"][i], g["committed"][i],
         g["last_index"][i], g["term_start"][i]) = s[:7]
        g["n_members"][i] = len(s[7])
        mem += [tuple(m) for m in s[7]]
    return g, np.array(mem, hq.MEMBER_DTYPE)


def same_output(a, b):
    for k in ARRAYS:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def snapshot(w, handles):
    r = w.get_groups(np.array(handles, np.uint32))
    return {k: r[k].tobytes() for k in ARRAYS}


class World:
    """The oracle's groups by cluster id, the handle model and the workers (name -> Worker), each
    behind a step_harness.WorkerBackend of its stream form. Device workers must never read back."""

    def __init__(self, hq, workers, streams, seed=3):
        self.hq = hq
        self.oracle = OracleBackend()
        self.model = HandleModel()
        self.workers = workers
        self.backs = {n: WorkerBackend(hq, worker=NoReadback(w, self.model), seed=seed,
                                       stream=streams[n]) for n, w in workers.items()}
        self.node_of = {}

    def close(self):
        for b in self.backs.values():
            if b.pin:
                b.pin.close()
        for w in self.workers.values():
            w.close()

    def start(self, specs, via_add=False):
        """specs as step_random.random_groups gives them. via_add: hq_worker_add_group (the first
        groups of a fresh worker: the same handles as the model's)."""
        want = self.model.start([s[0] for s in specs])
        for s in specs:
            self.oracle.add_group(*s)
            self.node_of[s[0]] = s[1]
        g, m = group_arrays(self.hq, specs)
        for b in self.backs.values():
            if via_add:
                b.w.add_groups(g, m)
                got = [b.w.find(s[0]) for s in specs]
            else:
                got = b.w.start_groups(g, m).tolist()
            assert got == want, (got, want)
        return want

    def stop(self, handles):
        cids = [self.model.cluster[h] for h in handles]
        self.model.stop(handles)
        for c in cids:
            del self.oracle.groups[c]
        for b in self.backs.values():
            b.w.stop_groups(np.array(handles, np.uint32))
        return cids

    def step(self, per):
        """One step on the oracle and every worker; every listed cluster must match."""
        want = self.oracle.step(per)
        for name, b in self.backs.items():
            got = b.step(per)
            assert got["_fallback"] == [], (name, got["_fallback"])
            for cid in per:
                same_step(want, got, cid)
        return want

    def no_readback(self):
        for name, w in self.workers.items():
            assert w.readback_count() == 0, name


def leader(cid, n, last, committed=None, node=1, term=2, observers=0):
    """A leader of n remotes (node ids 1 .. n, the node itself `node`) and `observers` observers,
    every follower at `committed`."""
    committed = last if committed is None else committed
    mem = [(i, last if i == node else committed, sc.REMOTE, 0) for i in range(1, n + 1)]
    mem += [(100 + i, committed, sc.OBSERVER, 0) for i in range(observers)]
    return (cid, node, term, sc.LEADER, committed, last, committed, mem, None)
