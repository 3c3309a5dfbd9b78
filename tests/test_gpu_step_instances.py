"""The device step's kernel instances, one case per pair of member-slot width and input form: the
launchers of hq_dstep_step.hip / hq_dstep_layout.hip pick k_step<..., 8 | 16> and the rows /
stream / jobs kernels from the worker's widest group and the step's input, and every pick must give
what the host worker gives for the same events, list by list and bit for bit.

The device lists every record in input group order. The host worker lists a step's records pass
by pass (a group whose events need a second decision pass has its later records behind every
group's first-pass ones), each group's in the same order; so its lists are regrouped by listed
position with a stable sort before the comparison, and the device's must be in that order as they
come.

Each form must also take the path it is named for. The copy path and the single-job path both
report gpu_jobs = 1, so the workers run with HQ_WAIT_CLOCK: only the jobs path (a pinned stream
alone, or fused) stamps the device's clock ahead of its first launch, and the step then reports
device_start_ticks with device_end_ticks no more than a second (10^8 ticks of 100 MHz) after it.

The world is 600 leader groups: three 256-group tiles of pass A, the last one partial (88 groups:
one full wave and a partial one)."""
import numpy as np
import pytest

import step_random as sr
import step_scenarios as sc
from step_harness import WorkerBackend, event_record

pytestmark = pytest.mark.gpu

G, STEPS = 600, 3
WIDTHS = {"8-slots": 3, "16-slots": 9}      # members per group -> k_step<..., 8> / <..., kDMembers>
FORMS = ["rows", "stream", "sized32-pageable", "sized16-pinned", "sized16-pinned-fused"]
LISTS = ("commits", "ready", "read_resps", "state_changes", "dropped_reads", "deferred",
         "fallback_groups")


def _regrouped(res, off):
    """res's lists with the records in order of their group's listed position, stably: the
    groups are cluster ids 1..G listed in that order, `deferred` holds event indexes."""
    out = {}
    for k in LISTS:
        a = res[k]
        pos = np.searchsorted(off, a, side="right") if k == "deferred" else \
            a if k == "fallback_groups" else a["cluster_id"]
        out[k] = a[np.argsort(pos, kind="stable")]
    return out


def _leader_world(rng, n_members):
    """G leaders (node 1) of n_members members with node ids 1..n: three voting remotes, the rest
    observers (which hold the top ids, as step_random._run_events expects)."""
    groups = []
    for j in range(G):
        last = 100 + int(rng.integers(0, 50))
        committed = last - int(rng.integers(0, 9))
        mem = [(i, last if i == 1 else int(rng.integers(max(0, committed - 3), last + 1)),
                sc.REMOTE if i <= 3 else sc.OBSERVER, int(rng.random() < 0.5))
               for i in range(1, n_members + 1)]
        groups.append((1 + j, 1, int(rng.integers(2, 9)), sc.LEADER, committed, last,
                       last - int(rng.integers(0, 6)), [mem[k] for k in rng.permutation(n_members)]))
    return groups


@pytest.fixture(scope="module")
def worlds(hq):
    """Per width: the groups, each step's rows (handles, offsets, events) and the host worker's
    results for them, computed once and shared by the forms."""
    out = {}
    for name, n_members in WIDTHS.items():
        rng = np.random.default_rng(600 + n_members)
        groups = _leader_world(rng, n_members)
        host = WorkerBackend(hq, n_max=3, on_device=False)
        try:
            for g in groups:
                host.add_group(*g)
            ctx_seq, steps = [0], []
            for s in range(STEPS):
                # every group listed, in handle order; runs of consecutive senders for the even
                # groups (the stream's run form, take_run), the general mix for the odd ones
                handles, offsets, recs = [], [0], []
                for g in groups:
                    st = host.state(g[0])
                    ev = sr._run_events(rng, st, ctx_seq) if g[0] % 2 == 0 else \
                        sr.random_events(rng, st, s, ctx_seq)
                    handles.append(host.w.find(g[0]))
                    recs += [event_record(hq, e) for e in ev]
                    offsets.append(len(recs))
                rows = (np.array(handles, np.uint32), np.array(offsets, np.uint64),
                        np.array(recs, hq.EVENT_DTYPE))
                steps.append((rows, _regrouped(host.w.step(*rows), rows[1])))
            assert sum(len(w["commits"]) for _, w in steps) > G // 4
            assert sum(len(w["ready"]) for _, w in steps) > G // 8
            out[name] = (groups, steps)
        finally:
            host.close()
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("width", list(WIDTHS))
def test_every_instance_equals_host_worker(hq, worlds, width, form):
    groups, steps = worlds[width]
    devs = [hq.Worker(0, 3, on_device=True) for _ in range(2 if form.endswith("fused") else 1)]
    pin = hq.Context(0) if "pinned" in form else None
    try:
        for w in devs:
            w.set_wait(clock=True)
            for g in groups:
                w.add_group(*g)

        def pinned(a):
            p = pin.pinned(max(len(a), 1), a.dtype)
            p[:len(a)] = a
            return p[:len(a)]

        for s, ((grp, off, ev), want) in enumerate(steps):
            if form == "rows":
                gots = [devs[0].step(grp, off, ev)]
            elif form == "stream":
                data, boff = hq.encode_events(off, ev)
                gots = [devs[0].step_stream(grp, off, boff, data)]
            else:
                data, sizes = hq.encode_events_sized(off, ev)
                if form.startswith("sized16"):
                    sizes = hq.sizes16_of(sizes)
                if pin:
                    data, sizes = pinned(data), pinned(sizes)
                job = hq.SizedStream(grp, sizes, len(ev), data)
                if len(devs) == 2:          # hq_worker_step_jobs: shared launches for both
                    gots = hq.step_jobs([(w, job) for w in devs])
                    assert [g["gpu_jobs"] for g in gots] == [2, 2]
                else:
                    gots = [devs[0].step_sized(*job)]
            for j, got in enumerate(gots):
                if pin:                     # the jobs path: pass A read the pinned stream in place
                    t0, t1 = got["device_start_ticks"], got["device_end_ticks"]
                    assert 0 < t0 <= t1 < t0 + 10**8, (width, form, s, j, t0, t1)
                ordered = _regrouped(got, off)
                for k in LISTS:
                    assert got[k].tobytes() == ordered[k].tobytes(), (width, form, s, j, k)
                    assert got[k].dtype == want[k].dtype and \
                        got[k].tobytes() == want[k].tobytes(), (width, form, s, j, k)
    finally:
        for w in devs:
            w.close()
        if pin:
            pin.close()
