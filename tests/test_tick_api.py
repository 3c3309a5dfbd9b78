"""The Raft-timer entries of the ABI without a device (include/hipquorum.h "raft timers"): the
header declares them, the built library exports them, the refusals that need no worker,
hq_tick_timeout against the model of tick_model.py, the one-tick transition of
dragonboat_amd/csrc/hq_tick.h (the source the host worker and the kernels share) compiled into a
program of its own with -fsanitize=address,undefined and replayed against the model, and the seeds
of the GPU tests' random worlds, which must produce every kind of reset on the oracle alone. No
Python process loads sanitized code."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import tick_model as tm
import tick_world as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hipquorum.h")
ENTRIES = ("hq_worker_set_tick_config", "hq_worker_tick", "hq_tick_timeout", "hq_worker_get_timers",
           "hq_worker_set_timers")
U64 = (1 << 64) - 1


def header_text():
    s = open(HEADER).read()
    return " ".join(re.sub(r"/\*.*?\*/", " ", s, flags=re.S).split())


def struct_fields(s, name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), s)
    assert m, name
    return [(" ".join(t.split()), n) for t, n in re.findall(r"((?:const )?\w+ \*?)(\w+);", m.group(1))]


def test_header_declares_the_entries_and_the_structs():
    s = header_text()
    assert "int hq_worker_set_tick_config(hq_worker *w, const hq_tick_config *cfg);" in s
    assert ("int hq_worker_tick(hq_worker *w, uint64_t n_contact, const uint32_t *contact, "
            "hq_tick_output *out);") in s
    # (the value as an int: every exported entry of the header returns int, void or a string)
    assert ("int hq_tick_timeout(uint64_t seed, uint64_t cluster_id, uint64_t term, uint32_t state, "
            "uint32_t election_rtt);") in s
    assert "int hq_worker_get_timers(hq_worker *w, uint64_t n, const uint32_t *handles, hq_timer *out);" in s
    assert ("int hq_worker_set_timers(hq_worker *w, uint64_t n, const uint32_t *handles, "
            "const hq_timer *timers);") in s
    assert struct_fields(s, "hq_tick_config") == [
        ("uint32_t", "election_rtt"), ("uint32_t", "heartbeat_rtt"), ("uint32_t", "check_quorum"),
        ("uint32_t", "reserved"), ("uint64_t", "seed")]
    assert struct_fields(s, "hq_tick_output") == [
        ("const uint32_t *", "check_quorum"), ("uint64_t", "n_check_quorum"),
        ("const uint32_t *", "heartbeat"), ("uint64_t", "n_heartbeat"),
        ("const uint32_t *", "election"), ("uint64_t", "n_election"),
        ("uint64_t", "n_ticked"), ("uint64_t", "gpu_ns")]
    m = re.search(r"typedef struct hq_timer \{(.*?)\} hq_timer;", s)
    assert m and " ".join(m.group(1).split()) == \
        "uint32_t election_tick, heartbeat_tick, randomized_timeout, reserved;"
    assert re.search(r"#define HQ_ABI_VERSION 21u?\b", s)      # new symbols only: still ABI 21


def test_library_exports_them_and_the_binding_lists_them(hq):
    for name in ENTRIES:
        assert getattr(hq.lib, name) is not None
        assert name in hq.SIGNATURES
    assert [n for n, _ in hq.TickConfig._fields_] == ["election_rtt", "heartbeat_rtt", "check_quorum",
                                                      "reserved", "seed"]
    assert [n for n, _ in hq.TickOutput._fields_] == ["check_quorum", "n_check_quorum", "heartbeat",
                                                      "n_heartbeat", "election", "n_election",
                                                      "n_ticked", "gpu_ns"]
    assert hq.TIMER_DTYPE.names == ("election_tick", "heartbeat_tick", "randomized_timeout", "reserved")
    assert (ctypes.sizeof(hq.TickConfig), ctypes.sizeof(hq.TickOutput), hq.TIMER_DTYPE.itemsize) == \
        (24, 64, 16)
    for method in ("set_tick_config", "tick", "get_timers", "set_timers"):
        assert callable(getattr(hq.Worker, method))
    assert callable(hq.tick_timeout)


LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "hipquorum.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(hq_tick_config), sizeof(hq_tick_output), sizeof(hq_timer),
         offsetof(hq_tick_config, seed), offsetof(hq_tick_output, n_ticked), offsetof(hq_timer, reserved));
  return 0;
}
"""


def test_struct_sizes_in_c(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [24, 64, 16, 16, 48, 12]


def test_refusals_without_a_worker(hq):
    """A NULL worker is HQ_E_INVAL whatever else is passed (it is checked first: an out-of-range
    config with a NULL worker is refused for the worker), and nothing is written."""
    lib, inval = hq.lib, hq.HQ_E_INVAL
    good, bad = hq.TickConfig(10, 1, 1, 0, 7), hq.TickConfig(0, 1, 1, 0, 7)
    assert lib.hq_worker_set_tick_config(None, ctypes.byref(good)) == inval
    assert lib.hq_worker_set_tick_config(None, ctypes.byref(bad)) == inval
    assert lib.hq_worker_set_tick_config(None, None) == inval
    out = hq.TickOutput()
    out.n_ticked = 7
    h = np.zeros(1, np.uint32)
    t = np.full(1, 9, np.uint32).repeat(4).view(hq.TIMER_DTYPE)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.hq_worker_tick(None, 0, None, ctypes.byref(out)) == inval
    assert lib.hq_worker_tick(None, 1, vp(h), ctypes.byref(out)) == inval
    assert lib.hq_worker_tick(None, 0, None, None) == inval
    assert lib.hq_worker_get_timers(None, 1, vp(h), vp(t)) == inval
    assert lib.hq_worker_get_timers(None, 1, None, None) == inval
    assert lib.hq_worker_get_timers(None, 0, None, None) == inval
    assert lib.hq_worker_set_timers(None, 1, vp(h), vp(t)) == inval
    assert lib.hq_worker_set_timers(None, 1, None, None) == inval
    assert lib.hq_worker_set_timers(None, 0, None, None) == inval
    assert out.n_ticked == 7 and t["election_tick"][0] == 9     # nothing written
    # no timeout for an election_rtt a config cannot hold
    assert hq.tick_timeout(1, 2, 3, 0, 0) == 0 and hq.tick_timeout(1, 2, 3, 0, 32768) == 0


def test_timeout_equals_the_model(hq):
    rng = np.random.default_rng(20)
    edge = [0, 1, 2, U64 - 1, U64]
    cases = [(s, c, t, st, E) for E in (1, 2, 16, 32767) for s in (0, U64) for c in edge for t in edge
             for st in (0, 1, 2)]
    while len(cases) < 10_000:
        wide = [int(x) for x in rng.integers(0, 1 << 64, 3, dtype=np.uint64)]
        narrow = [int(x) for x in rng.integers(0, 1000, 3)]
        s, c, t = [w if rng.random() < 0.7 else n for w, n in zip(wide, narrow)]
        E = int(rng.choice([1, 2, 3, 10, 16, 1000, 32766, 32767])) if rng.random() < 0.5 else \
            int(rng.integers(1, 32768))
        cases.append((s, c, t, int(rng.integers(0, 3)), E))
    for s, c, t, st, E in cases:
        got = hq.tick_timeout(s, c, t, st, E)
        assert got == tm.timeout(s, c, t, st, E), (s, c, t, st, E)
        assert E <= got < 2 * E


def test_timeout_reaches_every_value(hq):
    """E = 16 over 65 536 consecutive cluster ids (seed 0x5EED, term 3, follower): every value of
    [16, 32) occurs. The counts lie between 4021 and 4147 (4096 expected: -1.8 % .. +1.2 %; a
    binomial's standard deviation here is 62); only presence is asserted, which is a property of
    the mix function, not a tuned number."""
    counts = np.bincount([hq.tick_timeout(0x5EED, c, 3, 0, 16) for c in range(1000, 1000 + 65536)],
                         minlength=32)
    print("timeout counts over [16, 32):", counts[16:].tolist())
    assert counts[:16].sum() == 0 and (counts[16:] > 0).all()


# ------------------------------------------------------------------ hq_tick.h on the CPU ------
TICK_CPP = r"""
// Replays a scenario through hq_tick.h's transition: the timers are a heap array of exactly the
// handles' count, so an access beyond it is the sanitizer's to report.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "hq_tick.h"

int main() {
    unsigned long long n, E, H, cq, seed;
    if (std::scanf("%llu %llu %llu %llu %llu", &n, &E, &H, &cq, &seed) != 5) return 2;
    const hq_tick_params p{(uint32_t)E, (uint32_t)H, (uint32_t)cq, seed};
    std::vector<hq_tick_timer> timers(n, tick_unseen());
    char op;
    unsigned long long h, cid, term, a, b, c;
    unsigned state, flag;
    while (std::scanf(" %c %llu %llu %llu %u %u %llu %llu %llu", &op, &h, &cid, &term, &state, &flag, &a, &b, &c) == 9) {
        if (h >= n) return 3;
        if (op == 't') {                                  // tick: flag = suspended | contact << 1
            const uint32_t bits = tick_step(timers[h], p, cid, term, state, flag & 1, (flag >> 1) & 1);
            std::printf("%u\n", bits);
        } else if (op == 'g') {
            const hq_timer t = tick_public(timers[h], p, cid, term, state);
            std::printf("%u %u %u %u\n", t.election_tick, t.heartbeat_tick, t.randomized_timeout, t.reserved);
        } else if (op == 's') {
            const hq_timer t{(uint32_t)a, (uint32_t)b, (uint32_t)c, 0};
            if (!tick_settable(t, p)) return 4;
            timers[h] = tick_from_public(t, p, cid, term, state);
        } else if (op == 'r') {
            timers[h] = tick_unseen();
        } else if (op == 'v') {                           // is (a, b, c) a settable timer?
            std::printf("%d\n", (int)tick_settable(hq_timer{(uint32_t)a, (uint32_t)b, (uint32_t)c, 0}, p));
        } else {
            return 5;
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def tick_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("tick_ref")
    src, exe = d / "tick_ref.cpp", d / "tick_ref"
    src.write_text(TICK_CPP)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "dragonboat_amd", "csrc"),
                    "-o", str(exe), str(src)], check=True)
    return str(exe)


@pytest.mark.parametrize("E,H,cq", [(1, 1, 1), (2, 1, 0), (3, 2, 1), (5, 3, 1), (32767, 65535, 1)])
def test_shared_transition_equals_the_model(tick_exe, E, H, cq):
    """Random groups that change term and state, get suspended, stopped, re-synced and have their
    timers set, ticked 60 times through hq_tick.h and through the model."""
    rng = np.random.default_rng(100 + E)
    n, seed = 40, int(rng.integers(0, 1 << 64, dtype=np.uint64))
    model = tm.TickModel(E, H, cq, seed)
    groups = [[1000 + h, int(rng.integers(1, 5)), int(rng.integers(0, 3)), False] for h in range(n)]
    groups[7][1] = U64 - 3                                           # a term at the u64 edge
    lines, want = ["%d %d %d %d %d" % (n, E, H, cq, seed)], []

    def line(op, h, flag=0, a=0, b=0, c=0):
        g = groups[h]
        lines.append("%s %d %d %d %d %d %d %d %d" % (op, h, g[0], g[1], g[2], flag, a, b, c))

    for tick in range(60):
        contact = [h for h in range(n) if rng.random() < 0.3]
        cq_l, hb_l, el_l, _ = model.tick([tuple(g) for g in groups], contact)
        for h in range(n):
            line("t", h, int(groups[h][3]) | (h in contact) << 1)
            bits = (h in cq_l) | (h in hb_l) << 1 | (h in el_l) << 2 | (0 if groups[h][3] else 8)
            want.append(str(bits))
        for h in range(n):
            line("g", h)
            want.append("%d %d %d 0" % model.get(h, tuple(groups[h])))
        for h in range(n):                                           # what a step, a fallback, a
            r, g = rng.random(), groups[h]                           # re-sync or a set_timers does
            if r < 0.08 and g[2] != tm.LEADER and g[1] < U64 - 1:
                g[1], g[2] = g[1] + 1, tm.CANDIDATE                  # campaign
            elif r < 0.14 and g[2] == tm.CANDIDATE:
                g[2] = tm.LEADER if rng.random() < 0.5 else tm.FOLLOWER   # a vote outcome
            elif r < 0.18 and g[2] == tm.LEADER:
                g[2] = tm.FOLLOWER                                   # a lost CheckQuorum
            elif r < 0.22 and g[1] < U64 - 1:
                g[1], g[2] = g[1] + 1, tm.FOLLOWER                   # a higher term
            elif r < 0.26:
                g[3] = not g[3]                                      # suspended / handed back
                if not g[3]:
                    model.reset(h)
                    line("r", h)
            elif r < 0.30:
                g[0] += 5000                                         # restarted as another cluster
                model.reset(h)
                line("r", h)
            elif r < 0.36:
                et, ht = int(rng.integers(0, 2 * E)), int(rng.integers(0, H))
                rt = 0 if rng.random() < 0.5 else int(rng.integers(E, 2 * E))
                model.set(h, tuple(g), et, ht, rt)
                line("s", h, 0, et, ht, rt)
    for a, b, c, ok in ((2 * E - 1, H - 1, 0, 1), (2 * E, 0, 0, 0), (0, H, 0, 0), (0, 0, E, 1),
                        (0, 0, 2 * E - 1, 1), (0, 0, 2 * E, 0), (0, 0, E - 1, E == 1)):
        line("v", 0, 0, a, b, c)           # (E - 1 = 0 for E = 1: "draw by the formula")
        want.append(str(int(ok)))
    r = subprocess.run([tick_exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    bad = [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, bad[:5]
    assert model.resets > 20


# ------------------------------------------------------------------ the GPU tests' seeds ------
@pytest.mark.parametrize("cq", [1, 0])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("E", [2, 5])
@pytest.mark.parametrize("G", [17, 300])
def test_random_world_seeds_show_every_reset(hq, G, E, H, cq):
    """The random worlds of test_gpu_tick.py on the oracle and the model alone (no worker): each
    must list every kind of due group and reset timers after a vote outcome, a lost CheckQuorum
    and a higher term."""
    tw.check_seen(tw.run(hq, {}, {}, G, E, H, cq), cq)
