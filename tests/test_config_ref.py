"""Membership changes without a GPU: the Python restatement (tests/config_ref.py) against the
reference's tables (tests/golden/config_change_kats.json), and the bitmap remaps and position
arithmetic of dragonboat_amd/csrc/hq_config.h — the one source the host worker, the device kernel
and this check share — compiled into a program of its own with -fsanitize=address,undefined and
checked exhaustively against a naive list model. No Python process loads sanitized code."""
import os
import subprocess

import pytest

import config_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kat_group(case):
    g = dict(case["group"])
    g["members"] = [{"node_id": i, "match": m, "role": r, "active": a} for i, m, r, a in g["members"]]
    g["reads"] = []
    g["suspended"] = 0
    return g


@pytest.mark.parametrize("case", ref.kats(), ids=lambda c: c["name"])
def test_restatement_against_reference_tables(case):
    g = kat_group(case)
    for step in case["steps"]:
        change = (0, step["type"], step["node_id"])
        if step.get("inval"):
            assert ref.invalid({0: g}, [change])
            assert ref.member_tuples(g) == [tuple(m) for m in step["members"]]
            continue
        assert not ref.invalid({0: g}, [change])
        status, g, commit = ref.apply(g, step["type"], step["node_id"], n_max=8, member_limit=16)
        assert (status, commit) == (step["status"], step["commit"]), step
        assert ref.member_tuples(g) == [tuple(m) for m in step["members"]], step
        assert g["suspended"] == step.get("suspended", 0)
        if commit is not None:
            assert g["committed"] == commit


def test_restatement_rules():
    """The worker's own rules: list order, the fallbacks, what the whole list is refused for."""
    g = {"node_id": 1, "state": ref.LEADER, "committed": 5, "last_index": 9, "term_start": 4,
         "suspended": 0, "reads": [],
         "members": [{"node_id": i, "match": m, "role": r, "active": 0}
                     for i, m, r in ((4, 6, 1), (1, 9, 0), (2, 7, 0), (3, 5, 2))]}
    # a removed member's successors move down; the smaller quorum commits (1: 9, 3: 5 -> 5; no)
    s, a, c = ref.apply(g, ref.REMOVE_NODE, 2, 8, 16)
    assert (s, c, [m["node_id"] for m in a["members"]]) == (ref.APPLIED, None, [4, 1, 3])
    s, a, c = ref.apply(g, ref.REMOVE_NODE, 3, 8, 16)
    assert (s, c, a["committed"]) == (ref.APPLIED, 7, 7)
    # a non-member: nothing deleted, tryCommit all the same (9, 7, 5: the second largest is 7)
    assert ref.apply(g, ref.REMOVE_NODE, 9, 8, 16)[::2] == (ref.NOOP, 7)
    # new members go to the end; a promoted observer stays where it is
    s, a, _ = ref.apply(g, ref.ADD_WITNESS, 7, 8, 16)
    assert ref.member_tuples(a)[-1] == (7, 0, ref.WITNESS, 0) and len(a["members"]) == 5
    s, a, _ = ref.apply(g, ref.ADD_NODE, 4, 8, 16)
    assert ref.member_tuples(a)[0] == (4, 6, ref.REMOTE, 0)
    # fallbacks: (a) voting / member limits, (b) the node itself, (c) a recorded vote or ack
    assert ref.apply(g, ref.ADD_NODE, 7, 3, 16)[0] == ref.FALLBACK
    assert ref.apply(g, ref.ADD_NODE, 4, 3, 16)[0] == ref.FALLBACK
    assert ref.apply(g, ref.ADD_OBSERVER, 7, 3, 4)[0] == ref.FALLBACK
    assert ref.apply(g, ref.ADD_OBSERVER, 7, 3, 5)[0] == ref.APPLIED
    assert ref.apply(g, ref.REMOVE_NODE, 1, 8, 16)[0] == ref.FALLBACK
    s, a, _ = ref.apply(g, ref.REMOVE_NODE, 2, 8, 16, acked={2})
    assert s == ref.FALLBACK and a["suspended"] == 1 and ref.member_tuples(a) == ref.member_tuples(g)
    assert ref.apply(g, ref.REMOVE_NODE, 4, 8, 16, acked={4})[0] == ref.APPLIED   # an observer
    assert ref.apply(a, ref.ADD_NODE, 7, 8, 16)[0] == ref.SUSPENDED
    # the whole list refused
    gs = {0: g, 1: g}
    assert not ref.invalid(gs, [(0, ref.ADD_NODE, 7), (1, ref.REMOVE_NODE, 2)])
    for bad in ([(2, ref.ADD_NODE, 7)], [(0, ref.ADD_NODE, 7), (0, ref.REMOVE_NODE, 2)],
                [(0, 4, 7)], [(0, ref.ADD_NODE, 0)], [(0, ref.ADD_NODE, 3)],
                [(0, ref.ADD_OBSERVER, 2)], [(0, ref.ADD_WITNESS, 4)], [(0, ref.ADD_WITNESS, 2)]):
        assert ref.invalid(gs, bad), bad
    # routes follow the list
    row = list(range(16))
    assert ref.routes_after(row, g, ref.REMOVE_NODE, 1, ref.APPLIED) == \
        [0, 2, 3, ref.ROUTE_NONE] + list(range(4, 16))
    assert ref.routes_after(row, g, ref.ADD_NODE, 7, ref.APPLIED) == \
        [0, 1, 2, 3, ref.ROUTE_NONE] + list(range(5, 16))
    assert ref.routes_after(row, g, ref.ADD_NODE, 4, ref.APPLIED) == row
    assert ref.routes_after(row, g, ref.REMOVE_NODE, 2, ref.FALLBACK) == row


SWEEP_CPP = r"""
// Every role layout of up to 8 voting members and up to 16 members, every removable, insertable
// and promotable position, every 8-bit bitmap: hq_config.h against a naive list model. The lists
// are heap vectors of exactly their size, so a position out of range is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hq_config.h"

struct M { int id, role; };
static unsigned long long checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { std::printf("FAILED %s line %d\n", #c, __LINE__); std::exit(1); } } while (0)

// the naive model: a member's class in pool order
static int cls(int role) { return role == HQ_ROLE_REMOTE ? 0 : role == HQ_ROLE_WITNESS ? 1 : 2; }
static std::vector<M> naive_insert(const std::vector<M> &l, M m) {
    std::vector<M> out;
    bool done = false;
    for (const M &x : l) {
        if (!done && cls(x.role) > cls(m.role)) { out.push_back(m); done = true; }
        out.push_back(x);
    }
    if (!done) out.push_back(m);
    return out;
}
static int find(const std::vector<M> &l, int id) {
    for (size_t i = 0; i < l.size(); ++i) if (l[i].id == id) return (int)i;
    return -1;
}
static unsigned n_voting(const std::vector<M> &l) {
    unsigned n = 0;
    for (const M &x : l) n += x.role != HQ_ROLE_OBSERVER;
    return n;
}
// a slot bitmap carried over by member identity: bit of old slot t goes to the member's new slot
static unsigned naive_bits(unsigned b, const std::vector<M> &before, const std::vector<M> &after) {
    unsigned out = 0;
    const unsigned nb = n_voting(before);
    for (unsigned t = 0; t < 8; ++t) {
        if (!((b >> t) & 1)) continue;
        if (t >= nb) continue;                       // not a member's bit
        const int p = find(after, before[t].id);
        if (p >= 0 && (unsigned)p < n_voting(after)) out |= 1u << p;
    }
    return out;
}

int main() {
    for (unsigned nr = 1; nr <= 8; ++nr)
        for (unsigned nw = 0; nr + nw <= 8; ++nw)
            for (unsigned no = 0; nr + nw + no <= 16; ++no) {
                std::vector<M> l;
                int id = 1;
                for (unsigned i = 0; i < nr; ++i) l.push_back({id++, (int)HQ_ROLE_REMOTE});
                for (unsigned i = 0; i < nw; ++i) l.push_back({id++, (int)HQ_ROLE_WITNESS});
                for (unsigned i = 0; i < no; ++i) l.push_back({id++, (int)HQ_ROLE_OBSERVER});
                const unsigned n = (unsigned)l.size(), nv = nr + nw;
                const hq_cfg_layout lay{nr, nv, n};
                const unsigned mask = cfg_low(nv);
                // removal of every member but the node itself
                for (unsigned src = 1; src < n; ++src) {
                    std::vector<M> after(l);
                    after.erase(after.begin() + src);
                    std::vector<int> placed(n - 1, 0);
                    for (unsigned j = 0; j < n; ++j) {
                        if (j == src) continue;
                        const unsigned p = cfg_pos_after_remove(j, src);
                        CHECK(p == (unsigned)find(after, l[j].id));
                        placed[p] = l[j].id;
                    }
                    for (unsigned j = 0; j + 1 < n; ++j) CHECK(placed[j] == after[j].id);
                    const unsigned slot = cfg_remove_slot(src, lay);
                    CHECK((slot == kCfgNoSlot) == (l[src].role == (int)HQ_ROLE_OBSERVER));
                    if (slot == kCfgNoSlot) continue;
                    CHECK(slot == src);
                    for (unsigned b = 0; b < 256; ++b) {
                        const unsigned got = cfg_remove_bit(b, slot);
                        CHECK(got <= 0xFF);
                        CHECK((got & cfg_low(nv - 1)) == naive_bits(b & mask & ~(1u << slot), l, after));
                        // the bits above the voting slots move as slots would: none is made up
                        CHECK(__builtin_popcount(got) == __builtin_popcount(b & ~(1u << slot)));
                    }
                }
                // a new member of each kind
                for (unsigned type : {HQ_CC_ADD_NODE, HQ_CC_ADD_OBSERVER, HQ_CC_ADD_WITNESS}) {
                    const int role = type == HQ_CC_ADD_NODE ? HQ_ROLE_REMOTE
                                     : type == HQ_CC_ADD_WITNESS ? HQ_ROLE_WITNESS : HQ_ROLE_OBSERVER;
                    if (n == 16 || (role != (int)HQ_ROLE_OBSERVER && nv == 8)) continue;
                    const std::vector<M> after = naive_insert(l, M{99, role});
                    const unsigned dst = cfg_insert_pos(type, lay);
                    CHECK(dst == (unsigned)find(after, 99));
                    std::vector<int> placed(n + 1, 0);
                    placed[dst] = 99;
                    for (unsigned j = 0; j < n; ++j) {
                        const unsigned p = cfg_pos_after_insert(j, dst);
                        CHECK(p == (unsigned)find(after, l[j].id));
                        placed[p] = l[j].id;
                    }
                    for (unsigned j = 0; j <= n; ++j) CHECK(placed[j] == after[j].id);
                    const unsigned slot = cfg_insert_slot(type, lay);
                    CHECK((slot == kCfgNoSlot) == (role == (int)HQ_ROLE_OBSERVER));
                    if (slot == kCfgNoSlot) continue;
                    CHECK(slot == dst);
                    for (unsigned b = 0; b < 256; ++b) {
                        const unsigned got = cfg_insert_bit(b, slot);
                        CHECK(!((got >> slot) & 1));
                        CHECK((got & cfg_low(nv + 1)) == naive_bits(b & mask, l, after));
                        CHECK(cfg_remove_bit(got, slot) == b);      // the two are inverses
                    }
                }
                // promotion of every observer
                for (unsigned src = nv; src < n && nv < 8; ++src) {
                    std::vector<M> rest(l);
                    rest.erase(rest.begin() + src);
                    const std::vector<M> after = naive_insert(rest, M{l[src].id, (int)HQ_ROLE_REMOTE});
                    const unsigned dst = cfg_promote_pos(lay);
                    CHECK(dst == (unsigned)find(after, l[src].id));
                    std::vector<int> placed(n, 0);
                    for (unsigned j = 0; j < n; ++j) {
                        const unsigned p = cfg_pos_after_promote(j, src, dst);
                        CHECK(p == (unsigned)find(after, l[j].id));
                        placed[p] = l[j].id;
                    }
                    for (unsigned j = 0; j < n; ++j) CHECK(placed[j] == after[j].id);
                    for (unsigned b = 0; b < 256; ++b)
                        CHECK((cfg_insert_bit(b, dst) & cfg_low(nv + 1)) == naive_bits(b & mask, l, after));
                }
                // list positions close the gap of a removal
                for (unsigned removed = 0; removed < n; ++removed)
                    for (unsigned o = 0; o < n; ++o) {
                        if (o == removed) continue;
                        unsigned rank = 0;
                        for (unsigned x = 0; x < o; ++x) rank += x != removed;
                        CHECK(cfg_order_after_remove(o, removed) == rank);
                    }
            }
    std::printf("ok %llu\n", checks);
    return 0;
}
"""


@pytest.fixture(scope="module")
def sweep_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("config_change")
    src, exe = d / "config_sweep.cpp", d / "config_sweep"
    src.write_text(SWEEP_CPP)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "dragonboat_amd", "csrc"), "-o", str(exe), str(src)],
                   check=True)
    return str(exe)


def test_sanitizer_remaps_and_positions_stand_alone(sweep_program):
    r = subprocess.run([sweep_program], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "" and r.stdout.startswith("ok ")
    assert int(r.stdout.split()[1]) >= 1000000
