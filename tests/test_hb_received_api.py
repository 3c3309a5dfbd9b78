"""The received-heartbeat entries of the ABI without a device (include/hipquorum.h "heartbeats
received"): the header declares them, the built library exports them, the refusals that need no
worker, hq_heartbeat_replies_expand against the model of hb_received_model.py and through
hq_wire_encode_batch -> hq_wire_decode_batch, the per-message transition of
dragonboat_amd/csrc/hq_hb_received.h (the source the host worker and the kernel share) compiled
into a program of its own with -fsanitize=address,undefined and replayed against the model, and
the seeds of the GPU tests, which must reach every branch on the model alone. No Python process
loads sanitized code."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import hb_received_model as hm
import hb_received_world as hw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hipquorum.h")
ENTRIES = ("hq_worker_heartbeats_received", "hq_heartbeat_replies_expand")
U64 = (1 << 64) - 1


def header_text():
    s = open(HEADER).read()
    return " ".join(re.sub(r"/\*.*?\*/", " ", s, flags=re.S).split())


def struct_body(s, name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), s)
    assert m, name
    return " ".join(m.group(1).split())


def test_header_declares_the_entries_and_the_structs():
    s = header_text()
    assert ("int hq_worker_heartbeats_received(hq_worker *w, const hq_hb_received_input *in, "
            "hq_hb_received_output *out);") in s
    assert ("int hq_heartbeat_replies_expand(const hq_hb_received_input *in, const hq_hb_received_output *out, "
            "const uint64_t *cluster_id, const uint64_t *node_id, hq_wire_message *msgs, uint64_t cap, "
            "uint64_t *n);") in s
    assert struct_body(s, "hq_hb_received") == "uint64_t from, term, commit, hint, hint_high;"
    assert struct_body(s, "hq_hb_received_input") == (
        "uint64_t n_groups; const uint32_t *groups; const uint64_t *offsets; const hq_hb_received *msgs; "
        "uint32_t check_quorum; uint32_t reserved;")
    assert struct_body(s, "hq_hb_reply") == "uint64_t term; uint32_t type; uint32_t reserved;"
    assert struct_body(s, "hq_hb_group_result") == (
        "uint64_t term; uint64_t commit; uint64_t leader; uint32_t state; uint16_t flags, n_resets;")
    assert struct_body(s, "hq_hb_received_output") == (
        "const hq_hb_reply *replies; uint64_t n_msgs; const hq_hb_group_result *results; uint64_t n_groups; "
        "uint64_t n_resp, n_noop, n_contact, n_committed, n_state_changed, n_suspended; uint64_t gpu_ns;")
    for name, value in (("HQ_MSG_NOOP", 4), ("HQ_HBR_COMMITTED", 1), ("HQ_HBR_COMMIT_ABOVE_LAST", 2),
                        ("HQ_HBR_CONTACT", 4), ("HQ_HBR_SUSPENDED", 8)):
        assert re.search(r"#define %s %du\b" % (name, value), s), name
    assert re.search(r"#define HQ_ABI_VERSION 21u?\b", s)      # new symbols only: still ABI 21


def test_library_exports_them_and_the_binding_lists_them(hq):
    for name in ENTRIES:
        assert getattr(hq.lib, name) is not None
        assert name in hq.SIGNATURES
        assert hq.SIGNATURES[name][0] is ctypes.c_int
    assert hq.HB_RECEIVED_DTYPE.names == ("from", "term", "commit", "hint", "hint_high")
    assert hq.HB_REPLY_DTYPE.names == ("term", "type", "reserved")
    assert hq.HB_GROUP_RESULT_DTYPE.names == ("term", "commit", "leader", "state", "flags", "n_resets")
    assert (hq.HB_RECEIVED_DTYPE.itemsize, hq.HB_REPLY_DTYPE.itemsize, hq.HB_GROUP_RESULT_DTYPE.itemsize) == \
        (40, 16, 32)
    assert (hq.HQ_MSG_NOOP, hq.HQ_HBR_COMMITTED, hq.HQ_HBR_COMMIT_ABOVE_LAST, hq.HQ_HBR_CONTACT,
            hq.HQ_HBR_SUSPENDED) == (hm.MSG_NOOP, hm.COMMITTED, hm.COMMIT_ABOVE_LAST, hm.CONTACT, hm.SUSPENDED)
    assert callable(hq.Worker.heartbeats_received) and callable(hq.heartbeat_replies_expand)


LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "hipquorum.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(hq_hb_received), sizeof(hq_hb_reply),
         sizeof(hq_hb_group_result), sizeof(hq_hb_received_input), sizeof(hq_hb_received_output),
         offsetof(hq_hb_group_result, flags), offsetof(hq_hb_received_input, check_quorum),
         offsetof(hq_hb_received_output, gpu_ns));
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
    assert [int(x) for x in out] == [40, 16, 32, 40, 88, 28, 32, 80]


def test_refusals_without_a_worker(hq):
    """A NULL worker is HQ_E_INVAL whatever else is passed, and nothing is written."""
    lib, inval = hq.lib, hq.HQ_E_INVAL
    inp, keep = hq.hb_received_input(np.array([0], np.uint32), np.array([0, 1], np.uint64),
                                     np.array([(2, 3, 4, 0, 0)], hq.HB_RECEIVED_DTYPE))
    out = hq.HbReceivedOutput()
    out.n_resp = 7
    assert lib.hq_worker_heartbeats_received(None, ctypes.byref(inp), ctypes.byref(out)) == inval
    assert lib.hq_worker_heartbeats_received(None, None, ctypes.byref(out)) == inval
    assert lib.hq_worker_heartbeats_received(None, ctypes.byref(inp), None) == inval
    assert out.n_resp == 7 and out.replies is None
    # the stateless expansion's own refusals: *n is always set
    n = ctypes.c_uint64(9)
    wire = np.zeros(4, hq.WIRE_MESSAGE_DTYPE)
    ids = np.array([5], np.uint64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.hq_heartbeat_replies_expand(None, ctypes.byref(out), vp(ids), vp(ids), vp(wire), 4,
                                           ctypes.byref(n)) == inval and n.value == 0
    n.value = 9
    assert lib.hq_heartbeat_replies_expand(ctypes.byref(inp), None, vp(ids), vp(ids), vp(wire), 4,
                                           ctypes.byref(n)) == inval and n.value == 0
    assert lib.hq_heartbeat_replies_expand(ctypes.byref(inp), ctypes.byref(out), vp(ids), vp(ids), vp(wire), 4,
                                           None) == inval
    n.value = 9                       # the output is not this input's (0 groups against 1)
    assert lib.hq_heartbeat_replies_expand(ctypes.byref(inp), ctypes.byref(out), vp(ids), vp(ids), vp(wire), 4,
                                           ctypes.byref(n)) == inval and n.value == 0
    assert not wire.view(np.uint8).any()


def random_call(rng, G, u64=False):
    """G groups with 0 .. 4 messages each on the model: (rows, replies, results, cluster ids, node ids)."""
    rows, replies, results, cids, nids = [], [], [], [], []
    for i in range(G):
        term = int(rng.integers(2, 9))
        last = int(rng.integers(50, 100))
        g = {"term": term, "state": int(rng.integers(0, 3)), "committed": last - int(rng.integers(0, 9)),
             "last": last, "suspended": rng.random() < 0.1}
        msgs = hm.random_messages(rng, g)
        rep, res, _ = hm.handle(g, msgs, True)
        rows.append(msgs)
        replies += rep
        results.append(res)
        cids.append(int(rng.integers(1, 1 << 64, dtype=np.uint64)) if u64 else 1000 + i)
        nids.append(int(rng.integers(1, 64)))
    return rows, replies, results, cids, nids


def call_arrays(hq, rows, replies, results):
    groups = np.arange(len(rows), dtype=np.uint32)
    offsets = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    msgs = np.array([m for r in rows for m in r], hq.HB_RECEIVED_DTYPE)
    rep = np.array([(t, ty, 0) for ty, t in replies], hq.HB_REPLY_DTYPE)
    rs = np.array([(r["term"], r["commit"], r["leader"], r["state"], r["flags"], r["n_resets"])
                   for r in results], hq.HB_GROUP_RESULT_DTYPE)
    return groups, offsets, msgs, {"replies": rep, "results": rs}


@pytest.mark.parametrize("G", [0, 1, 40])
def test_expand_equals_the_model_and_survives_the_wire(hq, G):
    rng = np.random.default_rng(300 + G)
    rows, replies, results, cids, nids = random_call(rng, G, u64=True)
    groups, offsets, msgs, res = call_arrays(hq, rows, replies, results)
    wire = hq.heartbeat_replies_expand(groups, offsets, msgs, res, cids, nids)
    want = hm.expand(rows, replies, cids, nids)
    assert len(wire) == len(want) and (G == 0 or len(want) > 0 or G == 1)

    def fields(m):
        return {"kind": int(m["ev"]["kind"]), "type": int(m["ev"]["type"]), "from": int(m["ev"]["from"]),
                "to": int(m["to"]), "cluster_id": int(m["cluster_id"]), "term": int(m["ev"]["term"]),
                "hint": int(m["ev"]["hint"]), "hint_high": int(m["ev"]["hint_high"])}

    def rest_is_zero(m, decoded=False):
        # (a marshalled Message always carries its non-nullable Snapshot field: the decoder sees it)
        return (int(m["ev"]["log_index"]), int(m["ev"]["reject"]), int(m["ev"]["reserved"]), int(m["log_term"]),
                int(m["commit"]), int(m["n_entries"]), int(m["has_snapshot"])) == (0,) * 6 + (int(decoded),)

    for m, w in zip(wire, want):
        assert fields(m) == w and rest_is_zero(m)
    # through the wire: every field comes back
    if want:
        data = hq.encode_wire_batch(wire, deployment_id=0x5EED, source_address=b"n1:1")
        back, info = hq.decode_batch(data.tobytes())
        assert info.n_messages == len(want) and info.deployment_id == 0x5EED
        for m, w in zip(back, want):
            assert fields(m) == w and rest_is_zero(m, decoded=True)
    # a short buffer: HQ_E_STATE, the count needed, nothing written
    if want:
        with pytest.raises(hq.HQError) as e:
            hq.heartbeat_replies_expand(groups, offsets, msgs, res, cids, nids, cap=len(want) - 1)
        assert e.value.code == hq.HQ_E_STATE and e.value.n == len(want)


# ------------------------------------------------------------- hq_hb_received.h on the CPU ------
REPLAY_CPP = r"""
// Replays received heartbeats through hq_hb_received.h's transition: the groups and the replies are
// heap arrays of exactly the input's counts, so an access beyond them is the sanitizer's to report.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "hq_hb_received.h"

int main() {
    unsigned long long G, cq;
    if (std::scanf("%llu %llu", &G, &cq) != 2) return 2;
    std::vector<hq_hbr_group> groups(G);
    for (unsigned long long i = 0; i < G; ++i) {
        unsigned long long term, committed, last, k;
        unsigned state, suspended;
        if (std::scanf("%llu %u %llu %llu %u %llu", &term, &state, &committed, &last, &suspended, &k) != 6) return 3;
        groups[i] = hq_hbr_group{term, committed, last, state, false};
        hq_hbr_acc a{0, 0, 0, 0};
        std::vector<hq_hb_reply> replies(k);
        for (unsigned long long m = 0; m < k; ++m) {
            unsigned long long from, t, commit, hint, high;
            if (std::scanf("%llu %llu %llu %llu %llu", &from, &t, &commit, &hint, &high) != 5) return 4;
            if (suspended) {
                replies[m] = hq_hb_reply{0, 0, 0};
                continue;
            }
            const uint32_t type = hbr_message(groups[i], a, hq_hb_received{from, t, commit, hint, high}, (uint32_t)cq);
            replies[m] = hq_hb_reply{type ? groups[i].term : 0, type, 0};
        }
        if (suspended) a.flags = HQ_HBR_SUSPENDED;
        for (const hq_hb_reply &r : replies) std::printf("r %u %" PRIu64 "\n", r.type, r.term);
        const hq_hbr_group &g = groups[i];
        std::printf("g %" PRIu64 " %u %" PRIu64 " %d %" PRIu64 " %" PRIu64 " %u %u\n", g.term, g.state, g.committed,
                    (int)g.reset, a.commit, a.leader, a.flags, a.n_resets);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def replay_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("hb_received_ref")
    src, exe = d / "replay.cpp", d / "replay"
    src.write_text(REPLAY_CPP)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "dragonboat_amd", "csrc"),
                    "-o", str(exe), str(src)], check=True)
    return str(exe)


@pytest.mark.parametrize("cq", [1, 0])
@pytest.mark.parametrize("shift", [0, (1 << 32) - 4, (1 << 63) - 4, U64 - 110])
def test_shared_transition_equals_the_model(replay_exe, cq, shift):
    """Random rows (terms below, at and above the group's and 0; all three states; commits below,
    at and above committed and last; 0 .. 4 messages per group) through hq_hb_received.h and the
    model, the terms and indexes also shifted to the u64 edges."""
    rng = np.random.default_rng(500 + cq + shift % 1000)
    G = 400
    seen = hm.Seen()
    lines, want = ["%d %d" % (G, cq)], []
    for i in range(G):
        term = shift + int(rng.integers(2, 6))
        last = shift + int(rng.integers(50, 100))
        g = {"term": term, "state": int(rng.integers(0, 3)), "committed": last - int(rng.integers(0, 9)),
             "last": last, "suspended": rng.random() < 0.05}
        msgs = hm.random_messages(rng, g, u64=True)
        replies, res, after = hm.handle(g, msgs, cq)
        seen.add(g, replies, res)
        lines.append("%d %d %d %d %d %d" % (g["term"], g["state"], g["committed"], g["last"], g["suspended"],
                                            len(msgs)))
        lines += ["%d %d %d %d %d" % m for m in msgs]
        want += ["r %d %d" % r for r in replies]
        want.append("g %d %d %d %d %d %d %d %d" % (after["term"], after["state"], after["committed"],
                                                    after["reset"], res["commit"], res["leader"], res["flags"],
                                                    res["n_resets"]))
    seen.check(suspended=True, noop=bool(cq))
    r = subprocess.run([replay_exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    bad = [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, bad[:5]


# ------------------------------------------------------------------ the GPU tests' seeds ------
@pytest.mark.parametrize("cq", [1, 0])
@pytest.mark.parametrize("G", [17, 300])
def test_random_world_seeds_reach_every_branch(hq, G, cq):
    """The random worlds of test_gpu_hb_received.py on the oracle and the models alone (no worker):
    each must produce every reply type, every flag, n_resets of 0, 1 and 2, a leader demoted by a
    higher term and a candidate that becomes a follower and then meets a higher term; and its
    election lists must differ from the same world's without the received call."""
    seen, elections = hw.run(hq, {}, {}, G, cq)
    seen.check(noop=bool(cq))
    _, without = hw.run(hq, {}, {}, G, cq, received=False)
    assert elections != without


@pytest.mark.parametrize("G", [1, 31, 32, 33, 63, 64, 65, 257, 1025])
def test_edge_rows_reach_every_branch(G):
    """The listed-group edges of test_gpu_hb_received.py: the rows over all sizes together."""
    seen = hm.Seen()
    for size in hw.EDGE_SIZES:
        specs, rows = hw.edge_rows(size)
        for s, msgs in zip(specs, rows):
            g = hw.spec_group(s)
            replies, res, _ = hm.handle(g, msgs, True)
            seen.add(g, replies, res)
    seen.check()
    specs, rows = hw.edge_rows(G)
    assert len(specs) == G and any(len(r) == 0 for r in rows) or G == 1
