"""hq_wire_codec.h (dragonboat_amd/csrc; host code, no GPU): the one reader of raftpb.Message that
the host decoder and the decode kernels share. The host decoder (hq_wire_decode_batch) must equal
the referee (wire_decode_ref.py) on every message of wire_cases.py — the same accept / reject
decision and, where accepted, the same fields — so that the device tests, which compare the kernel
with the host decoder on the same messages, stand on the referee. A stand-alone C++ program built
with the address and undefined-behaviour sanitizers runs the header's decode_message in the
kernels' two instantiations (32- and 64-bit positions) and the header hop over exactly sized heap
buffers. The words of hq_wire_last_error are pinned."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import wire_cases
import wire_decode_ref as ref
import wire_encode as we

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_decode_one(hq, body):
    """(rejected, record) of the host decoder for the one-message batch holding `body`."""
    data = np.frombuffer(we.f_bytes(1, bytes(body)), np.uint8)
    out = np.zeros(1, hq.WIRE_MESSAGE_DTYPE)
    n = ctypes.c_uint64(0)
    rc = hq.lib.hq_wire_decode_batch(hq._p(data), len(data), hq._p(out), 1, ctypes.byref(n), None)
    assert rc in (hq.HQ_OK, hq.HQ_E_INVAL)
    return rc != hq.HQ_OK, out[0]


def test_parity_messages_equal_the_referee(hq):
    msgs = wire_cases.parity_messages()
    assert len(msgs) == 4000
    want = np.array([ref.as_record(hq, ref.decode_message(m)) for m in msgs], hq.WIRE_MESSAGE_DTYPE)
    got, info = hq.decode_batch(we.batch(msgs, deployment_id=7))
    assert info.n_messages == len(msgs)
    for f in ("cluster_id", "to", "log_term", "commit", "n_entries", "has_snapshot"):
        np.testing.assert_array_equal(got[f], want[f])
    for f in hq.EVENT_DTYPE.names:
        np.testing.assert_array_equal(got["ev"][f], want["ev"][f])
    assert got.tobytes() == want.tobytes()
    # the cases are what they claim: both encodings, entries, snapshots present and absent
    assert set(want["n_entries"]) == {0, 1} and set(want["has_snapshot"]) == {0, 1}


def test_rejection_slices_equal_the_referee(hq):
    slices, owner, n_fixtures = wire_cases.rejection_slices()
    host = [host_decode_one(hq, s) for s in slices]
    rejected = np.array([r for r, _ in host])
    assert list(rejected) == [ref.rejected(s) for s in slices]
    for k in range(0, n_fixtures, 2):       # both outcomes for every fixture's message
        mine = rejected[np.array(owner) == k]
        assert mine.any() and not mine.all(), k
    for s, (bad, got) in zip(slices, host):
        if not bad:
            assert got.tobytes() == ref.as_record(hq, ref.decode_message(s)).tobytes(), s.hex()


# hq_wire_last_error after hq_wire_add_batch, as the library worded it before the reader became
# a header (the header reports a code, hq_wire.cpp the words)
PREFIX = "hq_wire_add_batch: malformed MessageBatch"
MALFORMED_FIXTURE_ERRORS = {
    "message_longer_than_batch": "",
    "truncated_varint_in_message": ": Message: unexpected end of data in a varint",
    "known_field_wrong_wire_type": ": Message: wrong wire type 2 for field 1",
    "group_wire_type": ": Message: wrong wire type 7 for field 1",
    "varint_overflow": "",
}
OTHER_ERRORS = [
    ("0a020000", ": Message: illegal field number 0"),
    ("0a0c08ffffffffffffffffffff01", ": Message: varint overflows 64 bits"),
    ("0a0bffffffffffffffffffff01", ": Message: varint overflows 64 bits"),
    ("0a035a0500", ": Message: unexpected end of data in a length-delimited field"),
    ("0a026000", ": Message: wrong wire type 0 for field 12"),
    ("0a03790000", ": Message: unexpected end of data in a field"),
    ("0a037a0500", ": Message: unexpected end of data in a field"),
    ("0a027880", ": Message: unexpected end of data in a varint"),
    ("0a056d00000000", ": Message: wrong wire type 5 for field 13"),
    ("0a027b00", ": Message: unsupported wire type (groups are not part of raft.proto)"),
    ("0000", ""),
    ("1200", ""),
]


def test_error_strings(hq):
    cases = [(fx["hex"], MALFORMED_FIXTURE_ERRORS[fx["name"]]) for fx in wire_cases.FIX["malformed"]]
    assert len(cases) == len(MALFORMED_FIXTURE_ERRORS) == 5
    w = hq.Wire(0)
    try:
        for hexed, words in cases + OTHER_ERRORS:
            with pytest.raises(hq.HQError) as e:
                w.add_batch(bytes.fromhex(hexed))
            assert e.value.code == hq.HQ_E_INVAL
            assert hq.lib.hq_wire_last_error(w.h).decode() == PREFIX + words, hexed
    finally:
        w.close()


SANITIZER_MAIN = r"""
#include <cstdio>
#include <cstring>
#include "hq_wire_codec.h"
%(tables)s
struct Out {
    bool ok;
    hq_wire_message m;
    hqw::error e;
};
// decode_message over a heap copy of exactly len bytes, in the kernels' two instantiations
template <class I>
static Out decode(const uint8_t *src, size_t len) {
    uint8_t *b = new uint8_t[len ? len : 1];
    if (len) memcpy(b, src, len);
    Out o;
    memset(&o, 0, sizeof o);
    o.ok = hqw::decode_message<I>(b, (I)len, o.m, o.e);
    delete[] b;
    return o;
}
// 0 accepted, 1 rejected, 2+ a result that is neither or on which the instantiations differ
static int status(const uint8_t *src, size_t len) {
    const Out a = decode<uint32_t>(src, len), b = decode<uint64_t>(src, len);
    if (a.ok != b.ok || memcmp(&a.e, &b.e, sizeof a.e)) return 2;
    if (a.ok != (a.e.code == hqw::kOk) || a.e.code > hqw::kBytesEnd) return 3;
    if (a.ok && memcmp(&a.m, &b.m, sizeof a.m)) return 4;
    return a.ok ? 0 : 1;
}
// the header hop over a heap copy: 0 a `requests` header within the bytes, 1 not one
template <class I>
static int hop(const uint8_t *src, size_t len, uint64_t *pos, uint64_t *n) {
    uint8_t *b = new uint8_t[len ? len : 1];
    if (len) memcpy(b, src, len);
    I p = 0;
    const bool ok = hqw::header<I>(b, p, (I)len, *n);
    *pos = p;
    delete[] b;
    return ok ? 0 : 1;
}
static int hop_status(const uint8_t *src, size_t len) {
    uint64_t p32, n32, p64, n64;
    const int a = hop<uint32_t>(src, len, &p32, &n32), b = hop<uint64_t>(src, len, &p64, &n64);
    if (a != b || p32 != p64) return 2;
    if (a == 0 && (n32 != n64 || p32 > len || n32 > len - p32)) return 3;
    return a;
}
template <class F>
static int sweep(const char *what, const uint8_t *m, size_t len, const int8_t *truncated, F f,
                 unsigned *runs) {
    for (size_t n = 0; n <= len; ++n) {
        const int s = f(m, n);
        if (s != truncated[n]) return printf("%%s: truncation %%zu: %%d, expected %%d\n", what, n, s, (int)truncated[n]), 1;
    }
    uint8_t *b = new uint8_t[len ? len : 1];
    memcpy(b, m, len);
    for (size_t i = 0; i < len; ++i) {
        const uint8_t keep = b[i];
        for (unsigned v = 0; v < 256; ++v) {
            b[i] = (uint8_t)v;
            const int s = f(b, len);
            if (s != 0 && s != 1) return printf("%%s: byte %%zu = %%u: %%d\n", what, i, v, s), 1;
            ++*runs;
        }
        b[i] = keep;
    }
    delete[] b;
    return 0;
}
int main() {
    unsigned runs = 0;
    for (unsigned k = 0; k < sizeof kMessages / sizeof *kMessages; ++k) {
        if (sweep("decode", kMessages[k].p, kMessages[k].n, kMessages[k].truncated, status, &runs)) return 1;
        if (sweep("hop", kMessages[k].p, kMessages[k].n, kMessages[k].hop, hop_status, &runs)) return 1;
    }
    printf("ok %%u\n", runs);
    return 0;
}
"""


def hop_status(b):
    """The referee of the header hop: 0 when b starts with a `requests` header (field 1, length
    delimited) whose body lies within b, else 1."""
    try:
        tag, p = ref.read_varint(b, 0)
        if (tag >> 3) & 0xFFFFFFFF != 1 or tag & 7 != 2:
            return 1
        ref.read_length(b, p)
        return 0
    except ref.Rejected:
        return 1


def test_sanitizer_sweeps_stand_alone(tmp_path):
    """The header alone compiled into a program of its own with -fsanitize=address,undefined:
    every truncation (statuses as the referee gives them) and every single-byte replacement of
    every fixture message and of every fixture taken as one message, each over a heap copy of
    exactly the input's size, through decode_message<uint32_t>, decode_message<uint64_t> (which
    must agree on the status, the error and every field) and the header hop."""
    msgs = []
    for fx in wire_cases.FIX["batches"]:
        raw = bytes.fromhex(fx["hex"])
        msgs += [raw[2:2 + raw[1]], raw]
    c_array = lambda name, typ, data: \
        f"static const {typ} {name}[] = {{{','.join(map(str, data)) or '0'}}};\n"
    tables, seen = "", set()
    for i, m in enumerate(msgs):
        cut = [int(ref.rejected(m[:n])) for n in range(len(m) + 1)]
        hops = [hop_status(m[:n]) for n in range(len(m) + 1)]
        seen |= set(cut) | {2 + h for h in hops}
        tables += c_array(f"kMsg{i}", "uint8_t", m) + c_array(f"kCut{i}", "int8_t", cut) + \
            c_array(f"kHop{i}", "int8_t", hops)
    assert seen == {0, 1, 2, 3}                    # both outcomes of both
    tables += "static const struct { const uint8_t *p; size_t n; const int8_t *truncated, *hop; } " \
        "kMessages[] = {" + ",".join(f"{{kMsg{i}, {len(m)}, kCut{i}, kHop{i}}}"
                                     for i, m in enumerate(msgs)) + "};\n"
    src = tmp_path / "codec_sweeps.cpp"
    src.write_text(SANITIZER_MAIN % {"tables": tables})
    exe = tmp_path / "codec_sweeps"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "dragonboat_amd", "csrc"),
                    "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "" and r.stdout.startswith("ok ")
    assert int(r.stdout.split()[1]) == 2 * 256 * sum(len(m) for m in msgs)
