"""hq_wire_frame_batch (dragonboat_amd/csrc/hq_wire_frame.cpp; host code, no GPU): the framing of a
MessageBatch into spans for the device decoder. It must agree with the host decoder
(hq_wire_decode_batch) on what is a batch, never look into a message, and cut spans the decode
kernel can take: at most 64 messages and HQ_WIRE_SPAN_BYTES bytes, back to back, a larger message
alone and flagged. A Python restatement of the framing walk is the reference for truncations; a
stand-alone C++ program built with the address and undefined-behaviour sanitizers runs the
truncation and mutation sweeps over exactly sized heap buffers."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import wire_encode as we

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "wire_fixtures.json")))


# ---- the reference walk of the framing (hq_wire_codec.h walk_batch, without the message decode) ----
class Malformed(Exception):
    pass


def rd_varint(b, p, end):
    v = 0
    for shift in range(0, 64, 7):
        if p >= end:
            raise Malformed("end of data in a varint")
        x = b[p]
        p += 1
        v |= (x & 0x7F) << shift
        if x < 0x80:
            return v & ((1 << 64) - 1), p
    raise Malformed("varint overflows 64 bits")


def rd_bytes(b, p, end):
    n, p = rd_varint(b, p, end)
    if end - p < n:
        raise Malformed("end of data in a length-delimited field")
    return p, p + n


def ref_walk(b):
    """(fields, info): fields lists ("m", field start, body start, body end) for every message
    and ("x",) for any other field, in order; raises Malformed as the C walk returns HQ_E_INVAL."""
    p, end, fields = 0, len(b), []
    info = {"deployment_id": 0, "source_address_len": 0, "bin_ver": 0}
    while p < end:
        f0 = p
        tag, p = rd_varint(b, p, end)
        field, wt = (tag >> 3) & 0xFFFFFFFF, tag & 7
        if field == 1 and wt == 2:
            s, p = rd_bytes(b, p, end)
            fields.append(("m", f0, s, p))
            continue
        fields.append(("x",))
        if field == 2 and wt == 0:
            info["deployment_id"], p = rd_varint(b, p, end)
        elif field == 3 and wt == 2:
            s, p = rd_bytes(b, p, end)
            info["source_address_len"] = p - s
        elif field == 4 and wt == 0:
            v, p = rd_varint(b, p, end)
            info["bin_ver"] = v & 0xFFFFFFFF
        elif field <= 4:
            raise Malformed("field 0 or a known field's wrong wire type")
        elif wt == 0:
            _, p = rd_varint(b, p, end)
        elif wt == 2:
            _, p = rd_bytes(b, p, end)
        elif wt in (1, 5):
            n = 8 if wt == 1 else 4
            if end - p < n:
                raise Malformed("end of data in a field")
            p += n
        else:
            raise Malformed("group wire type")
    info["n_messages"] = sum(f[0] == "m" for f in fields)
    return fields, info


def ref_status(b):
    try:
        ref_walk(b)
        return 0
    except Malformed:
        return -1


# ---- inputs ----
def message_of_len(n):
    """A valid Message of exactly n bytes (an unknown length-delimited field pads it)."""
    if n == 0:
        return b""
    if n == 2:
        return we.f_varint(1, 13)
    k = n - 3 - (1 if n - 4 < 128 else 2)
    m = we.f_varint(1, 13) + we.f_bytes(15, b"\xee" * k)
    assert len(m) == n
    return m


def random_messages(rng, n):
    big = [0, 1, 127, 128, 300, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1]
    v = lambda: big[int(rng.integers(len(big)))] if rng.random() < 0.3 else int(rng.integers(0, 1 << 40))
    out = []
    for _ in range(n):
        ents = [we.entry(v(), v(), bytes(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8)))
                for _ in range(int(rng.integers(0, 3)))]
        out.append(we.message(type=int(rng.integers(0, 26)), to=v(), frm=v(), cluster_id=v(),
                              term=v(), log_term=v(), log_index=v(), commit=v(),
                              reject=bool(rng.random() < 0.5), hint=v(), entries=ents, hint_high=v()))
    return out


def five_message_batch():
    return we.batch(random_messages(np.random.default_rng(5), 5), deployment_id=9,
                    source_address=b"n1:7")


def inputs():
    rng = np.random.default_rng(3)
    out = [(fx["name"], bytes.fromhex(fx["hex"])) for fx in FIX["batches"] + FIX["malformed"]]
    for n in (1, 63, 64, 65, 200):
        out.append((f"random_{n}", we.batch(random_messages(rng, n), deployment_id=n,
                                            source_address=b"10.0.0.1:26000")))
    out.append(("empty", b""))
    out.append(("message_lengths_0_127_128",
                we.batch([message_of_len(n) for n in (0, 127, 128, 0, 128, 127)])))
    big = we.message(type=3, cluster_id=4, entries=[we.entry(1, 1, b"\x5a" * 5000)])
    small = random_messages(rng, 6)
    out.append(("entries_over_the_budget", we.batch(small[:3] + [big] + small[3:])))
    out.append(("only_a_large_message", we.batch([big])))
    # other fields between the messages (any field order), an unknown field among them
    m = [we.f_bytes(1, x) for x in random_messages(rng, 6)]
    out.append(("fields_between_messages",
                m[0] + m[1] + m[2] + we.f_varint(2, 5) + m[3] + we.key(9, 5) + b"abcd" + m[4]
                + we.f_bytes(3, b"a:1") + we.f_varint(4, 210) + m[5]))
    # many short messages: the 64-message limit cuts before the byte budget does
    out.append(("short_messages", we.batch([message_of_len(n % 3 * 2) for n in range(300)])))
    # long messages: the byte budget cuts first
    out.append(("long_messages", we.batch([message_of_len(1000 + n) for n in range(20)])))
    return out


INPUTS = inputs()


def frame_raw(hq, data, cap=None):
    """(rc, spans, n_spans, info) of hq_wire_frame_batch over an exactly sized copy of data."""
    buf = np.frombuffer(bytes(data), np.uint8).copy()
    n = ctypes.c_uint64(0)
    info = hq.WireBatchInfo()
    rc = hq.lib.hq_wire_frame_batch(hq._p(buf) if len(buf) else None, len(buf), 0, None, 0,
                                    ctypes.byref(n), ctypes.byref(info))
    if rc != hq.HQ_OK:
        return rc, None, n.value, info
    cap = n.value if cap is None else cap
    spans = np.zeros(max(1, cap), hq.WIRE_SPAN_DTYPE)
    rc = hq.lib.hq_wire_frame_batch(hq._p(buf) if len(buf) else None, len(buf), 0, hq._p(spans),
                                    cap, ctypes.byref(n), ctypes.byref(info))
    return rc, spans[:min(cap, n.value)], n.value, info


def decode_raw(hq, data):
    buf = np.frombuffer(bytes(data), np.uint8).copy()
    n = ctypes.c_uint64(0)
    info = hq.WireBatchInfo()
    rc = hq.lib.hq_wire_decode_batch(hq._p(buf) if len(buf) else None, len(buf), None, 0,
                                     ctypes.byref(n), ctypes.byref(info))
    return rc, n.value, info


@pytest.mark.parametrize("name,data", INPUTS, ids=[n for n, _ in INPUTS])
def test_agrees_with_the_host_decoder(hq, name, data):
    drc, dn, dinfo = decode_raw(hq, data)
    frc, _, _, finfo = frame_raw(hq, data)
    assert drc in (hq.HQ_OK, hq.HQ_E_INVAL) and frc in (hq.HQ_OK, hq.HQ_E_INVAL)
    if drc == hq.HQ_OK:
        assert frc == hq.HQ_OK
        assert finfo.n_messages == dinfo.n_messages == dn
        for f in ("deployment_id", "source_address_len", "bin_ver", "reserved"):
            assert getattr(finfo, f) == getattr(dinfo, f), f
    if frc == hq.HQ_E_INVAL:
        assert drc == hq.HQ_E_INVAL
    assert frc == ref_status(data)


def test_the_inputs_hold_both_outcomes(hq):
    rcs = [frame_raw(hq, d)[0] for _, d in INPUTS]
    assert hq.HQ_OK in rcs and hq.HQ_E_INVAL in rcs
    # a batch the framing accepts and the decoder rejects: the message is not looked into
    data = bytes.fromhex(next(f["hex"] for f in FIX["malformed"] if f["name"] == "group_wire_type"))
    assert frame_raw(hq, data)[0] == hq.HQ_OK and decode_raw(hq, data)[0] == hq.HQ_E_INVAL


@pytest.mark.parametrize("name,data", INPUTS, ids=[n for n, _ in INPUTS])
def test_span_invariants(hq, name, data):
    rc, spans, n, info = frame_raw(hq, data)
    if rc != hq.HQ_OK:
        assert ref_status(data) == -1
        return
    fields, rinfo = ref_walk(data)
    want = [(s, e) for f in fields if f[0] == "m" for s, e in [f[2:]]]
    assert len(spans) == n and info.n_messages == len(want) == rinfo["n_messages"]
    assert int(spans["count"].sum()) == len(want)
    got, first = [], 0
    for sp in spans:
        count, length, off = int(sp["count"]), int(sp["len"]), int(sp["offset"])
        assert 1 <= count <= hq.HQ_WIRE_SPAN_MESSAGES
        if sp["flags"] & hq.HQ_WIRE_SPAN_LARGE:
            assert count == 1 and length > hq.HQ_WIRE_SPAN_BYTES
        else:
            assert sp["flags"] == 0 and length <= hq.HQ_WIRE_SPAN_BYTES
        assert int(sp["first"]) == first
        first += count
        # the headers hopped from the span's offset: tag, length, body, back to back
        p, end = off, off + length
        assert end <= len(data)
        for _ in range(count):
            tag, p = rd_varint(data, p, end)
            assert tag >> 3 == 1 and tag & 7 == 2
            s, p = rd_bytes(data, p, end)
            got.append((s, p))
        assert p == end
    assert got == want
    # spans are as long as the rules allow: two neighbours could not have been one
    starts = {f[1]: i for i, f in enumerate(fields) if f[0] == "m"}
    for a, b in zip(spans[:-1], spans[1:]):
        adjacent = int(a["offset"] + a["len"]) == int(b["offset"]) and \
            fields[starts[int(b["offset"])] - 1][0] == "m"
        if adjacent and not (a["flags"] | b["flags"]):
            size_b0 = want[int(b["first"])][1] - int(b["offset"])
            assert a["count"] == hq.HQ_WIRE_SPAN_MESSAGES or \
                int(a["len"]) + size_b0 > hq.HQ_WIRE_SPAN_BYTES


def test_expected_cuts(hq):
    """The cases are what they claim to be: both limits cut, a large message is alone."""
    by = dict(INPUTS)
    _, spans, _, _ = frame_raw(hq, by["short_messages"])
    assert list(spans["count"]) == [64, 64, 64, 64, 44]
    _, spans, _, _ = frame_raw(hq, by["long_messages"])
    assert list(spans["count"]) == [4] * 5
    _, spans, _, _ = frame_raw(hq, by["entries_over_the_budget"])
    assert [(int(s["count"]), int(s["flags"])) for s in spans] == [(3, 0), (1, 1), (3, 0)]
    _, spans, _, _ = frame_raw(hq, by["fields_between_messages"])
    assert list(spans["count"]) == [3, 1, 1, 1]
    _, spans, n, info = frame_raw(hq, b"")
    assert n == 0 and info.n_messages == 0


def test_base_and_first_offsets(hq):
    data = dict(INPUTS)["random_200"]
    a, _ = hq.frame_batch(data)
    b, info = hq.frame_batch(data, base=1 << 40, first=77)
    assert info.n_messages == 200
    assert list(b["offset"] - a["offset"]) == [1 << 40] * len(a)
    assert list(b["first"] - a["first"]) == [77] * len(a)
    for f in ("len", "count", "flags"):
        assert list(a[f]) == list(b[f])


def test_every_truncation_of_a_batch(hq):
    data = five_message_batch()
    assert ref_walk(data)[1]["n_messages"] == 5
    seen = set()
    for n in range(len(data) + 1):
        rc = frame_raw(hq, data[:n])[0]
        assert rc == ref_status(data[:n]), n
        seen.add(rc)
    assert seen == {hq.HQ_OK, hq.HQ_E_INVAL}


def test_arguments(hq):
    data = dict(INPUTS)["random_200"]
    buf = np.frombuffer(data, np.uint8)
    n = ctypes.c_uint64(0)
    f = hq.lib.hq_wire_frame_batch
    assert f(None, len(data), 0, None, 0, ctypes.byref(n), None) == hq.HQ_E_INVAL
    assert f(hq._p(buf), len(data), 0, None, 0, None, None) == hq.HQ_E_INVAL
    assert f(None, 0, 0, None, 0, ctypes.byref(n), None) == hq.HQ_OK and n.value == 0
    assert f(hq._p(buf), len(data), 0, None, 0, ctypes.byref(n), None) == hq.HQ_OK   # info optional
    need = n.value
    assert need >= 4
    rc, spans, got, _ = frame_raw(hq, data, cap=need - 1)
    assert rc == hq.HQ_E_STATE and got == need
    full = frame_raw(hq, data)[1]
    assert spans.tobytes() == full[:need - 1].tobytes()    # what fits is written
    assert ctypes.sizeof(ctypes.c_uint64) * 3 == hq.WIRE_SPAN_DTYPE.itemsize == 24


SANITIZER_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "hipquorum.h"
%(tables)s
// one call to count and one to fill, over heap copies of exactly len bytes and exactly n spans
static int frame(const uint8_t *src, size_t len, uint64_t *messages) {
    uint8_t *b = new uint8_t[len ? len : 1];
    if (len) memcpy(b, src, len);
    uint64_t n = 0, n2 = 0;
    hq_wire_batch_info bi, bi2;
    int rc = hq_wire_frame_batch(len ? b : nullptr, len, 0, nullptr, 0, &n, &bi);
    if (rc == HQ_OK) {
        hq_wire_span *s = new hq_wire_span[n ? n : 1];
        const int rc2 = hq_wire_frame_batch(len ? b : nullptr, len, 0, s, n, &n2, &bi2);
        uint64_t sum = 0;
        bool good = rc2 == HQ_OK && n2 == n && bi2.n_messages == bi.n_messages;
        for (uint64_t i = 0; good && i < n; ++i) {
            good = s[i].count >= 1 && s[i].count <= HQ_WIRE_SPAN_MESSAGES && s[i].offset <= len &&
                   s[i].len <= len - s[i].offset && s[i].first == sum;
            sum += s[i].count;
        }
        if (!good || sum != bi.n_messages) rc = 99;
        *messages = bi.n_messages;
        delete[] s;
    }
    delete[] b;
    return rc;
}
int main() {
    uint64_t m = 0;
    for (size_t n = 0; n <= sizeof kBatch; ++n) {
        const int rc = frame(kBatch, n, &m);
        if (rc != kTruncated[n]) {
            printf("truncation %%zu: %%d, expected %%d\n", n, rc, (int)kTruncated[n]);
            return 1;
        }
    }
    unsigned runs = 0;
    for (unsigned f = 0; f < sizeof kFixtures / sizeof *kFixtures; ++f) {
        std::vector<uint8_t> b(kFixtures[f].p, kFixtures[f].p + kFixtures[f].n);
        for (size_t i = 0; i < b.size(); ++i) {
            const uint8_t keep = b[i];
            for (unsigned v = 0; v < 256; ++v) {
                b[i] = (uint8_t)v;
                const int rc = frame(b.data(), b.size(), &m);
                if (rc != HQ_OK && rc != HQ_E_INVAL) {
                    printf("fixture %%u byte %%zu = %%u: %%d\n", f, i, v, rc);
                    return 1;
                }
                ++runs;
            }
            b[i] = keep;
        }
    }
    printf("ok %%u\n", runs);
    return 0;
}
"""


def c_array(name, data):
    return f"static const uint8_t {name}[] = {{{','.join(map(str, data)) or '0'}}};\n"


def test_sanitizer_sweeps_stand_alone(tmp_path):
    """hq_wire_frame.cpp compiled into a program of its own with -fsanitize=address,undefined: the
    truncation sweep (statuses as the reference walk gives them) and every single-byte mutation of
    every fixture, each over a heap copy of exactly the input's size."""
    data = five_message_batch()
    fixtures = [bytes.fromhex(f["hex"]) for f in FIX["batches"] + FIX["malformed"]]
    tables = c_array("kBatch", data)
    tables += "static const int8_t kTruncated[] = {" + \
        ",".join(str(ref_status(data[:n])) for n in range(len(data) + 1)) + "};\n"
    for i, f in enumerate(fixtures):
        tables += c_array(f"kFix{i}", f)
    tables += "static const struct { const uint8_t *p; size_t n; } kFixtures[] = {" + \
        ",".join(f"{{kFix{i}, {len(f)}}}" for i, f in enumerate(fixtures)) + "};\n"
    src = tmp_path / "frame_sweeps.cpp"
    src.write_text(SANITIZER_MAIN % {"tables": tables})
    exe = tmp_path / "frame_sweeps"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
                    "-o", str(exe), str(src),
                    os.path.join(ROOT, "dragonboat_amd", "csrc", "hq_wire_frame.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "" and r.stdout.startswith("ok ")
    assert int(r.stdout.split()[1]) == 256 * sum(len(f) for f in fixtures)
