"""The segment walker of hq_wire_codec.h (walk_segment, guess_entry, chain_batch: what
hq_wire_frame_dev.hip runs on the device) on the CPU, no GPU: a stand-alone program built with the
address and undefined-behaviour sanitizers frames every input by segments, over exactly sized heap
copies, and holds the result to hq_wire_frame_batch. The property is "never wrong, sometimes
unconfirmed": a batch comes back framed only with the host's messages, malformed only where the
host says so, and otherwise unconfirmed; at the default segment size the steady-state inputs must
all be confirmed."""
import os
import struct
import subprocess

import numpy as np
import pytest

import wire_cases
import wire_encode as we
from wire_cases import FIX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEGMENTS = (64, 100, 256, 4096, 65536)
MUST_CONFIRM = 1          # flag: no status 3 at 65536

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hipquorum.h"
#include "hq_wire_codec.h"

static std::vector<uint8_t> file;
static unsigned long runs, unconfirmed, unconfirmed_default, overflowed, malformed, framed, voids_seen,
    multi_framed;

struct Host {
    int rc;
    std::vector<hq_wire_span> spans;
    hq_wire_batch_info info;
};

static Host host_frame(const uint8_t *b, size_t len) {
    Host h{};
    uint64_t n = 0;
    h.rc = hq_wire_frame_batch(len ? b : nullptr, len, 0, nullptr, 0, &n, &h.info);
    if (h.rc == HQ_OK) {
        h.spans.resize(n);
        uint64_t n2 = 0;
        const int rc2 = hq_wire_frame_batch(len ? b : nullptr, len, 0, h.spans.data(), n, &n2, &h.info);
        if (rc2 != HQ_OK || n2 != n) abort();
    }
    return h;
}

// the (field start, field size) of every message of the spans, hopped header by header; false
// when a span breaks a rule
static bool messages_of(const uint8_t *b, size_t len, const std::vector<hq_wire_span> &spans,
                        std::vector<uint64_t> &out) {
    uint64_t first = 0;
    for (const hq_wire_span &s : spans) {
        if (s.count < 1 || s.count > HQ_WIRE_SPAN_MESSAGES || s.offset > len || s.len > len - s.offset)
            return false;
        if (s.flags & HQ_WIRE_SPAN_LARGE) {
            if (s.flags != HQ_WIRE_SPAN_LARGE || s.count != 1 || s.len <= HQ_WIRE_SPAN_BYTES) return false;
        } else if (s.flags || s.len > HQ_WIRE_SPAN_BYTES) {
            return false;
        }
        if (s.first != first) return false;
        first += s.count;
        uint64_t p = s.offset;
        const uint64_t end = s.offset + s.len;
        for (unsigned k = 0; k < s.count; ++k) {
            const uint64_t f0 = p;
            uint64_t n;
            if (!hqw::header<uint64_t>(b, p, end, n)) return false;
            p += n;
            out.push_back(f0);
            out.push_back(p - f0);
        }
        if (p != end) return false;
    }
    return true;
}

struct Framed {
    hq_wire_frame_result r;
    uint32_t voids;
    std::vector<hq_wire_span> spans;     // the dense list, as k_wire_spans makes it
    std::vector<hqw::Segment> seg;
};

// window == 0: every segment walked over the whole batch; else over windows of `window` bytes,
// each an exactly sized heap copy (what the kernel keeps in LDS), the guess reading behind its
// window from the batch
static Framed frame_by_segments(const uint8_t *b, size_t len, uint64_t S, uint64_t window) {
    Framed f{};
    const uint64_t n = hqw::segment_count(S, len), cap = S / 128 + 8;
    f.seg.resize(n);
    std::vector<hq_wire_span> region(n * cap);
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t lo = k * S, end = hqw::segment_end(k, S, len);
        hq_wire_span *const mine = region.data() + k * cap;
        auto put = [&](uint64_t i, const hq_wire_span &s) {
            if (i < cap) mine[i] = s;
        };
        hqw::SegmentWalk w;
        if (!window) {
            const hqw::Window all{b, 0, len};
            hqw::segment_begin(w, k ? hqw::guess_entry(all, lo, end, len) : 0);
            if (w.s.entry != hqw::kNoEntry && !hqw::walk_segment(all, len, len, end, w, put)) abort();
        } else {
            uint64_t entry = k ? hqw::kNoEntry : 0;
            for (uint64_t at = lo; k && entry == hqw::kNoEntry && at < end; at += window) {
                const uint64_t hi = at + window < len ? at + window : len;
                uint8_t *copy = new uint8_t[hi - at];
                memcpy(copy, b + at, hi - at);
                const hqw::WindowOver over{hqw::Window{copy, at, hi}, b};
                entry = hqw::guess_entry(over, at, at + window < end ? at + window : end, len);
                delete[] copy;
            }
            hqw::segment_begin(w, entry);
            for (uint64_t turn = 0; entry != hqw::kNoEntry; ++turn) {
                if (turn > end - lo) abort();                  // every window takes a field
                const uint64_t at = w.pos, hi = at + window < len ? at + window : len;
                uint8_t *copy = new uint8_t[hi - at ? hi - at : 1];
                memcpy(copy, b + at, hi - at);
                const bool done = hqw::walk_segment(hqw::Window{copy, at, hi}, hi, len, end, w, put);
                delete[] copy;
                if (done) break;
            }
        }
        f.seg[k] = w.s;
    }
    std::vector<hqw::SegmentPlace> place(n);
    hqw::chain_batch(f.seg.data(), n, S, len, cap, place.data(), f.r, f.voids);
    if (f.r.status == hqw::kFramed)
        for (uint64_t k = 0; k < n; ++k) {
            if (place[k].first_span == hqw::kNoEntry) continue;
            for (uint64_t i = 0; i < f.seg[k].n_spans; ++i) {
                hq_wire_span s = region[k * cap + i];
                s.first += (uint32_t)place[k].first_message;
                if (f.spans.size() != place[k].first_span + i) abort();
                f.spans.push_back(s);
            }
        }
    return f;
}

static bool same_span(const hq_wire_span &a, const hq_wire_span &b) {
    return a.offset == b.offset && a.len == b.len && a.first == b.first && a.count == b.count &&
           a.flags == b.flags;
}

static int check(unsigned index, uint32_t flags, const uint8_t *src, size_t len) {
    uint8_t *b = new uint8_t[len ? len : 1];               // exactly sized: the sanitizer's bounds
    if (len) memcpy(b, src, len);
    const Host h = host_frame(b, len);
    std::vector<uint64_t> want;
    if (h.rc == HQ_OK && !messages_of(b, len, h.spans, want)) abort();
    static const uint64_t kSegments[] = {%(segments)s};
    int bad = 0;
    for (uint64_t S : kSegments) {
        for (uint64_t window : {uint64_t(0), uint64_t(96)}) {
            if (window && len > 20000) continue;           // (the long inputs: whole-batch only)
            const Framed f = frame_by_segments(b, len, S, window);
            const uint64_t n = hqw::segment_count(S, len);
            ++runs;
            voids_seen += f.voids;
            const char *why = nullptr;
            switch (f.r.status) {
            case hqw::kFramed: {
                ++framed;
                multi_framed += n > 1;
                std::vector<uint64_t> got;
                if (h.rc != HQ_OK) why = "framed, the host rejects";
                else if (!messages_of(b, len, f.spans, got)) why = "a span breaks a rule";
                else if (got != want) why = "other messages than the host's";
                else if (f.r.n_messages != h.info.n_messages || f.r.n_spans != f.spans.size() ||
                         f.r.deployment_id != h.info.deployment_id ||
                         f.r.source_address_len != h.info.source_address_len ||
                         f.r.bin_ver != h.info.bin_ver)
                    why = "other info than the host's";
                else if (n <= 1) {
                    if (f.spans.size() != h.spans.size()) why = "one segment: other spans";
                    for (size_t i = 0; !why && i < f.spans.size(); ++i)
                        if (!same_span(f.spans[i], h.spans[i])) why = "one segment: other spans";
                }
                break;
            }
            case hqw::kMalformed:
                ++malformed;
                if (h.rc != HQ_E_INVAL) why = "malformed, the host accepts";
                break;
            case hqw::kSpansDidNotFit: {
                ++overflowed;
                bool over = false;
                for (const hqw::Segment &s : f.seg) over = over || s.n_spans > S / 128 + 8;
                if (!over || h.rc != HQ_OK) why = "status 2 without a full region";
                break;
            }
            case hqw::kUnconfirmed:
                ++unconfirmed;
                if (n <= 1) why = "one segment unconfirmed";
                if (S == 65536 && (flags & %(must)d)) {
                    ++unconfirmed_default;
                    why = "unconfirmed at the default segment size";
                }
                break;
            default: why = "unknown status";
            }
            if (why) {
                printf("input %%u (%%zu bytes) S=%%llu window=%%llu: %%s\n", index, len,
                       (unsigned long long)S, (unsigned long long)window, why);
                ++bad;
            }
        }
    }
    delete[] b;
    return bad;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    fseek(fp, 0, SEEK_END);
    file.resize((size_t)ftell(fp));
    fseek(fp, 0, SEEK_SET);
    if (fread(file.data(), 1, file.size(), fp) != file.size()) return 2;
    fclose(fp);
    size_t p = 0;
    unsigned index = 0;
    int bad = 0;
    while (p < file.size() && bad < 20) {
        uint32_t flags;
        uint64_t len;
        memcpy(&flags, &file[p], 4);
        memcpy(&len, &file[p + 4], 8);
        p += 12;
        bad += check(index++, flags, file.data() + p, (size_t)len);
        p += (size_t)len;
    }
    printf("inputs=%%u runs=%%lu framed=%%lu multi_framed=%%lu malformed=%%lu status2=%%lu unconfirmed=%%lu "
           "unconfirmed_default=%%lu voids=%%lu\n", index, runs, framed, multi_framed, malformed,
           overflowed, unconfirmed, unconfirmed_default, voids_seen);
    return bad ? 1 : 0;
}
"""


def steady_batch():
    """200 KB of 51-byte steady-state messages (one-byte varints but the 2-byte log index), as a
    leader's transport drains them."""
    rng = np.random.default_rng(20)
    msgs = []
    for _ in range(3930):
        m = we.message(type=13, to=1, frm=int(rng.integers(1, 8)), cluster_id=int(rng.integers(1, 128)),
                       term=5, log_index=int(rng.integers(128, 16384)),
                       commit=int(rng.integers(0, 128)))
        assert len(m) + 2 == 51
        msgs.append(m)
    return we.batch(msgs, deployment_id=1, source_address=b"10.0.0.1:26000")


def replacements(raw):
    for i, b in enumerate(raw):
        for v in (0x00, 0x7F, 0x80, 0xFF, b ^ 1, b ^ 0x80):
            yield raw[:i] + bytes([v]) + raw[i + 1:]


def inputs():
    """(flags, bytes) of every input."""
    out = []
    fixtures = [bytes.fromhex(fx["hex"]) for fx in FIX["batches"]]
    out += [(0, f) for f in fixtures]
    out += [(0, bytes.fromhex(fx["hex"])) for fx in FIX["malformed"]]
    # the fixtures in one batch, so that their truncations and replacements cross segment edges
    joined = b"".join(fixtures) * 2 + we.f_varint(2, 7) + we.f_bytes(3, b"n1:1") + we.f_varint(4, 210)
    for raw in fixtures + [joined]:
        out += [(0, raw[:n]) for n in range(len(raw))]
        out += [(0, r) for r in replacements(raw)]
    msgs = wire_cases.parity_messages()
    out.append((MUST_CONFIRM, we.batch(msgs, deployment_id=3, source_address=b"n:1")))
    for k in range(0, len(msgs), 500):
        out.append((MUST_CONFIRM, we.batch(msgs[k:k + 500], deployment_id=k)))
    out.append((MUST_CONFIRM, steady_batch()))
    # long messages: void segments at the small sizes, a large span, fields between messages
    big = we.message(type=3, cluster_id=4, entries=[we.entry(1, i, b"\x5a" * 3000) for i in range(3)])
    out.append((MUST_CONFIRM, we.batch(msgs[:40] + [big] + msgs[40:90], deployment_id=9)))
    m = [we.f_bytes(1, x) for x in msgs[:8]]
    out.append((0, m[0] + m[1] + we.f_varint(2, 5) + m[2] + we.key(9, 5) + b"abcd" + m[3]
                + we.f_bytes(3, b"a:1") + m[4] + we.f_bytes(9, b"\x0a" * 300) + m[5]
                + we.f_varint(4, 210) + m[6] + m[7]))
    # many other fields: more spans than a segment's region holds
    out.append((0, b"".join(we.f_bytes(1, b"") + we.f_varint(7, 1) for _ in range(400))))
    out.append((0, b""))
    return out


def test_segment_walker_under_sanitizers(tmp_path):
    data = tmp_path / "inputs.bin"
    ins = inputs()
    with open(data, "wb") as f:
        for flags, raw in ins:
            f.write(struct.pack("<IQ", flags, len(raw)) + raw)
    src = tmp_path / "frame_segments.cpp"
    src.write_text(PROGRAM % {"segments": ",".join(map(str, SEGMENTS)), "must": MUST_CONFIRM})
    exe = tmp_path / "frame_segments"
    csrc = os.path.join(ROOT, "dragonboat_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "include"), "-I", csrc, "-o", str(exe), str(src),
                    os.path.join(csrc, "hq_wire_frame.cpp")], check=True)
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stderr == ""
    got = dict(kv.split("=") for kv in r.stdout.strip().splitlines()[-1].split())
    got = {k: int(v) for k, v in got.items()}
    assert got["inputs"] == len(ins)
    assert got["unconfirmed_default"] == 0
    # every outcome was met: batches of several segments framed, framing errors found from a
    # confirmed segment, a full span region, wrong guesses caught by the chain, void segments
    for k in ("multi_framed", "malformed", "status2", "unconfirmed", "voids"):
        assert got[k] > 0, k


def test_the_inputs_hold_what_they_claim():
    ins = inputs()
    assert len(steady_batch()) > 200_000
    assert sum(f == MUST_CONFIRM and len(b) > 3 * 65536 for f, b in ins) >= 2
    assert sum(len(b) for _, b in ins) < 4 << 20
