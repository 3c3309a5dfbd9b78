"""The wire's and the event stream's C entries when an allocation fails, without a GPU:
hq_wire.cpp, hq_wire_frame.cpp, hq_stream.cpp and hq_stream16.cpp compiled into a program of
their own with -fsanitize=address,undefined, over stubs for the two worker entries they import
and for the device side of the wire. The program replaces operator new with a counter that throws
std::bad_alloc once, at the k-th allocation of a call. For every call below it counts the
allocations of a clean run and then repeats the call once per k, each time on a freshly prepared
wire: the call must answer HQ_E_NOMEM with "<entry>: out of memory", the same call must then
succeed, and the wire must step to the bytes, sizes and stats of a wire that never saw a failure
(all or nothing). A second program pins the task pool: a function that throws on one index of
four, plain and gang, gives parallel_for a code and leaves the pool usable. No Python process
loads sanitized code."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dragonboat_amd", "csrc")
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "wire_fixtures.json")))
SANITIZE = ["-std=c++17", "-O1", "-pthread", "-Wall", "-Wextra", "-Werror",
            "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC]

STUBS_CPP = r"""
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "hq_wire_dev.h"

static unsigned long checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { std::printf("FAILED %s line %d\n", #c, __LINE__); std::exit(1); } } while (0)

// ---- operator new: while armed, allocations are counted and the k-th throws (once)
static std::atomic<bool> armed{false};
static std::atomic<long> n_allocs{0}, fail_at{0};
static std::atomic<size_t> fired_size{0};      // the size of the allocation that failed, 0: none
static void arm(long k) { n_allocs = 0; fail_at = k; fired_size = 0; armed = true; }
static long disarm() { armed = false; return n_allocs; }
// f() with its k-th allocation failing (k 0: none fails, they are counted; k < 0: not armed)
static long counted = 0;
template <class F>
static int armed_rc(long k, F f) {
    if (k >= 0) arm(k);
    const int rc = f();
    if (k >= 0) counted = disarm();
    return rc;
}
void *operator new(size_t n) {
    if (armed && ++n_allocs == fail_at) {
        fired_size = n ? n : 1;
        throw std::bad_alloc();
    }
    if (void *p = std::malloc(n ? n : 1)) return p;
    throw std::bad_alloc();
}
void *operator new(size_t n, const std::nothrow_t &) noexcept { return std::malloc(n ? n : 1); }
void *operator new[](size_t n) { return operator new(n); }
void operator delete(void *p) noexcept { std::free(p); }
void operator delete(void *p, size_t) noexcept { std::free(p); }
void operator delete[](void *p) noexcept { std::free(p); }
void operator delete[](void *p, size_t) noexcept { std::free(p); }

// ---- the stub worker: cluster id -> handle
struct hq_worker {
    uint64_t n = 0;
    std::unordered_map<uint64_t, uint32_t> h;
    void add(uint64_t cid) { h.emplace(cid, (uint32_t)n++); }
};
extern "C" int hq_worker_find(hq_worker *w, uint64_t cid, uint32_t *handle) {
    auto it = w->h.find(cid);
    if (it == w->h.end()) return HQ_E_INVAL;
    *handle = it->second;
    return HQ_OK;
}
extern "C" int hq_worker_group_count(hq_worker *w, uint64_t *n) {
    *n = w->n;
    return HQ_OK;
}
// ---- the wire's device mode: never entered here
int hq_wire_dev_open(hq_worker *, hq_wire_dev **) { return HQ_E_DEVICE; }
void hq_wire_dev_close(hq_wire_dev *) {}
const char *hq_wire_dev_error(const hq_wire_dev *) { return ""; }
void hq_wire_dev_reset(hq_wire_dev *) {}
int hq_wire_dev_add_batch(hq_wire_dev *, const uint8_t *, size_t, const hq_wire_span *, uint64_t,
                          uint64_t, uint32_t) { return HQ_E_DEVICE; }
void hq_wire_dev_set_framing(hq_wire_dev *, bool, uint64_t) {}
bool hq_wire_dev_framing(const hq_wire_dev *) { return false; }
int hq_wire_dev_queue(hq_wire_dev *, const uint8_t *, size_t, uint32_t) { return HQ_E_DEVICE; }
void hq_wire_dev_frame_stats(const hq_wire_dev *, uint64_t[4]) {}
int hq_wire_dev_step(hq_wire_dev *, const hqs::WireEvent *, uint64_t, hq_step_output *, uint64_t[4],
                     const uint32_t **, uint64_t *, uint64_t *, uint64_t *, hq_wire_stats *) {
    return HQ_E_DEVICE;
}
"""

WIRE_CPP = STUBS_CPP + r"""
typedef std::vector<uint8_t> Bytes;
static const uint64_t kDeployment = 0;           // the fixtures' deployment id

static Bytes from_hex(const char *s) {
    Bytes b;
    for (; s[0] && s[1]; s += 2) {
        char x[3] = {s[0], s[1], 0};
        b.push_back((uint8_t)std::strtoul(x, nullptr, 16));
    }
    return b;
}
// n messages over `clusters` cluster ids from base on (acks and heartbeat acks of 3 senders, a
// few SnapshotReceived aside), marshalled by the library's own encoder
static Bytes make_batch(uint64_t n, uint64_t clusters, uint64_t base, uint64_t deployment) {
    std::vector<hq_wire_message> m(n);
    for (uint64_t i = 0; i < n; ++i) {
        hq_wire_message &x = m[i];
        std::memset(&x, 0, sizeof x);
        x.ev.kind = HQ_EV_MESSAGE;
        x.ev.type = i % 97 == 5 ? 22u /* SnapshotReceived */ : i % 3 ? HQ_MSG_REPLICATE_RESP : HQ_MSG_HEARTBEAT_RESP;
        x.ev.from = 2 + i % 3;
        x.ev.term = 5;
        x.ev.log_index = 100 + i / clusters;
        x.ev.hint = i % 3 ? 0 : 77;
        x.ev.reject = i % 41 == 0;
        x.cluster_id = base + (i * 7) % clusters;
        x.to = 1;
    }
    Bytes out(n * 160 + 64);
    uint64_t len = 0;
    CHECK(hq_wire_encode_batch(m.data(), n, deployment, nullptr, 0, out.data(), out.size(), &len) == HQ_OK);
    out.resize(len);
    return out;
}
struct Locals {
    std::vector<uint64_t> cids, off;
    std::vector<hq_event> ev;
};
static Locals make_locals(uint64_t n, uint64_t base) {
    Locals l;
    l.off.push_back(0);
    for (uint64_t c = 0; c < n; ++c) {
        l.cids.push_back(base + c * 3);
        for (uint64_t j = 0; j <= c % 3; ++j) {
            hq_event e;
            std::memset(&e, 0, sizeof e);
            e.kind = j == 0 ? HQ_EV_PROPOSE : j == 1 ? HQ_EV_READ : HQ_EV_CHECK_QUORUM;
            e.log_index = 1 + c;
            e.hint = c;
            l.ev.push_back(e);
        }
        l.off.push_back(l.ev.size());
    }
    return l;
}

// what a wire steps to: every byte the step hands out, and the stats
struct Stepped {
    int rc = 0;
    Bytes a, b, c, d;
    hq_wire_stats st;
    bool operator==(const Stepped &o) const {
        return rc == o.rc && a == o.a && b == o.b && c == o.c && d == o.d && !std::memcmp(&st, &o.st, sizeof st);
    }
};
template <class T>
static Bytes raw(const T *p, size_t n) {
    return n ? Bytes((const uint8_t *)p, (const uint8_t *)(p + n)) : Bytes();
}
// (k: armed_rc's, around the entry alone)
static Stepped step_stream(hq_wire *w, hq_worker *wk, long k = -1) {
    Stepped s;
    std::memset(&s.st, 0, sizeof s.st);
    hq_step_stream ss;
    s.rc = armed_rc(k, [&] { return hq_wire_step_stream(w, wk, &ss, &s.st); });
    if (s.rc) return s;
    s.a = raw(ss.groups, ss.n_groups);
    s.b = raw(ss.offsets, ss.n_groups + 1);
    s.c = raw(ss.boffsets, ss.n_groups + 1);
    s.d = raw(ss.bytes, ss.boffsets[ss.n_groups]);
    return s;
}
static Stepped step_input(hq_wire *w, hq_worker *wk, long k = -1) {
    Stepped s;
    std::memset(&s.st, 0, sizeof s.st);
    hq_step_input in;
    s.rc = armed_rc(k, [&] { return hq_wire_step_input(w, wk, &in, &s.st); });
    if (s.rc) return s;
    s.a = raw(in.groups, in.n_groups);
    s.b = raw(in.offsets, in.n_groups + 1);
    s.c = raw(in.events, in.offsets[in.n_groups]);
    return s;
}
static Stepped step_sized(hq_wire *w, hq_worker *wk, long k = -1) {
    Stepped s;
    std::memset(&s.st, 0, sizeof s.st);
    Bytes out(1 << 20);
    std::vector<uint16_t> sizes(wk->n);
    hq_step_stream ss;
    s.rc = armed_rc(k, [&] {
        return hq_wire_step_sized(w, out.data(), out.size(), sizes.data(), sizes.size(), &ss, &s.st);
    });
    if (s.rc) return s;
    s.a = raw(sizes.data(), sizes.size());
    s.b = raw(ss.bytes, ss.n_bytes);
    s.c = raw(&ss.n_events, 1);
    return s;
}

static hq_worker *g_worker;                      // runs the fixtures' clusters and 2 of 3 others
static Bytes g_base;                             // what every prepared wire has queued already
static Locals g_base_locals;
static unsigned long repetitions = 0, clean_allocs = 0;

static hq_wire *prepare(bool attached, const Bytes *more = nullptr) {
    hq_wire *w = nullptr;
    CHECK(hq_wire_open(kDeployment, &w) == HQ_OK);
    if (attached) CHECK(hq_wire_attach(w, g_worker) == HQ_OK);
    CHECK(hq_wire_add_batch(w, g_base.data(), g_base.size()) == HQ_OK);
    CHECK(hq_wire_add_locals(w, g_base_locals.cids.size(), g_base_locals.cids.data(), g_base_locals.off.data(),
                             g_base_locals.ev.data()) == HQ_OK);
    if (more) CHECK(hq_wire_add_batch(w, more->data(), more->size()) == HQ_OK);
    return w;
}

// `call(w, k)` (through armed_rc) once clean (its code rc0 and its allocations N), then once per
// k = 1 .. N with the k-th allocation failing, on a freshly prepared wire each time: HQ_E_NOMEM
// and the entry's message; then the call again, clean: rc0; then `step(w)` must give what it
// gives on the wire that never saw a failure. Every k fires: these calls allocate the same things
// every time, so no repetition may answer HQ_OK.
template <class Call, class Step>
static void sweep(const char *what, const char *entry, bool attached, Call call, Step step,
                  const Bytes *more = nullptr) {
    hq_wire *w = prepare(attached, more);
    const int rc0 = call(w, 0);
    const long N = counted;
    const Stepped want = step(w);
    CHECK(want.rc == HQ_OK);
    hq_wire_close(w);
    for (long k = 1; k <= N; ++k) {
        w = prepare(attached, more);
        const int rc = call(w, k);
        CHECK(fired_size != 0);
        CHECK(rc == HQ_E_NOMEM);
        CHECK(std::string(hq_wire_last_error(w)) == std::string(entry) + ": out of memory");
        CHECK(call(w, -1) == rc0);
        CHECK(step(w) == want);
        hq_wire_close(w);
        ++repetitions;
    }
    clean_allocs += N;
    std::printf("%-44s rc %2d  %3ld allocations, each failed once\n", what, rc0, N);
}

// ---- hq_events16_encode_sized_multi: 3 jobs, T threads
struct Job16 {
    std::vector<uint64_t> off;
    std::vector<hq_event16> recs;
    Bytes out;
    std::vector<uint16_t> sizes16;
    std::vector<uint32_t> sizes;
};
static Job16 make_job(uint64_t groups, uint64_t per, uint32_t seed, bool words) {
    Job16 j;
    j.off.push_back(0);
    for (uint64_t g = 0; g < groups; ++g) {
        for (uint64_t i = 0; i < per + g % 3; ++i) {
            hq_event16 r;
            std::memset(&r, 0, sizeof r);
            r.kind = HQ_EV_MESSAGE;
            r.type = (i + seed) % 4 ? HQ_MSG_REPLICATE_RESP : HQ_MSG_HEARTBEAT_RESP;
            r.from = (uint16_t)(2 + i % 3);
            r.term = 5;
            r.value = 100 + (g + seed) % 7;
            j.recs.push_back(r);
        }
        j.off.push_back(j.recs.size());
    }
    j.out.assign(j.recs.size() * HQ_EVENT_STREAM_MAX, 0);
    if (words) j.sizes16.assign(groups, 0);
    else j.sizes.assign(groups, 0);
    return j;
}
static int encode3(Job16 *js, uint32_t T, hq_encode16_job *jobs) {
    for (int i = 0; i < 3; ++i) {
        std::memset(&jobs[i], 0, sizeof jobs[i]);
        jobs[i].n_groups = js[i].off.size() - 1;
        jobs[i].offsets16 = js[i].off.data();
        jobs[i].recs = js[i].recs.data();
        jobs[i].out = js[i].out.data();
        jobs[i].cap = js[i].out.size();
        jobs[i].sizes = js[i].sizes.empty() ? nullptr : js[i].sizes.data();
        jobs[i].sizes16 = js[i].sizes16.empty() ? nullptr : js[i].sizes16.data();
    }
    return hq_events16_encode_sized_multi(jobs, 3, T);
}
// The caller is a fresh thread for every call, so its scratch starts empty and grows inside the
// call. The one case in which a repetition's k-th allocation does not happen, and the call then
// answers HQ_OK: a pool thread keeps its scratch from call to call and takes its chunks from a
// shared counter, so what it allocates in a call is not the same every time.
static void sweep_multi(uint32_t T) {
    // (32 chunks of 4096 records and more: T = 4 is not clamped, and the caller, which starts
    // first, takes its share of the chunks before the pool's threads have taken them all)
    Job16 js[3] = {make_job(9000, 8, 1, true), make_job(40, 100, 2, false), make_job(7000, 7, 3, true)};
    CHECK(js[0].recs.size() + js[1].recs.size() + js[2].recs.size() >= 32 * 4096);
    // the reference: one thread, straight
    std::vector<Bytes> want;
    std::vector<uint64_t> want_events;
    hq_encode16_job jobs[3];
    CHECK(encode3(js, 1, jobs) == HQ_OK);
    for (int i = 0; i < 3; ++i) {
        CHECK(jobs[i].rc == HQ_OK && jobs[i].n_bytes > 0);
        want.push_back(Bytes(js[i].out.begin(), js[i].out.begin() + jobs[i].n_bytes));
        want_events.push_back(jobs[i].n_events);
    }
    auto on_fresh_thread = [&](long k, int *rc, long *n, size_t *fired) {
        std::thread th([&] {
            arm(k);
            *rc = encode3(js, T, jobs);
            *n = disarm();
            *fired = fired_size;
        });
        th.join();
    };
    auto clean_and_same = [&] {
        int rc;
        long n;
        size_t f;
        for (auto &j : js) std::fill(j.out.begin(), j.out.end(), 0xEE);
        on_fresh_thread(0, &rc, &n, &f);
        CHECK(rc == HQ_OK);
        for (int i = 0; i < 3; ++i) {
            CHECK(jobs[i].rc == HQ_OK && jobs[i].n_events == want_events[i] && jobs[i].n_bytes == want[i].size());
            CHECK(!std::memcmp(js[i].out.data(), want[i].data(), want[i].size()));
        }
        return n;
    };
    const long N = clean_and_same();
    long fired_n = 0, in_threads = 0;
    for (long k = 1; k <= N; ++k) {
        int rc;
        long n;
        size_t fired;
        on_fresh_thread(k, &rc, &n, &fired);
        if (fired) {
            ++fired_n;
            if (fired >= (size_t(1) << 20)) ++in_threads;     // (a scratch: a thread's encode phase)
            CHECK(rc == HQ_E_NOMEM);
            for (int i = 0; i < 3; ++i) CHECK(jobs[i].rc == HQ_E_NOMEM && !jobs[i].n_events && !jobs[i].n_bytes);
        } else {
            CHECK(rc == HQ_OK);                                // (the kept scratch, above)
        }
        clean_and_same();
        ++repetitions;
    }
    clean_allocs += N;
    std::printf("hq_events16_encode_sized_multi T=%u %24s %3ld allocations, %ld failed, %ld of them a scratch\n",
                T, "", N, fired_n, in_threads);
    CHECK(fired_n >= 5 && in_threads >= 1);
}

int main(int argc, char **argv) {
    hq_worker worker;
    g_worker = &worker;
    for (uint64_t c = 1; c <= 20; ++c) worker.add(c);            // the fixtures' clusters
    for (uint64_t c = 0; c < 400; ++c)
        if (c % 3) worker.add(1000 + c);
    g_base = make_batch(100, 40, 1000, kDeployment);
    g_base_locals = make_locals(10, 1000);
    std::vector<std::pair<std::string, Bytes>> batches;
    for (int i = 1; i + 1 < argc; i += 2) batches.emplace_back(argv[i], from_hex(argv[i + 1]));
    batches.emplace_back("2000 messages over 300 clusters", make_batch(2000, 300, 1050, kDeployment));
    batches.emplace_back("a foreign deployment's batch", make_batch(200, 30, 1050, kDeployment + 1));
    for (int attached = 0; attached < 2; ++attached) {
        auto step = [&](hq_wire *w) { return attached ? step_sized(w, g_worker) : step_stream(w, g_worker); };
        for (auto &b : batches)
            sweep(((attached ? "add_batch attached: " : "add_batch: ") + b.first).c_str(), "hq_wire_add_batch",
                  attached, [&](hq_wire *w, long k) {
                      return armed_rc(k, [&] { return hq_wire_add_batch(w, b.second.data(), b.second.size()); });
                  }, step);
        const Locals l = make_locals(120, 1100);
        sweep(attached ? "add_locals attached" : "add_locals", "hq_wire_add_locals", attached,
              [&](hq_wire *w, long k) {
                  return armed_rc(k, [&] {
                      return hq_wire_add_locals(w, l.cids.size(), l.cids.data(), l.off.data(), l.ev.data());
                  });
              }, step);
    }
    // attach: allocates only to refuse (events queued); the wire stays as it was attached
    sweep("attach: events queued", "hq_wire_attach", false,
          [&](hq_wire *w, long k) { return armed_rc(k, [&] { return hq_wire_attach(w, g_worker); }); },
          [&](hq_wire *w) { return step_stream(w, g_worker); });
    sweep("attach: events queued, attached", "hq_wire_attach", true,
          [&](hq_wire *w, long k) { return armed_rc(k, [&] { return hq_wire_attach(w, nullptr); }); },
          [&](hq_wire *w) { return step_sized(w, g_worker); });
    {   // an empty wire attaches without an allocation
        hq_wire *w = nullptr;
        CHECK(hq_wire_open(kDeployment, &w) == HQ_OK);
        arm(0);
        CHECK(hq_wire_attach(w, g_worker) == HQ_OK);
        CHECK(disarm() == 0);
        hq_wire_close(w);
    }
    // the steps: the call under test is the step itself; a failed one leaves the queue and the
    // stats untouched (an unattached step counts the events it drops: once per successful call)
    const Bytes big = make_batch(2000, 300, 1050, kDeployment);
    sweep("step_input", "hq_wire_step_input", false,
          [&](hq_wire *w, long k) { return step_input(w, g_worker, k).rc; },
          [&](hq_wire *w) { return step_input(w, g_worker); }, &big);
    sweep("step_stream", "hq_wire_step_stream", false,
          [&](hq_wire *w, long k) { return step_stream(w, g_worker, k).rc; },
          [&](hq_wire *w) { return step_stream(w, g_worker); }, &big);
    sweep("step_sized", "hq_wire_step_sized", true,
          [&](hq_wire *w, long k) { return step_sized(w, g_worker, k).rc; },
          [&](hq_wire *w) { return step_sized(w, g_worker); }, &big);
    sweep_multi(1);
    sweep_multi(4);
    std::printf("ok repetitions %lu allocations %lu checks %lu\n", repetitions, clean_allocs, checks);
    return 0;
}
"""

POOL_CPP = r"""
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <stdexcept>

#include "hq_task_pool.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s line %d\n", #c, __LINE__); std::exit(1); } } while (0)

int main() {
    hqs::TaskPool &pool = hqs::task_pool();
    for (int round = 0; round < 3; ++round)
        for (bool gang : {false, true}) {
            std::atomic<int> ran{0};
            // index 2 of 4 throws; the others finish
            int rc = pool.parallel_for(4, [&](uint32_t i) {
                ++ran;
                if (i == 2) throw std::bad_alloc();
            }, gang);
            CHECK(rc == HQ_E_NOMEM && ran == 4);
            rc = pool.parallel_for(4, [&](uint32_t i) {
                if (i == 2) throw std::runtime_error("not in the table");
            }, gang);
            CHECK(rc == HQ_E_STATE);
            // a following call succeeds; in the gang form all four are there at the same time
            std::mutex m;
            std::condition_variable cv;
            int arrived = 0;
            ran = 0;
            rc = pool.parallel_for(4, [&](uint32_t) {
                ++ran;
                if (!gang) return;
                std::unique_lock<std::mutex> lk(m);
                if (++arrived == 4) cv.notify_all();
                else cv.wait(lk, [&] { return arrived == 4; });
            }, gang);
            CHECK(rc == HQ_OK && ran == 4);
        }
    // one index alone runs on the caller and throws to it, as it always did
    bool thrown = false;
    try {
        pool.parallel_for(1, [](uint32_t) { throw std::bad_alloc(); });
    } catch (const std::bad_alloc &) {
        thrown = true;
    }
    CHECK(thrown);
    CHECK(pool.parallel_for(300, [](uint32_t) {}) == HQ_E_INVAL);
    std::printf("ok\n");
    return 0;
}
"""


def build(d, name, text, sources):
    src, exe = d / (name + ".cpp"), d / name
    src.write_text(text)
    # each unit compiled by a process of its own, at the same time; the sanitizer's runtime as the
    # compiler links it (the program's own operator new does not go with the static one)
    units = [(str(src), str(d / (name + ".o")))] + [(os.path.join(CSRC, s), str(d / (s + ".o"))) for s in sources]
    procs = [subprocess.Popen(["g++", *SANITIZE, "-c", "-o", obj, unit]) for unit, obj in units]
    assert [p.wait() for p in procs] == [0] * len(units)
    subprocess.run(["g++", *SANITIZE, "-o", str(exe)] + [obj for _, obj in units], check=True)
    return str(exe)


def test_sanitizer_wire_and_stream_entries_when_an_allocation_fails(tmp_path):
    exe = build(tmp_path, "abi_wire_guard", WIRE_CPP,
                ["hq_wire.cpp", "hq_wire_frame.cpp", "hq_stream.cpp", "hq_stream16.cpp"])
    args = []
    for fx in FIX["batches"]:
        args += [fx["name"], fx["hex"]]
    for fx in FIX["malformed"]:
        args += ["malformed " + fx["name"], fx["hex"]]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == ""
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok", r.stdout
    reps, allocs = int(last[2]), int(last[4])
    # every k of every call was run, none skipped; the calls allocate (a few hundred in all)
    assert reps == allocs and reps >= 200, r.stdout
    for what in ("add_batch: ", "add_batch attached: ", "add_locals", "attach: events queued",
                 "step_input", "step_stream", "step_sized",
                 "hq_events16_encode_sized_multi T=1", "hq_events16_encode_sized_multi T=4"):
        assert what in r.stdout, what


def test_sanitizer_task_pool_survives_a_function_that_throws(tmp_path):
    exe = build(tmp_path, "abi_task_pool", POOL_CPP, [])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=10)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "" and r.stdout == "ok\n"
