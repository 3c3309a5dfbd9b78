"""The exception guard of the step worker's C entries without a GPU:
dragonboat_amd/csrc/hq_guard.h — the one template every entry of hq_worker*.cpp and hq_jobs.cpp
runs its body in — compiled into a program of its own with -fsanitize=address,undefined. A body's
code passes through unchanged with nothing recorded; a body that throws gives the code and the
message of the header's table, under the entry's name. No Python process loads sanitized code."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GUARD_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hq_guard.h"

static unsigned checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { std::printf("FAILED %s line %d\n", #c, __LINE__); std::exit(1); } } while (0)

struct Recorded {                                    // what a worker's fail() keeps
    int code = 12345, calls = 0;
    std::string msg = "untouched";
};

template <class Body>
static int run(const char *entry, Recorded &r, Body body) {
    return hq::guard(entry, [&r](int code, const std::string &m) {
        r.code = code;
        r.msg = m;
        ++r.calls;
    }, body);
}

struct NotStd { int x; };

int main() {
    {
        auto rec = [](int, const std::string &) {};
        auto body = [] { return 0; };
        static_assert(noexcept(hq::guard("e", rec, body)), "nothing leaves the guard");
        CHECK(hq::guard("e", rec, body) == 0);
    }
    // a body's own code comes back unchanged and records nothing
    const int codes[] = {HQ_OK, HQ_E_INVAL, HQ_E_NOMEM, HQ_E_STATE, -2, -5, -6, 1 << 30, 7};
    for (int c : codes) {
        Recorded r;
        CHECK(run("hq_worker_step", r, [c] { return c; }) == c);
        CHECK(r.calls == 0 && r.code == 12345 && r.msg == "untouched");
    }
    // the table, under two entries' names
    for (const char *entry : {"hq_worker_step", "hq_worker_add_groups"}) {
        const std::string e(entry);
        Recorded r;
        CHECK(run(entry, r, []() -> int { throw std::bad_alloc(); }) == HQ_E_NOMEM);
        CHECK(r.calls == 1 && r.code == HQ_E_NOMEM && r.msg == e + ": out of memory");
        r = Recorded();
        CHECK(run(entry, r, []() -> int { throw std::length_error("vector::reserve"); }) == HQ_E_NOMEM);
        CHECK(r.calls == 1 && r.code == HQ_E_NOMEM && r.msg == e + ": out of memory");
        r = Recorded();
        const std::system_error se(std::make_error_code(std::errc::resource_unavailable_try_again),
                                   "thread spawn");
        CHECK(run(entry, r, [&se]() -> int { throw se; }) == HQ_E_NOMEM);
        CHECK(r.calls == 1 && r.code == HQ_E_NOMEM && r.msg == e + ": " + se.what());
        CHECK(r.msg.find("thread spawn") != std::string::npos);
        r = Recorded();
        CHECK(run(entry, r, []() -> int { throw NotStd{3}; }) == HQ_E_STATE);
        CHECK(r.calls == 1 && r.code == HQ_E_STATE && r.msg == e + ": unexpected exception");
        r = Recorded();
        CHECK(run(entry, r, []() -> int { throw 42; }) == HQ_E_STATE);
        CHECK(r.msg == e + ": unexpected exception");
        // (std exceptions outside the table are "anything else"; a subclass of a listed one is its
        // base: future_error is a logic_error, not a system_error)
        r = Recorded();
        CHECK(run(entry, r, []() -> int { throw std::out_of_range("at"); }) == HQ_E_STATE);
        CHECK(r.msg == e + ": unexpected exception");
        r = Recorded();
        CHECK(run(entry, r, []() -> int { throw std::bad_array_new_length(); }) == HQ_E_NOMEM);
        CHECK(r.msg == e + ": out of memory");
    }
    // the real thing: a vector asked for more than max_size
    {
        Recorded r;
        std::vector<char> v;
        CHECK(run("hq_worker_step_stream", r, [&v]() -> int { v.reserve(v.max_size() + 1); return 0; })
              == HQ_E_NOMEM);
        CHECK(r.msg == "hq_worker_step_stream: out of memory");
    }
    // a recorder that throws itself: the code still comes back, nothing escapes
    CHECK(hq::guard("e", [](int, const std::string &) { throw std::bad_alloc(); },
                    []() -> int { throw std::bad_alloc(); }) == HQ_E_NOMEM);
    // what the body built is unwound before the guard returns
    {
        static int live = 0;
        struct Live { Live() { ++live; } ~Live() { --live; } };
        Recorded r;
        CHECK(run("e", r, []() -> int { Live a, b; throw std::bad_alloc(); }) == HQ_E_NOMEM && live == 0);
    }
    std::printf("ok %u\n", checks);
    return 0;
}
"""


@pytest.fixture(scope="module")
def guard_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("abi_guard")
    src, exe = d / "abi_guard.cpp", d / "abi_guard"
    src.write_text(GUARD_CPP)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "dragonboat_amd", "csrc"), "-o", str(exe), str(src)],
                   check=True)
    return str(exe)


def test_sanitizer_guard_codes_and_messages_stand_alone(guard_program):
    r = subprocess.run([guard_program], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "" and r.stdout.startswith("ok ")
    assert int(r.stdout.split()[1]) == 53          # every CHECK of the program ran
