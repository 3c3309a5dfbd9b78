"""The packed group record of hq_worker_get_groups / hq_worker_set_groups without a GPU:
dragonboat_amd/csrc/hq_groups.h — the one source the host side of both calls, the device kernels
and this check share — compiled into a program of its own with -fsanitize=address,undefined.
pack -> unpack is the identity, every packed byte beyond the used reads and members is zero, and
the mapping of a slot bitmap to list positions is exact against a naive loop. No Python process
loads sanitized code."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GROUPS_CPP = r"""
// Records are heap arrays of exactly their size, so an access beyond the used reads or members is
// the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hq_groups.h"

static unsigned long long checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { std::printf("FAILED %s line %d\n", #c, __LINE__); std::exit(1); } } while (0)

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {                              // splitmix64
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static void fill(void *p, size_t n) {
    unsigned char *b = static_cast<unsigned char *>(p);
    for (size_t i = 0; i < n; ++i) b[i] = (unsigned char)rnd();
}

int main() {
    static_assert(kGrpRecordBytes == 768 && kGrpRecordWords == 48, "the record");
    // pack -> unpack over random records with 1 .. 16 members and 0 .. 8 reads
    for (unsigned nm = 1; nm <= kDMembers; ++nm)
        for (unsigned nr = 0; nr <= kDReads; ++nr)
            for (int rep = 0; rep < 20; ++rep) {
                hq_dgroup g;
                fill(&g, sizeof g);
                g.n_members = (uint8_t)nm;
                g.n_reads = (uint8_t)nr;
                std::vector<hq_dread> reads(nr), reads2(nr);
                std::vector<hq_dmember> mem(nm), mem2(nm);
                if (nr) fill(reads.data(), nr * sizeof(hq_dread));
                fill(mem.data(), nm * sizeof(hq_dmember));
                hq_grp_record *rec = new hq_grp_record;
                fill(rec, sizeof *rec);              // pack must overwrite every byte
                grp_pack(*rec, g, reads.data(), mem.data());
                const unsigned char *b = reinterpret_cast<const unsigned char *>(rec);
                CHECK(std::memcmp(b, &g, sizeof g) == 0);
                CHECK(nr == 0 || std::memcmp(b + 64, reads.data(), nr * sizeof(hq_dread)) == 0);
                CHECK(std::memcmp(b + 64 + 320, mem.data(), nm * sizeof(hq_dmember)) == 0);
                for (size_t i = 64 + nr * sizeof(hq_dread); i < 64 + 320; ++i) CHECK(b[i] == 0);
                for (size_t i = 64 + 320 + nm * sizeof(hq_dmember); i < kGrpRecordBytes; ++i) CHECK(b[i] == 0);
                hq_dgroup g2;
                CHECK(grp_unpack(*rec, g2, reads2.data(), mem2.data()));
                CHECK(std::memcmp(&g2, &g, sizeof g) == 0);
                CHECK(nr == 0 || std::memcmp(reads2.data(), reads.data(), nr * sizeof(hq_dread)) == 0);
                CHECK(std::memcmp(mem2.data(), mem.data(), nm * sizeof(hq_dmember)) == 0);
                CHECK(grp_fits(g.mem, nm, nr, (uint64_t)g.mem + nm));
                CHECK(!grp_fits(g.mem, nm, nr, (uint64_t)g.mem + nm - 1));
                delete rec;
            }
    // counts beyond the record's arrays are refused before anything is indexed
    {
        hq_grp_record *rec = new hq_grp_record();
        hq_dgroup g;
        rec->g.n_members = kDMembers + 1;
        CHECK(!grp_unpack(*rec, g, nullptr, nullptr));
        rec->g.n_members = 1;
        rec->g.n_reads = kDReads + 1;
        CHECK(!grp_unpack(*rec, g, nullptr, nullptr));
        CHECK(!grp_fits(0, kDMembers + 1, 0, 1000) && !grp_fits(0, 1, kDReads + 1, 1000));
        CHECK(!grp_fits(0xFFFFFFFFu, 1, 0, 0xFFFFFFFFull) && grp_fits(0xFFFFFFFFu, 1, 0, 0x100000000ull));
        delete rec;
    }
    // slot bitmap -> list positions: every n_voting, every 8-bit mask, random list orders
    for (unsigned nv = 1; nv <= HQ_MAX_VOTERS; ++nv)
        for (int rep = 0; rep < 24; ++rep) {
            const unsigned n = nv + (unsigned)(rnd() % (kDMembers - nv + 1));
            std::vector<hq_dmember> mem(n);           // exactly n records: slot >= n is out of bounds
            std::vector<unsigned> perm(n);
            for (unsigned i = 0; i < n; ++i) perm[i] = i;
            for (unsigned i = n; i > 1; --i) std::swap(perm[i - 1], perm[rnd() % i]);
            for (unsigned i = 0; i < n; ++i) {
                mem[i] = hq_dmember{};
                mem[i].order = (uint8_t)perm[i];
            }
            for (unsigned bits = 0; bits < 256; ++bits) {
                unsigned want = 0;
                for (unsigned pos = 0; pos < n; ++pos)      // list position pos is pool slot s
                    for (unsigned s = 0; s < nv; ++s)
                        if (perm[s] == pos && ((bits >> s) & 1)) want |= 1u << pos;
                const unsigned got = grp_slots_to_list(bits, nv, mem.data());
                CHECK(got == want);
                CHECK(__builtin_popcount(got) == __builtin_popcount(bits & ((1u << nv) - 1)));
            }
        }
    std::printf("ok %llu\n", checks);
    return 0;
}
"""


@pytest.fixture(scope="module")
def groups_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("groups_ref")
    src, exe = d / "groups_ref.cpp", d / "groups_ref"
    src.write_text(GROUPS_CPP)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "dragonboat_amd", "csrc"), "-o", str(exe), str(src)],
                   check=True)
    return str(exe)


def test_sanitizer_pack_unpack_and_masks_stand_alone(groups_program):
    r = subprocess.run([groups_program], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "" and r.stdout.startswith("ok ")
    assert int(r.stdout.split()[1]) >= 100000
