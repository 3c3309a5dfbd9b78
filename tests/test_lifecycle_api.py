"""The group-lifecycle entries of the ABI without a device (include/hipquorum.h "group
lifecycle"): the header declares them, the built library exports them, the refusals that need no
worker, and the invariants of the handle model the GPU tests hold the workers to."""
import ctypes
import os
import re

import numpy as np

import lifecycle_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hipquorum.h")
ENTRIES = ("hq_worker_start_groups", "hq_worker_stop_groups", "hq_worker_pool_info", "hq_worker_compact")
FIELDS = ("handles", "live_groups", "vacant_handles", "member_records", "live_member_records", "epoch")


def header_text():
    s = open(HEADER).read()
    return re.sub(r"/\*.*?\*/", " ", s, flags=re.S)


def test_header_declares_the_entries_and_the_struct():
    s = " ".join(header_text().split())
    assert ("int hq_worker_start_groups(hq_worker *w, uint64_t n, const hq_worker_group *groups, "
            "const hq_member *members, uint32_t *handles , uint64_t *gpu_ns );") in s
    assert "int hq_worker_stop_groups(hq_worker *w, uint64_t n, const uint32_t *handles, uint64_t *gpu_ns);" in s
    assert "int hq_worker_compact(hq_worker *w, uint64_t *gpu_ns);" in s
    m = re.search(r"typedef struct hq_worker_pool_info \{(.*?)\} (\w+);", s)
    assert m, "struct hq_worker_pool_info"
    names = re.findall(r"(\w+)\s*[,;]", m.group(1))
    assert tuple(names) == FIELDS
    assert all(t == "uint64_t" for t in re.findall(r"(\w+) \w+(?:, \w+)*;", m.group(1)))
    assert "int hq_worker_pool_info(hq_worker *w, %s *out);" % m.group(2) in s
    assert re.search(r"#define HQ_ABI_VERSION 21u?\b", s)      # new symbols only: still ABI 21


def test_library_exports_them_and_the_binding_lists_them(hq):
    for name in ENTRIES:
        assert getattr(hq.lib, name) is not None
        assert name in hq.SIGNATURES
    assert [n for n, _ in hq.PoolInfo._fields_] == list(FIELDS)
    assert ctypes.sizeof(hq.PoolInfo) == 48
    for method in ("start_groups", "stop_groups", "pool_info", "compact"):
        assert callable(getattr(hq.Worker, method))


def test_refusals_without_a_worker(hq):
    lib, inval = hq.lib, hq.HQ_E_INVAL
    g = np.zeros(1, hq.WORKER_GROUP_DTYPE)
    m = np.zeros(1, hq.MEMBER_DTYPE)
    h = np.zeros(1, np.uint32)
    ns = ctypes.c_uint64(7)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.hq_worker_start_groups(None, 1, vp(g), vp(m), vp(h), ctypes.byref(ns)) == inval
    assert lib.hq_worker_start_groups(None, 0, None, None, None, None) == inval
    assert lib.hq_worker_stop_groups(None, 1, vp(h), ctypes.byref(ns)) == inval
    assert lib.hq_worker_stop_groups(None, 0, None, None) == inval
    info = hq.PoolInfo()
    assert lib.hq_worker_pool_info(None, ctypes.byref(info)) == inval
    assert lib.hq_worker_pool_info(None, None) == inval
    assert lib.hq_worker_compact(None, ctypes.byref(ns)) == inval
    assert lib.hq_worker_compact(None, None) == inval
    assert ns.value == 7 and int(h[0]) == 0          # nothing written


def test_handle_model_invariants():
    rng = np.random.default_rng(5)
    md = lm.HandleModel()
    assert md.start([10, 11, 12, 13]) == [0, 1, 2, 3]
    md.stop([1, 3, 0])
    assert md.vacant == [1, 3, 0] and md.live() == [2] and md.handles == 4
    assert md.start([20, 21]) == [0, 3]              # the most recently vacated first
    assert md.start([22, 23]) == [1, 4]              # then the next new handle
    assert md.find(22) == 1 and md.live_cids() == [20, 22, 12, 21, 23]
    next_cid, top = 100, md.handles
    for _ in range(200):
        live = md.live()
        k = int(rng.integers(0, min(6, len(live)) + 1))
        stop = [int(x) for x in rng.choice(live, k, replace=False)] if k else []
        vac0, e0 = list(md.vacant), md.epoch
        md.stop(stop)
        assert md.vacant == vac0 + stop and md.epoch == e0 + (1 if stop else 0)
        n = int(rng.integers(0, 7))
        vac1 = list(md.vacant)
        got = md.start(list(range(next_cid, next_cid + n)))
        next_cid += n
        reuse = min(n, len(vac1))
        assert got[:reuse] == vac1[::-1][:reuse]                     # LIFO
        assert got[reuse:] == list(range(top, top + n - reuse))      # then new handles, in order
        assert md.handles >= top                                     # the space never shrinks
        top = md.handles
        assert sorted(md.live() + md.vacant) == list(range(top))
        assert len(set(md.live_cids())) == len(md.live())
