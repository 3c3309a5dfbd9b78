"""What the launchers pick: every arm of the template dispatch of the commit, lag, bitmap and
multi-ctx ReadIndex entry points, at the smallest sizes that reach it, bit-exact with the CPU
oracle (oracle/qref). It pins which kernel instance a combination of n_max, form, layout,
alignment and per-group columns selects; the kernels themselves are covered at size by
test_gpu_parity, test_gpu_tiles and test_readindex_multi.

Sizes: G = 257 for commit and lags (two full 128-group tiles plus one group: the full tile, the
partial tile, a lane's pair and its lone group), 2049 for the bitmap kernels (two 1024-group
tiles plus one group), 258 / 257 for multi-ctx ReadIndex (even: the pair kernel, odd: one group
per lane)."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import qref
from test_gpu_parity import check_commit, check_commit_lag, upload_commit
from test_gpu_tiles import _bits_tiled, run_tiled
from test_readindex_multi import _check_outputs, random_batch

pytestmark = pytest.mark.gpu

SEED = 0x5EEDD150
G_COMMIT, G_BITS = 257, 2049
FORMS = [0, 1, 2, 3]


@functools.lru_cache(maxsize=None)
def commit_inputs(n, pern, seed=0, G=G_COMMIT):
    """One generated batch per (n, per-group n); per-group voter counts cover 0 and n + 1
    (fallback) and every valid count."""
    inp = qref.CommitInputs(qref.spec(SEED + 16 * seed + n, G, n, parity_extras=True))
    if pern:
        rng = np.random.default_rng(SEED + n)
        inp.n_voting[:] = rng.integers(1, n + 1, G)
        inp.n_voting[::37] = 0
        inp.n_voting[5::41] = n + 1
    return inp


@functools.lru_cache(maxsize=None)
def commit_want(n, pern, form, seed=0, G=G_COMMIT):
    out, chg, fb, rc = commit_inputs(n, pern, seed, G).run(form, pern, nthreads=1)
    assert rc == 0
    return out, chg, fb


def assert_commit(got, want):
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


# ---- hq_commit_dev ---------------------------------------------------------------------------
@pytest.mark.parametrize("pern", [False, True])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", range(1, 9))
def test_commit_every_arm(gpu_ctx, hq, n, form, pern):
    inp = commit_inputs(n, pern)
    want = commit_want(n, pern, form)
    # 16-byte aligned columns and an even row stride: two groups per lane
    check_commit(gpu_ctx, hq, inp, form, pern, stride_pad=1)
    # every column offset by 8 bytes: the one-group-per-lane kernel
    check_commit(gpu_ctx, hq, inp, form, pern, offset_elems=1)
    for layout in (hq.HQ_LAYOUT_TILES, hq.HQ_LAYOUT_TILES_LEADER):
        assert_commit(run_tiled(gpu_ctx, hq, inp, form, pern, layout), want)


def _in_place_args(ctx, hq, inp, form, pern):
    d = upload_commit(ctx, hq, inp, form, pern)
    lay = hq.HQ_LAYOUT_TILES_LEADER
    tiles = ctx.empty(hq.commit_tiles(inp.G) * hq.commit_tile_words(inp.n_max, form, lay), np.uint64)
    ctx.tile_commit_dev(d["args"], tiles, lay)
    a = hq.CommitArgs()
    a.G, a.n_max, a.form, a.ring_len = inp.G, inp.n_max, form, inp.R
    a.layout = lay | hq.HQ_LAYOUT_IN_PLACE
    a.match, a.n_voting = tiles.ptr, d["args"].n_voting
    a.ring, a.ring32 = d["args"].ring, d["args"].ring32
    a.changed, a.fallback = d["chg"].ptr, d["fb"].ptr
    return a, tiles, d


@pytest.mark.parametrize("pern", [False, True])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", range(1, 9))
def test_commit_leader_tiles_in_place(gpu_ctx, hq, n, form, pern):
    """committed' lands in the tiles' committed row for the two forms a table holds; the ring
    forms are refused."""
    inp = commit_inputs(n, pern)
    a, tiles, d = _in_place_args(gpu_ctx, hq, inp, form, pern)
    if form in (hq.HQ_FORM_TERM_START, hq.HQ_FORM_TERM_MASK):
        gpu_ctx.commit_dev(a)
        com = gpu_ctx.empty(inp.G, np.uint64)
        gpu_ctx.table_committed_dev(tiles, inp.G, n, form, com)
        got = (gpu_ctx.download(com), gpu_ctx.download(d["chg"]), gpu_ctx.download(d["fb"]))
        gpu_ctx.free(com)
        assert_commit(got, commit_want(n, pern, form))
    else:
        assert hq.lib.hq_commit_dev(gpu_ctx.h, ctypes.byref(a)) == hq.HQ_E_INVAL
    for b in d["bufs"] + [tiles]:
        gpu_ctx.free(b)


# ---- hq_commit_lag_dev -----------------------------------------------------------------------
@pytest.mark.parametrize("lead", [False, True])
@pytest.mark.parametrize("pern", [False, True])
@pytest.mark.parametrize("form", [0, 2])
@pytest.mark.parametrize("n", range(1, 9))
def test_commit_lag_every_arm(gpu_ctx, hq, n, form, pern, lead):
    inp = commit_inputs(n, pern)
    # 16-byte aligned columns, row stride a multiple of 4: four groups per lane; else one
    for kw in (dict(stride_pad=3), dict(offset_elems=1)):
        check_commit_lag(gpu_ctx, hq, inp, form, pern, lead=lead, **kw)


def test_commit_lag_rejects_other_forms(gpu_ctx, hq):
    b = hq.alloc_commit_lag(gpu_ctx, G_COMMIT, 3, hq.HQ_FORM_TERM_START)
    a = b.args()
    for form in (hq.HQ_FORM_TERM_RING, hq.HQ_FORM_TERM_RING32):
        a.form = form
        assert hq.lib.hq_commit_lag_dev(gpu_ctx.h, ctypes.byref(a)) == hq.HQ_E_INVAL
    hq.free_commit(gpu_ctx, b)


# ---- fused launches --------------------------------------------------------------------------
# three batches with every n <= 5 (the big block where the form has one), three with one n of 7
FUSED_NS = [(1, 3, 5), (3, 7, 5)]


def _launches(ctx, call):
    ctx.sync()
    ctx.timing_reset()
    ctx.timing(True)
    call()
    ctx.sync()
    ctx.timing(False)
    return ctx.timing_read()[1]


@pytest.mark.parametrize("ns", FUSED_NS)
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("form", FORMS)
def test_commit_fused_every_arm(gpu_ctx, hq, form, layout, ns):
    """One launch over three batches = the same batches launched one by one = the oracle."""
    bufs = []
    for k, n in enumerate(ns):
        b = hq.alloc_commit(gpu_ctx, G_COMMIT, n, form, 16, tiled=layout != 0,
                            tile_layout=layout or hq.HQ_LAYOUT_TILES)
        inp = commit_inputs(n, False, seed=k + 1)
        d = upload_commit(gpu_ctx, hq, inp, form, False, stride_pad=1)   # even: fusable
        a = d["args"]
        a.committed_out, a.changed, a.fallback = b.committed_out.ptr, b.changed.ptr, b.fallback.ptr
        if layout:
            gpu_ctx.tile_commit_dev(a, b.tiles, layout)
            a.layout, a.match, a.match_stride = layout, b.tiles.ptr, 0
            a.committed_in = a.last_index = a.term_start = a.term = a.term_mask = None
        bufs.append((b, d, a))
    batch = hq.commit_batch_array([a for _, _, a in bufs])

    def outputs():
        return [[gpu_ctx.download(x) for x in (b.committed_out, b.changed, b.fallback)]
                for b, _, _ in bufs]

    assert _launches(gpu_ctx, lambda: gpu_ctx.commit_many_dev(batch)) == len(ns)
    one_by_one = outputs()
    for b, _, _ in bufs:
        for x in (b.committed_out, b.changed, b.fallback):
            gpu_ctx.memset(x, 0xFF)
    assert _launches(gpu_ctx, lambda: gpu_ctx.commit_fused_dev(batch)) == 1
    fused = outputs()
    for k, n in enumerate(ns):
        assert_commit(fused[k], one_by_one[k])
        assert_commit(fused[k], commit_want(n, False, form, seed=k + 1))
    for b, d, _ in bufs:
        hq.free_commit(gpu_ctx, b)
        for x in d["bufs"]:
            gpu_ctx.free(x)


@pytest.mark.parametrize("ns", [(1, 3, 4), (3, 7, 4)])
@pytest.mark.parametrize("lead", [False, True])
@pytest.mark.parametrize("form", [0, 2])
def test_commit_lag_fused_every_arm(gpu_ctx, hq, form, lead, ns):
    bufs = []
    for k, n in enumerate(ns):
        b = hq.alloc_commit_lag(gpu_ctx, G_COMMIT, n, form, 16, with_last=True)
        gpu_ctx.synth_commit_lag_dev(hq.synth_spec(SEED + 90 + k, G_COMMIT, n, parity_extras=True),
                                     b.args(), b.last_index)
        bufs.append((b, qref.CommitInputs(qref.spec(SEED + 90 + k, G_COMMIT, n,
                                                    parity_extras=True))))
    batch = hq.lag_batch_array([b.args(lead) for b, _ in bufs])

    def outputs():
        return [[gpu_ctx.download(x) for x in (b.cout_lag, b.changed, b.fallback)]
                for b, _ in bufs]

    def one_by_one():
        for a in batch:
            gpu_ctx.commit_lag_dev(a)

    assert _launches(gpu_ctx, one_by_one) == len(ns)
    alone = outputs()
    for b, _ in bufs:
        for x in (b.cout_lag, b.changed, b.fallback):
            gpu_ctx.memset(x, 0xFF)
    assert _launches(gpu_ctx, lambda: gpu_ctx.commit_lag_fused_dev(batch)) == 1
    for (b, inp), got, want in zip(bufs, outputs(), alone):
        assert_commit(got, want)
        com = inp.committed_in.copy()
        hq.unpack_lags(inp.last_index, got[0], com, got[2])
        assert_commit((com, got[1], got[2]), inp.run(form, False)[:3])
        hq.free_commit(gpu_ctx, b)


def test_commit_lag_fused_takes_at_most_eight(gpu_ctx, hq):
    """A fused lag launch holds 2..8 batches (include/hipquorum.h): eight share one launch, nine
    fusable ones are launched one by one, with the same results."""
    form, ns = hq.HQ_FORM_TERM_START, (1, 2, 3, 4, 5, 6, 7, 8, 3)
    bufs = []
    for k, n in enumerate(ns):
        b = hq.alloc_commit_lag(gpu_ctx, G_COMMIT, n, form, 16, with_last=True)
        gpu_ctx.synth_commit_lag_dev(hq.synth_spec(SEED + 120 + k, G_COMMIT, n, parity_extras=True),
                                     b.args(), b.last_index)
        bufs.append((b, qref.CommitInputs(qref.spec(SEED + 120 + k, G_COMMIT, n,
                                                    parity_extras=True))))
    for count in (8, 9):
        batch = hq.lag_batch_array([b.args() for b, _ in bufs[:count]])
        for b, _ in bufs:
            for x in (b.cout_lag, b.changed, b.fallback):
                gpu_ctx.memset(x, 0xFF)
        launches = _launches(gpu_ctx, lambda: gpu_ctx.commit_lag_fused_dev(batch))
        assert launches == (1 if count == 8 else 9)
        for b, inp in bufs[:count]:
            fb = gpu_ctx.download(b.fallback)
            com = inp.committed_in.copy()
            hq.unpack_lags(inp.last_index, gpu_ctx.download(b.cout_lag), com, fb)
            assert_commit((com, gpu_ctx.download(b.changed), fb), inp.run(form, False)[:3])
    for b, _ in bufs:
        hq.free_commit(gpu_ctx, b)


# ---- launch_bits: ReadIndex / vote / CheckQuorum over u8 columns and byte tiles ---------------
@functools.lru_cache(maxsize=None)
def bitmap_inputs(pern):
    inp = qref.BitmapInputs(qref.spec(SEED + pern, G_BITS, 8 if pern else 7, mixed_n=pern,
                                      parity_extras=True))
    if pern:
        inp.n_voting[::53] = 0
        inp.n_voting[7::59] = 9
    return inp


@pytest.mark.parametrize("pern", [False, True])
@pytest.mark.parametrize("mode", ["readindex", "vote", "readindex_vote", "check_quorum"])
def test_bits_columns_every_arm(gpu_ctx, hq, mode, pern):
    inp, G = bitmap_inputs(pern), G_BITS
    nv, nu = (inp.n_voting, 0) if pern else (None, 7)
    d = {k: gpu_ctx.upload(v) for k, v in (("ack", inp.ack), ("gr", inp.granted),
                                           ("rj", inp.rejected), ("nv", inp.n_voting))}
    dn = d["nv"] if pern else None
    conf, hasq, fb = (gpu_ctx.empty(hq.words64(G), np.uint64) for _ in range(3))
    outc = gpu_ctx.empty(hq.words32(G), np.uint64)
    for x in (conf, hasq, fb, outc):
        gpu_ctx.memset(x, 0xFF)
    want_conf, want_fb = qref.readindex_batch(inp.ack, nv, nu)
    want_out, want_fb2 = qref.vote_batch(inp.granted, inp.rejected, nv, nu)
    if mode == "readindex":
        gpu_ctx.readindex_dev(G, d["ack"], dn, nu, conf, fb)
        np.testing.assert_array_equal(gpu_ctx.download(conf), want_conf)
    elif mode == "vote":
        gpu_ctx.vote_dev(G, d["gr"], d["rj"], dn, nu, outc, fb)
        np.testing.assert_array_equal(gpu_ctx.download(outc), want_out)
    elif mode == "readindex_vote":
        gpu_ctx.readindex_vote_dev(G, d["ack"], d["gr"], d["rj"], dn, nu, conf, outc, fb)
        np.testing.assert_array_equal(gpu_ctx.download(conf), want_conf)
        np.testing.assert_array_equal(gpu_ctx.download(outc), want_out)
        np.testing.assert_array_equal(want_fb, want_fb2)
    else:   # the ack column as the active flags, self slot 1
        want_hq, want_fb, want_active = qref.check_quorum_batch(inp.ack, nv, nu, 1)
        gpu_ctx.check_quorum_dev(G, d["ack"], dn, nu, 1, hasq, fb)
        np.testing.assert_array_equal(gpu_ctx.download(hasq), want_hq)
        np.testing.assert_array_equal(gpu_ctx.download(d["ack"]), want_active)
    np.testing.assert_array_equal(gpu_ctx.download(fb), want_fb)
    for x in list(d.values()) + [conf, hasq, fb, outc]:
        gpu_ctx.free(x)


@pytest.mark.parametrize("with_fb", [True, False])
@pytest.mark.parametrize("pern", [False, True])
def test_bits_tiles_every_arm(gpu_ctx, hq, pern, with_fb):
    """3-row (uniform n) and 4-row (per-group n) tiles, with and without a fallback array."""
    inp, G = bitmap_inputs(pern), G_BITS
    nv, nu = (inp.n_voting, 0) if pern else (None, 7)
    want_conf, want_fb = qref.readindex_batch(inp.ack, nv, nu)
    want_out, _ = qref.vote_batch(inp.granted, inp.rejected, nv, nu)
    if with_fb:
        conf, outc, fb = _bits_tiled(gpu_ctx, hq, inp, G, pern, nu)
        np.testing.assert_array_equal(fb, want_fb)
    else:
        cols = [gpu_ctx.upload(a) if a is not None else None
                for a in (inp.ack, inp.granted, inp.rejected, nv)]
        tiles = gpu_ctx.empty(hq.bits_tile_bytes(G, pern), np.uint8)
        gpu_ctx.tile_bits_dev(G, *cols, tiles)
        dc, do = gpu_ctx.empty(hq.words64(G), np.uint64), gpu_ctx.empty(hq.words32(G), np.uint64)
        gpu_ctx.readindex_vote_tiles_dev(G, tiles, pern, nu, dc, do, None)
        conf, outc = gpu_ctx.download(dc), gpu_ctx.download(do)
        for x in [c for c in cols if c is not None] + [tiles, dc, do]:
            gpu_ctx.free(x)
    np.testing.assert_array_equal(conf, want_conf)
    np.testing.assert_array_equal(outc, want_out)


# ---- multi-ctx ReadIndex ---------------------------------------------------------------------
RI_N_MAX = 5


def _ri_case(K_max, n_max, G, perk, pern, nu=None):
    rng = np.random.default_rng(SEED + 1000 * K_max + 10 * n_max + G)
    ord_, idx, K, n = random_batch(rng, G, K_max, n_max)
    if pern:
        n[::97] = 0
    idx.reshape(K_max, G)[:, 5] = np.arange(K_max, 0, -1)   # decreasing (K_max > 1): fallback
    Kp, nv = (K if perk else None), (n if pern else None)
    nu = 0 if pern else (n_max if nu is None else nu)
    want = qref.readindex_multi_batch(ord_, idx, Kp, nv, nu, K_max, n_max)
    return ord_, idx, Kp, nv, nu, want


def _ri_outputs(ctx, hq, K_max, G):
    rel, cnt = ctx.empty(K_max * G, np.uint64), ctx.empty(G, np.uint8)
    bend, fb = ctx.empty(G, np.uint8), ctx.empty(hq.words64(G), np.uint64)
    ctx.memset(fb, 0xFF)
    return rel, cnt, bend, fb


@pytest.mark.parametrize("G", [258, 257])
@pytest.mark.parametrize("pern", [False, True])
@pytest.mark.parametrize("perk", [False, True])
@pytest.mark.parametrize("K_max", [1, 2, 3, 4, 8])
def test_ri_multi_columns_every_arm(gpu_ctx, hq, K_max, perk, pern, G):
    """Even G: the pair kernel with 2, 4 or 8 ctx slots; odd G: one group per lane."""
    ord_, idx, Kp, nv, nu, want = _ri_case(K_max, RI_N_MAX, G, perk, pern)
    d = [gpu_ctx.upload(x) if x is not None else None for x in (ord_, idx, Kp, nv)]
    rel, cnt, bend, fb = _ri_outputs(gpu_ctx, hq, K_max, G)
    gpu_ctx.readindex_multi_dev(G, K_max, RI_N_MAX, d[0], d[1], d[2], d[3], nu, rel, cnt, fb, bend)
    _check_outputs(gpu_ctx, hq, K_max, idx, rel, cnt, fb, bend, False, want)
    for x in [x for x in d if x is not None] + [rel, cnt, bend, fb]:
        gpu_ctx.free(x)


def _ri_tiles(ctx, hq, K_max, n_max, G, perk, pern, nu=None):
    ord_, idx, Kp, nv, nu, want = _ri_case(K_max, n_max, G, perk, pern, nu)
    tiles_h, flags = hq.tile_ri_multi_host(G, K_max, n_max, ord_, idx, Kp, nv)
    dt = ctx.upload(tiles_h)
    rel, cnt, bend, fb = _ri_outputs(ctx, hq, K_max, G)
    rc = hq.lib.hq_readindex_multi_tiles_dev(ctx.h, G, K_max, n_max, dt.ptr, flags, nu, rel.ptr,
                                             cnt.ptr, bend.ptr, fb.ptr)
    if rc == hq.HQ_OK:
        _check_outputs(ctx, hq, K_max, idx, rel, cnt, fb, bend, False, want)
    for x in (dt, rel, cnt, bend, fb):
        ctx.free(x)
    return rc


@pytest.mark.parametrize("pern", [False, True])
@pytest.mark.parametrize("perk", [False, True])
@pytest.mark.parametrize("K_max", [1, 2, 3, 4, 8])
def test_ri_multi_tiles_every_arm(gpu_ctx, hq, K_max, perk, pern):
    """K_max in {2, 4, 8} reads a voter's ctx dwords as vectors, 1 and 3 dword by dword; the
    uniform case (no per-group column, n = n_max) of {2, 4, 8} runs k_ri_tiles_u."""
    assert _ri_tiles(gpu_ctx, hq, K_max, RI_N_MAX, 258, perk, pern) == hq.HQ_OK
    # odd G: the pair kernel's 16-byte column stores have no aligned rows
    assert _ri_tiles(gpu_ctx, hq, K_max, RI_N_MAX, 257, perk, pern) == hq.HQ_E_INVAL


@pytest.mark.parametrize("K_max", [1, 2, 3, 4, 8])
def test_ri_multi_tiles_uniform_below_n_max(gpu_ctx, hq, K_max):
    """n_uniform < n_max leaves k_ri_tiles_u for the general pair kernel."""
    assert _ri_tiles(gpu_ctx, hq, K_max, RI_N_MAX, 258, False, False, nu=3) == hq.HQ_OK


@pytest.mark.parametrize("n_max", range(1, 9))
@pytest.mark.parametrize("K_max", [2, 4, 8])
def test_ri_multi_tiles_uniform_every_n(gpu_ctx, hq, K_max, n_max):
    """k_ri_tiles_u has one instance per (K_max, n_max)."""
    assert _ri_tiles(gpu_ctx, hq, K_max, n_max, 258, False, False) == hq.HQ_OK
