"""The second and later grid-stride passes of every kernel whose grid grid_for() sizes.

The grid cap (kMaxBlocks = 16384 blocks of 256 threads) is reached only beyond 4 M lanes, so at
test sizes no kernel loops. A context opened under HQ_MAX_BLOCKS=4 (read at hq_open) caps every
such launch at 1024 threads (the commit streams: the same 1024 threads in one or two blocks), and
a few thousand groups then take three passes and more, ragged last pass included. Every case is
bit-exact against the oracle, through the helpers of the parent tests."""
import numpy as np
import pytest

import test_bits3 as bits3
import test_gpu_parity as par
import test_gpu_tiles as til
from oracle import qref
from test_gpu_ri_multi_edges import make_case, open_context, run_columns, run_tiles, seed_of

pytestmark = pytest.mark.gpu

SEED = 0x5EED0000
G = 5003
FUSED = [(3, 5003), (5, 4099), (7, 2049)]


@pytest.fixture(scope="module")
def ctx4(hq):
    ctx = open_context(hq, HQ_MAX_BLOCKS=4)
    try:
        yield ctx
    finally:
        ctx.close()


# ---- multi-ctx ReadIndex: 2048 groups a pass on the pair kernels, 1024 on the one-group kernel
@pytest.mark.parametrize("perk,pern", [(True, True), (False, False)])
@pytest.mark.parametrize("compact", [False, True])
def test_ri_multi_columns_in_passes(ctx4, hq, perk, pern, compact):
    """G = 4098 on k_ri_multi2: three passes, the last holding 2 groups; G = 4097 on k_ri_multi:
    five passes."""
    for Gr in (4098, 4097):
        for K_max, n_max, nu in ((3, 5, 5), (8, 8, 4)):
            case = make_case(seed_of(6, Gr, K_max, perk, pern), Gr, K_max, n_max, perk, pern, nu)
            run_columns(ctx4, hq, case, Gr, K_max, n_max, compact)


@pytest.mark.parametrize("K_max,n_max,nu,perk,pern", [(4, 5, 5, False, False),    # k_ri_tiles_u
                                                      (4, 5, 2, False, False),    # tiles, exact
                                                      (8, 8, 8, False, False),
                                                      (3, 7, 0, True, True),      # tiles, dwords
                                                      (5, 3, 3, True, False)])
@pytest.mark.parametrize("compact", [False, True])
def test_ri_multi_tiles_in_passes(ctx4, hq, K_max, n_max, nu, perk, pern, compact):
    """The three tile routes at G = 4098 (33 tiles: three passes of 16 waves, the last tile
    holding 2 groups), and the tile packer (one thread per 16 bytes: tens of passes)."""
    case = make_case(seed_of(7, K_max, n_max, nu), 4098, K_max, n_max, perk, pern, nu)
    run_tiles(ctx4, hq, case, 4098, K_max, n_max, compact)


# ---- commit: 1024 threads a pass, two groups per lane on the 16-byte path
@pytest.mark.parametrize("form", par.FORMS)
def test_commit_columns_in_passes(ctx4, hq, form):
    inp = qref.CommitInputs(qref.spec(SEED + 70, G, 5, parity_extras=True))
    _, chg, _ = par.check_commit(ctx4, hq, inp, form, per_group_n=False)
    assert 0 < par.popcount(chg) < G
    par.check_commit(ctx4, hq, inp, form, per_group_n=False, stride_pad=1)      # 8-byte path
    inp8 = qref.CommitInputs(qref.spec(SEED + 71, G, 8, mixed_n=True, parity_extras=True))
    par.check_commit(ctx4, hq, inp8, form, per_group_n=True)
    par.check_commit(ctx4, hq, inp8, form, per_group_n=True, stride_pad=1)


@pytest.mark.parametrize("form", par.FORMS)
@pytest.mark.parametrize("layout", [1, 2])
def test_commit_tiles_in_passes(ctx4, hq, form, layout):
    """Plain and leader-row tiles (40 tiles over 16 waves), and the tile packer."""
    for n, mixed in ((5, False), (8, True)):
        inp = qref.CommitInputs(qref.spec(SEED + 72 + n, G, n, mixed_n=mixed, parity_extras=True))
        out, chg, fb = til.run_tiled(ctx4, hq, inp, form, mixed, layout)
        want_out, want_chg, want_fb, rc = inp.run(form, mixed, nthreads=8)
        assert rc == 0
        np.testing.assert_array_equal(out, want_out)
        np.testing.assert_array_equal(chg, want_chg)
        np.testing.assert_array_equal(fb, want_fb)


@pytest.mark.parametrize("form", [0, 2])
@pytest.mark.parametrize("lead", [False, True])
def test_commit_lag_in_passes(ctx4, hq, form, lead):
    """The lag stream: four groups per lane on the vector path, one on the 4-byte path."""
    inp = qref.CommitInputs(qref.spec(SEED + 80, G, 5, parity_extras=True))
    chg = par.check_commit_lag(ctx4, hq, inp, form, per_group_n=False, lead=lead)
    assert 0 < par.popcount(chg) < G
    par.check_commit_lag(ctx4, hq, inp, form, per_group_n=False, lead=lead, stride_pad=1)
    inp8 = qref.CommitInputs(qref.spec(SEED + 81, G, 8, mixed_n=True, parity_extras=True))
    par.check_commit_lag(ctx4, hq, inp8, form, per_group_n=True, lead=lead)


@pytest.mark.parametrize("form", [0, 2])
def test_fused_launches_in_passes(ctx4, hq, form):
    """One commit_fused_dev and one commit_lag_fused_dev of three buckets: every bucket's block
    range is capped on its own and strides over its own groups."""
    par.test_commit_fused_buckets(ctx4, hq, form, FUSED)
    par.test_commit_lag_fused_buckets(ctx4, hq, form, FUSED, False)


# ---- bitmaps
def _bits_want(inp, pern, nu):
    nv = inp.n_voting if pern else None
    conf, fb = qref.readindex_batch(inp.ack, nv, nu)
    outc, fb2 = qref.vote_batch(inp.granted, inp.rejected, nv, nu)
    np.testing.assert_array_equal(fb, fb2)
    return conf, outc, fb


@pytest.mark.parametrize("pern", [True, False])
def test_bitmap_columns_in_passes(ctx4, hq, pern):
    """readindex_vote_dev at G = 70 001: 16 groups per lane, five passes."""
    Gb, n = 70_001, 8 if pern else 7
    nu = 0 if pern else n
    inp = qref.BitmapInputs(qref.spec(SEED + 90 + pern, Gb, n, mixed_n=pern, parity_extras=True))
    cols = [ctx4.upload(a) if a is not None else None
            for a in (inp.ack, inp.granted, inp.rejected, inp.n_voting if pern else None)]
    conf = ctx4.empty(hq.words64(Gb), np.uint64)
    outc = ctx4.empty(hq.words32(Gb), np.uint64)
    fb = ctx4.empty(hq.words64(Gb), np.uint64)
    for x in (conf, outc, fb):
        ctx4.memset(x, 0xFF)
    ctx4.readindex_vote_dev(Gb, *cols, nu, conf, outc, fb)
    want = _bits_want(inp, pern, nu)
    for got, w in zip((conf, outc, fb), want):
        np.testing.assert_array_equal(ctx4.download(got), w)
    for x in [c for c in cols if c is not None] + [conf, outc, fb]:
        ctx4.free(x)


@pytest.mark.parametrize("pern", [True, False])
def test_bitmap_tiles_in_passes(ctx4, hq, pern):
    """k_bits over 1024-group tiles, one tile per wave: 69 tiles over 16 waves, five passes; the
    packer with them."""
    Gb, n = 70_001, 8 if pern else 7
    nu = 0 if pern else n
    inp = qref.BitmapInputs(qref.spec(SEED + 92 + pern, Gb, n, mixed_n=pern, parity_extras=True))
    got = til._bits_tiled(ctx4, hq, inp, Gb, pern, nu)
    for g, w in zip(got, _bits_want(inp, pern, nu)):
        np.testing.assert_array_equal(g, w)


def test_bitmap_tiles3_and_planes_in_passes(ctx4, hq):
    """k_bits3 takes two 1024-group tiles per wave and pass (69 tiles: 32, 32 and 5, the last wave
    with one tile of its two), k_planes one 2048-group tile (35 tiles: 16, 16 and 3); G = 70 001
    gives each three passes, and their packers 69."""
    bits3.test_device_packer_equals_host_and_decides(ctx4, hq, 70_001)
    bits3.test_plane_device_packer_equals_host_and_decides(ctx4, hq, 70_001)


# ---- the synthetic generators against their CPU twins, 98 passes
@pytest.mark.parametrize("kw", [dict(n_max=5, parity_extras=True),
                                dict(n_max=8, mixed_n=True, parity_extras=True)])
def test_synth_generators_in_passes(ctx4, hq, kw):
    Gs = 100_003
    par.test_synth_commit_matches_cpu_generator(ctx4, hq, kw)            # G = 100 003 too
    par.test_synth_commit_lag_matches_host_packer(ctx4, hq, kw)          # G = 50 003
    host = qref.BitmapInputs(qref.spec(SEED + 3, Gs, **kw))
    arrs = [ctx4.empty(Gs, np.uint8) for _ in range(4)]
    ctx4.synth_bitmaps_dev(hq.synth_spec(SEED + 3, Gs, **kw), *arrs)
    ctx4.sync()
    for d, h in zip(arrs, (host.ack, host.granted, host.rejected, host.n_voting)):
        np.testing.assert_array_equal(ctx4.download(d), h)
        ctx4.free(d)
