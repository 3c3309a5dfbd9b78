"""Multi-ctx ReadIndex on adversarial batches (ri_multi_cases.adversarial).

CPU: the oracle's message replay equals the closed form on those batches, each of six defects
built into the closed form changes at least 2 % of their groups (and none of random_batch's for
five of them), and the batches meet the share floors that keep a parity test from passing
vacuously. GPU: every route into every kernel of hq_ri_multi.hip, bit-exact against the oracle,
with and without released_index, every output between poisoned 64-byte guards."""
import os

import numpy as np
import pytest

from oracle import qref
from ri_multi_cases import (DEFECTS, adversarial, assert_shares, changed_groups,
                            closed_form_defect, unpack_fallback)
from test_readindex_multi import (U64MAX, _check_outputs, closed_form, random_batch,
                                  tiles_reference)

POISON = 0x5A
FLAGS = [(False, False), (False, True), (True, False), (True, True)]
BIG = 4097          # from this G on a batch's shares are asserted


def make_case(seed, G, K_max, n_max, perk, pern, nu):
    """An adversarial batch with the oracle's outputs: (ord, idx, K, n, Kp, nv, nu, want), Kp /
    nv the per-group columns handed to the kernel (None when uniform). Batches of BIG groups and
    more must meet the share floors."""
    rng = np.random.default_rng(seed)
    nu = 0 if pern else nu
    ord_, idx, K, n = adversarial(rng, G, K_max, n_max, perk, pern, nu)
    Kp, nv = (K if perk else None), (n if pern else None)
    want = qref.readindex_multi_batch(ord_, idx, Kp, nv, nu, K_max, n_max)
    if G >= BIG:
        assert_shares(K, K_max, want, G)
    return ord_, idx, K, n, Kp, nv, nu, want


def uniform_ns(n_max):
    """n_uniform equal to n_max and, where there is room, below it."""
    return [n_max] if n_max == 1 else [n_max, max(1, n_max // 2)]


def seed_of(*v):
    s = 0
    for x in v:
        s = s * 1009 + int(x)
    return s


# ------------------------------------------------------------------------------ CPU ---------
@pytest.mark.parametrize("K_max,n_max", [(8, 8), (6, 7), (3, 5), (1, 1), (2, 3)])
def test_replay_equals_closed_form_on_adversarial_batches(K_max, n_max):
    G = 3000
    for perk, pern in FLAGS:
        for nu in ([0] if pern else uniform_ns(n_max)):
            rng = np.random.default_rng(seed_of(K_max, n_max, perk, pern, nu))
            ord_, idx, K, n = adversarial(rng, G, K_max, n_max, perk, pern, nu)
            rel, cnt, fbw, bend = qref.readindex_multi_batch(
                ord_, idx, K if perk else None, n if pern else None, nu, K_max, n_max)
            fb = unpack_fallback(fbw, G)
            # flagged groups: nothing released; the closed form is not asked about them
            want_rel, want_cnt, want_bend = closed_form(ord_, idx, np.where(fb, 0, K), n, K_max,
                                                        n_max, G)
            np.testing.assert_array_equal(rel, want_rel)
            np.testing.assert_array_equal(cnt, want_cnt)
            np.testing.assert_array_equal(bend, want_bend)
            assert (rel.reshape(K_max, G)[:, fb] == U64MAX).all()
            assert not cnt[fb].any() and not bend[fb].any()
            # the flags are the contract breaks, and nothing else
            Ki, ni = K.astype(int), n.astype(int)
            x = idx.reshape(K_max, G)
            dec = np.zeros(G, bool)
            for k in range(1, K_max):
                dec |= (k < Ki) & (x[k] < x[k - 1])
            broken = (ni < 1) | (ni > n_max) | (Ki > K_max)
            np.testing.assert_array_equal(fb, broken | dec)
            assert_shares(K, K_max, (rel, cnt, fbw, bend), G)
            if perk and pern:       # every contract break is present
                assert (Ki == 0).any() and (Ki == K_max + 1).any() and (Ki == 255).any()
                assert (ni == 0).any() and (ni == n_max + 1).any() and (ni == 255).any()
                assert (dec & ~broken).any() or K_max < 2


def test_adversarial_batch_covers_its_edges():
    """What the generator promises, read back from a batch: the ordinal pools, distinct ordinals
    over all cells, live cells outside k < K and s < n, the index regions with rows crossing
    2^32 and 2^63, the ceiling of 2^64 - 2, and decreasing rows beyond K."""
    K_max = n_max = 8
    G = 2048
    ord_, idx, K, n = adversarial(np.random.default_rng(3), G, K_max, n_max, True, True, 0)
    o = ord_.reshape(K_max * n_max, G).astype(int)
    x = idx.reshape(K_max, G)
    for g in range(G):
        live = o[:, g][(o[:, g] != 0xFFFF) & (o[:, g] != 0)]
        assert len(set(live)) == len(live)
    assert 0.40 < (o == 0xFFFF).mean() < 0.50 and 0.06 < (o == 0).mean() < 0.10
    live = np.where((o == 0xFFFF) | (o == 0), -1, o)
    assert (live >= 0xFF00).any() and ((live > 0) & (live <= 64)).any()
    lo = np.where(live < 0, 1 << 20, live).min(axis=0)
    assert ((lo < 0x8000) & (live.max(axis=0) >= 0x8000) & (live.max(axis=0) - lo < 64)).any()
    Ki, ni = K.astype(int), n.astype(int)
    o3 = o.reshape(K_max, n_max, G)
    ok = (Ki <= K_max) & (ni >= 1) & (ni <= n_max)
    beyond_n = beyond_k = 0
    for g in np.flatnonzero(ok):
        beyond_n += (o3[:, ni[g]:, g] != 0xFFFF).any()
        beyond_k += (o3[Ki[g]:, :, g] != 0xFFFF).any()
    assert beyond_n > G // 4 and beyond_k > G // 4
    assert int(x.max()) <= 2**64 - 2 and int(x.max()) >= 2**64 - 40
    first = np.zeros(G, bool)
    cross32 = np.zeros(G, bool)
    cross63 = np.zeros(G, bool)
    runs = np.zeros(G, bool)
    junk = np.zeros(G, bool)
    last = x[np.where(ok & (Ki >= 1), Ki, 1) - 1, np.arange(G)]     # row K - 1
    for k in range(1, K_max):
        inside = ok & (k < Ki)
        cross32 |= inside & (x[k - 1] < 2**32) & (x[k] >= 2**32)
        cross63 |= inside & (x[k - 1] < 2**63) & (x[k] >= 2**63)
        runs |= inside & (x[k] == x[k - 1])
        junk |= ok & (k >= Ki) & (Ki >= 1) & (x[k] < last)
        first |= ok & (Ki == 0) & (x[k] < x[k - 1])
    assert cross32.mean() > 0.05 and cross63.mean() > 0.05 and runs.mean() > 0.3
    assert junk.mean() > 0.2 and first.any()
    assert (x.min(axis=0) < 64).any()


def test_mutants_are_caught_only_by_the_adversarial_batch():
    """Each defect in the closed form changes (count, fallback, released index) in at least 2 %
    of an adversarial batch's groups; random_batch sees none of the first five. The counts are
    recorded in ri_multi_cases' docstring."""
    K_max = n_max = 8
    G = 2048
    rng = np.random.default_rng(20)
    adv = adversarial(rng, G, K_max, n_max, True, True, 0)
    ben = random_batch(np.random.default_rng(20), G, K_max, n_max)
    for name, (ord_, idx, K, n) in (("adversarial", adv), ("random_batch", ben)):
        oracle = qref.readindex_multi_batch(ord_, idx, K, n, 0, K_max, n_max)
        assert changed_groups(closed_form_defect(ord_, idx, K, n, K_max, n_max, G), oracle,
                              K_max, G) == 0
        for d in DEFECTS:
            c = changed_groups(closed_form_defect(ord_, idx, K, n, K_max, n_max, G, d), oracle,
                               K_max, G)
            print(f"{name:12s} {d:10s} {c}")
            if name == "adversarial":
                assert c >= 0.02 * G, (d, c)
            elif d != "strict_tie":
                assert c == 0, (d, c)


def test_host_tile_packer_on_adversarial_batches(hq):
    for K_max, n_max, G, perk, pern in [(8, 8, 130, True, True), (3, 5, 258, False, True),
                                        (5, 7, 2, True, False), (4, 3, 129, False, False)]:
        rng = np.random.default_rng(seed_of(K_max, n_max, G))
        ord_, idx, K, n = adversarial(rng, G, K_max, n_max, perk, pern, 0 if pern else n_max)
        Kp, nv = (K if perk else None), (n if pern else None)
        tiles, flags = hq.tile_ri_multi_host(G, K_max, n_max, ord_, idx, Kp, nv)
        np.testing.assert_array_equal(tiles, tiles_reference(ord_, idx, Kp, nv, K_max, n_max, G))


# ------------------------------------------------------------------------------ GPU ---------
class Guarded:
    """A device array of `count` elements between two 64-byte guards, guards and body poisoned:
    the kernels' paired stores (u16 counts, 16-byte indexes) must stay inside the body."""

    def __init__(self, ctx, hq, count, dtype):
        dtype = np.dtype(dtype)
        self.ctx = ctx
        self.base = ctx.empty(count * dtype.itemsize + 128, np.uint8)
        ctx.memset(self.base, POISON)
        self.a = hq.DeviceArray(self.base.ptr + 64, count * dtype.itemsize, dtype, count)

    def untouched(self):
        return (self.ctx.download(self.a).view(np.uint8) == POISON).all()

    def release(self):
        raw = self.ctx.download(self.base)
        self.ctx.free(self.base)
        assert (raw[:64] == POISON).all() and (raw[-64:] == POISON).all()


class Outputs:
    def __init__(self, ctx, hq, G, K_max):
        self.rel = Guarded(ctx, hq, K_max * G, np.uint64)
        self.cnt = Guarded(ctx, hq, G, np.uint8)
        self.bend = Guarded(ctx, hq, G, np.uint8)
        self.fb = Guarded(ctx, hq, hq.words64(G), np.uint64)

    def args(self, compact, bend=True, fb=True):
        """(released_index, released_count, fallback, batch_end) as the launchers take them."""
        return (None if compact else self.rel.a, self.cnt.a, self.fb.a if fb else None,
                self.bend.a if bend else None)

    def check(self, ctx, hq, K_max, idx, compact, want, bend=True, fb=True):
        try:
            if bend and fb:
                _check_outputs(ctx, hq, K_max, idx, self.rel.a, self.cnt.a, self.fb.a,
                               self.bend.a, compact, want)
                return
            want_rel, want_cnt, want_fb, want_bend = want
            np.testing.assert_array_equal(ctx.download(self.cnt.a), want_cnt)
            if fb:
                np.testing.assert_array_equal(ctx.download(self.fb.a), want_fb)
            else:
                assert self.fb.untouched()
            if bend:
                np.testing.assert_array_equal(ctx.download(self.bend.a), want_bend)
            else:
                assert self.bend.untouched()
            if compact:
                assert self.rel.untouched()
            else:
                np.testing.assert_array_equal(ctx.download(self.rel.a), want_rel)
        finally:
            for g in (self.rel, self.cnt, self.bend, self.fb):
                g.release()


def run_columns(ctx, hq, case, G, K_max, n_max, compact, ord_shift=0, idx_shift=0, bend=True,
                fb=True):
    """hq_readindex_multi_dev on the case's columns against its oracle outputs. ord_shift /
    idx_shift: the column starts that many elements into its allocation (misaligned for the
    pair kernel's 4-byte and 16-byte loads)."""
    ord_, idx, _, _, Kp, nv, nu, want = case
    pad = lambda a, s: np.concatenate([np.zeros(s, a.dtype), a]) if s else a  # noqa: E731
    d = [ctx.upload(x) if x is not None else None
         for x in (pad(ord_, ord_shift), pad(idx, idx_shift), Kp, nv)]
    out = Outputs(ctx, hq, G, K_max)
    try:
        rel, cnt, fbp, bendp = out.args(compact, bend, fb)
        ctx.readindex_multi_dev(G, K_max, n_max, d[0].at(ord_shift), d[1].at(idx_shift), d[2],
                                d[3], nu, rel, cnt, fbp, bendp)
        out.check(ctx, hq, K_max, idx, compact, want, bend, fb)
    finally:
        for x in d:
            ctx.free(x)


def run_tiles(ctx, hq, case, G, K_max, n_max, compact, bend=True, fb=True):
    """The device packer equals the host packer on the case's columns; hq_readindex_multi_tiles_dev
    over those tiles against the oracle outputs."""
    ord_, idx, _, _, Kp, nv, nu, want = case
    tiles_h, flags = hq.tile_ri_multi_host(G, K_max, n_max, ord_, idx, Kp, nv)
    d = [ctx.upload(x) if x is not None else None for x in (ord_, idx, Kp, nv)]
    dt = Guarded(ctx, hq, len(tiles_h), np.uint8)
    out = Outputs(ctx, hq, G, K_max)
    try:
        ctx.tile_ri_multi_dev(G, K_max, n_max, d[0], d[1], d[2], d[3], dt.a)
        np.testing.assert_array_equal(ctx.download(dt.a), tiles_h)
        rel, cnt, fbp, bendp = out.args(compact, bend, fb)
        ctx.readindex_multi_tiles_dev(G, K_max, n_max, dt.a, flags, nu, rel, cnt, fbp, bendp)
        out.check(ctx, hq, K_max, idx, compact, want, bend, fb)
    finally:
        for x in d:
            ctx.free(x)
        dt.release()


def column_cases(G, K_max, n_max, tag):
    """Every (perk, pern) combination, the uniform voter count both equal to n_max and below."""
    for perk, pern in FLAGS:
        for nu in ([0] if pern else uniform_ns(n_max)):
            yield make_case(seed_of(tag, G, K_max, n_max, perk, pern, nu), G, K_max, n_max, perk,
                            pern, nu)


@pytest.mark.gpu
@pytest.mark.parametrize("K_max", [1, 2, 3, 4, 5, 8])
def test_pair_kernel_on_adversarial_columns(gpu_ctx, hq, K_max):
    """k_ri_multi2<PERK, PERN, KM> on columns: KM = 2, 4, 8, each with K_max == KM and below;
    one lane, a partial wave and several blocks; n_uniform < n_max on the uniform instances."""
    for G in (2, 130, 4098):
        for n_max in (1, 3, 5, 8):
            for case in column_cases(G, K_max, n_max, 1):
                for compact in (False, True):
                    run_columns(gpu_ctx, hq, case, G, K_max, n_max, compact)


ONE_GROUP_SHAPES = [(1, 1), (3, 5), (5, 7), (8, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("G,ord_shift,idx_shift", [(65, 0, 0), (4097, 0, 0), (4098, 1, 0),
                                                   (4098, 0, 1), (130, 1, 1)])
def test_one_group_kernel_on_adversarial_columns(gpu_ctx, hq, G, ord_shift, idx_shift):
    """k_ri_multi<PERK, PERN>: odd G, and even G whose ack_ordinal (one u16 in) or ctx_index
    (one u64 in) misses the pair kernel's alignment."""
    for K_max, n_max in ONE_GROUP_SHAPES:
        for case in column_cases(G, K_max, n_max, 2):
            for compact in (False, True):
                run_columns(gpu_ctx, hq, case, G, K_max, n_max, compact, ord_shift, idx_shift)


def open_context(hq, **env):
    """A context opened under open-time switches (read at hq_open only)."""
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        return hq.Context(0)
    finally:
        for k in env:
            del os.environ[k]


@pytest.mark.gpu
def test_one_group_kernel_with_pairs_off(hq):
    """HQ_RI_PAIRS=0 (read at hq_open) keeps an even, aligned batch on k_ri_multi."""
    ctx = open_context(hq, HQ_RI_PAIRS=0)
    try:
        for K_max, n_max in ONE_GROUP_SHAPES:
            for case in column_cases(4098, K_max, n_max, 3):
                for compact in (False, True):
                    run_columns(ctx, hq, case, 4098, K_max, n_max, compact)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K_max", [1, 2, 3, 4, 5, 6, 7, 8])
def test_tile_kernels_on_adversarial_tiles(gpu_ctx, hq, K_max):
    """Tiles: the device packer equals the host packer; uniform tiles with K_max in {2, 4, 8} and
    n_uniform == n_max run on k_ri_tiles_u<KM, N> (every N), the same tiles with n_uniform < n_max
    on k_ri_multi2<tiles, EXACT>, the other K_max on the dword-load instances; every flag
    combination, and G = 2, 130, 4098 leave a padded tile tail."""
    for G in (2, 130, 4098):
        for n_max in ((1, 3, 5, 8) if G != 4098 else range(1, 9)):
            for case in column_cases(G, K_max, n_max, 4):
                if n_max in (2, 4, 6, 7) and (case[4] is not None or case[5] is not None):
                    continue        # per-group columns: covered at the other n_max
                for compact in (False, True):
                    run_tiles(gpu_ctx, hq, case, G, K_max, n_max, compact)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["pairs", "one_group", "tiles_uniform", "tiles_general"])
def test_null_optional_outputs(gpu_ctx, hq, route):
    """batch_end = NULL with released_index given, and fallback = NULL: the other outputs are
    what they are with every output given, the buffer not passed stays untouched."""
    G = 4097 if route == "one_group" else 4098
    K_max, n_max, perk, pern = (4, 5, False, False) if route == "tiles_uniform" else \
                               (3, 5, True, True)
    case = make_case(seed_of(5, G, K_max), G, K_max, n_max, perk, pern, n_max)
    run = run_tiles if route.startswith("tiles") else run_columns
    run(gpu_ctx, hq, case, G, K_max, n_max, False, bend=False)
    run(gpu_ctx, hq, case, G, K_max, n_max, False, fb=False)
    run(gpu_ctx, hq, case, G, K_max, n_max, True, fb=False)
    run(gpu_ctx, hq, case, G, K_max, n_max, False, bend=False, fb=False)
