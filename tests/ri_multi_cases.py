"""Adversarial multi-ctx ReadIndex batches, and what proves them discriminating on the CPU.

`random_batch` (test_readindex_multi.py) draws ordinals 1..64 in the cells k < K, s < n only, ctx
indexes below 128 that never decrease in any row, K in 1..K_max and n in 1..n_max: a kernel that
dropped its voter padding, compared ordinals or indexes signed or truncated, or checked the index
order past K would still pass on it. `adversarial` draws what those defects need to show:

- ordinals distinct and non-zero over ALL K_max * n_max cells of a group (cells with k >= K or
  s >= n included: the decision must ignore them), from one of four pools per group (low 1..cells,
  top 0xFFFE downward, a run across 0x8000, uniform over 1..0xFFFE); then ~45 % of the cells are
  set to 0xFFFF (never acked; 15, 45 or 75 % per ctx row, so that unreached ctxs follow released
  ones) and ~8 % to 0 (carried). Distinct per group except 0: the contract.
- ctx indexes non-decreasing over the first K rows with runs of equal values, from bases near 0,
  just below 2^32, just below 2^63, around 2^64 - 40 (maximum <= 2^64 - 2: ~0 is "not released")
  and mid-range; in about half of the groups with K < K_max the rows k >= K hold values below row
  K - 1 (decreasing among themselves for K = 0), which is no fallback.
- perk: K in 0..K_max (the larger of two draws), ~3 % of the groups K_max + 1 or 255; pern: n in
  1..n_max, ~5 % of the groups 0, n_max + 1 or 255; ~3 % of the groups with K >= 2 take one
  decreasing step inside their first K rows. All of these are fallback.

`closed_form_defect` restates the kernels' closed form (reach time = max(q - 1, 1)-th smallest
first-ack ordinal of the first n voters, suffix-min release with ties to the earlier ctx) with one
of six defects switched on; `changed_groups` counts the groups whose (count, fallback, released
index) then differ from the oracle's message replay. Groups changed out of 2048 at K_max = n_max =
8, per-group K and n, seed 20 (test_mutants_are_caught_only_by_the_adversarial_batch asserts the
floor of 2 % = 41 on the right column and exactly 0 on the first five of the left):

    defect        random_batch   adversarial
    no_padding               0           939      voters s >= n not padded with 0xFFFF
    signed_ord               0           731      live ordinals compared as int16
    idx_past_K               0           759      index order checked over all K_max rows
    idx_low32                0           350      index order checked on the low 32 bits
    idx_signed               0           172      index order checked as int64
    strict_tie              41           136    equal reach times go to the later ctx
"""
import numpy as np

NONE = 0xFFFF
U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
DEFECTS = ("no_padding", "signed_ord", "idx_past_K", "idx_low32", "idx_signed", "strict_tie")

# the floors on the oracle's outputs that keep a parity test from passing vacuously
MAX_FALLBACK, MIN_RELEASING, MIN_PARTIAL, MIN_MULTI_BATCH = 0.15, 0.2, 0.05, 0.1


def adversarial(rng, G, K_max, n_max, perk, pern, n_uniform):
    """(ord [K_max * n_max * G] u16, idx [K_max * G] u64, K [G] u8, n [G] u8) as random_batch
    returns them. Without perk K is K_max everywhere, without pern n is n_uniform everywhere (the
    caller passes None for that column)."""
    cells = K_max * n_max
    # ---- counts
    if perk:
        # 0..K_max, leaning long: queues of two and more are where partial releases and
        # several release batches happen
        K = np.maximum(rng.integers(0, K_max + 1, G), rng.integers(0, K_max + 1, G))
        bad = rng.random(G) < 0.03
        K[bad] = np.where(rng.random(bad.sum()) < 0.5, K_max + 1, 255)
    else:
        K = np.full(G, K_max)
    if pern:
        n = rng.integers(1, n_max + 1, G)
        bad = rng.random(G) < 0.05
        n[bad] = rng.choice([0, n_max + 1, 255], bad.sum())
    else:
        n = np.full(G, n_uniform)
    Kin = np.where(K <= K_max, K, 0)                  # rows the decision may look at

    # ---- ordinals: `cells` distinct non-zero values per group, shuffled over the cells
    ar = np.arange(cells)
    pool = rng.integers(0, 4, G)
    low = np.broadcast_to(1 + ar, (G, cells))
    top = np.broadcast_to(0xFFFE - ar, (G, cells))
    if cells >= 2:
        start = 0x8000 - rng.integers(1, cells, G)    # start < 0x8000 <= start + cells - 1
    else:
        start = 0x7FFF + rng.integers(0, 2, G)
    run = start[:, None] + ar
    uni = np.sort(rng.integers(1, 0xFFFE - cells + 2, (G, cells)), axis=1) + ar
    vals = np.choose(pool[:, None], [low, top, run, uni])
    vals = np.take_along_axis(vals, np.argsort(rng.random((G, cells)), axis=1), axis=1)
    # ~45 % never acked over the batch, a ctx row's own rate 15, 45 or 75 % (a sparse row after
    # a dense one is a ctx left unreached behind a released one: partial releases); ~8 % carried
    none = np.repeat(rng.choice([0.15, 0.45, 0.75], (G, K_max)), n_max, axis=1)
    r = rng.random((G, cells))
    vals = np.where(r < none, NONE, np.where(r < none + 0.08, 0, vals))
    ord_ = np.ascontiguousarray(vals.T).astype(np.uint16)          # [k * n_max + s][g]

    # ---- ctx indexes: base + running sum of steps with runs of equal values
    region = rng.choice(5, G, p=[0.15, 0.25, 0.25, 0.15, 0.2])
    d = rng.integers(1, 2 * K_max + 3, G).astype(np.uint64)
    base = np.choose(region, [
        rng.integers(8, 50, G).astype(np.uint64),
        np.uint64(1 << 32) - d,
        np.uint64(1 << 63) - d,
        np.uint64((1 << 64) - 40) - rng.integers(0, 21, G).astype(np.uint64),
        rng.integers(1 << 40, 1 << 62, G).astype(np.uint64)])
    steps = rng.choice(np.array([0, 0, 0, 1, 1, 2, 3, 5], np.uint64), (K_max, G))
    steps[0] = 0
    idx = base[None, :] + np.cumsum(steps, axis=0, dtype=np.uint64)   # max add 35: <= 2^64 - 5
    rows = np.arange(K_max)[:, None]
    # rows k >= K below row K - 1 and decreasing: never looked at, so no fallback
    junk = (rng.random(G) < 0.5) & (Kin < K_max)
    last = np.where(Kin > 0, idx[np.maximum(Kin, 1) - 1, np.arange(G)], base)
    below = last[None, :] - np.uint64(1) - (rows - Kin[None, :]).clip(0).astype(np.uint64)
    idx = np.where(junk[None, :] & (rows >= Kin[None, :]), below, idx)
    # one decreasing step inside the first K rows: fallback
    dec = (rng.random(G) < 0.03) & (Kin >= 2)
    j = 1 + (rng.random(G) * (np.maximum(Kin, 2) - 1)).astype(np.int64)   # 1..K-1
    prev = idx[j - 1, np.arange(G)]
    idx = np.where(dec[None, :] & (rows == j[None, :]), prev[None, :] - np.uint64(1), idx)
    return (ord_.reshape(-1), np.ascontiguousarray(idx, np.uint64).reshape(-1),
            K.astype(np.uint8), n.astype(np.uint8))


def closed_form_defect(ord_, idx, K, n, K_max, n_max, G, defect=None):
    """(released index, count, fallback [G] bool, batch ends) by the kernels' closed form, with
    one of DEFECTS built in (None: the correct form)."""
    assert defect is None or defect in DEFECTS
    ord_ = ord_.reshape(K_max, n_max, G).astype(np.int64)
    idx = idx.reshape(K_max, G)
    rel = np.full((K_max, G), U64MAX)
    cnt = np.zeros(G, np.uint8)
    bend = np.zeros(G, np.uint8)
    fb = np.zeros(G, bool)

    def okey(x):        # how two ordinals compare (0xFFFF, never acked, stays last)
        return x - 0x10000 if defect == "signed_ord" and 0x8000 <= x < NONE else x

    def ikey(x):        # how two ctx indexes compare
        x = int(x)
        if defect == "idx_low32":
            return x & 0xFFFFFFFF
        if defect == "idx_signed":
            return x - (1 << 64) if x >= (1 << 63) else x
        return x

    for g in range(G):
        Kg, ng = int(K[g]), int(n[g])
        if ng < 1 or ng > n_max or Kg > K_max:
            fb[g] = True
            continue
        rows = K_max if defect == "idx_past_K" else Kg
        if any(ikey(idx[k, g]) < ikey(idx[k - 1, g]) for k in range(1, rows)):
            fb[g] = True
            continue
        r = max(ng // 2, 1)
        seen = n_max if defect == "no_padding" else ng
        t = []
        for k in range(Kg):
            v = [int(x) for x in ord_[k, :seen, g]]
            v += [NONE] * (8 - len(v))
            v.sort(key=okey)
            t.append(v[r - 1])
        best = None
        for k in reversed(range(Kg)):
            if t[k] != NONE and (best is None or
                                 (okey(t[k]) < okey(best[0]) if defect == "strict_tie"
                                  else okey(t[k]) <= okey(best[0]))):
                best = (t[k], k)
            if best is not None:
                rel[k, g] = idx[best[1], g]
                cnt[g] += 1
                if best[1] == k:
                    bend[g] |= 1 << k
    return rel.reshape(-1), cnt, fb, bend


def unpack_fallback(fb_words, G):
    return np.unpackbits(fb_words.view(np.uint8), bitorder="little")[:G].astype(bool)


def changed_groups(got, oracle, K_max, G):
    """Groups whose (count, fallback, released index) differ. got: closed_form_defect's outputs;
    oracle: qref.readindex_multi_batch's."""
    rel, cnt, fb, _ = got
    orel, ocnt, ofb, _ = oracle
    diff = (cnt != ocnt) | (fb != unpack_fallback(ofb, G))
    diff |= (rel.reshape(K_max, G) != orel.reshape(K_max, G)).any(axis=0)
    return int(diff.sum())


def shares(K, K_max, oracle, G):
    """(fallback, releasing, partial, multi-batch) shares of the G groups, from the oracle's
    outputs: flagged; releasing >= 1 entry; releasing a proper non-empty prefix of their K
    pending entries; closing two or more release batches."""
    _, cnt, fbw, bend = oracle
    fb = unpack_fallback(fbw, G)
    cnt = cnt.astype(int)
    nb = np.unpackbits(bend[:, None], axis=1).sum(axis=1)
    Kin = np.where(K.astype(int) <= K_max, K.astype(int), 0)
    return (fb.mean(), (cnt > 0).mean(), ((cnt > 0) & (cnt < Kin)).mean(), (nb >= 2).mean())


def assert_shares(K, K_max, oracle, G):
    """The floors that keep a parity test on this batch from passing vacuously."""
    f, r, p, m = shares(K, K_max, oracle, G)
    assert f <= MAX_FALLBACK and r >= MIN_RELEASING, (f, r)
    if K_max >= 3:
        assert p >= MIN_PARTIAL and m >= MIN_MULTI_BATCH, (p, m)
    return f, r, p, m
