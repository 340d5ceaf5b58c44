"""Hand-fed inputs of ocn_cn_colsum_exact (tests/test_colsum_host.py, tests/test_colsum_gpu.py), numpy only.

The entry reads nothing but arrays, so a case is put together directly: K designated columns are the nodes 0 .. K-1, batch row
e has its own source node K + e whose CSR row lists the designated columns it is a member of (ascending), ``off`` is the
cumulative sum of the row lengths, flags and walk counts are drawn per column, and ``hist`` is packed from the flags.  Which rows
a column is a member of — hence its entry count and where its flag positions lie — is chosen by the case.
"""
import functools
from collections import namedtuple

import numpy as np

from tests import colsum_mirror as M

Case = namedtuple("Case", "name variant N B K rowptr col src off flagsA flagsB wc hist")

VARIANTS = ("plain", "valued", "cn6")
# (a large value such as 2500 is of no use here: with nip = 7500 the S2 of almost every column is the same in any order —
# see LADDER_RESEED below — and the host condition cannot be met)
INNERPRODS = (0.37, -3.0, 7.3)

# Every case has the "anchor": a column of three cn1 entries, and no column with n1 = 2.  So min{n1 >= 2} = 3 and
# nip = 3 * innerprod in every case, whatever the other columns draw.
ANCHOR_STREAM = (5, 3, 0)

# A column's sum is the sum of three different values only (1 - t, -t, 1), so it is less order-sensitive than one would think: the
# rounding error of an add of -t depends on the binade of the running sum alone.  Whether a wrong order shows is therefore a
# property of the drawn flags — tests/test_colsum_host.py asserts it for every case column — and a column whose first draw does
# not discriminate takes a later one: {length: draw} (found by trying 0, 1, 2, ... against the mirror; nothing else depends on it).
LADDER_SEED = 5
LADDER_RESEED = {63: 113, 64: 124, 65: 677, 70: 329, 127: 1592, 128: 6636, 129: 737, 255: 421, 256: 5593, 257: 802, 511: 730,
                 512: 217, 513: 4047, 2047: 613, 2048: 73, 2049: 111, 4095: 10, 4096: 18, 4097: 286, 5000: 170}
MANY_SEED, MANY_IP, MANY_STREAMS = 13, 0.37, {False: 16, True: 4}      # streams per length: 65 .. 70, 513 .. 600
MANY_RESEED = {65: (14, 8, 3, 3, 7, 2, 3, 18, 7, 24, 5, 15, 44, 3, 4, 21), 66: (3, 6, 5, 3, 19, 14, 1, 3, 1, 9, 25, 5, 0, 8, 33,
               3), 67: (4, 4, 29, 21, 18, 4, 10, 5, 16, 4, 4, 8, 4, 5, 17, 6), 68: (0, 11, 1, 7, 5, 4, 8, 13, 6, 0, 6, 5, 7, 0,
               3, 7), 69: (0, 19, 1, 6, 3, 25, 5, 21, 36, 5, 7, 8, 14, 17, 15, 2), 70: (0, 4, 4, 26, 15, 14, 6, 0, 6, 10, 12, 0,
               5, 10, 11, 21), 513: (3, 0, 7, 1), 514: (7, 5, 36, 4), 515: (2, 4, 10, 18), 516: (0, 3, 3, 3), 517: (12, 8, 0,
               1), 518: (6, 8, 3, 5), 519: (1, 8, 0, 8), 520: (0, 2, 0, 5), 521: (6, 6, 3, 3), 522: (1, 17, 0, 13), 523: (1, 0,
               3, 0), 524: (4, 8, 3, 1), 525: (10, 14, 8, 1), 526: (6, 9, 5, 8), 527: (12, 0, 2, 2), 528: (7, 4, 26, 21), 529:
               (0, 9, 0, 12), 530: (5, 2, 1, 1), 531: (3, 0, 0, 1), 532: (1, 5, 1, 6), 533: (8, 5, 4, 3), 534: (11, 5, 1, 7),
               535: (2, 0, 14, 1), 536: (18, 9, 28, 5), 537: (4, 5, 7, 1), 538: (1, 7, 9, 1), 539: (16, 2, 3, 4), 540: (24, 1,
               3, 7), 541: (0, 5, 1, 1), 542: (4, 1, 10, 1), 543: (6, 2, 4, 5), 544: (6, 0, 11, 4), 545: (5, 2, 10, 1), 546:
               (17, 2, 4, 4), 547: (15, 9, 1, 17), 548: (0, 16, 1, 2), 549: (8, 3, 2, 12), 550: (0, 2, 16, 0), 551: (9, 2, 0,
               4), 552: (0, 0, 6, 0), 553: (6, 8, 2, 0), 554: (6, 19, 3, 3), 555: (5, 0, 3, 0), 556: (1, 9, 4, 7), 557: (10, 4,
               1, 22), 558: (3, 3, 13, 2), 559: (6, 0, 11, 14), 560: (1, 12, 2, 5), 561: (5, 1, 20, 9), 562: (1, 0, 8, 1), 563:
               (0, 6, 5, 9), 564: (0, 2, 2, 12), 565: (1, 0, 6, 5), 566: (7, 0, 0, 12), 567: (13, 16, 13, 6), 568: (5, 9, 1,
               22), 569: (6, 0, 13, 10), 570: (0, 5, 7, 3), 571: (15, 1, 0, 7), 572: (4, 3, 0, 1), 573: (1, 11, 18, 2), 574:
               (20, 6, 4, 0), 575: (0, 0, 12, 0), 576: (5, 9, 9, 11), 577: (6, 0, 1, 4), 578: (3, 6, 4, 5), 579: (1, 1, 8, 0),
               580: (8, 7, 19, 9), 581: (6, 9, 7, 13), 582: (11, 4, 5, 0), 583: (1, 10, 9, 6), 584: (5, 5, 14, 1), 585: (0, 0,
               1, 1), 586: (2, 2, 0, 17), 587: (8, 0, 0, 1), 588: (0, 12, 0, 4), 589: (3, 1, 0, 2), 590: (6, 6, 0, 6), 591: (3,
               13, 7, 0), 592: (4, 1, 6, 14), 593: (0, 1, 6, 1), 594: (1, 1, 9, 0), 595: (4, 16, 8, 0), 596: (10, 14, 3, 2),
               597: (5, 0, 0, 0), 598: (0, 7, 0, 1), 599: (17, 1, 1, 2), 600: (6, 1, 0, 10)}

# every path's first and last length: one wave (<= 64), 2 / 4 / 8 key registers (<= 128 / 256 / 512), LDS sort (<= 4096) with one
# or two staging rounds (<= 2048 / beyond), the in-memory sort
LADDER = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 5000)
LADDER_B = 5000
LDS_SORTED = tuple(L for L in LADDER if M.CS_MED_MAX < L <= M.CS_LDS)
FULL_BINS = (513, 2047, 2048, 2049, 4096)       # 10 753 consecutive positions: fit CS_BINS bins of CS_BIN_MAX
SHARD_CUTS = ((0, 2000, LADDER_B), (0, 1700, 3400, LADDER_B))
EARLY_ROWS = 1250                               # the "early" column's members all lie below every first cut


def build(name, variant, members, kinds, B, seed, cap=None, fix=None, streams=None):
    """``members[c]``: the batch rows (distinct) of designated column c.  ``kinds[c]``: how its flagsA bytes are drawn —
    "mixed" uniformly from {1, 2, 3}; "cn2" all 2 (n1 = 0: the closed form in cn5); "cn1" from {1, 3} (n1 = its length);
    "b" all 0 (a cn3-only column: entries for cn6 alone).  cn6 additionally clears a quarter of the flagsA bytes of the
    "mixed" / "cn2" columns and sets flagsB there, so that the wider union has entries outside the stage-1 union.
    Every column draws from its own stream (``streams[c]``, by default (seed, c)), so a column's values in position order do
    not depend on the other columns of the case, nor on which rows it is a member of."""
    assert variant in VARIANTS
    K, N = len(members), len(members) + B
    rows = np.concatenate([np.asarray(m, np.int64).reshape(-1) for m in members])
    cols = np.concatenate([np.full(len(m), c, np.int64) for c, m in enumerate(members)])
    assert rows.size == 0 or (0 <= rows.min() and rows.max() < B)
    o = np.lexsort((cols, rows))
    rows, cols = rows[o], cols[o]
    assert np.unique(rows * K + cols).size == rows.size
    T = rows.size
    deg = np.bincount(rows, minlength=B).astype(np.int64)
    off = np.zeros(B + 1, np.int64)
    np.cumsum(deg, out=off[1:])
    rowptr = np.zeros(N + 1, np.int64)
    rowptr[K + 1:] = off[1:]
    cap = T if cap is None else int(cap)
    assert cap >= T
    fa, fb, wc = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8), np.zeros(cap, np.int32)
    for c in range(K):
        q = np.flatnonzero(cols == c)
        rng = np.random.default_rng([seed, c] if streams is None else list(streams[c]))
        f = rng.integers(1, 4, q.size).astype(np.uint8)
        if kinds[c] == "cn2":
            f[:] = M.F_CN2
        elif kinds[c] == "cn1":
            f |= M.F_CN1
        elif kinds[c] == "b":
            f[:] = 0
        b = rng.integers(0, 2, q.size).astype(np.uint8)
        if variant == "cn6":
            drop = (rng.random(q.size) < 0.25) & (kinds[c] in ("mixed", "cn2"))
            f[drop] = 0
            b[f == 0] = 1
        fa[q], fb[q], wc[q] = f, b, rng.integers(1, 6, q.size)
    if fix is not None:
        fix(cols, fa, fb, wc)
    flagsB = fb if variant == "cn6" else None
    walks = wc if variant == "valued" else None
    hist = M.hist_of_flags(cols, fa, walks, N)
    return Case(name, variant, N, B, K, rowptr, cols.astype(np.int32), K + np.arange(B, dtype=np.int64), off, fa, flagsB, walks,
                hist)


def args(case, rows=None):
    """The mirror's (and ops.cn_colsum_exact's) leading arguments; ``rows`` = (first, last + 1): that edge shard's slices."""
    s, e = (0, case.B) if rows is None else rows
    return case.rowptr, case.col, case.src[s:e], case.off[s:e + 1], case.flagsA, case.flagsB, case.wc, case.hist


def spaced(L, B, shift):
    """L members evenly spaced over B rows."""
    return np.sort((np.arange(L, dtype=np.int64) * B // L + shift) % B)


def ladder_stream(L):
    return ANCHOR_STREAM if L == 3 else (LADDER_SEED, L, LADDER_RESEED.get(L, 0))


@functools.lru_cache(maxsize=None)
def ladder(variant, layout="even"):
    """One column per length of LADDER in one batch (the length-3 column is the anchor), and: "closed" (n1 = 0: the closed
    form in cn5), "early" (all members in the first rows: an edge shard's later ranks pass its sum through), "b_only" (cn3
    entries alone: untouched in cn5), and an untouched column.
    Layouts: "even" — the LDS-sorted columns' members evenly spaced, flag capacity == total; "tail" — the same with a flag
    buffer 64 times longer (zero tail), so that every position falls into the first bins."""
    rng = np.random.default_rng(2024)
    members, kinds = [], []
    for i, L in enumerate(LADDER):
        members.append(spaced(L, LADDER_B, 37 * i) if L in LDS_SORTED else np.sort(rng.choice(LADDER_B, L, replace=False)))
        kinds.append({2: "cn2", 3: "cn1"}.get(L, "mixed"))
    members += [np.sort(rng.choice(LADDER_B, 40, replace=False)), np.sort(rng.choice(EARLY_ROWS, 70, replace=False)),
                np.sort(rng.choice(LADDER_B, 30, replace=False)), np.zeros(0, np.int64)]
    kinds += ["cn2", "mixed", "b", "mixed"]
    total = sum(len(m) for m in members)
    return build("ladder/" + layout, variant, members, kinds, LADDER_B, seed=LADDER_SEED,
                 cap={"even": total, "tail": 64 * total}[layout], streams=[ladder_stream(len(m)) for m in members])


LADDER_EXTRA = {"closed": len(LADDER), "early": len(LADDER) + 1, "b_only": len(LADDER) + 2, "untouched": len(LADDER) + 3}


@functools.lru_cache(maxsize=None)
def consecutive(variant, layout):
    """Columns whose members are consecutive rows, one entry per row: a column's positions are one dense run (the anchor
    follows in three rows of its own).  "rows": the six LDS-sorted lengths, capacity == total (58 positions per bin);
    "full" / "over": five of them in a flag buffer of CS_BINS * CS_BIN_MAX (the bucket path with full bins) /
    CS_BINS * (CS_BIN_MAX + 1) positions.  The columns draw from the ladder's streams: the same values in position order."""
    lengths = (LDS_SORTED if layout == "rows" else FULL_BINS) + (3,)
    start = np.cumsum((0,) + lengths)
    members = [np.arange(start[i], start[i + 1], dtype=np.int64) for i in range(len(lengths))]
    cap = {"rows": int(start[-1]), "full": M.CS_BINS * M.CS_BIN_MAX, "over": M.CS_BINS * (M.CS_BIN_MAX + 1)}[layout]
    return build("consecutive/" + layout, variant, members, ["mixed"] * (len(lengths) - 1) + ["cn1"], int(start[-1]),
                 seed=LADDER_SEED, cap=cap, streams=[ladder_stream(L) for L in lengths])


def layout_case(variant, layout):
    return ladder(variant, layout) if layout in ("even", "tail") else consecutive(variant, layout)


LAYOUTS = ("even", "tail", "rows", "full", "over")


def lds_sorted_columns(case, res):
    return np.flatnonzero(res.ordered & (res.length > M.CS_MED_MAX) & (res.length <= M.CS_LDS))


def bin_occupancy(case, c):
    """The fullest bin of column c under the test's own rule: bin = position * CS_BINS // capacity."""
    k, pos = M.union_entries(*args(case)[:6])
    return int(np.bincount(pos[k == c] * M.CS_BINS // case.flagsA.size, minlength=M.CS_BINS).max())


def many_stream(L, c):
    j = c % MANY_STREAMS[L > 70]
    return (MANY_SEED, L, j, MANY_RESEED.get(L, (0,) * 16)[j])


@functools.lru_cache(maxsize=None)
def many(variant):
    """More columns than workgroups: 1000 columns of 513 .. 600 entries (the long kernel's grid is 768: some workgroup draws
    a second ticket) and 5000 of 65 .. 70 (the medium kernel's 1024 workgroups take four per round); the anchor is last.
    Columns of one length share 16 streams (the long ones 4): the same values in position order, at other positions."""
    B = 4096
    rng = np.random.default_rng(77)
    lengths = np.concatenate([rng.integers(513, 601, 1000), rng.integers(65, 71, 5000)])
    members = [np.sort(rng.permutation(B)[:L]) for L in lengths] + [np.arange(3)]
    streams = [many_stream(int(L), c) for c, L in enumerate(lengths)] + [ANCHOR_STREAM]
    return build("many", variant, members, ["mixed"] * lengths.size + ["cn1"], B, seed=MANY_SEED, streams=streams)


TWO21 = 1 << 21


@functools.lru_cache(maxsize=None)
def two24():
    """Valued, no column with n1 >= 2 (t = 0 everywhere).  Column 0: walks = 2^24 - 1, the closed form.  Column 1: twenty
    entries of 2^21 or 2^21 + 1, walks > 2^24: ordered by the integer rule, and the +1s survive or not by their place."""
    members = [np.arange(0, 8), np.arange(4, 24)]

    def fix(cols, fa, fb, wc):
        for c in (0, 1):
            q = np.flatnonzero(cols == c)
            fa[q] = M.F_CN2
            fa[q[2]] |= M.F_CN1                                        # n1 = 1: still t = 0
        q = np.flatnonzero(cols == 0)
        wc[q] = TWO21
        wc[q[-1]] -= 1
        q = np.flatnonzero(cols == 1)
        wc[q] = TWO21 + np.random.default_rng(7).integers(0, 2, q.size)    # (a draw for which the order matters: test_two24_case)
    return build("two24", "valued", members, ["cn2", "cn2"], 24, seed=1, fix=fix)


@functools.lru_cache(maxsize=None)
def singletons(variant):
    """No column with n1 >= 2 (each has one cn1 entry at most): nip = innerprod, t = 0, every touched column is unordered."""
    B = 700
    rng = np.random.default_rng(31)
    lengths = (1, 2, 5, 64, 65, 100, 513, 600)
    members = [np.sort(rng.choice(B, L, replace=False)) for L in lengths]

    def fix(cols, fa, fb, wc):
        for c in range(0, len(lengths), 2):
            fa[np.flatnonzero(cols == c)[0]] |= M.F_CN1
    return build("singletons", variant, members, ["cn2"] * len(lengths), B, seed=2, fix=fix)


# the orders a wrong rank would produce: a descending sort, the halves of a merge swapped, a wave's 64 values reversed
def descending(L):
    return np.arange(L)[::-1]


def halves_swapped(L):
    return np.concatenate([np.arange(L // 2, L), np.arange(L // 2)])


def runs_of_64_reversed(L):
    p = np.arange(L)
    for r0 in range(0, L, 64):
        p[r0:r0 + 64] = p[r0:r0 + 64][::-1].copy()
    return p


WRONG_ORDERS = (descending, halves_swapped, runs_of_64_reversed)
