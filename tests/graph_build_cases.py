"""The constructed inputs of the graph-build tests (tests/test_graph_build_host.py asserts their premises,
tests/test_graph_build_gpu.py runs them): fixed seeds, no files.  Every builder records in ``info`` which edge of the kernels
the case is there for; the host test asserts that the edge is really reached."""
import functools
from collections import namedtuple

import torch

from tests import graph_build_mirror as M

# the regime switches of the per-row sorts (rowsort.h) and the launch shapes of spgemm.hip, restated: the host test holds
# them against the sources
CC_WAVE_MAX = 64                 # rows up to this many staged entries: one wave
CC_LDS = 12288                   # longer rows up to this many: the LDS network; beyond: in place in memory
BLOCK = 256                      # threads of a workgroup
LDS_BYTES = 160 * 1024


def spgemm_grid(n_cols_b, n_items):
    """Workgroups of the A·B launches (count, fill, rows on demand) at this width for ``n_items`` rows / requests."""
    lds = (n_cols_b + 31) // 32 * 4
    per_cu = LDS_BYTES // (lds + 256)
    return min(256 * max(1, min(8, per_cu)), n_items)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _shuffled(g, row, col):
    p = torch.randperm(len(row), generator=g)
    return torch.as_tensor(row, dtype=torch.int64)[p].contiguous(), torch.as_tensor(col, dtype=torch.int64)[p].contiguous()


def _distinct(g, n, lo, hi):
    """n distinct integers of [lo, hi), in random order."""
    assert n <= hi - lo
    return (torch.randperm(hi - lo, generator=g)[:n] + lo).tolist()


# ---------------------------------------------------------------------------------------------
# COO -> CSR
# ---------------------------------------------------------------------------------------------
Coo = namedtuple("Coo", "name row col n_rows n_cols info")

LADDER = (0, 1, 2, 63, 64, 65, 127, 128, 129, 4096, 4097, 12288, 12289, 16384, 16385)


def _with_duplicates(g, length, n_cols):
    """``length`` columns of which about a quarter repeat an earlier one (a row of two is one column twice)."""
    if length < 2:
        return _distinct(g, length, 0, n_cols)
    d = length - max(1, length // 4)
    cols = _distinct(g, d, 0, n_cols)
    return cols + [cols[i] for i in torch.randint(0, d, (length - d,), generator=g).tolist()]


def coo_ladder():
    """A row at both sides of every switch of the sort — one wave | one workgroup (64 | 65), LDS | in place (12 288 | 12 289),
    a power of two | one past it — rectangular, every row with duplicates, an empty row between any two, shuffled."""
    g = _gen(101)
    n_cols = 20011
    row, col = [], []
    for i, length in enumerate(LADDER):
        cols = _with_duplicates(g, length, n_cols)
        row += [2 * i + 1] * length
        col += cols
    row, col = _shuffled(g, row, col)
    return Coo("ladder", row, col, 2 * len(LADDER) + 1, n_cols,
               {"staged": {2 * i + 1: length for i, length in enumerate(LADDER)}, "duplicates_from": 2})


def coo_one_column():
    """5 000 copies of one column: the in-LDS network on all-equal keys, one distinct column left."""
    row = torch.full((5000,), 3, dtype=torch.int64)
    col = torch.full((5000,), 17, dtype=torch.int64)
    return Coo("one_column", row, col, 5, 100, {"staged": {3: 5000}, "distinct": {3: 1}})


def coo_run_across_rounds():
    """130 entries whose sorted order has the same column at places 63 and 64: the duplicate run crosses the compaction
    kernel's 64-lane rounds."""
    g = _gen(103)
    sorted_cols = list(range(63)) + [63, 63] + list(range(64, 129))
    row, col = _shuffled(g, [1] * len(sorted_cols), sorted_cols)
    return Coo("run_across_rounds", row, col, 3, 200, {"staged": {1: 130}, "distinct": {1: 129}, "sorted": {1: sorted_cols}})


def coo_sixty_four_distinct():
    """200 staged entries (a workgroup sorts the row) that leave exactly 64 distinct columns."""
    g = _gen(104)
    cols = _distinct(g, 64, 0, 900)
    cols = cols + [cols[i] for i in torch.randint(0, 64, (136,), generator=g).tolist()]
    row, col = _shuffled(g, [2] * 200, cols)
    return Coo("sixty_four_distinct", row, col, 4, 900, {"staged": {2: 200}, "distinct": {2: 64}})


BIG = 2 ** 31 - 1


def coo_big_columns():
    """n_cols = 2^31 - 1 with the columns 0, 1, 2^31 - 3, 2^31 - 2 in a short row and in a row longer than a wave."""
    g = _gen(105)
    ends = [0, 1, BIG - 2, BIG - 1]
    short = ends + [1, BIG - 1, 12345, BIG - 2]
    long_ = ends + torch.randint(0, BIG, (100,), generator=g).tolist()
    long_ = long_ + long_[:30]
    row, col = _shuffled(g, [0] * len(short) + [2] * len(long_), short + long_)
    return Coo("big_columns", row, col, 4, BIG, {"staged": {0: len(short), 2: len(long_)}, "ends": ends})


def coo_symmetric():
    """Square, with self loops: rows 0 .. 3 reach the staged lengths 64, 65, 12 288 and 12 289 only when the transposed
    entries join (a self loop is staged twice); out-lists and in-lists overlap, so the symmetrised rows have duplicates."""
    g = _gen(106)
    n = 7000
    row, col = [], []

    def node(v, n_out, n_in, loop):
        outs = _distinct(g, n_out, 10, n)
        ins = outs[:n_out // 3] + _distinct(g, n_in - n_out // 3, 10, n)      # (the second part may repeat the first: still staged)
        row.extend([v] * n_out + ins + ([v] if loop else []))
        col.extend(outs + [v] * n_in + ([v] if loop else []))
    node(0, 30, 34, False)
    node(1, 30, 33, True)
    node(2, 6000, 6288, False)
    node(3, 6000, 6287, True)
    for v in (10, 500, 6999):                                             # further self loops, on partner rows
        row.append(v)
        col.append(v)
    row, col = _shuffled(g, row, col)
    return Coo("symmetric", row, col, n, n,
               {"staged_sym": {0: 64, 1: 65, 2: 12288, 3: 12289}, "staged_max_plain": {0: 30, 1: 31, 2: 6000, 3: 6001},
                "self_loops": (1, 3, 10, 500, 6999)})


COO_CASES = {c.__name__[4:]: c for c in (coo_ladder, coo_one_column, coo_run_across_rounds, coo_sixty_four_distinct,
                                         coo_big_columns, coo_symmetric)}


@functools.lru_cache(maxsize=None)
def coo_case(name):
    return COO_CASES[name]()


def coo_modes(case):
    """The legal (symmetrize, dedupe) pairs: the transposed entries join square matrices only."""
    return [(s, d) for s in (False, True) for d in (False, True) if not s or case.n_rows == case.n_cols]


def reshuffled(case, seed=9):
    row, col = _shuffled(_gen(seed), case.row, case.col)
    return case._replace(row=row, col=col)


# ---------------------------------------------------------------------------------------------
# A·B
# ---------------------------------------------------------------------------------------------
Product = namedtuple("Product", "name rowptrA colA rowptrB colB n_cols_b info")


def _product(name, rowsA, rowsB, n_cols_b, **info):
    return Product(name, *M.csr_of_rows(rowsA), *M.csr_of_rows(rowsB), n_cols_b, info)


def _random_rows(g, n_rows, n_cols, max_len, empty_every=0):
    rows = []
    for r in range(n_rows):
        k = 0 if empty_every and r % empty_every == 0 else int(torch.randint(1, max_len + 1, (1,), generator=g))
        rows.append(set(_distinct(g, k, 0, n_cols)))
    return rows


def product_tall():
    """(a) A 5 000 x 300, B 300 x 100: more rows than the launch has workgroups, so every workgroup loops and its LDS bitmap
    must come back to zero between rows.  Empty rows of A and of B, rows of A with one entry (some of them naming an empty
    row of B), one row of A that lists every row of B."""
    g = _gen(201)
    rowsB = _random_rows(g, 300, 100, 10, empty_every=5)
    rowsA = _random_rows(g, 5000, 300, 6, empty_every=7)
    for r in range(1, 5000, 11):
        rowsA[r] = {int(torch.randint(0, 300, (1,), generator=g))}
    rowsA[2] = {5}                                                        # a single entry that names an empty row of B
    rowsA[4321] = set(range(300))
    return _product("tall", rowsA, rowsB, 100, full_row=4321, single_to_empty=2)


def product_words(n_cols_b):
    """(b) 8 192 columns are 256 bitmap words, one per thread; 8 193 are 257: two words per thread, thread 128 owns the last
    word alone and the threads behind it own nothing.  About 600 rows; the columns at the word and range borders are there."""
    g = _gen(202)
    marks = [c for c in (0, 31, 32, 8191, 8192) if c < n_cols_b]
    rowsB = _random_rows(g, 50, n_cols_b, 40)
    for i, c in enumerate(marks):
        rowsB[3 * i].add(c)
    rowsB[20] |= set(marks)
    rowsA = _random_rows(g, 600, 50, 4, empty_every=9)
    rowsA[1] = {20}
    return _product(f"words_{n_cols_b}", rowsA, rowsB, n_cols_b, marks=marks)


def product_max_cols(max_cols):
    """(c) the widest product the library forms: the bitmap of one row fills the LDS a workgroup can opt in to.  8 rows of a
    few dozen entries, column 0 and the last column among them."""
    g = _gen(203)
    rowsB = _random_rows(g, 20, max_cols, 12)
    rowsB[0].add(0)
    rowsB[1].add(max_cols - 1)
    rowsB[2] |= {0, 31, 32, max_cols - 33, max_cols - 32, max_cols - 1}
    rowsA = [set(_distinct(g, 5, 0, 20)) for _ in range(8)]
    rowsA[0] |= {0, 1}
    rowsA[7] = {2}
    return _product("max_cols", rowsA, rowsB, max_cols)


N_SQUARE = 3001


def product_square():
    """(d) a symmetric sparse graph of about 3 000 nodes (one node of degree 300, isolated nodes), as A·A."""
    g = _gen(204)
    n = N_SQUARE
    r = torch.randint(0, n - 5, (6000,), generator=g)                     # the last five nodes stay isolated
    c = torch.randint(0, n - 5, (6000,), generator=g)
    hub = torch.tensor(_distinct(g, 300, 0, n - 5))
    r, c = torch.cat([r, torch.full((300,), 77)]), torch.cat([c, hub])
    rowptr, col = M.csr_of_coo(r, c, n, n, True, True)
    return Product("square", rowptr, col, rowptr, col, n, {"hub": 77})


@functools.lru_cache(maxsize=None)
def product_case(name, max_cols=None):
    if name == "tall":
        return product_tall()
    if name in ("words_8192", "words_8193"):
        return product_words(int(name[6:]))
    if name == "max_cols":
        return product_max_cols(max_cols)
    if name == "square":
        return product_square()
    if name == "cube":                                                    # (A·A)·A: the product of (d) as the left operand
        sq = product_case("square")
        rowptr2, col2 = product_pattern("square")
        return Product("cube", rowptr2, col2, sq.rowptrA, sq.colA, sq.n_cols_b, {})
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def product_pattern(name, max_cols=None):
    """The mirror's (rowptrC, colC) of a case, computed once; callers must not write to it."""
    p = product_case(name, max_cols)
    return M.pattern_of_product(p.rowptrA, p.colA, p.rowptrB, p.colB, p.n_cols_b)


PRODUCT_NAMES = ("tall", "words_8192", "words_8193", "max_cols", "square", "cube")


# ---------------------------------------------------------------------------------------------
# rows of A·A on demand, on (d)
# ---------------------------------------------------------------------------------------------
Demand = namedtuple("Demand", "rows done stride wanted")

SENTINEL = 0x5A5A5A5A


@functools.lru_cache(maxsize=None)
def demand_case():
    """A request list longer than the launch's grid: 1 500 distinct rows of the 3 001, 900 of them a second time, the ids -1
    and n_rows; 200 requested and 100 other rows marked done beforehand; a stride two words wider than the bit row."""
    g = _gen(205)
    n = N_SQUARE
    p = torch.randperm(n, generator=g)
    req, other = p[:1500], p[1500:]
    rows = torch.cat([req, req[:900], torch.tensor([-1, n] * 8)])
    rows = rows[torch.randperm(rows.numel(), generator=g)].contiguous()
    done = torch.zeros(n, dtype=torch.int32)
    done[req[:200]] = 1
    done[other[:100]] = 1
    wanted = torch.zeros(n, dtype=torch.bool)
    wanted[req[200:]] = True                                              # requested, in range, not yet done
    return Demand(rows, done, (n + 31) // 32 + 2, wanted)


# ---------------------------------------------------------------------------------------------
# block route
# ---------------------------------------------------------------------------------------------
BLOCK_NS = (33, 64, 65, 127, 128, 129, 191, 257)
BLOCK_SIZES = (32, 64, 96, 128, 160, 288)
BLOCK_SEEDS = {33: 0, 64: 0, 65: 0, 127: 0, 128: 0, 129: 0, 191: 0, 257: 0}    # a graph that misses the host test's condition gets another

BlockGraph = namedtuple("BlockGraph", "n rowptr col hub isolated removed")


@functools.lru_cache(maxsize=None)
def block_graph(n, seed=None):
    """Average degree about 3 in all; node 0 adjacent to everybody, then without its edges to a fixed third of the nodes (every
    third node, the one before the last in the last one's place: a one-row last block must not be empty); one of that third
    isolated, every other one tied to its successor.  A² is then dense on the hub's neighbours x neighbours — four ninths of the matrix, spread over
    every block — and sparse elsewhere: a spurious bit has room to show, and no block of the tile loop is empty."""
    g = _gen(1000 * (BLOCK_SEEDS[n] if seed is None else seed) + n)
    removed = [v if v != n - 1 else n - 2 for v in range(1, n) if v % 3 == 2]
    isolated = removed[len(removed) // 2]
    m = n // 2                                                            # random edges; with the hub's 2n/3 and the chain's n/3: 3n/2
    r = torch.randint(1, n, (m,), generator=g)
    c = torch.randint(1, n, (m,), generator=g)
    keep = (r != c) & (r != isolated) & (c != isolated)
    r, c = r[keep], c[keep]
    nb = torch.tensor([v for v in range(1, n) if v not in removed])
    chain = torch.tensor([v for v in removed if v != isolated])           # nobody else is isolated: v - (v + 1)
    r, c = torch.cat([r, torch.zeros_like(nb), chain]), torch.cat([c, nb, chain + 1])
    rowptr, col = M.csr_of_coo(r, c, n, n, True, True)
    return BlockGraph(n, rowptr, col, 0, isolated, tuple(removed))


@functools.lru_cache(maxsize=None)
def block_adj2(n, block, fold):
    """The mirror's dense 0/1 answer, computed once; callers must not write to it."""
    gph = block_graph(n)
    return M.block_adj2(gph.rowptr, gph.col, n, block, fold)


# the one direct call on a block that is not on the tile grid (257 nodes)
OFF_GRID = {"n": 257, "r0": 32, "r1": 70, "c0": 64, "c1": 200}


# ---------------------------------------------------------------------------------------------
# bit rows <-> CSR
# ---------------------------------------------------------------------------------------------
BITROW_COLS = (1, 31, 32, 33, 2016, 2048, 2049, 4097)                     # 1, 1, 1, 2, 63, 64, 65, 129 words: around the 64-word rounds
BITROW_KINDS = ("empty", "full", "first", "last", "31_and_32", "one_per_word", "random", "random", "random", "empty", "full")
BITROW_PAD = 3                                                            # extra words of the wider stride


@functools.lru_cache(maxsize=None)
def bitrow_case(n_cols):
    """(rowptr, col, kinds): one row of every kind; a kind that needs a column the width does not have keeps those it has."""
    g = _gen(400 + n_cols)
    rows = []
    for kind in BITROW_KINDS:
        if kind == "empty":
            cols = []
        elif kind == "full":
            cols = range(n_cols)
        elif kind == "first":
            cols = [0]
        elif kind == "last":
            cols = [n_cols - 1]
        elif kind == "31_and_32":
            cols = [c for c in (31, 32) if c < n_cols]
        elif kind == "one_per_word":
            cols = [c for c in (32 * w + (7 * w + 5) % 32 for w in range((n_cols + 31) // 32)) if c < n_cols]
        else:
            cols = _distinct(g, int(torch.randint(0, n_cols + 1, (1,), generator=g)), 0, n_cols)
        rows.append(set(cols))
    return M.csr_of_rows(rows) + (BITROW_KINDS,)
