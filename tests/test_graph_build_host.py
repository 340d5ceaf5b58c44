"""CPU suite of the graph build: the mirror (tests/graph_build_mirror.py) against brute force on inputs small enough to
enumerate, the premises of the constructed cases (tests/graph_build_cases.py) that tests/test_graph_build_gpu.py runs — each
really reaches the edge it is there for — and the argument checks of the C entries, which return before any HIP call."""
import ctypes
import itertools
import os
import re

import pytest
import torch

from tests import graph_build_cases as C
from tests import graph_build_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pairs(rowptr, col):
    return [(r, c) for r, cols in enumerate(M.rows_of(rowptr, col)) for c in cols]


def _random_csr(g, n_rows, n_cols, nnz):
    r = torch.randint(0, n_rows, (nnz,), generator=g)
    c = torch.randint(0, n_cols, (nnz,), generator=g)
    return M.csr_of_coo(r, c, n_rows, n_cols, False, True)


# ---------------------------------------------------------------------------------------------
# the mirror against brute force
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetrize,dedupe", list(itertools.product((False, True), repeat=2)))
def test_csr_of_coo_is_the_sorted_pair_list(symmetrize, dedupe):
    g = torch.Generator().manual_seed(1)
    n = 9
    row, col = torch.randint(0, n, (60,), generator=g), torch.randint(0, n, (60,), generator=g)
    pairs = list(zip(row.tolist(), col.tolist()))
    if symmetrize:
        pairs += [(c, r) for r, c in pairs]
    want = sorted(set(pairs)) if dedupe else sorted(pairs)
    assert len(set(pairs)) < len(pairs)                                  # there are duplicates to drop
    rowptr, out = M.csr_of_coo(row, col, n, n, symmetrize, dedupe)
    assert out.dtype == torch.int32 and rowptr.dtype == torch.int64
    assert _pairs(rowptr, out) == want and rowptr[-1] == len(want)
    rowptr, out = M.csr_of_coo(torch.tensor([1, 1, 0]), torch.tensor([C.BIG - 1, 0, C.BIG - 1]), 3, C.BIG, False, False)
    assert rowptr.tolist() == [0, 1, 3, 3] and out.tolist() == [C.BIG - 1, 0, C.BIG - 1]


def test_pattern_of_product_is_the_dense_matmul():
    g = torch.Generator().manual_seed(2)
    rpA, cA = _random_csr(g, 7, 5, 12)
    rpB, cB = _random_csr(g, 5, 40, 30)
    rpC, cC = M.pattern_of_product(rpA, cA, rpB, cB, 40)
    dense = M.dense_of_csr(rpA, cA, 7, 5) @ M.dense_of_csr(rpB, cB, 5, 40)
    assert (dense > 1).any()                                             # a column reached twice is listed once
    want = [(r, c) for r in range(7) for c in range(40) if dense[r, c] > 0]
    assert _pairs(rpC, cC) == want
    assert [torch.equal(a, b) for a, b in zip(M.csr_of_dense(dense), (rpC, cC))] == [True, True]


@pytest.mark.parametrize("n_cols,stride", [(1, 1), (32, 1), (33, 2), (70, 3), (70, 5)])
def test_bit_rows_bit_by_bit(n_cols, stride):
    g = torch.Generator().manual_seed(3)
    rp, c = _random_csr(g, 6, n_cols, 3 * n_cols)
    rows = M.rows_of(rp, c)
    rows[0], rows[1] = [], list(range(n_cols))
    rp, c = M.csr_of_rows(rows)
    bits = M.bit_rows(rp, c, n_cols, stride)
    assert bits.dtype == torch.int32 and tuple(bits.shape) == (6, stride)
    for r in range(6):
        for w in range(stride):
            word = sum(1 << (k - 32 * w) for k in rows[r] if k >> 5 == w)
            assert int(bits[r, w]) & 0xFFFFFFFF == word                  # nothing at or beyond n_cols, nothing in the padding
    if n_cols >= 32:
        assert int(bits[1, 0]) == -1                                     # bit 31 is the sign of the int32 word
    rp2, c2 = M.cols_of_bit_rows(bits, n_cols)
    assert torch.equal(rp2, rp) and torch.equal(c2, c)
    bits[2, stride - 1] = C.SENTINEL                                     # padding is not looked at; a bit beyond n_cols is refused
    if stride * 32 - n_cols >= 32:
        assert torch.equal(M.cols_of_bit_rows(bits, n_cols)[1], c)
    elif n_cols % 32:
        bits[2, stride - 1] = -1
        with pytest.raises(AssertionError):
            M.cols_of_bit_rows(bits, n_cols)


def test_block_adj2_is_the_product_and_its_fold():
    g = torch.Generator().manual_seed(4)
    n = 11
    rp, c = _random_csr(g, n, n, 25)
    A = M.dense_of_csr(rp, c, n, n)
    full = {(i, j) for i in range(n) for j in range(n) if any(A[i, k] and A[k, j] for k in range(n))}
    assert 0 < len(full) < n * n
    for block in (1, 3, 4, 11, 16):
        got = M.block_adj2(rp, c, n, block, False)
        assert {(i, j) for i, j in torch.nonzero(got).tolist()} == full
        got = M.block_adj2(rp, c, n, block, True)
        assert {(i, j) for i, j in torch.nonzero(got).tolist()} == {(i % block, j % block) for i, j in full}


def test_block_adj2_knows_the_path_graph():
    """The hand-derived answers of test_parity_gpu.py::test_block_route_known_answers_on_a_path: A² of a path has (i, i) and
    (i, i +- 2); folded, every entry lands on (i % block, j % block)."""
    n, bs = 70, 32
    i = torch.arange(n - 1)
    rp, c = M.csr_of_coo(i, i + 1, n, n, True, True)
    full = {(i, i) for i in range(n)} | {(i, i + 2) for i in range(n - 2)} | {(i + 2, i) for i in range(n - 2)}
    fold = {(i % bs, j % bs) for i, j in full}
    for quirk, want in ((False, full), (True, fold)):
        got = M.block_adj2(rp, c, n, bs, quirk)
        assert {(i, j) for i, j in torch.nonzero(got).tolist()} == want and int(got.max()) == 1


# ---------------------------------------------------------------------------------------------
# the cases reach the edges they claim
# ---------------------------------------------------------------------------------------------
def _define(src, name):
    m = re.findall(r"#define\s+%s\s+\(?(\d+)" % name, src)
    assert len(m) == 1, name
    return int(m[0])


def test_case_constants_are_the_kernels():
    rowsort = open(os.path.join(ROOT, "ocn_amd", "csrc", "rowsort.h")).read()
    common = open(os.path.join(ROOT, "ocn_amd", "csrc", "common.h")).read()
    spgemm = open(os.path.join(ROOT, "ocn_amd", "csrc", "spgemm.hip")).read()
    assert _define(rowsort, "CC_WAVE_MAX") == C.CC_WAVE_MAX and _define(rowsort, "CC_LDS") == C.CC_LDS
    assert "n > CC_WAVE_MAX" in rowsort and "n <= CC_LDS" in rowsort
    assert _define(common, "OCN_BLOCK") == C.BLOCK and _define(common, "OCN_WAVE") == 64
    assert spgemm.count("(160 * 1024) / (lds + 256)") == 2 and spgemm.count("256 * (per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu))") == 2
    assert C.spgemm_grid(100, 10 ** 6) == 2048 and C.spgemm_grid(8193, 10 ** 6) == 2048 and C.spgemm_grid(8193, 600) == 600


def _staged(case, symmetrize):
    rowptr, _ = M.csr_of_coo(case.row, case.col, case.n_rows, case.n_cols, symmetrize, False)
    return (rowptr[1:] - rowptr[:-1]).tolist()


def _distinct(case, symmetrize):
    rowptr, _ = M.csr_of_coo(case.row, case.col, case.n_rows, case.n_cols, symmetrize, True)
    return (rowptr[1:] - rowptr[:-1]).tolist()


def test_coo_ladder_stands_on_every_switch():
    case = C.coo_case("ladder")
    staged, distinct = _staged(case, False), _distinct(case, False)
    assert case.n_rows != case.n_cols and abs(case.n_cols - 20000) < 100 and case.row.numel() < 200000
    assert [staged[r] for r in sorted(case.info["staged"])] == list(C.LADDER)
    assert staged[0::2] == [0] * (len(C.LADDER) + 1)                     # an empty row on either side of every row
    for w in (C.CC_WAVE_MAX, C.CC_LDS, 128, 4096, 16384):                # both sides of every switch; a power of two and one past it
        assert w in staged and w + 1 in staged
    assert all(d < s for s, d in zip(staged, distinct) if s >= case.info["duplicates_from"])
    assert not torch.equal(case.row, torch.sort(case.row).values)        # shuffled
    again = C.reshuffled(case)
    assert not torch.equal(again.row, case.row) and _staged(again, False) == staged


def test_coo_small_cases_hold_their_premises():
    for name in ("one_column", "run_across_rounds", "sixty_four_distinct"):
        case = C.coo_case(name)
        staged, distinct = _staged(case, False), _distinct(case, False)
        for r, want in case.info["staged"].items():
            assert staged[r] == want and distinct[r] == case.info["distinct"][r]
    case = C.coo_case("run_across_rounds")
    _, col = M.csr_of_coo(case.row, case.col, case.n_rows, case.n_cols, False, False)
    assert col.tolist() == case.info["sorted"][1] and col[63] == col[64] and col[62] != col[63] != col[65]
    assert not torch.equal(case.col, torch.sort(case.col).values)
    assert _distinct(C.coo_case("sixty_four_distinct"), False)[2] == C.CC_WAVE_MAX < _staged(C.coo_case("sixty_four_distinct"), False)[2]


def test_coo_big_columns_reach_the_last_int32():
    case = C.coo_case("big_columns")
    assert case.n_cols == 2 ** 31 - 1 and case.info["ends"] == [0, 1, 2 ** 31 - 3, 2 ** 31 - 2]
    staged = _staged(case, False)
    assert staged[0] == case.info["staged"][0] <= C.CC_WAVE_MAX < case.info["staged"][2] == staged[2]
    rows = M.rows_of(*M.csr_of_coo(case.row, case.col, case.n_rows, case.n_cols, False, True))
    for r in (0, 2):
        assert rows[r][:2] == [0, 1] and rows[r][-2:] == [2 ** 31 - 3, 2 ** 31 - 2]
    assert C.coo_modes(case) == [(False, False), (False, True)]


def test_coo_symmetric_reaches_its_lengths_only_with_the_transpose():
    case = C.coo_case("symmetric")
    assert case.n_rows == case.n_cols and len(C.coo_modes(case)) == 4
    plain, sym = _staged(case, False), _staged(case, True)
    assert {r: sym[r] for r in range(4)} == case.info["staged_sym"] == {0: 64, 1: 65, 2: 12288, 3: 12289}
    assert {r: plain[r] for r in range(4)} == case.info["staged_max_plain"]
    transposed = _staged(case._replace(row=case.col, col=case.row), False)
    assert all(max(plain[r], transposed[r]) < want for r, want in ((0, 64), (1, 64), (2, 12288), (3, 12288)))
    assert all(d < s for s, d in list(zip(sym, _distinct(case, True)))[:4])
    loops = set(case.row[case.row == case.col].tolist())
    assert loops == set(case.info["self_loops"])
    assert sum(sym) < 200000


def _lens(rowptr):
    return (rowptr[1:] - rowptr[:-1]).tolist()


def test_product_tall_loops_over_rows():
    p = C.product_case("tall")
    lenA, lenB = _lens(p.rowptrA), _lens(p.rowptrB)
    assert len(lenA) == 5000 and len(lenB) == 300 and p.n_cols_b == 100
    assert len(lenA) > C.spgemm_grid(p.n_cols_b, len(lenA)) == 2048      # every workgroup takes a second row
    assert lenA.count(0) > 100 and lenB.count(0) == 60 and lenA.count(1) > 100
    assert M.rows_of(p.rowptrA, p.colA)[p.info["full_row"]] == list(range(300))
    single = M.rows_of(p.rowptrA, p.colA)[p.info["single_to_empty"]]
    assert len(single) == 1 and lenB[single[0]] == 0
    lenC = _lens(C.product_pattern("tall")[0])
    assert lenC[p.info["single_to_empty"]] == 0 and lenA[p.info["single_to_empty"]] == 1
    assert max(lenC) == lenC[p.info["full_row"]] and any(a > 0 and c == 0 for a, c in zip(lenA, lenC))
    first_pass, second_pass = lenC[:2048], lenC[2048:4096]
    assert any(a > 0 and b == 0 for a, b in zip(first_pass, second_pass))   # a stale bitmap would show in an empty later row


def test_product_words_cases_stand_on_the_word_per_thread_switch():
    for n_cols_b, words in ((8192, 256), (8193, 257)):
        p = C.product_case(f"words_{n_cols_b}")
        assert (p.n_cols_b + 31) // 32 == words and 500 < len(_lens(p.rowptrA)) < 700
        wpt = -(-words // C.BLOCK)
        assert wpt == (1 if words == 256 else 2)
        if words == 257:                                                  # thread 128 holds word 256 alone, 129 .. 255 nothing
            assert 128 * wpt == 256 and 129 * wpt > words
        cols = set(C.product_pattern(p.name)[1].tolist())
        assert p.info["marks"] == [c for c in (0, 31, 32, 8191, 8192) if c < n_cols_b] and set(p.info["marks"]) <= cols
        assert max(cols) == n_cols_b - 1


def test_product_max_cols_fills_the_lds(hiplib):
    mx = hiplib.ocn_spgemm_max_cols()
    p = C.product_case("max_cols", mx)
    assert p.n_cols_b == mx and (mx + 31) // 32 * 4 == 158 * 1024 > 64 * 1024
    lenC = _lens(C.product_pattern("max_cols", mx)[0])
    assert len(lenC) == 8 and all(12 <= k <= 80 for k in lenC)
    cols = C.product_pattern("max_cols", mx)[1]
    assert int(cols.min()) == 0 and int(cols.max()) == mx - 1


def test_product_square_and_its_cube():
    p = C.product_case("square")
    n = p.n_cols_b
    assert 2900 < n < 3100 and p.rowptrA is p.rowptrB
    A = M.rows_of(p.rowptrA, p.colA)
    assert all(r in A[c] for r in range(n) for c in A[r])                # symmetric
    assert len(A[p.info["hub"]]) >= 300 and sum(1 for a in A if not a) >= 5
    rp2, c2 = C.product_pattern("square")
    cube = C.product_case("cube")
    assert cube.rowptrA is rp2 and cube.colA is c2 and cube.colB is p.colA
    rp3, _ = C.product_pattern("cube")
    assert p.rowptrA[-1] < rp2[-1] < rp3[-1] < n * n // 4                 # sparse at every power


def test_demand_case_holds_its_premises():
    d = C.demand_case()
    n = C.N_SQUARE
    rows = d.rows.tolist()
    assert len(rows) > C.spgemm_grid(n, len(rows)) == 2048               # a workgroup takes a second request
    assert -1 in rows and n in rows and len(set(rows)) < len(rows)
    in_range = {r for r in rows if 0 <= r < n}
    assert len(in_range) == 1500 and sum(rows.count(r) > 1 for r in list(in_range)[:50]) > 0
    done = d.done.bool()
    assert int((done & d.wanted).sum()) == 0 and int(done.sum()) == 300
    assert sum(bool(done[r]) for r in in_range) == 200                   # requested rows that are done already
    assert {r for r in in_range if not done[r]} == set(torch.nonzero(d.wanted).flatten().tolist())
    assert d.stride == (n + 31) // 32 + 2
    untouched = ~d.wanted & ~done
    assert int(untouched.sum()) > 1000                                   # rows nobody asks for


@pytest.mark.parametrize("n", C.BLOCK_NS)
def test_block_graphs_are_sparse_in_every_block(n):
    gph = C.block_graph(n)
    deg = _lens(gph.rowptr)
    assert 2.5 < sum(deg) / n < 3.5
    assert [v for v in range(n) if deg[v] == 0] == [gph.isolated]
    rows = M.rows_of(gph.rowptr, gph.col)
    assert set(rows[gph.hub]) == set(range(1, n)) - set(gph.removed) and gph.isolated in gph.removed
    assert abs(len(gph.removed) - n / 3) <= 1.5 and n - 1 not in gph.removed
    for block in C.BLOCK_SIZES:
        d = C.block_adj2(n, block, False)
        assert 2 * int(d.sum()) < n * n                                  # fewer than half of the bits: a spurious one shows
        assert not d[gph.isolated].any() and not d[:, gph.isolated].any()
        for r0 in range(0, n, block):
            for c0 in range(0, n, block):
                assert d[r0:r0 + block, c0:c0 + block].any(), (block, r0, c0)
        folded = C.block_adj2(n, block, True)
        assert torch.equal(folded, d) == (block >= n)                    # a single block folds onto itself
    assert any(b > n for b in C.BLOCK_SIZES) and set(C.BLOCK_NS) == {33, 64, 65, 127, 128, 129, 191, 257}
    assert all(b % 32 == 0 for b in C.BLOCK_SIZES)


def test_off_grid_block_is_off_the_tile_grid():
    o = C.OFF_GRID
    assert (o["r0"], o["r1"], o["c0"], o["c1"]) == (32, 70, 64, 200) and o["n"] == 257
    assert o["r0"] % 32 == 0 and o["c0"] % 32 == 0 and (o["r1"] - o["r0"]) % 32 and (o["c1"] - o["c0"]) % 128
    full = C.block_adj2(257, 288, False)
    d = full[o["r0"]:o["r1"], o["c0"]:o["c1"]]
    assert 0 < int(d.sum()) < d.numel() // 2
    # the operand rows beyond the block are clamped to its last row and column: both are dense in the block, so a lost clamp
    # of the write mask would repeat them over the sparse bits the test pre-sets outside
    last_row, last_col = full[o["r1"] - 1, o["c0"]:o["c1"]], full[o["r0"]:o["r1"], o["c1"] - 1]
    assert 2 * int(last_row.sum()) > last_row.numel() and 2 * int(last_col.sum()) > last_col.numel()


@pytest.mark.parametrize("n_cols", C.BITROW_COLS)
def test_bitrow_cases_have_every_kind_of_row(n_cols):
    rowptr, col, kinds = C.bitrow_case(n_cols)
    rows = dict(zip(kinds[:7], M.rows_of(rowptr, col)[:7]))
    words = (n_cols + 31) // 32
    assert rows["empty"] == [] and rows["full"] == list(range(n_cols)) and rows["first"] == [0] and rows["last"] == [n_cols - 1]
    assert rows["31_and_32"] == [c for c in (31, 32) if c < n_cols]
    per_word = [c >> 5 for c in rows["one_per_word"]]
    assert per_word == list(range(words)) or (per_word == list(range(words - 1)) and n_cols % 32)
    assert len(kinds) == len(_lens(rowptr)) and kinds.count("random") == 3
    assert {(c + 31) // 32 for c in C.BITROW_COLS} == {1, 2, 63, 64, 65, 129}


# ---------------------------------------------------------------------------------------------
# the C entries refuse bad arguments before any HIP call
# ---------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_before_any_launch(hiplib):
    E, NULL = -1, None
    one = ctypes.c_int64(0)
    p = ctypes.cast(ctypes.pointer(one), ctypes.c_void_p)               # a non-NULL host pointer: never dereferenced on these paths
    l = hiplib
    # ocn_coo_to_csr(row, col, nnz, n_rows, n_cols, symmetrize, dedupe, rowptr, col_out, workspace, result, stream)
    assert l.ocn_coo_to_csr(p, p, 4, 5, 6, 1, 1, p, p, p, p, NULL) == E                     # symmetrize a rectangular matrix
    assert l.ocn_coo_to_csr(p, p, 2 ** 30, 5, 5, 1, 0, p, p, p, p, NULL) == E               # 2 nnz staged entries > 2^31 - 1
    assert l.ocn_coo_to_csr(p, p, 2 ** 31, 5, 5, 0, 0, p, p, p, p, NULL) == E
    assert l.ocn_coo_to_csr(p, p, 4, 5, 2 ** 31, 0, 1, p, p, p, p, NULL) == E               # a column id past int32
    assert l.ocn_coo_to_csr(p, p, 4, 5, 5, 0, 1, NULL, p, p, p, NULL) == E                  # no rowptr
    assert l.ocn_coo_to_csr(p, p, 4, 5, 5, 0, 1, p, NULL, p, p, NULL) == E                  # no column output
    assert l.ocn_coo_to_csr(p, p, 4, 5, 5, 0, 1, p, p, p, NULL, NULL) == E                  # no result words
    assert l.ocn_coo_to_csr(p, p, -1, 5, 5, 0, 1, p, p, p, p, NULL) == E
    mx = l.ocn_spgemm_max_cols()
    # ocn_spgemm_pattern_count(rowptrA, colA, n_rows, rowptrB, colB, n_cols_b, row_count, bitmap, stride, stream)
    for bad in (0, -3, mx + 1):
        assert l.ocn_spgemm_pattern_count(p, p, 4, p, p, bad, p, NULL, 0, NULL) == E
        assert l.ocn_spgemm_pattern_fill(p, p, 4, p, p, bad, p, p, NULL) == E
        assert l.ocn_spgemm_bit_rows(p, p, 4, p, p, bad, p, 2, p, p, 1 << 20, NULL) == E
    assert l.ocn_spgemm_pattern_count(p, p, 4, p, p, 65, p, p, 2, NULL) == E                # 65 columns are three words
    assert l.ocn_spgemm_pattern_count(p, p, 4, p, p, 64, NULL, NULL, 0, NULL) == E          # no counts
    assert l.ocn_spgemm_pattern_fill(p, p, 4, p, p, 64, NULL, p, NULL) == E
    assert l.ocn_spgemm_pattern_fill(p, p, 4, p, p, 64, p, NULL, NULL) == E
    # ocn_spgemm_bit_rows(rowptrA, colA, n_rows, rowptrB, colB, n_cols_b, rows, n_req, done, bitmap, stride, stream)
    assert l.ocn_spgemm_bit_rows(p, p, 4, p, p, 65, p, 2, p, p, 2, NULL) == E
    assert l.ocn_spgemm_bit_rows(p, p, 4, p, p, 64, p, 2, NULL, p, 2, NULL) == E            # no done marks
    assert l.ocn_spgemm_bit_rows(p, p, 4, p, p, 64, p, -1, p, p, 2, NULL) == E
    # ocn_bitrows_fill(bits, stride, n_rows, n_cols, rowptr, col, stream)
    assert l.ocn_bitrows_fill(p, 2, 4, 65, p, p, NULL) == E                                  # stride shorter than the columns
    assert l.ocn_bitrows_count(p, 2, 4, 65, p, NULL) == E


def test_zero_size_calls_return_at_once(hiplib):
    """No rows, or no requests: 0, with nothing launched (there is no device here) and no pointer looked at."""
    l, NULL = hiplib, None
    assert l.ocn_spgemm_pattern_count(NULL, NULL, 0, NULL, NULL, 64, NULL, NULL, 0, NULL) == 0
    assert l.ocn_spgemm_pattern_fill(NULL, NULL, 0, NULL, NULL, 64, NULL, NULL, NULL) == 0
    assert l.ocn_spgemm_bit_rows(NULL, NULL, 0, NULL, NULL, 64, NULL, 5, NULL, NULL, 0, NULL) == 0
    assert l.ocn_spgemm_bit_rows(NULL, NULL, 7, NULL, NULL, 64, NULL, 0, NULL, NULL, 0, NULL) == 0
    assert l.ocn_bitrows_from_csr(NULL, NULL, 0, NULL, 0, NULL) == 0
    assert l.ocn_bitrows_count(NULL, 2, 0, 64, NULL, NULL) == 0
    assert l.ocn_bitrows_fill(NULL, 2, 0, 64, NULL, NULL, NULL) == 0
    assert l.ocn_dense_from_csr(NULL, NULL, 0, 64, NULL, NULL, NULL) == 0
    one = ctypes.c_int64(0)
    p = ctypes.cast(ctypes.pointer(one), ctypes.c_void_p)
    assert l.ocn_dense_block_mm_bits(p, p, 64, 64, 32, 32, 0, 64, 0, p, 2, NULL) == 0       # an empty row range
