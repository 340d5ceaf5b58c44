"""GPU suite of the graph build: the COO -> CSR build and its per-row sorts (coo_csr.hip, rowsort.h), the pattern of A·B with
its dense bit rows and the rows built on demand (spgemm.hip), the block route on the int8 matrix cores and the bit-row <-> CSR
conversions (dense_adj2.hip), each against the CPU mirror (tests/graph_build_mirror.py) on the constructed cases of
tests/graph_build_cases.py, whose premises tests/test_graph_build_host.py asserts.  Everything is integer and order-canonical:
every comparison is exact equality."""
import pytest
import torch

from ocn_amd import _lib, ops
from tests import graph_build_cases as C
from tests import graph_build_mirror as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENT = torch.tensor(C.SENTINEL, dtype=torch.int32).item()


def _dev(*ts):
    return [t.to(DEV) for t in ts]


def _same(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got.cpu(), want), what


# ---------------------------------------------------------------------------------------------
# ops.coo_to_csr
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.COO_CASES))
def test_coo_to_csr_equals_the_mirror_in_any_entry_order(hiplib, name):
    case = C.coo_case(name)
    again = C.reshuffled(case)
    for symmetrize, dedupe in C.coo_modes(case):
        rp, col = M.csr_of_coo(case.row, case.col, case.n_rows, case.n_cols, symmetrize, dedupe)
        for c in (case, again):                       # the fill order is atomic: the sort must canonicalise any of them
            rowptr, out = ops.coo_to_csr(c.row.to(DEV), c.col.to(DEV), c.n_rows, c.n_cols, symmetrize=symmetrize, dedupe=dedupe)
            assert out.dtype == torch.int32 and rowptr.dtype == torch.int64
            _same(rowptr, rp, (symmetrize, dedupe))
            _same(out, col, (symmetrize, dedupe))


# ---------------------------------------------------------------------------------------------
# ops.spgemm_pattern
# ---------------------------------------------------------------------------------------------
def _poison(*shapes):
    """Fill and free tensors of these shapes: the allocator hands the same blocks to the next torch.empty of their sizes, so
    a word the kernels leave unwritten reads as the sentinel."""
    ts = [torch.full(s, SENT, dtype=torch.int32, device=DEV) for s in shapes]
    torch.cuda.synchronize()
    del ts


@pytest.mark.parametrize("name", C.PRODUCT_NAMES)
def test_spgemm_pattern_equals_the_mirror(hiplib, name):
    mx = ops.spgemm_max_cols() if name == "max_cols" else None
    p = C.product_case(name, mx)
    rpC, colC = C.product_pattern(name, mx)
    n, words = rpC.numel() - 1, (p.n_cols_b + 31) // 32
    want_bits = M.bit_rows(rpC, colC, p.n_cols_b, words)
    args = _dev(p.rowptrA, p.colA, p.rowptrB, p.colB)
    _poison((n,), (n, words))
    rowptr, col, bitmap = ops.spgemm_pattern(*args, p.n_cols_b)
    _same(rowptr, rpC)
    _same(col, colC)
    _same(bitmap, want_bits)                          # with the zero bits past n_cols_b in the last word
    _poison((n,))
    rowptr, col, bitmap = ops.spgemm_pattern(*args, p.n_cols_b, want_bitmap=False)
    assert bitmap is None
    _same(rowptr, rpC)
    _same(col, colC)
    _poison((n,), (n, words))
    rowptr, fill, bitmap = ops.spgemm_pattern(*args, p.n_cols_b, defer_fill=True)
    assert callable(fill)
    _same(rowptr, rpC)
    _same(bitmap, want_bits)
    _poison((max(int(rpC[-1]), 1),))
    _same(fill(), colC)
    _same(bitmap, want_bits)                          # the fill pass leaves the bit rows alone


# ---------------------------------------------------------------------------------------------
# ops.spgemm_bit_rows
# ---------------------------------------------------------------------------------------------
def test_spgemm_bit_rows_writes_the_requested_rows_only(hiplib):
    p = C.product_case("square")
    d = C.demand_case()
    n, words = C.N_SQUARE, (C.N_SQUARE + 31) // 32
    want = M.bit_rows(*C.product_pattern("square"), p.n_cols_b, words)
    args = _dev(p.rowptrA, p.colA, p.rowptrB, p.colB)
    rows, done = d.rows.to(DEV), d.done.to(DEV)
    bitmap = torch.full((n, d.stride), SENT, dtype=torch.int32, device=DEV)
    ops.spgemm_bit_rows(*args, p.n_cols_b, rows, done, bitmap)
    for second in (False, True):
        got = bitmap.cpu()
        assert torch.equal(got[d.wanted, :words], want[d.wanted])
        assert (got[~d.wanted] == SENT).all()         # rows nobody asked for, rows marked done beforehand, ids out of range
        assert (got[:, words:] == SENT).all()         # the two padding words of every row
        assert torch.equal(done.cpu().bool(), d.done.bool() | d.wanted)
        assert int(done.max()) == 1
        if not second:
            ops.spgemm_bit_rows(*args, p.n_cols_b, rows, done, bitmap)    # everything is done: nothing changes


# ---------------------------------------------------------------------------------------------
# ops.dense_block_adj2
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.BLOCK_NS)
def test_dense_block_adj2_equals_the_mirror(hiplib, n):
    gph = C.block_graph(n)
    rowptr, col = _dev(gph.rowptr, gph.col)
    words = (n + 31) // 32
    for block in C.BLOCK_SIZES:
        for fold in (False, True):
            d = C.block_adj2(n, block, fold)
            rp, c = M.csr_of_dense(d)
            rowptrC, colC, bits = ops.dense_block_adj2(rowptr, col, n, block, fold=fold)
            _same(bits, M.bit_rows(rp, c, n, words), (block, fold))       # the bits at or beyond n in the last word are zero
            _same(rowptrC, rp, (block, fold))
            _same(colC, c, (block, fold))


def test_dense_block_mm_bits_ors_into_its_block_only(hiplib):
    """One direct call on a block that is not on the tile grid (rows 32 .. 69, columns 64 .. 199 of the 257-node graph), into
    bit rows that already hold bits inside and outside the block: inside old OR new, outside unchanged."""
    o = C.OFF_GRID
    n, r0, r1, c0, c1 = o["n"], o["r0"], o["r1"], o["c0"], o["c1"]
    gph = C.block_graph(n)
    rowptr, col = _dev(gph.rowptr, gph.col)
    ld, words = (n + 63) // 64 * 64, (n + 31) // 32
    dense = torch.zeros(ld, ld, dtype=torch.int8, device=DEV)
    denseT = torch.zeros(ld, ld, dtype=torch.int8, device=DEV)
    l, ptr, st = hiplib, _lib.ptr, _lib.stream_ptr
    _lib.check(l.ocn_dense_from_csr(ptr(rowptr), ptr(col), n, ld, ptr(dense), ptr(denseT), st()), "ocn_dense_from_csr")
    A = M.dense_of_csr(gph.rowptr, gph.col, n, n)
    assert torch.equal(dense[:n, :n].cpu().to(torch.int64), A) and torch.equal(denseT[:n, :n].cpu().to(torch.int64), A.t())
    assert int(dense.sum()) == int(A.sum()) == int(denseT.sum())          # nothing in the padding
    g = torch.Generator().manual_seed(11)
    old = (torch.rand(n, n, generator=g) < 0.1).to(torch.int64)
    want = old.clone()
    want[r0:r1, c0:c1] |= ((A[r0:r1] @ A[:, c0:c1]) > 0).to(torch.int64)
    assert 0 < int((want != old).sum()) and int(old[r0:r1, c0:c1].sum()) > 0
    bits = M.bit_rows(*M.csr_of_dense(old), n, words).to(DEV)
    _lib.check(l.ocn_dense_block_mm_bits(ptr(dense), ptr(denseT), ld, n, r0, r1, c0, c1, 0, ptr(bits), words, st()),
               "ocn_dense_block_mm_bits")
    _same(bits, M.bit_rows(*M.csr_of_dense(want), n, words))


# ---------------------------------------------------------------------------------------------
# ops.bitrows_from_csr -> ocn_bitrows_count -> ops.bitrows_to_cols
# ---------------------------------------------------------------------------------------------
def _count(l, bits, n_cols):
    cnt = torch.full((bits.shape[0],), SENT, dtype=torch.int32, device=DEV)
    _lib.check(l.ocn_bitrows_count(_lib.ptr(bits), bits.shape[1], bits.shape[0], n_cols, _lib.ptr(cnt), _lib.stream_ptr()),
               "ocn_bitrows_count")
    return cnt.cpu()


@pytest.mark.parametrize("n_cols", C.BITROW_COLS)
def test_bit_rows_round_trip(hiplib, n_cols):
    rp, c, _ = C.bitrow_case(n_cols)
    n, words = rp.numel() - 1, (n_cols + 31) // 32
    lens = (rp[1:] - rp[:-1]).to(torch.int32)
    rowptr, col = _dev(rp, c)
    # the stride of the words, through ops
    bits = ops.bitrows_from_csr(rowptr, col, n_cols)
    _same(bits, M.bit_rows(rp, c, n_cols, words))
    assert torch.equal(_count(hiplib, bits, n_cols), lens)
    _same(ops.bitrows_to_cols(bits, n_cols, rowptr), c)
    # a wider stride, through the raw entries: the padding words hold a sentinel that survives the build and that neither
    # the count nor the fill reads
    stride = words + C.BITROW_PAD
    wide = torch.full((n, stride), SENT, dtype=torch.int32, device=DEV)
    wide[:, :words] = 0
    l, ptr, st = hiplib, _lib.ptr, _lib.stream_ptr
    _lib.check(l.ocn_bitrows_from_csr(ptr(rowptr), ptr(col), n, ptr(wide), stride, st()), "ocn_bitrows_from_csr")
    want = M.bit_rows(rp, c, n_cols, stride)
    want[:, words:] = SENT
    _same(wide, want)
    assert torch.equal(_count(hiplib, wide, n_cols), lens)
    out = torch.full((max(c.numel(), 1),), -1, dtype=torch.int32, device=DEV)
    _lib.check(l.ocn_bitrows_fill(ptr(wide), stride, n, n_cols, ptr(rowptr), ptr(out), st()), "ocn_bitrows_fill")
    _same(out[:c.numel()], c)
    _same(wide, want)
