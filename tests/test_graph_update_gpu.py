"""Edge insertion on the device (ocn_amd/update.py; ``ocn_csr_union_*``, ``ocn_bitrows_insert``).  The oracle of every case is
the from-scratch route on the same device — ``from_edge_index(cat)`` + ``to_symmetric()`` / ``coalesce()``, then ``@`` — or a
closed form written out by hand.  Everything is bit-exact: no tolerance anywhere."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import csr_of_rows as _csr, edges_of as _edges_of, product_adj2 as _product, random_graph as _graph, \
    same_adj as _same_adj, same_product as _same_product, st as _st

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _scratch(adj, new, undirected=True):
    """The long way round: every entry sorted again, the whole product formed again."""
    n = adj.size(0)
    out = _st().from_edge_index(torch.cat([_edges_of(adj), new], dim=1), sparse_sizes=(n, n))
    out = out.to_symmetric() if undirected else out.coalesce()
    return out, _product(out)


def _check(adj, new, undirected=True, donate=False):
    from ocn_amd.update import insert_edges
    adj2 = _product(adj)
    want, want2 = _scratch(adj, new, undirected)
    got, got2 = insert_edges(adj, new, adj2, undirected=undirected, donate=donate)
    _same_adj(got, want)
    _same_product(got2, want2)
    only, none = insert_edges(adj, new, None, undirected=undirected)
    assert none is None
    _same_adj(only, want)
    return got, got2, want, want2


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65, 97])
def test_word_boundaries(hiplib, n):
    """Random symmetric graphs around the 32-bit word sizes, D of 1 .. 2N entries, always with entries into row and column
    N - 1: the tail word and the last row."""
    rng = np.random.default_rng(100 + n)
    adj = _graph(n, 0.08, n)
    before = (adj._rowptr.clone(), adj._col.clone())
    for e in sorted({1, max(1, n // 2), 2 * n}):
        new = rng.integers(0, n, size=(2, e))
        new[0, 0] = n - 1                                      # (N - 1, x) and, transposed, (x, N - 1)
        if e > 1:
            new[:, 1] = (0, n - 1)
        if e > 2:
            new[:, 2] = (n - 1, n - 1)
        _check(adj, torch.from_numpy(new.astype(np.int64)).to(DEV))
    _check(adj, torch.zeros(2, 0, dtype=torch.int64, device=DEV))      # E == 0: the result equals the input in content
    assert torch.equal(adj._rowptr, before[0]) and torch.equal(adj._col, before[1])          # adj itself is never modified


def _hub_graph():
    """N = 3000: node 0 is a hub with 2500 neighbours (longer than a wave round, than one 256-element chunk and than the 512
    columns a union row stages in LDS), node 2999 is isolated, the rest is sparse."""
    n = 3000
    rng = np.random.default_rng(7)
    hub = np.stack([np.zeros(2500, dtype=np.int64), np.arange(1, 2501)])
    rest = rng.integers(1, n - 1, size=(2, 6000))
    ei = torch.from_numpy(np.concatenate([hub, rest], axis=1)).to(DEV)
    adj = _st().from_edge_index(ei, sparse_sizes=(n, n)).to_symmetric()
    assert int(adj.storage.rowcount()[0]) >= 2500 and int(adj.storage.rowcount()[n - 1]) == 0
    return n, rng, adj


def test_hub_and_chunking(hiplib):
    """Both item kinds on a multi-chunk row, a row that grows from length 0, and a D row longer than a wave: the isolated node
    joins the hub, the hub a leaf, half of the hub's non-neighbours arrive at once, plus 200 random entries."""
    n, rng, adj = _hub_graph()
    far = np.arange(2501, n - 1)[::2]                           # 50 % of the hub's non-neighbours
    assert far.size > 64
    new = np.concatenate([np.array([[n - 1, 0], [0, 2700]]),    # isolated -> hub, hub -> a node it did not have
                          np.stack([np.zeros(far.size, dtype=np.int64), far]),
                          rng.integers(0, n, size=(2, 200))], axis=1)
    got, got2, want, want2 = _check(adj, torch.from_numpy(new.astype(np.int64)).to(DEV))
    assert int(got.storage.rowcount()[n - 1]) >= 1
    assert got.max_rowcount() == want.max_rowcount() >= 2500 + far.size


def test_idempotence_and_counting(hiplib):
    from ocn_amd import ops
    from ocn_amd.update import insert_edges
    adj = _graph(200, 0.03, 11)
    adj2 = _product(adj)
    ei = _edges_of(adj)
    # D a subset of A: nothing changes and no bit counts as new
    sub = ei[:, ::3].contiguous()
    got, got2 = insert_edges(adj, sub, adj2)
    _same_adj(got, adj)
    _same_product(got2, adj2)
    assert got2.nnz() == adj2.nnz()
    d = _st().from_edge_index(sub, sparse_sizes=(200, 200)).to_symmetric()
    bits = adj2.product_bit_rows().clone()
    added = ops.bitrows_insert(adj._rowptr, adj._col, adj._rowptr, adj._col, d._rowptr, d._col, bits)
    assert int(added.abs().sum()) == 0 and torch.equal(bits, adj2.product_bit_rows())
    # D with every entry four times = D once
    rng = np.random.default_rng(12)
    new = torch.from_numpy(rng.integers(0, 200, size=(2, 150)).astype(np.int64)).to(DEV)
    four = torch.cat([new, new, new, new], dim=1)[:, torch.randperm(600, generator=torch.Generator().manual_seed(1)).to(DEV)]
    once, once2 = insert_edges(adj, new, adj2)
    many, many2 = insert_edges(adj, four, adj2)
    _same_adj(many, once)
    _same_product(many2, once2)
    _check(adj, four)


def test_two_entries_creating_the_same_bit_count_it_once(hiplib):
    """The path a - b - c (a = 0, b = 1, c = 2) and an isolated d = 3: adding a - d and c - d makes (a, c) reachable through d
    too, which it already was through b; new are (d, d), (d, b) and (b, d) alone — each counted once, although (d, d) and (d, b)
    are both set by two items (through a and through c) and (b, d) from two entries."""
    from ocn_amd import ops
    ST = _st()
    adj = ST.from_edge_index(torch.tensor([[0, 1, 2, 1], [1, 0, 1, 2]], device=DEV), sparse_sizes=(4, 4))
    adj2 = _product(adj)
    new = torch.tensor([[0, 2], [3, 3]], device=DEV)
    got, got2, want, want2 = _check(adj, new)
    rows = [[0, 2], [1, 3], [0, 2], [1, 3]]                     # A' is the 4-cycle 0 - 1 - 2 - 3 - 0
    assert got2._rowptr.tolist() == [0, 2, 4, 6, 8] and got2._col.tolist() == sum(rows, [])
    d = ST.from_edge_index(new, sparse_sizes=(4, 4)).to_symmetric()
    bits = adj2.product_bit_rows().clone()
    added = ops.bitrows_insert(got._rowptr, got._col, got._rowptr, got._col, d._rowptr, d._col, bits)
    assert added.tolist() == [0, 1, 0, 2]                       # row 1 gains {3}, row 3 gains {1, 3}; rows 0 and 2 had {0, 2}
    assert bits.view(-1).tolist() == [0b0101, 0b1010, 0b0101, 0b1010]


def test_directed_insertion_reads_the_transpose(hiplib):
    rng = np.random.default_rng(21)
    adj = _graph(65, 0.06, 20, symmetric=False)
    assert not torch.equal(adj._col, adj.t()._col)
    new = rng.integers(0, 65, size=(2, 90))
    new[:, 0] = (64, 3)
    new[:, 1] = (5, 64)
    _check(adj, torch.from_numpy(new.astype(np.int64)).to(DEV), undirected=False)
    _check(adj, torch.zeros(2, 0, dtype=torch.int64, device=DEV), undirected=False)


def test_csr_only_product(hiplib, monkeypatch):
    """A² without bit rows: the two thin products from the A·B pattern kernels, united into it row by row."""
    from ocn_amd import ops
    from ocn_amd.update import insert_edges
    monkeypatch.setattr(ops, "a2_bitmap_max_bytes", 0)
    rng = np.random.default_rng(31)
    for n, undirected in ((97, True), (65, False), (1, True)):
        adj = _graph(n, 0.06, 30 + n, symmetric=undirected)
        adj2 = _product(adj)
        assert adj2.product_bit_rows() is None
        new = torch.from_numpy(rng.integers(0, n, size=(2, n + 3)).astype(np.int64)).to(DEV)
        want, want2 = _scratch(adj, new, undirected)
        got, got2 = insert_edges(adj, new, adj2, undirected=undirected)
        assert got2.product_bit_rows() is None
        _same_adj(got, want)
        _same_product(got2, want2, bits=False)
    n, _, adj = _hub_graph()
    new = torch.from_numpy(np.concatenate([np.array([[n - 1, 0], [0, 2700]]), rng.integers(0, n, size=(2, 200))], axis=1)).to(DEV)
    want, want2 = _scratch(adj, new)
    got, got2 = insert_edges(adj, new, _product(adj))
    _same_adj(got, want)
    _same_product(got2, want2, bits=False)


def test_closed_form_ten_cycle(hiplib):
    """The path 0 - 1 - ... - 9 with (0, 9) inserted is the 10-cycle: row r of A² is exactly {r, r ± 2 mod 10}."""
    from ocn_amd.update import insert_edges
    ST = _st()
    i = torch.arange(9, device=DEV)
    path = ST.from_edge_index(torch.stack([torch.cat([i, i + 1]), torch.cat([i + 1, i])]), sparse_sizes=(10, 10))
    adj, adj2 = insert_edges(path, torch.tensor([[0], [9]], device=DEV), _product(path))
    a_rows = [[1, 9], [0, 2], [1, 3], [2, 4], [3, 5], [4, 6], [5, 7], [6, 8], [7, 9], [0, 8]]
    a2_rows = [[0, 2, 8], [1, 3, 9], [0, 2, 4], [1, 3, 5], [2, 4, 6], [3, 5, 7], [4, 6, 8], [5, 7, 9], [0, 6, 8], [1, 7, 9]]
    assert adj._rowptr.tolist() == list(range(0, 21, 2)) and adj._col.tolist() == sum(a_rows, [])
    assert adj2._rowptr.tolist() == list(range(0, 31, 3)) and adj2.nnz() == 30 and adj2._col.tolist() == sum(a2_rows, [])
    want_bits = [sum(1 << c for c in row) for row in a2_rows]
    assert adj2.product_bit_rows().view(-1).tolist() == want_bits


def test_donate(hiplib):
    from ocn_amd.update import insert_edges
    rng = np.random.default_rng(41)
    adj = _graph(97, 0.05, 40)
    new = torch.from_numpy(rng.integers(0, 97, size=(2, 60)).astype(np.int64)).to(DEV)
    want, want2 = _scratch(adj, new)
    # donate=False: the old product still equals its former self
    adj2 = _product(adj)
    old_bits, old_rowptr, old_col = adj2.product_bit_rows().clone(), adj2._rowptr.clone(), adj2._col.clone()
    got, got2 = insert_edges(adj, new, adj2, donate=False)
    _same_product(got2, want2)
    assert got2.product_bit_rows().data_ptr() != adj2.product_bit_rows().data_ptr()
    assert torch.equal(adj2.product_bit_rows(), old_bits) and torch.equal(adj2._rowptr, old_rowptr) and torch.equal(adj2._col, old_col)
    # donate=True: the same result in the old storage, and the old object is of no use any more
    adj2 = _product(adj)
    where = adj2.product_bit_rows().data_ptr()
    got, got2 = insert_edges(adj, new, adj2, donate=True)
    assert got2.product_bit_rows().data_ptr() == where
    _same_adj(got, want)
    _same_product(got2, want2)
    with pytest.raises(Exception):
        adj2.nnz()
    assert adj2.product_bit_rows() is None


def test_rows_on_demand_product_is_completed_first(hiplib):
    from ocn_amd.update import insert_edges
    ST = _st()
    adj = _graph(97, 0.05, 50)
    lazy = ST._lazy_product(adj, adj)
    assert lazy.rows_on_demand()
    new = torch.tensor([[0, 96, 5], [96, 96, 7]], device=DEV)
    want, want2 = _scratch(adj, new)
    got, got2 = insert_edges(adj, new, lazy)
    assert not lazy.rows_on_demand()
    _same_adj(got, want)
    _same_product(got2, want2)


def test_updated_pair_feeds_the_scoring_and_recommendation_loops(hiplib):
    from ocn_amd import pipeline, recommend
    from ocn_amd.model import predictor_dict
    from ocn_amd.update import insert_edges
    n, H = 300, 64
    rng = np.random.default_rng(61)
    adj = _graph(n, 0.03, 60)
    new = torch.from_numpy(rng.integers(0, n, size=(2, 80)).astype(np.int64)).to(DEV)
    want, want2 = _scratch(adj, new)
    got, got2 = insert_edges(adj, new, _product(adj))
    torch.manual_seed(0)
    pred = predictor_dict["cn5"](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()
    h = torch.randn(n, H, device=DEV)
    edges = torch.from_numpy(rng.integers(0, n, size=(500, 2)).astype(np.int64)).to(DEV)
    args = SimpleNamespace(sum=0.5)
    with torch.no_grad():
        a = pipeline.score_edges(pred, h, got, got2, edges, 256, args)
        b = pipeline.score_edges(pred, h, want, want2, edges, 256, args)
    assert a.shape == (500,) and torch.equal(a, b)
    sources = torch.arange(0, n, 7, device=DEV)
    for x2, y2 in ((got2, want2), (None, None)):
        (ptr_a, cand_a), (ptr_b, cand_b) = recommend.two_hop_candidates(got, x2, sources), recommend.two_hop_candidates(want, y2, sources)
        assert cand_a.shape[0] > 0 and torch.equal(ptr_a, ptr_b) and torch.equal(cand_a, cand_b)


# ---- the union entries directly ------------------------------------------------------------------------------------------------
def _union_reference(rows_a, rows_b, n_cols):
    """torch.unique of the concatenated (row, column) keys."""
    key = torch.tensor([r * n_cols + c for rows in (rows_a, rows_b) for r, row in enumerate(rows) for c in row], dtype=torch.int64)
    key = torch.unique(key)
    cnt = torch.bincount(torch.div(key, n_cols, rounding_mode="floor"), minlength=len(rows_a))
    rp = torch.zeros(len(rows_a) + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(cnt, 0)
    return rp, (key % n_cols).to(torch.int32)


def _check_union(rows_a, rows_b, n_cols):
    from ocn_amd import ops
    a, b = _csr(rows_a), _csr(rows_b)
    want_rp, want_col = _union_reference(rows_a, rows_b, n_cols)
    for x, y in ((a, b), (b, a)):                                # the union is symmetric in its operands
        cnt = ops.csr_union_count(x[0], x[1], y[0], y[1])
        assert cnt.dtype == torch.int32 and cnt.tolist() == (want_rp[1:] - want_rp[:-1]).tolist()
        rp = ops.scan_i32(cnt)
        col = ops.csr_union_fill(x[0], x[1], y[0], y[1], rp)
        assert torch.equal(rp.cpu(), want_rp) and col.dtype == torch.int32 and torch.equal(col.cpu(), want_col)
        rp2, col2 = ops.csr_union(x[0], x[1], y[0], y[1])
        assert torch.equal(rp2, rp) and torch.equal(col2, col)


def test_csr_union_entries(hiplib):
    n_cols = 20000
    rng = np.random.default_rng(71)

    def row(k):
        return sorted(rng.choice(n_cols, size=k, replace=False).tolist())

    lens = [0, 1, 63, 64, 65, 5000]
    _check_union([[] for _ in lens], [[] for _ in lens], n_cols)                       # both empty
    a = [row(k) for k in lens]
    _check_union(a, [[] for _ in lens], n_cols)                                        # one empty
    _check_union(a, a, n_cols)                                                         # identical
    evens = [[2 * c for c in row(k) if 2 * c < n_cols] for k in lens]
    odds = [[2 * c + 1 for c in row(k) if 2 * c + 1 < n_cols] for k in lens]
    _check_union(evens, odds, n_cols)                                                  # disjoint
    # interleaved: every pairing of the lengths, rows that overlap in part (B takes some of A's columns and some of its own)
    rows_a, rows_b = [], []
    for ka in lens:
        for kb in lens:
            ra, rb = row(ka), row(kb)
            rows_a.append(ra)
            rows_b.append(sorted(set(rb[::2]) | set(ra[::3])))
    _check_union(rows_a, rows_b, n_cols)
    _check_union([[0], [n_cols - 1], []], [[n_cols - 1], [0, n_cols - 1], [5]], n_cols)   # the ends of the column range
