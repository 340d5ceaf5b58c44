"""Edge removal on the device (ocn_amd/update.py; ``ocn_csr_minus_*``, ``ocn_bitrows_remove``).  The oracle of every case is the
from-scratch route on the same device — ``from_edge_index`` of the remaining entries, then ``@`` — or a closed form written out
by hand.  Everything is bit-exact: no tolerance anywhere."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import csr_of_rows as _csr, edges_of as _edges_of, product_adj2 as _product, random_graph as _graph, \
    same_adj as _same_adj, same_product as _same_product, st as _st

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int64)).to(DEV)


def _scratch(adj, gone, undirected=True):
    """The long way round: the entries that stay, picked out in plain torch, sorted again; the whole product formed again."""
    n = adj.size(0)
    ei = _edges_of(adj)
    key = gone[0] * n + gone[1]
    if undirected:
        key = torch.cat([key, gone[1] * n + gone[0]])
    out = _st().from_edge_index(ei[:, ~torch.isin(ei[0] * n + ei[1], key)], sparse_sizes=(n, n))
    return out, _product(out)


def _check(adj, gone, undirected=True, donate=False):
    from ocn_amd.update import remove_edges
    adj2 = _product(adj)
    want, want2 = _scratch(adj, gone, undirected)
    got, got2 = remove_edges(adj, gone, adj2, undirected=undirected, donate=donate)
    _same_adj(got, want)
    _same_product(got2, want2)
    only, none = remove_edges(adj, gone, None, undirected=undirected)
    assert none is None
    _same_adj(only, want)
    return got, got2, want, want2


def _outcomes(adj, got, gone, undirected=True):
    """(bits cleared, candidates that survived through another witness) of one removal, from the entries themselves: the
    old A enumerates the candidates of the removed entries D = gone ∩ A (a superset changes neither figure)."""
    n = adj.size(0)
    a = torch.zeros(n, n, dtype=torch.bool, device=DEV)
    a[adj.storage.row(), adj.storage.col()] = True
    a_new = torch.zeros_like(a)
    a_new[got.storage.row(), got.storage.col()] = True
    d = a & ~a_new
    f, f_new, fd = a.float(), a_new.float(), d.float()
    cand = ((fd @ f) + (f @ fd)) > 0                          # (u, k): u -> v -> k with (u, v) in D; (r, v): r -> u -> v
    now = (f_new @ f_new) > 0
    return int((cand & ~now).sum()), int((cand & now).sum())


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65, 97])
def test_word_boundaries(hiplib, n):
    """Random symmetric graphs around the 32-bit word sizes, D of 1 .. 2N entries, half of them entries of A and half at
    random, always with the entries A has in row and column N - 1: the tail word and the last row."""
    rng = np.random.default_rng(200 + n)
    adj = _graph(n, 0.08, n)
    before = (adj._rowptr.clone(), adj._col.clone())
    ei = _edges_of(adj).cpu().numpy()
    last = ei[:, (ei[0] == n - 1) | (ei[1] == n - 1)]         # where A has them
    cleared = survived = 0
    for e in sorted({1, max(1, n // 2), 2 * n}):
        half = (e + 1) // 2
        parts = [rng.integers(0, n, size=(2, e - half)), last]
        if ei.shape[1]:
            parts.append(ei[:, rng.integers(0, ei.shape[1], size=half)])
        else:
            parts.append(rng.integers(0, n, size=(2, half)))
        gone = _dev(np.concatenate(parts, axis=1))
        got, got2, want, want2 = _check(adj, gone)
        c, s = _outcomes(adj, got, gone)
        cleared, survived = cleared + c, survived + s
    if n >= 31:
        assert cleared >= 1 and survived >= 1, (cleared, survived)   # both outcomes of a decision are exercised
    _check(adj, torch.zeros(2, 0, dtype=torch.int64, device=DEV))    # E == 0: the result equals the input in content
    assert torch.equal(adj._rowptr, before[0]) and torch.equal(adj._col, before[1])          # adj itself is never modified


# ---- closed forms ---------------------------------------------------------------------------------------------------------------
def _cycle(n):
    i = torch.arange(n, device=DEV)
    j = (i + 1) % n
    return _st().from_edge_index(torch.stack([torch.cat([i, j]), torch.cat([j, i])]), sparse_sizes=(n, n))


def test_closed_form_ten_cycle_to_path(hiplib):
    """The 10-cycle minus (0, 9) is the path 0 - 1 - ... - 9: row r of A² is {r - 2, r, r + 2} within 0 .. 9."""
    from ocn_amd.update import remove_edges
    cyc = _cycle(10)
    adj, adj2 = remove_edges(cyc, torch.tensor([[0], [9]], device=DEV), _product(cyc))
    a_rows = [[1], [0, 2], [1, 3], [2, 4], [3, 5], [4, 6], [5, 7], [6, 8], [7, 9], [8]]
    a2_rows = [[0, 2], [1, 3], [0, 2, 4], [1, 3, 5], [2, 4, 6], [3, 5, 7], [4, 6, 8], [5, 7, 9], [6, 8], [7, 9]]
    assert adj._rowptr.tolist() == [0, 1, 3, 5, 7, 9, 11, 13, 15, 17, 18] and adj._col.tolist() == sum(a_rows, [])
    assert adj2._rowptr.tolist() == [0, 2, 4, 7, 10, 13, 16, 19, 22, 24, 26] and adj2.nnz() == 26
    assert adj2._col.tolist() == sum(a2_rows, [])
    want_bits = [0b0000000101, 0b0000001010, 0b0000010101, 0b0000101010, 0b0001010100,
                 0b0010101000, 0b0101010000, 0b1010100000, 0b0101000000, 0b1010000000]
    assert adj2.product_bit_rows().view(-1).tolist() == want_bits


def _remove_direct(adj, adj_new, gone):
    """``ops.bitrows_remove`` itself on a symmetric pair: (bits, removed)."""
    from ocn_amd import ops
    n = adj.size(0)
    d = _st().from_edge_index(gone, sparse_sizes=(n, n)).to_symmetric()
    bits = _product(adj).product_bit_rows().clone()
    removed = ops.bitrows_remove(adj._rowptr, adj._col, adj._rowptr, adj._col, adj_new._rowptr, adj_new._col, adj_new._rowptr,
                                 adj_new._col, d._rowptr, d._col, bits)
    return bits, removed


def test_closed_form_four_cycle(hiplib):
    cyc = _cycle(4)                                             # 0 - 1 - 2 - 3 - 0: A² row r = {r, r ± 2}
    # minus (0, 1): the path 1 - 2 - 3 - 0.  Every candidate survives through the other witness: A² is unchanged
    gone = torch.tensor([[0], [1]], device=DEV)
    got, got2, want, want2 = _check(cyc, gone)
    assert got._rowptr.tolist() == [0, 1, 2, 4, 6] and got._col.tolist() == [3, 2, 1, 3, 0, 2]
    assert got2._rowptr.tolist() == [0, 2, 4, 6, 8] and got2._col.tolist() == [0, 2, 1, 3, 0, 2, 1, 3]
    bits, removed = _remove_direct(cyc, got, gone)
    assert removed.tolist() == [0, 0, 0, 0]
    assert bits.view(-1).tolist() == [0b0101, 0b1010, 0b0101, 0b1010]
    # minus (0, 1) and (2, 3) at once: the two edges 1 - 2 and 3 - 0 remain, A'² is the identity pattern
    gone = torch.tensor([[0, 2], [1, 3]], device=DEV)
    got, got2, want, want2 = _check(cyc, gone)
    assert got._rowptr.tolist() == [0, 1, 2, 3, 4] and got._col.tolist() == [3, 2, 1, 0]
    assert got2._rowptr.tolist() == [0, 1, 2, 3, 4] and got2._col.tolist() == [0, 1, 2, 3]
    bits, removed = _remove_direct(cyc, got, gone)
    assert removed.tolist() == [1, 1, 1, 1]
    assert bits.view(-1).tolist() == [0b0001, 0b0010, 0b0100, 0b1000]


def test_removing_every_entry_leaves_nothing(hiplib):
    for adj, undirected in ((_graph(97, 0.06, 81), True), (_graph(65, 0.06, 82, symmetric=False), False)):
        got, got2, want, want2 = _check(adj, _edges_of(adj), undirected=undirected)
        assert got.nnz() == 0 and got2.nnz() == 0
        assert int(got._rowptr.abs().sum()) == 0 and int(got2._rowptr.abs().sum()) == 0
        assert int(got2.product_bit_rows().ne(0).sum()) == 0


# ---- hubs -----------------------------------------------------------------------------------------------------------------------
N_HUB = 4100


def _hub_graph(extra=()):
    """Node 0 is adjacent to 2 .. 2501 and node 1 to 2501 .. 4000: 2501 is their only shared leaf and 0 and 1 are not
    adjacent.  A few thousand sparse random edges join the other nodes (none touches 0 or 1).  ``extra``: further edges."""
    rng = np.random.default_rng(7)
    h0 = np.stack([np.zeros(2500, dtype=np.int64), np.arange(2, 2502)])
    h1 = np.stack([np.ones(1500, dtype=np.int64), np.arange(2501, 4001)])
    rest = rng.integers(2, N_HUB, size=(2, 4000))
    parts = [h0, h1, rest] + ([np.array(extra, dtype=np.int64).T] if len(extra) else [])
    adj = _st().from_edge_index(_dev(np.concatenate(parts, axis=1)), sparse_sizes=(N_HUB, N_HUB)).to_symmetric()
    rc = adj.storage.rowcount()
    assert int(rc[0]) == 2500 + sum(1 for e in extra if 0 in e) and int(rc[1]) == 1500 + sum(1 for e in extra if 1 in e)
    return adj


def _bit(sp, r, k):
    return bool((int(sp.product_bit_rows()[r, k >> 5]) >> (k & 31)) & 1)


def test_hub_pair_loses_its_only_witness(hiplib):
    """(0, 2501) leaves: bits (0, 1) and (1, 0) clear after a search of the full rows of both hubs (2 499 and 1 500 columns:
    the wave-cooperative form) that finds no witness."""
    adj = _hub_graph()
    adj2 = _product(adj)
    assert _bit(adj2, 0, 1) and _bit(adj2, 1, 0)
    got, got2, want, want2 = _check(adj, torch.tensor([[0], [2501]], device=DEV))
    assert not _bit(got2, 0, 1) and not _bit(got2, 1, 0)
    assert _bit(got2, 0, 0) and _bit(got2, 1, 1) and _bit(got2, 2501, 2501)


def test_hub_pair_keeps_its_second_witness(hiplib):
    adj = _hub_graph(extra=[(0, 4050), (1, 4050)])             # a second shared leaf, beyond both hubs' other columns
    got, got2, want, want2 = _check(adj, torch.tensor([[2501], [0]], device=DEV))
    assert _bit(got2, 0, 1) and _bit(got2, 1, 0)
    adj = _hub_graph(extra=[(0, 4050), (1, 4050)])
    got, got2, want, want2 = _check(adj, torch.tensor([[0], [4050]], device=DEV))          # ... and the other way round
    assert _bit(got2, 0, 1) and _bit(got2, 1, 0)


def test_hub_loses_three_hundred_leaves_at_once(hiplib):
    """A D row longer than a wave.  A leaf whose only edge went becomes isolated, and its A² row goes from the hub's 2 500
    bits to none (kind a over many chunks); every neighbour the hub keeps loses that leaf's bit (kind b over many chunks)."""
    adj = _hub_graph()
    rc = adj.storage.rowcount()
    leaves = torch.arange(2, 2501, device=DEV)
    only_hub = leaves[rc[leaves] == 1]                          # leaves with no edge but the hub's
    assert only_hub.numel() >= 1
    leaf = int(only_hub[0])
    others = leaves[leaves != leaf][:: 8][:299]
    gone = torch.stack([torch.zeros(300, dtype=torch.int64, device=DEV), torch.cat([torch.tensor([leaf], device=DEV), others])])
    adj2 = _product(adj)
    assert int(adj2.storage.rowcount()[leaf]) == 2500 and _bit(adj2, 2501, leaf)
    got, got2, want, want2 = _check(adj, gone)
    assert int(got.storage.rowcount()[leaf]) == 0 and int(got2.storage.rowcount()[leaf]) == 0
    assert int(got.storage.rowcount()[0]) == 2200
    assert not _bit(got2, 2501, leaf)                          # 2501 is still the hub's neighbour, the leaf no longer


# ---- D that overlaps A in part, or not at all ---------------------------------------------------------------------------------
def test_non_edges_and_repeats(hiplib):
    from ocn_amd import ops
    from ocn_amd.update import remove_edges
    n = 200
    adj = _graph(n, 0.03, 11)
    adj2 = _product(adj)
    rng = np.random.default_rng(12)
    # D disjoint from A: nothing changes and nothing counts
    cand = _dev(rng.integers(0, n, size=(2, 400)))
    ei = _edges_of(adj)
    non = cand[:, ~torch.isin(cand[0] * n + cand[1], ei[0] * n + ei[1])]
    assert non.shape[1] > 300
    got, got2 = remove_edges(adj, non, adj2)
    _same_adj(got, adj)
    _same_product(got2, adj2)
    d = _st().from_edge_index(non, sparse_sizes=(n, n)).to_symmetric()
    bits = adj2.product_bit_rows().clone()
    removed = ops.bitrows_remove(adj._rowptr, adj._col, adj._rowptr, adj._col, adj._rowptr, adj._col, adj._rowptr, adj._col,
                                 d._rowptr, d._col, bits)
    assert int(removed.abs().sum()) == 0 and torch.equal(bits, adj2.product_bit_rows())
    # D with every entry four times, shuffled = D once
    once_e = torch.cat([ei[:, ::5], non[:, :50]], dim=1)
    m = once_e.shape[1]
    four = torch.cat([once_e] * 4, dim=1)[:, torch.randperm(4 * m, generator=torch.Generator().manual_seed(1)).to(DEV)]
    once, once2 = remove_edges(adj, once_e, adj2)
    many, many2 = remove_edges(adj, four, adj2)
    assert once.nnz() < adj.nnz()
    _same_adj(many, once)
    _same_product(many2, once2)
    _check(adj, four)


def test_directed_removal_reads_both_transposes(hiplib):
    rng = np.random.default_rng(21)
    n = 65
    adj = _graph(n, 0.06, 20, symmetric=False)
    assert not torch.equal(adj._col, adj.t()._col)
    ei = _edges_of(adj).cpu().numpy()
    last = ei[:, (ei[0] == n - 1) | (ei[1] == n - 1)]
    assert (last[0] == n - 1).any() and (last[1] == n - 1).any()
    gone = np.concatenate([ei[:, rng.integers(0, ei.shape[1], size=60)], rng.integers(0, n, size=(2, 30)), last], axis=1)
    got, got2, want, want2 = _check(adj, _dev(gone), undirected=False)
    assert got.nnz() < adj.nnz() and got2.nnz() < _product(adj).nnz()
    # a directed removal takes (r, c) and leaves (c, r)
    r, c = int(ei[0, 0]), int(ei[1, 0])
    one = _check(adj, torch.tensor([[r], [c]], device=DEV), undirected=False)[0]
    assert one.nnz() == adj.nnz() - 1
    _check(adj, torch.zeros(2, 0, dtype=torch.int64, device=DEV), undirected=False)


# ---- the loop closed: insert, then remove ---------------------------------------------------------------------------------------
def _disjoint_new(adj, n, count, seed):
    rng = np.random.default_rng(seed)
    cand = _dev(rng.integers(0, n, size=(2, count)))
    ei = _edges_of(adj)
    key = ei[0] * n + ei[1]
    keep = ~torch.isin(cand[0] * n + cand[1], key) & ~torch.isin(cand[1] * n + cand[0], key)
    return cand[:, keep]


@pytest.mark.parametrize("donate", [False, True])
def test_round_trip_restores_the_pair(hiplib, donate):
    from ocn_amd.update import insert_edges, remove_edges
    n = 97
    adj = _graph(n, 0.05, 40)
    new = _disjoint_new(adj, n, 80, 41)
    assert new.shape[1] > 40
    adj2 = _product(adj)
    keep_bits, keep_rowptr, keep_col = adj2.product_bit_rows().clone(), adj2._rowptr.clone(), adj2._col.clone()
    mid, mid2 = insert_edges(adj, new, adj2)
    assert mid.nnz() > adj.nnz() and mid2.nnz() > adj2.nnz()
    mid_bits, mid_rowptr, mid_col = mid2.product_bit_rows().clone(), mid2._rowptr.clone(), mid2._col.clone()
    where = mid2.product_bit_rows().data_ptr()
    back, back2 = remove_edges(mid, new, mid2, donate=donate)
    _same_adj(back, adj)
    assert torch.equal(back2.product_bit_rows(), keep_bits) and torch.equal(back2._rowptr, keep_rowptr)
    assert back2.nnz() == adj2.nnz() and torch.equal(back2._col, keep_col)
    if donate:
        assert back2.product_bit_rows().data_ptr() == where
        with pytest.raises(Exception):
            mid2.nnz()
        assert mid2.product_bit_rows() is None
    else:
        assert back2.product_bit_rows().data_ptr() != where
        assert torch.equal(mid2.product_bit_rows(), mid_bits) and torch.equal(mid2._rowptr, mid_rowptr) and torch.equal(mid2._col, mid_col)


def test_rows_on_demand_product_stays_lazy(hiplib):
    from ocn_amd.update import remove_edges
    ST = _st()
    adj = _graph(97, 0.05, 50)
    ei = _edges_of(adj)
    gone = torch.cat([ei[:, ::7], torch.tensor([[0, 96], [96, 96]], device=DEV)], dim=1)
    want, want2 = _scratch(adj, gone)
    for donate in (False, True):
        lazy = ST._lazy_product(adj, adj)
        assert lazy.rows_on_demand()
        got, got2 = remove_edges(adj, gone, lazy, donate=donate)
        assert got2.rows_on_demand()                            # not completed: lazy again
        if donate:
            with pytest.raises(Exception):
                lazy.nnz()
        else:
            assert lazy.rows_on_demand()                        # ... and the old one was not completed either
        _same_adj(got, want)
        _same_product(got2, want2)                              # (completes it)
        assert not got2.rows_on_demand()


def test_csr_only_product(hiplib, monkeypatch):
    """A² without bit rows: formed again from A' with the pattern kernels."""
    from ocn_amd import ops
    from ocn_amd.update import remove_edges
    monkeypatch.setattr(ops, "a2_bitmap_max_bytes", 0)
    rng = np.random.default_rng(31)
    for n, undirected in ((97, True), (65, False), (1, True)):
        adj = _graph(n, 0.06, 30 + n, symmetric=undirected)
        adj2 = _product(adj)
        assert adj2.product_bit_rows() is None
        ei = _edges_of(adj)
        gone = torch.cat([ei[:, ::4], _dev(rng.integers(0, n, size=(2, n + 3)))], dim=1)
        want, want2 = _scratch(adj, gone, undirected)
        got, got2 = remove_edges(adj, gone, adj2, undirected=undirected)
        assert got2.product_bit_rows() is None
        _same_adj(got, want)
        _same_product(got2, want2, bits=False)


def test_updated_pair_feeds_the_scoring_and_recommendation_loops(hiplib):
    from ocn_amd import pipeline, recommend
    from ocn_amd.model import predictor_dict
    from ocn_amd.update import remove_edges
    n, H = 300, 64
    rng = np.random.default_rng(61)
    adj = _graph(n, 0.03, 60)
    ei = _edges_of(adj)
    gone = torch.cat([ei[:, ::6], _dev(rng.integers(0, n, size=(2, 40)))], dim=1)
    want, want2 = _scratch(adj, gone)
    got, got2 = remove_edges(adj, gone, _product(adj))
    torch.manual_seed(0)
    pred = predictor_dict["cn5"](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()
    h = torch.randn(n, H, device=DEV)
    edges = _dev(rng.integers(0, n, size=(500, 2)))
    args = SimpleNamespace(sum=0.5)
    with torch.no_grad():
        a = pipeline.score_edges(pred, h, got, got2, edges, 256, args)
        b = pipeline.score_edges(pred, h, want, want2, edges, 256, args)
    assert a.shape == (500,) and torch.equal(a, b)
    sources = torch.arange(0, n, 7, device=DEV)
    for x2, y2 in ((got2, want2), (None, None)):
        (ptr_a, cand_a), (ptr_b, cand_b) = recommend.two_hop_candidates(got, x2, sources), recommend.two_hop_candidates(want, y2, sources)
        assert cand_a.shape[0] > 0 and torch.equal(ptr_a, ptr_b) and torch.equal(cand_a, cand_b)


# ---- the difference entries directly --------------------------------------------------------------------------------------------
def _keys(rows, n_cols):
    return torch.tensor([r * n_cols + c for r, row in enumerate(rows) for c in row], dtype=torch.int64)


def _minus_reference(rows_a, rows_b, n_cols):
    """torch.unique of A's (row, column) keys without those torch.isin finds among B's."""
    ka, kb = _keys(rows_a, n_cols), _keys(rows_b, n_cols)
    key = torch.unique(ka[~torch.isin(ka, kb)])
    cnt = torch.bincount(torch.div(key, n_cols, rounding_mode="floor"), minlength=len(rows_a))
    rp = torch.zeros(len(rows_a) + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(cnt, 0)
    return rp, (key % n_cols).to(torch.int32)


def _check_minus(rows_a, rows_b, n_cols):
    from ocn_amd import ops
    a, b = _csr(rows_a), _csr(rows_b)
    for (x, rows_x), (y, rows_y) in (((a, rows_a), (b, rows_b)), ((b, rows_b), (a, rows_a))):      # A \ B and B \ A
        want_rp, want_col = _minus_reference(rows_x, rows_y, n_cols)
        cnt = ops.csr_minus_count(x[0], x[1], y[0], y[1])
        assert cnt.dtype == torch.int32 and cnt.tolist() == (want_rp[1:] - want_rp[:-1]).tolist()
        rp = ops.scan_i32(cnt)
        col = ops.csr_minus_fill(x[0], x[1], y[0], y[1], rp)
        assert torch.equal(rp.cpu(), want_rp) and col.dtype == torch.int32 and torch.equal(col.cpu(), want_col)
        rp2, col2 = ops.csr_minus(x[0], x[1], y[0], y[1])
        assert torch.equal(rp2, rp) and torch.equal(col2, col)


def test_csr_minus_entries(hiplib):
    n_cols = 20000
    rng = np.random.default_rng(71)

    def row(k):
        return sorted(rng.choice(n_cols, size=k, replace=False).tolist())

    lens = [0, 1, 63, 64, 65, 5000]
    _check_minus([[] for _ in lens], [[] for _ in lens], n_cols)                       # both empty
    a = [row(k) for k in lens]
    _check_minus(a, [[] for _ in lens], n_cols)                                        # B empty (and, swapped, A empty)
    _check_minus(a, a, n_cols)                                                         # identical
    evens = [[2 * c for c in row(k) if 2 * c < n_cols] for k in lens]
    odds = [[2 * c + 1 for c in row(k) if 2 * c + 1 < n_cols] for k in lens]
    _check_minus(evens, odds, n_cols)                                                  # disjoint
    # every pairing of the lengths, rows that overlap in part (B takes some of A's columns and some of its own)
    rows_a, rows_b = [], []
    for ka in lens:
        for kb in lens:
            ra, rb = row(ka), row(kb)
            rows_a.append(ra)
            rows_b.append(sorted(set(rb[::2]) | set(ra[::3])))
    _check_minus(rows_a, rows_b, n_cols)
    # every pairing again with B of exactly the length (its columns drawn from A's where A has enough)
    rows_a, rows_b = [], []
    for ka in lens:
        for kb in lens:
            ra = row(ka)
            in_a = set(ra)
            pool = ra[::2] + [c for c in row(kb) if c not in in_a]
            rows_a.append(ra)
            rows_b.append(sorted(pool[:kb]))
    assert sorted({len(r) for r in rows_b}) == lens
    _check_minus(rows_a, rows_b, n_cols)
    _check_minus([[0], [n_cols - 1], [0, n_cols - 1], []], [[n_cols - 1], [0, n_cols - 1], [0], [5]], n_cols)   # the ends of the range
