"""cn6 without a stored A³ on the GPU: ``ops.cn3_flags`` / ``utils.adjoverlap_3hop`` / ``CNState3(adj, adj2, None, e)`` against
(a) dense boolean algebra on the CPU — P3 = (A @ A @ A) > 0 in int64 numpy; for candidate e the expected flag row is
P3[dst[e], N(src[e])], the counts and the column histogram follow from it — and (b) the materialised route
``CNState(adj, adj3, None, e)`` with adj3 from torch's sparse product.  Everything is integer- or bit-exact."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import ocn_oracle as O
from tests.helpers import batch, close, make_graph, product_adj2, random_graph, to_product

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENTRY = 1 | (1 << 42)           # what one cn3 entry adds to word 0 of its column's histogram: n1 and n_union


def _dense(adj):
    return (adj.to_dense().cpu().numpy() != 0).astype(np.int64)


def _reference(A, e):
    """(flags of the whole batch, concatenated in batch order; cnt3 [B]; hist word 0 [N]) from the dense A."""
    P3 = (A @ A @ A) > 0
    rows, hist = [], np.zeros(A.shape[1], dtype=np.int64)
    for i, j in zip(*e.cpu().numpy()):
        nb = np.nonzero(A[i])[0]
        f = P3[j, nb]
        rows.append(f.astype(np.uint8))
        np.add.at(hist, nb[f], ENTRY)
    cnt = np.array([int(r.sum()) for r in rows], dtype=np.int32).reshape(-1)
    return (np.concatenate(rows) if rows else np.zeros(0, np.uint8)), cnt, hist


def _adj3(adj, adj2):
    from ocn_amd.sparse import SparseTensor
    return SparseTensor.from_torch_sparse_coo_tensor(adj2.to_torch_sparse_coo_tensor() @ adj.to_torch_sparse_coo_tensor(), False)


def _same_as_reference(st, ref):
    """A state of the (A, A³) pass (``CNState3.b`` or a hop3 handle's) against the dense reference."""
    flags, cnt, hist = ref
    assert st.flags[:flags.size].cpu().numpy().tolist() == flags.tolist()
    assert st.cnt1.cpu().numpy().tolist() == cnt.tolist()
    assert st.hist[:, 0].cpu().numpy().tolist() == hist.tolist() and not bool(st.hist[:, 1].any())
    assert st.status.cpu().tolist() == [0, 0, 0, 0]


def _same_states(b, m, total):
    """The A³-free pass ``b`` against the materialised pass ``m``: the bytes ``ocn_cn_flags`` leaves."""
    assert torch.equal(b.flags[:total], m.flags[:total]) and torch.equal(b.cnt1, m.cnt1) and torch.equal(b.hist, m.hist)


def _raw(adj, adj2, e, order=None, nds=None, undirected=True):
    """``ops.cn3_flags`` itself on offsets of its own: (flags, hist, cnt3, status, total)."""
    from ocn_amd import ops
    from ocn_amd.utils import _a2_bit_rows, _transposed
    src, dst = e[0].contiguous(), e[1].contiguous()
    off = ops.edge_offsets(adj._rowptr, src)
    rpt, colt, _ = _transposed(adj, undirected)
    out = ops.cn3_flags(adj._rowptr, adj._col, rpt, colt, _a2_bit_rows(adj2, dst), src, dst, adj.size(1), off, order,
                        adj.max_rowcount(), nds=nds)
    return out + (int(off[-1]),)


# ---- 1. the boundary graph -------------------------------------------------------------------------------------------
def _boundary_graph():
    """N = 100 (4 words per bit row, the last one partly used), directed so that every length can be set by hand.
    Source rows (out-degree): 10: 0, 11: 1, 12: 63, 13: 64, 14: 65, 15: 99.  Rows of Aᵀ (in-degree): column 23: 1, 22: 64,
    21: 65, 20: 99.  Column 24 has the in-neighbours {15, 95}; target 96 reaches 95 in two steps (96 -> 97 -> 95) and 15 not
    at all (only 15 points to 15), so for the candidate (15, 96) the only witness of neighbour 24 is the LAST entry of its
    row; neighbour 23 of the same candidate (in-neighbour 15 only) has no witness.  Row 10 is empty: as a target its row of
    A² is empty.  The free rows carry a sparse random pattern on columns 30..99."""
    n = 100
    A = np.zeros((n, n), dtype=bool)
    free = [r for r in range(n) if not 10 <= r <= 15]
    rng = np.random.default_rng(5)
    for r in free:
        A[r, 30:] = rng.random(n - 30) < 0.04
        A[r, 15] = False
    A[:, 20] = True
    A[16:77, 21] = True
    A[16:77, 22] = True
    A[10], A[11], A[12], A[13], A[14], A[15] = False, False, False, False, False, False
    A[11, 20] = True
    A[12, [20, 21]] = True; A[12, 30:91] = True
    A[13, [20, 21, 22]] = True; A[13, 30:91] = True
    A[14, [20, 21, 22]] = True; A[14, 30:92] = True
    A[15, :99] = True
    A[95, 24] = True
    A[96, 97] = True
    A[97, 95] = True
    return A


def test_boundary_graph(hiplib):
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.utils import CNState3, adjoverlap_3hop
    Ab = _boundary_graph()
    A = Ab.astype(np.int64)
    assert [int(A[r].sum()) for r in range(10, 16)] == [0, 1, 63, 64, 65, 99]
    assert [int(A[:, c].sum()) for c in (23, 22, 21, 20)] == [1, 64, 65, 99]
    P2 = (A @ A) > 0
    assert np.nonzero(A[:, 24])[0].tolist() == [15, 95] and P2[96, [15, 95]].tolist() == [False, True]      # last entry only
    assert np.nonzero(A[:, 23])[0].tolist() == [15] and not P2[96, 15] and A[15, 23]                        # no witness
    assert not P2[10].any()                                                                                  # isolated target
    r, c = np.nonzero(Ab)
    adj = SparseTensor.from_edge_index(torch.from_numpy(np.stack([r, c])).to(DEV), sparse_sizes=(100, 100))
    adj2 = product_adj2(adj)
    assert adj2.product_bit_rows().shape == (100, 4)
    e = torch.tensor([[15, 15, 15, 15, 10, 11, 12, 13, 14, 15, 12, 14, 13, 40, 96, 11],
                      [96, 40, 96, 15, 96, 96, 96, 16, 50, 10, 12, 10, 97, 15, 96, 10]], device=DEV)
    ref = _reference(A, e)
    assert 0 < ref[0].sum() < ref[0].size and ref[1][0] == ref[1][2] and ref[1][4] == 0 and ref[1][9] == 0
    p24 = np.nonzero(A[15])[0].tolist().index(24)
    p23 = np.nonzero(A[15])[0].tolist().index(23)
    assert ref[0][p24] == 1 and ref[0][p23] == 0

    st = CNState3(adj, adj2, None, e, undirected=False)
    _same_as_reference(st.b, ref)
    _same_states(st.b, CNState3(adj, adj2, _adj3(adj, adj2), e).b, ref[0].size)
    h3 = adjoverlap_3hop(adj, adj2, e, undirected=False)                 # standing alone: its own offsets
    assert h3.counts().cpu().tolist() == ref[1].tolist()
    m = h3.materialize()
    assert m.sizes() == [16, 100] and m.nnz() == int(ref[1].sum())
    assert torch.equal(m.to_dense().cpu()[0] != 0, torch.from_numpy(((A @ A @ A) > 0)[96] & Ab[15]))

    # the entry itself: batch order, a permutation as `order`, and items of one 64-neighbour chunk (no nds: rows 14 and 15
    # then take two items each, whose counts meet in one atomic counter)
    nds = torch.from_numpy(A @ A.sum(axis=0)).to(DEV)
    perm = torch.randperm(16, generator=torch.Generator().manual_seed(1)).to(DEV)
    for order, w in ((None, nds), (perm, nds), (None, None), (perm, None)):
        flags, hist, cnt3, status, total = _raw(adj, adj2, e, order, w, undirected=False)
        _same_as_reference(SimpleNamespace(flags=flags, hist=hist, cnt1=cnt3, status=status), ref)
        assert total == ref[0].size

    one = e[:, :1].contiguous()                                          # B = 1
    _same_as_reference(CNState3(adj, adj2, None, one, undirected=False).b, _reference(A, one))
    none = e[:, :0].contiguous()                                         # B = 0: empty outputs, no launch error
    flags, hist, cnt3, status, total = _raw(adj, adj2, none, undirected=False)
    assert total == 0 and cnt3.numel() == 0 and not bool(hist.any()) and status.cpu().tolist() == [0, 0, 0, 0]
    st0 = CNState3(adj, adj2, None, none, undirected=False)
    assert st0.cnt3.numel() == 0 and not bool(st0.b.hist.any())
    torch.cuda.synchronize()


# ---- 2. every pair of a small random graph ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 65])
def test_every_pair_of_a_random_graph(hiplib, n):
    from ocn_amd import ops
    from ocn_amd.utils import CNState, CNState3
    adj = random_graph(n, 0.1, seed=n)
    adj2 = product_adj2(adj)
    ii, jj = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
    e = torch.stack([ii.reshape(-1), jj.reshape(-1)]).to(DEV)
    assert (e.shape[1] >= ops.sort_edges_min_batch) == (n == 65)
    st = CNState3(adj, adj2, None, e)
    assert (st.a.order is not None) == (n == 65)
    ref = _reference(_dense(adj), e)
    _same_as_reference(st.b, ref)
    _same_states(st.b, CNState(adj, _adj3(adj, adj2), None, e), ref[0].size)


# ---- 3. a directed graph ---------------------------------------------------------------------------------------------
def test_directed_graph_reads_the_transpose(hiplib):
    from ocn_amd.utils import CNState3
    n = 70
    adj = random_graph(n, 0.1, seed=7, symmetric=False)
    adj2 = product_adj2(adj)
    g = torch.Generator().manual_seed(3)
    e = torch.randint(0, n, (2, 900), generator=g).to(DEV)
    ref = _reference(_dense(adj), e)
    st = CNState3(adj, adj2, None, e, undirected=False)
    _same_as_reference(st.b, ref)
    sym = CNState3(adj, adj2, None, e, undirected=True)                 # A's own rows in place of Aᵀ's: another matrix
    assert sym.b.flags[:ref[0].size].cpu().numpy().tolist() != ref[0].tolist()


# ---- 4 / 5 / 6 / 7. the case3 graph of test_parity_gpu.py ------------------------------------------------------------
@pytest.fixture(scope="module")
def case3(hiplib):
    n, B = 1500, 1200
    oadj = make_graph(n, 5, 60, 31, isolated=7)
    oadj2 = O.adj2_sparse(oadj)
    oadj3 = O.adj3_sparse(oadj, oadj2)
    e = batch(oadj, B, 91)
    adj = to_product(oadj, DEV)
    adj2 = product_adj2(adj)
    return SimpleNamespace(n=n, B=B, e=e, ed=e.to(DEV), adj=adj, adj2=adj2, adj3=_adj3(adj, adj2),
                           ocn=[O.adjoverlap(oadj, t, e) for t in (oadj, oadj2, oadj3)])


def _adj2_forms(c):
    from ocn_amd.sparse import SparseTensor
    lazy = SparseTensor._lazy_product(c.adj, c.adj)
    csr = SparseTensor(rowptr=c.adj2._rowptr.clone(), col=c.adj2._col.clone(), sparse_sizes=(c.n, c.n))
    assert lazy.rows_on_demand() and csr.product_bit_rows() is None
    return {"product": c.adj2, "rows_on_demand": lazy, "from_csr": csr}


@pytest.mark.parametrize("form", ["product", "rows_on_demand", "from_csr"])
def test_state_equals_the_materialised_route(case3, form):
    from ocn_amd.utils import CNState3
    c = case3
    adj2 = _adj2_forms(c)[form]
    x = torch.randn(c.n, 64, generator=torch.Generator().manual_seed(2)).to(DEV)
    for ip in (0.0, 0.37):
        free, mat = CNState3(c.adj, adj2, None, c.ed), CNState3(c.adj, c.adj2, c.adj3, c.ed)
        total = int(mat.a.off[-1])
        assert torch.equal(free.b.flags[:total], mat.b.flags[:total])
        assert torch.equal(free.cnt3, mat.cnt3) and torch.equal(free.b.hist, mat.b.hist)
        assert torch.equal(free.b.status, mat.b.status) and torch.equal(free.b.scal, mat.b.scal)
        assert free.cnt3.cpu().tolist() == torch.bincount(c.ocn[2].row, minlength=c.B).tolist()
        ipt = torch.tensor([ip], device=DEV)
        wf, wm = free.weights(ipt), mat.weights(ipt)
        assert all(torch.equal(a, b) for a, b in zip(wf, wm))
        assert all(torch.equal(a, b) for a, b in zip(free.gather(*wf, x), mat.gather(*wm, x)))


def _predictor(H, ln):
    from ocn_amd.model import predictor_dict
    torch.manual_seed(13)
    pred = predictor_dict["cn6"](H, H, 1, 3, 0.1, 0.0, ln, use_xlin=True, tailact=True, beta=0.7).eval()
    with torch.no_grad():
        pred.alpha.copy_(torch.tensor([0.3, -0.2, 0.9]))
    return pred


U = 2.0 ** -24


def _backward_reference(a, N):
    """fp64 sum and absolute sum per node of the terms ``ops.cn_gather3_backward`` adds, from its own arguments (the weights
    formed in fp32 in the kernel's order: tests/test_pool_backward_gpu.py, _check3), and the number of terms per node."""
    (rowptr, col, src, dst, off, fa_all, fb_all, wA, wB, nip, h, g1, g2, g3, g4) = [t.cpu() for t in a]
    B, total = src.numel(), int(off[-1])
    e = torch.repeat_interleave(torch.arange(B), off[1:] - off[:-1])
    key = torch.arange(total)
    k = col[rowptr[src[e]] + key - off[e]].long()
    fa_all, fb_all = fa_all[:total].int(), fb_all[:total].int() & 1
    live = (fa_all | fb_all) != 0
    e, k, fa, fb = e[live], k[live], fa_all[live], fb_all[live] != 0
    aw, inv3 = wA[k], wB[k][:, 0]
    zero, one = torch.zeros(()), torch.ones(())
    cn1, cn2 = (fa & 1) != 0, (fa & 2) != 0
    tt = torch.where(cn1, aw[:, 1], zero)
    w1 = torch.where(cn1, aw[:, 0], zero)
    w2 = (torch.where(cn2, one, zero) - tt) * aw[:, 2]
    w3 = ((torch.where(fb, one, zero) - tt) - nip * w2) * inv3
    node = torch.cat([k, src, dst])
    L = torch.bincount(node, minlength=N)
    p1, p2, p3 = (w.double()[:, None] * t[e].double() for w, t in ((w1, g1), (w2, g2), (w3, g3)))
    ps, pd = g4.double() * h[dst].double(), g4.double() * h[src].double()
    H = h.shape[1]
    ref = torch.zeros(N, H, dtype=torch.float64).index_add_(0, node, torch.cat([p1 + p2 + p3, ps, pd]))
    A = torch.zeros(N, H, dtype=torch.float64).index_add_(0, node, torch.cat([p1.abs() + p2.abs() + p3.abs(), ps.abs(), pd.abs()]))
    return ref, A, L


@pytest.mark.parametrize("H,ln", [(64, True), (256, False)])
def test_scores_and_gradient_equal_the_materialised_route(case3, H, ln, monkeypatch):
    """Scores: bit-equal to the materialised route and ``close`` to the oracle.  Gradient with respect to x: the backward of
    the pooling adds its terms with fp32 atomics, whose arrival order is not fixed, so two launches on the same bytes need
    not agree in the last bits.  What IS fixed is asserted: the two routes hand the backward byte-identical arguments; and each
    gradient lies within the bound tests/test_pool_backward_gpu.py derives for the atomic form, gamma(L + 3) * sum |terms| per
    node against the fp64 sum (L terms per node, three more roundings inside a term)."""
    from ocn_amd import ops
    from ocn_amd.utils import adjoverlap, adjoverlap_3hop
    c = case3
    pred = _predictor(H, ln)
    sd = {k: v.detach().clone() for k, v in pred.state_dict().items()}
    x = torch.randn(c.n, H, generator=torch.Generator().manual_seed(H))
    ref = O.cn6_forward(sd, x, *c.ocn, c.e, ln, True)
    pred = pred.to(DEV)
    xd = x.to(DEV)
    cn = lambda: (adjoverlap(c.adj, c.adj, c.ed), adjoverlap(c.adj, c.adj2, c.ed))
    with torch.no_grad():
        free = pred(xd, c.adj, *cn(), adjoverlap_3hop(c.adj, c.adj2, c.ed), c.ed, None)
        mat = pred(xd, c.adj, *cn(), adjoverlap(c.adj, c.adj3, c.ed), c.ed, None)
    assert free.shape == (c.B, 1) and torch.equal(free, mat)
    assert close(free, ref), (free.cpu() - ref).abs().max()

    calls = []
    real = ops.cn_gather3_backward

    def spy(*a, **kw):
        calls.append((a, kw))
        return real(*a, **kw)
    monkeypatch.setattr(ops, "cn_gather3_backward", spy)
    grads = []
    for third in (lambda: adjoverlap_3hop(c.adj, c.adj2, c.ed), lambda: adjoverlap(c.adj, c.adj3, c.ed)):
        xg = xd.clone().requires_grad_()
        pred.zero_grad()
        pred(xg, c.adj, *cn(), third(), c.ed, None).sum().backward()
        grads.append(xg.grad.clone())
    assert len(calls) == 2 and set(calls[0][1]) == set(calls[1][1]) == {"order"}
    total = int(calls[0][0][4][-1])
    for i, (p, q) in enumerate(zip(calls[0][0], calls[1][0])):
        assert torch.equal(p[:total], q[:total]) if i in (5, 6) else torch.equal(p, q), i      # (flag buffers: capacity beyond the total)
    r, A, L = _backward_reference(calls[0][0], c.n)
    n = (L + 3).double()
    bound = (n * U / (1.0 - n * U))[:, None] * A
    print(f"H={H}: gradients of the two routes bit-equal: {torch.equal(grads[0], grads[1])}")
    for g in grads:
        err = (g.cpu().double() - r).abs()
        print(f"  max |dx - fp64| = {err.max().item():.3e}, largest share of the bound used = {(err / bound.clamp(min=1e-300)).max().item():.3f}")
        assert bool((err <= bound).all())


def test_score_edges_serves_cn6(case3):
    from ocn_amd.pipeline import score_edges
    from ocn_amd.utils import PermIterator, adjoverlap, adjoverlap_3hop
    c = case3
    pred = _predictor(64, True).to(DEV)
    x = torch.randn(c.n, 64, generator=torch.Generator().manual_seed(4)).to(DEV)
    g = torch.Generator().manual_seed(8)
    edges = torch.randint(0, c.n, (3000, 2), generator=g).to(DEV)
    got = score_edges(pred, x, c.adj, c.adj2, edges, 1024, None)
    outs = []
    with torch.no_grad():
        for perm in PermIterator(edges.device, 3000, 1024, training=False):
            e = edges[perm].t().contiguous()
            outs.append(pred(x, c.adj, adjoverlap(c.adj, c.adj, e), adjoverlap(c.adj, c.adj2, e),
                             adjoverlap_3hop(c.adj, c.adj2, e), e, None).reshape(-1))
    assert [o.numel() for o in outs] == [1024, 1024, 952]
    assert got.shape == (3000,) and torch.equal(got, torch.cat(outs))
    with pytest.raises(ValueError):
        score_edges(pred, x, c.adj, c.adj2, edges, 1024, None, group=True)


def test_recommend_links_serves_cn6(case3):
    from ocn_amd.pipeline import score_edges
    from ocn_amd.recommend import _select, recommend_links, two_hop_candidates
    c = case3
    pred = _predictor(64, True).to(DEV)
    x = torch.randn(c.n, 64, generator=torch.Generator().manual_seed(5)).to(DEV)
    sources = torch.randperm(c.n, generator=torch.Generator().manual_seed(6))[:40].to(DEV)
    dst, score = recommend_links(pred, x, c.adj, c.adj2, sources, 10, 1024)
    ptr, edges = two_hop_candidates(c.adj, c.adj2, sources)
    want_dst, want_score = _select(score_edges(pred, x, c.adj, c.adj2, edges, 1024), ptr, edges, 10)
    assert dst.shape == (40, 10) and torch.equal(dst, want_dst) and torch.equal(score, want_score)
    with pytest.raises(ValueError):
        recommend_links(pred, x, c.adj, None, sources, 10, 1024)


def test_rows_on_demand_of_a_large_graph(hiplib):
    """Beyond ``ops.small_graph_cols()`` a product with rows on demand stays one: the cn3 pass builds and probes the bit rows of
    the batch's targets only.  (On the case3 graph above the (A, A, A²) pass needs the row lengths of A² and completes it.)"""
    from ocn_amd import ops
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.utils import CNState3, adjoverlap_3hop
    n = ops.small_graph_cols() + 900
    oadj = make_graph(n, 4, 40, 17)
    adj = to_product(oadj, DEV)
    adj2 = product_adj2(adj)
    lazy = SparseTensor._lazy_product(adj, adj)
    ed = batch(oadj, 500, 18).to(DEV)
    free, mat = CNState3(adj, lazy, None, ed), CNState3(adj, adj2, _adj3(adj, adj2), ed)
    assert lazy.rows_on_demand() and 0 < int(free.cnt3.sum())
    _same_states(free.b, mat.b, int(mat.a.off[-1]))
    assert torch.equal(free.a.flags[:int(mat.a.off[-1])], mat.a.flags[:int(mat.a.off[-1])])
    assert torch.equal(adjoverlap_3hop(adj, lazy, ed).counts(), mat.cnt3) and lazy.rows_on_demand()


# ---- 8. after an update: nothing beside (adj, adj2) has to be kept up to date ----------------------------------------
def test_after_insert_and_remove(hiplib):
    from ocn_amd.update import insert_edges, remove_edges
    from ocn_amd.utils import CNState3
    n = 300
    adj = random_graph(n, 0.02, seed=11)
    adj2 = product_adj2(adj)
    g = torch.Generator().manual_seed(12)
    new = torch.randint(0, n, (2, 40), generator=g).to(DEV)
    e = torch.randint(0, n, (2, 700), generator=g).to(DEV)
    adj_i, adj2_i = insert_edges(adj, new, adj2, donate=True)
    _same_as_reference(CNState3(adj_i, adj2_i, None, e).b, _reference(_dense(adj_i), e))
    adj_r, adj2_r = remove_edges(adj_i, new[:, :15].contiguous(), adj2_i, donate=True)
    A = _dense(adj_r)
    assert (A == A.T).all() and (A != _dense(adj)).any() and (A != _dense(adj_i)).any()
    _same_as_reference(CNState3(adj_r, adj2_r, None, e).b, _reference(A, e))


# ---- 9. capacity -------------------------------------------------------------------------------------------------------
def test_flag_buffer_one_byte_short(hiplib):
    from ocn_amd import ops
    n = 65
    adj = random_graph(n, 0.1, seed=65)
    adj2 = product_adj2(adj)
    e = torch.randint(0, n, (2, 200), generator=torch.Generator().manual_seed(9)).to(DEV)
    src, dst = e[0].contiguous(), e[1].contiguous()
    off = ops.edge_offsets(adj._rowptr, src)
    total = int(off[-1])
    last = int(off[-2])
    assert total - last > 0                                              # the last candidate's row does not fit
    room = torch.full((total + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    flags, hist, cnt3, status = ops.cn3_flags(adj._rowptr, adj._col, adj._rowptr, adj._col, adj2.product_bit_rows(), src, dst, n,
                                              off, None, adj.max_rowcount(), nds=adj.neighbor_degree_sum(), flags=room[:total - 1])
    assert status.cpu().tolist() == [ops.ST_CAP, 0, 0, ops.ST_CAP]
    assert bool((room[last:] == 0xAB).all())                             # nothing past the cap — nor of the row that does not fit
    ref = _reference(_dense(adj), e)
    assert room[:last].cpu().numpy().tolist() == ref[0][:last].tolist()   # the rows that fit are written
    assert cnt3.cpu().numpy().tolist() == ref[1].tolist()


# ---- a hub source: a row of many items, the run length adapted by nds ------------------------------------------------
def test_hub_source_spreads_over_items(hiplib):
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.utils import CNState3
    n = 600
    rng = np.random.default_rng(21)
    A = rng.random((n, n)) < 0.004
    A[580:] = False
    A[:, 580:] = False                                                   # the last twenty nodes stay isolated
    A[0, 10:580] = True                                                  # 570 neighbours: nine 64-neighbour chunks, at most 8 per item
    A = A | A.T
    np.fill_diagonal(A, False)
    r, c = np.nonzero(A)
    adj = SparseTensor.from_edge_index(torch.from_numpy(np.stack([r, c])).to(DEV), sparse_sizes=(n, n))
    adj2 = product_adj2(adj)
    g = torch.Generator().manual_seed(22)
    e = torch.randint(0, n, (2, 64), generator=g)
    e[0, ::4] = 0                                                        # the hub as a source ...
    e[1, 1::8] = 0                                                       # ... and as a target
    e[1, 2::8] = 599                                                     # an isolated target: no entry in a row of 570
    e = e.to(DEV)
    ref = _reference(A.astype(np.int64), e)
    assert 0 < ref[0].sum() < ref[0].size
    _same_as_reference(CNState3(adj, adj2, None, e).b, ref)
    for nds in (adj.neighbor_degree_sum(), None):
        flags, hist, cnt3, status, total = _raw(adj, adj2, e, None, nds)
        _same_as_reference(SimpleNamespace(flags=flags, hist=hist, cnt1=cnt3, status=status), ref)
