"""The certificate on the second operand of a candidate batch (``SparseTensor.covers``): which T2 the intersection pass is
told to be the complete A·A of a symmetric A (``ops.cn_flags`` ``t2_certified`` -> ``ocn_cn_flags_cover``), which it is not,
and that the scores do not depend on it (``ops.t2_cover`` on and off, bit for bit)."""
from types import SimpleNamespace

import pytest
import torch

from tests.helpers import batch, make_graph, product_adj2, to_product

DEV = torch.device("cuda:0")
gpu = pytest.mark.gpu


def test_symmetry_is_established_not_assumed():
    """No device needed: the pattern is compared with its transpose once, the answer cached; a matrix from arrays is nobody's
    certified product."""
    from ocn_amd.sparse import SparseTensor
    r = torch.tensor([0, 1, 1, 2, 2, 3])
    c = torch.tensor([1, 0, 2, 1, 3, 2])
    a = SparseTensor(row=r, col=c, sparse_sizes=(4, 4))
    assert a._symmetric is None and a.is_symmetric() and a._symmetric is True
    b = SparseTensor(row=r[:-1], col=c[:-1], sparse_sizes=(4, 4))           # (3, 2) gone, its mirror (2, 3) left
    assert not b.is_symmetric() and b._symmetric is False
    assert not SparseTensor(row=r, col=c, sparse_sizes=(4, 5)).is_symmetric()
    assert a.to_symmetric()._symmetric is True
    assert not a.covers(a) and not SparseTensor(rowptr=a._rowptr, col=a._col, sparse_sizes=(4, 4)).covers(a)


def _small():
    oadj = make_graph(3000, 14, 300, seed=21)
    return oadj, to_product(oadj, DEV)


@gpu
def test_which_products_are_certified(hiplib):
    from ocn_amd import ops
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.utils import sparse_tensor_multiply
    oadj, adj = _small()
    assert adj._symmetric is None                                          # from an edge list: nothing known yet
    adj2 = product_adj2(adj)
    assert adj2.covers(adj) and adj._symmetric is True                     # A @ A of a symmetric A (compared once)
    sym = adj.to_symmetric()
    assert sym._symmetric is True and product_adj2(sym).covers(sym) and not product_adj2(sym).covers(adj)     # that very object
    assert sparse_tensor_multiply(adj, 1024).covers(adj)                   # the block route
    # one entry whose mirror is missing
    ei = torch.stack([oadj.row, oadj.col])
    lop = SparseTensor.from_edge_index(ei[:, 1:].to(DEV), sparse_sizes=(3000, 3000))
    assert not product_adj2(lop).covers(lop) and lop._symmetric is False
    # built from arrays, or from a real torch sparse tensor
    assert not SparseTensor(rowptr=adj2._rowptr, col=adj2._col, sparse_sizes=(3000, 3000)).covers(adj)
    r2, c2, _ = adj2.coo()
    real = torch.sparse_coo_tensor(torch.stack([r2, c2]), torch.ones(r2.numel(), device=DEV), (3000, 3000))
    assert not SparseTensor.from_torch_sparse_coo_tensor(real, False).covers(adj)
    # a product of two different objects, and A³
    sp, sp2 = adj.to_torch_sparse_coo_tensor(), adj2.to_torch_sparse_coo_tensor()
    assert not SparseTensor.from_torch_sparse_coo_tensor(sp @ sym.to_torch_sparse_coo_tensor(), False).covers(adj)
    assert not SparseTensor.from_torch_sparse_coo_tensor(sp2 @ sp, False).covers(adj)
    # rows on demand (a large graph's product formed while autograd records): not certified, completed or not
    big = to_product(make_graph(20000, 10, 300, seed=8), DEV)
    assert ops.lazy_product_rows and torch.is_grad_enabled()
    lazy = product_adj2(big)
    assert lazy.rows_on_demand() and not lazy.covers(big)
    lazy.complete()
    assert not lazy.covers(big)
    with torch.no_grad():
        assert product_adj2(big).covers(big)


@gpu
def test_updates_drop_the_certificate(hiplib):
    from ocn_amd.update import insert_edges, remove_edges
    oadj, adj = _small()
    new = torch.tensor([[5, 17, 2999], [1200, 2100, 3]], device=DEV)
    for donate in (False, True):
        adj2 = product_adj2(adj)
        adj_i, adj2_i = insert_edges(adj, new, adj2, donate=donate)
        assert not adj2_i.covers(adj_i) and not adj2_i.covers(adj)
        assert adj2.covers(adj) == (not donate)                            # a donated product is nobody's any more
        adj_r, adj2_r = remove_edges(adj_i, new, adj2_i, donate=donate)
        assert not adj2_r.covers(adj_r) and not adj2_r.covers(adj_i)
    again = product_adj2(adj_i)                                            # re-established by the same rule only
    assert again.covers(adj_i) and adj_i._symmetric is True
    one_way, _ = insert_edges(adj, new, None, undirected=False)
    assert not product_adj2(one_way).covers(one_way)


@gpu
def test_the_walk_route_never_asks(hiplib, monkeypatch):
    from ocn_amd import ops
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.utils import CNState
    seen, orig = [], ops.cn_flags

    def spy(*a, **k):
        seen.append(bool(k.get("t2_certified")))
        return orig(*a, **k)

    def refuse(*a, **k):
        raise AssertionError("the walk route asked for the certificate")
    oadj, adj = _small()
    e = batch(oadj, 300, 2).to(DEV)
    monkeypatch.setattr(SparseTensor, "covers", refuse)
    monkeypatch.setattr(SparseTensor, "is_symmetric", refuse)
    monkeypatch.setattr(ops, "cn_flags", spy)
    st = CNState(adj, None, None, e, walk=True)
    torch.cuda.synchronize()
    assert seen == [False] and int(st.cnt1.sum()) > 0


@gpu
@pytest.mark.parametrize("loop", ["streams", "graphs"])
@pytest.mark.parametrize("kind", ["cn5", "cn5_trained", "cn7"])
def test_scores_do_not_depend_on_the_certificate(hiplib, monkeypatch, kind, loop):
    """Batches of 1 .. 128 candidates (half of them stored entries, ``synth.sample_edges``) through the four-stream loop and
    through GraphedPhases (batches of another size than its 128 run launch by launch; 24 more batches of 128 are replayed
    graphs): ``ops.t2_cover`` on — every batch handed over as certified — and off, bit for bit."""
    from ocn_amd import ops, pipeline
    from ocn_amd.model import predictor_dict
    from ocn_amd.utils import adjoverlap
    H, top = 64, 128
    oadj, adj = _small()
    adj2 = product_adj2(adj)
    adj.warm()                                                             # (bit rows, longest row, symmetry: before the loop forks)
    assert adj._symmetric is True and adj2.covers(adj)
    torch.manual_seed(3)
    x = torch.randn(3000, H, device=DEV)
    pred = predictor_dict["cn7" if kind == "cn7" else "cn5"](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()
    if kind == "cn5_trained":
        with torch.no_grad():
            pred.innerprod.fill_(0.37)
    args = SimpleNamespace(sum=0.5)
    sizes = list(range(1, top + 1)) + ([top] * 24 if loop == "graphs" else [])
    batches = [batch(oadj, B, 500 + q).to(DEV) for q, B in enumerate(sizes)]
    handles = lambda e: (adjoverlap(adj, adj, e), adjoverlap(adj, adj2, e))
    seen = []
    orig = ops.cn_flags

    def spy(*a, **k):
        seen.append(bool(k.get("t2_certified")))
        return orig(*a, **k)
    monkeypatch.setattr(ops, "cn_flags", spy)
    monkeypatch.setattr(ops, "overlap_depth_small", 4)                      # four batches in flight: three side streams and the caller's

    def run():
        made = []
        if loop == "graphs":
            gp = pipeline.GraphedPhases(pred, x, adj, handles, top, args)
            begin = lambda it: gp.begin(it, batches[it])

            def finish(tok):
                made.append(tok[0])
                return gp.finish(tok)
        else:
            begin = lambda it: pred.begin(x, adj, *handles(batches[it]), batches[it], slot=it, args=args)
            finish = lambda tok: pred.finish(x, tok, args)
        every = torch.cat(batches, dim=1)
        # (as the scoring loops do: ids checked once for the split — a captured batch cannot read its check back)
        with torch.no_grad(), ops.prevalidated(every[0], every[1], 3000, 3000):
            outs = [o.clone() for o in pipeline.overlapped_steps(begin, finish, len(batches), overlap=True, batch=top)]
        torch.cuda.synchronize()
        assert loop != "graphs" or made.count("graph") >= 8
        return outs
    monkeypatch.setattr(ops, "t2_cover", True)
    on = run()
    assert seen and all(seen)
    del seen[:]
    monkeypatch.setattr(ops, "t2_cover", False)
    off = run()
    assert seen and not any(seen)
    assert [o.shape[0] for o in on] == sizes
    for a, b in zip(on, off):
        assert torch.equal(a, b)
