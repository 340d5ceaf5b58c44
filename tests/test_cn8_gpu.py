"""cn8 (CNLinkPredictorbaselearnablation, model.py:3233-3449) on the GPU against its restatement from the oracle's helpers:
xcn1 = spmm_add(cn1, x), xcn2 = spmm_add(cn2, x) on the raw ``adjoverlap`` / ``get_cn1_cn2`` matrices (:3340, :3395 — the
normalised copies are dropped, the diagonal is the identity), then the heads and the mix of cn7 (:3431-3445)."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

from oracle import ocn_oracle as O
from ocn_amd.synth import chung_lu_graph, sample_edges
from tests.helpers import close, make_graph, product_adj2, to_product

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (16, 32, 64, 128, 256, 512)


def cn8_pools(x, cn1, cn2):
    return O.spmm_add(cn1, x), O.spmm_add(cn2, x)


def cn8_ref(sd, x, cn1, cn2, e, ln=False, tailact=False, twolayerlin=False):
    xcn1, xcn2 = cn8_pools(x, cn1, cn2)
    return O._heads(sd, x, xcn1, xcn2, e, ln, tailact, twolayerlin)


def rowcount(m):
    return torch.bincount(m.row, minlength=m.n_rows)


@pytest.fixture(scope="module")
def hubs(hiplib):
    """A Chung-Lu graph with cliques plus: a hub with 1 400 neighbours (longer than the 1 024 entries from which cn5 / cn7's pooling
    hands a row to a workgroup), a bare path a - b - c (the candidate (a, c) has cn1 = {b} and no cn2 entry) and isolated nodes
    (candidates with neither).  Candidates: sampled edges and random pairs, plus pairs with the hub as source, as target, and
    the path's ends."""
    n, core, B = 3000, 2980, 1500
    g = torch.Generator().manual_seed(11)
    ei = chung_lu_graph(core, avg_deg=12, max_deg=300, seed=5, clique_frac=0.5)
    hub = 7
    spokes = torch.randperm(core, generator=g)[:1400]
    spokes = spokes[spokes != hub]
    a, b, c = core, core + 1, core + 2                                  # ids core + 3 .. n - 1 stay isolated
    extra = torch.tensor([[a, b], [b, c]])
    ei = torch.cat([ei, torch.stack([torch.full_like(spokes, hub), spokes]), extra], dim=1)
    oadj = O.to_symmetric(O.from_edge_index(ei, n))
    oadj2 = O.adj2_sparse(oadj)
    e = sample_edges(oadj.row, oadj.col, n, B - 40, seed=13, pos_frac=0.6)
    other = torch.randint(0, core, (16,), generator=g)
    special = torch.cat([torch.stack([torch.full_like(other, hub), other]), torch.stack([other, torch.full_like(other, hub)]),
                         torch.tensor([[a, c, a, n - 1, n - 2, hub, b, 3], [c, a, b, 5, n - 1, n - 1, b, 3]])], dim=1)
    e = torch.cat([e, special], dim=1)
    e = e[:, torch.randperm(e.shape[1], generator=g)].contiguous()
    adj = to_product(oadj, DEV)
    adj2 = product_adj2(adj)
    ocn1, ocn2 = O.adjoverlap(oadj, oadj, e), O.adjoverlap(oadj, oadj2, e)
    return SimpleNamespace(n=n, B=e.shape[1], oadj=oadj, oadj2=oadj2, e=e, adj=adj, adj2=adj2, ocn1=ocn1, ocn2=ocn2, hub=hub)


@pytest.fixture(scope="module")
def mid(hiplib):
    """The shape the suite's score tests use (rows up to 400 entries, isolated nodes)."""
    n, B = 3000, 2048
    oadj = make_graph(n, 12, 400, 2, isolated=20)
    oadj2 = O.adj2_sparse(oadj)
    e = sample_edges(oadj.row, oadj.col, n, B, seed=52)
    adj = to_product(oadj, DEV)
    return SimpleNamespace(n=n, B=B, oadj=oadj, oadj2=oadj2, e=e, adj=adj, adj2=product_adj2(adj))


def assert_not_empty(ocn1, ocn2, B, every_class=False):
    """From the ORACLE's counts: no test here passes on empty sets.  At least a quarter of the candidates have cn1 entries, at
    least half have cn2 entries, at least one has neither; ``every_class``: all four combinations occur."""
    c1, c2 = rowcount(ocn1), rowcount(ocn2)
    assert int((c1 > 0).sum()) * 4 >= B and int((c2 > 0).sum()) * 2 >= B and bool(((c1 == 0) & (c2 == 0)).any())
    if every_class:
        for has1 in (False, True):
            for has2 in (False, True):
                assert bool((((c1 > 0) == has1) & ((c2 > 0) == has2)).any()), (has1, has2)
    return c1, c2


@pytest.mark.parametrize("order", [False, True], ids=["batch_order", "permuted"])
@pytest.mark.parametrize("form", ["bits", "csr", "bits1_csr2"])
@pytest.mark.parametrize("H", WIDTHS)
def test_cn8_pool_bit_equal_to_spmm_add(hubs, H, form, order):
    """``ocn_cn8_pool``: both pools bit-equal to the oracle's sequential ``spmm_add`` over the raw matrices, xij to the product,
    the counts to the oracle's row counts — hub rows, isolated nodes, every class of candidate, T1 / T2 as bit rows and as CSR,
    with and without a processing order."""
    from ocn_amd import ops
    c = hubs
    c1, c2 = assert_not_empty(c.ocn1, c.ocn2, c.B, every_class=True)
    deg = rowcount(c.oadj)
    assert int(deg[c.hub]) > 1024 and int((deg == 0).sum()) >= 10 and int((c.e[0] == c.hub).sum()) >= 16
    torch.manual_seed(100 + H)
    x = torch.randn(c.n, H)
    r1, r2 = cn8_pools(x, c.ocn1, c.ocn2)
    adj, adj2 = c.adj, c.adj2
    bm1 = ops.bitrows_from_csr(adj._rowptr, adj._col, c.n) if form != "csr" else None
    bm2 = ops.bitrows_from_csr(adj2._rowptr, adj2._col, c.n) if form == "bits" else None
    t1 = (adj._rowptr, adj._col) if form != "bits" else None
    t2 = (adj2._rowptr, adj2._col) if form != "bits" else None
    ed = c.e.to(DEV)
    perm = torch.randperm(c.B, generator=torch.Generator().manual_seed(3)).to(DEV) if order else None
    x1, x2, xij, n1, n2 = ops.cn8_pool(adj._rowptr, adj._col, t1, t2, ed[0].contiguous(), ed[1].contiguous(), x.to(DEV),
                                       t1_bitmap=bm1, t2_bitmap=bm2, order=perm)
    assert n1.dtype == torch.int32 and torch.equal(n1.cpu().long(), c1) and torch.equal(n2.cpu().long(), c2)
    assert torch.equal(x1.cpu(), r1) and torch.equal(x2.cpu(), r2)
    assert torch.equal(xij.cpu(), x[c.e[0]] * x[c.e[1]])
    none = (c1 == 0) & (c2 == 0)
    assert not bool(x1.cpu()[none].any()) and not bool(x2.cpu()[none].any())


@pytest.mark.parametrize("H", [16, 256, 512])
def test_cn8_pool_complete_bipartite_by_hand(hiplib, H):
    """K_{a,b} needs no oracle.  Two nodes of one side share the whole other side as neighbours and none of them is adjacent to
    either: cn1 = the other side (all of it).  A cross pair has no common neighbour.  A² links every node to its own side, the
    node itself included: N(i) ∩ A²(j) is empty for a same-side pair and the whole of j's side for a cross pair.  With integer
    embeddings every sum is exact."""
    from ocn_amd import ops
    from ocn_amd.sparse import SparseTensor
    a, b = 70, 9                                                       # (70 > 64: the left side's rows span two rounds of a wave)
    n = a + b + 2                                                      # ... and two isolated nodes
    left, right = torch.arange(a), torch.arange(a, a + b)
    ei = torch.stack([left.repeat_interleave(b), right.repeat(a)])
    ei = torch.cat([ei, ei.flip(0)], dim=1)
    adj = SparseTensor.from_edge_index(ei.to(DEV), sparse_sizes=(n, n))
    adj2 = product_adj2(adj)
    x = torch.randint(-8, 9, (n, H), generator=torch.Generator().manual_seed(H)).float()
    pairs = torch.tensor([[0, 3, a, a + 2, 0, a + 1, 5, n - 1, 2], [1, 3, a + 1, a + 8, a, 4, n - 1, n - 2, a + b - 1]])
    sumL, sumR = x[left].sum(0), x[right].sum(0)
    z = torch.zeros(H)
    #            L-L       L-L (i = j)  R-R      R-R      L-R     R-L     L-iso  iso-iso  L-R
    want1 = [sumR, sumR, sumL, sumL, z, z, z, z, z]
    want2 = [z, z, z, z, sumR, sumL, z, z, sumR]
    cnt1 = [b, b, a, a, 0, 0, 0, 0, 0]
    cnt2 = [0, 0, 0, 0, b, a, 0, 0, b]
    e = pairs.to(DEV)
    for bits in (False, True):
        bm1 = ops.bitrows_from_csr(adj._rowptr, adj._col, n) if bits else None
        bm2 = ops.bitrows_from_csr(adj2._rowptr, adj2._col, n) if bits else None
        x1, x2, xij, n1, n2 = ops.cn8_pool(adj._rowptr, adj._col, (adj._rowptr, adj._col), (adj2._rowptr, adj2._col),
                                           e[0].contiguous(), e[1].contiguous(), x.to(DEV), t1_bitmap=bm1, t2_bitmap=bm2)
        assert n1.tolist() == cnt1 and n2.tolist() == cnt2
        assert torch.equal(x1.cpu(), torch.stack(want1)) and torch.equal(x2.cpu(), torch.stack(want2))
        assert torch.equal(xij.cpu(), x[pairs[0]] * x[pairs[1]])


SCORE_CASES = [  # H, ln, tailact, twolayerlin, route
    (32, False, False, False, "pattern"), (64, True, False, False, "pattern"), (256, True, False, False, "pattern"),
    (256, False, False, False, "pattern"), (64, True, True, False, "pattern"), (64, True, False, True, "pattern"),
    (32, True, True, True, "pattern"), (64, True, False, False, "walk"), (32, False, False, False, "walk"),
    (256, True, True, False, "walk"),
]


@pytest.mark.parametrize("H,ln,tailact,two,route", SCORE_CASES)
def test_cn8_scores(mid, monkeypatch, H, ln, tailact, two, route):
    """Scores against the restatement within the suite's bar: the one-pass eval path, the unit-weight route (flags -> pooling
    with {1, 0, 1, 0}), explicit [B, N] matrices, and the walk route with its valued cn2."""
    from ocn_amd import ops
    from ocn_amd.model import predictor_dict
    from ocn_amd.utils import adjoverlap, get_cn1_cn2
    c = mid
    torch.manual_seed(7 + H)
    x = torch.randn(c.n, H)
    pred = predictor_dict["cn8"](H, H, 1, 3, 0.0, 0.0, ln, tailact=tailact, twolayerlin=two, beta=0.8).eval()
    with torch.no_grad():
        pred.alpha.copy_(torch.tensor([0.4, -0.3, 0.1]))
    sd = {k: v.detach().clone() for k, v in pred.state_dict().items()}
    if route == "walk":
        ocn1, ocn2 = O.get_cn1_cn2(c.oadj, c.e)
        assert bool((ocn2.val > 1).any())                              # valued: 2-walk counts
    else:
        ocn1, ocn2 = O.adjoverlap(c.oadj, c.oadj, c.e), O.adjoverlap(c.oadj, c.oadj2, c.e)
    assert_not_empty(ocn1, ocn2, c.B)
    ref = cn8_ref(sd, x, ocn1, ocn2, c.e, ln, tailact, two)
    pred = pred.to(DEV)
    e, xd = c.e.to(DEV), x.to(DEV)
    args = SimpleNamespace(sum=2.74)

    def handles():
        return get_cn1_cn2(c.adj, e) if route == "walk" else (adjoverlap(c.adj, c.adj, e), adjoverlap(c.adj, c.adj2, e))
    with torch.no_grad():
        monkeypatch.setattr(ops, "cn8_fused_eval", True)                # (pattern handles: ocn_cn8_pool; walk handles: the flag pass)
        out = pred(xd, c.adj, *handles(), e, args)
        print(f"cn8 scores {route} H={H}: max|out - ref| = {(out.cpu() - ref).abs().max().item():.3e}, max|ref| = {ref.abs().max().item():.3e}")
        assert out.shape == (c.B, 1) and close(out, ref)
        monkeypatch.setattr(ops, "cn8_fused_eval", False)
        unit = pred(xd, c.adj, *handles(), e, args)
        assert close(unit, ref)
        h1, h2 = handles()
        mat = pred(xd, c.adj, h1.materialize(), h2.materialize(), e, args)
        assert close(mat, ref)
        tok = pred.begin(xd, c.adj, *handles(), e, slot=1, args=args)
        assert torch.equal(pred.finish(xd, tok, args), pred(xd, c.adj, *handles(), e, args))
        monkeypatch.setattr(ops, "cn8_fused_eval", True)
        tok = pred.begin(xd, c.adj, *handles(), e, slot=2, args=None)
        assert torch.equal(pred.finish(xd, tok, None), out)
    pred.check_errors()


@pytest.mark.parametrize("fused", [False, True], ids=["unit_weights", "one_pass"])
def test_cn8_is_independent_of_the_batch(mid, monkeypatch, fused):
    """``score_edges`` over one split at two batch sizes: the pooled vectors are bit-equal (nothing of a candidate depends on the
    rest of its batch), the scores agree within the suite's bar; ``args.sum`` changes no bit; a sharded predictor performs no
    collective (no process group exists here); a captured loop replays the same bits; ``innerprod`` and ``n`` stay untouched
    by training-mode calls."""
    from ocn_amd import ops
    from ocn_amd.model import predictor_dict
    from ocn_amd.pipeline import score_edges
    from ocn_amd.utils import adjoverlap
    c = mid
    H = 64
    torch.manual_seed(3)
    x = torch.randn(c.n, H, device=DEV)
    pred = predictor_dict["cn8"](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()
    edges = c.e.t().contiguous().to(DEV)
    seen = []
    heads = pred._heads

    def spy(x_, xcn1, xcn2, xij, cls=None):
        seen.append((xcn1.clone(), xcn2.clone(), xij.clone()))
        return heads(x_, xcn1, xcn2, xij, cls)
    monkeypatch.setattr(pred, "_heads", spy)
    monkeypatch.setattr(ops, "overlap_min_batch", 0)
    monkeypatch.setattr(ops, "cn8_fused_eval", fused)
    runs = {}
    for bs in (c.B, 300):
        seen.clear()
        s = score_edges(pred, x, c.adj, c.adj2, edges, bs, SimpleNamespace(sum=1.0))
        torch.cuda.synchronize()
        runs[bs] = (s, [torch.cat([t[q] for t in seen]) for q in range(3)])
    assert len(runs[300][1][0]) == c.B
    for q in range(3):
        assert torch.equal(runs[c.B][1][q], runs[300][1][q])
    ocn1, ocn2 = O.adjoverlap(c.oadj, c.oadj, c.e), O.adjoverlap(c.oadj, c.oadj2, c.e)
    r1, r2 = cn8_pools(x.cpu(), ocn1, ocn2)
    assert torch.equal(runs[300][1][0].cpu(), r1) and torch.equal(runs[300][1][1].cpu(), r2)
    assert close(runs[c.B][0], runs[300][0])
    other = score_edges(pred, x, c.adj, c.adj2, edges, 300, SimpleNamespace(sum=-37.5))
    assert torch.equal(other, runs[300][0])
    pred.set_edge_sharding(None, True)                                 # no process group: any collective would raise
    assert torch.equal(score_edges(pred, x, c.adj, c.adj2, edges, 300, SimpleNamespace(sum=1.0)), runs[300][0])
    pred.set_edge_sharding(None, False)
    monkeypatch.setattr(pred, "_heads", heads)
    monkeypatch.setattr(ops, "graph_loops", True)                      # captured phases: 70 batches over the loop's scratch sets
    small = score_edges(pred, x, c.adj, c.adj2, edges, 30, SimpleNamespace(sum=1.0))
    monkeypatch.setattr(ops, "graph_loops", False)
    assert torch.equal(small, score_edges(pred, x, c.adj, c.adj2, edges, 30, SimpleNamespace(sum=1.0)))
    assert close(small, runs[300][0])
    # training-mode calls leave the cn5 running mean alone
    monkeypatch.undo()
    pred.train()
    e = c.e.to(DEV)[:, :256].contiguous()
    for _ in range(2):
        pred.multidomainforward(x, c.adj, adjoverlap(c.adj, c.adj, e), adjoverlap(c.adj, c.adj2, e), e, SimpleNamespace(sum=1.0))
    assert pred.n == 0 and pred.innerprod.tolist() == [0.0]


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("route", ["pattern", "walk"])
def test_cn8_backward_matches_oracle_autograd(mid, hubs, mode, route):
    """Gradients with respect to the embeddings and every used parameter against torch autograd through the restatement, in
    eval mode and in training mode with dropout 0; the unused heads get none.  On the pattern route the pools of the
    unit-weight path (what autograd runs) equal the one-pass eval pools bit for bit, hub rows included."""
    from ocn_amd import ops
    from ocn_amd.model import predictor_dict
    from ocn_amd.utils import adjoverlap, fuse, fuse8, get_cn1_cn2
    c = mid
    H = 32
    torch.manual_seed(23)
    x = torch.randn(c.n, H)
    pred = predictor_dict["cn8"](H, H, 1, 3, 0.0, 0.0, True)
    pred.train(mode == "train")
    with torch.no_grad():
        pred.alpha.copy_(torch.tensor([0.3, -0.2, 0.9]))
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point() and k != "innerprod") for k, v in pred.state_dict().items()}
    xr = x.clone().requires_grad_(True)
    ocn = O.get_cn1_cn2(c.oadj, c.e) if route == "walk" else (O.adjoverlap(c.oadj, c.oadj, c.e), O.adjoverlap(c.oadj, c.oadj2, c.e))
    assert_not_empty(*ocn, c.B)
    ref = cn8_ref(sd, xr, *ocn, c.e, True)
    wgt = torch.randn(c.B, 1, generator=torch.Generator().manual_seed(1))
    (ref * wgt).sum().backward()
    pred = pred.to(DEV)
    ed = c.e.to(DEV)
    xd = x.to(DEV).requires_grad_(True)

    def handles():
        return get_cn1_cn2(c.adj, ed) if route == "walk" else (adjoverlap(c.adj, c.adj, ed), adjoverlap(c.adj, c.adj2, ed))
    out = pred.multidomainforward(xd, c.adj, *handles(), ed, SimpleNamespace(sum=0.5))
    err = (out.detach().cpu() - ref.detach()).abs().max().item()
    print(f"cn8 autograd {mode} {route}: max|out - ref| = {err:.3e}, max|ref| = {ref.abs().max().item():.3e}")
    assert out.requires_grad and close(out, ref)
    (out * wgt.to(DEV)).sum().backward()
    scale = xr.grad.abs().max().item()
    gerr = (xd.grad.cpu() - xr.grad).abs().max().item()
    print(f"cn8 autograd {mode} {route}: max|dx - ref| = {gerr:.3e}, |g|max = {scale:.3e}")
    assert gerr <= 2e-5 * max(1.0, scale)
    seen = 0
    for k, p in pred.named_parameters():
        if sd[k].grad is None:
            assert p.grad is None or p.grad.abs().max().item() == 0.0, k
            continue
        g = sd[k].grad
        seen += 1
        perr = (p.grad.cpu() - g).abs().max().item()
        assert perr <= 2e-5 * max(1.0, g.abs().max().item()), (k, perr, g.abs().max().item())
    assert seen >= 20
    for k, p in pred.named_parameters():
        if k.startswith(("xcnlin", "xcn4lin")):
            assert p.grad is None, k
    assert pred.n == 0 and pred.innerprod.tolist() == [0.0]
    if route == "pattern":
        for g in (mid, hubs):                                          # (hubs: a source row longer than 1 024 entries)
            with torch.no_grad():
                xe = torch.randn(g.n, H, generator=torch.Generator().manual_seed(5)).to(DEV)
                eg = g.e.to(DEV)
                h8 = lambda: (adjoverlap(g.adj, g.adj, eg), adjoverlap(g.adj, g.adj2, eg))
                fused = fuse8(*h8(), eg).pool(xe)
                unit = fuse(*h8(), eg, adj=g.adj).gather(ops.unit_weights(g.n, DEV), xe)
                r1, r2 = cn8_pools(xe.cpu(), O.adjoverlap(g.oadj, g.oadj, g.e), O.adjoverlap(g.oadj, g.oadj2, g.e))
                assert torch.equal(unit[0].cpu(), r1) and torch.equal(unit[1].cpu(), r2)
                for a, b in zip(fused, unit):
                    assert torch.equal(a, b)


def test_cn8_example_driver_runs_one_epoch(hiplib):
    """examples/run_like_reference.py --predictor cn8 on the Cora shape, with the head flags the reference driver forwards for
    cn8 (NeighborOverlap_large.py:275-276): a finite loss and the three Hits@K."""
    import importlib.util
    import math
    spec = importlib.util.spec_from_file_location("run_like_reference", os.path.join(ROOT, "examples", "run_like_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--dataset", "cora", "--predictor", "cn8", "--epochs", "1", "--use_xlin", "--tailact", "--beta", "0.5"])
    assert len(out) == 1
    loss, results = out[0]
    assert math.isfinite(loss) and set(results) == {"Hits@20", "Hits@50", "Hits@100"}
    assert all(len(v) == 3 and all(0.0 <= h <= 1.0 for h in v) for v in results.values())
