"""Explaining a link on the GPU: ``ocn_cn_attribution`` against fp64 at every width and on both routes, against a known answer
that needs no reference, its bits fixed by its input, its sums against the pooling; ``explain_links`` end to end (scores,
gradients, the exact top-m, the counterfactual) and the example driver's flag."""
import copy
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from tests.helpers import make_graph, product_adj2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (16, 32, 64, 128, 256, 512)
U = 2.0 ** -24
NINF = float("-inf")
B = 257                                                                  # no multiple of the candidates per wave at any width


def bits(t):
    """int32 view of an fp32 tensor on the host: compared this way the signs of zeros count."""
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def graph(hiplib):
    """A Chung-Lu graph of 1 298 nodes and two isolated ones, plus a hub joined to 1 100 others: its row is longer than 1 024 and
    takes several rounds of a lane group at every width; and a bare path a - k - b of three more nodes.  257 candidates, among
    them the hub as a source twice (different targets), an isolated source, a pair without a common neighbour, a repeated pair
    and (a, b), whose one common neighbour k is a column no other candidate touches."""
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.synth import sample_edges
    o = make_graph(n=1300, avg_deg=8, max_deg=100, seed=23, isolated=2)
    n, hub, iso = 1304, 1300, 1299
    pa, pk, pb = 1301, 1302, 1303
    g = torch.Generator().manual_seed(5)
    spokes = torch.randperm(1298, generator=g)[:1100]
    ei = torch.cat([torch.stack([o.row, o.col]), torch.stack([torch.full_like(spokes, hub), spokes]),
                    torch.stack([spokes, torch.full_like(spokes, hub)]), torch.tensor([[pa, pk, pk, pb], [pk, pa, pb, pk]])], dim=1)
    adj = SparseTensor.from_edge_index(ei.to(DEV), sparse_sizes=(n, n))
    adj2 = product_adj2(adj)
    deg = torch.bincount(ei[0], minlength=n)
    assert int(deg[hub]) == 1100 > 1024 and int(deg[iso]) == 0 and int(deg[iso - 1]) == 0
    spoke = torch.zeros(n, dtype=torch.bool)
    spoke[spokes] = True
    lone = int(torch.nonzero((deg > 0) & ~spoke & (torch.arange(n) < 1298))[0])     # has neighbours, none of them is the hub
    e = sample_edges(o.row, o.col, 1298, B - 7, seed=7, pos_frac=0.6)
    special = torch.tensor([[hub, hub, iso, lone, int(e[0, 0]), 3, pa], [int(spokes[0]), int(spokes[1]), 5, iso, int(e[1, 0]), hub, pb]])
    #                        hub source twice     isolated source   no CN   a repeat   hub as the target   the bare path
    e = torch.cat([e, special], dim=1)
    e = e[:, torch.randperm(B, generator=g)].contiguous()
    assert e.shape == (2, B)
    return SimpleNamespace(n=n, hub=hub, iso=iso, lone=lone, path=(pa, pk, pb), adj=adj, adj2=adj2, e=e.to(DEV), e_cpu=e,
                           rowptr=adj._rowptr.cpu(), col=adj._col.cpu().long())


def random_table(n, seed):
    """Normal fp32 [n, 4] = {w1, t, inv2, 0}: t and inv2 matter; w1 = 0 on about a fifth of the columns and inv2 = 0 on about a
    fifth (independently), so that some members are fetched for one side only and some not at all."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, 4, generator=g)
    w[torch.rand(n, generator=g) < 0.2, 0] = 0.0
    w[torch.rand(n, generator=g) < 0.2, 2] = 0.0
    w[:, 3] = 0.0
    return w


def operands(n, H, seed):
    """Random h, g1, g2 with g scaled by 1e-3, 1 and 30 across three thirds of the batch."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(n, H, generator=g)
    scale = torch.tensor([1e-3, 1.0, 30.0]).repeat_interleave((B + 2) // 3)[:B, None]
    return h, torch.randn(B, H, generator=g) * scale, torch.randn(B, H, generator=g) * scale


def flat_reference(c, src, off, flags, wc, w, h, g1, g2):
    """Everything about the flagged positions of a batch, on the host: the candidate ``e`` and column ``k`` of every position
    below off[B], the flag byte, (wa, wb) restated in fp32 exactly as ``entry_weights`` forms them (difference and product
    rounded separately), the two dot products in fp64 and the sums of the absolute products."""
    off, src = off.cpu(), src.cpu()
    total = int(off[-1])
    lens = off[1:] - off[:-1]
    assert torch.equal(lens, c.rowptr[src + 1] - c.rowptr[src])
    e = torch.repeat_interleave(torch.arange(src.numel()), lens)
    p = torch.arange(total) - off[e]
    k = c.col[c.rowptr[src[e]] + p]
    f = flags.cpu()[:total].long()
    cv = wc.cpu()[:total].float() if wc is not None else torch.ones(total)
    w = w.cpu().float()
    is1, is2 = (f & 1) != 0, (f & 2) != 0
    zero = torch.zeros(())
    wa = torch.where(is1, w[k, 0], zero)
    wb = (torch.where(is2, cv, zero) - torch.where(is1, w[k, 1], zero)) * w[k, 2]
    hk = h.cpu().double()[k]
    pr1, pr2 = hk * g1.cpu().double()[e], hk * g2.cpu().double()[e]
    return SimpleNamespace(total=total, e=e, k=k, f=f, c=cv, wa=wa, wb=wb, member=f != 0, d1=pr1.sum(1), d2=pr2.sum(1),
                           ad1=pr1.abs().sum(1), ad2=pr2.abs().sum(1), off=off)


def attribute(c, st, w, h, g1, g2, order=None, sentinel=None):
    """``ops.cn_attribution`` on a batch state; with ``sentinel`` the outputs are pre-filled scratch."""
    from ocn_amd import ops
    ws = None
    if sentinel is not None:
        ws = {}
        cap = st.flags.numel()
        ops.buf(ws, "attr", (cap, 2), torch.float32, DEV).fill_(sentinel)
        ops.buf(ws, "attr_rank", cap, torch.float32, DEV).fill_(sentinel)
    return ops.cn_attribution(c.adj._rowptr, c.adj._col, st.src, st.off, st.flags, st.wc, w, h, g1, g2, order=order, wsd=ws)


def check_against_fp64(ref, attr, rank, H, sentinel):
    attr, rank = attr.cpu(), rank.cpu()
    t, mem = ref.total, ref.member
    a = attr[:t].double()
    for q, (wgt, d, ad) in enumerate(((ref.wa, ref.d1, ref.ad1), (ref.wb, ref.d2, ref.ad2))):
        live = mem & (wgt != 0)
        err = (a[:, q] - wgt.double() * d).abs()
        bound = (H + 2) * U * wgt.double().abs() * ad + 1e-37
        worst = (err[live] / bound[live]).max().item() if bool(live.any()) else 0.0
        print(f"attribution H={H} side {q + 1}: {int(live.sum())} live members, worst error / bound = {worst:.3f}")
        assert bool(live.any()) and bool((err[live] <= bound[live]).all())
        assert bool((bits(attr[:t, q])[~live] == 0).all())              # +0 exactly: non-members and zero weights
    none = mem & (ref.wa == 0) & (ref.wb == 0)
    assert bool(none.any()) and bool((~mem).any())
    assert bool((bits(rank[:t])[none] == 0).all())                      # rank +0 where nothing is fetched
    assert bool((rank[:t][~mem] == NINF).all()) and bool((bits(attr[:t])[~mem] == 0).all())
    assert torch.equal(bits(rank[:t][mem]), bits((attr[:t, 0] + attr[:t, 1])[mem]))
    assert attr.shape[0] > t                                            # (the cap exceeds the total: B x the longest row)
    assert bool((attr[t:] == sentinel).all()) and bool((rank[t:] == sentinel).all())


@pytest.mark.parametrize("H", WIDTHS)
def test_attribution_against_fp64_every_width(graph, H):
    from ocn_amd.utils import CNState
    c = graph
    st = CNState(c.adj, c.adj, c.adj2, c.e)
    w = random_table(c.n, 3).to(DEV)
    h, g1, g2 = (t.to(DEV) for t in operands(c.n, H, 10 + H))
    attr, rank = attribute(c, st, w, h, g1, g2, sentinel=12345.0)
    st.check_status()
    ref = flat_reference(c, st.src, st.off, st.flags, None, w, h, g1, g2)
    assert st.wc is None and int(ref.member.sum()) > 2000
    hub_rows = torch.nonzero(c.e_cpu[0] == c.hub).flatten()
    assert hub_rows.numel() == 2 and all(int(ref.member[ref.e == r].sum()) > 0 for r in hub_rows.tolist())
    check_against_fp64(ref, attr, rank, H, 12345.0)


@pytest.mark.parametrize("H", [32, 64])
def test_attribution_walk_route(graph, H):
    from ocn_amd.utils import CNState
    c = graph
    st = CNState(c.adj, None, None, c.e, walk=True)
    w = random_table(c.n, 4).to(DEV)
    h, g1, g2 = (t.to(DEV) for t in operands(c.n, H, 20 + H))
    attr, rank = attribute(c, st, w, h, g1, g2, sentinel=-777.0)
    st.check_status()
    assert st.wc is not None
    ref = flat_reference(c, st.src, st.off, st.flags, st.wc, w, h, g1, g2)
    assert int((((ref.f & 2) != 0) & (ref.c > 1)).sum()) > 0            # cn2 entries with a walk count above 1 exist
    check_against_fp64(ref, attr, rank, H, -777.0)


@pytest.mark.parametrize("H", WIDTHS)
def test_attribution_known_answer_identity_embeddings(hiplib, H):
    """N = H nodes with h = I: <h[k], g[e]> = g[e][k] exactly, every other product is an exact zero.  A star (node 0 joined to
    nodes 1 .. N/2 - 1) plus the path 1 - 2 - .. - N-1, power-of-two weights: attr[q] is bit for bit {wa g1[e][k], wb g2[e][k]}."""
    from ocn_amd import ops
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.utils import CNState
    n = H
    star = torch.stack([torch.zeros(n // 2 - 1, dtype=torch.long), torch.arange(1, n // 2)])
    path = torch.stack([torch.arange(1, n - 1), torch.arange(2, n)])
    ei = torch.cat([star, star.flip(0), path, path.flip(0)], dim=1)
    adj = SparseTensor.from_edge_index(ei.to(DEV), sparse_sizes=(n, n))
    adj2 = product_adj2(adj)
    e = torch.tensor([[0, 0, 1, 1, 2, 3, n - 1, 5, 0, 4, n - 1], [2, n // 2 - 1, 3, 2, 0, 1, n - 3, 5, 0, 9, 1]]).to(DEV)
    g = torch.Generator().manual_seed(H)
    pw = lambda: torch.pow(2.0, torch.randint(-2, 3, (n,), generator=g).float())
    w1, t, inv2 = pw(), pw(), pw()
    w1[::5] = 0.0; t[1::4] = 0.0; inv2[2::7] = 0.0
    w = torch.stack([w1, t, inv2, torch.zeros(n)], dim=1).contiguous().to(DEV)
    nb = e.shape[1]
    g1, g2 = torch.randn(nb, H, generator=g).to(DEV), torch.randn(nb, H, generator=g).to(DEV)
    st = CNState(adj, adj, adj2, e)
    attr, rank = ops.cn_attribution(adj._rowptr, adj._col, st.src, st.off, st.flags, None, w, torch.eye(H, device=DEV), g1, g2)
    st.check_status()
    c = SimpleNamespace(rowptr=adj._rowptr.cpu(), col=adj._col.cpu().long())
    ref = flat_reference(c, st.src, st.off, st.flags, None, w, torch.eye(H), g1, g2)
    assert int((ref.member & (ref.wa != 0)).sum()) >= 5 and int((ref.member & (ref.wb != 0)).sum()) >= 5
    assert int(ref.member.sum()) < ref.total
    want1 = torch.where(ref.member & (ref.wa != 0), ref.wa * g1.cpu()[ref.e, ref.k], torch.zeros(()))
    want2 = torch.where(ref.member & (ref.wb != 0), ref.wb * g2.cpu()[ref.e, ref.k], torch.zeros(()))
    got = attr.cpu()[:ref.total]
    assert torch.equal(bits(got[:, 0]), bits(want1)) and torch.equal(bits(got[:, 1]), bits(want2))
    want_rank = torch.where(ref.member, want1 + want2, torch.full((), NINF))
    assert torch.equal(bits(rank.cpu()[:ref.total]), bits(want_rank))


def test_attribution_is_fixed_by_its_input(graph):
    from ocn_amd.utils import CNState
    c, H = graph, 128
    st = CNState(c.adj, c.adj, c.adj2, c.e)
    w = random_table(c.n, 3).to(DEV)
    h, g1, g2 = (t.to(DEV) for t in operands(c.n, H, 77))
    total = int(st.off[-1])
    first = [bits(t[:total]) for t in attribute(c, st, w, h, g1, g2)]
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(9)).to(DEV)
    for order in (None, st.order, perm):
        again = [bits(t[:total]) for t in attribute(c, st, w, h, g1, g2, order=order)]
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    # every candidate moved to another place in another batch (a permuted subset), under the same table
    pick = torch.randperm(B, generator=torch.Generator().manual_seed(10))[:150]
    pick = torch.cat([pick, torch.nonzero(c.e_cpu[0] == c.hub).flatten()]).unique()
    pick = pick[torch.randperm(pick.numel(), generator=torch.Generator().manual_seed(11))]
    pd = pick.to(DEV)
    st2 = CNState(c.adj, c.adj, c.adj2, c.e[:, pd].contiguous())
    a2, r2 = attribute(c, st2, w, h, g1[pd].contiguous(), g2[pd].contiguous())
    off, off2 = st.off.cpu(), st2.off.cpu()
    a2, r2 = bits(a2), bits(r2)
    for new, old in enumerate(pick.tolist()):
        lo, hi, lo2, hi2 = int(off[old]), int(off[old + 1]), int(off2[new]), int(off2[new + 1])
        assert hi - lo == hi2 - lo2
        assert torch.equal(a2[lo2:hi2], first[0][lo:hi]) and torch.equal(r2[lo2:hi2], first[1][lo:hi]), old


def pooled_bound(ref, w_side, ad_side, H, nb):
    """(m_e + H + 3) u sum_k |w_k| sum_f |h[k][f] g[e][f]| per candidate, and the member counts m_e."""
    m_e = torch.zeros(nb, dtype=torch.double).index_add_(0, ref.e, ref.member.double())
    mass = torch.zeros(nb, dtype=torch.double).index_add_(0, ref.e, torch.where(ref.member, w_side.double().abs() * ad_side,
                                                                              torch.zeros((), dtype=torch.double)))
    return (m_e + H + 3) * U * mass, m_e


@pytest.mark.parametrize("route,H", [("pattern", 64), ("pattern", 256), ("walk", 32)])
def test_attribution_sums_to_the_pooling(graph, route, H):
    """sum_p a1 = <g1[e], xcn1[e]> for every candidate, the hub sources among them (there the pooling takes its hub path and the
    attribution many rounds), within the rounding of both sides."""
    from ocn_amd.utils import CNState
    c = graph
    st = CNState(c.adj, c.adj, c.adj2, c.e) if route == "pattern" else CNState(c.adj, None, None, c.e, walk=True)
    w = random_table(c.n, 6).to(DEV)
    h, g1, g2 = (t.to(DEV) for t in operands(c.n, H, 30 + H))
    xcn1, xcn2, _ = st.gather(w, h)
    attr, _ = attribute(c, st, w, h, g1, g2)
    st.check_status()
    ref = flat_reference(c, st.src, st.off, st.flags, st.wc, w, h, g1, g2)
    a = attr.cpu()[:ref.total].double()
    for q, (x, g, wgt, ad) in enumerate(((xcn1, g1, ref.wa, ref.ad1), (xcn2, g2, ref.wb, ref.ad2))):
        got = torch.zeros(B, dtype=torch.double).index_add_(0, ref.e, a[:, q])
        want = (g.cpu().double() * x.cpu().double()).sum(1)
        bound, m_e = pooled_bound(ref, wgt, ad, H, B)
        err = (got - want).abs()
        busy = bound > 0
        print(f"sums {route} H={H} side {q + 1}: worst error / bound = {(err[busy] / bound[busy]).max().item():.3f}, "
              f"largest member count {int(m_e.max())}")
        assert bool((err <= bound).all()) and int(busy.sum()) > 100
        assert all(m_e[r] > 100 for r in torch.nonzero(c.e_cpu[0] == c.hub).flatten().tolist())


# ---- explain_links ---------------------------------------------------------------------------------------------------------------
H_E = 64
CASES = ("cn5", "cn5_ip", "cn7", "cn8", "cn5_frozen")


def make_case(c, case):
    from ocn_amd.frozen import freeze_columns
    from ocn_amd.model import predictor_dict
    kind = case.split("_")[0]
    torch.manual_seed(31)
    pred = predictor_dict[kind](H_E, H_E, 1, 3, 0.0, 0.0, True).eval()
    with torch.no_grad():
        pred.alpha.copy_(torch.tensor([0.4, -0.3, 0.1]))
        if case == "cn5_ip":
            pred.innerprod.fill_(0.37)
    pred = pred.to(DEV)
    args = SimpleNamespace(sum=1.0) if kind == "cn7" else None
    fc = None
    if case == "cn5_frozen":
        fc = freeze_columns(pred, c.adj, c.adj2, c.e[:, :200].t().contiguous(), args)
        pred.set_frozen_columns(fc, args)
    return pred, args, fc


_explained = {}


def explained(c, case, rank="signed", counterfactual=False):
    """One ``explain_links`` call per (case, rank, counterfactual), shared by the tests that read it."""
    from ocn_amd.explain import explain_links
    key = (case, rank, counterfactual)
    if key not in _explained:
        pred, args, fc = make_case(c, case)
        x = torch.randn(c.n, H_E, generator=torch.Generator().manual_seed(41)).to(DEV)
        table = None if fc is None else fc.weights.clone()
        exp = explain_links(pred, x, c.adj, c.adj2, c.e.t().contiguous(), m=4 if counterfactual else 8, args=args, rank=rank,
                            counterfactual=counterfactual, return_flat=True)
        _explained[key] = SimpleNamespace(pred=pred, args=args, fc=fc, table=table, x=x, exp=exp)
    return _explained[key]


def heads64(pred):
    """The predictor's head modules as a ``.cpu().double()`` copy, evaluated through the modules themselves."""
    cp = copy.deepcopy(pred).cpu().double().eval()
    return lambda x1, x2, x3: cp._heads(None, x1, x2, x3, None).reshape(-1)


def batch_reference(c, r):
    """The flags, the table and the flat reference of the batch ``explain_links`` explained, formed again by hand."""
    from ocn_amd.utils import adjoverlap, fuse
    e = c.e
    with torch.no_grad():
        st = fuse(adjoverlap(c.adj, c.adj, e), adjoverlap(c.adj, c.adj2, e), e, None, adj=c.adj)
        w = r.pred._weights(st, r.args).clone()
    g1, g2, _ = r.exp._grads
    return st, w, flat_reference(c, st.src, st.off, st.flags, st.wc, w, r.x, g1, g2)


def host_topk(rank, off, m):
    """Per segment the m best positions under ocn_segment_topk's total order: higher value first (+0 == -0), then lower
    position; -inf entries never listed."""
    out = []
    for e in range(off.numel() - 1):
        lo, hi = int(off[e]), int(off[e + 1])
        seg = rank[lo:hi].tolist()
        cand = sorted((p for p in range(hi - lo) if seg[p] != NINF), key=lambda p: (-seg[p], p))[:m]
        out.append([lo + p for p in cand])
    return out


@pytest.mark.parametrize("case,rank", [(case, "signed") for case in CASES] + [("cn5_ip", "magnitude"), ("cn8", "magnitude")])
def test_explain_links_end_to_end(graph, case, rank):
    from ocn_amd.utils import adjoverlap
    c = graph
    r = explained(c, case, rank)
    exp, pred, m = r.exp, r.pred, 8
    # (e) nothing of the predictor changed
    assert all(p.grad is None for p in pred.parameters()) and not pred.training
    assert pred._frozen is r.fc and (r.fc is None or torch.equal(r.fc.weights, r.table))
    assert exp.score.shape == (B,) and exp.nodes.shape == (B, m) and exp.contrib.shape == (B, m, 2) and exp.kind.shape == (B, m)
    assert exp.nodes.dtype == torch.int64 and exp.kind.dtype == torch.uint8 and exp.drop is None
    # (a) the score is the direct call's
    with torch.no_grad():
        handles = (adjoverlap(c.adj, c.adj, c.e), adjoverlap(c.adj, c.adj2, c.e))
        direct = (pred(r.x, c.adj, *handles, c.e, r.args) if r.args is not None else pred(r.x, c.adj, *handles, c.e)).reshape(-1)
    err = (exp.score - direct).abs()
    print(f"explain {case} {rank}: max |score - direct| = {err.max().item():.3e}, max |score| = {direct.abs().max().item():.3e}")
    assert bool((err <= 1e-5 + 1e-5 * direct.abs()).all())
    # (b) the gradients are autograd's through an fp64 copy of the heads on the same pooled vectors
    xs = [t.detach().cpu().double().requires_grad_() for t in exp._pooled_vectors]
    with torch.enable_grad():
        want = torch.autograd.grad(heads64(pred)(*xs).sum(), xs)
    for got, wnt in zip(exp._grads, want):
        tol = 2e-5 * max(1.0, wnt.abs().max().item())
        assert (got.cpu().double() - wnt).abs().max().item() <= tol
    # (c) nodes / contrib / kind are exactly the top-m of the flat rank vector
    off, attr, rk = (t.cpu() for t in exp.flat)
    st, w, ref = batch_reference(c, r)
    assert torch.equal(off, ref.off)
    by = rk if rank == "signed" else torch.where(rk == NINF, rk, rk.abs())
    listed = host_topk(by[:ref.total], off, m)
    src = c.e_cpu[0]
    nodes, contrib, kind = exp.nodes.cpu(), exp.contrib.cpu(), exp.kind.cpu()
    flags = st.flags.cpu()
    short = 0
    for e, pos in enumerate(listed):
        n_e = len(pos)
        want_nodes = [int(c.col[int(c.rowptr[src[e]]) + p - int(off[e])]) for p in pos]
        assert nodes[e, :n_e].tolist() == want_nodes and nodes[e, n_e:].tolist() == [-1] * (m - n_e), e
        assert torch.equal(bits(contrib[e, :n_e]), bits(attr[pos])) if n_e else True
        assert kind[e, :n_e].tolist() == flags[pos].tolist() if n_e else True
        assert bool((bits(contrib[e, n_e:]) == 0).all()) and bool((kind[e, n_e:] == 0).all())
        assert n_e == min(m, int(ref.member[ref.e == e].sum()))
        short += n_e < m
    assert 0 < short < B                                                # padded and full rows both occur
    assert torch.equal(exp.cnt1.cpu(), st.cnt1.cpu()) and torch.equal(exp.cnt2.cpu(), st.cnt2.cpu())
    # (d) pooled and pair against the fp64 inner products
    x1, x2, x3 = (t.cpu().double() for t in exp._pooled_vectors)
    g1, g2, g3 = (t.cpu().double() for t in exp._grads)
    for q, (x, g, wgt, ad) in enumerate(((x1, g1, ref.wa, ref.ad1), (x2, g2, ref.wb, ref.ad2))):
        bound, _ = pooled_bound(ref, wgt, ad, H_E, B)
        assert bool(((exp.pooled[:, q].cpu().double() - (g * x).sum(1)).abs() <= bound).all())
    assert bool(((exp.pair.cpu().double() - (g3 * x3).sum(1)).abs() <= (H_E + 3) * U * (g3 * x3).abs().sum(1)).all())


def test_explain_links_frozen_is_batch_independent(graph):
    """Frozen, a candidate explained inside two different batches gets the same ``contrib`` rows bit for bit."""
    from ocn_amd.explain import explain_links
    c = graph
    r = explained(c, "cn5_frozen")
    pick = torch.randperm(B, generator=torch.Generator().manual_seed(3))[:90]
    pick = torch.cat([pick, torch.nonzero(c.e_cpu[0] == c.hub).flatten()]).unique()
    pick = pick[torch.randperm(pick.numel(), generator=torch.Generator().manual_seed(4))]
    other = explain_links(r.pred, r.x, c.adj, c.adj2, c.e[:, pick.to(DEV)].t().contiguous(), m=8, args=r.args)
    assert torch.equal(bits(other.contrib), bits(r.exp.contrib[pick.to(DEV)]))
    assert torch.equal(other.nodes.cpu(), r.exp.nodes.cpu()[pick]) and torch.equal(other.kind.cpu(), r.exp.kind.cpu()[pick])
    assert bool((other.nodes >= 0).any())


@pytest.mark.parametrize("case", ["cn8", "cn5_frozen", "cn5"])
def test_explain_links_counterfactual(graph, case):
    """``drop`` against the heads re-evaluated in fp64 on the CPU with the member's wa h[k] and wb h[k] removed from the fp64
    pooled sums; NaN on padding.  Unfrozen cn5: a listed member whose column occurs once in the batch as a cn1-only entry has
    wa = wb = 0 (w1 = 0 below two cn1 entries; t = nip w1 = 0, so wb = (0 - 0) inv2) and its ``drop`` is exactly 0.0.  (A column
    that occurs once as a cn2 entry has S2 = 1 and wb = 1: it is fetched, and its ``drop`` is not zero.)"""
    c = graph
    r = explained(c, case, counterfactual=True)
    exp, m = r.exp, 4
    st, w, ref = batch_reference(c, r)
    nodes, drop, kind = exp.nodes.cpu(), exp.drop.cpu(), exp.kind.cpu()
    assert drop.shape == (B, m) and torch.equal(drop.isnan(), nodes < 0) and bool((nodes < 0).any()) and bool((nodes >= 0).any())
    if case == "cn5":
        # the listed positions, by node id within the candidate's segment
        once = torch.bincount(ref.k[ref.member], minlength=c.n) == 1
        dead = []
        for e in range(B):
            seg = torch.nonzero(ref.e == e).flatten()
            for rr in range(m):
                if nodes[e, rr] >= 0 and once[nodes[e, rr]] and int(kind[e, rr]) == 1:
                    q = seg[ref.k[seg] == nodes[e, rr]]
                    assert q.numel() == 1 and float(ref.wa[q]) == 0.0 and float(ref.wb[q]) == 0.0
                    dead.append((e, rr))
        pa, pk, pb = c.path                                               # (a, b): its one member k is listed, and k is nobody else's
        assert any(c.e_cpu[:, e].tolist() == [pa, pb] and int(nodes[e, rr]) == pk for e, rr in dead)
        assert all(float(drop[e, rr]) == 0.0 for e, rr in dead)
        return
    hd = r.x.cpu().double()
    zero = torch.zeros((), dtype=torch.double)
    x1 = torch.zeros(B, H_E, dtype=torch.double).index_add_(0, ref.e, torch.where(ref.member, ref.wa.double(), zero)[:, None] * hd[ref.k])
    x2 = torch.zeros(B, H_E, dtype=torch.double).index_add_(0, ref.e, torch.where(ref.member, ref.wb.double(), zero)[:, None] * hd[ref.k])
    x3 = hd[c.e_cpu[0]] * hd[c.e_cpu[1]]
    rows, r1, r2, r3 = [], [x1], [x2], [x3]
    for e in range(B):
        seg = torch.nonzero(ref.e == e).flatten()
        for rr in range(m):
            if nodes[e, rr] >= 0:
                q = seg[ref.k[seg] == nodes[e, rr]]
                assert q.numel() == 1 and int(ref.f[q]) == int(kind[e, rr])
                rows.append((e, rr))
                r1.append((x1[e] - ref.wa[q].double() * hd[nodes[e, rr]])[None])
                r2.append((x2[e] - ref.wb[q].double() * hd[nodes[e, rr]])[None])
                r3.append(x3[e][None])
    with torch.no_grad():
        s = heads64(r.pred)(torch.cat(r1), torch.cat(r2), torch.cat(r3))
    worst = 0.0
    for i, (e, rr) in enumerate(rows):
        want = float(s[e] - s[B + i])
        tol = 2e-5 * max(1.0, abs(float(s[e])))
        worst = max(worst, abs(float(drop[e, rr]) - want) / tol)
        assert abs(float(drop[e, rr]) - want) <= tol, (e, rr, float(drop[e, rr]), want)
    print(f"counterfactual {case}: {len(rows)} listed members, worst error / tolerance = {worst:.3f}, "
          f"largest |drop| = {drop[~drop.isnan()].abs().max().item():.3e}")
    assert len(rows) > 200 and drop[~drop.isnan()].abs().max().item() > 1e-4


def test_example_driver_explains_its_recommendations(hiplib):
    """``--recommend 5 --recommend-explain 3`` in a child process on the smallest synthetic dataset: exit 0, and every printed
    common neighbour is a neighbour of its source."""
    from ocn_amd.synth import loaddataset_like
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_like_reference.py"), "--dataset", "cora", "--epochs", "1",
                          "--recommend", "5", "--recommend-explain", "3"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert re.search(r"explain: \d+ links as one batch, predictor frozen = False", out.stdout)
    data, _ = loaddataset_like("cora", False)
    rowptr, col = data.adj_t._rowptr.cpu(), data.adj_t._col.cpu()
    seen = 0
    for line in out.stdout.splitlines():
        mt = re.match(r"explain source (\d+) target (\d+) score \S+ pooled \S+ \S+ top-3:(.*)", line)
        if mt:
            s = int(mt.group(1))
            nbrs = set(col[int(rowptr[s]):int(rowptr[s + 1])].tolist())
            ids = [int(k) for k in re.findall(r"(\d+)\(", mt.group(3))]
            assert len(ids) <= 3 and all(k in nbrs for k in ids), line
            seen += len(ids)
    assert seen > 0
