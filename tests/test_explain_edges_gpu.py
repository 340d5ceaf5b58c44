"""Message saliency on the GPU: ``explain_link_edges`` against the test's own dense restatement of the encoders with mask
variables (torch, CPU), the score taken through the oracle's predictor forward — five encoders x three predictors — its support
in the graph, degenerate pairs, the selection, a frozen predictor inside two batches, and the example driver's flag.

The bar of the comparison is the project's bar for encoder input gradients (``test_encoder_backward_matches_oracle_autograd``):
3e-5 max(1, max|ref|).  The mask gradient of a layer is one length-H dot product per message of the same upstream gradient
that the input gradient sums."""
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from oracle import ocn_oracle as O
from tests.helpers import product_adj2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, B = 32, 64
N, HUB, ISO = 120, 117, 119                                              # 118 and 119 are isolated
BAR = 3e-5

# name -> (class, conv_fn, layers, ln, res, jk)
ENCODERS = {
    "GCN-gcn":     ("GCN", "gcn", 2, True, True, False),
    "GCN-gin":     ("GCN", "gin", 3, False, False, True),
    "GCN-puregcn": ("GCN", "puregcn", 2, False, False, False),
    "GCN-sage":    ("GCN", "sage", 2, True, False, False),
    "GCN2-gcn":    ("GCN2", "gcn", 2, True, False, False),
}
PREDICTORS = ("cn5", "cn7", "cn8")


@pytest.fixture(scope="module")
def graph(hiplib):
    """110 nodes of a clique-rich Chung-Lu graph, a hub joined to 60 of them, a bare path 110 - 111 - 112 - 113 in a component of
    its own, and isolated nodes; 64 candidates, among them a pair rich in common neighbours, the hub as a source, a pair with an
    isolated endpoint and a pair across the two components: both endpoints have neighbours, and no common neighbour of either
    kind."""
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.synth import chung_lu_graph, sample_edges
    ei = chung_lu_graph(110, avg_deg=8, max_deg=30, seed=11, clique_frac=0.5)
    gen = torch.Generator().manual_seed(3)
    spokes = torch.randperm(110, generator=gen)[:60]
    ei = torch.cat([ei, torch.stack([torch.full_like(spokes, HUB), spokes]), torch.tensor([[110, 111, 112], [111, 112, 113]])], dim=1)
    oadj = O.to_symmetric(O.from_edge_index(ei, N))
    oadj2 = O.adj2_sparse(oadj)
    A = torch.zeros(N, N)
    A[oadj.row, oadj.col] = 1.0
    assert int(A.diagonal().sum()) == 0 and torch.equal(A, A.t()) and int(A[HUB].sum()) == 60 and int(A[118:].sum()) == 0
    e = sample_edges(oadj.row, oadj.col, 110, B - 4, seed=7, pos_frac=0.6)
    far = int(torch.nonzero(A[:110].sum(1) > 0)[0])
    special = torch.tensor([[HUB, 110, int(e[0, 0]), 110], [int(spokes[0]), ISO, int(e[1, 0]), far]])
    e = torch.cat([e, special], dim=1).contiguous()
    assert e.shape == (2, B)
    ocn1, ocn2 = O.adjoverlap(oadj, oadj, e), O.adjoverlap(oadj, oadj2, e)
    c1, c2 = torch.bincount(ocn1.row, minlength=B), torch.bincount(ocn2.row, minlength=B)
    both = torch.where((c1 > 0) & (c2 > 0) & (e[0] != HUB), c1 + c2, torch.zeros_like(c1))
    rich = int(both.argmax())
    assert int(both[rich]) >= 8 and int(c1[B - 1] + c2[B - 1]) == 0 and int(c1[B - 3] + c2[B - 3]) == 0 and int(c2[B - 4]) > 0
    adj = SparseTensor.from_edge_index(torch.stack([oadj.row, oadj.col]).to(DEV), sparse_sizes=(N, N))
    rowptr, col = adj._rowptr.cpu(), adj._col.cpu().long()
    row = torch.repeat_interleave(torch.arange(N), rowptr[1:] - rowptr[:-1])
    assert torch.equal(row, oadj.row) and torch.equal(col, oadj.col)
    return SimpleNamespace(oadj=oadj, oadj2=oadj2, A=A, adj=adj, adj2=product_adj2(adj), e=e, ed=e.to(DEV), ocn1=ocn1, ocn2=ocn2,
                           row=row, col=col, nnz=int(col.numel()), which=dict(rich=rich, none=B - 1, hub=B - 4, iso=B - 3))


def make_encoder(name):
    import ocn_amd.model as M
    cls, conv, L, ln, res, jk = ENCODERS[name]
    torch.manual_seed(8)
    enc = getattr(M, cls)(H, H, H, L, 0.0, ln, res, -1, conv, jk).eval()
    return enc, {k: v.detach().clone() for k, v in enc.state_dict().items()}


def make_predictor(kind):
    from ocn_amd.model import predictor_dict
    torch.manual_seed(31)
    pred = predictor_dict[kind](H, H, 1, 3, 0.0, 0.0, True).eval()
    with torch.no_grad():
        pred.alpha.copy_(torch.tensor([0.4, -0.3, 0.1]))
        if kind == "cn5":
            pred.innerprod.fill_(0.37)
    return pred, {k: v.detach().clone() for k, v in pred.state_dict().items()}, (SimpleNamespace(sum=1.0) if kind == "cn7" else None)


def dense_encoder(sd, x, A, masks, name):
    """The encoders of ENCODERS restated densely from the state dict: every layer is post * ((C * M) x + self), C the layer's
    coefficient matrix on the pattern of A — formed from A alone, so it does not see the mask — and M the layer's mask variable."""
    cls, conv, L, ln, res, jk = ENCODERS[name]
    deg = A.sum(1)
    d = (1 + deg).rsqrt()
    pure = "pure" in conv
    if "xemb.1.weight" in sd:
        x = F.linear(x, sd["xemb.1.weight"], sd["xemb.1.bias"])
    jkx = []
    for i in range(L):
        Mi = masks[i]
        if cls == "GCN2":                                                # PureConv2 gcn: (A * n n^T) x, then Linear(no bias) + ReLU
            y = torch.relu(F.linear(((d[:, None] * A * d[None, :]) * Mi) @ x, sd[f"convs.{i}.lin.0.weight"]))
        elif pure:                                                       # PureConv gcn: n * (A (n * x) + n * x)
            y = d[:, None] * (((A * d[None, :]) * Mi) @ x + d[:, None] * x)
        else:
            xw = F.linear(x, sd[f"convs.{i}.lin.weight"])
            if conv == "gcn":                                            # D^-1/2 (A + I) D^-1/2: the self term is no message
                y = ((d[:, None] * A * d[None, :]) * Mi) @ xw + (d * d)[:, None] * xw
            elif conv == "gin":
                y = (A * Mi) @ xw
            else:                                                        # sage: mean
                y = ((A / deg.clamp(min=1)[:, None]) * Mi) @ xw
            y = y + sd[f"convs.{i}.bias"]
        if not pure and (i == 0 or i < L - 1):
            if ln:
                w = sd[f"lins.{i}.0.weight"]
                y = F.layer_norm(y, (w.numel(),), w, sd[f"lins.{i}.0.bias"], 1e-5)
            y = torch.relu(y)
        x = y + x if (res and y.shape[-1] == x.shape[-1]) else y
        if jk:
            jkx.append(x)
    if jk:
        x = torch.sum(torch.stack(jkx, 0) * sd["jkparams"].reshape(-1, 1, 1), dim=0)
    return x


def oracle_scores(kind, sd, h, c, args, e=None, ocn=None):
    e = c.e if e is None else e
    ocn1, ocn2 = (c.ocn1, c.ocn2) if ocn is None else ocn
    if kind == "cn5":
        return O.cn5_forward(sd, h, ocn1, ocn2, e, ln=True).reshape(-1)
    if kind == "cn7":
        return O.cn7_forward(sd, h, ocn1, ocn2, e, args.sum, ln=True).reshape(-1)
    return O._heads(sd, h, O.spmm_add(ocn1, h), O.spmm_add(ocn2, h), e, True, False, False).reshape(-1)


def reference(c, name, kind, x, dtype=torch.float32):
    """(scores [B], per_layer [which][L, nnz]) of the dense restatement, one forward, one backward per explained candidate."""
    _, esd = make_encoder(name)
    _, psd, args = make_predictor(kind)
    cast = lambda sd: {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    L = ENCODERS[name][2]
    masks = [torch.ones(N, N, dtype=dtype, requires_grad=True) for _ in range(L)]
    h = dense_encoder(cast(esd), x.to(dtype), c.A.to(dtype), masks, name)
    s = oracle_scores(kind, cast(psd), h, c, args)
    per = {}
    for tag, q in c.which.items():
        g = torch.autograd.grad(s[q], masks, retain_graph=True, allow_unused=True)
        per[tag] = torch.stack([torch.zeros(c.nnz, dtype=dtype) if t is None else t[c.row, c.col] for t in g])
    return s.detach(), per


_runs = {}


def explained(c, name, kind, tag, **kw):
    from ocn_amd.explain import explain_link_edges
    key = (name, kind, tag, tuple(sorted(kw.items())))
    if key not in _runs:
        enc, _ = make_encoder(name)
        pred, _, args = make_predictor(kind)
        x = torch.randn(N, H, generator=torch.Generator().manual_seed(41))
        enc, pred = enc.to(DEV), pred.to(DEV)
        ex = explain_link_edges(enc, pred, x.to(DEV), c.adj, c.adj2, c.ed.t().contiguous(), c.which[tag], args=args, return_flat=True, **kw)
        assert all(p.grad is None for p in list(enc.parameters()) + list(pred.parameters())) and not enc.training and not pred.training
        _runs[key] = SimpleNamespace(ex=ex, x=x, enc=enc, pred=pred, args=args)
    return _runs[key]


@pytest.mark.parametrize("kind", PREDICTORS)
@pytest.mark.parametrize("name", list(ENCODERS))
def test_per_layer_against_the_dense_reference(graph, name, kind):
    """``flat`` (every message of every layer) for the CN-rich pair, the pair without a common neighbour and the hub source; the
    score within the project's 2e-5 bar of the reference's and of the served one."""
    from ocn_amd.utils import adjoverlap
    c = graph
    L = ENCODERS[name][2]
    x = torch.randn(N, H, generator=torch.Generator().manual_seed(41))
    scores, per = reference(c, name, kind, x)
    for tag in ("rich", "none", "hub"):
        r = explained(c, name, kind, tag)
        ex, ref = r.ex, per[tag]
        assert ex.flat.shape == (L, c.nnz) and ex.per_layer.shape == (20, L) and ex.entries.shape == (20, 2)
        err = (ex.flat.cpu() - ref).abs().max().item()
        scale = max(1.0, ref.abs().max().item())
        print(f"explain-edges {name} {kind} {tag}: max |per_layer - ref| = {err:.3e}, max |ref| = {ref.abs().max().item():.3e}, "
              f"error / bar = {err / (BAR * scale):.3f}, non-zero per layer = {[int((ex.flat[l] != 0).sum()) for l in range(L)]}")
        assert err <= BAR * scale, (name, kind, tag, err, scale)
        assert abs(float(ex.score) - float(scores[c.which[tag]])) <= 2e-5 * max(1.0, abs(float(scores[c.which[tag]])))
        assert ex.input_share.shape == (N,) and bool(torch.isfinite(ex.input_share).all())
    with torch.no_grad():
        hs = r.enc(r.x.to(DEV), c.adj)
        hd = (adjoverlap(c.adj, c.adj, c.ed), adjoverlap(c.adj, c.adj2, c.ed))
        served = (r.pred(hs, c.adj, *hd, c.ed, r.args) if r.args is not None else r.pred(hs, c.adj, *hd, c.ed)).reshape(-1)
    q = c.which["hub"]
    assert abs(float(r.ex.score) - float(served[q])) <= 2e-5 * max(1.0, abs(float(served[q])))


def within(A, seeds, hops):
    """bool [N]: the nodes within ``hops`` hops of the seed set (the seeds themselves included)."""
    m = torch.zeros(N, dtype=torch.bool)
    m[list(seeds)] = True
    for _ in range(hops):
        m = m | ((A @ m.float()) > 0)
    return m


@pytest.mark.parametrize("name,kind", [("GCN-gcn", "cn5"), ("GCN-gin", "cn8"), ("GCN-puregcn", "cn7")])
def test_support_and_degenerate_pairs(graph, name, kind):
    """Layer l is exactly zero outside the rows within L - 1 - l hops of {i, j} and the pair's common-neighbour members; the
    CN-rich pair has at least 50 non-zero messages per layer; the pair without a common neighbour and the pair with an isolated
    endpoint give finite values."""
    c = graph
    L = ENCODERS[name][2]
    for tag, q in c.which.items():
        ex = explained(c, name, kind, tag).ex
        flat = ex.flat.cpu()
        assert bool(torch.isfinite(flat).all()) and bool(torch.isfinite(ex.saliency).all()) and bool(torch.isfinite(ex.score))
        i, j = c.e[:, q].tolist()
        members = set(c.ocn1.col[c.ocn1.row == q].tolist()) | set(c.ocn2.col[c.ocn2.row == q].tolist())
        assert (tag in ("none", "iso")) == (not members)
        for l in range(L):
            inside = within(c.A, {i, j} | members, L - 1 - l)[c.row]
            assert bool((flat[l][~inside] == 0).all()), (tag, l)
            assert bool((flat[l][inside] != 0).any()) or tag == "iso"
            if tag == "rich":
                assert int((flat[l] != 0).sum()) >= 50, (l, int((flat[l] != 0).sum()))
        if tag == "iso":                                                # nothing reaches the isolated endpoint: no row of it exists
            assert int(c.A[j].sum()) == 0 and bool((flat[:, c.row == j] == 0).all())


@pytest.mark.parametrize("rank", ["magnitude", "signed"])
def test_selection_equals_a_host_selection_from_flat(graph, rank):
    """``entries`` / ``saliency`` / ``per_layer``: the non-zero totals (the layers added in layer order) ranked by |.| or by the
    signed value, descending, ties to the lower position; padding -1 / 0."""
    c = graph
    top = 128
    seen_pad = False
    for tag in ("rich", "none", "iso"):
        ex = explained(c, "GCN-gcn", "cn8", tag, top=top, rank=rank).ex
        flat = ex.flat.cpu()
        total = flat[0].clone()
        for l in range(1, flat.shape[0]):
            total = total + flat[l]
        key = total.abs() if rank == "magnitude" else total
        order = sorted((p for p in range(c.nnz) if total[p] != 0), key=lambda p: (-float(key[p]), p))[:top]
        n = len(order)
        ent, sal, per = ex.entries.cpu(), ex.saliency.cpu(), ex.per_layer.cpu()
        assert ent.shape == (top, 2) and ent.dtype == torch.int64
        assert ent[:n, 0].tolist() == c.row[order].tolist() and ent[:n, 1].tolist() == c.col[order].tolist()
        assert torch.equal(sal[:n].view(torch.int32), total[order].view(torch.int32))
        assert torch.equal(per[:n], flat[:, order].t())
        assert bool((ent[n:] == -1).all()) and bool((sal[n:] == 0).all()) and bool((per[n:] == 0).all())
        seen_pad |= n < top
        assert n > 0
    assert seen_pad


def test_frozen_predictor_is_batch_independent(graph):
    """With frozen column weights the same pair inside two different batches gets the same ``per_layer`` within the bar."""
    from ocn_amd.explain import explain_link_edges
    from ocn_amd.frozen import freeze_columns
    c = graph
    enc, _ = make_encoder("GCN-gcn")
    pred, _, args = make_predictor("cn5")
    enc, pred = enc.to(DEV), pred.to(DEV)
    edges = c.ed.t().contiguous()
    pred.set_frozen_columns(freeze_columns(pred, c.adj, c.adj2, edges[:40].contiguous(), args), args)
    x = torch.randn(N, H, generator=torch.Generator().manual_seed(41)).to(DEV)
    q = c.which["rich"]
    a = explain_link_edges(enc, pred, x, c.adj, c.adj2, edges, q, return_flat=True)
    pick = torch.tensor([5, q, 9, 30, 31, 2, 50], device=DEV)
    b = explain_link_edges(enc, pred, x, c.adj, c.adj2, edges[pick].contiguous(), 1, return_flat=True)
    err = (a.flat - b.flat).abs().max().item()
    scale = max(1.0, a.flat.abs().max().item())
    print(f"frozen: max |per_layer(batch of 64) - per_layer(batch of 7)| = {err:.3e}, max = {a.flat.abs().max().item():.3e}")
    assert err <= BAR * scale and int((a.flat != 0).sum()) > 100
    assert abs(float(a.score) - float(b.score)) <= 2e-5 * max(1.0, abs(float(a.score)))
    assert pred._frozen is not None and all(p.grad is None for p in pred.parameters())


def test_example_driver_explains_down_to_the_edges(hiplib):
    """``--recommend 5 --recommend-explain-edges 6`` in a child process on the smallest synthetic dataset: exit 0, and every
    printed message is an edge of the graph."""
    from ocn_amd.synth import loaddataset_like
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_like_reference.py"), "--dataset", "cora", "--epochs", "1",
                          "--recommend", "5", "--recommend-explain-edges", "6"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert re.search(r"explain-edges source \d+ target \d+ score ", out.stdout)
    data, _ = loaddataset_like("cora", False)
    r, cc, _ = data.full_adj_t.coo()                                  # (symmetric: the adjacency the recommendation runs on)
    known = set(zip(r.tolist(), cc.tolist()))
    found = re.findall(r"explain-edges message (\d+)->(\d+) \(", out.stdout)
    assert 1 <= len(found) <= 6 and all((int(u), int(v)) in known for v, u in found)
