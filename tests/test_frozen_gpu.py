"""Frozen column weights (ocn_amd/frozen.py) on the GPU: ``ocn_cn_pool_frozen`` against the chain it replaces, against cn8's
one pass and against a closed form; the frozen predictors against the unfrozen ones on the reference batch; batch independence
of every frozen score, through ``score_edges`` and ``recommend_links``; the refusals that need a device."""
from types import SimpleNamespace

import pytest
import torch

from oracle import ocn_oracle as O
from ocn_amd.synth import chung_lu_graph, sample_edges
from tests.helpers import close, product_adj2, to_product

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WIDTHS = (16, 32, 64, 128, 256, 512)
N_REF = 750                                                              # candidates of the reference batch R; the rest is the served list C


def rowcount(m):
    return torch.bincount(m.row, minlength=m.n_rows)


def bits(t):
    """int32 view of an fp32 tensor on the host: compared this way the signs of zeros count."""
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def hubs(hiplib):
    """The ``hubs`` graph of tests/test_cn8_gpu.py, restated (same recipe, same seeds): a Chung-Lu graph with cliques, a hub with
    1 400 neighbours (source rows longer than the 1 024 entries from which the chain's pooling hands a row to a workgroup), a bare
    path a - b - c and isolated nodes; 1 500 candidates.  The first 750 are the reference batch R, the last 750 the served list C.
    From the ORACLE's counts: every class of entry and of row the frozen arithmetic distinguishes is populated — no test here
    passes on empty sets."""
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
    assert e.shape[1] == B
    adj = to_product(oadj, DEV)
    adj2 = product_adj2(adj)
    ocn1, ocn2 = O.adjoverlap(oadj, oadj, e), O.adjoverlap(oadj, oadj2, e)
    # the classes, from the oracle: cn1 entries of C on columns whose cn1 count in R is 0 / 1 / >= 2 (cn5: w1 = 0 below two,
    # cn7: the fill), cn2 entries of C on columns R never hit in cn2 (cn5: inv2 = 0), rows of C with cn1 / cn2 / no entries, hub sources
    in_c1, in_c2 = ocn1.row >= N_REF, ocn2.row >= N_REF
    r1 = torch.bincount(ocn1.col[~in_c1], minlength=n)
    r2 = torch.bincount(ocn2.col[~in_c2], minlength=n)
    k1 = r1[ocn1.col[in_c1]]
    classes = dict(cn1_on_0=int((k1 == 0).sum()), cn1_on_1=int((k1 == 1).sum()), cn1_on_2plus=int((k1 >= 2).sum()),
                   cn2_unseen=int((r2[ocn2.col[in_c2]] == 0).sum()))
    c1, c2 = rowcount(ocn1)[N_REF:], rowcount(ocn2)[N_REF:]
    rows = dict(with_cn1=int((c1 > 0).sum()), with_cn2=int((c2 > 0).sum()), with_neither=int(((c1 == 0) & (c2 == 0)).sum()),
                hub_source=int((e[0, N_REF:] == hub).sum()))
    print(f"frozen fixture: entries {classes}, rows {rows}")
    assert all(v >= 100 for v in classes.values()), classes
    assert rows["with_cn1"] >= 100 and rows["with_cn2"] >= 100 and rows["with_neither"] >= 20 and rows["hub_source"] >= 20, rows
    assert int(rowcount(oadj)[hub]) > 1024
    return SimpleNamespace(n=n, B=B, oadj=oadj, oadj2=oadj2, e=e, adj=adj, adj2=adj2, ocn1=ocn1, ocn2=ocn2, hub=hub,
                           eR=e[:, :N_REF].contiguous().to(DEV), eC=e[:, N_REF:].contiguous().to(DEV))


def random_table(n, seed):
    """Normal fp32 [n, 4] with a third of the w1, of the t and of the inv2 zeroed independently (the fetch rule: an entry is
    gathered exactly when wa != 0 or wb != 0); the fourth column is the table's zero."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, 4, generator=g)
    for q in range(3):
        w[torch.rand(n, generator=g) < 1 / 3, q] = 0.0
    w[:, 3] = 0.0
    assert all(50 < int((w[:, q] == 0).sum()) < n - 50 for q in range(3))
    return w.to(DEV)


_chain = {}


def chain_reference(c, H):
    """``ops.cn_flags`` -> ``ops.cn_gather(weights=table)`` of the whole candidate list, once per width."""
    from ocn_amd.utils import CNState
    if H not in _chain:
        torch.manual_seed(100 + H)
        x = torch.randn(c.n, H).to(DEV)
        w = random_table(c.n, 7)
        st = CNState(c.adj, c.adj, c.adj2, c.e.to(DEV))
        x1, x2, xij = st.gather(w, x)
        st.check_status()
        _chain[H] = (x, w, bits(x1), bits(x2), bits(xij))
    return _chain[H]


@pytest.mark.parametrize("order", [False, True], ids=["batch_order", "permuted"])
@pytest.mark.parametrize("form", ["bits", "csr", "bits1_csr2"])
@pytest.mark.parametrize("H", WIDTHS)
def test_pool_frozen_bit_equal_to_the_chain(hubs, H, form, order):
    """``ops.cn_pool_frozen`` with a random table against flags -> pooling with the same table: xcn1, xcn2 and xij bit for bit
    (zero signs included), the counts equal to the oracle's row counts whatever the weights — hub rows, isolated nodes, T1 / T2
    as bit rows and as CSR, with and without a processing order."""
    from ocn_amd import ops
    c = hubs
    x, w, r1, r2, rij = chain_reference(c, H)
    adj, adj2 = c.adj, c.adj2
    bm1 = ops.bitrows_from_csr(adj._rowptr, adj._col, c.n) if form != "csr" else None
    bm2 = ops.bitrows_from_csr(adj2._rowptr, adj2._col, c.n) if form == "bits" else None
    t1 = (adj._rowptr, adj._col) if form != "bits" else None
    t2 = (adj2._rowptr, adj2._col) if form != "bits" else None
    ed = c.e.to(DEV)
    perm = torch.randperm(c.B, generator=torch.Generator().manual_seed(3)).to(DEV) if order else None
    x1, x2, xij, n1, n2 = ops.cn_pool_frozen(adj._rowptr, adj._col, t1, t2, ed[0].contiguous(), ed[1].contiguous(), x, w,
                                             t1_bitmap=bm1, t2_bitmap=bm2, order=perm)
    assert n1.dtype == torch.int32 and torch.equal(n1.cpu().long(), rowcount(c.ocn1)) and torch.equal(n2.cpu().long(), rowcount(c.ocn2))
    assert torch.equal(bits(x1), r1) and torch.equal(bits(x2), r2) and torch.equal(bits(xij), rij)
    assert bool(x1.any()) and bool(x2.any())


@pytest.mark.parametrize("H", WIDTHS)
def test_pool_frozen_with_the_unit_table_is_cn8(hubs, H):
    """The unit table {1, 0, 1, 0} and a finite x: bit for bit ``ops.cn8_pool``."""
    from ocn_amd import ops
    c = hubs
    adj, adj2 = c.adj, c.adj2
    x = torch.randn(c.n, H, generator=torch.Generator().manual_seed(200 + H)).to(DEV)
    ed = c.e.to(DEV)
    src, dst = ed[0].contiguous(), ed[1].contiguous()
    t1, t2 = (adj._rowptr, adj._col), (adj2._rowptr, adj2._col)
    want = ops.cn8_pool(adj._rowptr, adj._col, t1, t2, src, dst, x)
    got = ops.cn_pool_frozen(adj._rowptr, adj._col, t1, t2, src, dst, x, ops.unit_weights(c.n, DEV))
    for a, b in zip(got[:3], want[:3]):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(got[3], want[3]) and torch.equal(got[4], want[4]) and int(got[3].sum()) > 0 and int(got[4].sum()) > 0


@pytest.mark.parametrize("H", [16, 256, 512])
def test_pool_frozen_complete_bipartite_by_hand(hiplib, H):
    """K_{a,b} needs no oracle.  Two nodes of one side share the whole other side as cn1 and have no cn2 entry (A² links a node
    to its own side); a cross pair has no cn1 entry and the whole of the target's side as cn2; a pair with an isolated node has
    no member at all and gets zero rows.  Power-of-two weights and small integer embeddings: every product and sum is exact, so
    the expected rows are plain fp64 sums of  w1[k] x[k],  -t[k] inv2[k] x[k]  (cn1-only entries) and  inv2[k] x[k]  (cn2-only)."""
    from ocn_amd import ops
    from ocn_amd.sparse import SparseTensor
    a, b = 70, 9                                                       # (70 > 64: the left side's rows span two rounds of a wave)
    n = a + b + 2                                                      # ... and two isolated nodes
    left, right = torch.arange(a), torch.arange(a, a + b)
    ei = torch.stack([left.repeat_interleave(b), right.repeat(a)])
    ei = torch.cat([ei, ei.flip(0)], dim=1)
    adj = SparseTensor.from_edge_index(ei.to(DEV), sparse_sizes=(n, n))
    adj2 = product_adj2(adj)
    g = torch.Generator().manual_seed(H)
    x = torch.randint(-8, 9, (n, H), generator=g).double()
    pw = lambda: torch.pow(2.0, torch.randint(-2, 3, (n,), generator=g).double())
    w1, t, inv2 = pw(), pw(), pw()
    w1[::5] = 0.0; t[1::4] = 0.0; inv2[2::7] = 0.0                     # (some entries are not fetched, some add to one side only)
    w = torch.stack([w1, t, inv2, torch.zeros(n, dtype=torch.double)], dim=1)
    pairs = torch.tensor([[0, a, 0, a + 1, 5, n - 1], [1, a + 1, a, 4, n - 1, n - 2]])
    #         L-L          R-R         L-R (cross)  R-L (cross)  L-iso  iso-iso
    s1 = lambda side: (w1[side, None] * x[side]).sum(0)
    s12 = lambda side: (-(t[side] * inv2[side])[:, None] * x[side]).sum(0)
    s2 = lambda side: (inv2[side, None] * x[side]).sum(0)
    z = torch.zeros(H, dtype=torch.double)
    want1 = torch.stack([s1(right), s1(left), z, z, z, z]).float()
    want2 = torch.stack([s12(right), s12(left), s2(right), s2(left), z, z]).float()
    cnt1, cnt2 = [b, a, 0, 0, 0, 0], [0, 0, b, a, 0, 0]
    e = pairs.to(DEV)
    xd, wd = x.float().to(DEV), w.float().to(DEV)
    for use_bits in (False, True):
        bm1 = ops.bitrows_from_csr(adj._rowptr, adj._col, n) if use_bits else None
        bm2 = ops.bitrows_from_csr(adj2._rowptr, adj2._col, n) if use_bits else None
        x1, x2, xij, n1, n2 = ops.cn_pool_frozen(adj._rowptr, adj._col, (adj._rowptr, adj._col), (adj2._rowptr, adj2._col),
                                                 e[0].contiguous(), e[1].contiguous(), xd, wd, t1_bitmap=bm1, t2_bitmap=bm2)
        assert n1.tolist() == cnt1 and n2.tolist() == cnt2
        assert torch.equal(x1.cpu(), want1) and torch.equal(x2.cpu(), want2)
        assert torch.equal(xij.cpu(), (x[pairs[0]] * x[pairs[1]]).float())
        assert bool(want1[:2].any()) and bool(want2[:4].any()) and not bool(x1[2:].any()) and not bool(x2[4:].any())


def make_predictor(kind, val, H):
    """A seeded cn5 (``val`` = the stored innerprod) or cn7 (``val`` = args.sum) in eval mode on the device, and its args."""
    from ocn_amd.model import predictor_dict
    torch.manual_seed(31)
    pred = predictor_dict[kind](H, H, 1, 3, 0.0, 0.0, True).eval()
    with torch.no_grad():
        pred.alpha.copy_(torch.tensor([0.4, -0.3, 0.1]))
        if kind == "cn5":
            pred.innerprod.fill_(val)
    return pred.to(DEV), (SimpleNamespace(sum=val) if kind == "cn7" else None)


def call(pred, x, adj, handles, e, args):
    return pred(x, adj, *handles, e, args) if args is not None else pred(x, adj, *handles, e)


class PoolSpy:
    """Records what every batch hands to the heads — the pooled rows of its batch state."""

    def __init__(self, pred, monkeypatch):
        self.seen, heads = [], pred._heads
        self.heads = heads

        def spy(x_, xcn1, xcn2, xij, cls=None):
            assert cls is None                                          # (batch-order rows: below ops.skip_zero_min_batch)
            self.seen.append((xcn1.clone(), xcn2.clone(), xij.clone()))
            return heads(x_, xcn1, xcn2, xij, cls)
        monkeypatch.setattr(pred, "_heads", spy)

    def take(self):
        out = [torch.cat([t[q] for t in self.seen]) for q in range(3)]
        self.seen.clear()
        return out


@pytest.mark.parametrize("kind,val,H", [("cn5", 0.0, 64), ("cn5", 0.37, 256), ("cn7", 0.0, 64), ("cn7", 0.5, 32)])
def test_frozen_on_its_reference_batch_is_the_unfrozen_predictor(hubs, monkeypatch, kind, val, H):
    """``fc = freeze_columns(.., R)``: the frozen predictor called on R pools bit-equal to the unfrozen predictor on R (which the
    parity tests pin to the oracle) and scores within the suite's bar — through the one pass, through the chain and, frozen
    with ``adj2=None``, on walk handles.  The table is a clone: the batches in between reuse the scratch it was formed in."""
    from ocn_amd import ops
    from ocn_amd.frozen import freeze_columns
    from ocn_amd.utils import adjoverlap, get_cn1_cn2
    c = hubs
    pred, args = make_predictor(kind, val, H)
    x = torch.randn(c.n, H, generator=torch.Generator().manual_seed(40 + H)).to(DEV)
    spy = PoolSpy(pred, monkeypatch)
    pattern = lambda e: (adjoverlap(c.adj, c.adj, e), adjoverlap(c.adj, c.adj2, e))
    walk = lambda e: get_cn1_cn2(c.adj, e)
    with torch.no_grad():
        for route, handles, adj2 in (("pattern", pattern, c.adj2), ("walk", walk, None)):
            want = call(pred, x, c.adj, handles(c.eR), c.eR, args)
            want_pools = spy.take()
            assert bool(want_pools[0].any()) and bool(want_pools[1].any())
            fc = freeze_columns(pred, c.adj, adj2, c.eR.t().contiguous(), args)
            assert (fc.kind, fc.n_cols, fc.valued, fc.ref_size) == (kind, c.n, route == "walk", N_REF)
            assert fc.weights.shape == (c.n, 4) and fc.weights.dtype == torch.float32 and fc.weights.device == x.device
            assert (fc.innerprod, fc.sum_fill) == ((pytest.approx(val), None) if kind == "cn5" else (None, val))      # (innerprod: fp32)
            call(pred, x, c.adj, pattern(c.eC), c.eC, args)              # another batch runs over the scratch the table was formed in
            spy.take()
            assert pred.set_frozen_columns(fc, args) is None
            for fused in ((True, False) if route == "pattern" else (True,)):      # (walk handles take the chain either way)
                monkeypatch.setattr(ops, "frozen_fused_eval", fused)
                got = call(pred, x, c.adj, handles(c.eR), c.eR, None if kind == "cn7" and fused else args)     # (a frozen cn7 needs no args)
                got_pools = spy.take()
                err = (got - want).abs().max().item()
                print(f"frozen {kind} {val} H={H} {route} fused={fused}: max|score - unfrozen| = {err:.3e}, max|score| = {want.abs().max().item():.3e}")
                for a, b in zip(got_pools, want_pools):
                    assert torch.equal(bits(a), bits(b)), (route, fused)
                assert got.shape == (N_REF, 1) and close(got, want)
            assert pred.set_frozen_columns(None) is fc
    pred.check_errors()


@pytest.mark.parametrize("fused", [False, True], ids=["chain", "one_pass"])
@pytest.mark.parametrize("kind,val", [("cn5", 0.37), ("cn7", 0.5)])
def test_frozen_scores_do_not_depend_on_the_batch(hubs, monkeypatch, kind, val, fused):
    """The served list C through ``score_edges`` at batch sizes 750, 64 and 7, reversed, and mixed into 300 foreign candidates:
    per candidate the pooled rows are bit-equal and the scores agree within the suite's bar.  Control: unfrozen, batch sizes 750
    and 64 move some candidate's score by more than 1e-3.  A captured loop (``ops.graph_loops``) replays the eager loop's bits."""
    from ocn_amd import ops
    from ocn_amd.frozen import freeze_columns
    from ocn_amd.pipeline import score_edges
    c = hubs
    H = 64
    pred, args = make_predictor(kind, val, H)
    x = torch.randn(c.n, H, generator=torch.Generator().manual_seed(9)).to(DEV)
    edges = c.eC.t().contiguous()
    n = edges.shape[0]
    monkeypatch.setattr(ops, "frozen_fused_eval", fused)
    loose = {bs: score_edges(pred, x, c.adj, c.adj2, edges, bs, args) for bs in (n, 64)}
    moved = (loose[n] - loose[64]).abs().max().item()
    print(f"unfrozen {kind}: batch sizes {n} and 64 move a score by up to {moved:.3e}")
    assert moved > 1e-3
    pred.set_frozen_columns(freeze_columns(pred, c.adj, c.adj2, c.eR.t().contiguous(), args), args)
    spy = PoolSpy(pred, monkeypatch)
    base = score_edges(pred, x, c.adj, c.adj2, edges, n, args)
    base_pools = spy.take()
    assert len(base_pools[0]) == n and bool(base_pools[0].any()) and bool(base_pools[1].any())
    g = torch.Generator().manual_seed(2)
    mix = torch.cat([edges, c.eR.t()[:300]])[torch.randperm(n + 300, generator=g).to(DEV)].contiguous()
    where = torch.full((c.n * c.n,), -1, dtype=torch.int64, device=DEV)
    key = mix[:, 0] * c.n + mix[:, 1]
    where[key] = torch.arange(n + 300, device=DEV)                      # (a pair that occurs twice has one score: any of its places)
    pick_mix = where[edges[:, 0] * c.n + edges[:, 1]]
    assert int(pick_mix.min()) >= 0
    rev = torch.arange(n - 1, -1, -1, device=DEV)
    runs = [("bs 64", edges, 64, None), ("bs 7", edges, 7, None), ("reversed", edges.flip(0).contiguous(), 64, rev),
            ("mixed", mix, 128, pick_mix)]
    for name, ed, bs, pick in runs:
        s = score_edges(pred, x, c.adj, c.adj2, ed, bs, None if kind == "cn7" else args)
        pools = spy.take()
        if pick is not None:
            s, pools = s[pick], [p[pick] for p in pools]
        err = (s - base).abs().max().item()
        print(f"frozen {kind} {'one pass' if fused else 'chain'} {name}: max|score - base| = {err:.3e}, bit-equal scores: {torch.equal(s, base)}")
        for a, b in zip(pools, base_pools):
            assert torch.equal(bits(a), bits(b)), name
        assert close(s, base), name
    # captured phases (ops.graph_loops: 50 batches over the loop's scratch sets) replay what the eager loop computes
    monkeypatch.setattr(pred, "_heads", spy.heads)
    monkeypatch.setattr(ops, "graph_loops", True)
    replayed = score_edges(pred, x, c.adj, c.adj2, edges, 15, args)
    monkeypatch.setattr(ops, "graph_loops", False)
    assert torch.equal(replayed, score_edges(pred, x, c.adj, c.adj2, edges, 15, args)) and close(replayed, base)


@pytest.mark.parametrize("fused", [False, True], ids=["chain", "one_pass"])
def test_frozen_recommendation_does_not_depend_on_the_other_sources(hubs, monkeypatch, fused):
    """``recommend_links`` for 40 sources and for every second one of them at another ``batch_size``: the shared sources' score
    rows agree within the suite's bar (unfrozen they are other numbers: the contract sentence of ``recommend_links``)."""
    from ocn_amd import ops
    from ocn_amd.frozen import freeze_columns
    from ocn_amd.recommend import recommend_links
    c = hubs
    H, k = 64, 10
    pred, args = make_predictor("cn5", 0.37, H)
    x = torch.randn(c.n, H, generator=torch.Generator().manual_seed(10)).to(DEV)
    sources = torch.cat([torch.tensor([c.hub]), torch.randperm(2980, generator=torch.Generator().manual_seed(4))[:39]]).to(DEV)
    monkeypatch.setattr(ops, "frozen_fused_eval", fused)
    pred.set_frozen_columns(freeze_columns(pred, c.adj, c.adj2, c.eR.t().contiguous()))
    dst_all, s_all = recommend_links(pred, x, c.adj, c.adj2, sources, k, 4096)
    dst_half, s_half = recommend_links(pred, x, c.adj, c.adj2, sources[::2].contiguous(), k, 1000)
    assert s_all.shape == (40, k) and s_half.shape == (20, k) and bool(torch.isfinite(s_all).any())
    print(f"frozen recommend {'one pass' if fused else 'chain'}: max|score - score| = {(s_all[::2] - s_half).abs().nan_to_num(0).max().item():.3e}, "
          f"same dst: {torch.equal(dst_all[::2], dst_half)}")
    assert close(s_all[::2], s_half)
    assert torch.equal(torch.isfinite(s_all[::2]), torch.isfinite(s_half))
    pred.set_frozen_columns(None)
    _, u_all = recommend_links(pred, x, c.adj, c.adj2, sources, k, 4096)
    _, u_half = recommend_links(pred, x, c.adj, c.adj2, sources[::2].contiguous(), k, 1000)
    assert not close(u_all[::2], u_half)


def test_frozen_refusals_on_the_device(hubs, monkeypatch):
    """What is refused with tensors on the device, and that removing the table restores the unfrozen scores exactly."""
    from ocn_amd import ops
    from ocn_amd.frozen import freeze_columns
    from ocn_amd.model import predictor_dict
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.utils import adjoverlap, get_cn1_cn2
    c = hubs
    H = 32
    pred, _ = make_predictor("cn5", 0.37, H)
    x = torch.randn(c.n, H, generator=torch.Generator().manual_seed(12)).to(DEV)
    ref = c.eR.t().contiguous()
    pattern = lambda: (adjoverlap(c.adj, c.adj, c.eC), adjoverlap(c.adj, c.adj2, c.eC))
    with torch.no_grad():
        before = pred(x, c.adj, *pattern(), c.eC)
    fc = freeze_columns(pred, c.adj, c.adj2, ref)
    fcw = freeze_columns(pred, c.adj, None, ref)
    assert fcw.valued and not fc.valued
    # freezing
    with pytest.raises(ValueError, match="batch-independent"):
        freeze_columns(predictor_dict["cn8"](H, H, 1, 3, 0.0).to(DEV).eval(), c.adj, c.adj2, ref)
    with pytest.raises(NotImplementedError):
        freeze_columns(predictor_dict["cn6"](H, H, 1, 3, 0.0).to(DEV).eval(), c.adj, c.adj2, ref)
    pred.set_edge_sharding(None, True)
    with pytest.raises(RuntimeError, match="sharded"):
        freeze_columns(pred, c.adj, c.adj2, ref)
    pred.set_edge_sharding(None, False)
    pred.train()
    with pytest.raises(RuntimeError, match="eval"):
        freeze_columns(pred, c.adj, c.adj2, ref)
    pred.eval()
    with pytest.raises(ValueError, match="ONE batch"):
        freeze_columns(pred, c.adj, c.adj2, ref[:0])
    with pytest.raises(ValueError, match="args"):
        freeze_columns(predictor_dict["cn7"](H, H, 1, 3, 0.0).to(DEV).eval(), c.adj, c.adj2, ref)
    # installing
    with pytest.raises(ValueError, match="cn5 table"):
        predictor_dict["cn7"](H, H, 1, 3, 0.0).to(DEV).eval().set_frozen_columns(fc)
    with pytest.raises(ValueError, match="lives on"):
        pred.set_frozen_columns(fc.to("cpu"))
    other = predictor_dict["cn5"](H, H, 1, 3, 0.0).to(DEV).eval()      # (innerprod 0, the table baked 0.37)
    with pytest.raises(ValueError, match="innerprod"):
        other.set_frozen_columns(fc)
    assert pred._frozen is None and other._frozen is None
    # scoring
    small = SparseTensor.from_edge_index(torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]], device=DEV), sparse_sizes=(40, 40))
    es = torch.tensor([[0], [2]], device=DEV)
    for fused in (False, True):
        monkeypatch.setattr(ops, "frozen_fused_eval", fused)
        with torch.no_grad():
            pred.set_frozen_columns(fc)
            with pytest.raises(ValueError, match="columns"):            # a table of 3 000 columns, a graph of 40
                pred(x[:40].contiguous(), small, adjoverlap(small, small, es), adjoverlap(small, small, es), es)
            with pytest.raises(ValueError, match="walk"):               # a pattern table on walk handles
                pred(x, c.adj, *get_cn1_cn2(c.adj, c.eC), c.eC)
            pred.set_frozen_columns(fcw)
            with pytest.raises(ValueError, match="walk"):               # ... and the reverse
                pred(x, c.adj, *pattern(), c.eC)
            pred.set_frozen_columns(fc)
        with pytest.raises(RuntimeError, match="eval path"):            # autograd on
            pred(x, c.adj, *pattern(), c.eC)
        pred.train()
        with torch.no_grad(), pytest.raises(RuntimeError, match="eval path"):
            pred(x, c.adj, *pattern(), c.eC)
        pred.eval()
        assert pred.n == 0 and pred.innerprod.item() == pytest.approx(0.37)      # (the refused training call updated nothing)
        with torch.no_grad():
            frozen = pred(x, c.adj, *pattern(), c.eC)
            assert not torch.equal(frozen, before)
            assert pred.set_frozen_columns(None) is fc
            assert torch.equal(pred(x, c.adj, *pattern(), c.eC), before)
    pred.check_errors()
