"""Pooling from a bf16 / f16 embedding table (cn_pool_h16.hip, ocn_cn_gather_h16) against the fp32 entry on the same table
widened: both widenings are exact and the sums are the fp32 entry's — same operands, same order, separately rounded multiply
and add — so every comparison is of raw bits (``view(torch.int32)``), never of values within a tolerance.  Output buffers
are pre-filled with NaN, the way tests/test_pool_pairs_gpu.py does, so that rows a launch leaves unwritten compare too.

One rule about those rows.  With class-major output rows the heads never read the xcn1 row of a candidate without cn1
entries, nor the xcn2 row of one without any entry, and the half entry does not write them (``_never_read`` asserts that it
left the NaN).  The fp32 entry leaves them too in its packed and pair forms, but its wave and hub-row forms (narrow widths
at small batches, source rows beyond 1 024 entries) write zeros there.  On exactly those rows the comparison is therefore
"the half entry wrote nothing, the fp32 entry left NaN or wrote +0"; on every other row, and on all of x_i * x_j, it is
bit equality."""
from types import SimpleNamespace

import pytest
import torch

from oracle import ocn_oracle as O
from tests.helpers import batch, make_graph, product_adj2, to_product
from tests.test_lane_group_gpu import KINDS, LEAVES, LENGTHS, N as N_STAR, matrix, target_rows
from tests.test_pool_pairs_gpu import N_REAL, _edges, _graph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
WIDTHS = (16, 32, 64, 128, 256, 512)
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
WEIGHTS = {"cn5_fresh": lambda st: st.weights_cn5(torch.zeros(1, device=DEV)),
           "cn5_trained": lambda st: st.weights_cn5(torch.tensor([0.37], device=DEV)),
           "cn7": lambda st: st.weights_cn7(0.7)}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _table(n, H, dt, seed):
    """A half table whose values spread over several binades (products and sums round), as made by ``embedding_table``."""
    from ocn_amd.pipeline import embedding_table
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(n, H, generator=g) * torch.exp2(torch.randint(-6, 7, (n, 1), generator=g).float())
    t = embedding_table(h.to(DEV), {torch.bfloat16: "bf16", torch.float16: "f16"}[dt])
    assert t.dtype == dt and not torch.equal(t.float(), h.to(DEV))           # (the rounding did something)
    return t


def _pooled(st, w, h, out_row=None):
    """st.gather into a NaN-filled buffer of its own."""
    from ocn_amd import ops
    ws = {}
    ops.buf(ws, "pooled", (3, st.B, h.shape[1]), torch.float32, DEV).fill_(NAN)
    st.ws = ws
    out = [o.clone() for o in st.gather(w, h, out_row=out_row)]
    torch.cuda.synchronize()
    return out


def _never_read(st, out_row):
    """Output rows the class-major heads never read: (of xcn1, of xcn2) as bool [B] over OUTPUT rows; all False in batch order."""
    none = torch.zeros(st.B, dtype=torch.bool, device=DEV)
    if out_row is None or st.cnt1 is None:
        return none, none
    no1, no_any = none.clone(), none.clone()
    no1[out_row] = st.cnt1 == 0
    no_any[out_row] = (st.cnt1 == 0) & (st.cnt2 == 0)
    return no1, no_any


def _assert_same(got, ref, st, out_row, what):
    """(xcn1, xcn2, xij) of the half entry against those of the fp32 entry: see the module docstring."""
    skip1, skip2 = _never_read(st, out_row)
    assert torch.equal(_bits(got[2]), _bits(ref[2])), what
    for g, r, skip in ((got[0], ref[0], skip1), (got[1], ref[1], skip2)):
        assert torch.equal(_bits(g[~skip]), _bits(r[~skip])), what
        assert bool(torch.isnan(g[skip]).all()), what                                       # left alone
        assert bool((torch.isnan(r[skip]).all(1) | (_bits(r[skip]) == 0).all(1)).all()), what
    assert not bool(torch.isnan(got[2]).any()), what


def _state(adj, t2, e, monkeypatch, sort):
    from ocn_amd import ops
    from ocn_amd.utils import CNState
    monkeypatch.setattr(ops, "sort_edges_min_batch", 0 if sort else 1 << 40)
    return CNState(adj, adj, t2, e)


# ---- 1. round and group edges -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def star(hiplib):
    """The star of tests/test_lane_group_gpu.py: source s_L has the leaves 0 .. L - 1 as its row, one target per (L, kind) whose
    rows of T1 = A and T2 pick the members.  43 candidates — the 40 and three repeats: no multiple of the 16, 8, 4 or 2
    candidates a wave holds at H = 16 .. 128."""
    a_rows, t2_rows, cand = {}, {}, []
    for q, L in enumerate(LENGTHS):
        s = LEAVES + q
        a_rows[s] = list(range(L))
        for kq, kind in enumerate(KINDS):
            t = LEAVES + len(LENGTHS) + 4 * q + kq
            r1, r2, _ = (list(r) for r in target_rows(kind, L))
            a_rows[t], t2_rows[t] = r1, r2
            cand.append((s, t))
    for r, cols in list(a_rows.items()):
        for c in cols:
            a_rows.setdefault(c, []).append(r)
    perm = torch.randperm(len(cand), generator=torch.Generator().manual_seed(5)).tolist()
    cand = [cand[p] for p in perm] + [cand[7], cand[21], cand[33]]
    assert len(cand) == 43
    e = torch.tensor(cand).t().contiguous().to(DEV)
    return SimpleNamespace(adj=matrix(a_rows), t2=matrix(t2_rows), e=e, B=len(cand))


@pytest.mark.parametrize("dt", DTYPES.values(), ids=DTYPES.keys())
@pytest.mark.parametrize("H", WIDTHS)
def test_star_every_width(star, monkeypatch, H, dt):
    from ocn_amd import ops
    t = _table(N_STAR, H, dt, 100 + H)
    tf = t.float()
    seen_skip = False
    for sort in (False, True):
        for kind, weights in WEIGHTS.items():
            for class_major in (False, True):
                st = _state(star.adj, star.t2, star.e, monkeypatch, sort)
                st.check_status()
                w = weights(st)
                out_row = ops.class_order(st.cnt1, st.cnt2, st.order)[1] if class_major else None
                got, ref = _pooled(st, w, t, out_row), _pooled(st, w, tf, out_row)
                _assert_same(got, ref, st, out_row, (sort, kind, class_major))
                assert bool((got[0] != 0).any()) and bool((got[1] != 0).any())
                seen_skip |= bool(_never_read(st, out_row)[1].any())
    assert seen_skip                                     # (some rows were left alone, and the check above looked at them)


# ---- 2. hub rows ------------------------------------------------------------------------------------------------------------------
_TAB = {}


def _hub_table(H, dt):
    if (H, dt) not in _TAB:
        _TAB[(H, dt)] = _table(N_REAL, H, dt, 7 * H)
    return _TAB[(H, dt)]


@pytest.mark.parametrize("dt", DTYPES.values(), ids=DTYPES.keys())
@pytest.mark.parametrize("H", [32, 256])
@pytest.mark.parametrize("B", [1, 7, 64, 128])
def test_hub_rows(hiplib, monkeypatch, B, H, dt):
    """Rows of 1 100, 1 030 and 700 entries, a source without neighbours, runs of one source; H = 32 is where the fp32 entry
    takes its narrow hub forms (a wave per hub row, a 1 024-thread workgroup at small batches)."""
    from ocn_amd import ops
    gr = _graph()
    e = _edges(gr, B, 100 + B).to(DEV)
    t = _hub_table(H, dt)
    tf = t.float()
    for sort in (True, False):
        for kind, weights in WEIGHTS.items():
            for class_major in (False, True):
                st = _state(gr.adj, gr.adj2, e, monkeypatch, sort)
                w = weights(st)
                out_row = ops.class_order(st.cnt1, st.cnt2, st.order)[1] if class_major else None
                got, ref = _pooled(st, w, t, out_row), _pooled(st, w, tf, out_row)
                _assert_same(got, ref, st, out_row, (sort, kind, class_major))
    assert int(st.adj.max_rowcount()) > 1024


@pytest.mark.parametrize("dt", DTYPES.values(), ids=DTYPES.keys())
@pytest.mark.parametrize("H", [32, 256])
def test_hub_rows_against_the_oracle(hiplib, monkeypatch, H, dt):
    """innerprod = 0, B = 128: the CPU oracle's pooling of the widened table, bit for bit — the strictly sequential
    ascending-column sum, hub rows included — and x_i * x_j from the widened endpoint rows."""
    gr = _graph()
    B = 128
    e = _edges(gr, B, 77)
    if "cn" not in _TAB:
        _TAB["cn"] = (O.adjoverlap(gr.oadj, gr.oadj, e), O.adjoverlap(gr.oadj, O.adj2_sparse(gr.oadj), e))
    t = _hub_table(H, dt)
    tf = t.float().cpu()
    ref1, ref2, _ = O.cn5_pool(tf, *_TAB["cn"], torch.tensor([0.0]))
    assert sum(int(gr.oadj.rowcount()[int(s)]) > 1024 for s in e[0]) >= 3
    for sort in (True, False):
        st = _state(gr.adj, gr.adj2, e.to(DEV), monkeypatch, sort)
        x1, x2, xij = _pooled(st, st.weights_cn5(torch.zeros(1, device=DEV)), t)
        assert torch.equal(x1.cpu(), ref1) and torch.equal(x2.cpu(), ref2)
        assert torch.equal(xij.cpu(), tf[e[0]] * tf[e[1]])


# ---- 3. walk route ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES.values(), ids=DTYPES.keys())
@pytest.mark.parametrize("H", [32, 64])
def test_walk_route(hiplib, H, dt):
    """``get_cn1_cn2`` handles: cn2 carries walk counts (a valued ``wc``)."""
    from ocn_amd.utils import fuse, get_cn1_cn2
    gr = _graph()
    e = _edges(gr, 64, 31).to(DEV)
    t = _hub_table(H, dt)
    for ip in (0.0, 0.37):
        st = fuse(*get_cn1_cn2(gr.adj, e), e, None, adj=gr.adj)
        assert st.walk and st.wc is not None
        w = st.weights_cn5(torch.tensor([ip], device=DEV))
        got, ref = _pooled(st, w, t), _pooled(st, w, t.float())
        _assert_same(got, ref, st, None, ip)
        assert bool((got[1] != 0).any())


# ---- 4. values --------------------------------------------------------------------------------------------------------------------
# +0, -0, the smallest subnormal, the smallest normal, the largest finite value, their negatives, the largest subnormal and a few
# ordinary numbers, as bit patterns
SPECIAL = {torch.bfloat16: [0x0000, 0x8000, 0x0001, 0x0080, 0x7F7F, 0x8001, 0x8080, 0xFF7F, 0x007F, 0x3F80, 0xBFC0, 0x4049,
                            0x0002, 0x3EAB, 0x7F00, 0x00FF],
           torch.float16: [0x0000, 0x8000, 0x0001, 0x0400, 0x7BFF, 0x8001, 0x8400, 0xFBFF, 0x03FF, 0x3C00, 0xBE00, 0x4248,
                           0x0002, 0x3555, 0x7800, 0x07FF]}


@pytest.mark.parametrize("dt", DTYPES.values(), ids=DTYPES.keys())
@pytest.mark.parametrize("H", [16, 64, 256])
def test_special_values_are_widened_exactly(hiplib, H, dt):
    """One candidate (0, 1) with the common neighbours 2, 3, 4 (and node 5, a neighbour that is none); every row is a rotation
    of SPECIAL, so each feature adds another triple; the weights are no powers of two.  A conversion that flushed subnormals
    or dropped low bits would differ from the fp32 entry, which reads the table widened by torch."""
    from ocn_amd import ops
    pat = torch.tensor(SPECIAL[dt], dtype=torch.int32)
    rows = torch.stack([torch.roll(pat, 3 * r).repeat(H // 16) for r in range(6)])
    t = ((rows + 0x8000) % 0x10000 - 0x8000).to(torch.int16).view(dt).to(DEV)      # (the same 16 bits, as a signed value)
    tf = t.float()
    assert bool(torch.isfinite(tf).all()) and bool((tf == 0).any()) and bool((tf.abs() > 1e30).any() or dt == torch.float16)
    assert float(tf[tf != 0].abs().min()) == (2.0 ** -133 if dt == torch.bfloat16 else 2.0 ** -24)
    rowptr = torch.tensor([0, 4, 4, 4, 4, 4, 4], dtype=torch.int64, device=DEV)
    col = torch.tensor([2, 3, 4, 5], dtype=torch.int32, device=DEV)
    src, dst = torch.tensor([0], device=DEV), torch.tensor([1], device=DEV)
    off = torch.tensor([0, 4], device=DEV)
    flags = torch.tensor([3, 1, 2, 0], dtype=torch.uint8, device=DEV)
    w = torch.tensor([[0.3, 0.7, 0.11, 0.0]], device=DEV).repeat(6, 1) * torch.tensor([1.0, 1.1, 0.9, 1.3, 0.77, 1.0], device=DEV)[:, None]

    def pool(h):
        ws = {}
        ops.buf(ws, "pooled", (3, 1, H), torch.float32, DEV).fill_(NAN)
        return [o.clone() for o in ops.cn_gather(rowptr, col, src, dst, off, flags, None, w.contiguous(), h, max_row_len=4, wsd=ws)]

    got, ref = pool(t), pool(tf)
    torch.cuda.synchronize()
    for g, r in zip(got, ref):
        assert torch.equal(_bits(g), _bits(r))
        assert bool((g != 0).any()) and not bool(torch.isnan(g).any())
    assert torch.equal(_bits(got[2][0].cpu()), _bits(tf[0].cpu() * tf[1].cpu()))


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------
_E2E = {}


def _e2e():
    if not _E2E:
        n = 2000
        oadj = make_graph(n, 10, 100, 11, isolated=3)
        adj = to_product(oadj, DEV)
        edges = batch(oadj, 300, 12).t().contiguous().to(DEV)                 # three batches of 128: a ragged tail of 44
        _E2E.update(n=n, adj=adj, adj2=product_adj2(adj), edges=edges, args=SimpleNamespace(sum=0.7))
    return SimpleNamespace(**_E2E)


def _predictor(name, H, innerprod=0.0):
    from ocn_amd.model import predictor_dict
    torch.manual_seed(3)
    pred = predictor_dict[name](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()
    pred.innerprod.fill_(innerprod)
    return pred


@pytest.mark.parametrize("dt", DTYPES.values(), ids=DTYPES.keys())
@pytest.mark.parametrize("H", [64, 256])
def test_score_edges(hiplib, monkeypatch, H, dt):
    from ocn_amd import ops
    from ocn_amd.pipeline import score_edges, score_edges_walk
    c = _e2e()
    t = _table(c.n, H, dt, H)
    tf = t.float()
    for name, ip in (("cn5", 0.0), ("cn5", 0.37), ("cn7", 0.0), ("cn8", 0.0)):
        pred = _predictor(name, H, ip)
        a, b = score_edges(pred, t, c.adj, c.adj2, c.edges, 128, c.args), score_edges(pred, tf, c.adj, c.adj2, c.edges, 128, c.args)
        assert a.dtype == torch.float32 and a.shape == (300,) and torch.equal(a, b), (name, ip)
        assert bool(torch.isfinite(a).all()) and float(a.std()) > 0
    # cn8 with the one-pass form asked for: a half table takes the chain
    monkeypatch.setattr(ops, "cn8_fused_eval", True)
    assert torch.equal(score_edges(pred, t, c.adj, c.adj2, c.edges, 128, c.args), a)
    pred = _predictor("cn5", H, 0.37)
    assert torch.equal(score_edges_walk(pred, t, c.adj, c.edges, 128), score_edges_walk(pred, tf, c.adj, c.edges, 128))
    # a split that is whole batches (the loop may then see an empty last batch)
    whole = c.edges[:256].contiguous()
    assert torch.equal(score_edges(pred, t, c.adj, c.adj2, whole, 128), score_edges(pred, tf, c.adj, c.adj2, whole, 128))
    empty = score_edges(pred, t, c.adj, c.adj2, c.edges[:0], 128)
    assert empty.dtype == torch.float32 and empty.numel() == 0


@pytest.mark.parametrize("dt", DTYPES.values(), ids=DTYPES.keys())
@pytest.mark.parametrize("H", [64, 256])
def test_frozen_predictor(hiplib, monkeypatch, H, dt):
    from ocn_amd import ops
    from ocn_amd.frozen import freeze_columns
    from ocn_amd.pipeline import score_edges
    c = _e2e()
    t = _table(c.n, H, dt, H + 1)
    pred = _predictor("cn5", H, 0.37)
    pred.set_frozen_columns(freeze_columns(pred, c.adj, c.adj2, c.edges[:200].contiguous()))
    out = {}
    for fused in (False, True):
        monkeypatch.setattr(ops, "frozen_fused_eval", fused)
        out[fused] = score_edges(pred, t, c.adj, c.adj2, c.edges, 128)
        assert torch.equal(out[fused], score_edges(pred, t.float(), c.adj, c.adj2, c.edges, 128)), fused
    assert torch.equal(out[False], out[True])


@pytest.mark.parametrize("dt", DTYPES.values(), ids=DTYPES.keys())
@pytest.mark.parametrize("H", [64, 256])
def test_recommend_links(hiplib, H, dt):
    from ocn_amd.recommend import recommend_links
    c = _e2e()
    t = _table(c.n, H, dt, H + 2)
    pred = _predictor("cn5", H, 0.37)
    sources = torch.arange(0, 12, device=DEV)
    for kw in (dict(), dict(prefilter=("ra", 32)), dict(prefilter=("ra", 32, 0.5), hops=3)):
        for adj2 in (c.adj2, None):
            d1, s1 = recommend_links(pred, t, c.adj, adj2, sources, 10, 256, **kw)
            d2, s2 = recommend_links(pred, t.float(), c.adj, adj2, sources, 10, 256, **kw)
            assert torch.equal(d1, d2) and torch.equal(s1, s2) and s1.dtype == torch.float32, (kw, adj2 is None)
            assert int((d1 >= 0).sum()) > 50


def test_rank_links_and_a_captured_batch(hiplib):
    """``rank_links`` passes a half table through like ``recommend_links``; the launch is capturable (``GraphedScorer``)."""
    from ocn_amd.pipeline import GraphedScorer
    from ocn_amd.ranking import rank_links
    from ocn_amd.sparse import SparseTensor
    c = _e2e()
    H = 256
    t = _table(c.n, H, torch.bfloat16, 9)
    pred = _predictor("cn5", H, 0.37)
    sources = torch.arange(0, 40, device=DEV)
    truth = SparseTensor.from_edge_index(c.edges.t().contiguous(), sparse_sizes=(c.n, c.n)).to_symmetric()
    r1 = rank_links(pred, t, c.adj, c.adj2, sources, truth, 128, prefilter=("ra", 32))
    r2 = rank_links(pred, t.float(), c.adj, c.adj2, sources, truth, 128, prefilter=("ra", 32))
    assert torch.equal(r1.rank, r2.rank) and torch.equal(r1.retrieval_rank, r2.retrieval_rank)
    e = c.edges[:128].t().contiguous()
    a = GraphedScorer(pred, t, c.adj, c.adj2, 128)(e).clone()
    b = GraphedScorer(pred, t.float(), c.adj, c.adj2, 128)(e).clone()
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


# ---- 6. refusals, on device tensors -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES.values(), ids=DTYPES.keys())
def test_refusals_on_the_device(hiplib, dt):
    from ocn_amd.explain import explain_link_edges, explain_links
    from ocn_amd.model import predictor_dict
    from ocn_amd.pipeline import score_edges
    from ocn_amd.recommend import EmbeddingIndex, EmbeddingNeighbours, recommend_links
    from ocn_amd.utils import adjoverlap, adjoverlap_3hop
    c = _e2e()
    H = 64
    t = _table(c.n, H, dt, 5)
    e = c.edges[:64].t().contiguous()
    cn1, cn2 = adjoverlap(c.adj, c.adj, e), adjoverlap(c.adj, c.adj2, e)
    fp32 = "fp32|float32"
    pred = _predictor("cn5", H)
    with pytest.raises(TypeError, match=fp32):                            # grad mode
        pred(t, c.adj, cn1, cn2, e)
    with torch.no_grad(), pytest.raises(TypeError, match=fp32):           # a table that asks for a gradient
        pred(t.clone().requires_grad_(), c.adj, cn1, cn2, e)
    pred.train()
    with torch.no_grad(), pytest.raises(TypeError, match=fp32):
        pred(t, c.adj, cn1, cn2, e)
    pred.eval()
    pred.set_edge_sharding(None, True)
    with torch.no_grad(), pytest.raises(TypeError, match=fp32):
        pred(t, c.adj, cn1, cn2, e)
    with torch.no_grad(), pytest.raises(TypeError, match=fp32):
        pred.begin(t, c.adj, cn1, cn2, e)
    pred.set_edge_sharding(None, False)
    with torch.no_grad():                                                  # ... and the path that takes it
        assert torch.equal(pred(t, c.adj, cn1, cn2, e), pred(t.float(), c.adj, cn1, cn2, e))
    pred6 = predictor_dict["cn6"](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()
    with torch.no_grad(), pytest.raises(TypeError, match=fp32):
        pred6(t, c.adj, cn1, cn2, adjoverlap_3hop(c.adj, c.adj2, e), e)
    with pytest.raises(TypeError, match=fp32):
        score_edges(pred6, t, c.adj, c.adj2, c.edges, 128)
    with pytest.raises(TypeError, match=fp32):
        explain_links(pred, t, c.adj, c.adj2, c.edges[:16].contiguous(), m=4)
    encoder = SimpleNamespace(training=False, convs=[SimpleNamespace(aggr="sum")])
    with pytest.raises(TypeError, match=fp32):
        explain_link_edges(encoder, pred, t, c.adj, c.adj2, c.edges[:16].contiguous(), 0, top=4)
    sources = torch.arange(0, 8, device=DEV)
    with pytest.raises(TypeError, match=fp32):
        recommend_links(pred, t, c.adj, c.adj2, sources, 4, 128, prefilter=EmbeddingNeighbours(8))
    # with a prebuilt index the stage serves a half table: the queries h[sources] widen exactly
    stage = EmbeddingNeighbours(8, keys=EmbeddingIndex(t.float()))
    d1, s1 = recommend_links(pred, t, c.adj, c.adj2, sources, 4, 128, prefilter=stage)
    d2, s2 = recommend_links(pred, t.float(), c.adj, c.adj2, sources, 4, 128, prefilter=stage)
    assert torch.equal(d1, d2) and torch.equal(s1, s2)
