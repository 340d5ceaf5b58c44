"""Pooling from an int8 embedding table (cn_pool_q8.hip, ocn_cn_gather_q8; ``ops.Int8Table``) against the project's own fp32 entries
on ``table.float()``, computed on the device in the same test: int8 -> fp32 is exact, an element is one fp32 multiply by the row's
scale, and the sums are the fp32 entry's — same operands, same order, separately rounded multiply and add — so every comparison
is of raw bits (``torch.equal`` / ``view(torch.int32)``), never of values within a tolerance.  Uncapped, the reference is
``ocn_cn_gather`` (pinned by tests/test_pool_pairs_gpu.py and tests/test_lane_group_gpu.py against the oracle); capped, it is
``ocn_cn_gather_cap`` (pinned by tests/test_pool_cap_gpu.py against tests/pool_cap_mirror.py).  Rows the class-major heads never
read are excluded the way tests/test_pool_h16_gpu.py excludes them (its module docstring states the rule)."""
import pytest
import torch

from tests.test_lane_group_gpu import N as N_STAR
from tests.test_pool_cap_gpu import ROWS, SENTINEL, _case, _dev, _run
from tests.test_pool_h16_gpu import WEIGHTS, _assert_same, _bits, _e2e, _pooled, _predictor, _state, star  # noqa: F401  (star: a fixture)
from tests.test_pool_pairs_gpu import N_REAL, _edges, _graph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
WIDTHS = (16, 32, 64, 128, 256, 512)          # ops.LN_WIDTHS


def _table(n, H, seed):
    """An int8 table of embeddings whose rows spread over several binades (scales that are no powers of two: products and sums
    round), as made by ``embedding_table_int8``."""
    from ocn_amd import ops
    from ocn_amd.pipeline import embedding_table_int8
    g = torch.Generator().manual_seed(seed)
    h = (torch.randn(n, H, generator=g) * torch.exp2(torch.randint(-6, 7, (n, 1), generator=g).float())).to(DEV)
    t = embedding_table_int8(h)
    assert isinstance(t, ops.Int8Table) and t.is_cuda and t.shape == (n, H) and t.rows.shape[1] == max(H, 64)
    tf = t.float()
    assert not torch.equal(tf, h) and bool(((h - tf).abs() <= t.scale[:, None] * (0.5 + 2.0 ** -14)).all())
    return t


# ---- 1. uncapped, every width -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", WIDTHS)
def test_star_every_width(star, monkeypatch, H):  # noqa: F811
    """With and without slot records / the schedule (``sort``), batch-order and class-major output rows."""
    from ocn_amd import ops
    assert WIDTHS == ops.LN_WIDTHS
    t = _table(N_STAR, H, 100 + H)
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
                seen_skip |= bool(_never_read_any(st, out_row))
    assert seen_skip                                     # (some rows were left alone, and the check above looked at them)


def _never_read_any(st, out_row):
    from tests.test_pool_h16_gpu import _never_read
    return _never_read(st, out_row)[1].any()


# ---- 2. hub rows ------------------------------------------------------------------------------------------------------------------
_TAB = {}


def _hub_table(H):
    if H not in _TAB:
        _TAB[H] = _table(N_REAL, H, 7 * H)
    return _TAB[H]


@pytest.mark.parametrize("H", [32, 256])
@pytest.mark.parametrize("B", [1, 7, 64, 128])
def test_hub_rows(hiplib, monkeypatch, B, H):
    """Rows of 1 100, 1 030 and 700 entries, a source without neighbours, runs of one source; B = 128 at H = 256 follows the
    schedule's visiting order."""
    from ocn_amd import ops
    gr = _graph()
    e = _edges(gr, B, 100 + B).to(DEV)
    t = _hub_table(H)
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


# ---- 3. walk route ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [32, 64])
def test_walk_route(hiplib, H):
    """``get_cn1_cn2`` handles: cn2 carries walk counts (a valued ``wc``)."""
    from ocn_amd.utils import fuse, get_cn1_cn2
    gr = _graph()
    e = _edges(gr, 64, 31).to(DEV)
    t = _hub_table(H)
    for ip in (0.0, 0.37):
        st = fuse(*get_cn1_cn2(gr.adj, e), e, None, adj=gr.adj)
        assert st.walk and st.wc is not None
        w = st.weights_cn5(torch.tensor([ip], device=DEV))
        got, ref = _pooled(st, w, t), _pooled(st, w, t.float())
        _assert_same(got, ref, st, None, ip)
        assert bool((got[1] != 0).any())


# ---- 4. values --------------------------------------------------------------------------------------------------------------------
Q_PATTERN = [127, -127, 0, 1, -1, 64, -64, 126, -126, 2, 85, -43, 0, 100, -3, 17]


@pytest.mark.parametrize("H", [16, 64, 256, 512])
def test_special_values_and_padding(hiplib, H):
    """One candidate (0, 1) with the common neighbours 2, 3, 4 (and node 5, a neighbour that is none).  Every row is a rotation
    of Q_PATTERN (q = +-127, 0, +-1 among them); the scales: near 2^-130 (the source row and a pooled row: every product is
    subnormal), near 2^-126 (a pooled row with products on both sides of the smallest normal), near 2^118 (a pooled row with
    elements up to 2^125: its weighted terms stay finite, and where its q is 0 the subnormal terms are the whole sum), near
    2^120 (the target row: x_i * x_j is subnormal times huge).  A multiply that flushed subnormals, or a scale folded into the
    weights, would differ from the fp32 entry, which reads the table dequantised by torch.  The padded columns hold garbage —
    at the index's own stride (64 for H = 16: 48 bytes of it per row) and at a longer one: a kernel that read them would
    differ too, the fp32 entry never sees them."""
    from ocn_amd import ops
    pat = torch.tensor(Q_PATTERN, dtype=torch.int8)
    scale = torch.tensor([1.37 * 2.0 ** -130, 0.9 * 2.0 ** 120, 1.1 * 2.0 ** -130, 1.21 * 2.0 ** 118, 1.7 * 2.0 ** -126, 0.013])
    rowptr = torch.tensor([0, 4, 4, 4, 4, 4, 4], dtype=torch.int64, device=DEV)
    col = torch.tensor([2, 3, 4, 5], dtype=torch.int32, device=DEV)
    src, dst = torch.tensor([0], device=DEV), torch.tensor([1], device=DEV)
    off = torch.tensor([0, 4], device=DEV)
    flags = torch.tensor([3, 1, 2, 0], dtype=torch.uint8, device=DEV)
    w = (torch.tensor([[0.3, 0.7, 0.11, 0.0]], device=DEV).repeat(6, 1)
         * torch.tensor([1.0, 1.1, 0.9, 1.3, 0.77, 1.0], device=DEV)[:, None]).contiguous()

    def pool(h, cap=None):
        ws = {}
        ops.buf(ws, "pooled", (3, 1, H), torch.float32, DEV).fill_(NAN)
        if cap is None:
            return [o.clone() for o in ops.cn_gather(rowptr, col, src, dst, off, flags, None, w, h, max_row_len=4, wsd=ws)]
        return [o.clone() for o in ops.cn_gather_cap(rowptr, col, src, dst, off, flags, None, w, h, cap, 1, max_row_len=4, wsd=ws)]

    g = torch.Generator().manual_seed(H)
    for Hp in (max(H, 64), max(H, 64) + 16):
        rows = torch.randint(-128, 128, (6, Hp), generator=g, dtype=torch.int16).to(torch.int8)      # garbage, -128 included
        rows[:, :H] = torch.stack([torch.roll(pat, 3 * r).repeat(H // 16) for r in range(6)])
        t = ops.Int8Table(rows.to(DEV), scale.to(DEV), H)
        tf = t.float()
        assert tf.shape == (6, H) and bool(torch.isfinite(tf).all()) and bool((tf == 0).any()) and bool((tf.abs() > 1e37).any())
        assert 0 < float(tf[tf != 0].abs().min()) < 2.0 ** -126                              # (torch kept the subnormal products)
        assert torch.equal(tf.cpu(), rows[:, :H].float() * scale[:, None])                  # ... and they are the host's IEEE products
        for cap in (None, 2, 8):                                                             # uncapped, sampled (3 members), within the cap
            got, ref = pool(t, cap), pool(tf, cap)
            torch.cuda.synchronize()
            for a, b in zip(got, ref):
                assert torch.equal(_bits(a), _bits(b)), (Hp, cap)
                assert bool((a != 0).any()) and not bool(torch.isnan(a).any())
            # x_i * x_j: a subnormal row times a huge one, from the dequantised rows on the host
            assert torch.equal(_bits(got[2][0].cpu()), _bits(tf[0].cpu() * tf[1].cpu()))
        if Hp > H:                                                                           # the garbage is there, and another gives the same bits
            rows2 = rows.clone()
            rows2[:, H:] = ~rows[:, H:]
            got2 = pool(ops.Int8Table(rows2.to(DEV), scale.to(DEV), H))
            assert bool(rows[:, H:].any()) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got2, pool(tf)))


# ---- 5. capped --------------------------------------------------------------------------------------------------------------------
_CASES, _CTAB = {}, {}


def _cap_table(H):
    from tests.test_pool_cap_gpu import N
    if H not in _CTAB:
        _CTAB[H] = _table(N, H, 50 + H)
    return _CTAB[H]


@pytest.mark.parametrize("cap", [1, 7, 64])
@pytest.mark.parametrize("H", [16, 64, 256, 512])
def test_capped_equals_the_fp32_capped_entry(hiplib, H, cap):
    """The constructed batch of tests/test_pool_cap_gpu.py (member counts on both sides of the cap, members at the start, at the
    end and alternating, candidates without members, zero weight rows, a hub row): outputs and ``mult`` of the int8 table equal
    those of ``ocn_cn_gather_cap`` on ``table.float()`` — with ``order``, per-row counts and a valued ``wc``, at B = 23, 7 and 1."""
    c = _CASES.setdefault(cap, _case(cap))
    assert max(c.u) > cap and min(c.u) == 0
    d, t = _dev(c), _cap_table(H)
    tf = t.float()
    total = int(c.off[-1])
    order = torch.randperm(c.B, generator=torch.Generator().manual_seed(cap)).to(DEV)
    for valued in (False, True):
        seed = 0x9E3779B97F4A7C15 if valued else 3                                   # (both halves of the key)
        for kw in (dict(), dict(order=order), dict(cnt1=d.cnt1, cnt2=d.cnt2), dict(order=order, cnt1=d.cnt1, cnt2=d.cnt2)):
            got, mult = _run(d, t, cap, seed, valued=valued, **kw)
            want, mult_ref = _run(d, tf, cap, seed, valued=valued, **kw)
            assert torch.equal(mult, mult_ref) and bool((mult[total:] == SENTINEL).all()), (valued, sorted(kw))
            assert int(mult[:total].max()) > 1 or cap >= max(c.u)
            for a, b in zip(got, want):
                assert torch.equal(_bits(a), _bits(b)) and not bool(torch.isnan(a).any()), (valued, sorted(kw))
    for B in (1, 7):
        got, mult = _run(d, t, cap, 3, B=B)
        want, mult_ref = _run(d, tf, cap, 3, B=B)
        assert torch.equal(mult, mult_ref) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want))


@pytest.mark.parametrize("H", [16, 64, 256, 512])
def test_a_cap_no_row_exceeds_is_the_uncapped_call(hiplib, H):
    c = _CASES.setdefault(7, _case(7))
    d, t = _dev(c), _cap_table(H)
    total = int(c.off[-1])
    for cap in (max(ROWS), (1 << 31) - 1, max(c.u)):                                 # (the last: counted first, then pooled exactly)
        for valued in (False, True):
            for kw in (dict(), dict(cnt1=d.cnt1, cnt2=d.cnt2)):
                got, mult = _run(d, t, cap, 5, valued=valued, **kw)
                want, _ = _run(d, t, cap, 5, valued=valued, exact=True, **kw)
                for a, b in zip(got, want):
                    assert torch.equal(_bits(a), _bits(b)) and not bool(torch.isnan(a).any())
                assert torch.equal(mult[:total], (d.flags[:total] != 0).int())


@pytest.mark.parametrize("H", [32, 256])
def test_capped_records_schedule_and_output_rows(hiplib, monkeypatch, H):
    """A batch of the intersection pass (hub rows, a source without neighbours): fed by the slot records and the schedule, by
    ``order`` alone, and with class-major output rows, which leave the rows the heads never read unwritten in both entries."""
    from ocn_amd import ops
    from ocn_amd.utils import CNState
    gr = _graph()
    e = _edges(gr, 128, 228).to(DEV)
    t = _hub_table(H)
    tf = t.float()
    for sort in (True, False):
        monkeypatch.setattr(ops, "sort_edges_min_batch", 0 if sort else 1 << 40)
        st = CNState(gr.adj, gr.adj, gr.adj2, e)
        st.check_status()
        w = st.weights_cn5(torch.tensor([0.37], device=DEV))
        out_row = ops.class_order(st.cnt1, st.cnt2, st.order)[1]
        for kw in (dict(), dict(order=st.order if st.order is not None else torch.arange(127, -1, -1, device=DEV)), dict(out_row=out_row)):
            res = []
            for h in (t, tf):
                ws = {}
                ops.buf(ws, "pooled", (3, 128, H), torch.float32, DEV).fill_(NAN)
                st.ws = ws
                mult = torch.full((st.flags.numel(),), SENTINEL, dtype=torch.int32, device=DEV)
                res.append(([o.clone() for o in st.gather(w, h, cap=(7, 11), mult=mult, **kw)], mult))
            torch.cuda.synchronize()
            (got, mult), (want, mult_ref) = res
            assert torch.equal(mult, mult_ref) and int(mult.max()) > 1
            for q, (a, b) in enumerate(zip(got, want)):
                assert torch.equal(_bits(a), _bits(b)), (sort, sorted(kw), q)                # (unwritten rows are the same NaN bits)
            assert bool(torch.isnan(got[0]).any()) == ("out_row" in kw) and not bool(torch.isnan(got[2]).any())


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------
def _e2e_table(H, seed):
    c = _e2e()
    key = ("e2e", H, seed)
    if key not in _TAB:
        _TAB[key] = _table(c.n, H, seed)
    return c, _TAB[key]


@pytest.mark.parametrize("H", [64, 256])
def test_score_edges(hiplib, monkeypatch, H):
    from ocn_amd import ops
    from ocn_amd.pipeline import score_edges, score_edges_walk
    c, t = _e2e_table(H, H)
    tf = t.float()
    for name, ip in (("cn5", 0.0), ("cn5", 0.37), ("cn7", 0.0), ("cn8", 0.0)):
        pred = _predictor(name, H, ip)
        a, b = score_edges(pred, t, c.adj, c.adj2, c.edges, 128, c.args), score_edges(pred, tf, c.adj, c.adj2, c.edges, 128, c.args)
        assert a.dtype == torch.float32 and a.shape == (300,) and torch.equal(a, b), (name, ip)
        assert bool(torch.isfinite(a).all()) and float(a.std()) > 0
    # cn8 with the one-pass form asked for: an int8 table takes the chain
    monkeypatch.setattr(ops, "cn8_fused_eval", True)
    assert torch.equal(score_edges(pred, t, c.adj, c.adj2, c.edges, 128, c.args), a)
    pred = _predictor("cn5", H, 0.37)
    assert torch.equal(score_edges_walk(pred, t, c.adj, c.edges, 128), score_edges_walk(pred, tf, c.adj, c.edges, 128))
    empty = score_edges(pred, t, c.adj, c.adj2, c.edges[:0], 128)
    assert empty.dtype == torch.float32 and empty.numel() == 0
    # direct calls under no_grad
    from ocn_amd.utils import adjoverlap
    e = c.edges[:64].t().contiguous()
    cn1, cn2 = adjoverlap(c.adj, c.adj, e), adjoverlap(c.adj, c.adj2, e)
    with torch.no_grad():
        assert torch.equal(pred(t, c.adj, cn1, cn2, e), pred(tf, c.adj, cn1, cn2, e))


@pytest.mark.parametrize("H", [64, 256])
def test_frozen_and_capped_predictors(hiplib, monkeypatch, H):
    from ocn_amd import ops
    from ocn_amd.frozen import freeze_columns
    from ocn_amd.pipeline import score_edges, score_edges_walk
    c, t = _e2e_table(H, H + 1)
    tf = t.float()
    pred = _predictor("cn5", H, 0.37)
    pred.set_frozen_columns(freeze_columns(pred, c.adj, c.adj2, c.edges[:200].contiguous()))
    out = {}
    for fused in (False, True):                                                    # (the one-pass form reads fp32 rows: the chain runs)
        monkeypatch.setattr(ops, "frozen_fused_eval", fused)
        out[fused] = score_edges(pred, t, c.adj, c.adj2, c.edges, 128)
        assert torch.equal(out[fused], score_edges(pred, tf, c.adj, c.adj2, c.edges, 128)), fused
    assert torch.equal(out[False], out[True])
    pred.set_cn_cap(3, seed=17)                                                    # frozen and capped
    capped = score_edges(pred, t, c.adj, c.adj2, c.edges, 128)
    assert torch.equal(capped, score_edges(pred, tf, c.adj, c.adj2, c.edges, 128)) and not torch.equal(capped, out[False])
    for name, ip in (("cn5", 0.37), ("cn7", 0.0), ("cn8", 0.0)):                    # capped, the batch's own weights
        pred = _predictor(name, H, ip)
        exact = score_edges(pred, t, c.adj, c.adj2, c.edges, 128, c.args)
        pred.set_cn_cap(int(c.adj.max_rowcount()))
        assert torch.equal(score_edges(pred, t, c.adj, c.adj2, c.edges, 128, c.args), exact), name      # a cap no row exceeds
        pred.set_cn_cap(3, seed=5)
        a, b = score_edges(pred, t, c.adj, c.adj2, c.edges, 128, c.args), score_edges(pred, tf, c.adj, c.adj2, c.edges, 128, c.args)
        assert torch.equal(a, b) and not torch.equal(a, exact) and bool(torch.isfinite(a).all()), name
        assert torch.equal(score_edges_walk(pred, t, c.adj, c.edges, 128, c.args), score_edges_walk(pred, tf, c.adj, c.edges, 128, c.args))


@pytest.mark.parametrize("H", [64, 256])
def test_recommend_links(hiplib, H):
    from ocn_amd.recommend import recommend_links
    c, t = _e2e_table(H, H + 2)
    pred = _predictor("cn5", H, 0.37)
    sources = torch.arange(0, 12, device=DEV)
    for kw in (dict(), dict(prefilter=("ra", 32))):
        for adj2 in (c.adj2, None):
            d1, s1 = recommend_links(pred, t, c.adj, adj2, sources, 10, 256, **kw)
            d2, s2 = recommend_links(pred, t.float(), c.adj, adj2, sources, 10, 256, **kw)
            assert torch.equal(d1, d2) and torch.equal(s1, s2) and s1.dtype == torch.float32, (kw, adj2 is None)
            assert int((d1 >= 0).sum()) > 50


def test_rank_links_and_a_captured_batch(hiplib):
    """``rank_links`` passes an int8 table through like ``recommend_links``; the launch is capturable (``GraphedScorer``)."""
    from ocn_amd.pipeline import GraphedScorer
    from ocn_amd.ranking import rank_links
    from ocn_amd.sparse import SparseTensor
    H = 256
    c, t = _e2e_table(H, 9)
    pred = _predictor("cn5", H, 0.37)
    sources = torch.arange(0, 40, device=DEV)
    truth = SparseTensor.from_edge_index(c.edges.t().contiguous(), sparse_sizes=(c.n, c.n)).to_symmetric()
    r1 = rank_links(pred, t, c.adj, c.adj2, sources, truth, 128, prefilter=("ra", 32))
    r2 = rank_links(pred, t.float(), c.adj, c.adj2, sources, truth, 128, prefilter=("ra", 32))
    assert torch.equal(r1.rank, r2.rank) and torch.equal(r1.retrieval_rank, r2.retrieval_rank)
    e = c.edges[:128].t().contiguous()
    for cap in (None, 4):
        pred.set_cn_cap(cap)
        a = GraphedScorer(pred, t, c.adj, c.adj2, 128)(e).clone()
        b = GraphedScorer(pred, t.float(), c.adj, c.adj2, 128)(e).clone()
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()), cap


def test_the_table_is_the_retrieval_index(hiplib):
    """An ``EmbeddingNeighbours`` stage without ``keys=`` retrieves from the table itself: the result of the call with
    ``keys=EmbeddingIndex.from_table(table)`` and ``h = table.float()``; ``rank_links`` alike; a cosine stage is refused, unless
    its index is passed."""
    from ocn_amd.ranking import rank_links
    from ocn_amd.recommend import EmbeddingIndex, EmbeddingNeighbours, ShortListUnion, recommend_links
    from ocn_amd.sparse import SparseTensor
    H = 64
    c, t = _e2e_table(H, 5)
    tf = t.float()
    pred = _predictor("cn5", H, 0.37)
    sources = torch.arange(0, 8, device=DEV)
    index = EmbeddingIndex.from_table(t)
    assert index.keys_q.data_ptr() == t.rows.data_ptr() and index.kscale.data_ptr() == t.scale.data_ptr()
    for stage, ref in ((EmbeddingNeighbours(8), EmbeddingNeighbours(8, keys=index)),
                       (ShortListUnion(("ra", 8), EmbeddingNeighbours(8)), ShortListUnion(("ra", 8), EmbeddingNeighbours(8, keys=index)))):
        d1, s1 = recommend_links(pred, t, c.adj, c.adj2, sources, 4, 128, prefilter=stage)
        d2, s2 = recommend_links(pred, tf, c.adj, c.adj2, sources, 4, 128, prefilter=ref)
        assert torch.equal(d1, d2) and torch.equal(s1, s2) and int((d1 >= 0).sum()) > 16
    # (the table's own image is also what EmbeddingIndex makes of the fp32 rows it stands for, up to re-quantisation: not assumed)
    truth = SparseTensor.from_edge_index(c.edges.t().contiguous(), sparse_sizes=(c.n, c.n)).to_symmetric()
    r1 = rank_links(pred, t, c.adj, c.adj2, sources, truth, 128, prefilter=EmbeddingNeighbours(8))
    r2 = rank_links(pred, tf, c.adj, c.adj2, sources, truth, 128, prefilter=EmbeddingNeighbours(8, keys=index))
    assert torch.equal(r1.rank, r2.rank) and torch.equal(r1.retrieval_rank, r2.retrieval_rank)
    with pytest.raises(TypeError, match="fp32|float32"):
        recommend_links(pred, t, c.adj, c.adj2, sources, 4, 128, prefilter=EmbeddingNeighbours(8, normalize=True))
    cos = EmbeddingNeighbours(8, normalize=True, keys=EmbeddingIndex(tf, normalize=True))          # a passed index is used as given
    d1, s1 = recommend_links(pred, t, c.adj, c.adj2, sources, 4, 128, prefilter=cos)
    d2, s2 = recommend_links(pred, tf, c.adj, c.adj2, sources, 4, 128, prefilter=cos)
    assert torch.equal(d1, d2) and torch.equal(s1, s2)


def test_refusals_on_the_device(hiplib):
    from ocn_amd.explain import explain_links
    from ocn_amd.model import predictor_dict
    from ocn_amd.pipeline import score_edges
    from ocn_amd.utils import adjoverlap
    H = 64
    c, t = _e2e_table(H, 5)
    e = c.edges[:64].t().contiguous()
    cn1, cn2 = adjoverlap(c.adj, c.adj, e), adjoverlap(c.adj, c.adj2, e)
    fp32 = "fp32|float32"
    pred = _predictor("cn5", H)
    with pytest.raises(TypeError, match=fp32):                            # grad mode
        pred(t, c.adj, cn1, cn2, e)
    pred.train()
    with torch.no_grad(), pytest.raises(TypeError, match=fp32):
        pred(t, c.adj, cn1, cn2, e)
    pred.eval()
    pred.set_edge_sharding(None, True)
    with torch.no_grad(), pytest.raises(TypeError, match=fp32):
        pred.begin(t, c.adj, cn1, cn2, e)
    pred.set_edge_sharding(None, False)
    pred6 = predictor_dict["cn6"](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()
    with pytest.raises(TypeError, match=fp32):
        score_edges(pred6, t, c.adj, c.adj2, c.edges, 128)
    with pytest.raises(TypeError, match=fp32):
        explain_links(pred, t, c.adj, c.adj2, c.edges[:16].contiguous(), m=4)


def test_example_driver_with_an_int8_table(hiplib):
    """examples/run_like_reference.py --table-dtype int8: training is fp32, test() and --recommend pool from the int8 table —
    capped too, and an embedding stage retrieves from the table itself."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "run_like_reference.py")
    spec = importlib.util.spec_from_file_location("run_like_reference", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--dataset", "cora", "--epochs", "2", "--hiddim", "64", "--feat", "64", "--batch_size", "1152", "--table-dtype", "int8",
                    "--cn-cap", "2:1", "--recommend", "3", "--recommend-emb", "8"])
    assert len(out) == 2 and all(o[0] == o[0] for o in out)
    assert all(0.0 <= v <= 1.0 for v in out[-1][1]["Hits@100"])
    for bad in (["--table-dtype", "int8", "--predictor", "cn6"], ["--table-dtype", "int8", "--recommend", "3", "--recommend-emb", "8:cos"],
                ["--table-dtype", "int4"]):
        with pytest.raises(SystemExit):
            mod.main(["--dataset", "cora"] + bad)
