"""The capped pooling on the device (cn_pool_cap.hip: ocn_cn_gather_cap; ``ops.cn_gather_cap``; ``predictor.set_cn_cap``)
against tests/pool_cap_mirror.py — the contract restated in numpy and Python integers — and against the exact pooling.  Every
comparison of pooled rows and multipliers is of raw bits (``view(torch.int32)``, ``torch.equal``); output buffers are
pre-filled with NaN and ``mult`` with a sentinel, so that what a launch leaves unwritten compares too."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import pool_cap_mirror as M
from tests.test_pool_h16_gpu import _e2e, _predictor
from tests.test_pool_pairs_gpu import _edges, _graph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
WIDTHS = (16, 32, 64, 128, 256, 512)          # ops.LN_WIDTHS
CAPS = (1, 2, 3, 7, 64, 65)
SENTINEL = -77
ROWS = (33, 63, 64, 65, 129, 513, 1100)       # source rows: both sides of every width's round (32 or 64 positions), one hub row
N = 1400


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the constructed batch --------------------------------------------------------------------------------------------------------
def _members(da, u, where):
    """The positions of u members of a row of da entries."""
    if where == "start":
        return list(range(u))
    if where == "end":
        return list(range(da - u, da))
    step = 2 if 2 * u - 1 <= da else 1                                   # alternating where the row is long enough
    return list(range(0, step * u, step))


def _case(cap):
    """Source s = 0 .. 6 has ROWS[s] sorted random neighbours; candidates with u in {d - 1, d, d + 1, 2 d, 2 d + 1, 3 d - 1}
    members packed at the start, at the end and alternating, with cn1-only, cn2-only and both flags, plus candidates without
    members (one of a source without neighbours).  23 candidates: no multiple of the candidates a wave or a workgroup holds
    at any width.  cn2 values above 1 (a valued ``wc``) and a weight table with zero rows (members that are selected and not
    fetched)."""
    g = np.random.default_rng(1000 + cap)
    rows = [np.sort(g.choice(np.arange(len(ROWS) + 1, N), size=L, replace=False)).astype(np.int32) for L in ROWS] + [np.zeros(0, np.int32)]
    rowptr = np.zeros(N + 1, np.int64)
    rowptr[1:len(rows) + 1] = np.cumsum([len(r) for r in rows])
    rowptr[len(rows) + 1:] = rowptr[len(rows)]
    col = np.concatenate(rows)
    cands, n = [], 0
    for u in sorted({cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1, 3 * cap - 1}):
        for where in ("start", "end", "alt"):
            fit = [s for s, L in enumerate(ROWS) if L >= max(u, 1)]
            s = fit[n % len(fit)]
            cands.append((s, 100 + n, _members(ROWS[s], u, where), (1, 2, 3)[n % 3]))
            n += 1
    cands += [(6, 90, [], 0), (len(ROWS), 91, [], 0), (2, 92, list(range(ROWS[2])), 3), (5, 93, [], 0), (0, 94, [5], 2)]
    while len(cands) < 23:                                                    # (the small caps have fewer distinct u)
        cands.append((6, 100 + n, _members(ROWS[6], cap + 2 + n, "alt"), (1, 2, 3)[n % 3]))
        n += 1
    assert len(cands) == 23
    src = np.array([c[0] for c in cands], np.int64)
    dst = np.array([c[1] for c in cands], np.int64)
    off = np.zeros(len(cands) + 1, np.int64)
    off[1:] = np.cumsum([rowptr[s + 1] - rowptr[s] for s in src])
    flags = np.zeros(int(off[-1]) + 5, np.uint8)                           # (five spare positions: nothing is written there)
    for e, (_, _, mem, f) in enumerate(cands):
        flags[off[e] + np.array(mem, np.int64)] = f
    wc = g.integers(1, 6, size=flags.shape[0]).astype(np.int32)
    w = g.standard_normal((N, 4)).astype(np.float32)
    w[:, 3] = 0
    w[g.random(N) < 0.15] = np.array([0.0, 0.7, 0.0, 0.0], np.float32)     # f != 0 but wa = wb = 0
    cnt1 = np.array([len(c[2]) if c[3] & 1 else 0 for c in cands], np.int32)
    cnt2 = np.array([len(c[2]) if c[3] & 2 else 0 for c in cands], np.int32)
    return SimpleNamespace(rowptr=rowptr, col=col, src=src, dst=dst, off=off, flags=flags, wc=wc, w=w, cnt1=cnt1, cnt2=cnt2,
                           B=len(cands), u=[len(c[2]) for c in cands])


_CASES, _TABLES, _REF = {}, {}, {}


def _table(H):
    if H not in _TABLES:
        g = torch.Generator().manual_seed(50 + H)
        _TABLES[H] = (torch.randn(N, H, generator=g) * torch.exp2(torch.randint(-4, 5, (N, 1), generator=g).float())).contiguous()
    return _TABLES[H]


def _ref(cap, H, valued, seed):
    """The mirror's (mult, xcn1, xcn2, xij) of the constructed batch, computed once per case."""
    key = (cap, H, valued, seed)
    if key not in _REF:
        c = _CASES.setdefault(cap, _case(cap))
        _REF[key] = M.pool(c.rowptr, c.col, c.src, c.dst, c.off, c.flags, c.wc if valued else None, c.w, _table(H).numpy(), cap, seed)
    return _REF[key]


def _dev(c):
    t = lambda a: torch.from_numpy(a).to(DEV)
    return SimpleNamespace(rowptr=t(c.rowptr), col=t(c.col), src=t(c.src), dst=t(c.dst), off=t(c.off), flags=t(c.flags), wc=t(c.wc),
                           w=t(c.w), cnt1=t(c.cnt1), cnt2=t(c.cnt2))


def _run(d, h, cap, seed, B=None, valued=False, exact=False, **kw):
    """One launch into NaN-filled rows and a sentinel-filled ``mult``; ``exact``: ``ops.cn_gather`` on the same arguments."""
    from ocn_amd import ops
    B = d.src.numel() if B is None else B
    ws = {}
    ops.buf(ws, "pooled", (3, B, h.shape[1]), torch.float32, DEV).fill_(NAN)
    args = (d.rowptr, d.col, d.src[:B], d.dst[:B], d.off[:B + 1], d.flags, d.wc if valued else None, d.w, h)
    if exact:
        out = ops.cn_gather(*args, max_row_len=max(ROWS), wsd=ws, **kw)
        return [o.clone() for o in out], None
    mult = torch.full((d.flags.numel(),), SENTINEL, dtype=torch.int32, device=DEV)
    out = ops.cn_gather_cap(*args, cap, seed, max_row_len=max(ROWS), wsd=ws, mult=mult, **kw)
    torch.cuda.synchronize()
    return [o.clone() for o in out], mult


# ---- 1. mirror equality -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("H", WIDTHS)
def test_mirror_equality(hiplib, H, cap):
    c = _CASES.setdefault(cap, _case(cap))
    assert c.B == 23 and max(c.u) > cap and min(c.u) == 0 and {cap, cap + 1, 2 * cap, 3 * cap - 1} <= set(c.u)
    d, h = _dev(c), _table(H).to(DEV)
    total = int(c.off[-1])
    order = torch.randperm(c.B, generator=torch.Generator().manual_seed(cap)).to(DEV)
    for valued in (False, True):
        seed = 0x9E3779B97F4A7C15 if valued else 3                                   # (both halves of the key)
        mult_ref, x1, x2, xij = _ref(cap, H, valued, seed)
        ref = [torch.from_numpy(a) for a in (x1, x2, xij)]
        for kw in (dict(), dict(order=order), dict(cnt1=d.cnt1, cnt2=d.cnt2), dict(order=order, cnt1=d.cnt1, cnt2=d.cnt2)):
            out, mult = _run(d, h, cap, seed, valued=valued, **kw)
            assert torch.equal(mult[:total].cpu().long(), torch.from_numpy(mult_ref)), (valued, sorted(kw))
            assert bool((mult[total:] == SENTINEL).all())                           # nothing past the batch's positions
            for got, want in zip(out, ref):
                assert torch.equal(_bits(got.cpu()), _bits(want)), (valued, sorted(kw))
        # every multiplier sums to the member count; some capped candidate pooled a reweighted row
        per = [int(mult_ref[c.off[e]:c.off[e + 1]].sum()) for e in range(c.B)]
        assert per == c.u and int(mult_ref.max()) > 1
    # B = 1, and a B that is no multiple of a wave's candidates at any width but 256 / 512 (there: of a workgroup's)
    for B in (1, 7):
        out, mult = _run(d, h, cap, 3, B=B)
        mult_ref, x1, x2, xij = _ref(cap, H, False, 3)
        upto = int(c.off[B])
        assert torch.equal(mult[:upto].cpu().long(), torch.from_numpy(mult_ref[:upto])) and bool((mult[upto:] == SENTINEL).all())
        for got, want in zip(out, (x1, x2, xij)):
            assert torch.equal(_bits(got.cpu()), _bits(torch.from_numpy(want[:B])))


@pytest.mark.parametrize("cap", [7, 64])
@pytest.mark.parametrize("H", [32, 256])
def test_records_schedule_and_output_rows(hiplib, monkeypatch, H, cap):
    """A batch of the intersection pass (hub rows of 1 100 and 1 030 entries, a source without neighbours, runs of one source):
    fed by the slot records and the schedule (``rec`` / ``perm``; B = 128 at H = 256 follows a visiting order), by ``order``
    alone, and in batch order; class-major output rows (``out_row``) leave the rows the heads never read unwritten."""
    from ocn_amd import ops
    from ocn_amd.utils import CNState
    gr = _graph()
    e = _edges(gr, 128, 228).to(DEV)
    g = torch.Generator().manual_seed(H)
    h = torch.randn(gr.adj.size(0), H, generator=g).to(DEV)
    ref, seen = None, set()
    for sort in (True, False):
        monkeypatch.setattr(ops, "sort_edges_min_batch", 0 if sort else 1 << 40)
        st = CNState(gr.adj, gr.adj, gr.adj2, e)
        st.check_status()
        w = st.weights_cn5(torch.tensor([0.37], device=DEV))
        if ref is None:
            ref = M.pool(gr.adj._rowptr.cpu().numpy(), gr.adj._col.cpu().numpy(), st.src.cpu().numpy(), st.dst.cpu().numpy(),
                         st.off.cpu().numpy(), st.flags.cpu().numpy(), None, w.cpu().numpy(), h.cpu().numpy(), cap, 11)
            u = torch.tensor([int((st.flags[int(st.off[q]):int(st.off[q + 1])] != 0).sum()) for q in range(128)])
            assert int((u > cap).sum()) >= 1 and int((u == 0).sum()) >= 1 and int(gr.adj.max_rowcount()) > 1024
        total = int(st.off[-1])
        out_row = ops.class_order(st.cnt1, st.cnt2, st.order)[1]
        for kw in (dict(), dict(order=st.order if st.order is not None else torch.arange(127, -1, -1, device=DEV)), dict(out_row=out_row)):
            seen.add((st.rec is not None and "order" not in kw, st.sched is not None and "order" not in kw and H == 256, *sorted(kw)))
            ws = {}
            ops.buf(ws, "pooled", (3, 128, H), torch.float32, DEV).fill_(NAN)
            st.ws = ws
            mult = torch.full((st.flags.numel(),), SENTINEL, dtype=torch.int32, device=DEV)
            out = [o.clone() for o in st.gather(w, h, cap=(cap, 11), mult=mult, **kw)]
            torch.cuda.synchronize()
            assert torch.equal(mult[:total].cpu().long(), torch.from_numpy(ref[0][:total])) and bool((mult[total:] == SENTINEL).all())
            rows = kw.get("out_row", torch.arange(128, device=DEV))
            no1, no_any = st.cnt1 == 0, (st.cnt1 == 0) & (st.cnt2 == 0)
            for q, (got, skip) in enumerate(zip(out, (no1, no_any, torch.zeros_like(no1)))):
                got = got[rows]                                                     # batch order again
                want = torch.from_numpy(ref[1 + q]).to(DEV)
                if "out_row" in kw:
                    assert bool(torch.isnan(got[skip]).all()) and bool(skip.any()) == (q < 2)
                    assert torch.equal(_bits(got[~skip]), _bits(want[~skip]))
                else:
                    assert torch.equal(_bits(got), _bits(want))
    assert any(s[0] for s in seen) and any(not s[0] for s in seen) and (H != 256 or any(s[1] for s in seen))


# ---- 2. the exact path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", WIDTHS)
def test_a_cap_no_row_exceeds_is_the_exact_pooling(hiplib, H):
    c = _CASES.setdefault(7, _case(7))
    d, h = _dev(c), _table(H).to(DEV)
    total = int(c.off[-1])
    for cap in (max(ROWS), max(ROWS) + 1, (1 << 31) - 1):
        for valued in (False, True):
            for kw in (dict(), dict(cnt1=d.cnt1, cnt2=d.cnt2)):
                got, mult = _run(d, h, cap, 5, valued=valued, **kw)
                want, _ = _run(d, h, cap, 5, valued=valued, exact=True, **kw)
                for a, b in zip(got, want):
                    assert torch.equal(_bits(a), _bits(b)) and not bool(torch.isnan(a).any())
                assert torch.equal(mult[:total], (d.flags[:total] != 0).int())
    # ... and a cap below the longest row that no candidate's member count exceeds: counted, then pooled exactly
    cap = max(c.u)
    assert cap < max(ROWS)
    got, mult = _run(d, h, cap, 5)
    want, _ = _run(d, h, cap, 5, exact=True)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want)) and torch.equal(mult[:total], (d.flags[:total] != 0).int())


# ---- 3. batch independence, 4. the seed -------------------------------------------------------------------------------------------
def _sub(c, idx):
    """The batch of the candidates ``idx`` of case c (repeats allowed), flags copied to the new offsets."""
    src, dst = c.src[idx], c.dst[idx]
    lens = np.array([c.off[e + 1] - c.off[e] for e in idx], np.int64)
    off = np.zeros(len(idx) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    flags = np.concatenate([c.flags[c.off[e]:c.off[e + 1]] for e in idx] + [np.zeros(3, np.uint8)])
    return SimpleNamespace(rowptr=c.rowptr, col=c.col, src=src, dst=dst, off=off, flags=flags, wc=np.ones(len(flags), np.int32), w=c.w,
                           cnt1=c.cnt1[idx], cnt2=c.cnt2[idx])


@pytest.mark.parametrize("H", [16, 256])
def test_a_candidate_does_not_depend_on_its_batch(hiplib, H):
    cap = 7
    c = _CASES.setdefault(cap, _case(cap))
    h = _table(H).to(DEV)
    base_out, base_mult = _run(_dev(c), h, cap, 21)
    rng = np.random.default_rng(4)
    for idx in (np.arange(c.B)[::-1].copy(), rng.permutation(c.B)[:9], np.array([12, 3, 12, 12, 17, 3]), np.array([17])):
        s = _sub(c, idx)
        d = _dev(s)
        for kw in (dict(), dict(order=torch.randperm(len(idx), generator=torch.Generator().manual_seed(1)).to(DEV))):
            out, mult = _run(d, h, cap, 21, **kw)
            for q, e in enumerate(idx):
                assert torch.equal(mult[int(s.off[q]):int(s.off[q + 1])], base_mult[int(c.off[e]):int(c.off[e + 1])])
                for a, b in zip(out, base_out):
                    assert torch.equal(_bits(a[q]), _bits(b[e]))


def test_the_seed_moves_capped_candidates_only(hiplib):
    cap, H = 7, 64
    c = _CASES.setdefault(cap, _case(cap))
    d, h = _dev(c), _table(H).to(DEV)
    out_a, mult_a = _run(d, h, cap, 1)
    out_b, mult_b = _run(d, h, cap, 2)
    out_c, mult_c = _run(d, h, cap, 1 << 32)                                        # (the key's high word alone)
    moved = 0
    for e, u in enumerate(c.u):
        lo, hi = int(c.off[e]), int(c.off[e + 1])
        same = torch.equal(mult_a[lo:hi], mult_b[lo:hi]) and torch.equal(mult_a[lo:hi], mult_c[lo:hi])
        if u <= cap:
            assert same and all(torch.equal(_bits(a[e]), _bits(b[e])) for a, b in zip(out_a, out_b))
        else:
            moved += not same
            assert int(mult_b[lo:hi].sum()) == u == int(mult_c[lo:hi].sum())
    assert moved > 0 and not torch.equal(mult_a, mult_c)


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------
def _args():
    return SimpleNamespace(sum=0.7)


# (cn8 pools without column weights: there is nothing to freeze)
@pytest.mark.parametrize("name,frozen", [("cn5", False), ("cn5", True), ("cn7", False), ("cn7", True), ("cn8", False)])
def test_score_edges_with_a_cap(hiplib, monkeypatch, name, frozen):
    from ocn_amd import ops
    from ocn_amd.frozen import freeze_columns
    from ocn_amd.pipeline import score_edges, score_edges_walk
    from ocn_amd.utils import adjoverlap, get_cn1_cn2
    c, H, args = _e2e(), 64, _args()
    h = torch.randn(c.n, H, generator=torch.Generator().manual_seed(8)).to(DEV)
    max_deg = int(c.adj.max_rowcount())
    for walk in (False, True):
        pred = _predictor(name, H, 0.37 if name == "cn5" else 0.0)
        if frozen:
            pred.set_frozen_columns(freeze_columns(pred, c.adj, None if walk else c.adj2, c.edges[:200].contiguous(), args), args)
        score = ((lambda: score_edges_walk(pred, h, c.adj, c.edges, 128, args)) if walk
                 else (lambda: score_edges(pred, h, c.adj, c.adj2, c.edges, 128, args)))
        exact = score()
        assert pred.set_cn_cap(max_deg) is None
        assert torch.equal(score(), exact), (walk, "a cap no row exceeds")
        for fused in (True, False):                                                # the one-pass forms fall to the chain
            monkeypatch.setattr(ops, "cn8_fused_eval", fused)
            monkeypatch.setattr(ops, "frozen_fused_eval", fused)
            assert pred.set_cn_cap(3, seed=17) is not None
            capped = score()
            assert capped.shape == exact.shape and bool(torch.isfinite(capped).all()) and not torch.equal(capped, exact)
            direct = []
            with torch.no_grad():
                for lo in range(0, 300, 128):
                    e = c.edges[lo:lo + 128].t().contiguous()
                    cn1, cn2 = get_cn1_cn2(c.adj, e) if walk else (adjoverlap(c.adj, c.adj, e), adjoverlap(c.adj, c.adj2, e))
                    direct.append(pred.multidomainforward(h, c.adj, cn1, cn2, e, args).reshape(-1))
            assert torch.equal(capped, torch.cat(direct)), (walk, fused)
        assert pred.set_cn_cap(3, seed=18) == (3, 17) and not torch.equal(score(), capped)      # the seed is read
        monkeypatch.setattr(ops, "cn8_fused_eval", False)
        monkeypatch.setattr(ops, "frozen_fused_eval", False)
        assert pred.set_cn_cap(None) == (3, 18)
        assert torch.equal(score(), exact), (walk, "restored")


@pytest.mark.parametrize("name", ["cn5", "cn7"])
def test_a_frozen_capped_predictor_scores_a_pair_alike_in_every_batch(hiplib, name):
    from ocn_amd.frozen import freeze_columns
    from ocn_amd.pipeline import score_edges
    from ocn_amd.utils import CNState
    c, H, args = _e2e(), 64, _args()
    h = torch.randn(c.n, H, generator=torch.Generator().manual_seed(9)).to(DEV)
    pred = _predictor(name, H, 0.37 if name == "cn5" else 0.0)
    fc = freeze_columns(pred, c.adj, c.adj2, c.edges[:200].contiguous(), args)
    pred.set_frozen_columns(fc, args)
    pred.set_cn_cap(3, seed=5)
    a, b = score_edges(pred, h, c.adj, c.adj2, c.edges, 128, args), score_edges(pred, h, c.adj, c.adj2, c.edges, 77, args)
    assert float((a - b).abs().max()) <= 1e-5                                     # (the heads' tiles differ with the batch size)
    # ... and the pooled vectors of a pair are the same bits wherever it stands
    whole = CNState(c.adj, c.adj, c.adj2, c.edges.t().contiguous())
    part = CNState(c.adj, c.adj, c.adj2, c.edges[40:117].t().contiguous())
    pw = [o.clone() for o in whole.gather(fc.weights, h, cap=(3, 5))]
    pp = [o.clone() for o in part.gather(fc.weights, h, cap=(3, 5))]
    u = torch.tensor([int((whole.flags[int(whole.off[q]):int(whole.off[q + 1])] != 0).sum()) for q in range(300)])
    assert int((u[40:117] > 3).sum()) >= 5
    for x, y in zip(pw, pp):
        assert torch.equal(_bits(x[40:117]), _bits(y))


def test_recommend_and_rank_links_run_with_a_cap(hiplib):
    from ocn_amd.ranking import rank_links
    from ocn_amd.recommend import recommend_links
    from ocn_amd.sparse import SparseTensor
    c, H = _e2e(), 64
    h = torch.randn(c.n, H, generator=torch.Generator().manual_seed(10)).to(DEV)
    pred = _predictor("cn5", H, 0.37)
    sources = torch.arange(0, 12, device=DEV)
    d0, s0 = recommend_links(pred, h, c.adj, c.adj2, sources, 10, 256)
    pred.set_cn_cap(int(c.adj.max_rowcount()))
    d1, s1 = recommend_links(pred, h, c.adj, c.adj2, sources, 10, 256)
    assert torch.equal(d0, d1) and torch.equal(s0, s1)
    pred.set_cn_cap(2, seed=1)
    d2, s2 = recommend_links(pred, h, c.adj, c.adj2, sources, 10, 256)
    assert d2.shape == d0.shape and int((d2 >= 0).sum()) > 50 and bool(torch.isfinite(s2[d2 >= 0]).all())
    assert all(torch.equal(x, y) for x, y in zip((d2, s2), recommend_links(pred, h, c.adj, c.adj2, sources, 10, 256)))
    truth = SparseTensor.from_edge_index(c.edges.t().contiguous(), sparse_sizes=(c.n, c.n)).to_symmetric()
    r = rank_links(pred, h, c.adj, c.adj2, torch.arange(0, 40, device=DEV), truth, 128, prefilter=("ra", 32))
    assert r.rank.numel() > 0


def test_score_mrr_split_with_a_cap(hiplib):
    """The citation2 layout (walk route): a cap no row exceeds returns the exact scores' MRR, a small cap runs."""
    from ocn_amd.evaluate import Evaluator
    from ocn_amd.pipeline import score_mrr_split
    c, H, args = _e2e(), 64, _args()
    h = torch.randn(c.n, H, generator=torch.Generator().manual_seed(12)).to(DEV)
    pred = _predictor("cn7", H)
    source, target = c.edges[:60, 0].contiguous(), c.edges[:60, 1].contiguous()
    neg = torch.randint(0, c.n, (60, 7), generator=torch.Generator().manual_seed(13)).to(DEV)
    ev = Evaluator(name="ogbl-citation2")
    exact = score_mrr_split(pred, h, c.adj, source, target, neg, 128, args, ev)
    pred.set_cn_cap(int(c.adj.max_rowcount()))
    assert score_mrr_split(pred, h, c.adj, source, target, neg, 128, args, ev) == exact
    pred.set_cn_cap(2, seed=3)
    capped = score_mrr_split(pred, h, c.adj, source, target, neg, 128, args, ev)
    assert 0.0 <= float(capped) <= 1.0


def test_example_driver_with_a_cap(hiplib):
    """examples/run_like_reference.py --cn-cap D:SEED: training pools exactly, test() and --recommend pool the capped sample."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "run_like_reference.py")
    spec = importlib.util.spec_from_file_location("run_like_reference", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--dataset", "cora", "--epochs", "2", "--hiddim", "64", "--feat", "64", "--batch_size", "1152", "--cn-cap", "2:1",
                    "--recommend", "3"])
    assert len(out) == 2 and all(o[0] == o[0] for o in out)
    assert all(0.0 <= v <= 1.0 for v in out[-1][1]["Hits@100"])
    for bad in (["--cn-cap", "0"], ["--cn-cap", "4:x"], ["--cn-cap", "4", "--predictor", "cn6"], ["--cn-cap", "4", "--table-dtype", "bf16"]):
        with pytest.raises(SystemExit):
            mod.main(["--dataset", "cora"] + bad)
