"""Ranking held-out links on the GPU (ocn_amd/ranking.py on ``ocn_segment_rank``).  The kernel against a numpy restatement — the
``lexsort((pos, -score, isnan))`` order of ``tests/test_recommend_gpu.ref_topk``, inverted — and against ``ocn_segment_topk`` on
the device; the public layer against ``recommend_links*`` with identical arguments.  Everything compared is an integer or a
position: every comparison is ``torch.equal``."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import ocn_oracle as O
from tests.helpers import make_graph, product_adj2, to_product

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def src_tensor(v):
    return torch.tensor(list(v), dtype=torch.int64, device=DEV)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def ref_place(seg):
    """place[i] = the 1-based place of entry i of one segment in the order {numbers before NaNs, higher score first (+0 == -0),
    lower position first}."""
    nan = np.isnan(seg)
    order = np.lexsort((np.arange(seg.size), -np.where(nan, np.float32(0), seg), nan))
    place = np.empty(seg.size, dtype=np.int64)
    place[order] = np.arange(1, seg.size + 1)
    return place


def ref_rank(scores, ptr, edges, tptr, tnode):
    """(rank, pos) of every target on the host."""
    s, ids, p, tp = scores.numpy(), edges[:, 1].tolist(), ptr.tolist(), tptr.tolist()
    rank, pos = torch.zeros(tnode.numel(), dtype=torch.int64), torch.full((tnode.numel(),), -1, dtype=torch.int64)
    for q in range(len(p) - 1):
        if tp[q + 1] == tp[q]:
            continue
        place = ref_place(s[p[q]:p[q + 1]])
        where = {c: i for i, c in enumerate(ids[p[q]:p[q + 1]])}
        for j in range(tp[q], tp[q + 1]):
            i = where.get(int(tnode[j]))
            if i is not None:
                rank[j], pos[j] = int(place[i]), p[q] + i
    return rank, pos


# segment length, targets: every member ("all"), 200 members ("some"), none.  63 .. 65 bracket the 64-score chunk, 255 .. 257 the
# four-chunk look-ahead window; empty target lists stand first, in the middle and last.
SEGMENTS = [(0, "none"), (0, "all"), (1, "all"), (2, "all"), (63, "all"), (64, "all"), (65, "all"), (100, "none"), (255, "all"),
            (256, "all"), (257, "all"), (1000, "all"), (70000, "some"), (5, "none"), (0, "none")]
FAR = [-1, -(1 << 40), 1 << 31, (1 << 31) + 5, 1 << 62]               # ids no segment holds: negative, and beyond int32


@pytest.fixture(scope="module")
def case(hiplib):
    """Scores quantised to four values — heavy ties — with +-0.0, +-inf and NaNs mixed in; ascending ids with gaps; per segment
    the targets of SEGMENTS, shuffled, then ids absent below the first id, above the last and in a gap, FAR, and three repeats."""
    from ocn_amd import ops
    g = torch.Generator().manual_seed(77)
    special = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan")])
    scores, edges, ptr, tptr, tnode, members = [], [], [0], [0], [], []
    for q, (n, mode) in enumerate(SEGMENTS):
        sc = torch.tensor([-0.5, 0.25, 1.0, 3.0])[torch.randint(0, 4, (n,), generator=g)]
        pick = torch.rand(n, generator=g) < 0.2
        sc[pick] = special[torch.randint(0, 5, (int(pick.sum()),), generator=g)]
        step = torch.randint(1, 4, (n,), generator=g)
        if n >= 2:
            step[1] = 3                                                  # a gap behind the first id
        ids = torch.cumsum(step, 0) + 10 + q
        scores.append(sc)
        edges.append(torch.stack([torch.full((n,), q, dtype=torch.int64), ids], dim=1))
        ptr.append(ptr[-1] + n)
        t = []
        if mode != "none":
            own = ids[torch.randperm(n, generator=g)]
            own = own if mode == "all" else own[:200]
            t = own.tolist() + FAR + [5] + own[:3].tolist()              # (5: below every id)
            if n:
                t += [int(ids[0]) - 1, int(ids[-1]) + 1]
            if n >= 2:
                t += [int(ids[0]) + 1, int(ids[1]) - 1]                  # the gap
            members.append((q, len(tnode), own.numel()))
        tnode += t
        tptr.append(len(tnode))
    c = SimpleNamespace(scores=torch.cat(scores), edges=torch.cat(edges), ptr=torch.tensor(ptr), tptr=torch.tensor(tptr),
                        tnode=torch.tensor(tnode, dtype=torch.int64), members=members)
    assert bool(c.scores.isnan().any()) and bool(c.scores.isinf().any()) and bool(torch.signbit(c.scores[c.scores == 0]).any())
    c.want_rank, c.want_pos = ref_rank(c.scores, c.ptr, c.edges, c.tptr, c.tnode)
    c.dev = [t.to(DEV) for t in (c.scores, c.ptr, c.edges, c.tptr, c.tnode)]
    c.rank, c.pos = ops.segment_rank(*c.dev)
    return c


def test_kernel_equals_the_restatement(case):
    c = case
    assert c.rank.dtype == torch.int64 and c.pos.dtype == torch.int64 and c.rank.is_cuda and c.rank.shape == c.tnode.shape
    assert torch.equal(c.pos.cpu(), c.want_pos)
    assert torch.equal(c.rank.cpu(), c.want_rank)
    rank = c.rank.cpu()
    for q, at, n_own in c.members:                                      # every member of a segment: the ranks are a permutation of 1 .. n
        n = SEGMENTS[q][0]
        got = rank[at:at + n_own]
        if SEGMENTS[q][1] == "all":
            assert torch.equal(got.sort().values, torch.arange(1, n + 1)), q
        else:
            assert n_own == 200 and got.unique().numel() == 200 and int(got.min()) >= 1 and int(got.max()) <= n
        rest, far, rep = rank[at + n_own:int(c.tptr[q + 1])], len(FAR) + 1, min(3, n_own)
        assert rest.numel() == far + rep + 2 * min(n, 2)
        assert bool((rest[:far] == 0).all())                             # negative, beyond int32, below every id
        assert torch.equal(rest[far:far + rep], got[:rep])               # a repeated target: the same answer
        assert bool((rest[far + rep:] == 0).all())                       # just below the first id, just above the last, in the gap
    assert torch.equal(c.pos.cpu() == -1, rank == 0)
    assert int((c.want_rank == 0).sum()) > 90 and int(c.want_rank.max()) > 60000


@pytest.mark.parametrize("k", [1, 64, 65, 128])
def test_kernel_agrees_with_the_topk_on_the_device(case, k):
    """rank <= k and "``segment_topk(k)`` lists it at that place" are one statement."""
    from ocn_amd import ops
    c = case
    scores, ptr, _, tptr, _ = c.dev
    _, top_pos = ops.segment_topk(scores, ptr, k)
    seg = torch.repeat_interleave(torch.arange(len(SEGMENTS), device=DEV), tptr[1:] - tptr[:-1])
    hit, miss = (c.rank >= 1) & (c.rank <= k), c.rank > k
    assert int(hit.sum()) >= 8 and int(miss.sum()) > 1000
    assert torch.equal(top_pos[seg[hit], c.rank[hit] - 1], c.pos[hit])
    assert not bool((top_pos[seg[miss]] == c.pos[miss][:, None]).any())


def test_wrapper_on_the_device(case):
    from ocn_amd import ops
    scores, ptr, edges, tptr, tnode = case.dev
    with pytest.raises(TypeError, match="scores: expected"):
        ops.segment_rank(scores.double(), ptr, edges, tptr, tnode)
    with pytest.raises(TypeError, match="tnode: expected"):
        ops.segment_rank(scores, ptr, edges, tptr, tnode.int())
    with pytest.raises(ValueError, match="tptr: one target list per segment"):
        ops.segment_rank(scores, ptr, edges, tptr[:-1], tnode)
    zero = torch.zeros(1, dtype=torch.int64, device=DEV)
    rank, pos = ops.segment_rank(scores[:0], zero, edges[:0], zero, tnode[:0])                    # Q = 0, P = 0
    assert rank.shape == (0,) and pos.shape == (0,) and rank.dtype == torch.int64
    rank, pos = ops.segment_rank(scores, ptr, edges, torch.zeros_like(tptr), tnode[:0])          # P = 0
    assert rank.shape == (0,) and pos.shape == (0,)
    three = torch.tensor([0, 2, 2, 3], device=DEV)
    rank, pos = ops.segment_rank(scores[:0], torch.zeros(4, dtype=torch.int64, device=DEV), edges[:0], three, tnode[:3])   # T = 0
    assert rank.tolist() == [0, 0, 0] and pos.tolist() == [-1, -1, -1]


# ---- graphs ----------------------------------------------------------------------------------------------------------------------
def device_graph(ei, n):
    """Undirected edge list [2, m] -> (adj, A²) on the device."""
    from ocn_amd.sparse import SparseTensor
    ei = torch.cat([ei, ei.flip(0)], dim=1)
    adj = SparseTensor.from_edge_index(ei.to(DEV), sparse_sizes=(n, n))
    return adj, product_adj2(adj)


def ragged(lists):
    tptr = torch.tensor([0] + [len(t) for t in lists], dtype=torch.int64).cumsum(0)
    return tptr.to(DEV), src_tensor([t for ts in lists for t in ts])


def test_closed_forms_path_and_star(hiplib):
    from ocn_amd import ranking as K
    n = 12
    adj, adj2 = device_graph(torch.stack([torch.arange(n - 1), torch.arange(1, n)]), n)
    lists = [[i + 2, i - 2, i, i + 1, i + 3] for i in range(n)]         # out of range at the ends: simply not found
    for a2 in (adj2, None):
        res = K.rank_links_heuristic(adj, a2, src_tensor(range(n)), ragged(lists), 64, "cn")
        both = [2 <= i < n - 2 for i in range(n)]
        want = [[(2 if b else 1) if i + 2 < n else 0, 1 if i >= 2 else 0, 0, 0, 0] for i, b in enumerate(both)]   # the tie goes to i - 2
        assert res.rank.view(n, 5).tolist() == want
        assert res.n_cand.tolist() == [(i >= 2) + (i + 2 < n) for i in range(n)] and res.retrieval_rank is None and res.m is None
    leaves = 300                                                         # centre 0, leaves 1 .. 300: every other leaf ties at cn = 1
    adj, adj2 = device_graph(torch.stack([torch.zeros(leaves, dtype=torch.int64), torch.arange(1, leaves + 1)]), leaves + 1)
    everyone = list(range(leaves, -1, -1))                               # descending: targets come in any order
    res = K.rank_links_heuristic(adj, adj2, src_tensor([7, 0, 300]), ragged([everyone, everyone, everyone]), 64, "cn")
    rank = res.rank.view(3, leaves + 1).flip(1)                          # column t = node t
    assert rank[0].tolist() == [0] + list(range(1, 7)) + [0] + list(range(7, leaves))            # the centre is a link, 7 is the source
    assert rank[1].tolist() == [0] * (leaves + 1)                        # the centre has no candidates
    assert rank[2].tolist() == [0] + list(range(1, leaves)) + [0]
    assert res.n_cand.tolist() == [leaves - 1, 0, leaves - 1]
    met = K.ranking_metrics(res, ks=(10, 299, 1000))
    assert met["n_eval"] == 3 and met["pair_hits@299"] == met["coverage"] == 2 * 299 / (3 * 301) and met["hit_rate@10"] == 2 / 3
    assert met["mrr"] == 2 / 3 and met["pair_hits@1000"] == met["coverage"] and met["pair_hits@10"] == 20 / (3 * 301)


# ---- end to end without a model --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prop(hiplib):
    """The hubbed Chung-Lu graph of ``tests/test_recommend_gpu.prop``, built again: 1 500 nodes, 5 of them isolated, a hand-added
    hub of 700 spokes, and 256 sources — the hub, the isolated nodes, repeats.  ``truth``: per distinct source up to six true
    candidates, two existing links, the source itself, and four nodes drawn from the whole graph (the isolated ones among
    them: beyond any number of hops)."""
    from ocn_amd.sparse import SparseTensor
    n, iso, hub = 1500, 5, 3
    base = make_graph(n, 8, 400, 21, isolated=iso)
    g = torch.Generator().manual_seed(6)
    spokes = torch.randperm(n - iso, generator=g)[:700]
    spokes = spokes[spokes != hub]
    ei = torch.cat([torch.stack([base.row, base.col]), torch.stack([torch.full_like(spokes, hub), spokes])], dim=1)
    oadj = O.to_symmetric(O.from_edge_index(ei, n))
    oadj2 = O.adj2_sparse(oadj)
    adj = to_product(oadj, DEV)
    adj2 = product_adj2(adj)
    rnd = torch.randint(0, n, (256 - 1 - iso - 20,), generator=g).tolist()
    sources = [hub] + list(range(n - iso, n)) + rnd
    sources = sources[:40] + sources[10:30] + sources[40:]               # twenty repeats
    assert len(sources) == 256 and len(set(sources)) < 256

    def rows(m):
        rp, col = m.rowptr().tolist(), m.col.tolist()
        return [set(col[rp[r]:rp[r + 1]]) for r in range(m.n_rows)]
    a_rows, a2_rows = rows(oadj), rows(oadj2)
    rng = np.random.default_rng(8)
    t_rows = {}
    for s in sorted(set(sources)):
        cand = sorted(a2_rows[s] - a_rows[s] - {s})
        t = set(rng.choice(cand, size=min(6, len(cand)), replace=False).tolist()) if cand else set()
        t |= set(sorted(a_rows[s])[:2]) | {s} | set(rng.integers(0, n, 3).tolist()) | {n - 1 - int(rng.integers(0, iso))}
        t_rows[s] = sorted(t)
    pairs = torch.tensor([(s, t) for s, ts in t_rows.items() for t in ts], dtype=torch.int64).t()
    truth = SparseTensor.from_edge_index(pairs.to(DEV), sparse_sizes=(n, n))
    lists = [t_rows[s] for s in sources]
    return SimpleNamespace(n=n, hub=hub, adj=adj, adj2=adj2, sources=sources, a_rows=a_rows, a2_rows=a2_rows, truth=truth, lists=lists)


def check_against_topk(res, dst, k):
    """A target is in ``dst[q, :k]`` exactly when ``1 <= rank <= k``, and then ``dst[q, rank - 1]`` is the target."""
    Q = res.sources.numel()
    seg = torch.repeat_interleave(torch.arange(Q, device=DEV), res.tptr[1:] - res.tptr[:-1])
    hit = (res.rank >= 1) & (res.rank <= k)
    listed = (dst[seg] == res.target[:, None]).any(1)
    assert torch.equal(listed, hit)
    assert torch.equal(dst[seg[hit], res.rank[hit] - 1], res.target[hit])
    return int(hit.sum())


def is_candidate(res, ptr, edges, n):
    """Per target: is (its segment, the node) a pair of the candidate list (ptr, edges)?"""
    Q = res.sources.numel()
    seg_e = torch.repeat_interleave(torch.arange(Q, device=DEV), ptr[1:] - ptr[:-1])
    seg_t = torch.repeat_interleave(torch.arange(Q, device=DEV), res.tptr[1:] - res.tptr[:-1])
    return torch.isin(seg_t * n + res.target, seg_e * n + edges[:, 1])


@pytest.mark.parametrize("hops", [2, 3])
@pytest.mark.parametrize("kind", ["cn", "ra"])
def test_rank_links_heuristic_against_recommend_links_heuristic(prop, kind, hops):
    from ocn_amd import ranking as K, recommend as R
    c = prop
    src = src_tensor(c.sources)
    bs = 1 << 20
    res = K.rank_links_heuristic(c.adj, c.adj2, src, c.truth, bs, kind, hops=hops)
    tptr, tnode = ragged(c.lists)                                        # the matrix, gathered: row s per occurrence of s, ascending
    assert torch.equal(res.tptr, tptr) and torch.equal(res.target, tnode) and torch.equal(res.sources, src)
    again = K.rank_links_heuristic(c.adj, c.adj2, src, (tptr, tnode), bs, kind, hops=hops)        # ... or handed in ready
    assert torch.equal(again.rank, res.rank) and torch.equal(again.n_cand, res.n_cand)
    ptr, edges = R.two_hop_candidates(c.adj, c.adj2, src) if hops == 2 else R.three_hop_candidates(c.adj, src)
    assert torch.equal(res.n_cand, ptr[1:] - ptr[:-1])
    cand = is_candidate(res, ptr, edges, c.n)
    assert torch.equal(res.rank > 0, cand)                               # links, the source itself, nodes out of reach: rank 0
    assert int(cand.sum()) > 500 and int((~cand).sum()) > 500
    if hops == 3:
        p2, e2 = R.two_hop_candidates(c.adj, c.adj2, src)
        assert int((cand & ~is_candidate(res, p2, e2, c.n)).sum()) > 50                           # truth holds nodes beyond two hops
    hits = []
    for k in (1, 7, 128):
        dst, _ = R.recommend_links_heuristic(c.adj, c.adj2, src, k, bs, kind, hops=hops)
        hits.append(check_against_topk(res, dst, k))
    assert 0 < hits[0] <= hits[1] <= hits[2] < int(cand.sum()) and hits[0] < hits[2]             # ranks beyond 128: what the top-k cannot say
    if hops == 2 and kind == "ra":
        walk = K.rank_links_heuristic(c.adj, None, src, c.truth, bs, kind)                        # a 1-hop kind never reads A²
        assert torch.equal(walk.rank, res.rank) and torch.equal(walk.n_cand, res.n_cand)
        with pytest.raises(IndexError):
            K.rank_links_heuristic(c.adj, c.adj2, torch.tensor([0, c.n], device=DEV), c.truth, bs, kind)
        none = K.rank_links_heuristic(c.adj, c.adj2, src[:0], c.truth, bs, kind)
        assert none.rank.shape == (0,) and none.tptr.tolist() == [0] and none.n_cand.shape == (0,)


# ---- with a model ----------------------------------------------------------------------------------------------------------------
def cn5(H):
    from ocn_amd.model import predictor_dict
    torch.manual_seed(12)
    pred = predictor_dict["cn5"](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()      # LayerNorm on
    with torch.no_grad():
        pred.innerprod.fill_(0.37)
    return pred


CASES = [("pattern", False, None, 2), ("pattern", False, ("ra", 16), 2), ("pattern", False, ("ra", 16, 0.5), 3),
         ("pattern", True, None, 2), ("pattern", True, ("ra", 16), 2), ("pattern", True, ("ra", 16, 0.5), 3),
         ("walk", False, ("ra", 16), 2)]


@pytest.mark.parametrize("route,frozen,prefilter,hops", CASES,
                         ids=[f"{r}{'_frozen' if f else ''}_{'full' if p is None else 'short'}_hops{h}" for r, f, p, h in CASES])
def test_rank_links_against_recommend_links(prop, monkeypatch, route, frozen, prefilter, hops):
    """cn5 with LayerNorm at the smallest hidden width, innerprod = 0.37: the invariant of the heuristic test against
    ``recommend_links`` with identical arguments; with a short list, the retrieval rank against ``prefilter_candidates``."""
    from ocn_amd import ops, ranking as K, recommend as R
    from ocn_amd.frozen import freeze_columns
    c = prop
    H, Q, bs = 16, 64, 4096
    pred = cn5(H)
    h = torch.randn(c.n, H, generator=torch.Generator().manual_seed(3)).to(DEV)
    a2 = c.adj2 if route == "pattern" else None
    src = src_tensor(c.sources[:Q])                                      # the hub, the isolated nodes, repeats among them
    truth = ragged(c.lists[:Q])
    if frozen:
        ref = torch.randint(0, c.n - 5, (600, 2), generator=torch.Generator().manual_seed(1)).to(DEV)
        pred.set_frozen_columns(freeze_columns(pred, c.adj, a2, ref))
    try:
        res = K.rank_links(pred, h, c.adj, a2, src, truth, bs, prefilter=prefilter, hops=hops)
        assert torch.equal(res.tptr, truth[0]) and torch.equal(res.target, truth[1])
        m = None if prefilter is None else prefilter[1]
        assert res.m == m
        hits = []
        for k in (1, 7, 128 if m is None else m):
            dst, _ = R.recommend_links(pred, h, c.adj, a2, src, k, bs, prefilter=prefilter, hops=hops)
            hits.append(check_against_topk(res, dst, k))
        assert hits[0] <= hits[1] <= hits[2] and hits[2] > 0
        if prefilter is None:
            ptr, edges = R.two_hop_candidates(c.adj, a2, src)
            assert res.retrieval_rank is None and torch.equal(res.n_cand, ptr[1:] - ptr[:-1])
            assert torch.equal(res.rank > 0, is_candidate(res, ptr, edges, c.n))
            assert int(res.rank.max()) > 128
            return
        decay = None if hops == 2 else prefilter[2]
        ptr_m, edges_m = R.prefilter_candidates(c.adj, src, "ra", m, hops=hops, decay=decay)
        kept = is_candidate(res, ptr_m, edges_m, c.n)
        rr = res.retrieval_rank
        assert torch.equal(res.n_cand, ptr_m[1:] - ptr_m[:-1])
        assert torch.equal(kept, (rr >= 1) & (rr <= m))                  # in the short list exactly when the heuristic ranked it there
        assert torch.equal(res.rank > 0, kept)
        assert int(kept.sum()) > 0 and int((rr > m).sum()) > 20 and int((rr == 0).sum()) > 20      # ranked, dropped, out of reach: all occur
        ptr, edges = R.two_hop_candidates(c.adj, None, src) if hops == 2 else R.three_hop_candidates(c.adj, src)
        assert torch.equal(rr > 0, is_candidate(res, ptr, edges, c.n))
        alone = K.rank_path_index(c.adj, src, truth, "ra", hops, decay=decay)
        assert torch.equal(alone.rank, rr) and torch.equal(alone.n_cand, ptr[1:] - ptr[:-1]) and alone.retrieval_rank is None
        met = K.ranking_metrics(res, ks=(5, 16))
        assert met["retention"] == int(kept.sum()) / int((rr > 0).sum()) and met["coverage"] == int((rr > 0).sum()) / rr.numel()
        assert met["pair_hits@16"] == int(kept.sum()) / rr.numel() and met["m"] == 16            # (a short list of 16: every rank is <= 16)
        if hops == 3:                                                    # the chunk loop: at least three chunks, and one
            count = ptr[1:] - ptr[:-1]
            small = int(count.sum()) // 4
            assert len(list(R._budget_chunks(count, small))) >= 3 and len(list(R._budget_chunks(count, 1 << 40))) == 1
            for budget in (small, 1 << 40):
                one = K.rank_path_index(c.adj, src, truth, "ra", 3, decay=decay, budget=budget)
                assert torch.equal(one.rank, rr) and torch.equal(one.n_cand, alone.n_cand), budget
                monkeypatch.setattr(ops, "prefilter_budget", budget)
                two = K.rank_links(pred, h, c.adj, a2, src, truth, bs, prefilter=prefilter, hops=3)
                assert torch.equal(two.rank, res.rank) and torch.equal(two.retrieval_rank, rr) and torch.equal(two.n_cand, res.n_cand), budget
    finally:
        pred.set_frozen_columns(None)
    with pytest.raises(RuntimeError, match="eval path"):
        K.rank_links(pred.train(), h, c.adj, a2, src, truth, bs, prefilter=prefilter, hops=hops)


def test_example_driver_evaluates(hiplib, capsys):
    """examples/run_like_reference.py --recommend 5 --recommend-eval 40 on the Cora shape: a heuristic, and a frozen cn5 with a
    short list beside its unfiltered run."""
    import importlib.util
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "run_like_reference.py")
    spec = importlib.util.spec_from_file_location("run_like_reference", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    line = (r"^recommend-eval {}: (\d+) sources, (\d+) pairs, coverage ([\d.]+){} mrr ([\d.]+)  recall/ndcg/hit@5 [\d.]+/[\d.]+/[\d.]+  "
            r"recall/ndcg/hit@10 [\d.]+/[\d.]+/[\d.]+  recall/ndcg/hit@50 [\d.]+/[\d.]+/[\d.]+  recall/ndcg/hit@100 [\d.]+/[\d.]+/[\d.]+$")
    mod.main(["--dataset", "cora", "--heuristic", "ra", "--recommend", "5", "--recommend-eval", "40"])
    out = capsys.readouterr().out
    got = re.search(line.format("ra over 2 hops", ""), out, re.M)
    assert got, out[-2000:]
    assert int(got.group(1)) == 40 and int(got.group(2)) >= 40 and 0 < float(got.group(3)) <= 1 and 0 < float(got.group(4)) <= 1
    mod.main(["--dataset", "cora", "--epochs", "1", "--recommend", "5", "--recommend-frozen", "--recommend-prefilter", "ra:32",
              "--recommend-eval", "40"])
    out = capsys.readouterr().out
    short = re.search(line.format(re.escape("cn5 over 2 hops prefilter ra:32"), r" retention ([\d.]+)"), out, re.M)
    full = re.search(line.format("cn5 over 2 hops unfiltered", ""), out, re.M)
    assert short and full, out[-2000:]
    assert short.group(1, 2, 3) == full.group(1, 2, 3) and 0 < float(short.group(4)) <= 1      # the same pairs, the same coverage
    for bad in (["--recommend-eval", "40"], ["--recommend", "5", "--recommend-eval", "-1"]):
        with pytest.raises(SystemExit):
            mod.main(["--dataset", "cora"] + bad)
    capsys.readouterr()


# ---- metrics ---------------------------------------------------------------------------------------------------------------------
def test_metrics_of_a_device_result_equal_those_of_the_restatement(case):
    from ocn_amd.ranking import RankResult, ranking_metrics
    c = case
    Q = len(SEGMENTS)
    n_cand = c.ptr[1:] - c.ptr[:-1]
    dev = RankResult(torch.arange(Q, device=DEV), c.dev[3], c.dev[4], n_cand.to(DEV), c.rank)
    host = RankResult(torch.arange(Q), c.tptr, c.tnode, n_cand, c.want_rank)
    ks = (1, 10, 100, 5000, 100000)
    got, want = ranking_metrics(dev, ks), ranking_metrics(host, ks)
    assert got == want and got["n_eval"] == sum(1 for _, mode in SEGMENTS if mode != "none")
    assert 0 < got["recall@10"] < got["recall@100"] < got["recall@100000"] and 0 < got["ndcg@10"] <= 1 and 0 < got["mrr"] <= 1
    assert got["pair_hits@100000"] == got["coverage"] == int((c.want_rank > 0).sum()) / c.tnode.numel()
    moved = dev.to("cpu")
    assert not moved.rank.is_cuda and torch.equal(moved.rank, c.want_rank) and ranking_metrics(moved, ks) == want
