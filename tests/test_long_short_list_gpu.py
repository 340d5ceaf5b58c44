"""Short lists beyond 128 through the recommendation layers (``recommend.PathSums``, ``prefilter_candidates_long``): a
constructed graph of 740 nodes whose sources have 2-hop lists well above 128, 200 and 256 — and ordinary ones below.  The
references are a torch restatement of the rule (sort by value descending and id ascending, keep ``m``, return ascending ids)
and the project's existing routes; lists and orders are exact, every such comparison is ``torch.equal``."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import close, product_adj2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, HUB_A, HUB_B = 740, 0, 1
ISOLATED = (8, 9)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def restate(ptr, edges, val, m):
    """Per source: order by (val descending, id ascending) — a stable descending sort of a list that ascends by id — keep the
    first ``m``, return them in ascending id."""
    ptr, edges, val = ptr.cpu(), edges.cpu(), val.cpu()
    out_ptr, keep = [0], []
    for q in range(ptr.numel() - 1):
        a, b = int(ptr[q]), int(ptr[q + 1])
        assert not bool(torch.isnan(val[a:b]).any())
        order = torch.sort(val[a:b], descending=True, stable=True).indices[:m]
        keep.append(order.sort().values + a)
        out_ptr.append(out_ptr[-1] + order.numel())
    keep = torch.cat(keep) if keep else torch.zeros(0, dtype=torch.int64)
    return torch.tensor(out_ptr, dtype=torch.int64), edges[keep]


def make_predictor(name, H, seed=12):
    from ocn_amd.model import predictor_dict
    torch.manual_seed(seed)
    return predictor_dict[name](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()


@pytest.fixture(scope="module")
def world(hiplib):
    """Hub 0 has the 300 leaves 10 .. 309, hub 1 the 500 leaves 200 .. 699; nodes 2 - 4 are joined to both hubs, 5 and 6 to hub 0,
    7 to hub 1, so their 2-hop lists hold about 700, 300 and 500 candidates in two or three tie classes; 1 400 random links among
    the leaves give the leaves and the hubs long lists of many different values; 8 and 9 are isolated; 700 .. 739 are a sparse
    component of their own with ordinary lists."""
    from ocn_amd import recommend as R
    from ocn_amd.sparse import SparseTensor
    rng = np.random.default_rng(41)
    a = np.zeros((N, N), dtype=bool)
    a[HUB_A, 10:310] = True
    a[HUB_B, 200:700] = True
    a[2:5, HUB_A] = a[2:5, HUB_B] = True
    a[5:7, HUB_A] = True
    a[7, HUB_B] = True
    x, y = rng.integers(10, 700, 1400), rng.integers(10, 700, 1400)
    a[x, y] = True
    a[700:740, 700:740] = np.triu(rng.random((40, 40)) < 0.1, 1)
    a = a | a.T
    np.fill_diagonal(a, False)
    r, c = np.nonzero(a)
    adj = SparseTensor.from_edge_index(torch.from_numpy(np.stack([r, c]).astype(np.int64)).to(DEV), sparse_sizes=(N, N))
    sources = [8, 2, 3, 4, 5, 6, 7, 0, 1, 15, 250, 9, 650, 33, 480, 2] + list(range(700, 716)) + [9]
    src = torch.tensor(sources, dtype=torch.int64, device=DEV)
    ptr, edges = R.two_hop_candidates(adj, None, src)
    sizes = (ptr[1:] - ptr[:-1]).cpu()
    assert int(sizes[1]) > 600 and 256 < int(sizes[4]) < 400 and int(sizes[6]) > 400          # both hubs, hub 0, hub 1
    assert int((sizes > 256).sum()) >= 12 and int(((sizes > 0) & (sizes < 128)).sum()) >= 10 and int((sizes == 0).sum()) == 3
    h = torch.randn(N, 64, generator=torch.Generator().manual_seed(3)).to(DEV)
    return SimpleNamespace(adj=adj, adj2=product_adj2(adj), sources=sources, src=src, sizes=sizes, h=h, args=SimpleNamespace(sum=0.5))


def test_two_hundred_best_by_ra_equal_the_restatement(world):
    from ocn_amd import recommend as R
    w = world
    for kind, m in (("ra", 200), ("aa", 256), ("cn", 129), ("ra", 600)):
        ptr, edges, val = R.two_hop_scored_candidates(w.adj, w.src, kind)
        want_ptr, want_edges = restate(ptr, edges, val, m)
        ptr_m, edges_m = R.prefilter_candidates_long(w.adj, w.src, R.PathSums(kind, m))
        assert ptr_m.dtype == torch.int64 and edges_m.dtype == torch.int64
        assert torch.equal(ptr_m.cpu(), want_ptr) and torch.equal(edges_m.cpu(), want_edges), (kind, m)
        assert torch.equal((ptr_m[1:] - ptr_m[:-1]).cpu(), w.sizes.clamp(max=m))
        assert int((w.sizes > m).sum()) >= 5                              # the list was cut
    p0, e0 = R.prefilter_candidates_long(w.adj, w.src[:0], R.PathSums("ra", 200))
    assert p0.tolist() == [0] and e0.shape == (0, 2)
    p1, e1 = R.prefilter_candidates_long(w.adj, torch.tensor(ISOLATED, device=DEV), R.PathSums("ra", 200))
    assert p1.tolist() == [0, 0, 0] and e1.shape == (0, 2)


def test_within_the_limit_it_is_the_tuple_stage(world):
    from ocn_amd import recommend as R
    w = world
    for kind, m in (("cn", 64), ("ra", 128), ("aa", 1)):
        old = R.prefilter_candidates(w.adj, w.src, kind, m)
        new = R.prefilter_candidates_long(w.adj, w.src, R.PathSums(kind, m))
        assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1]), (kind, m)


def test_recommend_links_scores_the_retained_list(world):
    """The contract sentence: the scores are exactly those ``score_edges`` gives the flat retained list at this batch size."""
    from ocn_amd import recommend as R
    from ocn_amd.pipeline import score_edges, score_edges_walk
    w = world
    k, bs, stage = 20, 1000, R.PathSums("ra", 200)
    pred = make_predictor("cn5", 64)
    ptr_m, edges_m = R.prefilter_candidates_long(w.adj, w.src, stage)
    assert edges_m.shape[0] > 2 * bs and edges_m.shape[0] % bs != 0      # several batches and a ragged last one
    for a2 in (w.adj2, None):
        flat = score_edges(pred, w.h, w.adj, a2, edges_m, bs, w.args) if a2 is not None else \
            score_edges_walk(pred, w.h, w.adj, edges_m, bs, w.args)
        want_dst, want_score = R._select(flat, ptr_m, edges_m, k)
        dst, score = R.recommend_links(pred, w.h, w.adj, a2, w.src, k, bs, w.args, prefilter=stage)
        assert dst.shape == (len(w.sources), k)
        assert torch.equal(dst, want_dst) and torch.equal(bits(score), bits(want_score)), a2 is None
        full_dst, _ = R.recommend_links(pred, w.h, w.adj, a2, w.src, k, bs, w.args)
        assert not torch.equal(dst, full_dst)                            # (the short list does change the request)


def test_a_list_that_keeps_everything_is_the_unfiltered_request(world):
    from ocn_amd import recommend as R
    w = world
    m = int(w.sizes.max())
    assert m > 600
    pred = make_predictor("cn5", 64)
    want_dst, want_score = R.recommend_links(pred, w.h, w.adj, w.adj2, w.src, 20, 1000, w.args)
    for stage in (R.PathSums("ra", m), R.PathSums("cn", 100000)):
        dst, score = R.recommend_links(pred, w.h, w.adj, w.adj2, w.src, 20, 1000, w.args, prefilter=stage)
        assert torch.equal(dst, want_dst) and torch.equal(bits(score), bits(want_score)), stage


def test_frozen_scores_of_retained_pairs_are_their_unfiltered_scores(world):
    """cn5 with frozen column weights: a retained pair's score is, within the frozen-scoring tolerance the existing prefilter
    tests use (``helpers.close``: 1e-5 absolute and relative), its score over the FULL candidate list."""
    from ocn_amd import recommend as R
    from ocn_amd.frozen import freeze_columns
    from ocn_amd.pipeline import score_edges
    w = world
    k, bs, stage = 20, 900, R.PathSums("ra", 200)
    pred = make_predictor("cn5", 64, seed=31)
    with torch.no_grad():
        pred.alpha.copy_(torch.tensor([0.4, -0.3, 0.1]))
        pred.innerprod.fill_(0.37)
    ptr, edges = R.two_hop_candidates(w.adj, w.adj2, w.src)
    ref = torch.randint(0, 700, (600, 2), generator=torch.Generator().manual_seed(1)).to(DEV)
    pred.set_frozen_columns(freeze_columns(pred, w.adj, w.adj2, ref))
    try:
        full = score_edges(pred, w.h, w.adj, w.adj2, edges, 4096)
        where = torch.full((N * N,), -1, dtype=torch.int64, device=DEV)
        where[edges[:, 0] * N + edges[:, 1]] = torch.arange(edges.shape[0], device=DEV)      # (a repeated source: any of its places)
        dst, score = R.recommend_links(pred, w.h, w.adj, w.adj2, w.src, k, bs, prefilter=stage)
        got = dst >= 0
        assert int(got.sum()) > 400 and torch.equal(got, torch.isfinite(score))
        at = where[(w.src[:, None] * N + dst.clamp(min=0))[got]]
        assert int(at.min()) >= 0
        err = (score[got] - full[at]).abs().max().item()
        print(f"frozen cn5, PathSums('ra', 200): max|score - unfiltered score| = {err:.3e} over {int(got.sum())} returned pairs")
        assert close(score[got], full[at])
    finally:
        pred.set_frozen_columns(None)


def test_three_hops_do_not_depend_on_the_budget(world):
    from ocn_amd import recommend as R
    from ocn_amd.pipeline import score_edges
    w = world
    stage = R.PathSums("ra", 200, 0.5)
    ptr, edges, val = R.path_scored_candidates(w.adj, w.src, "ra", 3, 0.5)
    sizes3 = (ptr[1:] - ptr[:-1]).cpu()
    assert int((sizes3 > 600).sum()) >= 10
    want_ptr, want_edges = restate(ptr, edges, val, 200)
    base = R.prefilter_candidates_long(w.adj, w.src, stage, hops=3)
    assert torch.equal(base[0].cpu(), want_ptr) and torch.equal(base[1].cpu(), want_edges)
    chunks = {budget: len(list(R._budget_chunks(sizes3, budget))) for budget in (1500, 1, int(sizes3.sum()))}
    assert 3 < chunks[1500] < chunks[1] <= len(w.sources) and chunks[int(sizes3.sum())] == 1
    for budget in chunks:                                                # several sources per chunk, one each, one chunk
        got = R.prefilter_candidates_long(w.adj, w.src, stage, hops=3, budget=budget)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), budget
    pred = make_predictor("cn5", 64)
    dst, _ = R.recommend_links(pred, w.h, w.adj, w.adj2, w.src, 20, 1000, w.args, prefilter=stage, hops=3)
    want_dst, _ = R._select(score_edges(pred, w.h, w.adj, w.adj2, base[1], 1000, w.args), base[0], base[1], 20)
    assert torch.equal(dst, want_dst)


def test_rank_links_ranks_exactly_what_the_long_list_kept(world):
    from ocn_amd import ranking, recommend as R
    w = world
    m = 200
    ptr, edges = R.two_hop_candidates(w.adj, None, w.src)
    p, ids = ptr.cpu().tolist(), edges[:, 1].cpu()
    rng = np.random.default_rng(9)
    tptr, tnode = [0], []
    for q, s in enumerate(w.sources):
        n = p[q + 1] - p[q]
        if n:
            tnode += ids[p[q] + rng.choice(n, min(n, 8), replace=False)].tolist()
        tnode.append(s)                                                  # the source itself: no candidate
        tptr.append(len(tnode))
    truth = (torch.tensor(tptr, device=DEV), torch.tensor(tnode, device=DEV))
    pred = make_predictor("cn5", 64)
    res = ranking.rank_links(pred, w.h, w.adj, w.adj2, w.src, truth, 1000, w.args, prefilter=R.PathSums("ra", m))
    rr = res.retrieval_rank
    assert res.m == m and rr is not None
    assert torch.equal(res.rank > 0, (rr >= 1) & (rr <= m))
    assert int((rr > m).sum()) > 20 and int(((rr >= 1) & (rr <= m)).sum()) > 50 and int((rr == 0).sum()) == len(w.sources)
    assert torch.equal((res.n_cand).cpu(), w.sizes.clamp(max=m))
    alone = ranking.rank_path_index(w.adj, w.src, truth, "ra", 2)
    assert torch.equal(alone.rank, rr)
    met = ranking.ranking_metrics(res, (20,))
    assert met["m"] == m and 0.0 < met["retention"] < 1.0


def test_a_union_with_a_long_stage_is_the_csr_union_of_the_lists(world):
    from ocn_amd import ops, recommend as R
    w = world
    long, short = R.PathSums("ra", 200), ("cn", 16)
    union = R._check_prefilter(R.ShortListUnion(long, short), 128)
    ptr, edges, rank = R._candidates(w.adj, w.adj2, w.src, None, 2, union)
    pa, ea = R.prefilter_candidates_long(w.adj, w.src, long)
    pb, eb = R.prefilter_candidates(w.adj, w.src, *short)
    want_ptr, want_col = ops.csr_union(pa, ea[:, 1].to(torch.int32).contiguous(), pb, eb[:, 1].to(torch.int32).contiguous())
    assert rank is None and torch.equal(ptr, want_ptr) and torch.equal(edges[:, 1], want_col.long())
    assert torch.equal(edges[:, 0], torch.repeat_interleave(w.src, ptr[1:] - ptr[:-1]))
    # two long stages: 300 by cn beside 200 by ra must add candidates wherever a source has 300
    both = R._check_prefilter(R.ShortListUnion(long, R.PathSums("cn", 300)), 128)
    ptr2, edges2, _ = R._candidates(w.adj, w.adj2, w.src, None, 2, both)
    pc, ec = R.prefilter_candidates_long(w.adj, w.src, R.PathSums("cn", 300))
    want_ptr2, want_col2 = ops.csr_union(pa, ea[:, 1].to(torch.int32).contiguous(), pc, ec[:, 1].to(torch.int32).contiguous())
    assert torch.equal(ptr2, want_ptr2) and torch.equal(edges2[:, 1], want_col2.long())
    assert int(((ptr2[1:] - ptr2[:-1]) > (pa[1:] - pa[:-1])).sum()) >= 10
    pred = make_predictor("cn5", 64)
    dst, _ = R.recommend_links(pred, w.h, w.adj, w.adj2, w.src, 128, 1000, w.args, prefilter=R.ShortListUnion(long, short))
    assert dst.shape == (len(w.sources), 128)


def test_example_driver_takes_a_long_short_list(hiplib, capsys):
    """examples/run_like_reference.py --recommend 5 --recommend-frozen --recommend-long ra:200 on the Cora shape: the stage is a
    ``PathSums``, the frozen self-check passes and the kept line is printed; --recommend-prefilter keeps its limit."""
    import importlib.util
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "run_like_reference.py")
    spec = importlib.util.spec_from_file_location("run_like_reference", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(["--dataset", "cora", "--epochs", "1", "--recommend", "5", "--recommend-frozen", "--recommend-long", "ra:200"])
    out = capsys.readouterr().out
    assert "returns the same rows = True" in out
    kept = re.search(r"^prefilter long ra:200 kept (\d+) of the (\d+) unfiltered top-5 links \(the model ranked (\d+) of (\d+) candidates\)$",
                     out, re.M)
    assert kept, out[-2000:]
    k, full, short, cands = map(int, kept.groups())
    assert 0 <= k <= full <= 25 and 0 < short <= cands
    for bad in (["--recommend-long", "ra:4"], ["--recommend-long", "jaccard:300"], ["--recommend-long", "ra:300:0.5"],
                ["--recommend-long", "ra:300", "--recommend-prefilter", "ra:32"], ["--recommend-prefilter", "ra:200"]):
        with pytest.raises(SystemExit):
            mod.main(["--dataset", "cora", "--recommend", "5"] + bad)
    capsys.readouterr()
