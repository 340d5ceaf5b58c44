"""Random-walk retrieval on the GPU (``ocn_rw_visits_count`` / ``_fill``; ocn_amd/recommend.py: ``random_walk_candidates``,
``random_walk_short_list``, ``RandomWalks`` as a ``prefilter``) against the CPU mirror of tests/rw_mirror.py.  A walk is fixed
bit for bit by (seed, source, walk index, adj), a count is an integer and ``val`` two fp32 roundings of integers, so every
comparison is ``torch.equal`` — ``val`` by its bit pattern."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import rw_mirror as RM
from tests import two_hop_sampling_mirror as TM
from tests.helpers import make_graph, product_adj2, to_product

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEED = (0x5EED << 32) | 0x4321           # both key words in use
DECAY = 0.3                              # not a power of two: the product rounds
WALKS = (1, 63, 64, 65, 255, 256, 257, 1024)       # around a wave and a workgroup of walks, several rounds of four per thread


def on_gpu(n, rowptr, col):
    from ocn_amd.sparse import SparseTensor
    return SparseTensor(rowptr=torch.from_numpy(rowptr).to(DEV), col=torch.from_numpy(col).to(DEV), sparse_sizes=(n, n))


def case(n, rows, sources, known_rows=None):
    rowptr, col = TM.csr_of(n, rows)
    c = SimpleNamespace(n=n, rowptr=rowptr, col=col, adj=on_gpu(n, rowptr, col), src=[int(s) for s in sources],
                        k_rowptr=None, k_col=None, known=None)
    if known_rows is not None:
        c.k_rowptr, c.k_col = TM.csr_of(n, known_rows)
        c.known = on_gpu(n, c.k_rowptr, c.k_col)
    return c


def of_adj(adj, sources):
    """A case around a SparseTensor that is on the device already: its CSR is the input, read back for the mirror."""
    return SimpleNamespace(n=adj.size(0), rowptr=adj._rowptr.cpu().numpy(), col=adj._col.cpu().numpy(), adj=adj,
                           src=[int(s) for s in sources], k_rowptr=None, k_col=None, known=None)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def src_tensor(sources):
    return torch.tensor(list(sources), dtype=torch.int64, device=DEV)


def mirror(c, walks, length, seed=SEED, src=None):
    ptr, edges, val, vis = RM.visits(c.rowptr, c.col, c.src if src is None else src, walks, length, seed,
                                     DECAY if length == 3 else None, c.k_rowptr, c.k_col)
    return torch.from_numpy(ptr), torch.from_numpy(edges), torch.from_numpy(val), torch.from_numpy(vis)


def device(c, walks, length, seed=SEED, src=None):
    from ocn_amd import recommend as R
    ptr, edges, val, vis = R.random_walk_candidates(c.adj, src_tensor(c.src if src is None else src), walks, length,
                                                    DECAY if length == 3 else None, c.known, seed)
    assert ptr.dtype == torch.int64 and edges.dtype == torch.int64 and val.dtype == torch.float32 and vis.dtype == torch.int32
    assert edges.shape == (int(ptr[-1]), 2) and vis.shape == edges.shape and val.shape == (edges.shape[0],)
    return ptr.cpu(), edges.cpu(), val.cpu(), vis.cpu()


def same(got, want, what=None):
    assert torch.equal(got[0], want[0]), ("ptr", what)
    assert torch.equal(got[1], want[1]), ("edges", what)
    assert torch.equal(got[3], want[3]), ("visits", what)
    assert torch.equal(bits(got[2]), bits(want[2])), ("val", what)


def check(c, walks, length, seed=SEED, src=None):
    want = mirror(c, walks, length, seed, src)
    same(device(c, walks, length, seed, src), want, (walks, length, seed))
    return want


# ---- graphs ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hands(hiplib):
    return [case(n, rows, range(n)) for _, n, rows, _ in TM.hand_cases()]


@pytest.fixture(scope="module")
def chung_lu(hiplib):
    """About 300 nodes under a power law, the last three without an edge; sources: the hub, light nodes, an isolated one, a
    repeat."""
    adj = to_product(make_graph(300, 8, 60, seed=11, isolated=3), DEV)
    deg = (adj._rowptr[1:] - adj._rowptr[:-1]).cpu()
    hub, light = int(deg.argmax()), [int(v) for v in torch.nonzero(deg == 1).flatten()[:2]]
    assert int(deg[hub]) >= 30 and len(light) == 2 and int(deg[299]) == 0
    return of_adj(adj, [hub, 5, 17] + light + [299, 120, 5, 250, 33])


@pytest.fixture(scope="module")
def directed(hiplib):
    """n = 97, directed: random rows of 1 .. 4 columns, empty rows (dead ends: a walk that enters one stops early), a stored
    self-loop, a row that leads only into dead ends."""
    n = 97
    rng = np.random.default_rng(97)
    rows = {s: sorted(rng.choice(n, size=int(rng.integers(1, 5)), replace=False).tolist()) for s in range(n)}
    for dead in (0, 7, 8, 9, 40, 41, 96):
        rows.pop(dead)
    rows[2] = [2, 40, 96]                # itself, and two dead ends
    rows[3] = [7, 8, 9]                  # every walk from 3 stops after its first step: nothing is ever counted
    rows[4] = [3, 50]                    # through 3 the second step is counted and the third does not exist
    c = case(n, rows, [2, 3, 4, 0, 10, 50, 60, 95, 10])
    reach = [len(RM.source_segment(c.rowptr, c.col, s, 256, 3, SEED, DECAY)) for s in (3, 0)]
    assert reach == [0, 0]
    return c


@pytest.fixture(scope="module")
def caterpillar(hiplib):
    """s = 0 - m = 1, and m with 6 000 leaves: a 6 001-entry row under the multiply-high, and at length 2 nearly every walk
    from s ends in a leaf of its own."""
    n = 6002
    return case(n, TM.undirected(n, [(0, 1)] + [(1, leaf) for leaf in range(2, n)]), [0, 1, 4000])


# ---- 1. the visits, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [2, 3])
@pytest.mark.parametrize("walks", WALKS)
def test_visits_equal_the_mirror(hands, chung_lu, directed, walks, length):
    for c in (*hands, chung_lu, directed):
        check(c, walks, length)


@pytest.mark.parametrize("length", [2, 3])
def test_the_largest_walk_count(hands, chung_lu, length):
    from ocn_amd import ops
    W = ops.rw_max_walks()
    assert 1024 <= W <= 65535
    check(hands[2], W, length, src=[0, 3])
    ptr, _, _, vis = check(chung_lu, W, length, src=chung_lu.src[:4])
    assert int(vis.sum()) > W                                # (the counts are no handful)


def test_hand_answers(hands):
    """K(3,4), source 0, 2048 walks of 3 steps: the counts pinned in the contract, through the device."""
    k34 = hands[2]
    for seed, c2 in ((0, {1: 696, 2: 658}), (7, {1: 656, 2: 695})):
        ptr, edges, val, vis = device(k34, 2048, 3, seed, src=[0])
        assert ptr.tolist() == [0, 2] and edges.tolist() == [[0, 1], [0, 2]]
        assert vis.tolist() == [[c2[1], 0], [c2[2], 0]] and val.tolist() == [float(c2[1]), float(c2[2])]
    star = hands[1]                                          # the centre: every neighbour is a leaf, every visit is excluded
    ptr, edges, _, _ = device(star, 256, 3, src=[0, 0])
    assert ptr.tolist() == [0, 0, 0] and edges.shape == (0, 2)


@pytest.mark.parametrize("walks", [1024, 2048])
def test_caterpillar_fills_the_table(caterpillar, walks):
    """W walks over 6 001 equally likely second steps visit about 6 001 · (1 - exp(-W / 6 001)) distinct nodes: 0.92 W at
    W = 1 024 and 0.85 W at 2 048, so nearly every walk claims a slot of its own.  (At the largest W, 3 968, the share is 0.73:
    that case is compared with the mirror below, without this bound.)"""
    c = caterpillar
    want = check(c, walks, 2)
    distinct = int(want[0][1] - want[0][0])                  # source 0: its visited leaves (m is excluded, s dropped)
    assert distinct >= 0.8 * walks, (distinct, walks)
    assert int(want[1][:distinct, 1].max()) > 5000           # (ranks near the end of the 6 001-entry row)
    check(c, walks, 3)


def test_caterpillar_at_the_largest_walk_count(caterpillar):
    from ocn_amd import ops
    for length in (2, 3):
        check(caterpillar, ops.rw_max_walks(), length)


# ---- 2. sources ----------------------------------------------------------------------------------------------------------
def test_sources_stand_alone(chung_lu):
    """Degree 0: an empty segment.  A repeated source: the same segment twice.  Another order, other company: every source keeps
    its segment."""
    c = chung_lu
    for length in (2, 3):
        ptr, edges, val, vis = device(c, 256, length)
        seg = {}
        for q, s in enumerate(c.src):
            a, b = int(ptr[q]), int(ptr[q + 1])
            this = (edges[a:b, 1].tolist(), bits(val[a:b]).tolist(), vis[a:b].tolist())
            assert seg.setdefault(s, this) == this           # the repeat of 5
            assert (b - a == 0) == (s == 299)
        order = list(reversed(c.src)) + [44]
        ptr2, edges2, val2, vis2 = device(c, 256, length, src=order)
        for q, s in enumerate(order[:-1]):
            a, b = int(ptr2[q]), int(ptr2[q + 1])
            assert (edges2[a:b, 1].tolist(), bits(val2[a:b]).tolist(), vis2[a:b].tolist()) == seg[s], s
        same((ptr2, edges2, val2, vis2), mirror(c, 256, length, src=order))


def test_no_query(chung_lu):
    from ocn_amd import ops, recommend as R
    c = chung_lu
    ptr, edges, val, vis = R.random_walk_candidates(c.adj, src_tensor([]), 64, 3, 0.5)
    assert ptr.tolist() == [0] and edges.shape == (0, 2) and val.shape == (0,) and vis.shape == (0, 2)
    p, e = R.random_walk_short_list(c.adj, src_tensor([]), R.RandomWalks(4, 64, 2))
    assert p.tolist() == [0] and e.shape == (0, 2)
    count = ops.rw_visits_count(c.adj._rowptr, c.adj._col, c.adj._rowptr, c.adj._col, src_tensor([]), 64, 2, 0)
    assert count.shape == (0,) and count.dtype == torch.int32


@pytest.mark.parametrize("seed", [0, 1, (1 << 64) - 1])
def test_seeds(chung_lu, directed, seed):
    a = check(chung_lu, 257, 3, seed)
    check(directed, 257, 2, seed)
    assert not torch.equal(a[3], mirror(chung_lu, 257, 3, SEED)[3])       # (the seed does move the walks)


def test_known_is_not_adj(hiplib):
    """``known`` with rows of its own: a superset of A's row, a disjoint row, an empty one."""
    n = 40
    rng = np.random.default_rng(5)
    pairs = [(int(x), int(y)) for x, y in zip(*np.nonzero(np.triu(rng.random((n, n)) < 0.12, 1)))]
    rows = TM.undirected(n, pairs)
    known = {s: sorted(set(cols) | {(s + 3) % n, (s * 7) % n}) for s, cols in rows.items()}
    known[1] = [c for c in range(n) if c not in rows[1]][:25]
    known.pop(2)
    c = case(n, rows, [0, 1, 2, 3, 17, 39], known)
    for length in (2, 3):
        want = check(c, 512, length)
        plain = mirror(case(n, rows, c.src), 512, length)
        assert not torch.equal(want[0], plain[0])            # (the exclusion is not A's)
        a, b = int(want[0][2]), int(want[0][3])
        if length == 3:                                      # an empty row of known: a walk that returns to 2 then counts a neighbour
            assert set(rows[2]) & set(want[1][a:b, 1].tolist())


def test_two_streams_give_the_same_bits(chung_lu):
    from ocn_amd import recommend as R
    c = chung_lu
    src = src_tensor(c.src)
    want = mirror(c, 1024, 3)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(s1):
        a = R.random_walk_candidates(c.adj, src, 1024, 3, DECAY, seed=SEED)
    with torch.cuda.stream(s2):
        b = R.random_walk_candidates(c.adj, src, 1024, 3, DECAY, seed=SEED)
    torch.cuda.synchronize(DEV)
    same([t.cpu() for t in a], want)
    same([t.cpu() for t in b], want)


# ---- 3. the short list ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 5, 128])
def test_short_list_keeps_the_m_most_visited_in_ascending_id(chung_lu, m):
    from ocn_amd import recommend as R
    c = chung_lu
    for length, walks in ((2, 256), (3, 1024)):
        ptr, edges, val, _ = mirror(c, walks, length)
        sizes = ptr[1:] - ptr[:-1]
        ties = sum(len(set(val[ptr[q]:ptr[q + 1]].tolist())) < int(sizes[q]) for q in range(len(c.src)))
        assert ties >= 6 and int(sizes.max()) > 5            # integer counts: nearly every list holds equal values
        want_ptr, want_edges = RM.short_list(ptr.numpy(), edges.numpy(), val.numpy(), m)
        rw = R.RandomWalks(m, walks, length, DECAY if length == 3 else None, SEED)
        ptr_m, edges_m = R.random_walk_short_list(c.adj, src_tensor(c.src), rw)
        assert ptr_m.dtype == torch.int64 and edges_m.dtype == torch.int64
        assert torch.equal(ptr_m.cpu(), torch.from_numpy(want_ptr)) and torch.equal(edges_m.cpu(), torch.from_numpy(want_edges))
        assert torch.equal(ptr_m.cpu()[1:] - ptr_m.cpu()[:-1], sizes.clamp(max=m))
        for q in range(len(c.src)):                          # ascending id inside every segment
            seg = edges_m[int(ptr_m[q]):int(ptr_m[q + 1]), 1].tolist()
            assert seg == sorted(seg)


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [2, 3])
def test_recommend_and_rank_with_random_walks(chung_lu, length):
    """recommend_links(prefilter=RandomWalks) = the scoring loop over the mirror's retained list and the top k of it;
    rank_links: the retrieval rank is the place by the mirror's ``val`` among all visited candidates, and the model ranks exactly
    the targets the short list kept."""
    from ocn_amd import recommend as R
    from ocn_amd.model import predictor_dict
    from ocn_amd.pipeline import score_edges, score_edges_walk
    from ocn_amd.ranking import rank_links, ranking_metrics
    c = chung_lu
    H, k, m, bs, walks = 16, 4, 9, 30, 512
    torch.manual_seed(12)
    pred = predictor_dict["cn5"](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()
    h = torch.randn(c.n, H, generator=torch.Generator().manual_seed(3)).to(DEV)
    args = SimpleNamespace(sum=0.5)
    src = src_tensor(c.src)
    rw = R.RandomWalks(m, walks, length, DECAY if length == 3 else None, SEED)
    ptr, edges, val, _ = mirror(c, walks, length)
    sptr, sedges = (torch.from_numpy(t).to(DEV) for t in RM.short_list(ptr.numpy(), edges.numpy(), val.numpy(), m))
    assert sedges.shape[0] > 2 * bs and int((ptr[1:] - ptr[:-1]).max()) > m
    # the truth: per source three visited nodes (the best, one past the cut where there is one, the last) and one never visited
    tptr, tnode, want_rr = [0], [], []
    for q, s in enumerate(c.src):
        a, b = int(ptr[q]), int(ptr[q + 1])
        order = sorted(range(a, b), key=lambda i: (-float(val[i]), int(edges[i, 1])))
        picks = [int(edges[i, 1]) for i in ([order[0], order[min(m, b - a - 1)], order[-1]] if b > a else [])]
        visited = set(edges[a:b, 1].tolist())
        picks.append(next(v for v in range(c.n) if v not in visited))
        tnode += picks
        want_rr += RM.ranks(ptr.numpy(), edges.numpy(), val.numpy(), q, picks)
        tptr.append(len(tnode))
    truth = (torch.tensor(tptr, dtype=torch.int64, device=DEV), torch.tensor(tnode, dtype=torch.int64, device=DEV))
    assert max(want_rr) > m and min(want_rr) == 0
    for a2 in (product_adj2(c.adj), None):
        flat = score_edges(pred, h, c.adj, a2, sedges, bs, args) if a2 is not None else score_edges_walk(pred, h, c.adj, sedges, bs, args)
        want_dst, want_score = R._select(flat, sptr, sedges, k)
        dst, score = R.recommend_links(pred, h, c.adj, a2, src, k, bs, args, prefilter=rw, hops=length)
        assert torch.equal(dst, want_dst) and torch.equal(bits(score), bits(want_score)), a2 is None
        res = rank_links(pred, h, c.adj, a2, src, truth, bs, args, prefilter=rw, hops=length)
        assert res.m == m and res.retrieval_rank.tolist() == want_rr
        assert torch.equal(res.rank > 0, (res.retrieval_rank >= 1) & (res.retrieval_rank <= m))
        assert torch.equal(res.n_cand, sptr[1:] - sptr[:-1])
        hit = res.rank.cpu()
        for q in range(len(c.src)):                          # a kept target stands where recommend_links lists it
            for t, r in zip(tnode[tptr[q]:tptr[q + 1]], hit[tptr[q]:tptr[q + 1]].tolist()):
                if 1 <= r <= k:
                    assert int(dst[q, r - 1]) == t
        met = ranking_metrics(res, ks=(1, 5))
        visited_pairs = sum(r > 0 for r in want_rr)
        assert met["coverage"] == visited_pairs / len(want_rr) and met["m"] == m
        assert met["retention"] == sum(1 <= r <= m for r in want_rr) / visited_pairs


# ---- 5. the example driver -------------------------------------------------------------------------------------------------
def test_example_driver_with_a_random_walk_short_list(hiplib, capsys):
    """examples/run_like_reference.py --recommend 5 --recommend-frozen --recommend-rw 8:256:3:0.5 --recommend-hops 3
    --recommend-eval 50 on the Cora shape: the frozen self-check compares walk short lists with walk short lists and passes, the
    kept line and the two evaluation lines (walk stage with its retention, unfiltered) are printed."""
    import importlib.util
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "run_like_reference.py")
    spec = importlib.util.spec_from_file_location("run_like_reference", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(["--dataset", "cora", "--epochs", "1", "--recommend", "5", "--recommend-hops", "3", "--recommend-frozen",
              "--recommend-rw", "8:256:3:0.5", "--recommend-eval", "50"])
    out = capsys.readouterr().out
    assert "returns the same rows = True" in out
    kept = re.search(r"^prefilter random walks 8:256:3:0.5 kept (\d+) of the (\d+) unfiltered top-5 links \(the model ranked (\d+) of (\d+) "
                     r"candidates\)$", out, re.M)
    assert kept, out[-2000:]
    k, full, short, cands = map(int, kept.groups())
    assert 0 <= k <= full <= 25 and 0 < short <= 5 * 8 and short < cands
    assert len(re.findall(r"^recommend source \d+ top-5: ", out, re.M)) == 5
    ev = re.search(r"^recommend-eval cn5 over 3 hops prefilter random walks 8:256:3:0.5: \d+ sources, \d+ pairs, coverage (\d\.\d{4}) "
                   r"retention (\d\.\d{4}) ", out, re.M)
    assert ev, out[-2000:]
    assert re.search(r"^recommend-eval cn5 over 3 hops unfiltered: ", out, re.M)
    for bad in (["--recommend-rw", "8:256:2", "--recommend-prefilter", "ra:8"], ["--recommend-rw", "8:256:3:0.5"],
                ["--recommend-hops", "3", "--recommend-rw", "8:256:3"], ["--recommend-rw", "8:256:2:0.5"], ["--recommend-rw", "4:256:2"],
                ["--recommend-rw", "8:0:2"], ["--recommend-rw", "8:256"], ["--recommend-rw", "8:x:2"],
                ["--heuristic", "ra", "--recommend-rw", "8:256:2"]):
        with pytest.raises(SystemExit):
            mod.main(["--dataset", "cora", "--recommend", "5"] + bad)
    capsys.readouterr()
