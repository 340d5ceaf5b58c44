"""Link recommendation on the GPU (ocn_amd/recommend.py on ``ocn_row_diff_count`` / ``_fill`` and ``ocn_segment_topk``) against
restatements written here: the candidate sets with Python sets over the oracle's CSRs, the selection with
``numpy.lexsort((pos, -score, isnan))`` per segment.  Sets and orders are exact, so every comparison is ``torch.equal``
(values are compared as bit patterns: a NaN equals itself there, and the sign of a zero is part of what is returned)."""
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import ocn_oracle as O
from tests.helpers import make_graph, product_adj2, to_product

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatements --------------------------------------------------------------------------------------------------
def row_sets(m):
    """Row -> set of columns of an oracle SpM."""
    rp = m.rowptr().tolist()
    col = m.col.tolist()
    return [set(col[rp[r]:rp[r + 1]]) for r in range(m.n_rows)]


def ref_diff(p_rows, m_rows, sources, drop_self=True):
    """Per source, ascending: P[s] \\ M[s] (\\ {s}).  Returns (ptr [Q + 1], edges [T, 2])."""
    ptr, pairs = [0], []
    for s in sources:
        out = p_rows[s] - m_rows[s] - ({s} if drop_self else set())
        pairs += [(s, c) for c in sorted(out)]
        ptr.append(len(pairs))
    return torch.tensor(ptr, dtype=torch.int64), torch.tensor(pairs, dtype=torch.int64).reshape(-1, 2)


def ref_topk(scores, ptr, k):
    """Per segment the k first entries of the order {numbers before NaNs, higher score first (+0 == -0), lower position first}."""
    s = scores.numpy()
    p = ptr.tolist()
    Q = len(p) - 1
    val = torch.full((Q, k), float("-inf"), dtype=torch.float32)
    pos = torch.full((Q, k), -1, dtype=torch.int64)
    for q in range(Q):
        seg = s[p[q]:p[q + 1]]
        nan = np.isnan(seg)
        order = np.lexsort((np.arange(seg.size), -np.where(nan, np.float32(0), seg), nan))[:k]
        val[q, :order.size] = torch.from_numpy(seg[order].copy())
        pos[q, :order.size] = torch.from_numpy(order + p[q])
    return val, pos


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


def check_topk(scores, ptr, k):
    from ocn_amd import recommend as R
    val, pos = R.segment_topk(scores.to(DEV), ptr.to(DEV), k)
    rv, rp = ref_topk(scores, ptr, k)
    assert val.dtype == torch.float32 and pos.dtype == torch.int64 and val.is_cuda and pos.is_cuda
    assert torch.equal(pos.cpu(), rp), k
    assert same_bits(val, rv), k
    return val.cpu(), pos.cpu()


def ref_select(scores, ptr, edges, k):
    """(dst, score) of a recommendation from its flat scores."""
    val, pos = ref_topk(scores, ptr, k)
    dst = torch.where(pos >= 0, edges[:, 1][pos.clamp(min=0)], torch.full_like(pos, -1)) if edges.shape[0] else torch.full_like(pos, -1)
    return dst, val


# ---- graphs ------------------------------------------------------------------------------------------------------------
def device_graph(ei, n):
    """Undirected edge list [2, m] -> (adj, A²) on the device."""
    from ocn_amd.sparse import SparseTensor
    ei = torch.cat([ei, ei.flip(0)], dim=1)
    adj = SparseTensor.from_edge_index(ei.to(DEV), sparse_sizes=(n, n))
    return adj, product_adj2(adj)


def candidates_of(adj, adj2, sources, known=None):
    from ocn_amd import recommend as R
    ptr, edges = R.two_hop_candidates(adj, adj2, torch.tensor(sources, dtype=torch.int64, device=DEV), known)
    assert ptr.dtype == torch.int64 and edges.dtype == torch.int64 and edges.dim() == 2 and edges.shape[1] == 2
    p = ptr.tolist()
    e = edges.cpu()
    for q, s in enumerate(sources):
        assert bool((e[p[q]:p[q + 1], 0] == s).all())
    return [e[p[q]:p[q + 1], 1].tolist() for q in range(len(sources))]


@pytest.fixture(scope="module")
def prop(hiplib):
    """The Chung-Lu graph of ``tests.helpers.make_graph`` (1 500 nodes, 5 of them isolated) with a hand-added hub of 700 spokes —
    its adjacency row is longer than the kernel's LDS staging — and 256 sources: the hub, the isolated nodes, repeats."""
    from ocn_amd import ops
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
    deg = oadj.rowcount()
    assert int(deg.argmax()) == hub and int(deg[hub]) > ops.row_diff_stage_cols()      # searched in memory, not in LDS
    assert int((deg == 0).sum()) >= iso and 0 < int(deg[deg > 0].min()) <= 2           # ... beside rows of one or two entries
    rnd = torch.randint(0, n, (256 - 1 - iso - 20,), generator=g).tolist()
    sources = [hub] + list(range(n - iso, n)) + rnd
    sources = sources[:40] + sources[10:30] + sources[40:]                             # twenty repeats
    assert len(sources) == 256 and len(set(sources)) < 256
    a_rows, a2_rows = row_sets(oadj), row_sets(oadj2)
    ptr, edges = ref_diff(a2_rows, a_rows, sources)
    return SimpleNamespace(n=n, hub=hub, iso=iso, oadj=oadj, oadj2=oadj2, adj=adj, adj2=adj2, sources=sources,
                           a_rows=a_rows, a2_rows=a2_rows, ptr=ptr, edges=edges)


# ---- row difference ----------------------------------------------------------------------------------------------------
def test_closed_forms_path_star_and_bipartite(hiplib):
    n = 12
    adj, adj2 = device_graph(torch.stack([torch.arange(n - 1), torch.arange(1, n)]), n)
    got = candidates_of(adj, adj2, list(range(n)))
    assert got == [[c for c in (i - 2, i + 2) if 0 <= c < n] for i in range(n)]
    leaves = 300                                                         # centre 0, leaves 1 .. 300
    adj, adj2 = device_graph(torch.stack([torch.zeros(leaves, dtype=torch.int64), torch.arange(1, leaves + 1)]), leaves + 1)
    got = candidates_of(adj, adj2, [7, 0, 300, 1])
    assert got[0] == [c for c in range(1, leaves + 1) if c != 7] and len(got[0]) == 299        # > 64: the running base crosses chunks
    assert got[1] == []                                                  # A² row of the centre = {centre}: dropped as self
    assert got[2] == list(range(1, 300)) and got[3] == list(range(2, 301))
    m, r = 5, 7                                                          # K_{5,7}: left ids 0 .. 4
    left, right = torch.arange(m), torch.arange(m, m + r)
    adj, adj2 = device_graph(torch.stack([left.repeat_interleave(r), right.repeat(m)]), m + r)
    got = candidates_of(adj, adj2, [2, 0, m, m + r - 1])
    assert got[0] == [0, 1, 3, 4] and got[1] == [1, 2, 3, 4]
    assert got[2] == list(range(m + 1, m + r)) and got[3] == list(range(m, m + r - 1))


def test_candidates_equal_the_set_restatement(prop):
    """256 sources with repeats, isolated nodes and the hub (M row beyond the LDS staging, P row = nearly every node): the
    pairs, the offsets and the counts."""
    from ocn_amd import ops, recommend as R
    c = prop
    sizes = (c.ptr[1:] - c.ptr[:-1])
    assert int((sizes > 0).sum()) * 2 >= len(c.sources) and bool((sizes == 0).any())          # (no test on empty sets)
    assert int(sizes.max()) > 1000 and int((sizes > 64).sum()) >= 32                          # rows of many 64-column chunks
    src = torch.tensor(c.sources, dtype=torch.int64, device=DEV)
    ptr, edges = R.two_hop_candidates(c.adj, c.adj2, src)
    assert torch.equal(ptr.cpu(), c.ptr) and torch.equal(edges.cpu(), c.edges)
    assert torch.equal(edges[:, 0], torch.repeat_interleave(src, ptr[1:] - ptr[:-1]))
    count = ops.row_diff_count(c.adj2._rowptr, c.adj2._col, c.adj._rowptr, c.adj._col, src)
    assert count.dtype == torch.int32 and torch.equal(count.cpu().long(), sizes)
    assert torch.equal(ops.scan_i32(count), ptr)
    ptr2, edges2 = R.two_hop_candidates(c.adj, c.adj2, src, known=c.adj)                      # the default, spelled out
    assert torch.equal(ptr2, ptr) and torch.equal(edges2, edges)
    with pytest.raises(IndexError):                                                           # ids are bounds-checked, as every op checks them
        R.two_hop_candidates(c.adj, c.adj2, torch.tensor([0, c.n], device=DEV))
    with pytest.raises(IndexError):
        R.two_hop_candidates(c.adj, c.adj2, torch.tensor([-1], device=DEV))


def test_drop_self_zero_keeps_the_diagonal(prop):
    from ocn_amd import ops
    c = prop
    src = torch.tensor(c.sources, dtype=torch.int64, device=DEV)
    args = (c.adj2._rowptr, c.adj2._col, c.adj._rowptr, c.adj._col, src)
    off = ops.scan_i32(ops.row_diff_count(*args, drop_self=False))
    edges = ops.row_diff_fill(*args, off, drop_self=False)
    rptr, redges = ref_diff(c.a2_rows, c.a_rows, c.sources, drop_self=False)
    assert torch.equal(off.cpu(), rptr) and torch.equal(edges.cpu(), redges)
    connected = torch.tensor([len(c.a_rows[s]) > 0 for s in c.sources])
    assert torch.equal((rptr[1:] - rptr[:-1]) - (c.ptr[1:] - c.ptr[:-1]), connected.long())    # exactly the diagonal entry more
    assert int((edges[:, 0] == edges[:, 1]).sum()) == int(connected.sum())


def test_known_superset_removes_exactly_the_extra_links(prop):
    from ocn_amd.sparse import SparseTensor
    c = prop
    p = c.ptr.tolist()
    extra = []
    for q in range(len(c.sources)):
        if p[q + 1] - p[q] >= 2 and len(extra) < 80:
            extra += [c.edges[p[q]].tolist(), c.edges[p[q + 1] - 1].tolist()]                  # first and last candidate of the source
    assert len(extra) == 80
    ex = torch.tensor(extra, dtype=torch.int64).t()
    ei = torch.cat([torch.stack([c.oadj.row, c.oadj.col]), ex], dim=1)
    known = SparseTensor.from_edge_index(ei.to(DEV), sparse_sizes=(c.n, c.n)).coalesce()
    k_rows = [set(r) for r in c.a_rows]
    for s, t in extra:
        k_rows[s].add(t)
    rptr, redges = ref_diff(c.a2_rows, k_rows, c.sources)
    gone = {(s, t) for s, t in extra}
    assert {tuple(e) for e in c.edges.tolist()} - {tuple(e) for e in redges.tolist()} == gone
    from ocn_amd import recommend as R
    ptr, edges = R.two_hop_candidates(c.adj, c.adj2, torch.tensor(c.sources, dtype=torch.int64, device=DEV), known=known)
    assert torch.equal(ptr.cpu(), rptr) and torch.equal(edges.cpu(), redges)


# ---- segmented top-k ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 64, 100, "k_max"])
def test_segment_lengths_around_k_and_the_chunk_size(hiplib, k):
    from ocn_amd import ops
    k = ops.segment_topk_max_k() if k == "k_max" else k
    lens = [0, 1, k - 1, k, k + 1, 63, 64, 65, 129, 5000]
    lens = lens + lens[::-1]                                             # twenty segments: five workgroups
    g = torch.Generator().manual_seed(100 + k)
    ptr = torch.tensor([0] + lens, dtype=torch.int64).cumsum(0)
    scores = torch.randn(int(ptr[-1]), generator=g)
    scores[: scores.numel() // 2] = (scores[: scores.numel() // 2] * 4).round() / 4            # ties: the first half is quantised
    val, pos = check_topk(scores, ptr, k)
    for q, n in enumerate(lens):
        assert int((pos[q] >= 0).sum()) == min(n, k)
        assert bool((pos[q, min(n, k):] == -1).all()) and bool((val[q, min(n, k):] == float("-inf")).all())
        assert bool(((pos[q, :min(n, k)] >= ptr[q]) & (pos[q, :min(n, k)] < ptr[q + 1])).all())
    assert scores[: scores.numel() // 2].unique().numel() < 100          # (the quantised half, a 5 000-long segment in it, is mostly ties)


def test_order_contract(hiplib):
    inf, nan = float("inf"), float("nan")
    mixed = torch.tensor([nan, -inf, 0.0, -0.0, inf, 1.0, -0.0, nan, 0.0, inf, -1.0, -inf])
    want = [4, 9, 5, 2, 3, 6, 8, 10, 1, 11, 0, 7]                        # inf, inf, 1, the four zeros by position, -1, -inf, -inf, NaN, NaN
    equal = torch.full((300,), 0.25)
    up, down = torch.arange(5000, dtype=torch.float32), torch.arange(5000, 0, -1, dtype=torch.float32)
    nans = torch.full((70,), nan)
    segs = [mixed, equal, up, down, nans, mixed.flip(0)]
    ptr = torch.tensor([0] + [s.numel() for s in segs], dtype=torch.int64).cumsum(0)
    scores = torch.cat(segs)
    for k in (5, 12, 64, 100):
        val, pos = check_topk(scores, ptr, k)
        assert pos[0, :min(k, 12)].tolist() == want[:k]
        if k >= 12:
            got = val[0, :12]
            assert got[:3].tolist() == [inf, inf, 1.0] and got[7:10].tolist() == [-1.0, -inf, -inf] and bool(got[10:].isnan().all())
            assert torch.signbit(got[3:7]).tolist() == [False, True, True, False]              # the zeros come back as they were stored
            assert bool((pos[0, 12:] == -1).all())
        assert pos[1].tolist() == list(range(int(ptr[1]), int(ptr[1]) + k))                             # all equal: the first k positions
        assert pos[2].tolist() == list(range(int(ptr[3]) - 1, int(ptr[3]) - 1 - k, -1))       # ascending: the best are in the last chunk
        assert pos[3].tolist() == list(range(int(ptr[3]), int(ptr[3]) + k))                   # descending: every later chunk is skipped
        assert pos[4, :min(k, 70)].tolist() == list(range(int(ptr[4]), int(ptr[4]) + min(k, 70)))      # NaNs among themselves: by position
        assert pos[5, :min(k, 12)].tolist() == [int(ptr[5]) + 11 - w for w in
                                               [9, 4, 5, 8, 6, 3, 2, 10, 11, 1, 7, 0]][:k]    # the same values reversed: ties the other way


def test_empty_inputs(hiplib):
    from ocn_amd import recommend as R
    val, pos = R.segment_topk(torch.zeros(0, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV), 7)      # Q = 0
    assert val.shape == (0, 7) and pos.shape == (0, 7) and val.dtype == torch.float32 and pos.dtype == torch.int64
    val, pos = R.segment_topk(torch.zeros(0, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV), 100)    # T = 0
    assert val.shape == (3, 100) and bool((val == float("-inf")).all()) and bool((pos == -1).all())
    val, pos = R.segment_topk(torch.ones(5, device=DEV), torch.tensor([0, 0, 5, 5], device=DEV), 3)              # empty segments around one
    assert pos.tolist() == [[-1] * 3, [0, 1, 2], [-1] * 3] and val[1].tolist() == [1.0] * 3
    n = 10                                                               # a path and four isolated nodes
    adj, adj2 = device_graph(torch.stack([torch.arange(5), torch.arange(1, 6)]), n)
    ptr, edges = R.two_hop_candidates(adj, adj2, torch.zeros(0, dtype=torch.int64, device=DEV))
    assert ptr.tolist() == [0] and edges.shape == (0, 2) and edges.dtype == torch.int64
    iso = torch.tensor([7, 9, 7], device=DEV)
    ptr, edges = R.two_hop_candidates(adj, adj2, iso)
    assert ptr.tolist() == [0, 0, 0, 0] and edges.shape == (0, 2)
    dst, score = R.recommend_links_heuristic(adj, adj2, iso, 4, 16, "aa")
    assert dst.shape == (3, 4) and bool((dst == -1).all()) and bool((score == float("-inf")).all())
    dst, score = R.recommend_links_heuristic(adj, adj2, torch.zeros(0, dtype=torch.int64, device=DEV), 4, 16, "aa")
    assert dst.shape == (0, 4) and score.shape == (0, 4)


# ---- end to end --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ip", [("cn5", 0.0), ("cn5", 0.37), ("cn7", None)], ids=["cn5_ip0", "cn5_ip037", "cn7"])
def test_recommend_links_equals_score_edges_and_the_restatement(prop, name, ip):
    """The contract: the scores are exactly those ``score_edges`` returns for the flat candidate list at that batch size (the
    normalisation of cn5 / cn7 couples the candidates of a batch), selected per source by the stated order."""
    from ocn_amd import recommend as R
    from ocn_amd.model import predictor_dict
    from ocn_amd.pipeline import score_edges
    c = prop
    H, Q, k, bs = 64, 64, 10, 4096
    torch.manual_seed(12)
    h = torch.randn(c.n, H, device=DEV)
    pred = predictor_dict[name](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()
    if ip is not None:
        pred.innerprod.fill_(ip)
    args = SimpleNamespace(sum=0.5)
    src = torch.tensor(c.sources[:Q], dtype=torch.int64, device=DEV)     # the hub, the isolated nodes, repeats among them
    ptr, edges = R.two_hop_candidates(c.adj, c.adj2, src)
    T = edges.shape[0]
    assert T > 2 * bs and T % bs != 0                                    # several batches and a ragged last one
    flat = score_edges(pred, h, c.adj, c.adj2, edges, bs, args)
    dst, score = R.recommend_links(pred, h, c.adj, c.adj2, src, k, bs, args)
    assert dst.shape == (Q, k) and dst.dtype == torch.int64 and score.shape == (Q, k) and score.dtype == torch.float32
    rdst, rscore = ref_select(flat.cpu(), ptr.cpu(), edges.cpu(), k)
    assert torch.equal(dst.cpu(), rdst) and same_bits(score, rscore)
    sizes = (ptr[1:] - ptr[:-1]).cpu()
    assert bool((sizes == 0).any()) and bool(((dst.cpu() == -1).sum(1) == (k - sizes.clamp(max=k))).all())
    for q, s in enumerate(c.sources[:Q]):                                # a recommendation is a 2-hop neighbour that is no link yet
        picked = [t for t in dst[q].tolist() if t >= 0]
        assert len(set(picked)) == len(picked) and all(t in c.a2_rows[s] and t not in c.a_rows[s] and t != s for t in picked)
    dst2, score2 = R.recommend_links(pred, h, c.adj, c.adj2, src, k, bs, args)
    assert torch.equal(dst2, dst) and same_bits(score2, score)
    with pytest.raises(RuntimeError, match="eval path"):
        R.recommend_links(pred.train(), h, c.adj, c.adj2, src, k, bs, args)


def test_recommend_links_heuristic(prop):
    from ocn_amd import heuristics as Hx, recommend as R
    m, r = 5, 7                                                          # K_{5,7}: two left nodes share all seven right nodes
    left, right = torch.arange(m), torch.arange(m, m + r)
    adj, adj2 = device_graph(torch.stack([left.repeat_interleave(r), right.repeat(m)]), m + r)
    src = torch.tensor([2, 0, 4], device=DEV)
    dst, score = R.recommend_links_heuristic(adj, adj2, src, 3, 8, "cn")
    assert dst.tolist() == [[0, 1, 3], [1, 2, 3], [0, 1, 2]] and bool((score == 7.0).all())   # ties: the smallest other left ids
    dst, score = R.recommend_links_heuristic(adj, adj2, src, 6, 8, "cn")
    assert dst.tolist() == [[0, 1, 3, 4, -1, -1], [1, 2, 3, 4, -1, -1], [0, 1, 2, 3, -1, -1]]
    assert score[:, :4].tolist() == [[7.0] * 4] * 3 and bool((score[:, 4:] == float("-inf")).all())
    c = prop
    k = 100
    sources = torch.tensor(c.sources, dtype=torch.int64, device=DEV)
    flat = Hx.link_heuristics(c.adj, c.adj2, c.edges.t().contiguous().to(DEV), ("ra",))[:, 0]
    rdst, rscore = ref_select(flat.cpu(), c.ptr, c.edges, k)
    for bs in (5000, 1 << 20):                                           # nothing depends on the batch
        dst, score = R.recommend_links_heuristic(c.adj, c.adj2, sources, k, bs, "ra")
        assert torch.equal(dst.cpu(), rdst) and same_bits(score, rscore)
    assert int((rdst >= 0).sum()) > 100 * 100 and bool((rscore[rdst >= 0] > 0).all())         # 2-hop neighbours share a neighbour


def test_example_driver_recommends(hiplib):
    """examples/run_like_reference.py --heuristic ra --recommend 5 on the Cora shape, in a fresh process: the metric line as
    before, then K ids per listed source."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_like_reference.py"), "--dataset", "cora",
                          "--heuristic", "ra", "--recommend", "5"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    assert re.search(r"heuristic ra hits@100 valid/test \d\.\d{4}/\d\.\d{4}", run.stdout)
    rows = re.findall(r"^recommend source (\d+) top-5: ((?:-?\d+ ){4}-?\d+)  scores: (.*)$", run.stdout, re.M)
    assert len(rows) == 5
    for s, ids, scores in rows:
        ids = [int(t) for t in ids.split()]
        assert len(ids) == 5 and len(scores.split()) == 5 and int(s) not in ids
        real = [t for t in ids if t >= 0]
        assert len(set(real)) == len(real) and all(0 <= t < 2708 for t in real)
    assert any(int(t) >= 0 for _, ids, _ in rows for t in ids.split())
