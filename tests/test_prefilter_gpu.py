"""Two-stage link recommendation on the GPU: the scored 2-hop expansion (``ocn_two_hop_sums_fill``), the short list
(``recommend.prefilter_candidates``) and ``recommend_links(prefilter=...)``.  The references are restatements written here —
Python sets over a dictionary of rows and numpy ``float32`` adds in ascending ``m`` — and the project's existing routes
(``two_hop_candidates``, ``link_heuristics``).  Sets, orders and sums are exact: every comparison is ``torch.equal``."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import close, product_adj2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KINDS = ("cn", "aa", "ra")
F0 = np.float32(0.0)


# ---- the restatements --------------------------------------------------------------------------------------------------
def sym_rows(n, pairs):
    rows = {v: set() for v in range(n)}
    for a, b in pairs:
        if a != b:
            rows[a].add(b)
            rows[b].add(a)
    return rows


def csr_of(rows, n):
    """Row sets (a dictionary; a missing row is empty) -> the project's SparseTensor on the device."""
    from ocn_amd.sparse import SparseTensor
    lens = torch.zeros(n, dtype=torch.int64)
    items = sorted((r, sorted(cs)) for r, cs in rows.items() if cs)
    if items:
        lens[torch.tensor([r for r, _ in items])] = torch.tensor([len(cs) for _, cs in items])
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = lens.cumsum(0)
    col = torch.tensor([c for _, cs in items for c in cs], dtype=torch.int32)
    return SparseTensor(rowptr=rowptr.to(DEV), col=col.to(DEV), sparse_sizes=(n, n))


def ref_scored_one(a_rows, m_rows, s, weight, descending=False):
    """Source ``s``: {c: fp32 sum of weight[m] over the m in A[s] whose row holds c, one add per member from 0.0f, in
    ascending m} without the columns of M[s] and s itself."""
    acc = {}
    for m in sorted(a_rows.get(s, ()), reverse=descending):
        wm = np.float32(weight[m])
        for c in a_rows.get(m, ()):
            acc[c] = np.float32(acc.get(c, F0) + wm)
    for c in m_rows.get(s, ()):
        acc.pop(c, None)
    acc.pop(s, None)
    return acc


def ref_scored(a_rows, m_rows, sources, weight, descending=False):
    """(ptr [Q + 1], edges [T, 2], val [T]) of the sources, a source's candidates ascending; each distinct source is expanded once."""
    per, ptr, pairs, vals = {}, [0], [], []
    for s in sources:
        if s not in per:
            per[s] = sorted(ref_scored_one(a_rows, m_rows, s, weight, descending).items())
        pairs += [(s, c) for c, _ in per[s]]
        vals += [v for _, v in per[s]]
        ptr.append(len(pairs))
    return (torch.tensor(ptr, dtype=torch.int64), torch.tensor(pairs, dtype=torch.int64).reshape(-1, 2),
            torch.from_numpy(np.array(vals, dtype=np.float32)))


def ref_prefilter(ptr, edges, val, m):
    """Per source: sort by (-val, id), take m, return ascending by id."""
    p, ids, v = ptr.tolist(), edges[:, 1].tolist(), val.tolist()
    out_ptr, keep = [0], []
    for q in range(len(p) - 1):
        seg = sorted(range(p[q], p[q + 1]), key=lambda i: (-v[i], ids[i]))[:m]
        keep += sorted(seg, key=lambda i: ids[i])
        out_ptr.append(len(keep))
    return torch.tensor(out_ptr, dtype=torch.int64), edges[torch.tensor(keep, dtype=torch.int64)].reshape(-1, 2)


def ref_select(scores, ptr, edges, k):
    """Per segment the k best: the higher score first, equal scores by position; padded with -1 / -inf."""
    s, p = scores.cpu().numpy(), ptr.tolist()
    Q = len(p) - 1
    dst = torch.full((Q, k), -1, dtype=torch.int64)
    val = torch.full((Q, k), float("-inf"), dtype=torch.float32)
    for q in range(Q):
        seg = s[p[q]:p[q + 1]]
        assert not np.isnan(seg).any()
        order = np.lexsort((np.arange(seg.size), -seg))[:k]
        dst[q, :order.size] = edges[p[q]:p[q + 1], 1].cpu()[torch.from_numpy(order)]
        val[q, :order.size] = torch.from_numpy(seg[order].copy())
    return dst, val


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def src_tensor(sources):
    return torch.tensor(sources, dtype=torch.int64, device=DEV)


def scored(adj, known, sources, w=None, wcol=0, window_cols=0):
    """(ptr, edges, val) on the host through the ops layer, where the table, its column and the window can be chosen."""
    from ocn_amd import ops
    src = src_tensor(sources)
    args = (adj._rowptr, adj._col, known._rowptr, known._col, src)
    off = ops.scan_i32(ops.two_hop_diff_count(*args))
    edges, val = ops.two_hop_sums_fill(*args, off, w, wcol, window_cols=window_cols)
    assert edges.dtype == torch.int64 and edges.dim() == 2 and edges.shape[1] == 2
    assert val.dtype == torch.float32 and val.shape == (edges.shape[0],)
    return off.cpu(), edges.cpu(), val.cpu()


def kind_weight(adj, kind):
    """The weight of every node under ``kind``, from the table the library reads (formed on the CPU by ``node_table``)."""
    from ocn_amd.heuristics import node_table
    n = adj.size(0)
    return np.ones(n, dtype=np.float32) if kind == "cn" else node_table(adj)[:, 0 if kind == "aa" else 1].cpu().numpy()


# ---- the 200-node graph ---------------------------------------------------------------------------------------------------
N, HUB, ISOLATED, TRIANGLE = 200, 3, (187, 188, 189), (190, 191, 192)


@pytest.fixture(scope="module")
def graph(hiplib):
    """Symmetric, random, 187 nodes at a density of a few percent; node 3 is a hub of 80 links; 187 - 189 are isolated (sources
    with an empty row); 190 - 192 form a triangle of their own (every 2-hop target of such a source is known); 193 - 199 a path.
    The sources are all nodes in a shuffled order with thirty of them repeated.  Python references once per kind.  (A neighbour
    with an EMPTY row cannot occur in a symmetric graph: the directed graph of ``ordered`` below has one.)"""
    rng = np.random.default_rng(17)
    a = np.triu(rng.random((187, 187)) < 0.05, 1)
    pairs = list(zip(*np.nonzero(a))) + [(HUB, v) for v in range(100, 180)]
    pairs += [(190, 191), (191, 192), (190, 192)] + [(v, v + 1) for v in range(193, 199)]
    a_rows = sym_rows(N, [(int(x), int(y)) for x, y in pairs])
    assert len(a_rows[HUB]) > 64 and all(not a_rows[v] for v in ISOLATED)
    adj = csr_of(a_rows, N)
    order = torch.randperm(N, generator=torch.Generator().manual_seed(2)).tolist()
    sources = order[:120] + order[30:60] + order[120:]
    assert len(sources) == N + 30 and set(sources) == set(range(N))
    ref = {kind: ref_scored(a_rows, a_rows, sources, kind_weight(adj, kind)) for kind in KINDS}
    sizes = ref["cn"][0][1:] - ref["cn"][0][:-1]
    for v in ISOLATED + TRIANGLE:
        assert int(sizes[sources.index(v)]) == 0
    assert int(sizes.max()) > 128 and int((sizes > 0).sum()) > 180
    return SimpleNamespace(n=N, a_rows=a_rows, adj=adj, sources=sources, ref=ref)


# ---- 1. the kernel against the reference and the existing routes -------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_scored_expansion_equals_the_candidates_the_heuristics_and_the_reference(graph, kind):
    from ocn_amd import recommend as R
    from ocn_amd.heuristics import link_heuristics, node_table
    g = graph
    src = src_tensor(g.sources)
    cptr, cedges = R.two_hop_candidates(g.adj, None, src)
    heur = link_heuristics(g.adj, None, cedges.t().contiguous(), (kind,))[:, 0]
    rptr, redges, rval = g.ref[kind]
    assert torch.equal(cptr.cpu(), rptr) and torch.equal(cedges.cpu(), redges)
    if kind != "cn":
        assert len(set(rval.tolist())) > 100                             # sums of many different weights, not a count
    w, wcol = (None, 0) if kind == "cn" else (node_table(g.adj), 0 if kind == "aa" else 1)
    for window in (64, 128, 0):
        ptr, edges, val = scored(g.adj, g.adj, g.sources, w, wcol, window)
        assert torch.equal(ptr, cptr.cpu()) and torch.equal(edges, cedges.cpu()), window
        assert torch.equal(bits(val), bits(heur)), window
        assert torch.equal(bits(val), bits(rval)), window
    ptr, edges, val = R.two_hop_scored_candidates(g.adj, src, kind)
    assert torch.equal(ptr, cptr) and torch.equal(edges, cedges) and torch.equal(bits(val), bits(rval))
    ptr0, edges0, val0 = R.two_hop_scored_candidates(g.adj, src[:0], kind)
    assert ptr0.tolist() == [0] and edges0.shape == (0, 2) and val0.shape == (0,) and val0.dtype == torch.float32
    with pytest.raises(IndexError):
        R.two_hop_scored_candidates(g.adj, torch.tensor([0, g.n], device=DEV), kind)


# ---- 2. order decides the bits ---------------------------------------------------------------------------------------------
MIDS = {5: 1e8, 10: 1.0, 20: -1e8, 33: 3e-1, 70: 1.0, 71: 3e-1, 90: 0.0, 130: -2.5, 131: 0.7, 150: 1.1, 160: 2.0, 199: 7.0}
TARGETS = [15, 16, 17, 31, 32, 47, 48, 63, 64, 65, 79, 80, 127, 128, 129, 191, 192, 198]   # both sides of every quarter (16) and window (64) edge
SOURCES2 = [0, 1, 2, 64, 16, 3, 0]


@pytest.fixture(scope="module")
def ordered(hiplib):
    """A directed hand-built A of 200 columns.  Source i links to the middle nodes MIDS without the i-th; a middle node's row
    holds the TARGETS without one of them, so every target collects a different ascending run of the weights 1e8, 1, -1e8, 0.3 ...
    (``wcol`` 2 of a hand-built table) from neighbours that lie at consecutive positions of the source row.  Node 70 has a row
    of more than 64 entries (entered by binary search), node 199 an empty row.  Column 101 is reached through the zero-weight
    node alone, column 103 through 1e8 and -1e8, column 105 through -2.5: sums that are 0.0, 0.0 and negative."""
    n = 200
    mids = sorted(MIDS)
    rows = {}
    for i, s in enumerate([0, 1, 2, 64, 16, 3]):
        rows[s] = set(mids) - {mids[i]}
    for j, m in enumerate(mids):
        rows[m] = set(TARGETS) - {TARGETS[(2, 0, 9, 1, 3, 4, 5, 6, 7, 8, 10, 11)[j]]}      # (5 and 20, the ±1e8 pair, keep every edge column)
    rows[70] |= set(range(20, 200, 2)) - {70}
    rows[199] = set()
    rows[90] |= {101}
    rows[5] |= {103}
    rows[20] |= {103}
    rows[130] |= {105}
    assert len(rows[70]) > 64
    weight = np.zeros(n, dtype=np.float32)
    for m, x in MIDS.items():
        weight[m] = x
    table = torch.zeros(n, 4)
    table[:, 2] = torch.from_numpy(weight)
    table[:, 0], table[:, 1], table[:, 3] = 1.0, -3.0, 11.0               # the other columns must not be read
    return SimpleNamespace(n=n, rows=rows, adj=csr_of(rows, n), weight=weight, table=table.to(DEV))


def test_ascending_m_summation_decides_the_bits(ordered):
    c = ordered
    rptr, redges, rval = ref_scored(c.rows, c.rows, SOURCES2, c.weight)
    _, _, other = ref_scored(c.rows, c.rows, SOURCES2, c.weight, descending=True)
    differ = bits(rval) != bits(other)
    print(f"ordered: {rval.numel()} candidates, {int(differ.sum())} whose descending-m sum has other bits")
    on_targets = torch.tensor([int(t) in TARGETS for t in redges[:, 1]])
    assert int((differ & on_targets).sum()) > int(on_targets.sum()) // 4                      # another order is another result
    for lo, hi in ((15, 16), (31, 32), (47, 48), (63, 64), (127, 128), (191, 192)):           # an edge with sensitive columns on both sides
        assert bool(differ[(redges[:, 1] == lo)].any()) and bool(differ[(redges[:, 1] == hi)].any()), (lo, hi)
    first = {int(t): float(v) for t, v in zip(redges[rptr[1]:rptr[2], 1], rval[rptr[1]:rptr[2]])}       # source 1: it links to 5 and 20
    assert first[101] == 0.0 and first[103] == 0.0 and first[105] == -2.5 and bool((rval < 0).any())
    for window in (64, 128, 0):
        ptr, edges, val = scored(c.adj, c.adj, SOURCES2, c.table, 2, window)
        assert torch.equal(ptr, rptr) and torch.equal(edges, redges), window
        assert torch.equal(bits(val), bits(rval)), window
    # the same graph without a table: a count, whatever the column says
    _, cedges, cn = scored(c.adj, c.adj, SOURCES2, None, 3, 64)
    _, _, rcn = ref_scored(c.rows, c.rows, SOURCES2, np.ones(c.n, dtype=np.float32))
    assert torch.equal(cedges, redges) and torch.equal(bits(cn), bits(rcn))


# ---- 3. wider than one default window -----------------------------------------------------------------------------------------
def test_graph_wider_than_the_default_sums_window(hiplib):
    """n = W + 65 for W = ``ocn_two_hop_sums_window_cols()``: source 5 reaches W - 1, W, W + 1 and n - 1 through two
    neighbours, one on each side of the window's edge — so each of those sums adds members found in different windows' passes
    over the source row — and source n - 2 lies beyond the first window itself."""
    from ocn_amd import ops, recommend as R
    from ocn_amd.heuristics import link_heuristics
    W = ops.two_hop_sums_window_cols()
    assert 64 <= W < ops.two_hop_window_cols() and W % 64 == 0
    n = W + 65
    far = [W - 1, W, W + 1, n - 1]
    pairs = [(5, 7), (5, W + 3), (5, 9000)]
    pairs += [(7, c) for c in far + [9, 100, 4097, W - 64, W - 33]]
    pairs += [(W + 3, c) for c in far + [2, W + 31, W + 32, W + 64]]
    pairs += [(9000, c) for c in far[1:] + [9, 2, W // 2, W // 4 - 1, W // 4, 3 * (W // 4) - 1, 3 * (W // 4)]]
    pairs += [(n - 2, n - 3), (n - 2, 11), (n - 3, W), (n - 3, 0), (n - 3, n - 1), (11, 12), (11, W - 1), (11, W + 40)]
    pairs += [(1000 + 3 * i, 2000 + 5 * i) for i in range(100)] + [(2000 + 5 * i, W + i % 60) for i in range(100)]
    a_rows = sym_rows(n, pairs)
    adj = csr_of(a_rows, n)
    sources = [5, n - 2, W, 7, W + 3, 0, n - 1, 1000, 2000, W - 1, 5, 9000]
    src = src_tensor(sources)
    cptr, cedges = R.two_hop_candidates(adj, None, src)
    for kind in KINDS:
        rptr, redges, rval = ref_scored(a_rows, a_rows, sources, kind_weight(adj, kind))
        mine = dict(zip(redges[rptr[0]:rptr[1], 1].tolist(), rval[rptr[0]:rptr[1]].tolist()))
        assert set(far) <= set(mine)
        if kind == "cn":
            assert mine[W - 1] == 2.0 and mine[W] == mine[W + 1] == mine[n - 1] == 3.0
        ptr, edges, val = R.two_hop_scored_candidates(adj, src, kind)
        assert torch.equal(ptr, cptr) and torch.equal(edges, cedges)
        assert torch.equal(ptr.cpu(), rptr) and torch.equal(edges.cpu(), redges) and torch.equal(bits(val), bits(rval)), kind
        assert torch.equal(bits(val), bits(link_heuristics(adj, None, edges.t().contiguous(), (kind,))[:, 0])), kind


# ---- 4. more queries than workgroups ----------------------------------------------------------------------------------------
def test_grid_stride_over_five_thousand_sources(graph):
    """The launch has at most 4 096 workgroups (ocn_hip.h); with 5 000 queries some workgroups take a second one."""
    g = graph
    sources = torch.randint(0, g.n, (5000,), generator=torch.Generator().manual_seed(8)).tolist()
    assert len(set(sources)) == g.n
    from ocn_amd.heuristics import node_table
    rptr, redges, rval = ref_scored(g.a_rows, g.a_rows, sources, kind_weight(g.adj, "ra"))
    for window in (0, 64):
        ptr, edges, val = scored(g.adj, g.adj, sources, node_table(g.adj), 1, window)
        assert torch.equal(ptr, rptr) and torch.equal(edges, redges) and torch.equal(bits(val), bits(rval)), window


# ---- 5. known differs from adj ------------------------------------------------------------------------------------------------
def test_known_superset_drops_targets_and_leaves_the_other_sums_alone(graph):
    from ocn_amd import recommend as R
    from ocn_amd.heuristics import node_table
    g = graph
    rptr, redges, rval = g.ref["aa"]
    known = {v: set(r) for v, r in g.a_rows.items()}
    rng = np.random.default_rng(4)
    dropped = set()
    for i in rng.choice(redges.shape[0], 400, replace=False).tolist():   # (one-sided: known is no adjacency)
        s, t = redges[i].tolist()
        known[s].add(t)
        dropped.add((s, t))
    s_full = g.sources[int((rptr[1:] - rptr[:-1]).argmax())]             # ... and one source loses its whole list
    known[s_full] |= set(range(g.n))
    kn = csr_of(known, g.n)
    kptr, kedges, kval = ref_scored(g.a_rows, known, g.sources, kind_weight(g.adj, "aa"))
    assert 0 < kedges.shape[0] < redges.shape[0] - 400
    full = {(int(s), int(t)): v for (s, t), v in zip(redges.tolist(), bits(rval).tolist())}
    ptr, edges, val = R.two_hop_scored_candidates(g.adj, src_tensor(g.sources), "aa", known=kn)
    assert torch.equal(ptr.cpu(), kptr) and torch.equal(edges.cpu(), kedges) and torch.equal(bits(val), bits(kval))
    got = {(int(s), int(t)) for s, t in edges.cpu().tolist()}
    assert not (got & dropped) and not any(s == s_full for s, _ in got)
    assert all(full[(int(s), int(t))] == v for (s, t), v in zip(edges.cpu().tolist(), bits(val).tolist()))
    cptr, cedges = R.two_hop_candidates(g.adj, None, src_tensor(g.sources), known=kn)
    assert torch.equal(ptr, cptr) and torch.equal(edges, cedges)
    for window in (64, 128):
        p, e, v = scored(g.adj, kn, g.sources, node_table(g.adj), 0, window)
        assert torch.equal(p, kptr) and torch.equal(e, kedges) and torch.equal(bits(v), bits(kval)), window


# ---- 6. the short list ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 5, 128])
def test_prefilter_candidates_keeps_the_m_best_in_ascending_id(graph, m):
    from ocn_amd import recommend as R
    g = graph
    rptr, redges, rval = g.ref["cn"]
    sizes = rptr[1:] - rptr[:-1]
    assert int(sizes.max()) > 128 and bool(((sizes > 0) & (sizes < m)).any()) == (m > 1)
    ties = sum(len(set(rval[rptr[q]:rptr[q + 1]].tolist())) < int(sizes[q]) for q in range(len(g.sources)))
    assert ties > 100                                                    # counts: most lists hold equal scores
    want_ptr, want_edges = ref_prefilter(rptr, redges, rval, m)
    ptr_m, edges_m = R.prefilter_candidates(g.adj, src_tensor(g.sources), "cn", m)
    assert ptr_m.dtype == torch.int64 and edges_m.dtype == torch.int64
    assert torch.equal(ptr_m.cpu(), want_ptr) and torch.equal(edges_m.cpu(), want_edges)
    assert torch.equal(ptr_m.cpu()[1:] - ptr_m.cpu()[:-1], sizes.clamp(max=m))           # a shorter list is kept whole
    for kind in ("aa", "ra"):
        _, _, v = g.ref[kind]
        want_ptr, want_edges = ref_prefilter(rptr, redges, v, m)
        ptr_m, edges_m = R.prefilter_candidates(g.adj, src_tensor(g.sources), kind, m)
        assert torch.equal(ptr_m.cpu(), want_ptr) and torch.equal(edges_m.cpu(), want_edges), kind
    p0, e0 = R.prefilter_candidates(g.adj, src_tensor(list(ISOLATED)), "cn", m)
    assert p0.tolist() == [0, 0, 0, 0] and e0.shape == (0, 2)


# ---- 7. recommend_links with a prefilter -----------------------------------------------------------------------------------------
def make_predictor(name, H, seed=12):
    from ocn_amd.model import predictor_dict
    torch.manual_seed(seed)
    return predictor_dict[name](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()


@pytest.mark.parametrize("name", ["cn5", "cn7", "cn6"])
def test_recommend_links_with_a_prefilter_is_the_composition(graph, name):
    """prefilter_candidates -> the scoring loop over the retained list -> the top k: ``dst`` and ``score`` bit for bit."""
    from ocn_amd import recommend as R
    from ocn_amd.pipeline import score_edges, score_edges_walk
    g = graph
    H, k, m, bs = 64, 7, 20, 1000
    pred = make_predictor(name, H)
    h = torch.randn(g.n, H, generator=torch.Generator().manual_seed(3)).to(DEV)
    args = SimpleNamespace(sum=0.5)
    src = src_tensor(g.sources)
    adj2 = product_adj2(g.adj)
    ptr_m, edges_m = R.prefilter_candidates(g.adj, src, "ra", m)
    assert edges_m.shape[0] > 2 * bs and edges_m.shape[0] % bs != 0      # several batches and a ragged last one
    for a2 in (adj2, None):
        if a2 is None and name == "cn6":
            with pytest.raises(ValueError, match="cn6 needs adj2"):
                R.recommend_links(pred, h, g.adj, None, src, k, bs, args, prefilter=("ra", m))
            continue
        flat = score_edges(pred, h, g.adj, a2, edges_m, bs, args) if a2 is not None else score_edges_walk(pred, h, g.adj, edges_m, bs, args)
        assert flat.shape == (edges_m.shape[0],) and bool(torch.isfinite(flat).all())
        want_dst, want_score = ref_select(flat, ptr_m, edges_m, k)
        dst, score = R.recommend_links(pred, h, g.adj, a2, src, k, bs, args, prefilter=("ra", m))
        assert dst.shape == (len(g.sources), k) and dst.dtype == torch.int64 and score.dtype == torch.float32
        assert torch.equal(dst.cpu(), want_dst) and torch.equal(bits(score), bits(want_score)), a2 is None
        full_dst, _ = R.recommend_links(pred, h, g.adj, a2, src, k, bs, args)
        assert not torch.equal(dst, full_dst)                            # (the short list does change the request)
    keep = {(int(s), int(t)) for s, t in edges_m.cpu().tolist()}
    assert all((s, int(t)) in keep for s, row in zip(g.sources, dst.cpu().tolist()) for t in row if t >= 0)


def test_a_prefilter_that_covers_every_list_changes_nothing(hiplib):
    """No source has more than 128 candidates, ``m`` is at least the longest list: the retained list is the full list, and even a
    batch-coupled cn5 returns the unfiltered result bit for bit — through A² and on the walk route."""
    from ocn_amd import recommend as R
    n = 120
    rng = np.random.default_rng(23)
    a_rows = sym_rows(n, [(int(x), int(y)) for x, y in zip(*np.nonzero(np.triu(rng.random((n, n)) < 0.05, 1)))])
    adj = csr_of(a_rows, n)
    sources = torch.randperm(n, generator=torch.Generator().manual_seed(6)).tolist() + [4, 4, 9]
    src = src_tensor(sources)
    ptr, edges = R.two_hop_candidates(adj, None, src)
    longest = int((ptr[1:] - ptr[:-1]).max())
    assert 20 < longest <= 128 and edges.shape[0] > 2000
    H, k, bs = 64, 10, 700
    pred = make_predictor("cn5", H)
    h = torch.randn(n, H, generator=torch.Generator().manual_seed(5)).to(DEV)
    for a2 in (product_adj2(adj), None):
        want_dst, want_score = R.recommend_links(pred, h, adj, a2, src, k, bs)
        assert bool(torch.isfinite(want_score).any())
        for m in (128, longest):
            for kind in ("cn", "ra"):
                dst, score = R.recommend_links(pred, h, adj, a2, src, k, bs, prefilter=(kind, m))
                assert torch.equal(dst, want_dst) and torch.equal(bits(score), bits(want_score)), (a2 is None, m, kind)
    other = R.recommend_links(pred, h, adj, None, src, k, bs, prefilter=("ra", longest // 2))[1]
    assert not torch.equal(bits(other), bits(want_score))                # the control: a shorter list moves the coupled scores


def test_frozen_prefiltered_scores_are_the_unfiltered_scores_of_the_retained_pairs(graph):
    """cn5 with frozen column weights, m = 5 well below the lists: every returned (source, dst, score) is found among the scores
    of ``score_edges`` over the FULL candidate list, within the frozen-scoring tolerance of tests/test_frozen_gpu.py
    (``helpers.close``: 1e-5 absolute and relative)."""
    from ocn_amd import recommend as R
    from ocn_amd.frozen import freeze_columns
    from ocn_amd.pipeline import score_edges
    g = graph
    H, k, m, bs = 64, 3, 5, 900
    pred = make_predictor("cn5", H, seed=31)
    with torch.no_grad():
        pred.alpha.copy_(torch.tensor([0.4, -0.3, 0.1]))
        pred.innerprod.fill_(0.37)
    h = torch.randn(g.n, H, generator=torch.Generator().manual_seed(10)).to(DEV)
    adj2 = product_adj2(g.adj)
    src = src_tensor(g.sources)
    ptr, edges = R.two_hop_candidates(g.adj, adj2, src)
    assert int(((ptr[1:] - ptr[:-1]) > m).sum()) > 150
    ref = torch.randint(0, 187, (600, 2), generator=torch.Generator().manual_seed(1)).to(DEV)
    pred.set_frozen_columns(freeze_columns(pred, g.adj, adj2, ref))
    full = score_edges(pred, h, g.adj, adj2, edges, 4096)
    where = torch.full((g.n * g.n,), -1, dtype=torch.int64, device=DEV)
    where[edges[:, 0] * g.n + edges[:, 1]] = torch.arange(edges.shape[0], device=DEV)       # (a repeated source: any of its places)
    dst, score = R.recommend_links(pred, h, g.adj, adj2, src, k, bs, prefilter=("ra", m))
    got = dst >= 0
    assert int(got.sum()) > 400 and torch.equal(got, torch.isfinite(score))
    at = where[(src[:, None] * g.n + dst.clamp(min=0))[got]]
    assert int(at.min()) >= 0                                            # every returned pair is a candidate of its source
    err = (score[got] - full[at]).abs().max().item()
    print(f"frozen cn5, prefilter ('ra', {m}): max|score - unfiltered score| = {err:.3e} over {int(got.sum())} returned pairs")
    assert close(score[got], full[at])
    pred.set_frozen_columns(None)


# ---- 8. the example driver ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [[], ["--recommend-walk"]], ids=["adj2", "walk"])
def test_example_driver_with_a_frozen_prefilter(hiplib, capsys, route):
    """examples/run_like_reference.py --recommend 5 --recommend-frozen --recommend-prefilter ra:5 on the Cora shape: m = 5 is below
    the sources' candidate lists, so the short list does filter; the frozen self-check (half the sources, a third of the batch
    size) compares prefiltered rows with prefiltered rows and passes, and the kept line is printed."""
    import importlib.util
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "run_like_reference.py")
    spec = importlib.util.spec_from_file_location("run_like_reference", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(["--dataset", "cora", "--epochs", "1", "--recommend", "5", "--recommend-frozen", "--recommend-prefilter", "ra:5"] + route)
    out = capsys.readouterr().out
    assert "returns the same rows = True" in out
    kept = re.search(r"^prefilter ra:5 kept (\d+) of the (\d+) unfiltered top-5 links \(the model ranked (\d+) of (\d+) candidates\)$", out, re.M)
    assert kept, out[-2000:]
    k, full, short, cands = map(int, kept.groups())
    assert 0 <= k <= full <= 25 and 0 < short <= 25 and short < cands     # five sources, at most five each: the list was cut
    assert len(re.findall(r"^recommend source \d+ top-5: ", out, re.M)) == 5
    for bad in ("ra:4", "jaccard:8", "ra:200", "ra"):
        with pytest.raises(SystemExit):
            mod.main(["--dataset", "cora", "--recommend", "5", "--recommend-prefilter", bad])
    capsys.readouterr()
