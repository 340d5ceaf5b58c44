"""Link recommendation without a materialised A² on the GPU (``ocn_two_hop_diff_count`` / ``_fill``, ``adj2=None`` in
ocn_amd/recommend.py, ``pipeline.score_edges_walk``).  The references are restatements written here — Python sets over the
rows of A — and, where A² can be formed, the route through the materialised product (``two_hop_candidates(adj, A², ...)``).
Sets and orders are exact, so every comparison is ``torch.equal`` (scores as bit patterns)."""
from collections import defaultdict
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import ocn_oracle as O
from tests.helpers import make_graph, product_adj2, to_product

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ---- the restatements --------------------------------------------------------------------------------------------------
def rows_of(n, pairs, symmetric=True, sparse=False):
    """Row -> set of columns of the graph with these links (``sparse``: a dictionary of the non-empty rows)."""
    rows = defaultdict(set) if sparse else [set() for _ in range(n)]
    for a, b in pairs:
        rows[a].add(b)
        if symmetric:
            rows[b].add(a)
    return rows


def oracle_rows(m):
    rp, col = m.rowptr().tolist(), m.col.tolist()
    return [set(col[rp[r]:rp[r + 1]]) for r in range(m.n_rows)]


def ref_two_hop(a_rows, m_rows, sources, drop_self=True):
    """Per source, ascending: (U_{m in A[s]} A[m]) \\ M[s] (\\ {s}).  Returns (ptr [Q + 1], edges [T, 2])."""
    ptr, pairs = [0], []
    for s in sources:
        out = set()
        for m in a_rows[s]:
            out |= a_rows[m]
        out -= m_rows[s]
        if drop_self:
            out.discard(s)
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


def ref_select(scores, ptr, edges, k):
    val, pos = ref_topk(scores, ptr, k)
    dst = torch.where(pos >= 0, edges[:, 1][pos.clamp(min=0)], torch.full_like(pos, -1)) if edges.shape[0] else torch.full_like(pos, -1)
    return dst, val


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


def csr_of(rows, n):
    """Row sets -> the project's SparseTensor on the device (sorted, duplicate-free rows by construction)."""
    from ocn_amd.sparse import SparseTensor
    items = sorted(rows.items()) if isinstance(rows, dict) else list(enumerate(rows))
    lens = torch.zeros(n, dtype=torch.int64)
    lens[torch.tensor([r for r, _ in items], dtype=torch.int64)] = torch.tensor([len(cs) for _, cs in items], dtype=torch.int64)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = lens.cumsum(0)
    col = torch.tensor([c for _, cs in items for c in sorted(cs)], dtype=torch.int32)
    return SparseTensor(rowptr=rowptr.to(DEV), col=col.to(DEV), sparse_sizes=(n, n))


def src_tensor(sources):
    return torch.tensor(sources, dtype=torch.int64, device=DEV)


def two_hop(adj, known, sources, drop_self=True, window_cols=0):
    """(ptr, edges) through the ops layer, where ``drop_self`` and ``window_cols`` can be chosen."""
    from ocn_amd import ops
    src = src_tensor(sources)
    args = (adj._rowptr, adj._col, known._rowptr, known._col, src)
    count = ops.two_hop_diff_count(*args, drop_self=drop_self, window_cols=window_cols)
    assert count.dtype == torch.int32 and count.shape == (len(sources),)
    off = ops.scan_i32(count)
    edges = ops.two_hop_diff_fill(*args, off, drop_self=drop_self, window_cols=window_cols)
    assert edges.dtype == torch.int64 and edges.dim() == 2 and edges.shape[1] == 2
    return off.cpu(), edges.cpu()


def candidates_of(adj, sources, known=None):
    from ocn_amd import recommend as R
    ptr, edges = R.two_hop_candidates(adj, None, src_tensor(sources), known)
    assert ptr.dtype == torch.int64 and edges.dtype == torch.int64 and edges.dim() == 2 and edges.shape[1] == 2
    p, e = ptr.tolist(), edges.cpu()
    for q, s in enumerate(sources):
        assert bool((e[p[q]:p[q + 1], 0] == s).all())
    return [e[p[q]:p[q + 1], 1].tolist() for q in range(len(sources))]


# ---- the small graph of the single-window and the end-to-end cases ------------------------------------------------------
@pytest.fixture(scope="module")
def small(hiplib):
    """``make_graph(n=300, avg_deg=6, max_deg=80)`` with five isolated nodes and a leaf hung on the hub by hand; the sources
    are all nodes in a shuffled order with ten of them repeated."""
    n, iso = 300, 5
    base = make_graph(n, 6, 80, 33, isolated=iso + 1)
    hub = int(base.rowcount().argmax())
    leaf = n - iso - 1                                                   # isolated so far: its only neighbour becomes the hub
    ei = torch.cat([torch.stack([base.row, base.col]), torch.tensor([[hub], [leaf]])], dim=1)
    oadj = O.to_symmetric(O.from_edge_index(ei, n))
    a_rows = oracle_rows(oadj)
    assert a_rows[leaf] == {hub} and len(a_rows[hub]) == max(len(r) for r in a_rows) >= 20
    assert all(len(a_rows[v]) == 0 for v in range(n - iso, n))
    adj = to_product(oadj, DEV)
    g = torch.Generator().manual_seed(5)
    order = torch.randperm(n, generator=g).tolist()
    sources = order[:150] + order[40:50] + order[150:]
    assert len(sources) == n + 10 and set(sources) == set(range(n))
    ptr, edges = ref_two_hop(a_rows, a_rows, sources)
    return SimpleNamespace(n=n, iso=iso, hub=hub, leaf=leaf, oadj=oadj, adj=adj, a_rows=a_rows, sources=sources, ptr=ptr, edges=edges)


# ---- 1. single window ---------------------------------------------------------------------------------------------------
def test_single_window_equals_the_sets_and_the_materialised_product(small):
    from ocn_amd import ops, recommend as R
    c = small
    assert c.n <= ops.two_hop_window_cols()
    sizes = c.ptr[1:] - c.ptr[:-1]
    assert bool((sizes == 0).any()) and int(sizes.max()) > 64 and int((sizes > 0).sum()) > c.n // 2
    q_leaf = c.sources.index(c.leaf)
    assert int(sizes[q_leaf]) == len(c.a_rows[c.hub]) - 1                # the leaf sees the hub's other neighbours
    src = src_tensor(c.sources)
    ptr, edges = R.two_hop_candidates(c.adj, None, src)
    assert torch.equal(ptr.cpu(), c.ptr) and torch.equal(edges.cpu(), c.edges)
    assert torch.equal(edges[:, 0], torch.repeat_interleave(src, ptr[1:] - ptr[:-1]))
    ptr2, edges2 = R.two_hop_candidates(c.adj, product_adj2(c.adj), src)                      # the route through A²
    assert torch.equal(ptr, ptr2) and torch.equal(edges, edges2)
    ptr3, edges3 = R.two_hop_candidates(c.adj, None, src, known=c.adj)                        # the default, spelled out
    assert torch.equal(ptr, ptr3) and torch.equal(edges, edges3)
    with pytest.raises(IndexError):                                                           # ids are bounds-checked, as every op checks them
        R.two_hop_candidates(c.adj, None, torch.tensor([0, c.n], device=DEV))
    with pytest.raises(IndexError):
        R.two_hop_candidates(c.adj, None, torch.tensor([-1], device=DEV))
    ptr0, edges0 = R.two_hop_candidates(c.adj, None, torch.zeros(0, dtype=torch.int64, device=DEV))
    assert ptr0.tolist() == [0] and edges0.shape == (0, 2) and edges0.dtype == torch.int64
    iso = torch.tensor([c.n - 1, c.n - 2, c.n - 1], device=DEV)
    ptr0, edges0 = R.two_hop_candidates(c.adj, None, iso)
    assert ptr0.tolist() == [0, 0, 0, 0] and edges0.shape == (0, 2)


# ---- 2. closed forms ----------------------------------------------------------------------------------------------------
def test_closed_forms_path_bipartite_and_star(hiplib):
    n = 12
    adj = csr_of(rows_of(n, [(i, i + 1) for i in range(n - 1)]), n)
    assert candidates_of(adj, list(range(n))) == [[c for c in (i - 2, i + 2) if 0 <= c < n] for i in range(n)]
    m, r = 5, 7                                                          # K_{5,7}: left ids 0 .. 4
    adj = csr_of(rows_of(m + r, [(a, m + b) for a in range(m) for b in range(r)]), m + r)
    got = candidates_of(adj, [2, 0, m, m + r - 1])
    assert got[0] == [0, 1, 3, 4] and got[1] == [1, 2, 3, 4]
    assert got[2] == list(range(m + 1, m + r)) and got[3] == list(range(m, m + r - 1))
    leaves = 300                                                         # centre 0, leaves 1 .. 300
    adj = csr_of(rows_of(leaves + 1, [(0, v) for v in range(1, leaves + 1)]), leaves + 1)
    got = candidates_of(adj, [7, 0, 300, 1])
    assert got[0] == [c for c in range(1, leaves + 1) if c != 7] and len(got[0]) == 299
    assert got[1] == []                                                  # from the centre: its 2-hop set is itself
    assert got[2] == list(range(1, 300)) and got[3] == list(range(2, 301))


# ---- 3. several windows through the ops layer ---------------------------------------------------------------------------
BOUNDARY = [63, 64, 65, 127, 128, 191, 192, 198]                         # both sides of every 64-column window and of 32-bit words


@pytest.fixture(scope="module")
def windows(hiplib):
    """199 = 64 * 3 + 7 nodes.  Nodes 20 and 30 link to every boundary column and to a few columns inside the windows, so every
    boundary column is a source (self at a boundary), a candidate (of the other boundary nodes, of 10 and of 11) and — through
    the extra links of ``known`` — a known column."""
    n = 64 * 3 + 7
    pairs = [(h, c) for h in (20, 30) for c in BOUNDARY + [0, 1, 31, 32, 33, 95, 96, 160]]
    pairs += [(10, 20), (11, 64), (11, 128), (12, 198), (12, 0)]
    g = torch.Generator().manual_seed(9)
    rnd = torch.randint(0, n, (150, 2), generator=g).tolist()
    pairs += [(a, b) for a, b in rnd if a != b]
    a_rows = rows_of(n, pairs)
    known = [set(r) for r in a_rows]
    for s, t in [(10, 63), (10, 128), (10, 198), (63, 64), (64, 127), (64, 128), (128, 192), (191, 192), (198, 63), (65, 198), (11, 20)]:
        known[s].add(t)                                                  # (one-sided: known is no adjacency)
    return SimpleNamespace(n=n, a_rows=a_rows, k_rows=known, adj=csr_of(a_rows, n), known=csr_of(known, n),
                           sources=list(range(n)) + BOUNDARY[::-1])


@pytest.mark.parametrize("drop_self", [True, False], ids=["drop_self", "keep_self"])
def test_every_window_size_gives_the_one_window_result(windows, drop_self):
    c = windows
    for name, m_rows, m in (("adj", c.a_rows, c.adj), ("known", c.k_rows, c.known)):
        rptr, redges = ref_two_hop(c.a_rows, m_rows, c.sources, drop_self)
        got = set(redges[:, 1].tolist())
        assert set(BOUNDARY) <= got and redges.shape[0] > 300, name
        ptr0, edges0 = two_hop(c.adj, m, c.sources, drop_self, 0)
        assert torch.equal(ptr0, rptr) and torch.equal(edges0, redges), name
        for w in (64, 128, 192):
            ptr, edges = two_hop(c.adj, m, c.sources, drop_self, w)
            assert torch.equal(ptr, ptr0) and torch.equal(edges, edges0), (name, w)
    p = ref_two_hop(c.a_rows, c.a_rows, [10], True)[1][:, 1].tolist()
    k = ref_two_hop(c.a_rows, c.k_rows, [10], True)[1][:, 1].tolist()
    assert set(p) - set(k) == {63, 128, 198}                             # the known columns at the boundaries were candidates


# ---- 4. the default window crossed --------------------------------------------------------------------------------------
def test_graph_wider_than_the_default_window(hiplib):
    """n = window + 65: more columns than the A·A pattern kernel takes.  Source 5 reaches window - 1, window, window + 1 and n - 1
    through two neighbours, one on each side of the window; source n - 2 lies beyond the window itself."""
    from ocn_amd import ops, recommend as R
    W = ops.two_hop_window_cols()
    n = W + 65
    assert n > ops.spgemm_max_cols()
    far = [W - 1, W, W + 1, n - 1]
    pairs = [(5, 7), (5, W + 3)]
    pairs += [(7, c) for c in far + [9, 100, 4097, W - 64, W - 33]]
    pairs += [(W + 3, c) for c in far + [2, W + 31, W + 32, W + 64]]
    pairs += [(n - 2, n - 3), (n - 2, 11), (n - 3, W), (n - 3, 0), (n - 3, n - 1), (11, 12), (11, W - 1), (11, W + 40)]
    pairs += [(1000 + 3 * i, 2000 + 5 * i) for i in range(100)] + [(2000 + 5 * i, W + i % 60) for i in range(100)]
    a_rows = rows_of(n, pairs, sparse=True)
    adj = csr_of(a_rows, n)
    sources = [5, n - 2, W, 7, W + 3, 0, n - 1, 1000, 2000, W - 1, 5]
    rptr, redges = ref_two_hop(a_rows, a_rows, sources)
    assert set(far) <= set(redges[rptr[0]:rptr[1], 1].tolist())
    assert {W, 0, n - 1, 12, W - 1, W + 40} <= set(redges[rptr[1]:rptr[2], 1].tolist())
    ptr, edges = R.two_hop_candidates(adj, None, src_tensor(sources))
    assert torch.equal(ptr.cpu(), rptr) and torch.equal(edges.cpu(), redges)
    with pytest.raises(NotImplementedError):                             # what the route lifts: A² cannot be formed at this n
        ops.spgemm_pattern(adj._rowptr, adj._col, adj._rowptr, adj._col, n)


# ---- 4b. one LDS limit for launches of any width, in any order ----------------------------------------------------------
def test_narrow_wide_narrow_launches_in_one_process(small):
    """The dynamic LDS limit of the kernel is raised once per device, not per launch: a 300-column launch, then one whose bitmap
    (600 000 columns: 75 000 bytes) is larger than the 65 536 bytes a kernel may ask for without the raised limit, then the
    300-column one again.  The wide graph: 2 000 random links among 1 500 nodes drawn from the whole column range (so that the
    2-hop sets are not empty); its sources are seven of those nodes and one isolated node."""
    c = small
    n = 600_000
    assert n // 8 > 65536
    g = torch.Generator().manual_seed(21)
    nodes = torch.randperm(n, generator=g)[:1500]
    ends = nodes[torch.randint(0, nodes.numel(), (2000, 2), generator=g)]
    a_rows = rows_of(n, [(a, b) for a, b in ends.tolist() if a != b], sparse=True)
    linked = sorted(a_rows)
    isolated = next(v for v in range(n - 1, -1, -1) if v not in a_rows)
    sources = linked[::len(linked) // 6][:6] + [linked[-1], isolated]
    assert len(sources) == 8
    wide = csr_of(a_rows, n)
    rptr, redges = ref_two_hop(a_rows, a_rows, sources)
    sizes = (rptr[1:] - rptr[:-1]).tolist()
    assert sum(1 for x in sizes if x > 0) >= 4 and sizes[-1] == 0 and int(redges[:, 1].max()) > 65536 * 8
    first = two_hop(c.adj, c.adj, c.sources)
    ptr, edges = two_hop(wide, wide, sources)
    assert torch.equal(ptr, rptr) and torch.equal(edges, redges)
    again = two_hop(c.adj, c.adj, c.sources)
    for ptr, edges in (first, again):
        assert torch.equal(ptr, c.ptr) and torch.equal(edges, c.edges)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


# ---- 5. known differs from adj ------------------------------------------------------------------------------------------
def test_known_superset_long_row_and_an_empty_segment_between_full_ones(hiplib):
    from ocn_amd import ops
    stage = ops.row_diff_stage_cols()
    n = 2 * stage + 200
    ring = [(i, (i + 1) % n) for i in range(n)] + [(i, (i + 7) % n) for i in range(0, n, 3)]
    a_rows = rows_of(n, ring)
    known = [set(r) for r in a_rows]
    long_s, full_s = 40, 41
    known[long_s] |= set(range(0, n, 2)) - {long_s, long_s + 2}                  # a known row longer than the row difference stages
    assert len(known[long_s]) > stage
    full = set()
    for m in a_rows[full_s]:
        full |= a_rows[m]
    known[full_s] |= full - {full_s}                                     # its whole 2-hop set is known ...
    known[100] |= {102}
    adj, kn = csr_of(a_rows, n), csr_of(known, n)
    sources = [39, long_s, full_s, 42, 100, full_s, long_s, 99]
    for drop_self in (True, False):
        rptr, redges = ref_two_hop(a_rows, known, sources, drop_self)
        sizes = (rptr[1:] - rptr[:-1]).tolist()
        if drop_self:
            assert sizes[2] == 0 and sizes[1] > 0 and sizes[3] > 0 and sizes[5] == 0       # ... an empty segment between full ones
        else:
            assert sizes[2] == 1 and all(len(a_rows[s]) >= 1 for s in sources)           # only s itself is left of it
            assert int((redges[:, 0] == redges[:, 1]).sum()) == len(sources)
        ptr, edges = two_hop(adj, kn, sources, drop_self)
        assert torch.equal(ptr, rptr) and torch.equal(edges, redges), drop_self
    from ocn_amd import recommend as R
    ptr, edges = R.two_hop_candidates(adj, None, src_tensor(sources), known=kn)
    rptr, redges = ref_two_hop(a_rows, known, sources)
    assert torch.equal(ptr.cpu(), rptr) and torch.equal(edges.cpu(), redges)
    p2, e2 = R.two_hop_candidates(adj, product_adj2(adj), src_tensor(sources), known=kn)
    assert torch.equal(ptr, p2) and torch.equal(edges, e2)


# ---- 6. the fill pass never overruns its segment ------------------------------------------------------------------------
def test_fill_with_foreign_offsets_writes_nothing_past_its_segment(windows):
    """Offsets counted against a LARGER known leave every segment too short for the sets of ``adj``: the fill pass then writes
    the first pairs of every set and nothing at or beyond off[q + 1] — nor beyond off[Q], where a sentinel tail waits."""
    from ocn_amd import _lib, ops
    from ocn_amd._lib import ptr, stream_ptr
    c = windows
    src = src_tensor(c.sources)
    Q = len(c.sources)
    off = ops.scan_i32(ops.two_hop_diff_count(c.adj._rowptr, c.adj._col, c.known._rowptr, c.known._col, src))
    rptr, redges = ref_two_hop(c.a_rows, c.a_rows, c.sources)
    short = off.cpu()
    assert int(short[-1]) < int(rptr[-1]) and bool(((short[1:] - short[:-1]) <= (rptr[1:] - rptr[:-1])).all())
    for w in (0, 64):
        T, tail = int(short[-1]), 64
        edges = torch.full((T + tail, 2), -7, dtype=torch.int64, device=DEV)
        st = _lib.lib().ocn_two_hop_diff_fill(ptr(c.adj._rowptr), ptr(c.adj._col), ptr(c.adj._rowptr), ptr(c.adj._col), c.n, ptr(src), Q,
                                              1, w, ptr(off), ptr(edges), stream_ptr())
        assert st == 0
        got = edges.cpu()
        assert bool((got[T:] == -7).all())
        for q in range(Q):
            a, b = int(short[q]), int(short[q + 1])
            assert torch.equal(got[a:b], redges[int(rptr[q]):int(rptr[q]) + (b - a)]), (w, q)


# ---- 7. a hub source ----------------------------------------------------------------------------------------------------
def test_hub_source_whose_neighbours_overlap_heavily(hiplib):
    """A hub of degree 2 000 whose neighbours all link to the same 40 columns (and to a few of their own): every one of those
    bits is set 2 000 times, from every lane of every wave — a set that is not atomic would lose columns."""
    n, deg = 6000, 2000
    spokes = list(range(100, 100 + deg))
    shared = list(range(3000, 3040)) + [2999, 3071, 3072, 5999]
    pairs = [(0, v) for v in spokes]
    pairs += [(v, c) for v in spokes for c in shared]
    pairs += [(v, 4000 + (v * 7) % 1500) for v in spokes] + [(v, v + 1) for v in spokes[::2]]
    a_rows = rows_of(n, pairs)
    assert len(a_rows[0]) == deg
    adj = csr_of(a_rows, n)
    sources = [0, 3000, 150, 0, 5999, 1]
    rptr, redges = ref_two_hop(a_rows, a_rows, sources)
    assert int(rptr[1]) > 1000 and set(shared) <= set(redges[:int(rptr[1]), 1].tolist())
    for drop_self in (True, False):
        rptr, redges = ref_two_hop(a_rows, a_rows, sources, drop_self)
        ptr, edges = two_hop(adj, adj, sources, drop_self)
        assert torch.equal(ptr, rptr) and torch.equal(edges, redges)
    from ocn_amd import recommend as R
    p1, e1 = R.two_hop_candidates(adj, None, src_tensor(sources))
    p2, e2 = R.two_hop_candidates(adj, product_adj2(adj), src_tensor(sources))
    assert torch.equal(p1, p2) and torch.equal(e1, e2)


# ---- 8. end to end ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bs", [("cn5", 1000), ("cn7", 2100)], ids=["cn5_one_stream", "cn7_side_streams"])
def test_recommend_links_walk_equals_score_edges_walk_and_the_restatement(small, name, bs):
    """The contract: the scores are exactly those ``score_edges_walk`` returns for the flat candidate list at that batch size,
    selected per source by the stated order; and ``score_edges_walk`` is the loop ``score_mrr_split`` runs.  The smaller batch
    runs on one stream, the larger one (``ops.overlap_min_batch`` and up) with phase A on side streams."""
    from ocn_amd import recommend as R
    from ocn_amd.model import predictor_dict
    from ocn_amd.pipeline import score_edges_walk, score_mrr_split
    c = small
    H = 64
    torch.manual_seed(12)
    h = torch.randn(c.n, H, device=DEV)
    pred = predictor_dict[name](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()
    args = SimpleNamespace(sum=0.5)
    src = src_tensor(c.sources)
    ptr, edges = R.two_hop_candidates(c.adj, None, src)
    T = edges.shape[0]
    assert T > 2 * bs and T % bs != 0                                    # several batches and a ragged last one
    flat = score_edges_walk(pred, h, c.adj, edges, bs, args)
    assert flat.shape == (T,) and flat.dtype == torch.float32 and bool(torch.isfinite(flat).all())
    neg = edges[:, 1:2].flip(0).contiguous()                             # any one-column target_neg
    pos_pred, _ = score_mrr_split(pred, h, c.adj, edges[:, 0].contiguous(), edges[:, 1].contiguous(), neg, bs, args)
    assert same_bits(flat, pos_pred)
    for k in (1, 10, 128):
        dst, score = R.recommend_links(pred, h, c.adj, None, src, k, bs, args)
        assert dst.shape == (len(c.sources), k) and dst.dtype == torch.int64 and score.dtype == torch.float32
        rdst, rscore = ref_select(flat.cpu(), ptr.cpu(), edges.cpu(), k)
        assert torch.equal(dst.cpu(), rdst) and same_bits(score, rscore), k
    sizes = (ptr[1:] - ptr[:-1]).cpu()
    assert bool((sizes == 0).any()) and bool(((dst.cpu() == -1).sum(1) == (k - sizes.clamp(max=k))).all())
    for q, s in enumerate(c.sources):                                    # a recommendation is a 2-hop neighbour that is no link yet
        picked = [t for t in dst[q].tolist() if t >= 0]
        assert len(set(picked)) == len(picked) and all(t not in c.a_rows[s] and t != s for t in picked)
        assert all(c.a_rows[s] & c.a_rows[t] for t in picked)
    with pytest.raises(RuntimeError, match="eval path"):
        R.recommend_links(pred.train(), h, c.adj, None, src, 10, bs, args)


def test_one_hop_heuristic_does_not_read_adj2(small):
    from ocn_amd import recommend as R
    c = small
    src = src_tensor(c.sources)
    adj2 = product_adj2(c.adj)
    for kind, k in (("ra", 10), ("cn", 128), ("jaccard", 1)):
        dst, score = R.recommend_links_heuristic(c.adj, None, src, k, 700, kind)
        rdst, rscore = R.recommend_links_heuristic(c.adj, adj2, src, k, 700, kind)
        assert torch.equal(dst, rdst) and same_bits(score, rscore), kind
        assert int((dst >= 0).sum()) > len(c.sources) // 2 and bool((score[dst >= 0] > 0).all())
    with pytest.raises(ValueError, match="adj2, which is None"):
        R.recommend_links_heuristic(c.adj, None, src, 10, 700, "ra2")
