"""Frontier expansion with ordered path sums on the GPU (``ocn_frontier_count`` / ``ocn_frontier_sums_fill``) and the 3-hop
recommendation built from it (``recommend.three_hop_candidates``, ``path_scored_candidates``, ``prefilter_candidates(hops=3)``,
``recommend_links(hops=3)``).  The references: closed forms worked out by hand, dense integer matrix powers, the existing 2-hop
kernels, and a numpy ``float32`` loop in the documented order (seed first, then one add per frontier member in ascending node
id).  Sets, orders and sums are exact: every comparison of a list is ``torch.equal``, of a value its bits."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import close, product_adj2
from tests.test_prefilter_gpu import bits, csr_of, kind_weight, make_predictor, ref_prefilter, ref_select, src_tensor, sym_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KINDS = ("cn", "aa", "ra")
F0 = np.float32(0.0)


# ---- the restatements --------------------------------------------------------------------------------------------------
def ref_expand_one(a_rows, m_rows, s, F, S=(), drop_self=True, descending=False, seed_last=False):
    """One query in the documented order: {t: seed value of t (else 0.0f) + f_c for every (c, f_c) of F whose row holds t, one
    fp32 add per member in ascending c} without the columns of M[s] and, under drop_self, s.  ``descending`` / ``seed_last``: the
    orders the contract rules out, for the tests that show the order decides the bits."""
    acc = {} if seed_last else {t: np.float32(v) for t, v in S}
    for c, f in sorted(F, reverse=descending):
        for t in a_rows.get(c, ()):
            acc[t] = np.float32(acc.get(t, F0) + np.float32(f))
    if seed_last:
        for t, v in S:
            acc[t] = np.float32(acc.get(t, F0) + np.float32(v))
    for t in m_rows.get(s, ()):
        acc.pop(t, None)
    if drop_self:
        acc.pop(s, None)
    return sorted(acc.items())


def flat(per_query, sources):
    """[(node, value)] per query -> (ptr [Q + 1], pairs [T, 2] of (source, node), val [T]) on the host."""
    ptr, pairs, vals = [0], [], []
    for s, items in zip(sources, per_query):
        pairs += [(s, c) for c, _ in items]
        vals += [v for _, v in items]
        ptr.append(len(pairs))
    return (torch.tensor(ptr, dtype=torch.int64), torch.tensor(pairs, dtype=torch.int64).reshape(-1, 2),
            torch.from_numpy(np.array(vals, dtype=np.float32)))


def ref_path3(a_rows, m_rows, sources, weight, decay, **kw):
    """``path_scored_candidates(hops=3)`` restated: L2 unexcluded with u = P2 (ascending m), f = (decay32 * w[c]) * u, then the
    expansion of (L2, f) seeded with (L2, u), without M[s] and s.  Each distinct source once."""
    d32, per = np.float32(decay), {}
    for s in sources:
        if s in per:
            continue
        u = ref_expand_one(a_rows, {}, s, [(m, weight[m]) for m in a_rows.get(s, ())], drop_self=False)
        f = [(c, np.float32(np.float32(d32 * np.float32(weight[c])) * uc)) for c, uc in u]
        per[s] = ref_expand_one(a_rows, m_rows, s, f, u, **kw)
    return flat([per[s] for s in sources], sources)


def dev_list(lst):
    ptr, pairs, val = lst
    return ptr.to(DEV), pairs.to(DEV), (None if val is None else val.to(DEV))


def expand(adj, known, sources, F, S=None, drop_self=True, window=0, values=True):
    """count -> scan -> fill through the ops layer: (ptr, edges, val) on the host."""
    from ocn_amd import ops
    src = src_tensor(sources)
    pF, nF, vF = dev_list(F)
    pS, nS, vS = dev_list(S) if S is not None else (None, None, None)
    A = (adj._rowptr, adj._col, known._rowptr, known._col, src)
    count = ops.frontier_count(*A, pF, nF, pS, nS, drop_self=drop_self, window_cols=window)
    assert count.dtype == torch.int32 and count.shape == (len(sources),)
    off = ops.scan_i32(count)
    edges, val = ops.frontier_sums_fill(*A, pF, nF, vF, pS, nS, vS, off, drop_self=drop_self, window_cols=window, values=values)
    assert edges.dtype == torch.int64 and edges.shape == (int(off[-1]), 2)
    assert (val is None) if not values else (val.dtype == torch.float32 and val.shape == (edges.shape[0],))
    return off.cpu(), edges.cpu(), (None if val is None else val.cpu())


def same(got, want, what=""):
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), what
    if want[2] is not None and got[2] is not None:
        assert torch.equal(bits(got[2]), bits(want[2])), what


def empty_adj(n):
    return csr_of({}, n)


def as_dict(lst, q):
    ptr, edges, val = (t.cpu() for t in lst)
    return dict(zip(edges[ptr[q]:ptr[q + 1], 1].tolist(), val[ptr[q]:ptr[q + 1]].tolist()))


# ---- 1. closed forms ------------------------------------------------------------------------------------------------------
def path_graph(n):
    return sym_rows(n, [(v, v + 1) for v in range(n - 1)])


def cycle_graph(n):
    return sym_rows(n, [(v, (v + 1) % n) for v in range(n)])


def tree_graph():
    """root 0; children 1, 2; their children 3 - 5 and 6 - 8; two leaves under each of those: 9 - 20."""
    pairs = [(0, 1), (0, 2)] + [(1, c) for c in (3, 4, 5)] + [(2, c) for c in (6, 7, 8)]
    pairs += [(p, 9 + 2 * (p - 3) + j) for p in range(3, 9) for j in (0, 1)]
    return sym_rows(21, pairs)


def test_closed_forms_with_unit_weights(hiplib):
    """decay = 0.5, "cn": val = A² + A³ / 2 by hand.  P8, C7 and the tree are bipartite-like at this range: a target is reached
    by 2-paths or by 3-walks, never both; in C5 node 3 gets one 2-path (0-4-3) and one 3-walk (0-1-2-3) from node 0."""
    from ocn_amd import recommend as R
    cases = [
        (path_graph(8), 8, [0, 3, 7], [{2: 1.0, 3: 0.5}, {1: 1.0, 5: 1.0, 0: 0.5, 6: 0.5}, {5: 1.0, 4: 0.5}]),
        (cycle_graph(5), 5, [0], [{2: 1.5, 3: 1.5}]),
        (cycle_graph(7), 7, [0], [{2: 1.0, 5: 1.0, 3: 0.5, 4: 0.5}]),
        (tree_graph(), 21, [0, 9], [{**{c: 1.0 for c in range(3, 9)}, **{c: 0.5 for c in range(9, 21)}},
                                    {10: 1.0, 1: 1.0, 4: 0.5, 5: 0.5, 0: 0.5}]),
    ]
    for rows, n, sources, want in cases:
        adj = csr_of(rows, n)
        got = R.path_scored_candidates(adj, src_tensor(sources), "cn", 3, 0.5)
        cptr, cedges = R.three_hop_candidates(adj, src_tensor(sources))
        assert torch.equal(cptr, got[0]) and torch.equal(cedges, got[1])
        p2, e2 = R.two_hop_candidates(adj, None, src_tensor(sources))
        for q, s in enumerate(sources):
            assert as_dict(got, q) == want[q], (n, s)
            two = set(e2[p2[q]:p2[q + 1], 1].tolist())
            assert two == {t for t, v in want[q].items() if v >= 1.0}          # the 2-hop targets are those with a 2-path
            if n != 5:
                assert all(v in (1.0, 0.5) for v in want[q].values())            # ... and disjoint from the 3-walk ones


def test_closed_forms_with_ra_weights(hiplib):
    """decay = 0.5, "ra": w = 1 / deg.  P8 from node 0: P2(0, 2) = w[1] = 1/2, and 3 is reached through c = 2 alone:
    (0.5 * w[2]) * P2(0, 2) = 1/8.  C5 from node 0 (every w = 1/2): node 3 = its seed 1/2 + (0.5 * w[2]) * P2(0, 2) = 1/2 + 1/8.
    The tree from its root: a grandchild 1/4 (its parent has degree 4), a leaf (0.5 * w[grandchild]) * 1/4 with w = 1/3 rounded."""
    from ocn_amd import recommend as R
    adj = csr_of(path_graph(8), 8)
    assert as_dict(R.path_scored_candidates(adj, src_tensor([0]), "ra", 3, 0.5), 0) == {2: 0.5, 3: 0.125}
    adj = csr_of(cycle_graph(5), 5)
    assert as_dict(R.path_scored_candidates(adj, src_tensor([0]), "ra", 3, 0.5), 0) == {2: 0.625, 3: 0.625}
    adj = csr_of(tree_graph(), 21)
    w = kind_weight(adj, "ra")
    assert w[1] == np.float32(0.25) and w[9] == np.float32(1.0)
    leaf = float(np.float32(np.float32(np.float32(0.5) * w[3]) * np.float32(0.25)))
    want = {**{c: 0.25 for c in range(3, 9)}, **{c: leaf for c in range(9, 21)}}
    assert as_dict(R.path_scored_candidates(adj, src_tensor([0]), "ra", 3, 0.5), 0) == want
    same(R.path_scored_candidates(adj, src_tensor([0, 9, 3]), "ra", 3, 0.5), ref_path3(tree_graph(), tree_graph(), [0, 9, 3], w, 0.5))


# ---- the 200-node graph of the prefilter tests --------------------------------------------------------------------------------
N, HUB, ISOLATED = 200, 3, (187, 188, 189)


@pytest.fixture(scope="module")
def graph(hiplib):
    """Symmetric, random, 187 nodes at a density of 3 %; node 3 is a hub of 80 links; 187 - 189 are isolated (an empty frontier);
    190 - 192 a triangle of their own; 193 - 199 a path.  Sources: every node in a shuffled order, thirty of them repeated."""
    rng = np.random.default_rng(17)
    a = np.triu(rng.random((187, 187)) < 0.03, 1)
    pairs = list(zip(*np.nonzero(a))) + [(HUB, v) for v in range(100, 180)]
    pairs += [(190, 191), (191, 192), (190, 192)] + [(v, v + 1) for v in range(193, 199)]
    a_rows = sym_rows(N, [(int(x), int(y)) for x, y in pairs])
    adj = csr_of(a_rows, N)
    order = torch.randperm(N, generator=torch.Generator().manual_seed(2)).tolist()
    sources = order[:120] + order[30:60] + order[120:]
    return SimpleNamespace(n=N, a_rows=a_rows, adj=adj, sources=sources, _ref={})


def ref3(g, kind, decay=0.5):
    if (kind, decay) not in g._ref:
        g._ref[(kind, decay)] = ref_path3(g.a_rows, g.a_rows, g.sources, kind_weight(g.adj, kind), decay)
    return g._ref[(kind, decay)]


# ---- 2. agreement with the existing kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_rows_of_a_as_the_frontier_is_the_two_hop_kernel(graph, kind):
    """F = the row of s in A, valF = w[m], no seed: counts, pairs and values of ocn_two_hop_diff_count / _sums_fill bit for bit."""
    from ocn_amd import ops
    from ocn_amd.heuristics import node_table
    g = graph
    w, wcol = (None, 0) if kind == "cn" else (node_table(g.adj), 0 if kind == "aa" else 1)
    weight = kind_weight(g.adj, kind)
    F = flat([[(m, weight[m]) for m in sorted(g.a_rows[s])] for s in g.sources], g.sources)
    src = src_tensor(g.sources)
    A = (g.adj._rowptr, g.adj._col, g.adj._rowptr, g.adj._col, src)
    count = ops.two_hop_diff_count(*A)
    off = ops.scan_i32(count)
    edges, val = ops.two_hop_sums_fill(*A, off, w, wcol)
    assert edges.shape[0] > 2000
    pF, nF, vF = dev_list(F)
    for window in (0, 64):
        assert torch.equal(ops.frontier_count(*A, pF, nF, window_cols=window), count), window
        same(expand(g.adj, g.adj, g.sources, F, window=window), (off.cpu(), edges.cpu(), val.cpu()), window)
        if kind == "cn":                                                   # unit weights by default, and the pairs alone
            same(expand(g.adj, g.adj, g.sources, (F[0], F[1], None), window=window), (off.cpu(), edges.cpu(), val.cpu()), window)
            p, e, v = expand(g.adj, g.adj, g.sources, F, window=window, values=False)
            assert v is None and torch.equal(e, ops.two_hop_diff_fill(*A, off).cpu())


# ---- 3. walk counts ------------------------------------------------------------------------------------------------------------
def test_chained_expansions_count_walks_exactly(hiplib):
    """Unit weights, decay = 1, n = 200: chained to 3 and to 4 hops the values are the dense A² + A³ (+ A⁴) entries — integers
    below 2^24, so exact in any order — and the presence bits their non-zero pattern."""
    from ocn_amd import recommend as R
    n = 200
    rng = np.random.default_rng(5)
    a = np.triu(rng.random((n, n)) < 0.03, 1)
    a_rows = sym_rows(n, [(int(x), int(y)) for x, y in zip(*np.nonzero(a))])
    adj, none = csr_of(a_rows, n), empty_adj(n)
    A1 = np.zeros((n, n), dtype=np.int64)
    for r, cs in a_rows.items():
        A1[r, list(cs)] = 1
    A2 = A1 @ A1
    A3, A4 = A2 @ A1, A2 @ A2
    assert (A2 + A3 + A4).max() < (1 << 24) and ((A3 > 0) & (A2 == 0)).sum() > 500
    sources = list(range(n))

    def dense(M):
        ptr, pairs, vals = [0], [], []
        for s in sources:
            cols = np.nonzero(M[s])[0]
            pairs += [(s, int(c)) for c in cols]
            vals += [float(M[s, c]) for c in cols]
            ptr.append(len(pairs))
        return torch.tensor(ptr), torch.tensor(pairs).reshape(-1, 2), torch.tensor(vals, dtype=torch.float32)

    L1 = flat([[(m, 1.0) for m in sorted(a_rows[s])] for s in sources], sources)
    L2 = expand(adj, none, sources, L1, drop_self=False)
    same(L2, dense(A2), "A²")
    S3 = expand(adj, none, sources, L2, L2, drop_self=False)
    same(S3, dense(A2 + A3), "A² + A³")
    L3 = expand(adj, none, sources, L2, drop_self=False)
    same(L3, dense(A3), "A³")
    for window in (0, 64):
        same(expand(adj, none, sources, L3, S3, drop_self=False, window=window), dense(A2 + A3 + A4), "A² + A³ + A⁴")
    lpi = (A2 + A3) * (1 - A1) * (1 - np.eye(n, dtype=np.int64))
    same(R.path_scored_candidates(adj, src_tensor(sources), "cn", 3, 1.0), dense(lpi), "local path index")
    same(R.three_hop_candidates(adj, src_tensor(sources)) + (None,), dense(lpi)[:2] + (None,), "its pattern")


# ---- 4. the order decides the bits ------------------------------------------------------------------------------------------
BIG = {5: 1e8, 10: 1.0, 20: -1e8, 33: 3e-1, 70: 1.0, 71: 3e-1, 90: 0.0, 130: -2.5, 131: 0.7, 150: 1.1, 160: 2.0, 199: 7.0}
TARGETS = [15, 16, 17, 31, 32, 47, 48, 63, 64, 65, 79, 80, 127, 128, 129, 191, 192, 198]   # both sides of every quarter and window edge
ONES = {40: 1e8, 41: 1.0, 42: -1e8, 43: 0.3}                                              # rows of one column: they meet in column 120
MANY = list(range(100, 127)) + list(range(132, 150)) + list(range(151, 160)) + list(range(161, 190))   # 83 more: a second batch of 64


@pytest.fixture(scope="module")
def ordered(hiplib):
    """A directed hand-built A of 200 columns.  The frontier nodes BIG have rows over TARGETS (each without one of them), so a
    target collects an ascending run of 1e8, 1, -1e8, 0.3 ...; node 70 has a row of more than 64 entries, node 199 an empty one.
    ONES have one-column rows that all name column 120, MANY one-column rows that name 121 (weights drawn from ±1e8, 16, 3, 1 and 0.3) or a
    column of their own: runs of one-column hits whose lanes meet in a column, across two batches of 64 entries.  Seeds put
    1.0, 0.25 or -1e8 under some of those columns first."""
    n = 200
    rows = {}
    mids = sorted(BIG)
    for j, m in enumerate(mids):
        rows[m] = set(TARGETS) - {TARGETS[(2, 0, 9, 1, 3, 4, 5, 6, 7, 8, 10, 11)[j]]}
    rows[70] |= set(range(20, 200, 2)) - {70}
    rows[199] = set()
    rows[90] |= {101}
    rows[5] |= {103}
    rows[20] |= {103}
    for m in ONES:
        rows[m] = {120}
    weight = dict(BIG)
    weight.update(ONES)
    pool = np.random.default_rng(7).choice([1e8, -1e8, 1.0, 3.0, 0.3, 16.0], len(MANY))
    for i, m in enumerate(MANY):
        rows[m] = {121} if i % 3 else {(7 * i) % 200}
        weight[m] = float(pool[i])
    frontier = sorted(weight)
    assert len(frontier) > 64 and len(rows[70]) > 64
    per_q = [[(c, weight[c]) for c in frontier],                           # everything
             [(c, weight[c]) for c in frontier if c not in (5, 41)],       # other runs
             [],                                                           # an empty frontier, seeds alone
             [(c, weight[c]) for c in frontier if c < 100]]
    seeds = [[(16, 1.0), (64, -1e8), (103, 0.25), (120, 1.0), (121, 1.0), (151, 2.0)],
             [(15, 1.0), (120, -1e8), (121, 0.25), (198, 1.0)],
             [(7, 3.0), (120, -1.0), (199, 0.0)],
             []]
    return SimpleNamespace(n=n, rows=rows, adj=csr_of(rows, n), per_q=per_q, seeds=seeds, sources=[0, 1, 2, 1])


def test_seed_first_and_ascending_c_decide_the_bits(ordered):
    c = ordered
    none = empty_adj(c.n)

    def ref(**kw):
        return flat([ref_expand_one(c.rows, {}, s, F, S, drop_self=False, **kw) for s, F, S in zip(c.sources, c.per_q, c.seeds)], c.sources)

    want, desc, last = ref(), ref(descending=True), ref(seed_last=True)
    assert torch.equal(want[1], desc[1]) and torch.equal(want[1], last[1])
    d_desc, d_last = bits(want[2]) != bits(desc[2]), bits(want[2]) != bits(last[2])
    print(f"ordered: {want[2].numel()} pairs, {int(d_desc.sum())} differ in descending c, {int(d_last.sum())} with the seed added last")
    cols = want[1][:, 1]
    assert int(d_desc.sum()) > 15 and int(d_last.sum()) >= 3
    for col in (120, 121):                                                 # the columns the one-column runs meet in
        assert bool(d_desc[cols == col].any()), col
    for col in (103, 120):                                                 # a seed under 1e8 - 1e8: first it is lost, last it survives
        assert bool(d_last[cols == col].any()), col
    first = as_dict(want, 0)
    assert first[101] == 0.0 and first[151] == 2.0 and first[7 * 3 % 200] != 0.0     # a zero sum is a member; a seed nobody adds to
    assert as_dict(want, 2) == {7: 3.0, 120: -1.0, 199: 0.0}                         # seeds alone, a zero seed included
    F, S = flat(c.per_q, c.sources), flat(c.seeds, c.sources)
    for window in (0, 64, 128):
        same(expand(c.adj, none, c.sources, F, S, drop_self=False, window=window), want, window)
        p, e, v = expand(c.adj, none, c.sources, F, S, drop_self=False, window=window, values=False)
        assert v is None and torch.equal(p, want[0]) and torch.equal(e, want[1])
    # M = A, drop_self: source 1's own column and its (empty) row change nothing but the dropped pairs
    same(expand(c.adj, c.adj, c.sources, F, S, drop_self=True, window=64),
         flat([ref_expand_one(c.rows, c.rows, s, F_, S_) for s, F_, S_ in zip(c.sources, c.per_q, c.seeds)], c.sources))


# ---- 5. the sweep and the edge cases ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graph300(hiplib):
    n = 300
    rng = np.random.default_rng(41)
    a = np.triu(rng.random((n, n)) < 0.025, 1)
    a_rows = sym_rows(n, [(int(x), int(y)) for x, y in zip(*np.nonzero(a))])
    a_rows[299], a_rows[298] = set(), set()
    for v in range(n):
        a_rows[v] -= {298, 299}
    return SimpleNamespace(n=n, a_rows=a_rows, adj=csr_of(a_rows, n))


def test_window_64_on_300_columns_equals_the_default(graph300):
    g = graph300
    sources = list(range(0, 300, 3)) + [299, 5, 5]
    w = kind_weight(g.adj, "ra")
    want = ref_path3(g.a_rows, g.a_rows, sources, w, 0.5)
    assert want[1].shape[0] > 10000
    L2 = flat([ref_expand_one(g.a_rows, {}, s, [(m, w[m]) for m in g.a_rows[s]], drop_self=False) for s in sources], sources)
    f = torch.from_numpy(np.array([np.float32(np.float32(np.float32(0.5) * w[c]) * u) for c, u in zip(L2[1][:, 1].tolist(), L2[2].numpy())],
                                  dtype=np.float32))
    for window in (0, 64, 192):
        same(expand(g.adj, g.adj, sources, (L2[0], L2[1], f), L2, window=window), want, window)


def test_graph_wider_than_the_default_window(hiplib):
    """n = W + 65 for W = ``ocn_frontier_window_cols()``: the frontier rows of source 5 reach W - 1, W, W + 1 and n - 1, through
    members on both sides of the window's edge; seeds lie on both sides too."""
    from ocn_amd import ops, recommend as R
    W = ops.frontier_window_cols()
    assert 64 <= W <= ops.two_hop_sums_window_cols() and W % 64 == 0
    n = W + 65
    far = [W - 1, W, W + 1, n - 1]
    pairs = [(5, 7), (5, W + 3), (5, 9000)]
    pairs += [(7, c) for c in far + [9, 100, 4097, W - 64, W - 33]]
    pairs += [(W + 3, c) for c in far + [2, W + 31, W + 32, W + 64]]
    pairs += [(9000, c) for c in far[1:] + [9, 2, W // 2, W // 4 - 1, W // 4, 3 * (W // 4) - 1, 3 * (W // 4)]]
    pairs += [(n - 2, n - 3), (n - 2, 11), (n - 3, W), (n - 3, 0), (n - 3, n - 1), (11, 12), (11, W - 1), (11, W + 40)]
    pairs += [(W - 1, 20), (W, 21), (W + 1, 22), (n - 1, 23), (100, W + 7)]
    a_rows = sym_rows(n, pairs)
    adj = csr_of(a_rows, n)
    sources = [5, n - 2, W, 7, n - 1, 5]
    for kind in ("cn", "ra"):
        want = ref_path3(a_rows, a_rows, sources, kind_weight(adj, kind), 0.5)
        mine = as_dict(want, 0)
        assert set(far) | {20, 21, 22, 23, W + 7} <= set(mine)             # 2-hop targets beyond the edge, 3-hop ones on both sides
        same(R.path_scored_candidates(adj, src_tensor(sources), kind, 3, 0.5), want, kind)
    got = R.three_hop_candidates(adj, src_tensor(sources))
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])


def test_grid_stride_over_five_thousand_sources(graph):
    g = graph
    from ocn_amd import recommend as R
    sources = torch.randint(0, g.n, (5000,), generator=torch.Generator().manual_seed(8)).tolist()
    want = ref_path3(g.a_rows, g.a_rows, sources, kind_weight(g.adj, "ra"), 0.5)
    same(R.path_scored_candidates(g.adj, src_tensor(sources), "ra", 3, 0.5), want)


def test_repeated_sources_empty_lists_known_superset_and_self(graph):
    """Sources repeat and some are isolated (an empty frontier, no seed: an empty set) in the fixture; here: frontier nodes with
    empty rows, ``known`` a strict superset of ``adj``, and drop_self off."""
    from ocn_amd import recommend as R
    g = graph
    for kind in KINDS:
        want = ref3(g, kind)
        same(R.path_scored_candidates(g.adj, src_tensor(g.sources), kind, 3, 0.5), want, kind)
    sizes = want[0][1:] - want[0][:-1]
    for v in ISOLATED:
        assert int(sizes[g.sources.index(v)]) == 0
    two = R.two_hop_candidates(g.adj, None, src_tensor(g.sources))
    assert want[1].shape[0] > 2 * two[1].shape[0]                          # three hops reach well beyond two
    p0 = R.path_scored_candidates(g.adj, src_tensor([])[:0], "cn", 3, 0.5)
    assert p0[0].tolist() == [0] and p0[1].shape == (0, 2) and p0[2].shape == (0,)
    with pytest.raises(IndexError):
        R.three_hop_candidates(g.adj, torch.tensor([0, g.n], device=DEV))
    # known ⊋ adj: 600 candidates become known links, one source loses its whole list; the other sums stay bit for bit
    known = {v: set(r) for v, r in g.a_rows.items()}
    rng = np.random.default_rng(4)
    dropped = set()
    for i in rng.choice(want[1].shape[0], 600, replace=False).tolist():
        s, t = want[1][i].tolist()
        known[s].add(t)
        dropped.add((s, t))
    s_full = g.sources[int(sizes.argmax())]
    known[s_full] |= set(range(g.n))
    kn = csr_of(known, g.n)
    kwant = ref_path3(g.a_rows, known, g.sources, kind_weight(g.adj, "ra"), 0.5)
    got = R.path_scored_candidates(g.adj, src_tensor(g.sources), "ra", 3, 0.5, known=kn)
    same(got, kwant)
    pairs = {(int(s), int(t)) for s, t in got[1].cpu().tolist()}
    assert not (pairs & dropped) and not any(s == s_full for s, _ in pairs) and 0 < len(pairs) < want[1].shape[0] - 600
    full = {(int(s), int(t)): v for (s, t), v in zip(want[1].tolist(), bits(want[2]).tolist())}
    assert all(full[(int(s), int(t))] == v for (s, t), v in zip(got[1].cpu().tolist(), bits(got[2]).tolist()))
    same(R.three_hop_candidates(g.adj, src_tensor(g.sources), known=kn) + (None,), kwant[:2] + (None,))
    # drop_self off (ops layer), and frontier nodes whose rows are empty: the isolated nodes as the frontier of every query
    srcs = [0, 3, 187, 0]
    w = kind_weight(g.adj, "aa")
    F = flat([sorted([(m, w[m]) for m in g.a_rows[s]] + [(v, 5.0) for v in ISOLATED]) for s in srcs], srcs)
    S = flat([[(s, 1.0), (188, 2.0)] if s < 188 else [(s, 1.0)] for s in srcs], srcs)
    for drop in (False, True):
        want_d = flat([ref_expand_one(g.a_rows, g.a_rows, s, [(m, w[m]) for m in g.a_rows[s]], [(s, 1.0), (188, 2.0)] if s < 188 else [(s, 1.0)],
                                      drop_self=drop) for s in srcs], srcs)
        same(expand(g.adj, g.adj, srcs, F, S, drop_self=drop), want_d, drop)
        assert (0 in as_dict(want_d, 0)) == (not drop) and as_dict(want_d, 2) == ({188: 2.0} if drop else {187: 1.0, 188: 2.0})


# ---- 6. the evidence identity --------------------------------------------------------------------------------------------------
def test_three_hop_candidates_are_the_pairs_with_cn1_or_cn2(graph300):
    """n = 300, 16 sources: {t : cn1 count > 0 or cn2 count > 0} from the project's own intersections over all 16 x 300 pairs,
    minus known and self, is the candidate list."""
    from ocn_amd import recommend as R
    from ocn_amd.utils import adjoverlap
    g = graph300
    sources = list(range(4, 300, 20)) + [299]
    assert len(sources) == 16
    adj2 = product_adj2(g.adj)
    pairs = torch.tensor([(s, t) for s in sources for t in range(g.n)], dtype=torch.int64, device=DEV).t().contiguous()
    c1 = adjoverlap(g.adj, g.adj, pairs).counts().cpu()
    c2 = adjoverlap(g.adj, adj2, pairs).counts().cpu()
    keep = (c1 > 0) | (c2 > 0)
    want = [(s, t) for (s, t), k in zip(pairs.t().cpu().tolist(), keep.tolist()) if k and t != s and t not in g.a_rows[s]]
    only2 = int(((c1 == 0) & (c2 > 0)).sum())
    print(f"evidence: {len(want)} candidates, {only2} pairs have cn2 alone")
    assert only2 > 100
    ptr, edges = R.three_hop_candidates(g.adj, src_tensor(sources))
    assert edges.cpu().tolist() == [list(p) for p in want]
    assert ptr.cpu().tolist() == [0] + list(np.cumsum([sum(1 for s_, _ in want if s_ == s) for s in sources]))


# ---- 7. the Python layer ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 5, 128])
def test_prefilter_over_three_hops_keeps_the_m_best(graph, m):
    from ocn_amd import recommend as R
    g = graph
    src = src_tensor(g.sources)
    for kind in ("cn", "ra"):
        rptr, redges, rval = ref3(g, kind)
        sizes = rptr[1:] - rptr[:-1]
        assert int(sizes.max()) > 128
        want = ref_prefilter(rptr, redges, rval, m)
        got = R.prefilter_candidates(g.adj, src, kind, m, hops=3, decay=0.5)
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), kind
        assert int(sizes.sum()) > 20000 and int(sizes.max()) < 1000 < int(sizes.max()) * 6
        chunked = R.prefilter_candidates(g.adj, src, kind, m, hops=3, decay=0.5, budget=1000)      # ~ 40 chunks
        assert torch.equal(chunked[0], got[0]) and torch.equal(chunked[1], got[1]), kind
        alone = R.prefilter_candidates(g.adj, src, kind, m, hops=3, decay=0.5, budget=int(sizes.max()) - 1)   # a source above the budget
        assert torch.equal(alone[0], got[0]) and torch.equal(alone[1], got[1]), kind
    p0, e0 = R.prefilter_candidates(g.adj, src_tensor(list(ISOLATED)), "cn", m, hops=3, decay=0.5)
    assert p0.tolist() == [0, 0, 0, 0] and e0.shape == (0, 2)


@pytest.mark.parametrize("name", ["cn5", "cn7", "cn8", "cn6"])
def test_recommend_links_over_three_hops_is_the_composition(graph, name):
    """Candidates (all within three hops, or the 3-hop short list) -> the one scoring call -> the top k: bit for bit."""
    from ocn_amd import recommend as R
    from ocn_amd.pipeline import score_edges, score_edges_walk
    g = graph
    H, k, m, bs = 64, 7, 20, 1500
    pred = make_predictor(name, H)
    h = torch.randn(g.n, H, generator=torch.Generator().manual_seed(3)).to(DEV)
    args = SimpleNamespace(sum=0.5)
    src = src_tensor(g.sources[:60])
    adj2 = product_adj2(g.adj)
    full = R.three_hop_candidates(g.adj, src)
    short = R.prefilter_candidates(g.adj, src, "ra", m, hops=3, decay=0.5)
    assert full[1].shape[0] > 2 * bs and short[1].shape[0] < full[1].shape[0]
    for a2 in (adj2, None):
        if a2 is None and name == "cn6":
            with pytest.raises(ValueError, match="cn6 needs adj2"):
                R.recommend_links(pred, h, g.adj, None, src, k, bs, args, hops=3)
            continue
        for (ptr, edges), pf in ((full, None), (short, ("ra", m, 0.5))):
            sc = score_edges(pred, h, g.adj, a2, edges, bs, args) if a2 is not None else score_edges_walk(pred, h, g.adj, edges, bs, args)
            want_dst, want_score = ref_select(sc, ptr, edges, k)
            dst, score = R.recommend_links(pred, h, g.adj, a2, src, k, bs, args, prefilter=pf, hops=3)
            assert torch.equal(dst.cpu(), want_dst) and torch.equal(bits(score), bits(want_score)), (a2 is None, pf)
    hd, hs = R.recommend_links_heuristic(g.adj, adj2, src, k, bs, "ra", hops=3)
    hd2, hs2 = R.recommend_links_heuristic(g.adj, adj2, src, k, bs, "ra")
    assert torch.equal(hd[hs > 0], hd2[hs2 > 0])                           # a 1-hop heuristic scores the pairs beyond two hops 0


def test_frozen_scores_of_the_two_hop_pairs_do_not_move_with_hops(graph):
    """cn5 with frozen column weights: the flat score of every 2-hop pair in the hops=3 list is its score in the hops=2 list,
    within the frozen-scoring tolerance of tests/test_frozen_gpu.py (``helpers.close``: 1e-5 absolute and relative)."""
    from ocn_amd import recommend as R
    from ocn_amd.frozen import freeze_columns
    from ocn_amd.pipeline import score_edges
    g = graph
    H = 64
    pred = make_predictor("cn5", H, seed=31)
    with torch.no_grad():
        pred.alpha.copy_(torch.tensor([0.4, -0.3, 0.1]))
        pred.innerprod.fill_(0.37)
    h = torch.randn(g.n, H, generator=torch.Generator().manual_seed(10)).to(DEV)
    adj2 = product_adj2(g.adj)
    src = src_tensor(g.sources[:80])
    ref = torch.randint(0, 187, (600, 2), generator=torch.Generator().manual_seed(1)).to(DEV)
    pred.set_frozen_columns(freeze_columns(pred, g.adj, adj2, ref))
    try:
        p2, e2 = R.two_hop_candidates(g.adj, adj2, src)
        p3, e3 = R.three_hop_candidates(g.adj, src)
        s2 = score_edges(pred, h, g.adj, adj2, e2, 900)
        s3 = score_edges(pred, h, g.adj, adj2, e3, 4096)
        where = torch.full((g.n * g.n,), -1, dtype=torch.int64, device=DEV)
        where[e3[:, 0] * g.n + e3[:, 1]] = torch.arange(e3.shape[0], device=DEV)
        at = where[e2[:, 0] * g.n + e2[:, 1]]
        assert int(at.min()) >= 0 and e2.shape[0] > 2000                   # every 2-hop pair is a 3-hop candidate
        err = (s3[at] - s2).abs().max().item()
        print(f"frozen cn5: max|score in the hops=3 list - score in the hops=2 list| = {err:.3e} over {e2.shape[0]} 2-hop pairs")
        assert close(s3[at], s2)
    finally:
        pred.set_frozen_columns(None)


def test_a_three_hop_prefilter_that_covers_every_list_changes_nothing(hiplib):
    """No source has more than 128 candidates within three hops and ``m`` is at least the longest list: the retained list is
    the full list, and even a batch-coupled cn5 returns the unfiltered ``hops=3`` result bit for bit, on both routes."""
    from ocn_amd import recommend as R
    n = 120
    rng = np.random.default_rng(23)
    a_rows = sym_rows(n, [(int(x), int(y)) for x, y in zip(*np.nonzero(np.triu(rng.random((n, n)) < 0.025, 1)))])
    adj = csr_of(a_rows, n)
    src = src_tensor(torch.randperm(n, generator=torch.Generator().manual_seed(6)).tolist() + [4, 4, 9])
    ptr, edges = R.three_hop_candidates(adj, src)
    longest = int((ptr[1:] - ptr[:-1]).max())
    assert 20 < longest <= 128 and edges.shape[0] > 1500
    H, k, bs = 64, 10, 700
    pred = make_predictor("cn5", H)
    h = torch.randn(n, H, generator=torch.Generator().manual_seed(5)).to(DEV)
    for a2 in (product_adj2(adj), None):
        want_dst, want_score = R.recommend_links(pred, h, adj, a2, src, k, bs, hops=3)
        for m, kind in ((128, "cn"), (longest, "ra")):
            dst, score = R.recommend_links(pred, h, adj, a2, src, k, bs, prefilter=(kind, m, 0.5), hops=3)
            assert torch.equal(dst, want_dst) and torch.equal(bits(score), bits(want_score)), (a2 is None, m, kind)


def test_example_driver_over_three_hops(hiplib, capsys):
    """examples/run_like_reference.py --recommend 5 --recommend-hops 3 --recommend-frozen --recommend-prefilter ra:32:0.5 on the
    Cora shape: the frozen self-check passes and the kept line is printed."""
    import importlib.util
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "run_like_reference.py")
    spec = importlib.util.spec_from_file_location("run_like_reference", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(["--dataset", "cora", "--epochs", "1", "--recommend", "5", "--recommend-hops", "3", "--recommend-frozen",
              "--recommend-prefilter", "ra:32:0.5"])
    out = capsys.readouterr().out
    assert "returns the same rows = True" in out
    kept = re.search(r"^prefilter ra:32:0.5 over 3 hops kept (\d+) of the (\d+) unfiltered top-5 links \(the model ranked (\d+) of (\d+) "
                     r"candidates\)$", out, re.M)
    assert kept, out[-2000:]
    k, full, short, cands = map(int, kept.groups())
    assert 0 <= k <= full <= 25 and 0 < short <= 5 * 32 and short < cands
    assert len(re.findall(r"^recommend source \d+ top-5: ", out, re.M)) == 5
    for bad in (["--recommend-hops", "3", "--recommend-prefilter", "ra:32"], ["--recommend-prefilter", "ra:32:0.5"],
                ["--recommend-hops", "3", "--recommend-prefilter", "ra:32:-1"], ["--recommend-hops", "3", "--recommend-prefilter", "ra:32:nan"],
                ["--recommend-hops", "4"]):
        with pytest.raises(SystemExit):
            mod.main(["--dataset", "cora", "--recommend", "5"] + bad)
    capsys.readouterr()
