"""Embedding retrieval on the GPU (``ocn_mips_topm_i8``; ocn_amd/ops.py: ``mips_topm_i8``, ``quantize_rows_i8``;
ocn_amd/recommend.py: ``EmbeddingIndex``, ``embedding_candidates``, ``EmbeddingNeighbours``, ``ShortListUnion``) against the
CPU mirror of tests/mips_mirror.py.  The dot products are exact integers and a value is ONE fp32 multiply of an exactly
converted integer, so every comparison is ``torch.equal``."""
from types import SimpleNamespace

import pytest
import torch

from tests import mips_mirror as MM
from tests.helpers import make_graph, product_adj2, to_product

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SPLITS = (1, 2, 3, 16, 0)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def operands(Q, N, H, seed):
    """Asymmetric data: the query rows are uniform over [-127, 127], the key rows skewed and sparse, the scales spread over a
    factor of four — a transposed fragment, a swapped operand or a scale of the wrong row cannot pass."""
    g = gen(seed)
    query = torch.randint(-127, 128, (Q, H), generator=g, dtype=torch.int64).to(torch.int8)
    keys = torch.randint(-40, 128, (N, H), generator=g, dtype=torch.int64)
    keys = (keys * (torch.rand(N, H, generator=g) < 0.7)).to(torch.int8)
    kscale = (0.5 + 1.5 * torch.rand(N, generator=g)) / 127.0
    return query, keys, kscale


def csr(n, rows):
    """(rowptr int64 [n + 1], col int32) of {row: sorted columns}."""
    rp, col = [0], []
    for r in range(n):
        col += sorted(rows.get(r, []))
        rp.append(len(col))
    return torch.tensor(rp, dtype=torch.int64), torch.tensor(col, dtype=torch.int32)


def run(query, keys, kscale, m, rows=None, excl=None, drop_self=True, n_split=0):
    from ocn_amd import ops
    val, node = ops.mips_topm_i8(query.to(DEV), keys.to(DEV), kscale.to(DEV), m, None if rows is None else rows.to(DEV),
                                 None if excl is None else (excl[0].to(DEV), excl[1].to(DEV)), drop_self, n_split)
    assert val.dtype == torch.float32 and node.dtype == torch.int64 and val.shape == node.shape == (query.shape[0], m)
    return val.cpu(), node.cpu()


def same(got, want, what=None):
    assert torch.equal(got[1], want[1]), ("node", what)
    assert torch.equal(got[0], want[0]), ("val", what)


# ---- 1. the kernel: edges of every tile --------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 128, 256, 192])
def test_topm_equals_the_mirror_at_the_edges_of_every_tile(hiplib, H):
    """Q around the 32 queries of a wave (all inside the first 128-query tile of a workgroup; the test below goes beyond it), N
    around the 32 keys of a tile and beyond one slice, every list length around the 64 slots of a lane register, every split.
    H = 192 takes the form that keeps no fragment in registers.  The sources exclude themselves and a random row."""
    for Q in (1, 2, 31, 33, 70):
        for N in (1, 63, 64, 65, 1037, 4099):
            query, keys, kscale = operands(Q, N, H, 1000 * Q + N + H)
            g = gen(Q + N)
            rows = torch.randint(0, N, (Q,), generator=g)
            excl = csr(N, {int(s): torch.randperm(N, generator=g)[:min(N, 5)].tolist() for s in rows.tolist()})
            val = MM.values(query, keys, kscale)
            plain, masked = MM.ordered(val), MM.ordered(val, rows, excl, True)
            query, keys, kscale, rows, excl = query.to(DEV), keys.to(DEV), kscale.to(DEV), rows.to(DEV), (excl[0].to(DEV), excl[1].to(DEV))
            for m in (1, 63, 64, 65, 128):
                want_plain, want_masked = MM.cut(val, plain, m), MM.cut(val, masked, m)
                for ns in SPLITS:
                    same(run(query, keys, kscale, m, n_split=ns), want_plain, (Q, N, H, m, ns))
                    same(run(query, keys, kscale, m, rows, excl, True, ns), want_masked, (Q, N, H, m, ns, "excl"))


@pytest.mark.parametrize("H", [64, 192])
def test_topm_beyond_one_query_tile(hiplib, H):
    """A workgroup serves 128 queries: Q = 127, 128, 129 and 300 put the last query of a tile, a tile of one query and a third
    tile into the grid — the wave's first query ``tile * 128 + wave * 32``, the place of a query's partial lists in the
    workspace and the merge's stride over the queries — for both list lengths (m <= 64, m > 64), one slice, three and the
    automatic split, with and without sources and an exclusion.  A query's row must also be the row it gets alone."""
    N = 1037
    for Q in (127, 128, 129, 300):
        query, keys, kscale = operands(Q, N, H, 7000 + Q + H)
        g = gen(Q)
        rows = torch.randint(0, N, (Q,), generator=g)
        excl = csr(N, {int(s): torch.randperm(N, generator=g)[:7].tolist() for s in rows.tolist()})
        val = MM.values(query, keys, kscale)
        plain, masked = MM.ordered(val), MM.ordered(val, rows, excl, True)
        dq, dk, ds, dr, de = query.to(DEV), keys.to(DEV), kscale.to(DEV), rows.to(DEV), (excl[0].to(DEV), excl[1].to(DEV))
        for m in (64, 65):
            want_plain, want_masked = MM.cut(val, plain, m), MM.cut(val, masked, m)
            for ns in (1, 3, 0):
                same(run(dq, dk, ds, m, n_split=ns), want_plain, (Q, H, m, ns))
                same(run(dq, dk, ds, m, dr, de, True, ns), want_masked, (Q, H, m, ns, "excl"))
            last = run(dq[Q - 1:], dk, ds, m, dr[Q - 1:], de, True, 3)       # the last query on its own: the same row
            assert torch.equal(last[1][0], want_masked[1][Q - 1]) and torch.equal(last[0][0], want_masked[0][Q - 1])


def test_exact_at_the_width_bound(hiplib):
    """H = 1024 and every operand +-127: |dot| reaches 1024 * 127^2 = 16 516 096 < 2^24; scales that are powers of two keep the
    product exact as well."""
    Q, N, H = 5, 70, 1024
    g = gen(7)
    sign = lambda *shape: (torch.randint(0, 2, shape, generator=g) * 2 - 1)      # noqa: E731
    query, keys = sign(Q, H) * 127, sign(N, H) * 127
    keys[0] = query[0]                   # + the bound
    keys[1] = -query[0]                  # - the bound
    keys[2] = query[1]
    keys[2, :512] *= -1                  # exactly 0
    kscale = 2.0 ** torch.randint(-6, 3, (N,), generator=g).float()
    kscale[0] = kscale[1] = 1.0
    query, keys = query.to(torch.int8), keys.to(torch.int8)
    val = MM.values(query, keys, kscale)
    assert float(val[0, 0]) == 16516096.0 and float(val[0, 1]) == -16516096.0 and float(val[1, 2]) == 0.0
    for m in (3, 70):
        want = MM.topm(query, keys, kscale, m)
        for ns in (1, 2, 0):
            got = run(query, keys, kscale, m, n_split=ns)
            same(got, want, (m, ns))
        assert int(want[1][0, 0]) == 0 and float(want[0][0, 0]) == 16516096.0
    assert int(want[1][0, -1]) == 1                          # (the list of all 70: the negative bound comes last)


# ---- 2. order ------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_id_across_slices(hiplib):
    """Groups of identical key rows with one scale, spread over the whole range: with n_split = 3 the 32-key tiles of N = 200
    fall into slices of 96, 96 and 8 keys, and the members of a group lie on both sides of the boundaries."""
    Q, N, H = 3, 200, 64
    query, keys, kscale = operands(Q, 8, H, 3)
    idx = torch.arange(N) % 8
    keys, kscale = keys[idx].contiguous(), kscale[idx].contiguous()
    val = MM.values(query, keys, kscale)
    assert len(set(val[0].tolist())) <= 8
    for m in (5, 30, 128):
        want = MM.topm(query, keys, kscale, m)
        for q in range(Q):                                   # the winners of a tie are the lowest ids of their group
            best = int(want[1][q, 0])
            k = min(m, N // 8)
            assert want[1][q, :k].tolist() == list(range(best % 8, N, 8))[:k]
        for ns in SPLITS:
            same(run(query, keys, kscale, m, n_split=ns), want, (m, ns))


def test_all_zero_keys_keep_the_first_ids(hiplib):
    Q, N, H, m = 4, 300, 64, 17
    query, _, kscale = operands(Q, N, H, 5)
    keys = torch.zeros(N, H, dtype=torch.int8)
    kscale[::2] *= -1                                        # -0.0 and +0.0 are one value
    for ns in SPLITS:
        val, node = run(query, keys, kscale, m, n_split=ns)
        assert node.tolist() == [list(range(m))] * Q and bool((val == 0).all())
    rows = torch.tensor([0, 5, 16, 299])
    val, node = run(query, keys, kscale, m, rows, None, True)
    assert node[0].tolist() == list(range(1, m + 1)) and node[1].tolist() == [i for i in range(m + 1) if i != 5]
    assert node[2].tolist() == list(range(16)) + [17] and node[3].tolist() == list(range(m))


def test_scales_invert_the_order_and_negative_dots(hiplib):
    """Raw dots ascend with the node id; the scales descend faster, so the order by value is the reverse of the order by dot.
    Then all-negative dots: the best is the one nearest zero, and a negative scale turns the order once more."""
    N, H = 96, 64
    query = torch.zeros(2, H, dtype=torch.int8)
    query[0, 0], query[1, 0] = 1, -1
    keys = torch.zeros(N, H, dtype=torch.int8)
    keys[:, 0] = torch.arange(1, N + 1).to(torch.int8)       # dot[0][n] = n + 1, dot[1][n] = -(n + 1)
    kscale = 1.0 / (torch.arange(1, N + 1).float() ** 2)     # val[0][n] = 1 / (n + 1)
    want = MM.topm(query, keys, kscale, 10)
    assert want[1][0].tolist() == list(range(10)) and want[1][1].tolist() == list(range(N - 1, N - 11, -1))
    for ns in (1, 2, 3):
        same(run(query, keys, kscale, 10, n_split=ns), want, ns)
    want = MM.topm(query, keys, -kscale, 96)
    assert want[1][1].tolist() == list(range(N)) and float(want[0][0, 0]) < 0
    for ns in (1, 2, 3):
        same(run(query, keys, -kscale, 96, n_split=ns), want, ns)


# ---- 3. eligibility ------------------------------------------------------------------------------------------------------
def test_eligibility(hiplib):
    Q, N, H, m = 6, 500, 128, 20
    query, keys, kscale = operands(Q, N, H, 11)
    val = MM.values(query, keys, kscale)
    free = MM.ordered(val)
    rows = torch.tensor([int(free[0][0]), 7, 8, 9, 7, 499])  # query 0 is its own best; 7 repeats
    f1, f2 = [n for n in free[1].tolist() if n != 7], [n for n in free[2].tolist() if n != 8]
    # 7: the unexcluded best, second and m-th are known; 8: a hub row that leaves m - 3 nodes; 9: everything is known
    known = {7: [f1[i] for i in (0, 1, m - 1)],
             8: sorted(set(range(N)) - set(f2[40:40 + m - 3])),
             9: list(range(N))}
    excl = csr(N, known)
    for drop in (True, False):
        want = MM.topm(query, keys, kscale, m, rows, excl, drop)
        assert (int(want[1][0, 0]) == int(rows[0])) == (not drop)
        assert not set(want[1][1].tolist()) & set(known[7]) and (not drop or int(want[1][1, 0]) == f1[2])
        assert want[1][2, m - 3:].tolist() == [-1] * 3 and want[1][2, :m - 3].tolist() == f2[40:40 + m - 3]
        assert want[1][3].tolist() == [-1] * m and want[0][3].tolist() == [float("-inf")] * m
        for ns in SPLITS:
            got = run(query, keys, kscale, m, rows, excl, drop, ns)
            same(got, want, (drop, ns))
    # a repeated source, given the same query, repeats its row of the output
    q2 = query.clone()
    q2[4] = q2[1]
    got = run(q2, keys, kscale, m, rows, excl, True)
    assert torch.equal(got[1][4], got[1][1]) and torch.equal(got[0][4], got[0][1])
    # rows without an exclusion: only the source itself goes
    same(run(query, keys, kscale, m, rows, None, True), MM.topm(query, keys, kscale, m, rows, None, True))
    same(run(query, keys, kscale, m, rows, None, False), MM.cut(val, free, m))


def test_no_query(hiplib):
    _, keys, kscale = operands(1, 40, 64, 2)
    val, node = run(torch.zeros(0, 64, dtype=torch.int8), keys, kscale, 5)
    assert val.shape == (0, 5) and node.shape == (0, 5)
    val, node = run(torch.zeros(0, 64, dtype=torch.int8), keys, kscale, 5, torch.zeros(0, dtype=torch.int64), csr(40, {}), True)
    assert val.shape == (0, 5) and node.shape == (0, 5)


# ---- 4. the Python layer -------------------------------------------------------------------------------------------------
def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def src_tensor(sources):
    return torch.tensor(list(sources), dtype=torch.int64, device=DEV)


def mirror_candidates(index, queries, sources, m, known, normalize=False):
    """(ptr, edges, val) of ``embedding_candidates`` from the mirror; the int8 operands are the device's (the quantiser has its
    own test on the CPU), everything after them is the mirror's."""
    from ocn_amd import ops
    qq, _ = ops.quantize_rows_i8(queries, normalize)
    excl = None if known is None else (known._rowptr.cpu(), known._col.cpu())
    rows = sources.cpu()
    val = MM.values(qq.cpu(), index.keys_q.cpu(), index.kscale.cpu())
    ptr, pairs, vals = [0], [], []
    for q, o in enumerate(MM.ordered(val, rows, excl, True)):
        keep = sorted(o[:m].tolist())
        pairs += [[int(rows[q]), t] for t in keep]
        vals += [val[q, t] for t in keep]
        ptr.append(len(pairs))
    return (torch.tensor(ptr, dtype=torch.int64), torch.tensor(pairs, dtype=torch.int64).reshape(-1, 2),
            torch.stack(vals) if vals else torch.zeros(0))


@pytest.fixture(scope="module")
def world(hiplib):
    """About 300 nodes under a power law, the last three without an edge; sources: the hub, light nodes, an isolated one, a
    repeat.  ``known`` = adj; ``wide``: adj with a row for node 5 that leaves it 20 eligible nodes (a short segment)."""
    from ocn_amd.sparse import SparseTensor
    adj = to_product(make_graph(300, 8, 60, seed=11, isolated=3), DEV)
    n = adj.size(0)
    deg = (adj._rowptr[1:] - adj._rowptr[:-1]).cpu()
    hub = int(deg.argmax())
    assert int(deg[hub]) >= 30 and int(deg[299]) == 0
    sources = [hub, 5, 17, 299, 120, 5, 250, 33, 298]
    row, col = adj.storage.row().long(), adj.storage.col().long()
    own = set(adj._col[int(adj._rowptr[5]):int(adj._rowptr[6])].tolist())
    extra = [t for t in range(n) if t not in own and t != 5][:n - 1 - len(own) - 20]
    ei = torch.stack([torch.cat([row, torch.full((len(extra),), 5, device=DEV)]), torch.cat([col, torch.tensor(extra, device=DEV)])])
    wide = SparseTensor.from_edge_index(ei, sparse_sizes=(n, n))
    return SimpleNamespace(adj=adj, n=n, hub=hub, sources=sources, src=src_tensor(sources), wide=wide)


@pytest.mark.parametrize("H", [16, 32, 48, 64])
@pytest.mark.parametrize("normalize", [False, True])
def test_embedding_candidates_equal_the_mirror(world, H, normalize):
    """Widths below the alignment go through the zero padding; ascending ids per source; ``ptr`` with a short segment."""
    from ocn_amd import ops, recommend as R
    w = world
    h = (torch.randn(w.n, H, generator=gen(H)) * torch.logspace(-1, 1, w.n)[:, None]).to(DEV)
    index = R.EmbeddingIndex(h, normalize)
    assert index.keys_q.shape == (w.n, 64) and index.kscale.shape == (w.n,) and not bool(index.keys_q[:, H:].any())
    if normalize:                                            # = quantising the normalised matrix
        unit = h / torch.linalg.vector_norm(h, dim=1, keepdim=True)
        q2, s2 = ops.quantize_rows_i8(unit)
        assert torch.equal(index.keys_q, q2) and torch.equal(index.kscale, s2)
    for m, known in ((7, None), (40, w.adj), (128, w.wide)):
        ptr, edges, val = R.embedding_candidates(index, h[w.src], w.src, m, known)
        want = mirror_candidates(index, h[w.src], w.src, m, known, normalize)
        assert ptr.dtype == torch.int64 and edges.dtype == torch.int64 and val.dtype == torch.float32
        assert torch.equal(ptr.cpu(), want[0]) and torch.equal(edges.cpu(), want[1]) and torch.equal(val.cpu(), want[2]), (m, H)
        sizes = (ptr[1:] - ptr[:-1]).tolist()
        assert sizes == [min(m, 20) if (known is w.wide and s == 5) else m for s in w.sources]
        for q in range(len(w.sources)):
            seg = edges[int(ptr[q]):int(ptr[q + 1]), 1].tolist()
            assert seg == sorted(set(seg)) and w.sources[q] not in seg
    p0, e0, v0 = R.embedding_candidates(index, h[:0], src_tensor([]), 5)
    assert p0.tolist() == [0] and e0.shape == (0, 2) and v0.shape == (0,)


def test_index_survives_torch_save(world, tmp_path):
    from ocn_amd import recommend as R
    index = R.EmbeddingIndex(torch.randn(world.n, 32, generator=gen(1)).to(DEV), True)
    torch.save(index, tmp_path / "index.pt")
    back = torch.load(tmp_path / "index.pt", weights_only=False)
    assert (back.n, back.width, back.normalize) == (index.n, 32, True)
    assert torch.equal(back.keys_q, index.keys_q) and torch.equal(back.kscale, index.kscale)


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------
def make_predictor(name, H, seed=12):
    from ocn_amd.model import predictor_dict
    torch.manual_seed(seed)
    return predictor_dict[name](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()


@pytest.fixture(scope="module")
def served(world):
    """cn5 with frozen column weights and cn7, H = 16, with the embeddings they score."""
    from ocn_amd.frozen import freeze_columns
    H = 16
    h = torch.randn(world.n, H, generator=gen(3)).to(DEV)
    adj2 = product_adj2(world.adj)
    cn5 = make_predictor("cn5", H, seed=31)
    with torch.no_grad():
        cn5.alpha.copy_(torch.tensor([0.4, -0.3, 0.1]))
        cn5.innerprod.fill_(0.37)
    ref = torch.randint(0, world.n, (600, 2), generator=gen(1)).to(DEV)
    cn5.set_frozen_columns(freeze_columns(cn5, world.adj, adj2, ref))
    return SimpleNamespace(h=h, adj2=adj2, preds={"cn5": cn5, "cn7": make_predictor("cn7", H)}, args=SimpleNamespace(sum=0.5))


@pytest.mark.parametrize("name", ["cn5", "cn7"])
def test_recommend_links_with_embedding_neighbours_is_the_composition(world, served, name):
    """The contract sentence: the scores are exactly those the scoring loop returns for the flat retained list at this
    batch size — through A² and on the walk route.  The isolated sources get k finite-scored targets here and nothing from the
    graph-local stages."""
    from ocn_amd import recommend as R
    from ocn_amd.pipeline import score_edges, score_edges_walk
    w, s = world, served
    pred, k, m, bs = s.preds[name], 4, 9, 30
    stage = R.EmbeddingNeighbours(m)
    sptr, sedges, _ = R.embedding_candidates(R.EmbeddingIndex(s.h), s.h[w.src], w.src, m, w.adj)
    assert sedges.shape[0] == m * len(w.sources) > 2 * bs
    cold = [q for q, v in enumerate(w.sources) if v >= 297]
    for a2 in ((s.adj2,) if name == "cn5" else (s.adj2, None)):          # (the frozen table was made on the pattern route)
        flat = score_edges(pred, s.h, w.adj, a2, sedges, bs, s.args) if a2 is not None else \
            score_edges_walk(pred, s.h, w.adj, sedges, bs, s.args)
        want_dst, want_score = R._select(flat, sptr, sedges, k)
        dst, score = R.recommend_links(pred, s.h, w.adj, a2, w.src, k, bs, s.args, prefilter=stage)
        assert torch.equal(dst, want_dst) and torch.equal(bits(score), bits(want_score)), a2 is None
        assert bool((dst[cold] >= 0).all()) and bool(torch.isfinite(score[cold]).all())
        again = R.recommend_links(pred, s.h, w.adj, a2, w.src, k, bs, s.args, prefilter=R.EmbeddingNeighbours(m, keys=R.EmbeddingIndex(s.h)))
        assert torch.equal(again[0], dst) and torch.equal(bits(again[1]), bits(score))
        for local in (("ra", m), R.RandomWalks(m, 256, 2)):
            d2, s2 = R.recommend_links(pred, s.h, w.adj, a2, w.src, k, bs, s.args, prefilter=local)
            assert bool((d2[cold] == -1).all()) and bool(torch.isinf(s2[cold]).all())


def test_short_list_union_is_the_sorted_union_of_its_stages(world, served):
    from ocn_amd import recommend as R
    from ocn_amd.pipeline import score_edges
    w, s = world, served
    union = R.ShortListUnion(("ra", 32), R.EmbeddingNeighbours(32))
    pa, ea = R.prefilter_candidates(w.adj, w.src, "ra", 32)
    pb, eb, _ = R.embedding_candidates(R.EmbeddingIndex(s.h), s.h[w.src], w.src, 32, w.adj)
    ptr, edges, rank = R._candidates(w.adj, s.adj2, w.src, None, 2, R._check_prefilter(union, 32), None, s.h)
    assert rank is None and ptr.dtype == torch.int64 and edges.dtype == torch.int64
    at, both = 0, 0
    for q, v in enumerate(w.sources):
        a = set(ea[int(pa[q]):int(pa[q + 1]), 1].tolist())
        b = set(eb[int(pb[q]):int(pb[q + 1]), 1].tolist())
        want = sorted(a | b)
        both += len(a & b)
        assert int(ptr[q]) == at and edges[at:at + len(want)].tolist() == [[v, t] for t in want], q
        at += len(want)
    assert int(ptr[-1]) == at == edges.shape[0] and both > 0 and at > 32 * len(w.sources)
    pred, k, bs = s.preds["cn7"], 32, 50
    want_dst, want_score = R._select(score_edges(pred, s.h, w.adj, s.adj2, edges, bs, s.args), ptr, edges, k)
    dst, score = R.recommend_links(pred, s.h, w.adj, s.adj2, w.src, k, bs, s.args, prefilter=union)
    assert torch.equal(dst, want_dst) and torch.equal(bits(score), bits(want_score))
    three = R.ShortListUnion(("ra", 8, 0.5), R.RandomWalks(8, 128, 3, 0.5), R.EmbeddingNeighbours(8))       # every kind of stage
    dst3, _ = R.recommend_links(pred, s.h, w.adj, s.adj2, w.src, 8, bs, s.args, prefilter=three, hops=3)
    assert bool((dst3[:, 0] >= 0).all())


def test_a_list_that_holds_every_candidate_changes_nothing(hiplib):
    """60 nodes at a density that puts every non-neighbour within two hops: the eligible nodes of a source ARE its 2-hop
    candidates and there are at most m of them, so the embedding short list is the unfiltered list and frozen cn5 returns the
    unfiltered result (the frozen scoring tolerance of tests/test_frozen_gpu.py)."""
    import numpy as np
    from ocn_amd import recommend as R
    from ocn_amd.frozen import freeze_columns
    from ocn_amd.sparse import SparseTensor
    n, H, k, bs = 60, 16, 5, 200
    up = np.triu(np.random.default_rng(4).random((n, n)) < 0.5, 1)
    r, c = np.nonzero(up | up.T)
    adj = SparseTensor.from_edge_index(torch.from_numpy(np.stack([r, c]).astype(np.int64)).to(DEV), sparse_sizes=(n, n))
    adj2 = product_adj2(adj)
    src = src_tensor(range(n))
    h = torch.randn(n, H, generator=gen(8)).to(DEV)
    ptr, edges = R.two_hop_candidates(adj, adj2, src)
    p2, e2, _ = R.embedding_candidates(R.EmbeddingIndex(h), h[src], src, 128, adj)
    assert torch.equal(ptr, p2) and torch.equal(edges, e2) and int((ptr[1:] - ptr[:-1]).max()) <= 128
    pred = make_predictor("cn5", H, seed=31)
    pred.set_frozen_columns(freeze_columns(pred, adj, adj2, torch.randint(0, n, (300, 2), generator=gen(1)).to(DEV)))
    want_dst, want_score = R.recommend_links(pred, h, adj, adj2, src, k, bs)
    dst, score = R.recommend_links(pred, h, adj, adj2, src, k, bs, prefilter=R.EmbeddingNeighbours(128))
    assert torch.equal(dst, want_dst) and torch.allclose(score, want_score, atol=1e-5, rtol=1e-5)


def test_rank_links_with_the_embedding_stage(world, served):
    """``retrieval_rank`` = the mirror's ranks among all eligible nodes; the model ranks exactly the targets the short list
    kept; a target of rank r <= k is where ``recommend_links`` lists it.  A union reports membership only."""
    from ocn_amd import ops, recommend as R
    from ocn_amd.ranking import rank_links, ranking_metrics
    w, s = world, served
    pred, k, m, bs = s.preds["cn7"], 4, 9, 30
    index = R.EmbeddingIndex(s.h)
    qq = ops.quantize_rows_i8(s.h[w.src])[0].cpu()
    excl = (w.adj._rowptr.cpu(), w.adj._col.cpu())
    val = MM.values(qq, index.keys_q.cpu(), index.kscale.cpu())
    lists = MM.ordered(val, w.src.cpu(), excl, True)
    tptr, tnode = [0], []
    for q, v in enumerate(w.sources):                        # the best, the m-th, one past the cut, the last, itself, a neighbour
        o = lists[q].tolist()
        tnode += [o[0], o[m - 1], o[m], o[-1], v] + excl[1][int(excl[0][v]):int(excl[0][v + 1])].tolist()[:1]
        tptr.append(len(tnode))
    truth = (torch.tensor(tptr, dtype=torch.int64, device=DEV), torch.tensor(tnode, dtype=torch.int64, device=DEV))
    want_rr = MM.ranks(qq, index.keys_q.cpu(), index.kscale.cpu(), w.src.cpu(), excl, True, *truth)
    assert int(want_rr.max()) > 250 and int(want_rr.min()) == 0
    stage = R.EmbeddingNeighbours(m)
    res = rank_links(pred, s.h, w.adj, s.adj2, w.src, truth, bs, s.args, prefilter=stage)
    assert res.m == m and torch.equal(res.retrieval_rank.cpu(), want_rr)
    assert torch.equal(res.rank > 0, (res.retrieval_rank >= 1) & (res.retrieval_rank <= m))
    assert res.n_cand.tolist() == [m] * len(w.sources)
    dst, _ = R.recommend_links(pred, s.h, w.adj, s.adj2, w.src, k, bs, s.args, prefilter=stage)
    hit = res.rank.cpu().tolist()
    for q in range(len(w.sources)):
        for j in range(tptr[q], tptr[q + 1]):
            listed = [i + 1 for i, t in enumerate(dst[q].tolist()) if t == tnode[j]]
            assert listed == ([hit[j]] if 1 <= hit[j] <= k else []), (q, j)
    met = ranking_metrics(res, ks=(1, 5))
    eligible = int((want_rr > 0).sum())
    assert met["coverage"] == eligible / len(tnode) and met["m"] == m
    assert met["retention"] == int(((want_rr >= 1) & (want_rr <= m)).sum()) / eligible
    # chunks of the restatement: one query at a time gives the same ranks
    small = R.embedding_retrieval_rank(index, s.h[w.src], w.src, w.adj, *truth, chunk_elems=w.n)
    assert torch.equal(small.cpu(), want_rr)
    union = R.ShortListUnion(("ra", m), stage)
    ures = rank_links(pred, s.h, w.adj, s.adj2, w.src, truth, bs, s.args, prefilter=union)
    assert ures.retrieval_rank is None and ures.m is None
    uptr, uedges, _ = R._candidates(w.adj, s.adj2, w.src, None, 2, R._check_prefilter(union, 1), None, s.h)
    member = [tnode[j] in uedges[int(uptr[q]):int(uptr[q + 1]), 1].tolist() for q in range(len(w.sources)) for j in range(tptr[q], tptr[q + 1])]
    assert (ures.rank > 0).cpu().tolist() == member
    umet = ranking_metrics(ures, ks=(1,))
    assert umet["coverage"] == sum(member) / len(member) and "retention" not in umet


# ---- 6. the example driver -------------------------------------------------------------------------------------------------
def test_example_driver_with_an_embedding_short_list(hiplib, capsys):
    """examples/run_like_reference.py --recommend 5 --recommend-emb 8 --recommend-eval 50 on the Cora shape, then the union with
    an "ra" short list: the evaluation lines of the stage (with its retention) and of the union (coverage alone) are printed
    beside the unfiltered one; the combinations that make no request are refused."""
    import importlib.util
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "run_like_reference.py")
    spec = importlib.util.spec_from_file_location("run_like_reference", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ["--dataset", "cora", "--epochs", "1", "--recommend", "5"]
    mod.main(base + ["--recommend-emb", "8", "--recommend-eval", "50"])
    out = capsys.readouterr().out
    assert len(re.findall(r"^recommend source \d+ top-5: ", out, re.M)) == 5
    assert re.search(r"^recommend-eval cn5 over 2 hops prefilter embedding 8: \d+ sources, \d+ pairs, coverage (\d\.\d{4}) retention "
                     r"(\d\.\d{4}) ", out, re.M), out[-2000:]
    assert re.search(r"^recommend-eval cn5 over 2 hops unfiltered: ", out, re.M)
    mod.main(base + ["--recommend-prefilter", "ra:8", "--recommend-emb", "8:cos", "--recommend-union", "--recommend-eval", "50"])
    out = capsys.readouterr().out
    ev = re.search(r"^recommend-eval cn5 over 2 hops prefilter union of ra:8 \+ embedding 8:cos: \d+ sources, \d+ pairs, coverage "
                   r"(\d\.\d{4}) mrr ", out, re.M)
    assert ev, out[-2000:]
    for bad in (["--recommend-emb", "8", "--recommend-prefilter", "ra:8"], ["--recommend-union", "--recommend-emb", "8"],
                ["--recommend-union", "--recommend-prefilter", "ra:8"], ["--recommend-emb", "4"], ["--recommend-emb", "8:sin"],
                ["--recommend-emb", "x"], ["--recommend-emb", "0"], ["--heuristic", "ra", "--recommend-emb", "8"]):
        with pytest.raises(SystemExit):
            mod.main(base + bad)
    capsys.readouterr()
