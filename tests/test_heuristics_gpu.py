"""Link heuristics (ocn_amd/heuristics.py on ``ocn_cn_node_sums``) on the GPU against a restatement from the oracle's
``adjoverlap``: the explicit (row, col) pattern of adjoverlap(oadj, oadj | oadj2, e), each candidate's sum formed by a
sequential fp32 loop over its columns in ascending order on the CPU.  Every operation has a defined order and rounding, so
every comparison is ``torch.equal``."""
import os
from types import SimpleNamespace

import pytest
import torch

from oracle import ocn_oracle as O
from ocn_amd.synth import chung_lu_graph, sample_edges
from tests.helpers import make_graph, product_adj2, to_product

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("cn", "aa", "ra", "jaccard", "pa", "cn2", "aa2", "ra2")
GROUP = 16                       # candidates per workgroup of cn_node_sums_kernel


# ---- the restatement ---------------------------------------------------------------------------------------------------
def rowcount(m):
    return torch.bincount(m.row, minlength=m.n_rows)


def ref_table(oadj, user=None):
    """{1 / log deg, 1 / deg, user0, user1} per node in fp32 on the CPU (deg = the stored row length)."""
    deg = rowcount(oadj)
    degf = deg.to(torch.float32)
    t = torch.zeros(oadj.n_rows, 4, dtype=torch.float32)
    t[:, 0] = torch.where(deg >= 2, 1.0 / torch.log(degf), torch.zeros(()))
    t[:, 1] = torch.where(deg >= 1, 1.0 / degf, torch.zeros(()))
    if user is not None:
        t[:, 2:2 + user.reshape(oadj.n_rows, -1).shape[1]] = user.reshape(oadj.n_rows, -1)
    return t


def seq_sums(cn, w):
    """out[e] = w[c_0] + w[c_1] + ... over the columns of row e of ``cn`` in ascending order, one fp32 add each, from 0:
    step r adds the r-th entry of every row that has one (sequential per candidate, vectorised over the candidates)."""
    cnt = rowcount(cn)
    start = torch.cumsum(cnt, 0) - cnt
    assert bool((cn.col[1:] > cn.col[:-1])[cn.row[1:] == cn.row[:-1]].all())      # ascending inside every row
    out = torch.zeros(cn.n_rows, w.shape[1], dtype=torch.float32)
    for r in range(int(cnt.max()) if cnt.numel() else 0):
        rows = (cnt > r).nonzero().reshape(-1)
        out[rows] = out[rows] + w[cn.col[start[rows] + r]]
    return out


def restate(oadj, oadj2, e, user=None):
    """All eight kinds [B, 8] (the order of KINDS), the two counts and the user-column sums."""
    cn1, cn2 = O.adjoverlap(oadj, oadj, e), O.adjoverlap(oadj, oadj2, e)
    w = ref_table(oadj, user)
    s1, s2 = seq_sums(cn1, w), seq_sums(cn2, w)
    c1, c2 = rowcount(cn1), rowcount(cn2)
    deg = rowcount(oadj)
    di, dj = deg[e[0]], deg[e[1]]
    union = di + dj - c1
    jac = torch.where(union > 0, c1.to(torch.float32) / union.clamp(min=1).to(torch.float32), torch.zeros(()))
    pa = di.to(torch.float32) * dj.to(torch.float32)
    scores = torch.stack([c1.to(torch.float32), s1[:, 0], s1[:, 1], jac, pa, c2.to(torch.float32), s2[:, 0], s2[:, 1]], dim=1)
    return SimpleNamespace(scores=scores, c1=c1, c2=c2, s1=s1, s2=s2)


def assert_not_empty(r, B, every_class=False):
    """From the restatement's counts: no test here passes on empty sets.  At least a quarter of the candidates have 1-hop
    members, at least half have 2-hop members, at least one has neither; ``every_class`` (the hub graph, whose bare path gives
    a candidate with a 1-hop member and no 2-hop one): all four combinations occur."""
    assert int((r.c1 > 0).sum()) * 4 >= B and int((r.c2 > 0).sum()) * 2 >= B and bool(((r.c1 == 0) & (r.c2 == 0)).any())
    if every_class:
        for has1 in (False, True):
            for has2 in (False, True):
                assert bool((((r.c1 > 0) == has1) & ((r.c2 > 0) == has2)).any()), (has1, has2)


# ---- graphs ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hubs(hiplib):
    """The ``hubs`` graph of tests/test_cn8_gpu.py, rebuilt: a Chung-Lu graph with cliques plus a hub with 1 400 neighbours (as
    source and as target), a bare path a - b - c, isolated nodes, i == j and duplicate candidates."""
    n, core, B = 3000, 2980, 1500
    g = torch.Generator().manual_seed(11)
    ei = chung_lu_graph(core, avg_deg=12, max_deg=300, seed=5, clique_frac=0.5)
    hub = 7
    spokes = torch.randperm(core, generator=g)[:1400]
    spokes = spokes[spokes != hub]
    a, b, c = core, core + 1, core + 2                                  # ids core + 3 .. n - 1 stay isolated
    extra = torch.tensor([[a, b], [b, c]])
    ei = torch.cat([ei, torch.stack([torch.full_like(spokes, hub), spokes]), extra], dim=1)
    oadj = O.to_symmetric(O.from_edge_index(ei, n))
    oadj2 = O.adj2_sparse(oadj)
    e = sample_edges(oadj.row, oadj.col, n, B - 40, seed=13, pos_frac=0.6)
    other = torch.randint(0, core, (16,), generator=g)
    special = torch.cat([torch.stack([torch.full_like(other, hub), other]), torch.stack([other, torch.full_like(other, hub)]),
                         torch.tensor([[a, c, a, n - 1, n - 2, hub, b, 3], [c, a, b, 5, n - 1, n - 1, b, 3]])], dim=1)
    e = torch.cat([e, special], dim=1)
    e = e[:, torch.randperm(e.shape[1], generator=g)].contiguous()
    adj = to_product(oadj, DEV)
    deg = rowcount(oadj)
    assert int(deg[hub]) > 1024 and int((deg == 0).sum()) >= 10 and int((e[0] == hub).sum()) >= 16 and int((e[1] == hub).sum()) >= 16
    assert e.shape[1] % GROUP != 0                                      # the last workgroup is not full
    return SimpleNamespace(n=n, B=e.shape[1], oadj=oadj, oadj2=oadj2, e=e, adj=adj, adj2=product_adj2(adj), hub=hub, path=(a, b, c))


@pytest.fixture(scope="module")
def mid(hiplib):
    """A mid-size Chung-Lu graph (rows up to 400 entries, isolated nodes) with a batch large enough for a processing order."""
    from ocn_amd import ops
    n, B = 3000, 4500
    oadj = make_graph(n, 12, 400, 2, isolated=20)
    oadj2 = O.adj2_sparse(oadj)
    e = sample_edges(oadj.row, oadj.col, n, B, seed=52)
    adj = to_product(oadj, DEV)
    assert B >= ops.sort_edges_min_batch and B % GROUP != 0
    return SimpleNamespace(n=n, B=B, oadj=oadj, oadj2=oadj2, e=e, adj=adj, adj2=product_adj2(adj))


def bipartite(m, n_right, extra=0):
    """K_{m, n_right} (left ids first) plus ``extra`` isolated nodes, on the device, with its A²."""
    from ocn_amd.sparse import SparseTensor
    n = m + n_right + extra
    left, right = torch.arange(m), torch.arange(m, m + n_right)
    ei = torch.stack([left.repeat_interleave(n_right), right.repeat(m)])
    ei = torch.cat([ei, ei.flip(0)], dim=1)
    adj = SparseTensor.from_edge_index(ei.to(DEV), sparse_sizes=(n, n))
    return adj, product_adj2(adj)


def chain(vals):
    """The fp32 sequential sum of ``vals`` from 0."""
    acc = torch.zeros((), dtype=torch.float32)
    for v in vals:
        acc = acc + v
    return float(acc)


# ---- the kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [False, True], ids=["batch_order", "permuted"])
@pytest.mark.parametrize("form2", ["csr2", "bits2"])
@pytest.mark.parametrize("form1", ["csr1", "bits1", "both1"])
def test_cn_node_sums_every_membership_form(hubs, form1, form2, order):
    """``ops.cn_node_sums``: all four weight columns of both sums, the counts and the degrees, T1 and T2 as CSR and as bit rows,
    with and without a processing order, on a batch that is not a multiple of the candidates per workgroup; the counts also
    against the ones ``ocn_cn_flags`` produces for the same batch."""
    from ocn_amd import ops
    c = hubs
    user = torch.randn(c.n, 2, generator=torch.Generator().manual_seed(4))
    r = restate(c.oadj, c.oadj2, c.e, user)
    assert_not_empty(r, c.B, every_class=True)
    adj, adj2 = c.adj, c.adj2
    bm1 = ops.bitrows_from_csr(adj._rowptr, adj._col, c.n) if form1 != "csr1" else None
    bm2 = ops.bitrows_from_csr(adj2._rowptr, adj2._col, c.n) if form2 == "bits2" else None
    t1 = (adj._rowptr, adj._col) if form1 != "bits1" else None
    t2 = (adj2._rowptr, adj2._col) if form2 == "csr2" else None
    ed = c.e.to(DEV)
    src, dst = ed[0].contiguous(), ed[1].contiguous()
    perm = torch.randperm(c.B, generator=torch.Generator().manual_seed(3)).to(DEV) if order else None
    s1, s2, n1, n2, deg = ops.cn_node_sums(adj._rowptr, adj._col, t1, t2, src, dst, ref_table(c.oadj, user).to(DEV),
                                           t1_bitmap=bm1, t2_bitmap=bm2, order=perm)
    assert n1.dtype == torch.int32 and torch.equal(n1.cpu().long(), r.c1) and torch.equal(n2.cpu().long(), r.c2)
    assert s1.shape == (c.B, 4) and torch.equal(s1.cpu(), r.s1) and torch.equal(s2.cpu(), r.s2)
    if form1 == "bits1":
        assert deg is None
    else:
        d = rowcount(c.oadj)
        assert torch.equal(deg.cpu(), torch.stack([d[c.e[0]], d[c.e[1]]], dim=1).to(torch.float32))
    _, _, _, _, _, f1, f2, status, _ = ops.cn_flags(adj._rowptr, adj._col, (adj._rowptr, adj._col), (adj2._rowptr, adj2._col),
                                                     src, dst, c.n, adj.max_rowcount())
    assert torch.equal(f1, n1) and torch.equal(f2, n2) and status[0].item() == 0 and status[3].item() == 0
    # without a 2-hop matrix: the same 1-hop outputs, zero 2-hop outputs
    s1b, s2b, n1b, n2b, _ = ops.cn_node_sums(adj._rowptr, adj._col, t1, None, src, dst, ref_table(c.oadj, user).to(DEV),
                                             t1_bitmap=bm1, order=perm)
    assert torch.equal(s1b, s1) and torch.equal(n1b, n1) and not bool(s2b.any()) and not bool(n2b.any())


@pytest.mark.parametrize("graph", ["hubs", "mid"])
@pytest.mark.parametrize("form", ["bit_rows", "csr"])
def test_all_eight_kinds_against_the_restatement(request, monkeypatch, graph, form):
    """``link_heuristics`` on the hub graph and on a mid-size Chung-Lu graph (a batch with a processing order): every kind
    ``torch.equal`` to the restatement, with the adjacencies' bit rows and with CSR alone; subsets and orders of kinds pick
    the same columns; the node table is the CPU expression bit for bit and is cached on the adjacency."""
    from ocn_amd import heuristics as Hx, ops
    from ocn_amd.sparse import SparseTensor
    c = request.getfixturevalue(graph)
    r = restate(c.oadj, c.oadj2, c.e)
    assert_not_empty(r, c.B, every_class=(graph == "hubs"))
    adj, adj2 = c.adj, c.adj2
    if form == "csr":
        monkeypatch.setattr(ops, "a1_bitmap_max_bytes", 0)
        adj = to_product(c.oadj, DEV)
        adj2 = SparseTensor(rowptr=c.adj2._rowptr, col=c.adj2._col, sparse_sizes=(c.n, c.n))
        assert adj.bit_rows() is None and adj2.product_bit_rows() is None
    else:
        assert adj.bit_rows() is not None and adj2.product_bit_rows() is not None
    ed = c.e.to(DEV)
    table = Hx.node_table(adj)
    assert table.is_cuda and torch.equal(table.cpu(), ref_table(c.oadj)) and Hx.node_table(adj) is table
    out = Hx.link_heuristics(adj, adj2, ed)
    assert out.shape == (c.B, 8) and out.dtype == torch.float32 and out.is_cuda
    for q, kind in enumerate(KINDS):
        assert torch.equal(out[:, q].cpu(), r.scores[:, q]), kind
    none = (r.c1 == 0) & (r.c2 == 0)
    assert not bool(out.cpu()[none][:, [0, 1, 2, 3, 5, 6, 7]].any())           # neither set: zeros (pa is the degrees' product)
    pick = ("ra2", "jaccard", "cn")
    assert torch.equal(Hx.link_heuristics(adj, adj2, ed, pick, wsd={}), out[:, [7, 3, 0]])
    assert torch.equal(Hx.link_heuristics(adj, None, ed, ("aa", "pa")), out[:, [1, 4]])
    user = torch.randn(c.n, 2, generator=torch.Generator().manual_seed(9))
    ru = restate(c.oadj, c.oadj2, c.e, user)
    u1, u2 = Hx.weighted_cn(adj, adj2, ed, user.to(DEV))
    assert torch.equal(u1.cpu(), ru.s1[:, 2:]) and torch.equal(u2.cpu(), ru.s2[:, 2:])
    assert Hx.node_table(adj) is table and Hx.node_table(adj, user.to(DEV)) is not table      # user columns are not cached
    v1, v2 = Hx.weighted_cn(adj, None, ed, user[:, 0].contiguous().to(DEV))
    assert torch.equal(v1[:, 0], u1[:, 0]) and not bool(v1[:, 1].any()) and not bool(v2.any())


@pytest.mark.parametrize("fillers", [0, 40, 200], ids=["three_entries", "one_block", "three_blocks"])
def test_the_order_of_the_adds_decides_the_result(hiplib, fillers):
    """Three common neighbours a < b < c.  With the weights {2^24, 1, 1} the sequential sum is 16777216 (each 1 is absorbed),
    with {1, 1, 2^24} it is 16777218: any other order of the adds gives another number.  ``fillers`` more neighbours of the
    source alone spread a, b, c over the lanes of one probe block and, at 200, over three blocks of 64 positions."""
    from ocn_amd import heuristics as Hx
    from ocn_amd.sparse import SparseTensor
    n, i, j = 300, 0, 1
    row = list(range(10, 10 + max(fillers, 3)))                          # N(i): ascending ids from 10
    pos = (0, 1, 2) if fillers == 0 else ((5, 20, 38) if fillers == 40 else (5, 90, 180))
    a, b, c = (row[p] for p in pos)
    if fillers == 200:
        assert pos[0] // 64 < pos[1] // 64 < pos[2] // 64
    ei = torch.tensor([[i] * len(row) + [j] * 3, row + [a, b, c]])
    ei = torch.cat([ei, ei.flip(0)], dim=1)
    adj = SparseTensor.from_edge_index(ei.to(DEV), sparse_sizes=(n, n))
    big = float(2 ** 24)
    w = torch.zeros(n, 2)
    w[[a, b, c], 0] = torch.tensor([big, 1.0, 1.0])
    w[[a, b, c], 1] = torch.tensor([1.0, 1.0, big])
    w[row[-1] if fillers else 299] += 0.5                                # (a neighbour of i alone: never added)
    e = torch.tensor([[i, j], [j, i]]).to(DEV)
    for t2 in (adj, product_adj2(adj)):                                  # as T2: A itself, and A² (a, b, c are 2-hop members of neither)
        s1, s2 = Hx.weighted_cn(adj, t2, e, w.to(DEV))
        assert s1.tolist() == [[16777216.0, 16777218.0]] * 2
        if t2 is adj:
            assert s2.tolist() == [[16777216.0, 16777218.0]] * 2
    assert Hx.link_heuristics(adj, None, e, ("cn",)).tolist() == [[3.0], [3.0]]


def test_closed_forms_on_a_complete_bipartite_graph_and_a_path(hiplib):
    """K_{m,n} needs no oracle.  Two nodes of L share the whole of R (n nodes of degree m) and nothing else: cn = n, jaccard =
    n / (n + n - n) = 1, pa = n², ra / aa = n copies of fl(1 / m) / fl(1 / log m) added one by one; A² links a node to its own
    side only, so cn2 = 0 for the pair and n for a cross pair, whose cn is 0.  The ends of a path a - b - c: aa = fl(1 / log 2)."""
    from ocn_amd import heuristics as Hx
    from ocn_amd.sparse import SparseTensor
    m, n = 70, 9                                                         # (70 > 64: a pair of R walks two probe blocks)
    adj, adj2 = bipartite(m, n, extra=2)
    inv = lambda d: 1.0 / torch.tensor(float(d), dtype=torch.float32)
    invlog = lambda d: 1.0 / torch.log(torch.tensor(float(d), dtype=torch.float32))
    pairs = torch.tensor([[0, m, 0, m + 1, 5, m + n], [1, m + 1, m, 4, m + n, m + n + 1]])       # L-L, R-R, L-R, R-L, L-iso, iso-iso
    out = Hx.link_heuristics(adj, adj2, pairs.to(DEV)).cpu()
    want = torch.tensor([
        # cn  aa                          ra                       jaccard  pa      cn2  aa2                         ra2
        [n, chain([invlog(m)] * n), chain([inv(m)] * n), 1.0, n * n, 0, 0.0, 0.0],
        [m, chain([invlog(n)] * m), chain([inv(n)] * m), 1.0, m * m, 0, 0.0, 0.0],
        [0, 0.0, 0.0, 0.0, n * m, n, chain([invlog(m)] * n), chain([inv(m)] * n)],
        [0, 0.0, 0.0, 0.0, m * n, m, chain([invlog(n)] * m), chain([inv(n)] * m)],
        [0, 0.0, 0.0, 0.0, 0.0, 0, 0.0, 0.0],
        [0, 0.0, 0.0, 0.0, 0.0, 0, 0.0, 0.0]], dtype=torch.float32)
    assert torch.equal(out, want), (out, want)
    a, b, c = 0, 1, 2
    path = SparseTensor.from_edge_index(torch.tensor([[a, b, b, c], [b, a, c, b]]).to(DEV), sparse_sizes=(4, 4))
    got = Hx.link_heuristics(path, None, torch.tensor([[a], [c]]).to(DEV), ("cn", "aa", "ra", "jaccard", "pa")).cpu()
    assert torch.equal(got, torch.tensor([[1.0, float(invlog(2)), 0.5, 1.0, 1.0]]))
    assert float(invlog(2)) == pytest.approx(1.4426950408889634, rel=1e-6)


def test_empty_batches_and_candidates_without_any_set(hiplib):
    from ocn_amd import heuristics as Hx, ops
    adj, adj2 = bipartite(5, 3, extra=3)
    none = torch.tensor([[8, 9, 10], [9, 10, 8]]).to(DEV)               # isolated nodes: no set, no degree
    assert not bool(Hx.link_heuristics(adj, adj2, none).any())
    u1, u2 = Hx.weighted_cn(adj, adj2, none, torch.ones(11, device=DEV))
    assert not bool(u1.any()) and not bool(u2.any())
    empty = torch.zeros(2, 0, dtype=torch.int64, device=DEV)
    out = Hx.link_heuristics(adj, adj2, empty)
    assert out.shape == (0, 8) and out.dtype == torch.float32 and out.is_cuda
    s1, s2, n1, n2, deg = ops.cn_node_sums(adj._rowptr, adj._col, (adj._rowptr, adj._col), None, empty[0], empty[1], Hx.node_table(adj))
    assert s1.shape == (0, 4) and s2.shape == (0, 4) and n1.shape == (0,) and n2.shape == (0,) and deg.shape == (0, 2)
    assert Hx.score_edges_heuristic(adj, adj2, empty.t(), 16, "aa2").shape == (0,)
    with pytest.raises(IndexError):                                      # ids are bounds-checked, as every op checks them
        Hx.link_heuristics(adj, None, torch.tensor([[0], [11]]).to(DEV), ("cn",))


@pytest.mark.parametrize("kind", ["ra", "aa2", "jaccard"])
def test_scoring_loop_equals_its_batches_and_the_restatement(mid, kind):
    """``score_edges_heuristic`` = the per-batch ``link_heuristics`` calls over the same ``PermIterator`` batches, concatenated;
    two runs are bit-equal; the scores are the restatement's, and so are the Hits@K they give through ``Evaluator``."""
    from ocn_amd import heuristics as Hx
    from ocn_amd.evaluate import Evaluator
    from ocn_amd.utils import PermIterator
    c = mid
    edges = c.e.t().contiguous().to(DEV)                                 # [n, 2]: the split_edge layout
    bs = 700                                                             # six full batches and a ragged tail
    got = Hx.score_edges_heuristic(c.adj, c.adj2, edges, bs, kind)
    assert got.shape == (c.B,) and got.dtype == torch.float32 and got.is_cuda
    parts = [Hx.link_heuristics(c.adj, c.adj2, edges[perm].t(), (kind,))[:, 0] for perm in PermIterator(DEV, c.B, bs, training=False)]
    assert len(parts) == 7 and torch.equal(got, torch.cat(parts))
    assert torch.equal(Hx.score_edges_heuristic(c.adj, c.adj2, edges, bs, kind, run_ahead=1), got)
    assert torch.equal(Hx.score_edges_heuristic(c.adj, c.adj2, edges, c.B, kind), got)       # nothing depends on the batch
    ref = restate(c.oadj, c.oadj2, c.e).scores[:, KINDS.index(kind)]
    assert torch.equal(got.cpu(), ref)
    half = c.B // 2
    ev = Evaluator(name="ogbl-collab")
    for K in (20, 50, 100):
        ev.K = K
        mine = ev.eval({"y_pred_pos": got[:half], "y_pred_neg": got[half:]})[f"hits@{K}"]
        theirs = ev.eval({"y_pred_pos": ref[:half], "y_pred_neg": ref[half:]})[f"hits@{K}"]
        assert mine == theirs
    assert 0.0 < mine <= 1.0


def test_heuristic_example_driver_prints_the_metric(hiplib, capsys):
    """examples/run_like_reference.py --heuristic ra on the Cora shape: no training, the dataset's metric on valid and test."""
    import importlib.util
    import re
    spec = importlib.util.spec_from_file_location("run_like_reference", os.path.join(ROOT, "examples", "run_like_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.main(["--dataset", "cora", "--heuristic", "ra"])
    line = re.search(r"heuristic ra hits@100 valid/test (\d\.\d{4})/(\d\.\d{4})", capsys.readouterr().out)
    assert line and set(res) == {"valid", "test"}
    assert float(line.group(1)) == pytest.approx(res["valid"], abs=1e-4) and float(line.group(2)) == pytest.approx(res["test"], abs=1e-4)
    assert all(0.0 <= v <= 1.0 for v in res.values())
    res2 = mod.main(["--dataset", "cora", "--heuristic", "cn2", "--use_valedges_as_input"])
    assert set(res2) == {"valid", "test"} and all(0.0 <= v <= 1.0 for v in res2.values())
