"""Structured negative sampling (ocn_amd/sampling.py on ``ocn_sample_complement_rows`` / ``_pairs``) on the GPU against the CPU
mirror of tests/sampling_mirror.py.  A sample is an integer fixed by (seed, its own index, known), so every comparison is
``torch.equal``; the properties (in range, not the source, not a stored link) are computed with torch on the result."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import sampling_mirror as SM
from tests.helpers import make_graph, to_product

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PERS = (1, 63, 64, 65, 1000)     # below, at and above a wave's 64-sample chunk, and many chunks
SEED = (0x5EED << 32) | 0x1234   # both key words in use


# ---- graphs ------------------------------------------------------------------------------------------------------------
def csr_case(n, rows, sources):
    """``rows``: {row id: ascending columns}.  The CSR as numpy arrays (the mirror's operand) and as a SparseTensor on the GPU."""
    from ocn_amd.sparse import SparseTensor
    rowptr = np.zeros(n + 1, dtype=np.int64)
    for s in range(n):
        rowptr[s + 1] = rowptr[s] + len(rows.get(s, ()))
    col = np.array([c for s in range(n) for c in rows.get(s, ())], dtype=np.int32)
    for s, cols in rows.items():
        assert list(cols) == sorted(set(cols)) and (not len(cols) or (0 <= cols[0] and cols[-1] < n)), s
    adj = SparseTensor(rowptr=torch.from_numpy(rowptr).to(DEV), col=torch.from_numpy(col).to(DEV), sparse_sizes=(n, n))
    dense = torch.zeros(n, n, dtype=torch.bool)
    dense[torch.from_numpy(np.repeat(np.arange(n), np.diff(rowptr))), torch.from_numpy(col).long()] = True
    src = np.array(sources, dtype=np.int64)
    return SimpleNamespace(n=n, rowptr=rowptr, col=col, adj=adj, dense=dense.to(DEV), src=src,
                           sources=torch.from_numpy(src).to(DEV))


def with_mirror(c):
    """The mirror of the longest call, once per graph: every shorter ``per`` is a prefix of it by the mirror's construction."""
    c.want = torch.from_numpy(SM.negative_targets(c.rowptr, c.col, c.n, c.src, max(PERS), SEED))
    return c


@pytest.fixture(scope="module")
def special(hiplib):
    """n = 97: an empty row, a row adjacent to every other node, a stored self-loop, rows of length 1, excluded sets that start
    at column 0 or end at column 96, a repeated source; random rows elsewhere."""
    n = 97
    rng = np.random.default_rng(97)
    rows = {s: sorted(rng.choice(n, size=int(rng.integers(1, 30)), replace=False).tolist()) for s in range(20, n - 1)}
    rows[1] = [c for c in range(n) if c != 1]                # adjacent to every other node: all -1
    rows[2] = [0, 2, 40, 96]                                 # stored self-loop
    rows[3], rows[4], rows[5] = [50], [0], [96]              # length 1
    rows[6] = [0, 1, 2, 3, 4, 5]                             # run from column 0 that the source extends: excluded 0..6
    rows[7] = list(range(90, 97))                            # run up to column 96
    rows[8] = list(range(0, 97, 2))
    rows[9] = [c for c in range(n) if c not in (9, 33)]      # one member left
    rows[96] = list(range(80, 96))                           # the source closes the run at column 96: excluded 80..96
    sources = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 96, 20, 21, 50, 95, 6, 0, 2, 33]      # row 0 is empty; 6, 0 and 2 repeat
    c = csr_case(n, rows, sources)
    assert c.rowptr[1] == c.rowptr[0] and 0 not in rows
    return with_mirror(c)


@pytest.fixture(scope="module")
def hubs(hiplib):
    """n = 2 cap + 200 with hub rows of cap, cap + 1 and cap + 70 columns: the LDS path, its boundary and the in-memory path."""
    from ocn_amd import ops
    cap = ops.sample_stage_cols()
    n = 2 * cap + 200
    rng = np.random.default_rng(cap)
    rows = {s: sorted(rng.choice(n, size=int(rng.integers(0, 40)), replace=False).tolist()) for s in range(n)}
    for s, d in ((10, cap), (11, cap + 1), (12, cap + 70), (n - 1, cap - 1)):
        rows[s] = sorted(rng.choice(n, size=d, replace=False).tolist())
    rows[13] = sorted(set(rng.choice(n, size=cap, replace=False).tolist()) | {13})      # a long row that stores its source
    c = csr_case(n, rows, [10, 11, 12, 13, n - 1, 0, 500, 11])
    deg = np.diff(c.rowptr)
    assert (deg[10], deg[11], deg[12]) == (cap, cap + 1, cap + 70) and deg[13] in (cap, cap + 1)
    c.cap = cap
    return with_mirror(c)


def key_set(c):
    return torch.from_numpy(np.repeat(np.arange(c.n), np.diff(c.rowptr)) * c.n + c.col.astype(np.int64)).to(DEV)


def sparse_case(n, avg_deg, seed):
    """A sparse random directed graph as numpy CSR and on the GPU (no dense matrix: n is large)."""
    from ocn_amd.sparse import SparseTensor
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, n, size=n * avg_deg, dtype=np.int64) * n + rng.integers(0, n, size=n * avg_deg, dtype=np.int64))
    row, col = keys // n, (keys % n).astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))]).astype(np.int64)
    adj = SparseTensor(rowptr=torch.from_numpy(rowptr).to(DEV), col=torch.from_numpy(col).to(DEV), sparse_sizes=(n, n))
    has_self = np.bincount(row[row == col], minlength=n)
    cptr = np.concatenate([[0], np.cumsum(n - np.diff(rowptr) - (1 - has_self))]).astype(np.int64)
    return SimpleNamespace(n=n, rowptr=rowptr, col=col, adj=adj, cptr=cptr, keys=torch.from_numpy(keys).to(DEV))


# ---- 1. the generator ---------------------------------------------------------------------------------------------------
def bits(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def test_generator_gives_the_known_answers_and_equals_the_mirror(hiplib):
    from ocn_amd import ops
    for ctr, key, want in SM.KNOWN_ANSWERS:
        got = ops.philox4x32(bits(np.array([ctr], dtype=np.uint32)), key[0], key[1])
        assert got.dtype == torch.int32 and got.shape == (1, 4)
        assert tuple(int(v) for v in got.cpu().numpy().view(np.uint32)[0]) == want
    rng = np.random.default_rng(1000)
    ctr = rng.integers(0, 1 << 32, size=(1000, 4), dtype=np.uint64).astype(np.uint32)
    key = (0xDEADBEEF, 0x00C0FFEE)
    got = ops.philox4x32(bits(ctr), *key).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, SM.philox4x32_np(ctr, key))
    assert ops.philox4x32(torch.zeros(0, 4, dtype=torch.int32, device=DEV), 0, 0).shape == (0, 4)


# ---- 2. per-source samples ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", PERS)
@pytest.mark.parametrize("graph", ["special", "hubs"])
def test_negative_targets_equal_the_mirror_bit_for_bit(graph, per, request):
    from ocn_amd.sampling import negative_targets
    c = request.getfixturevalue(graph)
    got = negative_targets(c.adj, c.sources, per, SEED)
    assert got.dtype == torch.int64 and got.shape == (len(c.src), per) and got.is_contiguous()
    assert torch.equal(got.cpu(), c.want[:, :per])


@pytest.mark.parametrize("graph", ["special", "hubs"])
def test_negative_targets_are_non_edges_of_their_source(graph, request):
    from ocn_amd.sampling import negative_targets
    c = request.getfixturevalue(graph)
    got = negative_targets(c.adj, c.sources, 1000, SEED + 1)
    src = c.sources[:, None].expand_as(got)
    full = (c.dense | torch.eye(c.n, dtype=torch.bool, device=DEV)).all(dim=1)[c.sources]      # nothing left outside the row
    assert bool((got[full] == -1).all()) and bool((got[~full] >= 0).all())
    if graph == "special":
        assert bool(full[1]) and int(full.sum()) == 1
        assert bool((got[9] == 33).all())                                                     # the one member left
    ok, s = got[~full], src[~full]
    assert bool((ok < c.n).all()) and bool((ok != s).all()) and not bool(c.dense[s, ok].any())
    # not degenerate: a source with many free columns sees many of them
    assert got[0].unique().numel() > 50 if graph == "special" else got[5].unique().numel() > 300


def test_negative_targets_prefix_chunk_seed_and_position(special, hubs):
    from ocn_amd.sampling import negative_targets
    for c in (special, hubs):
        long = negative_targets(c.adj, c.sources, 1000, SEED)
        assert torch.equal(long[:, :65], negative_targets(c.adj, c.sources, 65, SEED))
        Q1 = 3
        chunked = torch.cat([negative_targets(c.adj, c.sources[:Q1].contiguous(), 65, SEED, first=0),
                             negative_targets(c.adj, c.sources[Q1:].contiguous(), 65, SEED, first=Q1)])
        assert torch.equal(chunked, long[:, :65])
        assert not torch.equal(long, negative_targets(c.adj, c.sources, 1000, SEED + 1))
    # the same source at two query positions (6 at 6 and 15, 0 at 0 and 16) draws other samples
    long = negative_targets(special.adj, special.sources, 1000, SEED)
    assert special.src[6] == special.src[15] and special.src[0] == special.src[16]
    assert not torch.equal(long[6], long[15]) and not torch.equal(long[0], long[16])


# ---- 3. pairs -----------------------------------------------------------------------------------------------------------
def test_complement_ptr_counts_the_non_edges_and_is_cached(special):
    from ocn_amd.sampling import complement_ptr
    c = special
    cptr, total = complement_ptr(c.adj)
    want = SM.complement_ptr(c.rowptr, c.col, c.n)
    assert cptr.dtype == torch.int64 and cptr.cpu().tolist() == want and total == want[-1]
    assert total == int((~(c.dense | torch.eye(c.n, dtype=torch.bool, device=DEV))).sum())
    again, total2 = complement_ptr(c.adj)
    assert again is cptr and total2 == total


def test_negative_edges_equal_the_mirror_on_the_special_graph(special):
    from ocn_amd.sampling import negative_edges
    c = special
    num = 700                                                # three workgroups, a ragged last one
    got = negative_edges(c.adj, num, SEED)
    assert got.dtype == torch.int64 and got.shape == (2, num) and got.is_contiguous()
    assert torch.equal(got.cpu(), torch.from_numpy(SM.negative_edges(c.rowptr, c.col, c.n, num, SEED)))
    s, t = got[0], got[1]
    assert bool(((s >= 0) & (s < c.n) & (t >= 0) & (t < c.n)).all())
    assert bool((s != t).all()) and not bool(c.dense[s, t].any())
    assert not bool((s == 1).any())                          # row 1 has an empty complement: never a source
    assert s.unique().numel() > 60
    # prefix in num and in first
    assert torch.equal(got[:, :300], negative_edges(c.adj, 300, SEED))
    assert torch.equal(got[:, 300:], negative_edges(c.adj, num - 300, SEED, first=300))
    assert not torch.equal(got, negative_edges(c.adj, num, SEED + 1))
    assert negative_edges(c.adj, 0, SEED).shape == (2, 0)


def test_negative_edges_with_more_than_2_to_the_32_non_edges(hiplib):
    """n = 70 001, sparse: M = n (n - 1) - nnz is about 4.9e9 > 2^32, so the 64-bit rank, the search of the int64 prefix and the
    multiply-high are exercised.  The mirror is evaluated on the 4096 samples only; the prefix comes from numpy."""
    from ocn_amd.sampling import complement_ptr, negative_edges
    c = sparse_case(70_001, 6, seed=70)
    cptr, total = complement_ptr(c.adj)
    assert total == int(c.cptr[-1]) > (1 << 32) and torch.equal(cptr.cpu(), torch.from_numpy(c.cptr))
    num = 4096
    got = negative_edges(c.adj, num, SEED)
    want = SM.negative_edges(c.rowptr, c.col, c.n, num, SEED, cptr=c.cptr.tolist())
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    s, t = got[0], got[1]
    assert bool(((s >= 0) & (s < c.n) & (t >= 0) & (t < c.n) & (s != t)).all())
    assert not bool(torch.isin(s * c.n + t, c.keys).any())
    assert int(s.max()) > c.n * 9 // 10 and int(s.min()) < c.n // 10         # ranks beyond 2^32 reach the last rows
    assert torch.equal(got[:, 1000:], negative_edges(c.adj, num - 1000, SEED, first=1000))


def test_negative_edges_refuses_a_graph_without_a_non_edge(hiplib):
    from ocn_amd.sampling import negative_edges
    n = 5
    c = csr_case(n, {s: [x for x in range(n) if x != s] for s in range(n)}, [0])
    with pytest.raises(ValueError, match="no non-edge"):
        negative_edges(c.adj, 4, 1)


# ---- 4. fit with the loops ----------------------------------------------------------------------------------------------
def test_negative_targets_feed_score_mrr_split_as_they_are(hiplib):
    from ocn_amd.model import predictor_dict
    from ocn_amd.pipeline import score_mrr_split
    from ocn_amd.sampling import negative_targets
    n, H, Q = 300, 64, 40
    adj = to_product(make_graph(n, 8, 40, seed=5), DEV)
    torch.manual_seed(3)
    h = torch.randn(n, H, device=DEV)
    pred = predictor_dict["cn7"](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()
    src = torch.arange(Q, device=DEV)
    dst = torch.arange(Q, 2 * Q, device=DEV)
    neg = negative_targets(adj, src, 3, seed=9)
    assert neg.shape == (Q, 3) and neg.dtype == torch.int64 and bool((neg >= 0).all())
    with torch.no_grad():
        pos_pred, neg_pred = score_mrr_split(pred, h, adj, src, dst, neg, 64, SimpleNamespace(sum=0.5))
    assert pos_pred.shape == (Q,) and neg_pred.shape == (Q, 3) and neg_pred.dtype == torch.float32
