"""Edge removal (ocn_amd/update.py; ``ocn_csr_minus_count`` / ``_fill``, ``ocn_bitrows_remove``) without a GPU: the entries'
argument checks, the refusals of ``remove_edges``, its CPU route against an independent dense numpy model, and a numpy
restatement of the kernel's candidate schedule against ``(A'·A') > 0``.  Everything is exact: no tolerance anywhere."""
import os
import re
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from ocn_amd import _lib
from tests.test_graph_update_host import _case, _dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = c_void_p(4096)             # a non-NULL address that is never read: every call below returns before its first HIP call
Z = c_void_p(0)
NEW = ("ocn_csr_minus_count", "ocn_csr_minus_fill", "ocn_bitrows_remove_workspace_bytes", "ocn_bitrows_remove")


def test_new_entries_are_additions_to_abi_9(hiplib):
    hdr = open(os.path.join(ROOT, "include", "ocn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(hiplib, name)
        m = re.search(name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, f"{name} is not declared in ocn_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "#define OCN_ABI_VERSION 9" in hdr
    assert hiplib.ocn_abi_version() == _lib.ABI_VERSION == 9
    history = hdr[hdr.index("Later additions to 9"):hdr.index("#define OCN_ABI_VERSION")]
    for name in ("ocn_csr_minus_count", "ocn_bitrows_remove_workspace_bytes", "ocn_bitrows_remove"):
        assert name in history
    # items int32[2 E] + offsets int64[2 E + 1] + rows int32[E] + the scan's state
    assert hiplib.ocn_bitrows_remove_workspace_bytes(1000) >= 1000 * (8 + 16 + 4) + hiplib.ocn_scan_workspace_bytes(2000)
    assert hiplib.ocn_bitrows_remove_workspace_bytes(-1) == 0


def test_minus_entries_reject_bad_arguments_before_any_hip_call(hiplib):
    def count(**kw):
        a = dict(rpA=P, cA=P, rpB=P, cB=P, n=4, count=P)
        a.update(kw)
        return hiplib.ocn_csr_minus_count(a["rpA"], a["cA"], a["rpB"], a["cB"], a["n"], a["count"], Z)

    def fill(**kw):
        a = dict(rpA=P, cA=P, rpB=P, cB=P, n=4, rpC=P, cC=P)
        a.update(kw)
        return hiplib.ocn_csr_minus_fill(a["rpA"], a["cA"], a["rpB"], a["cB"], a["n"], a["rpC"], a["cC"], Z)

    for name in ("rpA", "cA", "rpB", "cB", "count"):
        assert count(**{name: Z}) == -1, name
    for name in ("rpA", "cA", "rpB", "cB", "rpC", "cC"):
        assert fill(**{name: Z}) == -1, name
    assert count(n=-1) == -1 and fill(n=-1) == -1
    assert count(n=0, rpA=Z) == -1 and fill(n=0, rpC=Z) == -1             # (an empty call is still checked)
    assert count(n=0) == 0 and fill(n=0) == 0                              # ... and a valid one launches nothing


def test_bitrows_remove_entry_rejects_bad_arguments_before_any_hip_call(hiplib):
    ptrs = ("rpA0", "cA0", "rpT0", "cT0", "rpA", "cA", "rpT", "cT", "rpD", "cD", "bits", "removed", "ws")

    def rem(**kw):
        a = dict({name: P for name in ptrs}, n=64, nnz=3, stride=2)
        a.update(kw)
        return hiplib.ocn_bitrows_remove(a["rpA0"], a["cA0"], a["rpT0"], a["cT0"], a["rpA"], a["cA"], a["rpT"], a["cT"], a["rpD"],
                                         a["cD"], a["n"], a["nnz"], a["bits"], a["stride"], a["removed"], a["ws"], Z)

    for name in ptrs:
        assert rem(**{name: Z}) == -1, name
    assert rem(n=-1) == -1 and rem(nnz=-1) == -1 and rem(stride=-1) == -1
    assert rem(n=65) == -1                                                 # two words hold 64 columns
    assert rem(nnz=1 << 30) == -1
    assert rem(nnz=0, bits=Z) == -1 and rem(n=0, stride=0, removed=Z) == -1   # (an empty call is still checked)
    assert rem(nnz=0, cA0=Z) == -1 and rem(n=0, stride=0, rpT=Z) == -1
    assert rem(nnz=0) == 0 and rem(n=0, stride=0) == 0                     # ... and a valid one launches nothing


def test_op_wrappers_refuse_cpu_tensors_and_mismatched_shapes(hiplib, monkeypatch):
    from ocn_amd import ops
    rp3, rp2 = torch.tensor([0, 1, 2, 2]), torch.tensor([0, 1, 2])
    col = torch.tensor([1, 0], dtype=torch.int32)
    bits3, bits2 = torch.zeros(3, 1, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.csr_minus_count(rp3, col, rp3, col)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.csr_minus_fill(rp3, col, rp3, col, rp3)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.csr_minus(rp3, col, rp3, col)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.bitrows_remove(rp3, col, rp3, col, rp3, col, rp3, col, rp3, col, bits3)
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name, ndim=None: t)
    with pytest.raises(ValueError, match="A has 3 rows, B 2"):
        ops.csr_minus_count(rp3, col, rp2, col)
    with pytest.raises(ValueError, match="rowptrC: one entry per row and the total"):
        ops.csr_minus_fill(rp3, col, rp3, col, rp2)
    for at in (2, 4, 6, 8):                                                # the old transpose, A', its transpose, D
        args = [rp3, col] * 5
        args[at] = rp2
        with pytest.raises(ValueError, match="must all be n x n"):
            ops.bitrows_remove(*args, bits3)
    with pytest.raises(ValueError, match="must all be n x n"):
        ops.bitrows_remove(*([rp3, col] * 5), bits2)


# ---- remove_edges on CPU tensors against a dense numpy model ------------------------------------------------------------------
def _pair(a, n):
    """(adj, adj2) of the dense boolean matrix ``a``: the product from numpy, not from the code under test."""
    from ocn_amd.sparse import SparseTensor
    r, c = np.nonzero(a)
    adj = SparseTensor.from_edge_index(torch.from_numpy(np.stack([r, c])), sparse_sizes=(n, n))
    r2, c2 = np.nonzero((a.astype(np.int64) @ a.astype(np.int64)) > 0)
    return adj, SparseTensor.from_edge_index(torch.from_numpy(np.stack([r2, c2])), sparse_sizes=(n, n))


def _delta(n, edges, undirected):
    d = np.zeros((n, n), dtype=bool)
    d[edges[0], edges[1]] = True
    return d | d.T if undirected else d


@pytest.mark.parametrize("seed", range(40))
def test_remove_edges_cpu_matches_the_dense_model(seed):
    """The sweep of the insertion test read as removals: E == 0, duplicates, entries A has (kind 2 appends five of them; at
    density 0.15 the random ones hit A too), entries A lacks, self loops, directed and undirected, n = 1 .. 70."""
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.update import remove_edges
    n, a, gone, undirected = _case(seed)
    adj, adj2 = _pair(a, n)
    before = (adj._rowptr.clone(), adj._col.clone(), adj2._rowptr.clone(), adj2._col.clone())

    want = a & ~_delta(n, gone, undirected)
    want2 = (want.astype(np.int64) @ want.astype(np.int64)) > 0

    e = torch.from_numpy(gone)
    adj_new, adj2_new = remove_edges(adj, e, adj2, undirected=undirected)
    assert adj_new.sparse_sizes() == (n, n) and adj2_new.sparse_sizes() == (n, n)
    assert not adj_new.has_value() and not adj2_new.has_value()
    assert (_dense(adj_new, n) == want).all()
    assert (_dense(adj2_new, n) == want2).all()
    only, none = remove_edges(adj, e, None, undirected=undirected)           # the walk route: no stored product
    assert none is None and torch.equal(only._rowptr, adj_new._rowptr) and torch.equal(only._col, adj_new._col)
    # the same content as the long way round
    r, c = np.nonzero(want)
    long_way = SparseTensor.from_edge_index(torch.from_numpy(np.stack([r, c])), sparse_sizes=(n, n))
    assert torch.equal(long_way._rowptr, adj_new._rowptr) and torch.equal(long_way._col, adj_new._col)
    if gone.shape[1] == 0:
        assert torch.equal(adj_new._rowptr, adj._rowptr) and torch.equal(adj_new._col, adj._col)
        assert torch.equal(adj2_new._rowptr, adj2._rowptr) and torch.equal(adj2_new._col, adj2._col)
    for was, now in zip(before, (adj._rowptr, adj._col, adj2._rowptr, adj2._col)):    # the inputs are never modified
        assert torch.equal(was, now)


def test_remove_edges_cpu_donate_retires_the_old_product():
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.update import remove_edges
    i = torch.arange(3)
    adj = SparseTensor.from_edge_index(torch.stack([torch.cat([i, i + 1]), torch.cat([i + 1, i])]), sparse_sizes=(4, 4))
    adj2 = SparseTensor.from_edge_index(torch.tensor([[0, 0, 1, 1, 2, 2, 3, 3], [0, 2, 1, 3, 0, 2, 1, 3]]), sparse_sizes=(4, 4))
    adj_new, adj2_new = remove_edges(adj, torch.tensor([[2], [3]]), adj2, donate=True)
    # the path 0-1-2-3 minus (2, 3) is the path 0-1-2 and an isolated node: A² rows {0, 2}, {1}, {0, 2}, {}
    assert adj_new.nnz() == 4 and adj2_new.nnz() == 5
    assert adj2_new._rowptr.tolist() == [0, 2, 3, 5, 5] and adj2_new._col.tolist() == [0, 2, 1, 0, 2]
    with pytest.raises(Exception):
        adj2.nnz()


def test_remove_edges_raises_value_errors_on_misuse():
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.update import remove_edges
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    adj = SparseTensor.from_edge_index(ei, sparse_sizes=(4, 4))
    ok = torch.tensor([[0], [1]])
    with pytest.raises(ValueError, match="remove_edges: .*valued"):
        remove_edges(adj.fill_value(1.0), ok)
    with pytest.raises(ValueError, match="remove_edges: .*valued"):
        remove_edges(adj, ok, adj.fill_value(1.0))
    for bad in (torch.tensor([[0], [4]]), torch.tensor([[4], [0]]), torch.tensor([[-1], [0]]), torch.tensor([[1, 0], [2, -1]])):
        for undirected in (True, False):
            with pytest.raises(ValueError, match="remove_edges: .*out of range"):
                remove_edges(adj, bad, undirected=undirected)
    for bad in (torch.tensor([0, 3]), torch.tensor([[0, 3]]), torch.tensor([[0, 3], [1, 2], [2, 1]]), torch.zeros(0, dtype=torch.int64),
                torch.tensor([[0], [3]], dtype=torch.int32), torch.tensor([[0.0], [3.0]]), [[0], [3]]):
        with pytest.raises(ValueError, match=r"remove_edges: .*int64 tensor of shape \[2, E\]"):
            remove_edges(adj, bad)
    other = SparseTensor.from_edge_index(ei, sparse_sizes=(5, 5))
    with pytest.raises(ValueError, match="remove_edges: adj2 is"):
        remove_edges(adj, ok, other)
    with pytest.raises(ValueError, match="remove_edges: .*not square"):
        remove_edges(SparseTensor.from_edge_index(ei, sparse_sizes=(4, 5)), ok)
    with pytest.raises(ValueError, match="remove_edges: adj"):
        remove_edges(ei, ok)


def test_insert_edges_still_names_itself_in_its_refusals():
    """``_check_args`` serves both functions now; what ``insert_edges`` raises is what it raised before."""
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.update import insert_edges
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(4, 4))
    with pytest.raises(ValueError) as e:
        insert_edges(adj.fill_value(1.0), torch.tensor([[0], [3]]))
    assert str(e.value) == "insert_edges: a valued adjacency cannot take new entries (pattern matrices only)"
    with pytest.raises(ValueError) as e:
        insert_edges(adj, torch.tensor([0, 3]))
    assert str(e.value) == "insert_edges: new_edges must be an int64 tensor of shape [2, E]"


def test_removing_what_was_inserted_restores_the_pair_on_the_cpu_route():
    from ocn_amd.update import insert_edges, remove_edges
    for seed in range(6):
        rng = np.random.default_rng(900 + seed)
        n = int(rng.integers(5, 60))
        undirected = bool(seed % 2)
        a = rng.random((n, n)) < 0.1
        if undirected:
            a = a | a.T
        new = rng.integers(0, n, size=(2, 2 * n))
        new = new[:, ~(a[new[0], new[1]] | a[new[1], new[0]])]            # disjoint from A (and from its transpose)
        assert new.shape[1] > 0
        adj, adj2 = _pair(a, n)
        e = torch.from_numpy(new.astype(np.int64))
        mid, mid2 = insert_edges(adj, e, adj2, undirected=undirected)
        assert mid.nnz() > adj.nnz()
        back, back2 = remove_edges(mid, e, mid2, undirected=undirected)
        assert torch.equal(back._rowptr, adj._rowptr) and torch.equal(back._col, adj._col)
        assert torch.equal(back2._rowptr, adj2._rowptr) and torch.equal(back2._col, adj2._col)


# ---- the candidate schedule of ocn_bitrows_remove, restated in numpy -----------------------------------------------------------
CHUNK = 256                    # graph_update.hip: BI_CHUNK


def _schedule(a_old, a_new, d, chunk=CHUNK):
    """What the kernel does, item by item and in a shuffled order: per entry (u, v) of D, chunks of old row v (kind a:
    candidates (u, k)) and of old transposed row u (kind b: candidates (r, v)); a candidate whose bit is set is decided by
    'row r of A' meets row k of A'^T', cleared otherwise, and counted when the word still had the bit."""
    n = a_old.shape[0]
    bits = (a_old.astype(np.int64) @ a_old.astype(np.int64)) > 0
    removed = np.zeros(n, dtype=np.int64)
    items, candidates, survived = [], 0, 0
    for u, v in zip(*np.nonzero(d)):
        row_a, row_t = np.nonzero(a_old[v])[0], np.nonzero(a_old[:, u])[0]
        items += [(u, v, True, row_a[c:c + chunk]) for c in range(0, row_a.size, chunk)]
        items += [(u, v, False, row_t[c:c + chunk]) for c in range(0, row_t.size, chunk)]
    order = np.random.default_rng(n).permutation(len(items))
    for u, v, kind_a, elems in (items[i] for i in order):
        for x in elems:
            r, k = (u, x) if kind_a else (x, v)
            candidates += 1
            if not bits[r, k]:
                continue
            if (a_new[r] & a_new[:, k]).any():
                survived += 1
                continue
            had = bits[r, k]                                   # (atomicAnd hands back the word as it was)
            bits[r, k] = False
            removed[r] += int(had)
    return bits, removed, candidates, survived


def test_candidate_schedule_restated_in_numpy_is_exact():
    cleared = kept = 0
    for seed in range(120):
        rng = np.random.default_rng(3000 + seed)
        n = int(rng.integers(1, 71))
        undirected = bool(seed % 2)
        a = rng.random((n, n)) < rng.choice([0.03, 0.08, 0.3])
        e = int(rng.integers(1, 2 * n + 1))
        gone = rng.integers(0, n, size=(2, e))
        if a.any():                                                   # half from A, half at random: D overlaps A only in part
            r, c = np.nonzero(a)
            pick = rng.integers(0, r.size, size=e)
            gone = np.concatenate([gone, np.stack([r[pick], c[pick]])], axis=1)
        if undirected:
            a = a | a.T
        d = _delta(n, gone, undirected)
        a_new = a & ~d
        want = (a_new.astype(np.int64) @ a_new.astype(np.int64)) > 0
        old = (a.astype(np.int64) @ a.astype(np.int64)) > 0
        bits, removed, candidates, survived = _schedule(a, a_new, d, chunk=CHUNK if seed % 3 else 4)
        assert (bits == want).all()
        assert (removed == old.sum(1) - want.sum(1)).all()
        cleared += int(removed.sum())
        kept += survived
    assert cleared >= 100 and kept >= 100                               # both outcomes, in numbers
