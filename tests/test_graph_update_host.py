"""Edge insertion (ocn_amd/update.py; ``ocn_csr_union_count`` / ``_fill``, ``ocn_bitrows_insert``) without a GPU: the entries'
argument checks, the refusals of ``insert_edges``, and its CPU route against an independent dense numpy model."""
import os
import re
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from ocn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = c_void_p(4096)             # a non-NULL address that is never read: every call below returns before its first HIP call
Z = c_void_p(0)
NEW = ("ocn_csr_union_count", "ocn_csr_union_fill", "ocn_bitrows_insert")


def test_new_entries_are_additions_to_abi_9(hiplib):
    hdr = open(os.path.join(ROOT, "include", "ocn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW + ("ocn_bitrows_insert_workspace_bytes",):
        assert name in _lib.SIGNATURES and hasattr(hiplib, name)
        m = re.search(name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, f"{name} is not declared in ocn_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "#define OCN_ABI_VERSION 9" in hdr
    assert hiplib.ocn_abi_version() == _lib.ABI_VERSION == 9
    history = hdr[hdr.index("Later additions to 9"):hdr.index("#define OCN_ABI_VERSION")]
    for name in ("ocn_csr_union_count", "ocn_bitrows_insert"):
        assert name in history
    # items int32[2 E] + offsets int64[2 E + 1] + rows int32[E] + the scan's state
    assert hiplib.ocn_bitrows_insert_workspace_bytes(1000) >= 1000 * (8 + 16 + 4) + hiplib.ocn_scan_workspace_bytes(2000)
    assert hiplib.ocn_bitrows_insert_workspace_bytes(-1) == 0


def test_union_entries_reject_bad_arguments_before_any_hip_call(hiplib):
    def count(**kw):
        a = dict(rpA=P, cA=P, rpB=P, cB=P, n=4, count=P)
        a.update(kw)
        return hiplib.ocn_csr_union_count(a["rpA"], a["cA"], a["rpB"], a["cB"], a["n"], a["count"], Z)

    def fill(**kw):
        a = dict(rpA=P, cA=P, rpB=P, cB=P, n=4, rpC=P, cC=P)
        a.update(kw)
        return hiplib.ocn_csr_union_fill(a["rpA"], a["cA"], a["rpB"], a["cB"], a["n"], a["rpC"], a["cC"], Z)

    for name in ("rpA", "cA", "rpB", "cB", "count"):
        assert count(**{name: Z}) == -1, name
    for name in ("rpA", "cA", "rpB", "cB", "rpC", "cC"):
        assert fill(**{name: Z}) == -1, name
    assert count(n=-1) == -1 and fill(n=-1) == -1
    assert count(n=0, rpA=Z) == -1 and fill(n=0, rpC=Z) == -1             # (an empty call is still checked)
    assert count(n=0) == 0 and fill(n=0) == 0                              # ... and a valid one launches nothing


def test_bitrows_insert_entry_rejects_bad_arguments_before_any_hip_call(hiplib):
    def ins(**kw):
        a = dict(rpA=P, cA=P, rpT=P, cT=P, rpD=P, cD=P, n=64, nnz=3, bits=P, stride=2, added=P, ws=P)
        a.update(kw)
        return hiplib.ocn_bitrows_insert(a["rpA"], a["cA"], a["rpT"], a["cT"], a["rpD"], a["cD"], a["n"], a["nnz"], a["bits"],
                                         a["stride"], a["added"], a["ws"], Z)

    for name in ("rpA", "cA", "rpT", "cT", "rpD", "cD", "bits", "added", "ws"):
        assert ins(**{name: Z}) == -1, name
    assert ins(n=-1) == -1 and ins(nnz=-1) == -1 and ins(stride=-1) == -1
    assert ins(n=65) == -1                                                 # two words hold 64 columns
    assert ins(nnz=1 << 30) == -1
    assert ins(nnz=0, bits=Z) == -1 and ins(n=0, stride=0, added=Z) == -1  # (an empty call is still checked)
    assert ins(nnz=0) == 0 and ins(n=0, stride=0) == 0                     # ... and a valid one launches nothing


def test_op_wrappers_refuse_cpu_tensors_and_mismatched_shapes(hiplib, monkeypatch):
    from ocn_amd import ops
    rp3, rp2 = torch.tensor([0, 1, 2, 2]), torch.tensor([0, 1, 2])
    col = torch.tensor([1, 0], dtype=torch.int32)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.csr_union_count(rp3, col, rp3, col)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.csr_union_fill(rp3, col, rp3, col, rp3)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.bitrows_insert(rp3, col, rp3, col, rp3, col, torch.zeros(3, 1, dtype=torch.int32))
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name, ndim=None: t)
    with pytest.raises(ValueError, match="A has 3 rows, B 2"):
        ops.csr_union_count(rp3, col, rp2, col)
    with pytest.raises(ValueError, match="rowptrC: one entry per row and the total"):
        ops.csr_union_fill(rp3, col, rp3, col, rp2)
    with pytest.raises(ValueError, match="must all be n x n"):
        ops.bitrows_insert(rp3, col, rp3, col, rp2, col, torch.zeros(3, 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="must all be n x n"):
        ops.bitrows_insert(rp3, col, rp3, col, rp3, col, torch.zeros(2, 1, dtype=torch.int32))


# ---- insert_edges on CPU tensors against a dense numpy model -----------------------------------------------------------------
def _dense(sp, n):
    d = np.zeros((n, n), dtype=bool)
    rp, col = sp._rowptr.numpy(), sp._col.numpy()
    for r in range(n):
        row = col[rp[r]:rp[r + 1]]
        assert (np.diff(row) > 0).all(), "columns must be ascending and duplicate-free"
        d[r, row] = True
    assert col.dtype == np.int32 and rp[-1] == col.size
    return d


def _case(seed):
    """(n, A dense bool, new entries [2, E], undirected) — the sweep covers n = 1 .. 70, E == 0, duplicates, entries already
    present and self loops; symmetric A where undirected."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 71)) if seed >= 8 else (1, 2, 31, 32, 33, 64, 65, 70)[seed]
    undirected = bool(seed % 2)
    a = rng.random((n, n)) < rng.choice([0.0, 0.03, 0.15])
    if undirected:
        a = a | a.T
    kind = seed % 5
    e = 0 if kind == 0 else int(rng.integers(1, 2 * n + 1))
    new = rng.integers(0, n, size=(2, e))
    if kind == 1 and e:                                       # duplicates: every entry twice, and once more reversed
        new = np.concatenate([new, new, new[::-1]], axis=1)
    if kind == 2 and a.any():                                 # entries A already has
        r, c = np.nonzero(a)
        pick = rng.integers(0, r.size, size=min(5, r.size))
        new = np.concatenate([new, np.stack([r[pick], c[pick]])], axis=1)
    if kind == 3:                                             # self loops
        loops = rng.integers(0, n, size=3)
        new = np.concatenate([new, np.stack([loops, loops])], axis=1)
    return n, a, new.astype(np.int64), undirected


@pytest.mark.parametrize("seed", range(40))
def test_insert_edges_cpu_matches_the_dense_model(seed):
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.update import insert_edges
    n, a, new, undirected = _case(seed)
    r, c = np.nonzero(a)
    adj = SparseTensor.from_edge_index(torch.from_numpy(np.stack([r, c])), sparse_sizes=(n, n))
    a2 = (a.astype(np.int64) @ a.astype(np.int64)) > 0
    r2, c2 = np.nonzero(a2)
    adj2 = SparseTensor.from_edge_index(torch.from_numpy(np.stack([r2, c2])), sparse_sizes=(n, n))
    before = (adj._rowptr.clone(), adj._col.clone(), adj2._rowptr.clone(), adj2._col.clone())

    want = a.copy()
    want[new[0], new[1]] = True
    if undirected:
        want[new[1], new[0]] = True
    want2 = (want.astype(np.int64) @ want.astype(np.int64)) > 0

    e = torch.from_numpy(new)
    adj_new, adj2_new = insert_edges(adj, e, adj2, undirected=undirected)
    assert adj_new.sparse_sizes() == (n, n) and adj2_new.sparse_sizes() == (n, n)
    assert not adj_new.has_value() and not adj2_new.has_value()
    assert (_dense(adj_new, n) == want).all()
    assert (_dense(adj2_new, n) == want2).all()
    only, none = insert_edges(adj, e, None, undirected=undirected)           # the walk route: no stored product
    assert none is None and torch.equal(only._rowptr, adj_new._rowptr) and torch.equal(only._col, adj_new._col)
    # the same content as the long way round
    cat = torch.cat([torch.stack([adj.storage.row(), adj.storage.col()]), e], dim=1)
    long_way = SparseTensor.from_edge_index(cat, sparse_sizes=(n, n))
    long_way = long_way.to_symmetric() if undirected else long_way.coalesce()
    assert torch.equal(long_way._rowptr, adj_new._rowptr) and torch.equal(long_way._col, adj_new._col)
    if new.shape[1] == 0:
        assert torch.equal(adj_new._rowptr, adj._rowptr) and torch.equal(adj_new._col, adj._col)
        assert torch.equal(adj2_new._rowptr, adj2._rowptr) and torch.equal(adj2_new._col, adj2._col)
    for was, now in zip(before, (adj._rowptr, adj._col, adj2._rowptr, adj2._col)):    # the inputs are never modified
        assert torch.equal(was, now)


def test_insert_edges_cpu_donate_retires_the_old_product():
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.update import insert_edges
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), sparse_sizes=(4, 4))
    adj2 = SparseTensor.from_edge_index(torch.tensor([[0, 0, 1, 2, 2], [0, 2, 1, 0, 2]]), sparse_sizes=(4, 4))
    adj_new, adj2_new = insert_edges(adj, torch.tensor([[2], [3]]), adj2, donate=True)
    assert adj2_new.nnz() == 8 and adj_new.nnz() == 6              # the path 0-1-2-3: A² row r = {r, r ± 2}
    with pytest.raises(Exception):
        adj2.nnz()


def test_insert_edges_raises_value_errors_on_misuse():
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.update import insert_edges
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    adj = SparseTensor.from_edge_index(ei, sparse_sizes=(4, 4))
    ok = torch.tensor([[0], [3]])
    with pytest.raises(ValueError, match="valued"):
        insert_edges(adj.fill_value(1.0), ok)
    with pytest.raises(ValueError, match="valued"):
        insert_edges(adj, ok, adj.fill_value(1.0))
    for bad in (torch.tensor([[0], [4]]), torch.tensor([[4], [0]]), torch.tensor([[-1], [0]]), torch.tensor([[1, 0], [2, -1]])):
        for undirected in (True, False):
            with pytest.raises(ValueError, match="out of range"):
                insert_edges(adj, bad, undirected=undirected)
    for bad in (torch.tensor([0, 3]), torch.tensor([[0, 3]]), torch.tensor([[0, 3], [1, 2], [2, 1]]), torch.zeros(0, dtype=torch.int64),
                torch.tensor([[0], [3]], dtype=torch.int32), torch.tensor([[0.0], [3.0]]), [[0], [3]]):
        with pytest.raises(ValueError, match=r"int64 tensor of shape \[2, E\]"):
            insert_edges(adj, bad)
    other = SparseTensor.from_edge_index(ei, sparse_sizes=(5, 5))
    with pytest.raises(ValueError, match="adj2 is"):
        insert_edges(adj, ok, other)
    with pytest.raises(ValueError, match="not square"):
        insert_edges(SparseTensor.from_edge_index(ei, sparse_sizes=(4, 5)), ok)
