"""Refreshing the encoder output after an edge update (ocn_amd/update.py: ``affected_rows``, ``EncoderState``;
``ocn_spmm_csr_rows``, ``ocn_rows_neighbourhood``, ``ocn_bitlist_count`` / ``_fill``) without a GPU: the row-set rule against an
independent numpy BFS, the argument refusals that need no device, and the entries' own argument checks."""
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
NEW = ("ocn_spmm_csr_rows", "ocn_rows_neighbourhood_workspace_bytes", "ocn_rows_neighbourhood", "ocn_bitlist_count",
       "ocn_bitlist_fill")


def test_new_entries_are_additions_to_abi_9(hiplib):
    hdr = open(os.path.join(ROOT, "include", "ocn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(hiplib, name)
        m = re.search(name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, f"{name} is not declared in ocn_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert len(_lib.SIGNATURES["ocn_spmm_csr_rows"][1]) == len(_lib.SIGNATURES["ocn_spmm_csr"][1]) + 2     # + rows, n_list
    assert "#define OCN_ABI_VERSION 9" in hdr
    assert hiplib.ocn_abi_version() == _lib.ABI_VERSION == 9
    history = hdr[hdr.index("Later additions to 9"):hdr.index("#define OCN_ABI_VERSION")]
    for name in ("ocn_spmm_csr_rows", "ocn_rows_neighbourhood"):
        assert name in history
    # items int32[n] + offsets int64[n + 1] + the scan's state
    assert hiplib.ocn_rows_neighbourhood_workspace_bytes(1000) >= 1000 * 4 + 1001 * 8 + hiplib.ocn_scan_workspace_bytes(1000)
    assert hiplib.ocn_rows_neighbourhood_workspace_bytes(-1) == 0


def test_spmm_csr_rows_entry_rejects_bad_arguments_before_any_launch(hiplib):
    def rows(**kw):
        a = dict(rp=P, col=P, val=Z, n=8, x=P, F=32, pre=Z, post=Z, mode=0, es=0, sm=0, rows=P, nl=3, y=P)
        a.update(kw)
        return hiplib.ocn_spmm_csr_rows(a["rp"], a["col"], a["val"], a["n"], a["x"], a["F"], a["pre"], a["post"], a["mode"],
                                        a["es"], a["sm"], a["rows"], a["nl"], a["y"], Z)

    for name in ("rp", "col", "x", "rows", "y"):
        assert rows(**{name: Z}) == -1, name
    assert rows(n=-1) == -1 and rows(nl=-1) == -1
    for F in (0, -16, 8, 24, 48, 1024):
        assert rows(F=F) == -1, F
    assert rows(mode=3) == -1 and rows(mode=-1) == -1 and rows(sm=3) == -1 and rows(sm=-1) == -1
    assert rows(nl=0, y=Z) == -1 and rows(nl=0, rows=Z) == -1              # (an empty call is still checked)
    assert rows(nl=0) == 0                                                 # ... and a valid one launches nothing
    for F in (16, 32, 64, 128, 256, 512):
        assert rows(nl=0, F=F) == 0


def test_neighbourhood_and_bitlist_entries_reject_bad_arguments_before_any_hip_call(hiplib):
    def nb(**kw):
        a = dict(rpT=P, cT=P, n=64, rows=P, nl=3, bits=P, ws=P)
        a.update(kw)
        return hiplib.ocn_rows_neighbourhood(a["rpT"], a["cT"], a["n"], a["rows"], a["nl"], a["bits"], a["ws"], Z)

    for name in ("rpT", "cT", "rows", "bits", "ws"):
        assert nb(**{name: Z}) == -1, name
    assert nb(n=-1) == -1 and nb(nl=-1) == -1 and nb(nl=1 << 30) == -1
    assert nb(nl=0, bits=Z) == -1 and nb(n=0, rows=Z) == -1                # (an empty call is still checked)
    assert nb(nl=0) == 0 and nb(n=0) == 0                                  # ... and a valid one launches nothing

    assert hiplib.ocn_bitlist_count(Z, 64, P, Z) == -1 and hiplib.ocn_bitlist_count(P, 64, Z, Z) == -1
    assert hiplib.ocn_bitlist_count(P, -1, P, Z) == -1 and hiplib.ocn_bitlist_count(P, 0, P, Z) == 0
    for args in ((Z, 64, P, P), (P, 64, Z, P), (P, 64, P, Z), (P, -1, P, P)):
        assert hiplib.ocn_bitlist_fill(*args, Z) == -1
    assert hiplib.ocn_bitlist_fill(P, 0, P, P, Z) == 0


def test_op_wrappers_refuse_cpu_tensors_and_mismatched_shapes(hiplib, monkeypatch):
    from ocn_amd import ops
    rp = torch.tensor([0, 1, 2, 2])
    col = torch.tensor([1, 0], dtype=torch.int32)
    rows = torch.tensor([0, 2])
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.spmm_csr_rows(rp, col, torch.zeros(3, 16), rows)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.rows_neighbourhood(rp, col, rows, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.bits_to_list(torch.zeros(1, dtype=torch.int32), 3)
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name, ndim=None: t)
    with pytest.raises(ValueError, match="unsupported width"):
        ops.spmm_csr_rows(rp, col, torch.zeros(3, 24), rows)
    with pytest.raises(ValueError, match="pre must have one entry per row of x"):
        ops.spmm_csr_rows(rp, col, torch.zeros(3, 16), rows, pre=torch.zeros(2))
    with pytest.raises(ValueError, match="post must have one entry per output row"):
        ops.spmm_csr_rows(rp, col, torch.zeros(3, 16), rows, post=torch.zeros(2))
    with pytest.raises(ValueError, match="val must have one entry per stored column"):
        ops.spmm_csr_rows(rp, col, torch.zeros(3, 16), rows, val=torch.zeros(3))
    with pytest.raises(ValueError, match="words of bits"):
        ops.rows_neighbourhood(rp, col, rows, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="words for"):
        ops.bits_to_list(torch.zeros(1, dtype=torch.int32), 33)
    assert 0.0 < ops.refresh_full_share < 1.0


# ---- affected_rows against a numpy BFS ------------------------------------------------------------------------------------------
def _bfs_sets(a, edges, hops, normalised, undirected):
    """R_1 .. R_hops from the definition, on a dense bool matrix: readers[k] = the rows r with a[r, k]."""
    n = a.shape[0]
    readers = [set(np.nonzero(a[:, k])[0].tolist()) for k in range(n)]
    if undirected:
        assert (a == a.T).all()

    def nb(s):
        out = set()
        for k in s:
            out |= readers[k]
        return out

    d = set(edges.reshape(-1).tolist())
    dplus = d | nb(d) if normalised else set(d)
    sets, prev = [], set()
    for _ in range(hops):
        prev = dplus | prev | nb(prev)
        sets.append(sorted(prev))
    return sets


def _adj_of(a):
    from ocn_amd.sparse import SparseTensor
    r, c = np.nonzero(a)
    return SparseTensor.from_edge_index(torch.from_numpy(np.stack([r, c]).astype(np.int64)), sparse_sizes=a.shape)


def _hub_dense(symmetric):
    """The N = 3000 hub graph of the update tests as a dense matrix: row 0 has 2500 entries, node 2999 is isolated."""
    n = 3000
    rng = np.random.default_rng(7)
    a = np.zeros((n, n), dtype=bool)
    a[0, 1:2501] = True
    rest = rng.integers(1, n - 1, size=(2, 6000))
    a[rest[0], rest[1]] = True
    if symmetric:
        a = a | a.T
    assert not a[n - 1].any() and not a[:, n - 1].any()
    return a, rng


def _check_sets(a, edges, undirected):
    from ocn_amd.update import affected_rows
    adj = _adj_of(a)
    e = torch.from_numpy(edges.astype(np.int64))
    for normalised in (False, True):
        for hops in range(4):
            got = affected_rows(adj, e, hops, normalised, undirected=undirected)
            want = _bfs_sets(a, edges, hops, normalised, undirected)
            assert len(got) == hops
            for g, w in zip(got, want):
                assert g.dtype == torch.int64 and g.tolist() == w


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 65])
def test_affected_rows_word_boundaries(n, symmetric):
    rng = np.random.default_rng(10 * n + symmetric)
    a = rng.random((n, n)) < 0.06
    if symmetric:
        a = a | a.T
    for e in (0, 1, 3):
        edges = rng.integers(0, n, size=(2, e))
        if e:
            edges[:, 0] = (n - 1, 0)                                       # the last row, the tail word
        _check_sets(a, edges, undirected=symmetric)


@pytest.mark.parametrize("symmetric", [True, False])
def test_affected_rows_hub_graph(symmetric):
    a, rng = _hub_dense(symmetric)
    n = a.shape[0]
    for edges in (np.array([[0], [0]]),                                   # the hub alone
                  np.array([[n - 1], [n - 1]]),                            # the isolated node alone: nothing to reach
                  np.array([[n - 1], [0]]),                                # isolated -> hub
                  rng.integers(0, n, size=(2, 50))):
        _check_sets(a, edges, undirected=symmetric)
    from ocn_amd.update import affected_rows
    alone = affected_rows(_adj_of(a), torch.tensor([[n - 1], [n - 1]]), 3, True, undirected=symmetric)
    assert [s.tolist() for s in alone] == [[n - 1]] * 3


def test_affected_rows_raises_value_errors_on_misuse():
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.update import affected_rows
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    adj = SparseTensor.from_edge_index(ei, sparse_sizes=(4, 4))
    ok = torch.tensor([[0], [3]])
    assert [s.tolist() for s in affected_rows(adj, ok, 2, False)] == [[0, 3], [0, 1, 3]]
    with pytest.raises(ValueError, match="valued"):
        affected_rows(adj.fill_value(1.0), ok, 2, True)
    for bad in (torch.tensor([[0], [4]]), torch.tensor([[4], [0]]), torch.tensor([[-1], [0]]), torch.tensor([[1, 0], [2, -1]])):
        with pytest.raises(ValueError, match="out of range"):
            affected_rows(adj, bad, 2, True)
    for bad in (torch.tensor([0, 3]), torch.tensor([[0, 3]]), torch.tensor([[0, 3], [1, 2], [2, 1]]), torch.zeros(0, dtype=torch.int64),
                torch.tensor([[0], [3]], dtype=torch.int32), torch.tensor([[0.0], [3.0]]), [[0], [3]]):
        with pytest.raises(ValueError, match=r"int64 tensor of shape \[2, E\]"):
            affected_rows(adj, bad, 2, True)
    with pytest.raises(ValueError, match="SparseTensor"):
        affected_rows(ei, ok, 2, True)
    with pytest.raises(ValueError, match="4 x 5"):
        affected_rows(SparseTensor.from_edge_index(ei, sparse_sizes=(4, 5)), ok, 2, True)


def test_encoder_state_refuses_misuse_without_a_device():
    """Training mode, grad enabled and a valued adjacency are refused before anything is computed; CPU tensors then meet the
    library's usual error (the encoder has no CPU path)."""
    from ocn_amd.model import GCN
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.update import EncoderState
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), sparse_sizes=(4, 4))
    x = torch.randn(4, 32)
    model = GCN(32, 32, 32, 2, 0.0, conv_fn="gcn")
    with torch.no_grad(), pytest.raises(ValueError, match="eval mode"):
        EncoderState(model.train(), x, adj)
    with pytest.raises(ValueError, match="eval mode"):
        EncoderState(model.eval(), x, adj)                                 # grad enabled
    with torch.no_grad(), pytest.raises(ValueError, match="without values"):
        EncoderState(model.eval(), x, adj.fill_value(1.0))
    with torch.no_grad(), pytest.raises(ValueError, match="x has 5 rows"):
        EncoderState(model.eval(), torch.randn(5, 32), adj)
    with torch.no_grad(), pytest.raises(_lib.OcnHipError, match="no CPU path"):
        EncoderState(model.eval(), x, adj)
