"""Shared builders for the parity tests: the same seeded graph as an oracle SpM and as the product
SparseTensor on the GPU; the builders and bit-exact comparisons of the graph-update tests."""
import numpy as np
import torch

from oracle import ocn_oracle as O
from ocn_amd.synth import chung_lu_graph, sample_edges


def make_graph(n, avg_deg, max_deg, seed, clique_frac=0.5, isolated=0):
    """Oracle-side symmetric adjacency; the last ``isolated`` node ids keep degree 0."""
    m = n - isolated
    ei = chung_lu_graph(m, avg_deg=avg_deg, max_deg=min(max_deg, m - 1), seed=seed, clique_frac=clique_frac)
    return O.to_symmetric(O.from_edge_index(ei, n))


def to_product(oadj, dev):
    from ocn_amd.sparse import SparseTensor
    return SparseTensor.from_edge_index(torch.stack([oadj.row, oadj.col]).to(dev),
                                        sparse_sizes=(oadj.n_rows, oadj.n_cols))


def product_adj2(adj):
    from ocn_amd.sparse import SparseTensor
    sp = adj.to_torch_sparse_coo_tensor()
    return SparseTensor.from_torch_sparse_coo_tensor(sp @ sp, False)


def batch(oadj, B, seed):
    return sample_edges(oadj.row, oadj.col, oadj.n_rows, B, seed=seed)


def header_defines():
    """name -> int of every ``#define OCN_* <integer>`` of include/ocn_hip.h."""
    import os
    import re
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ocn_hip.h")).read()
    return {k: int(v, 0) for k, v in re.findall(r"^#define\s+(OCN_\w+)\s+\(?(-?(?:0x[0-9a-fA-F]+|\d+))u?\)?\s*(?:/\*.*)?$", txt, re.M)}


_REC = header_defines()
_LEN, _FULL2, _HAS1, _HAS2 = (_REC[k] for k in ("OCN_REC_LEN_SHIFT", "OCN_REC_FULL2_BIT", "OCN_REC_HAS1_BIT", "OCN_REC_HAS2_BIT"))


def slot_record(e, i, j, a0, da, base, has1, has2, full2):
    """The OCN_REC_WORDS int64 words of a slot record (include/ocn_hip.h, ocn_cn_flags ``rec``), as Python ints: the unsigned
    words of the layout, reinterpreted as int64."""
    words = [e, i | j << 32, a0 | da << _LEN, base | int(bool(full2)) << _FULL2 | int(bool(has1)) << _HAS1 | int(bool(has2)) << _HAS2]
    assert len(words) == _REC["OCN_REC_WORDS"] and all(0 <= w < 1 << 64 for w in words)
    return [w - (1 << 64) if w >> 63 else w for w in words]


def slot_record_fields(words):
    """The inverse of ``slot_record``: (e, i, j, a0, da, base, has1, has2, full2)."""
    w = [int(x) & ((1 << 64) - 1) for x in words]
    return (w[0], w[1] & 0xffffffff, w[1] >> 32, w[2] & ((1 << _LEN) - 1), w[2] >> _LEN, w[3] & ((1 << _FULL2) - 1),
            bool(w[3] >> _HAS1 & 1), bool(w[3] >> _HAS2 & 1), bool(w[3] >> _FULL2 & 1))


def spm_equal(prod, spm):
    """product SparseTensor (device) vs oracle SpM: identical pattern."""
    r, c, _ = prod.coo()
    return (r.cpu().tolist() == spm.row.tolist()) and (c.cpu().tolist() == spm.col.tolist())


def close(a, b, atol=1e-5, rtol=1e-5):
    return torch.allclose(a.detach().cpu(), b.detach().cpu(), atol=atol, rtol=rtol)


# ---- graph updates (test_graph_update_gpu.py, test_graph_remove_gpu.py): everything bit-exact ------------------------------------
def st():
    from ocn_amd.sparse import SparseTensor
    return SparseTensor


def edges_of(adj):
    return torch.stack([adj.storage.row(), adj.storage.col()])


def random_graph(n, density, seed, symmetric=True, dev="cuda:0"):
    rng = np.random.default_rng(seed)
    a = rng.random((n, n)) < density
    if symmetric:
        a = a | a.T
    r, c = np.nonzero(a)
    ei = torch.from_numpy(np.stack([r, c]).astype(np.int64)).to(dev)
    return st().from_edge_index(ei, sparse_sizes=(n, n))


def same_adj(got, want):
    assert got._rowptr.dtype == torch.int64 and got._col.dtype == torch.int32
    assert torch.equal(got._rowptr, want._rowptr)
    assert torch.equal(got._col, want._col)


def same_product(got, want, bits=True):
    """Indistinguishable from the product formed from scratch: bit rows, row pointers, nnz and the ids behind the thunk."""
    if bits:
        assert got.product_bit_rows() is not None and want.product_bit_rows() is not None
        assert torch.equal(got.product_bit_rows(), want.product_bit_rows())
    assert torch.equal(got._rowptr, want._rowptr)
    assert got.nnz() == want.nnz()
    assert got._col.dtype == torch.int32 and torch.equal(got._col, want._col)


def csr_of_rows(rows, dev="cuda:0"):
    """(rowptr int64, col int32) on the device from one list of column ids per row."""
    rp = torch.tensor([0] + list(np.cumsum([len(r) for r in rows])), dtype=torch.int64, device=dev)
    col = torch.tensor([c for r in rows for c in r], dtype=torch.int32, device=dev)
    return rp, col
