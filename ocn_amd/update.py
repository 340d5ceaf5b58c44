"""Insert edges into a resident graph, or remove them: the adjacency and its stored A² updated exactly, without starting over.

The first thing a user does with recommended links is accept some of them (the reference adds its validation edges to the
adjacency under ``use_valedges_as_input``, NeighborOverlap_large.py:143-145 — and leaves A² stale).  Rebuilding sorts every
entry of A again and rewrites every bit row of A·A.  Both structures can be updated instead.  With D the new entries and
A' = A U D as 0/1 matrices,

    pattern(A'·A') = pattern(A·A) U pattern(D·A') U pattern(A'·D)

so ``insert_edges`` unions D (a CSR of the new entries alone, ``ocn_coo_to_csr``) into A row by row (``ocn_csr_union_*``) and
ORs the two thin products into the bit rows of A² (``ocn_bitrows_insert``): one row length of A' per new entry.

The way back — a link that is rejected, expires or was accepted by mistake, a hold-out split — is ``remove_edges``.  A pattern
cannot be decremented (that takes walk counts), but a bit can be decided again: bit (r, k) of A'·A', A' = A \\ D, is set
exactly when row r of A' and row k of A'^T share a column, and only bits with a witness walk through a removed entry can
differ from A·A.  ``remove_edges`` takes D out of A row by row (``ocn_csr_minus_*``) and re-decides those bits
(``ocn_bitrows_remove``): one row length of the old A per removed entry, each a short sorted-list intersection.

Valued adjacencies, updating the node embeddings ``h`` and more than one GPU are out of scope.
"""
from __future__ import annotations

import warnings
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import ops
from .sparse import SparseTensor


# function -> (the name of its edge argument, what a valued adjacency cannot do), for its error messages
_WORDS = {"insert_edges": ("new_edges", "take new entries"), "remove_edges": ("edges", "give up entries")}


def _check_args(fn: str, adj: SparseTensor, edges: Tensor, adj2: Optional[SparseTensor]) -> int:
    arg, verb = _WORDS[fn]
    if not isinstance(adj, SparseTensor) or (adj2 is not None and not isinstance(adj2, SparseTensor)):
        raise ValueError(f"{fn}: adj (and adj2) must be SparseTensor objects")
    if adj.has_value() or (adj2 is not None and not adj2.rows_on_demand() and adj2.has_value()):
        raise ValueError(f"{fn}: a valued adjacency cannot {verb} (pattern matrices only)")
    n, m = adj.sparse_sizes()
    if n != m:
        raise ValueError(f"{fn}: adj is {n} x {m}, not square")
    if adj2 is not None and tuple(adj2.sparse_sizes()) != (n, n):
        raise ValueError(f"{fn}: adj2 is {tuple(adj2.sparse_sizes())}, adj {(n, n)}")
    if not isinstance(edges, Tensor) or edges.dtype != torch.int64 or edges.dim() != 2 or edges.shape[0] != 2:
        raise ValueError(f"{fn}: {arg} must be an int64 tensor of shape [2, E]")
    if edges.device != adj.device():
        raise ValueError(f"{fn}: {arg} on {edges.device}, adj on {adj.device()}")
    return n


def _retire(adj2: SparseTensor) -> None:
    """A donated A² gives up everything it held: any later use fails instead of reading updated bits through a stale thunk."""
    adj2._lazy = adj2._done = None
    adj2._rowptr_v = None
    adj2._col_v = adj2._col_thunk = None
    adj2._bitmap = None
    adj2._row_cache = adj2._maxdeg = adj2._nds = None
    adj2._ready = {}


def _cpu_pair(row: Tensor, col: Tensor, n: int, with_product: bool):
    """(adj_new, adj_new @ adj_new or None) from the sorted, duplicate-free entries of the new adjacency, in plain torch."""
    adj_new = SparseTensor(row=row, col=col, sparse_sizes=(n, n), is_sorted=True, trust_data=True)
    if not with_product:
        return adj_new, None
    a = torch.sparse_coo_tensor(torch.stack([row, col]), torch.ones(row.numel(), dtype=torch.float64), (n, n))
    with warnings.catch_warnings():                          # (torch announces its sparse CSR support as beta on first use)
        warnings.simplefilter("ignore", UserWarning)
        p = torch.sparse.mm(a, a).coalesce()                 # walk counts (<= n: exact), every stored entry positive
    pr, pc = p.indices()
    return adj_new, SparseTensor(row=pr, col=pc, sparse_sizes=(n, n), is_sorted=True, trust_data=True)


def _delta_csr(fn: str, edges: Tensor, n: int, undirected: bool) -> Tuple[Tensor, Tensor]:
    """D: the entries ``edges`` names, alone, as a CSR (with their transposes when ``undirected``) — A is never sorted again."""
    try:
        return ops.coo_to_csr(edges[0], edges[1], n, n, symmetrize=undirected, dedupe=True)
    except IndexError as e:
        raise ValueError(f"{fn}: {_WORDS[fn][0]} holds an index out of range for the adjacency") from e


def _bit_row_product(adj2: SparseTensor, bits: Tensor, changed: Tensor, sign: int, n: int) -> SparseTensor:
    """The product whose bit rows are ``bits`` (those of ``adj2``, updated): its row lengths are ``adj2``'s plus ``sign`` times
    ``changed`` (int32 [n], the bits turned on or off per row), its columns are read off the bits when somebody asks."""
    rp2 = adj2._rowptr
    rowptr2 = ops.scan_i32(torch.add((rp2[1:] - rp2[:-1]).to(torch.int32), changed, alpha=sign))
    adj2_new = SparseTensor._deferred_product(rowptr2, lambda: ops.bitrows_to_cols(bits, n, rowptr2), bits, (n, n))
    adj2_new._published("bitmap")
    return adj2_new


def _cpu_route(route, adj: SparseTensor, edges: Tensor, adj2: Optional[SparseTensor], n: int, undirected: bool, donate: bool):
    """CPU tensors: the whole job in plain torch by ``route``; a donated ``adj2`` is retired as on the device."""
    out = route(adj, edges, adj2, n, undirected)
    if donate and adj2 is not None:
        _retire(adj2)
    return out


def _insert_cpu(adj: SparseTensor, new_edges: Tensor, adj2: Optional[SparseTensor], n: int, undirected: bool):
    r, c = new_edges[0], new_edges[1]
    if new_edges.numel() and (int(new_edges.min()) < 0 or int(new_edges.max()) >= n):
        raise ValueError("insert_edges: new_edges holds an index out of range for the adjacency")
    keys = [adj._row64() * n + adj._col.to(torch.int64), r * n + c]
    if undirected:
        keys.append(c * n + r)
    key = torch.unique(torch.cat(keys))
    row, col = torch.div(key, max(n, 1), rounding_mode="floor"), key % max(n, 1)
    return _cpu_pair(row, col, n, adj2 is not None)


def insert_edges(adj: SparseTensor, new_edges: Tensor, adj2: Optional[SparseTensor] = None, *, undirected: bool = True,
                 donate: bool = False) -> Tuple[SparseTensor, Optional[SparseTensor]]:
    """``(adj_new, adj2_new)``: the pattern adjacency with ``new_edges`` (int64 ``[2, E]``, ``E == 0`` allowed) inserted, and
    — where ``adj2 = adj @ adj`` is given — the product of the new adjacency with itself.

    ``adj_new`` equals, bit for bit in row pointers and (sorted, duplicate-free int32) columns, what
    ``SparseTensor.from_edge_index(cat(adj edges, new_edges))`` gives, followed by ``to_symmetric()`` when ``undirected`` (the
    transposed entries join; ``adj`` must itself be symmetric, which is not checked) and by ``coalesce()`` otherwise.
    ``adj2_new`` is indistinguishable from ``adj_new @ adj_new`` formed from scratch: bit rows, row pointers, ``nnz()`` and column
    ids.  Self loops are inserted as given; duplicates within ``new_edges`` and entries ``adj`` already has are harmless.

    ``adj`` is never modified.  ``adj2`` stays valid under ``donate=False`` (its bit rows are cloned); ``donate=True`` updates
    them in place, hands them to ``adj2_new`` and empties the old object, whose every later use fails.  A product with rows
    on demand is completed first.  A product without bit rows is updated as a CSR: the thin products D·A' and A'·D from the
    A·B pattern kernels, united into it row by row.  Cached per-matrix data (bit rows of A, degree sums, longest row, the
    transpose) is not carried over: the new objects rebuild it lazily.

    Raises ``ValueError`` for a valued adjacency, for ``new_edges`` of another type or shape and for an index outside the
    matrix (one host read of the device flag of ``ocn_coo_to_csr``).  CPU tensors take a plain torch route of the same
    meaning (concatenate and coalesce; ``torch.sparse.mm``)."""
    n = _check_args("insert_edges", adj, new_edges, adj2)
    if not new_edges.is_cuda:
        return _cpu_route(_insert_cpu, adj, new_edges, adj2, n, undirected, donate)
    rowptrD, colD = _delta_csr("insert_edges", new_edges, n, undirected)
    rowptrN, colN = ops.csr_union(adj._rowptr, adj._col, rowptrD, colD)
    adj_new = SparseTensor(rowptr=rowptrN, col=colN, sparse_sizes=(n, n))
    if adj2 is None:
        return adj_new, None

    bits = adj2.product_bit_rows()                           # (completes a product with rows on demand)
    if bits is not None:
        if not donate:
            bits = bits.clone()
        at = adj_new if undirected else adj_new.t()
        added = ops.bitrows_insert(rowptrN, colN, at._rowptr, at._col, rowptrD, colD, bits)
        adj2_new = _bit_row_product(adj2, bits, added, 1, n)
    else:
        # CSR only: D·A' and A'·D are products with few non-empty rows / few columns — the existing pattern kernels, no bit rows
        p1 = ops.spgemm_pattern(rowptrD, colD, rowptrN, colN, n, want_bitmap=False)
        p2 = ops.spgemm_pattern(rowptrN, colN, rowptrD, colD, n, want_bitmap=False)
        rp, col = ops.csr_union(adj2._rowptr, adj2._col, p1[0], p1[1])
        rp, col = ops.csr_union(rp, col, p2[0], p2[1])
        adj2_new = SparseTensor(rowptr=rp, col=col, sparse_sizes=(n, n))
    if donate:
        _retire(adj2)
    return adj_new, adj2_new


def _remove_cpu(adj: SparseTensor, edges: Tensor, adj2: Optional[SparseTensor], n: int, undirected: bool):
    r, c = edges[0], edges[1]
    if edges.numel() and (int(edges.min()) < 0 or int(edges.max()) >= n):
        raise ValueError("remove_edges: edges holds an index out of range for the adjacency")
    row, col = adj._row64(), adj._col.to(torch.int64)
    gone = torch.cat([r * n + c, c * n + r]) if undirected else r * n + c
    keep = ~torch.isin(row * n + col, gone)
    return _cpu_pair(row[keep], col[keep], n, adj2 is not None)


def remove_edges(adj: SparseTensor, edges: Tensor, adj2: Optional[SparseTensor] = None, *, undirected: bool = True,
                 donate: bool = False) -> Tuple[SparseTensor, Optional[SparseTensor]]:
    """``(adj_new, adj2_new)``: the pattern adjacency without the entries ``edges`` names (int64 ``[2, E]``, ``E == 0`` allowed),
    and — where ``adj2 = adj @ adj`` is given — the product of the new adjacency with itself.

    ``adj_new`` equals, bit for bit in row pointers and (sorted, duplicate-free int32) columns, ``SparseTensor.from_edge_index``
    of the entries of ``adj`` that ``edges`` does not name — nor, when ``undirected``, names transposed (``adj`` must itself be
    symmetric, which is not checked).  ``adj2_new`` is indistinguishable from ``adj_new @ adj_new`` formed from scratch: bit rows,
    row pointers, ``nnz()`` and column ids.  Entries the graph never had, duplicates within ``edges`` and self loops are harmless.

    ``adj`` is never modified.  ``adj2`` stays valid under ``donate=False`` (its bit rows are cloned); ``donate=True`` updates
    them in place, hands them to ``adj2_new`` and empties the old object, whose every later use fails.  A product with rows
    on demand is NOT completed: the result is a product of the new adjacency with rows on demand again.  A product without
    bit rows is a REBUILD: it is formed again from ``adj_new`` with the A·B pattern kernels (only the adjacency is spared its
    sort; a CSR splice is not offered).  Cached per-matrix data (bit rows of A, degree sums, longest row, the transpose) is not
    carried over: the new objects rebuild it lazily.

    Raises ``ValueError`` for a valued adjacency, for ``edges`` of another type or shape and for an index outside the matrix
    (one host read of the device flag of ``ocn_coo_to_csr``).  CPU tensors take a plain torch route of the same meaning
    (``torch.isin`` on the entry keys; ``torch.sparse.mm``)."""
    n = _check_args("remove_edges", adj, edges, adj2)
    if not edges.is_cuda:
        return _cpu_route(_remove_cpu, adj, edges, adj2, n, undirected, donate)
    rowptrD, colD = _delta_csr("remove_edges", edges, n, undirected)
    rowptrN, colN = ops.csr_minus(adj._rowptr, adj._col, rowptrD, colD)
    adj_new = SparseTensor(rowptr=rowptrN, col=colN, sparse_sizes=(n, n))
    if adj2 is None:
        return adj_new, None

    if adj2.rows_on_demand():                                # nothing of it exists yet: nothing to update
        adj2_new = SparseTensor._lazy_product(adj_new, adj_new)
    elif (bits := adj2.product_bit_rows()) is not None:
        if not donate:
            bits = bits.clone()
        at0, at = (adj, adj_new) if undirected else (adj.t(), adj_new.t())
        removed = ops.bitrows_remove(adj._rowptr, adj._col, at0._rowptr, at0._col, rowptrN, colN, at._rowptr, at._col,
                                     rowptrD, colD, bits)
        adj2_new = _bit_row_product(adj2, bits, removed, -1, n)
    else:                                                    # CSR only: formed again from A' (a rebuild of the product)
        rp, col, _ = ops.spgemm_pattern(rowptrN, colN, rowptrN, colN, n, want_bitmap=False)
        adj2_new = SparseTensor(rowptr=rp, col=col, sparse_sizes=(n, n))
    if donate:
        _retire(adj2)
    return adj_new, adj2_new
