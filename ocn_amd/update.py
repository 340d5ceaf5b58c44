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

The third resident object, the encoder output ``h``, follows through ``EncoderState``: an L-layer message-passing encoder
can change only the rows inside the L-hop ball of the updated rows, and every eval-mode op of the encoder works a row at a
time in a fixed order.  ``EncoderState.refresh`` recomputes those rows alone, layer by layer (``ocn_spmm_csr_rows`` over the
row lists of ``ocn_rows_neighbourhood``), and ends with ``h`` bit-equal to a full pass over the new adjacency.

The 3-hop predictor cn6 needs nothing more: the pair ``(adj, adj2)`` these functions return is all it reads — its cn3 pass
(``utils.adjoverlap_3hop``, ``ocn_cn3_flags``) decides A³[j, k] from the rows of A and the bit rows of A², so no third matrix
is kept beside them that could go stale on the first accepted link.

Valued adjacencies, changed node features, training-mode refresh and more than one GPU are out of scope.
"""
from __future__ import annotations

import warnings
from typing import List, Optional, Tuple

import torch
import torch.nn as nn
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
    adj2._square_of = None                                   # (and is no longer anybody's certified product)
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


# ------------------------------------------------------------------------------------------
# the encoder output after an edge update: only the rows that can have changed
# ------------------------------------------------------------------------------------------
def _check_refresh_args(fn: str, adj: SparseTensor, edges: Tensor, n: Optional[int] = None) -> int:
    if not isinstance(adj, SparseTensor):
        raise ValueError(f"{fn}: adj must be a SparseTensor")
    if adj.has_value():
        raise ValueError(f"{fn}: a valued adjacency is not supported (pattern matrices only)")
    rows, cols = adj.sparse_sizes()
    if rows != cols or (n is not None and rows != n):
        raise ValueError(f"{fn}: adj is {rows} x {cols}, the state holds {rows if n is None else n} nodes")
    if not isinstance(edges, Tensor) or edges.dtype != torch.int64 or edges.dim() != 2 or edges.shape[0] != 2:
        raise ValueError(f"{fn}: edges must be an int64 tensor of shape [2, E]")
    if edges.device != adj.device():
        raise ValueError(f"{fn}: edges on {edges.device}, adj on {adj.device()}")
    if edges.numel() and (int(edges.min()) < 0 or int(edges.max()) >= rows):
        raise ValueError(f"{fn}: edges holds an index out of range for the adjacency")
    return rows


def affected_rows(adj_new: SparseTensor, edges: Tensor, hops: int, normalised: bool, undirected: bool = True) -> List[Tensor]:
    """``[R_1, ..., R_hops]``: the rows of each layer's output that the update ``edges`` (the ``[2, E]`` tensor given to
    ``insert_edges`` / ``remove_edges``) can have changed, sorted int64 ids — in plain torch, on the device of its operands.

    D = the endpoints of ``edges``.  N'(S) = S's neighbourhood in the NEW adjacency: the rows that read a column of S (rows of
    the transpose; of ``adj_new`` itself when ``undirected``, which takes it to be symmetric).  D+ = D U N'(D) for the
    degree-normalised convolutions (``normalised``: a changed degree changes ``pre[k]`` for every reader of k), D+ = D
    otherwise.  R_1 = D+, R_l = D+ U R_(l-1) U N'(R_(l-1)).  A superset is harmless, so edges the graph already had (or never
    had) need no special case.  ``EncoderState.refresh`` forms the same lists on the device (``ocn_rows_neighbourhood``)."""
    n = _check_refresh_args("affected_rows", adj_new, edges)
    at = adj_new if undirected else adj_new.t()
    rp, col = at._rowptr, at._col.to(torch.int64)
    deg = rp[1:] - rp[:-1]

    def closed(mask: Tensor) -> Tensor:
        out = mask.clone()
        out[col[torch.repeat_interleave(mask, deg)]] = True
        return out

    d = torch.zeros(n, dtype=torch.bool, device=edges.device)
    d[edges.reshape(-1)] = True
    cur = closed(d) if normalised else d
    sets = []
    for _ in range(int(hops)):
        sets.append(torch.nonzero(cur).reshape(-1))
        cur = closed(cur)
    return sets


class _LayerPlan:
    """One conv layer as the ops its eval forward runs: ``lin_first`` (GCNConv: Linear, then aggregate), the aggregation's
    arguments (``norm``: "" none, "pre" = pre only, "prepost" = pre and post), ``bias``, ``lin_after`` (PureConv2/3 with
    ``use_lin``: aggregate, then Linear + ReLU)."""

    def __init__(self, lin_first=None, norm="", kw=None, bias=None, lin_after=None):
        self.lin_first, self.norm, self.kw, self.bias, self.lin_after = lin_first, norm, kw or {}, bias, lin_after

    def spmm_kw(self, dinv: Optional[Tensor]) -> dict:
        kw = dict(self.kw)
        if self.norm:
            kw["pre"] = dinv
        if self.norm == "prepost":
            kw["post"] = dinv
        return kw


def _plan_of(conv) -> Optional[_LayerPlan]:
    """The plan of a conv of ``convdict`` / ``convdict2`` / ``convdict3``; None for anything else (such a layer is only ever run
    whole, through the module itself)."""
    from .model import GCNConv, PureConv, PureConv2
    if type(conv) is PureConv and isinstance(conv.lin, nn.Identity):
        if conv.aggr in ("mean", "max", "sum"):
            return _LayerPlan(kw=dict(mode=conv.aggr))
        if conv.aggr == "gcn":
            return _LayerPlan(norm="prepost", kw=dict(mode="sum", edge_scale=False, self_mode=1))
    elif type(conv) is GCNConv:
        if conv.normalize:
            return _LayerPlan(lin_first=conv.lin, norm="pre", bias=conv.bias,
                              kw=dict(mode="sum", edge_scale=True, self_mode=2 if conv.add_self_loops else 0))
        return _LayerPlan(lin_first=conv.lin, kw=dict(mode=conv.aggr), bias=conv.bias)
    elif isinstance(conv, PureConv2) and conv.aggr in ("mean", "max", "sum", "gcn"):
        after = None
        if isinstance(conv.lin, nn.Sequential):
            after = conv.lin[0]
        elif not isinstance(conv.lin, nn.Identity):
            return None
        if conv.aggr == "gcn":
            return _LayerPlan(norm="pre", kw=dict(mode="sum", edge_scale=True), lin_after=after)
        return _LayerPlan(kw=dict(mode=conv.aggr), lin_after=after)
    return None


def _row_exact_linear(lin: nn.Linear) -> bool:
    """Does ``_lin_eval`` take this Linear to the library's MFMA kernel, which computes every output row on its own (the same
    bits whatever the row count)?  torch's own GEMM, the other route, picks its kernel by the shape."""
    w = lin.weight
    return bool(ops.fast_linear and w.is_cuda and w.shape[0] in ops.LINEAR_WIDTHS and w.shape[1] % 16 == 0)


def _row_exact_tail(tail) -> bool:
    """Is this layer tail (``_Encoder.lins[i]``) row-wise whatever the row count: nothing, or LayerNorm at a width of
    ``ops.rows_ln_relu`` and / or ReLU?"""
    if not isinstance(tail, nn.Sequential):
        return isinstance(tail, (nn.Identity, nn.Dropout))
    for m in tail:
        if isinstance(m, (nn.Dropout, nn.Identity, nn.ReLU)):
            continue
        if not (isinstance(m, nn.LayerNorm) and m.elementwise_affine and len(m.normalized_shape) == 1
                and m.normalized_shape[0] in ops.LN_WIDTHS):
            return False
    return True


class EncoderState:
    """The output ``h = model(x, adj)`` of a ``GCN`` / ``GCN2`` / ``GCN3`` encoder kept current under edge updates.

        state = EncoderState(model, x, adj)            # eval mode, no_grad: one full pass; state.h
        adj, adj2 = insert_edges(adj, new, adj2, donate=True)
        rows = state.refresh(adj, new)                 # state.h is now bit-equal to model(x, adj)

    The constructor walks the eval path of ``_Encoder.forward`` layer by layer with the forward's own ops and keeps ``xemb(x)``,
    every layer output ``x_l`` and — for convolutions that apply their Linear before they aggregate (``GCNConv``) — that
    Linear's output ``Z_l``: at most 2 L + 1 buffers of N x H fp32 for L layers (L + 1 without a Linear-first conv; 7 buffers =
    1.7 GB at the collab shape, 3 layers, H = 256, N = 235 868).  ``state.h`` equals ``model(x, adj)`` bit for bit.

    ``refresh(adj_new, edges)`` recomputes, layer l, the rows R_l of ``affected_rows`` only: the Linear of a Linear-first conv
    on the rows R_(l-1) of its input, ``ops.spmm_csr_rows`` over R_l, bias / Linear + ReLU / LayerNorm + ReLU / residual on the
    compact rows, ``index_copy_`` into ``x_l``.  Every one of these ops computes a row on its own and in a fixed order, so the
    rows written carry the bits of a full pass, and the rows not written cannot have changed.  JumpingKnowledge is mixed again
    over all rows with the forward's own expression.  ``state.h`` is updated IN PLACE (a new tensor under JumpingKnowledge).

    The full layer walk runs instead (``state.route == "full"``; ``"rows"`` otherwise), as exact, when (a) a layer needs an op
    whose bits may depend on the row count — a conv Linear outside ``ops.linear_ok`` (torch's GEMM), a LayerNorm width outside
    ``ops.LN_WIDTHS``, a conv that is not one of the three ``convdict``s — or (b) the listed rows hold more than
    ``ops.refresh_full_share`` of the adjacency entries the full walk reads.

    ``state.row_sets`` = [R_1 .. R_L] of the last refresh.  Raises ``ValueError`` for a model in training mode or with grad
    enabled, a valued adjacency, an adjacency of another size, ``edges`` of another type or shape or with an index out of
    range.  CPU tensors: the encoder has no CPU path (the library's usual error)."""

    def __init__(self, model, x: Tensor, adj: SparseTensor):
        self.model = model
        self._mode_check("EncoderState")
        if not isinstance(adj, SparseTensor) or adj.has_value():
            raise ValueError("EncoderState: adj must be a SparseTensor without values (pattern matrices only)")
        from .model import _seq_eval
        if torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2:
            x0 = _seq_eval(model.xemb, x)                    # (the forward's own condition and route)
        else:
            x0 = model.xemb(x)
        self.n = int(x0.shape[0])
        if tuple(adj.sparse_sizes()) != (self.n, self.n):
            raise ValueError(f"EncoderState: adj is {tuple(adj.sparse_sizes())}, x has {self.n} rows")
        self.convs = list(getattr(model, "convs", ()))
        self.plans = [_plan_of(c) for c in self.convs]
        self.normalised = any(p is not None and p.norm for p in self.plans)
        self.xs: List[Tensor] = [x0]                         # x_0 = xemb(x), then every layer output
        self.zs: List[Optional[Tensor]] = [None]             # Z_l of a Linear-first conv (index l), else None
        self.row_sets: List[Tensor] = []
        self.route = "full"
        self._full(adj)

    # ---- the layer ops, shared by the full walk and the row walk ------------------------------------------------------------
    def _mode_check(self, fn: str) -> None:
        if self.model.training or torch.is_grad_enabled():
            raise ValueError(f"{fn}: the encoder must be in eval mode under torch.no_grad()")

    def _after_aggregate(self, i: int, y: Tensor, x_in: Tensor) -> Tensor:
        """Bias, Linear + ReLU, the layer tail and the residual of layer i on the rows ``y`` (all of them, or compact ones)
        whose layer inputs are ``x_in``: every op row-wise."""
        from .model import _lin_eval, _seq_eval
        plan, tail = self.plans[i], self.model.lins[i]
        if plan is not None and plan.bias is not None:
            y = y + plan.bias
        if plan is not None and plan.lin_after is not None:
            y = _lin_eval(plan.lin_after, y, relu=True)
        if isinstance(tail, nn.Sequential) and y.is_cuda and y.dim() == 2 and y.dtype == torch.float32 and y.is_contiguous():
            y = _seq_eval(tail, y)
        else:
            y = tail(y)
        return y + x_in if (self.model.res and y.shape[-1] == x_in.shape[-1]) else y

    def _finish(self) -> None:
        m = self.model
        if getattr(m, "jk", False) and len(self.xs) > 1:
            self.h = torch.sum(torch.stack(self.xs[1:], dim=0) * m.jkparams.reshape(-1, 1, 1), dim=0)
        else:
            self.h = self.xs[-1]

    def _full(self, adj: SparseTensor) -> None:
        from .model import _lin_eval
        x = self.xs[0]
        self.xs, self.zs = [x], [None]
        dinv = ops.deg_rsqrt(adj._rowptr, 1.0) if self.normalised else None
        for i, (conv, plan) in enumerate(zip(self.convs, self.plans)):
            z = None
            if plan is None:                                 # a conv of another kind: the module itself, whole
                x = self._after_aggregate(i, conv(x, adj), x)
            else:
                if plan.lin_first is not None:
                    z = src = _lin_eval(plan.lin_first, x).contiguous()
                else:
                    src = x.contiguous()
                y = ops.spmm_csr(adj._rowptr, adj._col, src, **plan.spmm_kw(dinv))
                x = self._after_aggregate(i, y, x)
            self.xs.append(x)
            self.zs.append(z)
        self._finish()

    # ---- refresh ------------------------------------------------------------------------------------------------------------
    def _rows_exact(self) -> bool:
        x0 = self.xs[0]
        if not (x0.is_cuda and x0.dtype == torch.float32 and x0.dim() == 2 and x0.is_contiguous()):
            return False
        for plan, tail in zip(self.plans, self.model.lins):
            if plan is None or not _row_exact_tail(tail):
                return False
            for lin in (plan.lin_first, plan.lin_after):
                if lin is not None and not _row_exact_linear(lin):
                    return False
        return True

    def _device_row_sets(self, adj_new: SparseTensor, edges: Tensor, undirected: bool) -> List[Tensor]:
        """[R_1 .. R_L] of ``affected_rows``, on the device: one bit row that only grows (R_(l-1) is part of R_l), each step the
        closed neighbourhood of the last list."""
        at = adj_new if undirected else adj_new.t()
        bits = torch.zeros((self.n + 31) // 32, dtype=torch.int32, device=edges.device)
        cur = torch.unique(edges.reshape(-1))
        if self.normalised:
            cur = ops.bits_to_list(ops.rows_neighbourhood(at._rowptr, at._col, cur, bits), self.n)
        sets = [cur]
        for _ in range(len(self.convs) - 1):
            cur = ops.bits_to_list(ops.rows_neighbourhood(at._rowptr, at._col, cur, bits), self.n)
            sets.append(cur)
        return sets

    def refresh(self, adj_new: SparseTensor, edges: Tensor, *, undirected: bool = True) -> Tensor:
        """Bring ``state.h`` to ``model(x, adj_new)``, bit for bit, after ``insert_edges`` / ``remove_edges`` of ``edges`` gave
        ``adj_new``; ``undirected`` as there.  Returns the sorted int64 ids of the rows of ``h`` that were recomputed (every
        row that changed is among them): the sources whose recommendations are stale.  ``E == 0`` returns an empty list and
        leaves ``h`` alone."""
        self._mode_check("EncoderState.refresh")
        _check_refresh_args("EncoderState.refresh", adj_new, edges, self.n)
        L = len(self.convs)
        if edges.numel() == 0 or L == 0:
            self.row_sets = [edges.new_empty(0) for _ in range(L)]
            return edges.new_empty(0)
        self.row_sets = sets = self._device_row_sets(adj_new, edges, undirected)
        rows_ok = self._rows_exact()
        if rows_ok:
            rp = adj_new._rowptr
            deg = rp[1:] - rp[:-1]
            read = sum(int(deg[r].sum()) for r in sets)      # (one host read per layer, beside the one for each list's size)
            rows_ok = read <= ops.refresh_full_share * L * max(adj_new.nnz(), 1)
        if not rows_ok:
            self.route = "full"
            self._full(adj_new)
            return sets[-1]
        self.route = "rows"
        from .model import _lin_eval
        dinv = ops.deg_rsqrt(adj_new._rowptr, 1.0) if self.normalised else None      # all N rows: one trivial pass
        prev = edges.new_empty(0)
        for i, plan in enumerate(self.plans):
            R, x_in = sets[i], self.xs[i]
            if plan.lin_first is not None:
                if prev.numel():
                    self.zs[i + 1].index_copy_(0, prev, _lin_eval(plan.lin_first, x_in[prev]).contiguous())
                src = self.zs[i + 1]
            else:
                src = x_in
            y = ops.spmm_csr_rows(adj_new._rowptr, adj_new._col, src, R, **plan.spmm_kw(dinv))
            self.xs[i + 1].index_copy_(0, R, self._after_aggregate(i, y, x_in[R]))
            prev = R
        self._finish()
        return sets[-1]
