"""Structured negative sampling on the device: negatives that are guaranteed not to be links, for the training and the
evaluation loops.

``torch.randint`` negatives can be existing links — false negatives depress Hits@K and MRR in an evaluation set and teach a
model to score real links low in a training set — and a rejection sampler pays a sort of every stored edge and a host sync per
round.  The samplers here read the CSR the scoring loops read and need neither: for a row ``s`` of a square ``known`` matrix
the excluded set is ``X(s) = known[s, :] ∪ {s}`` (``s`` is counted once, whether or not the row stores it), its complement
``C(s)`` has ``m_s = n − |X(s)|`` members, and a sample is the ``r``-th smallest member of ``C(s)`` for
``r = floor(u · m_s / 2^64)``, ``u`` one 64-bit word of Philox4x32-10 — a binary search on the row (``r + i`` with ``i`` the
first index where ``x_i − i > r``), so a hub row or a dense graph costs what a sparse one does.

Contract (include/ocn_hip.h, ``ocn_sample_complement_*``):

* every sample is exactly uniform over its complement (the bias of the multiply-high is below ``m / 2^64``);
* samples are drawn WITH replacement: duplicates are possible, among the negatives of one source as among the pairs;
* a sample is fixed, bit for bit, by ``(seed, its own index, known)``: the key is ``(seed & 0xffffffff, seed >> 32)``, the
  counter of per-source sample ``j`` of query ``q`` is ``(j, q & 0xffffffff, q >> 32, 2)`` and that of pair sample ``t`` is
  ``(t & 0xffffffff, t >> 32, 0, 1)``.  It does not depend on the device, on the launch, on ``per``, on the number of
  sources or on ``num``: a prefix of a longer call is the shorter call, and ``first`` continues a split produced in chunks.

Hard negatives (``two_hop_negative_targets``, ``two_hop_negative_edges``; ``ocn_sample_two_hop``).  The uniform samplers above
almost never hit a pair with a common neighbour — a source has a few hundred nodes within two hops among all the others —
while ``recommend_links`` and ``rank_links`` order exactly such pairs.  These two draw from the set that is served: the
candidates ``recommend.two_hop_candidates(adj, None, sources, known)`` lists for a source, uniformly and with replacement,
under the same contract — a sample is fixed by ``(seed, its own index, adj, known)``, with Philox counter streams of its own
(word 3 = 3 and 4), so it is independent of the uniform draw for the same index.  The candidates are never materialised: the
kernel expands a source's neighbourhood into the LDS bitmap of the 2-hop passes and picks the ``r``-th set bit there, so the
memory is that of the samples and there is no size sync.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import ops
from .sparse import SparseTensor


def _square(known: SparseTensor) -> int:
    n = known.size(0)
    if known.size(1) != n:
        raise ValueError(f"negative sampling needs a square known matrix, got {tuple(known.sparse_sizes())}")
    return n


def complement_ptr(known: SparseTensor) -> Tuple[Tensor, int]:
    """(``cptr`` int64 [n + 1], ``M``): the prefix of the complement sizes ``m_s`` of every row of ``known`` on its device, and
    their total ``M = cptr[n]``, the number of ordered non-edge, non-self pairs.  Cached on the adjacency, as
    ``heuristics.node_table`` is, behind an event that the streams of later readers wait for; reading the total costs one
    host sync per adjacency."""
    _square(known)
    cached = getattr(known, "_complement_ptr", None)
    if cached is not None:
        known._await("complement_ptr")
        return cached
    cptr = ops.scan_i32(ops.complement_count(known._rowptr, known._col))
    total = ops._total(cptr[-1])
    known._complement_ptr = (cptr, total)
    known._published("complement_ptr")
    return known._complement_ptr


def negative_targets(known: SparseTensor, sources: Tensor, per: int, seed: int, first: int = 0) -> Tensor:
    """``per`` negative targets for every source: int64 [Q, per], the ``target_neg`` argument of
    ``pipeline.score_mrr_split`` and the layout of ogbl-citation2's ``target_node_neg``.

    ``out[q, j]`` is uniform over the nodes that are neither ``sources[q]`` nor stored in row ``sources[q]`` of ``known``
    (pass ``full_adj_t`` to exclude the validation edges as well), drawn with replacement: a source's negatives may repeat.
    It is -1 where a source is linked to every other node.  ``sources``: 1-d int64 node ids, bounds-checked (one host sync);
    a source may repeat, and gets other samples at another position.  ``out[q, j]`` is fixed by
    ``(seed, first + q, j, known)``: ``per`` and the number of sources do not enter, so ``out[:, :k]`` is the call with
    ``per = k``, and a long split produced in chunks with ``first`` = the number of sources before the chunk equals the
    one-shot call."""
    _square(known)
    if not isinstance(sources, Tensor) or sources.dim() != 1 or sources.dtype != torch.int64:
        raise ValueError("sources must be a 1-d int64 tensor of node ids")
    if int(per) < 1:
        raise ValueError(f"per must be at least 1, got {per}")
    return ops.sample_complement_rows(known._rowptr, known._col, sources.contiguous(), per, seed, first)


def negative_edges(known: SparseTensor, num: int, seed: int, first: int = 0) -> Tensor:
    """``num`` negative pairs: int64 [2, num], sources then targets — the layout of ``tar_ei``, what the training loops
    index by batch.

    Every pair is uniform over the ordered pairs ``(s, c)`` with ``c != s`` and ``c`` not stored in row ``s`` of ``known``
    (the default semantics of PyG's ``negative_sampling`` for a directed pair), drawn with replacement: pairs may repeat.
    Pair ``t`` is fixed by ``(seed, first + t, known)``: a prefix of a longer call is the shorter call, ``first`` continues
    one.  The prefix of the complement sizes is built once per adjacency (``complement_ptr``: one host sync).  Raises
    ``ValueError`` when the graph has no non-edge."""
    _square(known)
    if int(num) < 0:
        raise ValueError(f"num must not be negative, got {num}")
    cptr, total = complement_ptr(known)
    if total == 0:
        raise ValueError("negative_edges: every ordered pair of distinct nodes is a link of known — there is no non-edge to draw")
    return ops.sample_complement_pairs(known._rowptr, known._col, cptr, num, seed, first)


def _check_fallback(fallback) -> None:
    if fallback not in ("uniform", None):
        raise ValueError(f"fallback must be 'uniform' or None, got {fallback!r}")


def _two_hop_operands(adj: SparseTensor, known: Optional[SparseTensor]) -> Tuple[SparseTensor, int]:
    known = adj if known is None else known
    n = adj.size(0)
    for name, m in (("adj", adj), ("known", known)):
        if tuple(m.sparse_sizes()) != (n, n):
            raise ValueError(f"{name} is {tuple(m.sparse_sizes())}, expected the square size ({n}, {n}) of adj")
    return known, n


def two_hop_negative_targets(adj: SparseTensor, sources: Tensor, per: int, seed: int, known: Optional[SparseTensor] = None,
                             first: int = 0, fallback: Optional[str] = "uniform") -> Tensor:
    """``per`` hard negative targets for every source: int64 [Q, per], the layout of ``negative_targets`` (``target_neg`` of
    ``pipeline.score_mrr_split``).

    ``out[q, j]`` is uniform, with replacement, over exactly the targets ``recommend.two_hop_candidates(adj, None, sources,
    known)`` lists for ``sources[q]``: within two hops in ``adj``, not the source, not stored in its row of ``known`` (``adj``
    by default; pass ``full_adj_t`` to exclude the validation edges as well).  It is fixed by ``(seed, first + q, j, adj,
    known)``: ``out[:, :k]`` is the call with ``per = k``, and ``first`` = the number of sources before a chunk continues a
    split produced in chunks.  A source may repeat and gets other samples at another position.

    A source without a candidate (no neighbour, or every node within two hops is known): ``fallback="uniform"`` gives its
    slots, bit for bit, the samples of ``negative_targets(known, sources, per, seed, first)`` — computed for every slot and
    selected on the device, no sync; ``fallback=None`` leaves -1.  A source linked to every other node has no non-link at all:
    its slots stay -1 either way.  ``sources``: 1-d int64 node ids, bounds-checked (one host sync)."""
    known, n = _two_hop_operands(adj, known)
    _check_fallback(fallback)
    if not isinstance(sources, Tensor) or sources.dim() != 1 or sources.dtype != torch.int64:
        raise ValueError("sources must be a 1-d int64 tensor of node ids")
    per = int(per)
    if per < 1:
        raise ValueError(f"per must be at least 1, got {per}")
    sources = sources.contiguous()
    Q = sources.numel()
    with ops.prevalidated(sources, sources, n, n):
        sptr = torch.arange(Q + 1, dtype=torch.int64, device=sources.device) * per
        out = ops.sample_two_hop(adj._rowptr, adj._col, known._rowptr, known._col, sources, sptr, seed, first=first,
                                 total=Q * per).view(Q, per)
        if fallback == "uniform" and Q:
            out = torch.where(out < 0, ops.sample_complement_rows(known._rowptr, known._col, sources, per, seed, first), out)
    return out


def two_hop_negative_edges(adj: SparseTensor, pos_edges: Tensor, seed: int, known: Optional[SparseTensor] = None,
                           first: int = 0, fallback: Optional[str] = "uniform") -> Tensor:
    """The corrupted-target hard negative of every positive: int64 [2, E], sources then targets — the layout of ``tar_ei``
    and of ``negative_edges``.

    ``pos_edges``: int64 [2, E].  Pair ``t`` is ``(pos_edges[0, t], c)`` with ``c`` uniform over the 2-hop candidates of that
    source (as ``two_hop_negative_targets`` defines them) and fixed by ``(seed, first + t, its source, adj, known)``: two
    positives of one source draw independently from the same set, a prefix of a longer list is the shorter call and ``first``
    continues one.  The target is corrupted as given; a caller that wants both ends corrupted passes the flipped pairs too.
    The positives are grouped by source (``torch.unique``: one host sync), so a source is expanded once however many positives
    it has.

    ``fallback``: as for ``two_hop_negative_targets`` — "uniform" gives a pair whose source has no candidate the target
    ``negative_targets(known, pos_edges[0], 1, seed, first)[t, 0]``, None leaves -1; a source linked to every other node keeps -1
    either way."""
    known, n = _two_hop_operands(adj, known)
    _check_fallback(fallback)
    if not isinstance(pos_edges, Tensor) or pos_edges.dim() != 2 or pos_edges.shape[0] != 2 or pos_edges.dtype != torch.int64:
        raise ValueError("pos_edges must be an int64 [2, E] tensor of node ids")
    first = int(first)
    if first < 0:
        raise ValueError(f"first must not be negative, got {first}")
    src = pos_edges[0].contiguous()
    E = src.numel()
    if E == 0:
        return pos_edges.new_empty(2, 0)
    with ops.prevalidated(src, src, n, n):
        rows, inverse, counts = torch.unique(src, return_inverse=True, return_counts=True)
        order = torch.argsort(inverse, stable=True)          # the positions of the positives, grouped by source in `rows` order
        sptr = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=src.device)
        torch.cumsum(counts, 0, out=sptr[1:])
        slots = ops.sample_two_hop(adj._rowptr, adj._col, known._rowptr, known._col, rows, sptr, seed, sid=order + first, total=E)
        tgt = torch.empty_like(slots)
        tgt[order] = slots
        if fallback == "uniform":
            tgt = torch.where(tgt < 0, ops.sample_complement_rows(known._rowptr, known._col, src, 1, seed, first)[:, 0], tgt)
    return torch.stack((src, tgt))
