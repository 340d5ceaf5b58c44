"""Top-K link recommendation: "for these nodes, which links do you predict?".

The scoring loops (``pipeline.score_edges``, ``heuristics.score_edges_heuristic``) take candidate pairs that somebody else
made and return a flat score vector.  This module makes the pairs and picks from the scores, both on the device:

* the natural candidate set of a common-neighbour predictor is the 2-hop neighbourhood of a source that is not yet linked,
  ``pattern(A² row s) \\ (N(s) ∪ {s})`` — any other target has empty ``cn1`` and ``cn2`` and is scored from ``x_i ⊙ x_j``
  alone.  ``two_hop_candidates`` enumerates that set difference row by row (``ops.row_diff_count`` -> ``ops.scan_i32`` ->
  ``ops.row_diff_fill``) straight into the [T, 2] layout the scoring loops take: no dense [Q, N] mask, no host loop;
* where A² is not stored — more columns than the A·A pattern kernel takes, or a product too large to keep, the ppa and
  citation2 shapes — ``adj2=None`` expands the same set from A itself (``ops.two_hop_diff_count`` / ``_fill``) and the
  model scores it on the walk route (``pipeline.score_edges_walk``), as the drivers of those datasets score;
* candidate lists are ragged — under a power law from a handful to tens of thousands per source — so the best ``k`` per
  source are selected segment by segment (``ops.segment_topk``) instead of padding to a [Q, max_len] rectangle;
* retrieve, then rank: the expansion from A that enumerates the candidates of ``s`` visits, for every neighbour ``m`` of ``s``,
  every ``c`` in N(m) — adding the weight of ``m`` to an accumulator of column ``c`` there yields the cn / aa / ra score of
  every candidate in the same pass (``two_hop_scored_candidates``, ``ops.two_hop_sums_fill``).  ``prefilter_candidates`` keeps
  the ``m`` best per source and ``recommend_links(..., prefilter=(kind, m))`` lets the model rank only those.  Opt-in.

Everything runs on one GPU; dealing the sources over several is not built here.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import ops
from .sparse import SparseTensor


def _check_k(k) -> int:
    k = int(k)
    if not 1 <= k <= ops.segment_topk_max_k():
        raise ValueError(f"k must be in 1..{ops.segment_topk_max_k()}, got {k}")
    return k


def two_hop_candidates(adj: SparseTensor, adj2: Optional[SparseTensor], sources: Tensor,
                       known: Optional[SparseTensor] = None) -> Tuple[Tensor, Tensor]:
    """The candidate targets of ``sources`` (int64 [Q]; a source may repeat): for each source ``s``, in source order, the
    columns of row ``s`` of ``adj2`` that are neither ``s`` nor in row ``s`` of ``known``, ascending.  Returns
    (``ptr`` int64 [Q + 1], ``edges`` int64 [T, 2]): ``edges[ptr[q]:ptr[q + 1]]`` are the pairs ``(sources[q], c)`` — the
    layout of ``split_edge[...]['edge']``, which ``pipeline.score_edges`` takes as it is.

    ``adj2``: the project's A² (diagonal included), or any square ``SparseTensor`` of ``adj``'s size.  ``known``: the links
    that are no news, ``adj`` by default; pass ``full_adj_t`` to exclude the validation edges as well.  It must have
    ``adj``'s size.  Reading the CSR of ``adj2`` forces the deferred passes of a product: the fill pass of ``A @ A`` whose
    column ids were left for later, and the counting pass as well of a product formed under autograd.

    ``adj2=None``: row ``s`` of the pattern of A·A is expanded from ``adj`` on the fly (the union of the rows of the
    neighbours of ``s``; ``ops.two_hop_diff_*``) — the same pairs as with the materialised product, for a graph of any size:
    neither the column limit of the A·A pattern kernel nor the memory of A² applies.  It redoes per call the expansion that a
    stored A² holds ready.

    ``sources`` are bounds-checked once (one host sync); the output size costs a second one."""
    known = adj if known is None else known
    if not isinstance(sources, Tensor) or sources.dim() != 1 or sources.dtype != torch.int64:
        raise ValueError("sources must be a 1-d int64 tensor of node ids")
    n = adj.size(0)
    for name, m in (("adj", adj), ("adj2", adj2), ("known", known)):
        if m is not None and tuple(m.sparse_sizes()) != (n, n):
            raise ValueError(f"{name} is {tuple(m.sparse_sizes())}, expected the square size ({n}, {n}) of adj")
    sources = sources.contiguous()
    rpk, colk = known._rowptr, known._col
    with ops.prevalidated(sources, sources, n, n):
        if adj2 is None:
            rpa, cola = adj._rowptr, adj._col
            count = ops.two_hop_diff_count(rpa, cola, rpk, colk, sources, drop_self=True)
            ptr = ops.scan_i32(count)
            edges = ops.two_hop_diff_fill(rpa, cola, rpk, colk, sources, ptr, drop_self=True)
        else:
            rp2, col2 = adj2._rowptr, adj2._col
            count = ops.row_diff_count(rp2, col2, rpk, colk, sources, drop_self=True)
            ptr = ops.scan_i32(count)
            edges = ops.row_diff_fill(rp2, col2, rpk, colk, sources, ptr, drop_self=True)
    return ptr, edges


PATH_SUMS = ("cn", "aa", "ra")       # the heuristics that are a sum of a node weight over the 2-paths s - m - c


def _check_path_sum(kind) -> str:
    if kind not in PATH_SUMS:
        raise ValueError(f"{kind!r} is no path sum: the 2-hop expansion scores one of {PATH_SUMS} "
                         "(jaccard, pa and the 2-hop kinds are not sums over the common neighbours alone)")
    return kind


def two_hop_scored_candidates(adj: SparseTensor, sources: Tensor, kind: str,
                              known: Optional[SparseTensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """``two_hop_candidates(adj, None, sources, known)`` with the heuristic score of every candidate from the same expansion:
    (``ptr`` int64 [Q + 1], ``edges`` int64 [T, 2], ``val`` float32 [T]).  ``kind``: "cn", "aa" or "ra" — the path sums: the
    pass that visits, for every neighbour ``m`` of ``s``, every ``c`` in N(m) adds the weight of ``m`` (1, 1 / log deg,
    1 / deg: ``heuristics.node_table``) to the accumulator of column ``c`` (``ops.two_hop_sums_fill``), in ascending ``m``.
    For a symmetric ``adj``, ``val`` equals ``heuristics.link_heuristics(adj, None, edges.t(), (kind,))[:, 0]`` bit for bit,
    without an intersection per candidate."""
    _check_path_sum(kind)
    known = adj if known is None else known
    if not isinstance(sources, Tensor) or sources.dim() != 1 or sources.dtype != torch.int64:
        raise ValueError("sources must be a 1-d int64 tensor of node ids")
    n = adj.size(0)
    for name, m in (("adj", adj), ("known", known)):
        if tuple(m.sparse_sizes()) != (n, n):
            raise ValueError(f"{name} is {tuple(m.sparse_sizes())}, expected the square size ({n}, {n}) of adj")
    sources = sources.contiguous()
    w = None
    if kind != "cn":
        from .heuristics import node_table
        w = node_table(adj)
    rpa, cola, rpk, colk = adj._rowptr, adj._col, known._rowptr, known._col
    with ops.prevalidated(sources, sources, n, n):
        count = ops.two_hop_diff_count(rpa, cola, rpk, colk, sources, drop_self=True)
        ptr = ops.scan_i32(count)
        edges, val = ops.two_hop_sums_fill(rpa, cola, rpk, colk, sources, ptr, w, 1 if kind == "ra" else 0, drop_self=True)
    return ptr, edges, val


def _check_m(m) -> int:
    m = int(m)
    if not 1 <= m <= ops.segment_topk_max_k():
        raise ValueError(f"m must be in 1..{ops.segment_topk_max_k()}, got {m}")
    return m


def prefilter_candidates(adj: SparseTensor, sources: Tensor, kind: str, m: int,
                         known: Optional[SparseTensor] = None) -> Tuple[Tensor, Tensor]:
    """The ``m`` best candidates of every source by a path-sum heuristic: (``ptr_m`` int64 [Q + 1], ``edges_m`` int64 [T_m, 2])
    in the layout of ``two_hop_candidates``.  Per source the candidates of ``two_hop_scored_candidates`` are ranked in the total
    order of ``segment_topk`` — higher ``val`` first, ties to the lower node id — the first ``m`` are kept (all of them where a
    source has no more) and returned in ASCENDING node id, so that "ties go to the lower node id" still holds for whoever ranks
    the retained list again.  ``1 <= m <= ops.segment_topk_max_k()``.  One host sync more than the candidates cost (the size of
    the retained list)."""
    _check_path_sum(kind)
    m = _check_m(m)
    ptr, edges, val = two_hop_scored_candidates(adj, sources, kind, known)
    Q = ptr.numel() - 1
    ptr_m = torch.zeros_like(ptr)
    torch.cumsum((ptr[1:] - ptr[:-1]).clamp(max=m), 0, out=ptr_m[1:])
    if Q == 0 or edges.shape[0] == 0:
        return ptr_m, edges
    _, pos = ops.segment_topk(val, ptr, m)
    total = int(ptr_m[-1].item())
    # positions into the flat list ascend with (source order, node id); the -1 pads of the short segments sort to the front
    keep = pos.reshape(-1).sort().values[Q * m - total:]
    return ptr_m, edges[keep]


def _check_prefilter(prefilter, k: int) -> Tuple[str, int]:
    if not isinstance(prefilter, (tuple, list)) or len(prefilter) != 2 or not isinstance(prefilter[0], str) \
            or isinstance(prefilter[1], bool) or not isinstance(prefilter[1], int):
        raise ValueError(f"prefilter must be None or (kind, m) with kind one of {PATH_SUMS} and m an int, got {prefilter!r}")
    kind, m = _check_path_sum(prefilter[0]), _check_m(prefilter[1])
    if k > m:
        raise ValueError(f"prefilter keeps m = {m} candidates per source, fewer than k = {k}")
    return kind, m


def segment_topk(scores: Tensor, ptr: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    """The ``k`` best scores of every segment ``scores[ptr[q]:ptr[q + 1]]``, best first: (values float32 [Q, k], positions
    int64 [Q, k] into ``scores``), padded with -inf and -1.  The order is total: the higher score first (+0.0 and -0.0 are
    equal), equal scores by ascending position, NaN after every number and NaNs among themselves by position."""
    return ops.segment_topk(scores, ptr, _check_k(k))


def _select(scores: Tensor, ptr: Tensor, edges: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    val, pos = ops.segment_topk(scores, ptr, k)
    if edges.shape[0] == 0:
        return torch.full_like(pos, -1), val
    dst = edges[:, 1][pos.clamp(min=0)]
    return torch.where(pos >= 0, dst, torch.full_like(dst, -1)), val


@torch.no_grad()
def recommend_links(predictor, h: Tensor, adj: SparseTensor, adj2: Optional[SparseTensor], sources: Tensor, k: int,
                    batch_size: int, args=None, known: Optional[SparseTensor] = None, run_ahead: int = 6,
                    prefilter: Optional[Tuple[str, int]] = None) -> Tuple[Tensor, Tensor]:
    """The ``k`` best predicted links of every source: (``dst`` int64 [Q, k], ``score`` float32 [Q, k]), best first, ``dst``
    = -1 and ``score`` = -inf where a source has fewer than ``k`` candidates.

    The candidates of all ``Q`` sources (``two_hop_candidates``, in source order) are scored by ONE
    ``pipeline.score_edges(predictor, h, adj, adj2, edges, batch_size, args, run_ahead)`` call and selected per source.
    The normalisation of cn5 and cn7 couples the candidates of a batch, so the contract is stated in terms of that call:
    the scores are exactly those ``score_edges`` returns for the flat candidate list at this ``batch_size``.  Another set of
    ``sources`` or another ``batch_size`` puts other candidates into a batch and changes cn5 / cn7 scores — as it does in the
    reference's ``test()`` — unless the predictor carries frozen column weights (``predictor.set_frozen_columns``,
    ``ocn_amd.frozen``): then a source's scores depend on neither.  Ties go to the lower node id (candidates are in ascending order).

    ``adj2=None``: the candidates come from ``adj`` alone and the one scoring call is
    ``pipeline.score_edges_walk(predictor, h, adj, edges, batch_size, args, run_ahead)``; the contract is the same sentence
    with that call in it.  The candidate LIST is the one a materialised A² gives; the SCORES are not those of the pattern
    route: on the walk route cn2 carries walk counts (``utils.get_cn1_cn2``, the route of the ppa and citation2 drivers), by
    design, so the two routes may rank a source's candidates differently.

    The 3-hop predictor cn6 is served with ``adj2`` given: ``score_edges`` forms its third handle from ``adj`` and the bit rows
    of ``adj2`` (``utils.adjoverlap_3hop``), no A³ is stored.  With ``adj2=None`` it raises ValueError: the walk route has no
    3-hop form.

    ``prefilter=(kind, m)``, ``kind`` in ("cn", "aa", "ra") and ``k <= m <= ops.segment_topk_max_k()``: retrieve, then rank.
    The candidates are short-listed by the heuristic first — ``prefilter_candidates(adj, sources, kind, m, known)``: the ``m``
    best per source, expanded and scored from ``adj`` in one pass, whether or not ``adj2`` is given (the list equals that of
    ``adj2`` where ``adj2`` has the pattern of A·A) — and the one scoring call above, ``score_edges`` with ``adj2`` given (cn6
    included) and ``score_edges_walk`` without, sees the retained list only.  The contract is the same sentence: the scores
    are exactly those the scoring loop returns for the flat RETAINED list at this ``batch_size``.  A batch of the retained list
    holds other candidates than a batch of the full one, so batch-coupled cn5 / cn7 scores differ from the unfiltered run's;
    with frozen column weights a retained pair's score is, within the frozen scoring tolerance, its score in the unfiltered
    run, and the result differs from the unfiltered one only where the heuristic dropped a pair the model would have ranked
    among the ``k`` best.  Where no source has more than ``m`` candidates the retained list is the full list and the result
    is the unfiltered one.  ``prefilter=None``: every candidate is scored, as described above."""
    from .pipeline import score_edges, score_edges_walk
    if predictor.training:
        raise RuntimeError("recommend_links is the eval path; call predictor.eval() first")
    k = _check_k(k)
    from .model import CNLinkPredictor3hopCNs
    if adj2 is None and isinstance(predictor, CNLinkPredictor3hopCNs):
        raise ValueError("cn6 needs adj2 = adj @ adj: the walk route has no 3-hop form")
    if prefilter is not None:
        kind, m = _check_prefilter(prefilter, k)
        ptr, edges = prefilter_candidates(adj, sources, kind, m, known)
        if adj2 is None:
            scores = score_edges_walk(predictor, h, adj, edges, batch_size, args, run_ahead)
        else:
            scores = score_edges(predictor, h, adj, adj2, edges, batch_size, args, run_ahead)
        return _select(scores, ptr, edges, k)
    ptr, edges = two_hop_candidates(adj, adj2, sources, known)
    if adj2 is None:
        scores = score_edges_walk(predictor, h, adj, edges, batch_size, args, run_ahead)
    else:
        scores = score_edges(predictor, h, adj, adj2, edges, batch_size, args, run_ahead)
    return _select(scores, ptr, edges, k)


@torch.no_grad()
def recommend_links_heuristic(adj: SparseTensor, adj2: Optional[SparseTensor], sources: Tensor, k: int, batch_size: int,
                              kind: str, known: Optional[SparseTensor] = None) -> Tuple[Tensor, Tensor]:
    """``recommend_links`` with one training-free heuristic (``heuristics.score_edges_heuristic``) in place of a model.  A
    heuristic score depends on its candidate alone: the result does not change with ``batch_size`` or with the other sources.
    ``adj2=None`` serves the 1-hop kinds (cn, aa, ra, jaccard, pa), which never read A²: same candidates, same scores as with
    the product given.  The 2-hop kinds intersect with the rows of ``adj2`` and refuse None."""
    from .heuristics import _check_kinds, score_edges_heuristic
    _check_kinds((kind,), adj2)
    k = _check_k(k)
    ptr, edges = two_hop_candidates(adj, adj2, sources, known)
    scores = score_edges_heuristic(adj, adj2, edges, batch_size, kind)
    return _select(scores, ptr, edges, k)
