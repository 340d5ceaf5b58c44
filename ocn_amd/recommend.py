"""Top-K link recommendation: "for these nodes, which links do you predict?".

The scoring loops (``pipeline.score_edges``, ``heuristics.score_edges_heuristic``) take candidate pairs that somebody else
made and return a flat score vector.  This module makes the pairs and picks from the scores, both on the device:

* the default candidate set of a common-neighbour predictor is the 2-hop neighbourhood of a source that is not yet linked,
  ``pattern(A² row s) \\ (N(s) ∪ {s})`` — any other target has an empty ``cn1``.  (Not an empty ``cn2``: ``cn2(s, t) = N(s) ∩
  pattern(A² row t)`` is non-empty for every target within THREE hops; ``hops=3`` below serves those.)
  ``two_hop_candidates`` enumerates that set difference row by row (``ops.row_diff_count`` -> ``ops.scan_i32`` ->
  ``ops.row_diff_fill``) straight into the [T, 2] layout the scoring loops take: no dense [Q, N] mask, no host loop;
* where A² is not stored — more columns than the A·A pattern kernel takes, or a product too large to keep, the ppa and
  citation2 shapes — ``adj2=None`` expands the same set from A itself (``ops.two_hop_diff_count`` / ``_fill``) and the
  model scores it on the walk route (``pipeline.score_edges_walk``), as the drivers of those datasets score;
* candidate lists are ragged — under a power law from a handful to tens of thousands per source — so the best ``k`` per
  source are selected segment by segment (``ops.segment_topk``) instead of padding to a [Q, max_len] rectangle;
* retrieve, then rank: the expansion from A that enumerates the candidates of ``s`` visits, for every neighbour ``m`` of ``s``,
  every ``c`` in N(m) — adding the weight of ``m`` to an accumulator of column ``c`` there yields the cn / aa / ra score of
  every candidate in the same pass (``two_hop_scored_candidates``, ``ops.two_hop_sums_fill``).  ``prefilter_candidates`` keeps
  the ``m`` best per source and ``recommend_links(..., prefilter=(kind, m))`` lets the model rank only those.  Opt-in;
* three hops: a pair at distance exactly 3 has an empty ``cn1`` and a non-empty ``cn2`` — its only evidence is the higher-order
  common neighbours.  For a symmetric ``adj``, ``{t : cn1 or cn2 non-empty} \\ (N(s) ∪ {s})`` is ``(pattern(A² row s) ∪
  pattern(A³ row s)) \\ (N(s) ∪ {s})``.  The expansion above with the frontier made explicit (``ops.frontier_count`` /
  ``ops.frontier_sums_fill``: a per-query list of nodes and weights, and seeds) chains: the unexcluded 2-hop list of ``s``,
  weighted by ``decay · w[c] · P₂(s, c)`` and seeded with ``P₂``, expands into the candidates within three hops and their
  local path index ``P₂ + decay · P₃`` in ordered fp32 (``three_hop_candidates``, ``path_scored_candidates``).  ``hops=3`` in
  ``recommend_links`` takes its candidates from there, with ``prefilter=(kind, m, decay)`` through a short list.  Opt-in;
* random-walk retrieval: the expansions above enumerate every candidate within ``hops`` before they keep ``m``, so a request
  costs what the neighbourhood of its worst source holds.  ``W`` uniform walks of 2 or 3 steps from a source cost ``W · L``
  dependent row reads whatever its degree, and their visit counts estimate the "ra" path index: ``E[c₂(t)] / W = RA(s, t) /
  deg s``, ``E[c₃(t)] / W = P₃(s, t) / deg s`` (``random_walk_candidates``, ``ops.rw_visits_count`` / ``_fill``).
  ``random_walk_short_list`` keeps the ``m`` most visited and ``prefilter=RandomWalks(m, walks, length[, decay, seed])`` lets the
  model rank only those.  A sample, not the exact list: ``ranking.rank_links`` measures what it keeps.  Opt-in;
* embedding retrieval: every stage above is graph-local — a target beyond three hops is never proposed and a source without
  neighbours gets nothing — while the model scores any pair.  ``EmbeddingIndex`` quantises the node embeddings to int8 once,
  ``embedding_candidates`` takes, per source, the ``m`` nodes with the largest inner product over ALL nodes
  (``ops.mips_topm_i8``: an exact int8 GEMM on the matrix cores whose epilogue keeps ``m`` keys per query — no [Q, N] matrix),
  ``prefilter=EmbeddingNeighbours(m)`` lets the model rank those, and ``prefilter=ShortListUnion(...)`` the per-source union
  of several stages' lists: graph evidence where there is some, embeddings for the cold sources.  Opt-in;
* short lists beyond 128: the tuple form keeps its ``m`` best through ``ops.segment_topk``, whose sorted list a wave holds in
  two registers per lane — ``m <= 128``.  A short list needs the SET of the ``m`` best in ascending node id, not their ranked
  order: ``prefilter=PathSums(kind, m[, decay])`` means what the tuple means and takes the set through
  ``ops.segment_keep_best`` — a radix select of the cut and one ordered compaction — for any ``m``
  (``prefilter_candidates_long``).  Opt-in.

Everything runs on one GPU; dealing the sources over several is not built here.
"""
from __future__ import annotations

from dataclasses import dataclass
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
    sources = _check_sources(adj, sources, known)
    n = adj.size(0)
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


def _check_hops(hops) -> int:
    if isinstance(hops, bool) or hops not in (2, 3):
        raise ValueError(f"hops must be 2 or 3, got {hops!r}")
    return int(hops)


def _check_decay(decay) -> float:
    import math
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not math.isfinite(decay) or decay < 0:
        raise ValueError(f"decay must be a finite number >= 0 (the weight of a 3-walk beside a 2-path; it has no default), got {decay!r}")
    return float(decay)


def _check_sources(adj: SparseTensor, sources: Tensor, known: SparseTensor) -> Tensor:
    if not isinstance(sources, Tensor) or sources.dim() != 1 or sources.dtype != torch.int64:
        raise ValueError("sources must be a 1-d int64 tensor of node ids")
    n = adj.size(0)
    for name, m in (("adj", adj), ("known", known)):
        if tuple(m.sparse_sizes()) != (n, n):
            raise ValueError(f"{name} is {tuple(m.sparse_sizes())}, expected the square size ({n}, {n}) of adj")
    return sources.contiguous()


class _ThreeHop:
    """The first half of a 3-hop expansion, for all sources: the unexcluded 2-hop list ``L2`` (empty ``M``, the source itself
    stays in) with ``u = P₂``, the frontier weights ``f = (decay32 · w[c]) · u`` — two rounded fp32 products in eager torch,
    ``w ≡ 1`` for "cn" — and the size of every source's candidate set (the count pass).  ``fill(a, b)`` runs the second
    expansion for the sources ``a .. b``.  ``kind=None``: unit weights and no values (the candidates alone)."""

    def __init__(self, adj: SparseTensor, sources: Tensor, kind: Optional[str], decay: float, known: SparseTensor):
        n, dev = adj.size(0), sources.device
        self.rows = sources
        self.A = (adj._rowptr, adj._col)
        self.M = (known._rowptr, known._col)
        none = (torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))   # M = 0: every row empty
        self.n = n
        with ops.prevalidated(sources, sources, n, n):
            self.ptr2 = ops.scan_i32(ops.two_hop_diff_count(*self.A, *none, sources, drop_self=False))
            if kind is None:
                self.L2 = ops.two_hop_diff_fill(*self.A, *none, sources, self.ptr2, drop_self=False)
                self.u = self.f = None
            else:
                w = None
                if kind != "cn":
                    from .heuristics import node_table
                    w = node_table(adj)
                wcol = 1 if kind == "ra" else 0
                self.L2, self.u = ops.two_hop_sums_fill(*self.A, *none, sources, self.ptr2, w, wcol, drop_self=False)
                d32 = torch.tensor(decay, dtype=torch.float32, device=dev)
                self.f = (d32 * self.u) if w is None else ((d32 * w[self.L2[:, 1], wcol]) * self.u)
            self.count = ops.frontier_count(*self.A, *self.M, sources, self.ptr2, self.L2, self.ptr2, self.L2, drop_self=True)
            self.ptr = ops.scan_i32(self.count)

    def fill(self, a: int, b: int, total: Optional[int] = None) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
        """(ptr [b - a + 1] from 0, edges, val) of the sources ``a .. b``: the lists are addressed by absolute offsets, so a chunk
        is a slice of ``rows`` and of the two offset vectors."""
        p2 = self.ptr2[a:b + 1]
        off = self.ptr[a:b + 1] if a == 0 else self.ptr[a:b + 1] - self.ptr[a]
        with ops.prevalidated(self.rows, self.rows, self.n, self.n):
            edges, val = ops.frontier_sums_fill(*self.A, *self.M, self.rows[a:b], p2, self.L2, self.f, p2, self.L2, self.u,
                                                off.contiguous(), drop_self=True, total=total, values=self.u is not None)
        return off, edges, val


def three_hop_candidates(adj: SparseTensor, sources: Tensor, known: Optional[SparseTensor] = None) -> Tuple[Tensor, Tensor]:
    """The candidate targets of ``sources`` within THREE hops, in the layout of ``two_hop_candidates``: for each source ``s``
    the columns of ``pattern(A² row s) ∪ pattern(A³ row s)`` that are neither ``s`` nor in row ``s`` of ``known`` (``adj`` by
    default), ascending.  For a symmetric ``adj`` these are exactly the targets with a non-empty ``cn1`` or ``cn2`` — a pair
    at distance 3 has only the latter.  Two chained expansions from ``adj`` (``ops.two_hop_diff_*`` without an exclusion, then
    ``ops.frontier_*`` seeded with its own frontier); ``adj2`` is never read, so the list serves the pattern route and the
    walk route alike.  Under a power law the list is tens of times the 2-hop one."""
    known = adj if known is None else known
    sources = _check_sources(adj, sources, known)
    ptr, edges, _ = _ThreeHop(adj, sources, None, 0.0, known).fill(0, sources.numel())
    return ptr, edges


def path_scored_candidates(adj: SparseTensor, sources: Tensor, kind: str, hops: int, decay: float,
                           known: Optional[SparseTensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """The candidates within ``hops`` hops with their local path index: (``ptr`` int64 [Q + 1], ``edges`` int64 [T, 2], ``val``
    float32 [T]).  ``hops=2``: ``two_hop_scored_candidates(adj, sources, kind, known)``, unchanged (``decay`` is checked and not
    used).  ``hops=3``: the candidates of ``three_hop_candidates`` with ``val = P₂ + decay · P₃`` — ``P₂`` the path sum of
    ``two_hop_scored_candidates`` (0 where no 2-path exists), ``P₃(s, t)`` the sum of ``w[m] · w[c]`` over the 3-walks
    ``s – m – c – t``.  In fp32, in a fixed order: ``P₂`` first, then for every ``c`` of the 2-hop list whose row holds ``t``, in
    ascending ``c``, the term ``(decay32 · w[c]) · P₂(s, c)`` (two rounded products), one add each.  With ``kind="cn"`` that is
    the local path index ``A² + decay · A³``.  ``decay``: finite and >= 0; which value ranks well is a modelling decision."""
    _check_path_sum(kind)
    hops, decay = _check_hops(hops), _check_decay(decay)
    if hops == 2:
        return two_hop_scored_candidates(adj, sources, kind, known)
    known = adj if known is None else known
    sources = _check_sources(adj, sources, known)
    return _ThreeHop(adj, sources, kind, decay, known).fill(0, sources.numel())


def _keep_m_best(ptr: Tensor, edges: Tensor, val: Tensor, m: int) -> Tuple[Tensor, Tensor]:
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


def _keep_m_long(ptr: Tensor, edges: Tensor, val: Tensor, m: int) -> Tuple[Tensor, Tensor]:
    """What ``_keep_m_best`` returns, for any ``m``: the kept positions come from ``ops.segment_keep_best`` already ascending —
    no ranked [Q, m] rectangle, no sort."""
    ptr_m, keep = ops.segment_keep_best(val, ptr.contiguous(), m)
    return ptr_m, edges[keep]


def _budget_chunks(count: Tensor, budget: int):
    """Consecutive runs [a, b) of sources whose candidate total stays at or below ``budget``; a source above it goes alone."""
    sizes = count.tolist()
    a, run = 0, 0
    for q, c in enumerate(sizes):
        if q > a and run + c > budget:
            yield a, q, run
            a, run = q, 0
        run += c
    if len(sizes) > a:
        yield a, len(sizes), run


def _path_index_pass(adj: SparseTensor, sources: Tensor, kind: str, m: Optional[int], known: Optional[SparseTensor], hops: int,
                     decay: Optional[float], budget: Optional[int], targets: Optional[Tuple[Tensor, Tensor]] = None,
                     keep=_keep_m_best):
    """One pass over the path-scored candidates of every source, shared by ``prefilter_candidates`` and ``ocn_amd.ranking``:
    (``short``, ``rank``, ``count``).  ``short``: the (``ptr_m``, ``edges_m``) of ``prefilter_candidates`` where ``m`` is given,
    else None; ``keep(ptr, edges, val, m)`` selects it — ``_keep_m_best`` (``m <= ops.segment_topk_max_k()``) or
    ``_keep_m_long`` (any ``m``).  ``rank``: with ``targets = (tptr int64 [Q + 1], tnode int64 [P])``, the place of every target among ALL the
    candidates of its source by the path index (``ops.segment_rank``: 0 = no candidate), else None.  ``count`` int64 [Q]: the
    candidates of every source.  Under ``hops=3`` both are taken chunk by chunk — a chunk's targets are ranked against the
    chunk's ``val`` before it is reduced to its ``m`` best — so the full three-hop list never exists at once and neither result
    depends on ``budget``.  Ranking costs one host copy of ``tptr`` (the chunks slice ``tnode`` by it)."""
    _check_path_sum(kind)
    if _check_hops(hops) == 3:
        decay = _check_decay(decay)
        budget = int(ops.prefilter_budget if budget is None else budget)
        if budget < 1:
            raise ValueError(f"budget must be a positive number of candidates, got {budget}")
        known = adj if known is None else known
        sources = _check_sources(adj, sources, known)
        plan = _ThreeHop(adj, sources, kind, decay, known)
        tp = targets[0].tolist() if targets is not None else None
        parts, ranks = [], []
        for a, b, total in _budget_chunks(plan.count, budget):
            ptr, edges, val = plan.fill(a, b, total)
            if targets is not None:
                ranks.append(ops.segment_rank(val, ptr, edges, targets[0][a:b + 1] - tp[a], targets[1][tp[a]:tp[b]])[0])
            if m is not None:
                parts.append(keep(ptr, edges, val, m))
        rank = None
        if targets is not None:
            rank = torch.cat(ranks) if ranks else torch.zeros_like(targets[1])
        short = None
        if m is not None:
            ptr_m = torch.zeros(sources.numel() + 1, dtype=torch.int64, device=sources.device)
            if not parts:
                short = ptr_m, torch.empty(0, 2, dtype=torch.int64, device=sources.device)
            else:
                torch.cumsum(torch.cat([p[1:] - p[:-1] for p, _ in parts]), 0, out=ptr_m[1:])
                short = ptr_m, torch.cat([e for _, e in parts])
        return short, rank, plan.count.long()
    if decay is not None or budget is not None:
        raise ValueError("decay and budget belong to hops=3")
    ptr, edges, val = two_hop_scored_candidates(adj, sources, kind, known)
    rank = ops.segment_rank(val, ptr, edges, *targets)[0] if targets is not None else None
    return (keep(ptr, edges, val, m) if m is not None else None), rank, ptr[1:] - ptr[:-1]


def prefilter_candidates(adj: SparseTensor, sources: Tensor, kind: str, m: int, known: Optional[SparseTensor] = None,
                         hops: int = 2, decay: Optional[float] = None, budget: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """The ``m`` best candidates of every source by a path-sum heuristic: (``ptr_m`` int64 [Q + 1], ``edges_m`` int64 [T_m, 2])
    in the layout of ``two_hop_candidates``.  Per source the candidates of ``two_hop_scored_candidates`` are ranked in the total
    order of ``segment_topk`` — higher ``val`` first, ties to the lower node id — the first ``m`` are kept (all of them where a
    source has no more) and returned in ASCENDING node id, so that "ties go to the lower node id" still holds for whoever ranks
    the retained list again.  ``1 <= m <= ops.segment_topk_max_k()``.  One host sync more than the candidates cost (the size of
    the retained list).

    ``hops=3`` (with ``decay``, see ``path_scored_candidates``): the candidates within three hops, ranked by ``P₂ + decay · P₃``.
    Their list is tens of times the 2-hop one, so the sources are dealt into consecutive chunks whose candidate total, known
    from the count pass, stays at or below ``budget`` (``ops.prefilter_budget`` by default; a single source above it goes alone);
    a chunk is filled, ranked and reduced to its ``m`` best before the next.  The result does not depend on ``budget``."""
    _check_path_sum(kind)
    return _path_index_pass(adj, sources, kind, _check_m(m), known, hops, decay, budget)[0]


@dataclass(frozen=True)
class PathSums:
    """A path-sum retrieval stage without the 128 limit, a ``prefilter`` of ``recommend_links`` / ``ranking.rank_links`` and a
    stage of a ``ShortListUnion``: it means what the tuple ``(kind, m[, decay])`` means — the same candidates, the same path
    index, the same total order, the same ascending short list — and takes its ``m`` best through ``ops.segment_keep_best``
    for every ``m``.  Checked on construction: ``kind`` in ``PATH_SUMS``, ``m`` an int in 1 .. ``ops.SEGMENT_KEEP_MAX_M``,
    ``decay`` None or finite and >= 0.  ``decay`` is required under ``hops=3`` and refused under ``hops=2``; that is checked
    where ``hops`` is known (``_check_prefilter``)."""
    kind: str
    m: int
    decay: Optional[float] = None

    def __post_init__(self):
        _check_path_sum(self.kind)
        if isinstance(self.m, bool) or not isinstance(self.m, int) or not 1 <= self.m <= ops.SEGMENT_KEEP_MAX_M:
            raise ValueError(f"m must be an int in 1..{ops.SEGMENT_KEEP_MAX_M}, got {self.m!r}")
        if self.decay is not None:
            _check_decay(self.decay)


def _check_path_sums_hops(stage: PathSums, hops: int) -> PathSums:
    if not isinstance(stage, PathSums):
        raise ValueError(f"stage must be a PathSums, got {stage!r}")
    if hops == 3 and stage.decay is None:
        raise ValueError("a PathSums stage under hops=3 needs decay (the weight of a 3-walk beside a 2-path; it has no default)")
    if hops == 2 and stage.decay is not None:
        raise ValueError("decay belongs to hops=3")
    return stage


def prefilter_candidates_long(adj: SparseTensor, sources: Tensor, stage: PathSums, known: Optional[SparseTensor] = None,
                              hops: int = 2, budget: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """``prefilter_candidates(adj, sources, stage.kind, stage.m, known, hops, stage.decay, budget)`` for any ``m``: the same
    (``ptr_m`` int64 [Q + 1], ``edges_m`` int64 [T_m, 2]) — bit for bit where ``m <= ops.segment_topk_max_k()`` — with the ``m``
    best of every source taken as a set (``ops.segment_keep_best``: the cut by a radix select, then one ordered compaction)
    instead of a ranked top-``m`` that is sorted back.  Under ``hops=3`` every chunk is reduced that way before the next is
    filled; the result does not depend on ``budget``."""
    stage = _check_path_sums_hops(stage, _check_hops(hops))
    return _path_index_pass(adj, sources, stage.kind, stage.m, known, hops, stage.decay, budget, keep=_keep_m_long)[0]


# ---------------------------------------------------------------------------------------------
# random-walk retrieval
# ---------------------------------------------------------------------------------------------
def _check_rw(walks, length, decay, seed) -> Tuple[int, int, float, int]:
    """(walks, length, decay32-to-be, seed) of a random-walk stage: ``walks`` in 1 .. ``ops.rw_max_walks()``, ``length`` 2 or 3,
    ``decay`` required with ``length=3`` (``_check_decay``) and refused with ``length=2``, ``seed`` in 0 .. 2^64 - 1."""
    if isinstance(length, bool) or length not in (2, 3):
        raise ValueError(f"length must be 2 or 3 (the steps of a walk), got {length!r}")
    if isinstance(walks, bool) or not isinstance(walks, int) or not 1 <= walks <= ops.rw_max_walks():
        raise ValueError(f"walks must be an int in 1..{ops.rw_max_walks()}, got {walks!r}")
    if length == 3:
        decay = _check_decay(decay)
    elif decay is not None:
        raise ValueError("decay belongs to length=3")
    else:
        decay = 0.0
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < (1 << 64):
        raise ValueError(f"seed must be an int in 0 .. 2^64 - 1, got {seed!r}")
    return int(walks), int(length), decay, int(seed)


@dataclass(frozen=True)
class RandomWalks:
    """A random-walk retrieval stage, the ``prefilter`` of ``recommend_links`` / ``ranking.rank_links``: the ``m`` most visited
    candidates of ``walks`` uniform walks of ``length`` steps per source, ranked by ``c₂ + decay · c₃`` (``decay`` with
    ``length=3`` only, no default there).  Checked on construction: ``1 <= m <= ops.segment_topk_max_k()``, ``1 <= walks <=
    ops.rw_max_walks()``, ``length`` in (2, 3), ``decay`` finite and >= 0, ``seed`` in 0 .. 2^64 - 1."""
    m: int
    walks: int
    length: int
    decay: Optional[float] = None
    seed: int = 0

    def __post_init__(self):
        if isinstance(self.m, bool) or not isinstance(self.m, int):
            raise ValueError(f"m must be an int, got {self.m!r}")
        _check_m(self.m)
        _check_rw(self.walks, self.length, self.decay, self.seed)


def random_walk_candidates(adj: SparseTensor, sources: Tensor, walks: int, length: int, decay: Optional[float] = None,
                           known: Optional[SparseTensor] = None, seed: int = 0) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The nodes that ``walks`` uniform random walks of ``length`` (2 or 3) steps from every source visit, in the layout of
    ``path_scored_candidates`` with the counts beside it: (``ptr`` int64 [Q + 1], ``edges`` int64 [T, 2], ``val`` float32 [T],
    ``visits`` int32 [T, 2]).  Walk ``w`` of source ``s`` starts at ``s`` and takes, at every step, the ``floor(u · deg / 2⁶⁴)``-th
    entry of the row of ``adj`` it stands on (a walk that meets an empty row ends); ``visits[:, 0] = c₂`` counts the walks whose
    second step ends in the node, ``visits[:, 1] = c₃`` those whose third does (``length=3``; the first step is never counted),
    and ``val = float32(c₂) + float32(decay) · float32(c₃)``, two roundings (``float32(c₂)`` for ``length=2``).  A source's
    segment holds every visited node that is neither the source nor in its row of ``known`` (``adj`` by default), ascending, at
    most ``walks · (length - 1)`` of them.

    With uniform steps ``E[c₂(t)] / walks = RA(s, t) / deg s`` and ``E[c₃(t)] / walks = P₃(s, t) / deg s`` with ``P₃`` the
    3-walk sum of ``path_scored_candidates(kind="ra", hops=3)``: ``val`` estimates ``deg s · walks`` times the "ra" path index
    ``P₂ + decay · P₃``, and a source's ranking by it estimates the exact one.  The random words are Philox4x32-10 blocks whose
    counter carries the SOURCE id (ocn_hip.h: ocn_rw_visits_count): a source's segment is fixed bit for bit by (``seed``, the
    source, ``adj``, ``known``, ``walks``, ``length``) — not by the other sources, their order, or the launch — and a repeated
    source repeats its segment.  ``decay``: required for ``length=3``, refused for ``length=2``.  ``adj`` may be directed.
    The cost is ``walks · length`` dependent row reads per source, whatever its degree.  Two host syncs, as the other builders."""
    walks, length, decay, seed = _check_rw(walks, length, decay, seed)
    known = adj if known is None else known
    sources = _check_sources(adj, sources, known)
    n = adj.size(0)
    rpa, cola, rpk, colk = adj._rowptr, adj._col, known._rowptr, known._col
    with ops.prevalidated(sources, sources, n, n):
        count = ops.rw_visits_count(rpa, cola, rpk, colk, sources, walks, length, seed)
        ptr = ops.scan_i32(count)
        edges, val, visits = ops.rw_visits_fill(rpa, cola, rpk, colk, sources, walks, length, seed, ptr, decay)
    return ptr, edges, val, visits


def _rw_pass(adj: SparseTensor, sources: Tensor, rw: RandomWalks, known: Optional[SparseTensor],
             targets: Optional[Tuple[Tensor, Tensor]] = None):
    """``_path_index_pass`` for a random-walk stage: (``short``, ``rank``, ``count``) — the ``m`` most visited per source, the
    place of every target among ALL visited candidates of its source by ``val`` (``ops.segment_rank``: 0 = not visited), the
    visited candidates of every source."""
    if not isinstance(rw, RandomWalks):
        raise ValueError(f"rw must be a RandomWalks, got {rw!r}")
    ptr, edges, val, _ = random_walk_candidates(adj, sources, rw.walks, rw.length, rw.decay, known, rw.seed)
    rank = ops.segment_rank(val, ptr, edges, *targets)[0] if targets is not None else None
    return _keep_m_best(ptr, edges, val, rw.m), rank, ptr[1:] - ptr[:-1]


def random_walk_short_list(adj: SparseTensor, sources: Tensor, rw: RandomWalks,
                           known: Optional[SparseTensor] = None) -> Tuple[Tensor, Tensor]:
    """The ``rw.m`` most visited candidates of every source: (``ptr_m`` int64 [Q + 1], ``edges_m`` int64 [T_m, 2]), the contract
    of ``prefilter_candidates`` — the candidates of ``random_walk_candidates`` ranked by ``val`` in the total order of
    ``segment_topk`` (ties, which integer counts make often, go to the lower node id), the first ``m`` kept and returned in
    ASCENDING node id."""
    return _rw_pass(adj, sources, rw, known)[0]


# ---------------------------------------------------------------------------------------------
# embedding retrieval
# ---------------------------------------------------------------------------------------------
class EmbeddingIndex:
    """The int8 image of a node-embedding matrix, made once: ``keys_q`` int8 [N, Hp] and ``kscale`` float32 [N] of
    ``ops.quantize_rows_i8(keys, normalize)`` (``Hp``: the width ``H`` padded to ``ops.mips_h_align()``), with ``n = N``,
    ``width = H`` and ``normalize`` (rows scaled to unit L2 norm first: cosine retrieval).  A plain object of two tensors and
    three Python values: ``torch.save`` stores it, ``to(device)`` moves it.  Quantisation is one pass over [N, H]: after
    ``insert_edges`` and a refresh of ``h`` the index is simply made again."""

    def __init__(self, keys: Tensor, normalize: bool = False):
        if not isinstance(normalize, bool):
            raise ValueError(f"normalize must be a bool, got {normalize!r}")
        if not isinstance(keys, Tensor) or keys.dim() != 2 or keys.dtype != torch.float32:
            raise ValueError("keys must be a float32 [N, H] matrix of node embeddings")
        if keys.shape[0] < 1 or keys.shape[1] < 1 or keys.shape[1] > ops.MIPS_H_MAX:
            raise ValueError(f"keys must have at least one row and 1..{ops.MIPS_H_MAX} columns, got {tuple(keys.shape)}")
        self.n, self.width, self.normalize = int(keys.shape[0]), int(keys.shape[1]), normalize
        self.keys_q, self.kscale = ops.quantize_rows_i8(keys.detach(), normalize)

    @classmethod
    def from_table(cls, table) -> "EmbeddingIndex":
        """The index an ``ops.Int8Table`` already is (``pipeline.embedding_table(h, "int8")``), on the same storage: what
        ``EmbeddingIndex(h)`` makes, without a second image of the embeddings.  ``normalize`` is False."""
        if not isinstance(table, ops.Int8Table):
            raise ValueError(f"table must be an ops.Int8Table, got {type(table).__name__}")
        if table.shape[0] < 1 or table.width > ops.MIPS_H_MAX:
            raise ValueError(f"the table must have at least one row and 1..{ops.MIPS_H_MAX} columns, got {tuple(table.shape)}")
        other = object.__new__(EmbeddingIndex)
        other.n, other.width, other.normalize = int(table.shape[0]), int(table.width), False
        other.keys_q, other.kscale = table.rows, table.scale
        return other

    def to(self, device) -> "EmbeddingIndex":
        other = object.__new__(EmbeddingIndex)
        other.n, other.width, other.normalize = self.n, self.width, self.normalize
        other.keys_q, other.kscale = self.keys_q.to(device), self.kscale.to(device)
        return other


def _check_queries(index: EmbeddingIndex, queries: Tensor, sources: Tensor, known: Optional[SparseTensor]) -> Tensor:
    if not isinstance(index, EmbeddingIndex):
        raise ValueError(f"index must be an EmbeddingIndex, got {type(index).__name__}")
    if not isinstance(sources, Tensor) or sources.dim() != 1 or sources.dtype != torch.int64:
        raise ValueError("sources must be a 1-d int64 tensor of node ids")
    if not isinstance(queries, Tensor) or queries.dim() != 2 or queries.dtype != torch.float32 or \
            tuple(queries.shape) != (sources.numel(), index.width):
        raise ValueError(f"queries must be float32 [{sources.numel()}, {index.width}]: one row of the index's width per source")
    if known is not None and tuple(known.sparse_sizes()) != (index.n, index.n):
        raise ValueError(f"known is {tuple(known.sparse_sizes())}, expected the square size ({index.n}, {index.n}) of the index")
    return sources.contiguous()


def embedding_candidates(index: EmbeddingIndex, queries: Tensor, sources: Tensor, m: int,
                         known: Optional[SparseTensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """The ``m`` nearest nodes of every source by inner product, over ALL nodes of the index: (``ptr`` int64 [Q + 1], ``edges``
    int64 [T, 2], ``val`` float32 [T]) in the layout of ``path_scored_candidates``.  ``queries`` float32 [Q, H] — for instance
    ``h[sources]`` — are quantised per call as the index was (``ops.quantize_rows_i8`` with the index's ``normalize``); source
    ``q`` is offered every node but ``sources[q]`` itself and, with ``known`` (a square ``SparseTensor`` of the index's size;
    default: no further exclusion — the recommendation paths pass ``adj``), the nodes of its row there.  The eligible nodes are
    ranked by ``val = float32(dot) * kscale[node]`` — ``dot`` the exact int32 inner product of the int8 rows, the multiply the
    only rounding (``ops.mips_topm_i8``) — in the total order of ``segment_topk`` with the node id as the position (higher
    first, ties to the lower id); the first ``m`` are kept (all where fewer are eligible) and returned in ASCENDING node id, as
    every short list is.  ``val`` is the kernel's value: ``val * qscale[q]``, with ``qscale`` the query's own quantisation
    scale, approximates the inner product ``<queries[q], keys[node]>`` (the cosine under ``normalize``); a source's order does
    not need that factor, so it is not applied.  Quantising the retrieval stage is the usual trade: the model re-ranks the list
    in fp32.  ``1 <= m <= ops.mips_max_m()``.  One host sync for the sources' bounds, one for the output size."""
    m = _check_m(m)
    sources = _check_queries(index, queries, sources, known)
    qq, _ = ops.quantize_rows_i8(queries, index.normalize)
    val, node = ops.mips_topm_i8(qq, index.keys_q, index.kscale, m, rows=sources,
                                 excl=None if known is None else (known._rowptr, known._col), drop_self=True)
    Q = sources.numel()
    have = node >= 0
    ptr = torch.zeros(Q + 1, dtype=torch.int64, device=sources.device)
    torch.cumsum(have.sum(1), 0, out=ptr[1:])
    big = torch.iinfo(torch.int64).max
    ids, at = torch.where(have, node, torch.full_like(node, big)).sort(dim=1)          # ascending id, the pads last
    keep = ids < big
    dst = ids[keep]
    src = sources[:, None].expand(Q, m)[keep]
    return ptr, torch.stack([src, dst], 1), val.gather(1, at)[keep]


def embedding_retrieval_rank(index: EmbeddingIndex, queries: Tensor, sources: Tensor, known: Optional[SparseTensor],
                             tptr: Tensor, tnode: Tensor, chunk_elems: int = 1 << 24) -> Tensor:
    """The place of given nodes in the order ``embedding_candidates`` cuts: rank int64 [P], 1 + the eligible nodes that precede
    target ``tnode[j]`` of its source, 0 where the target is not eligible (the source itself, in ``known``, no node id).  An
    independent restatement in plain torch on the device — the kernel is not called: the integer dot products are exact, so a
    float64 matmul of the int8 matrices, ``float32(dot) * kscale`` and a count of the keys that precede give the kernel's order.
    Chunks of queries (and of targets) of about ``chunk_elems`` matrix entries; evaluation only."""
    sources = _check_queries(index, queries, sources, known)
    n, dev, Q, P = index.n, sources.device, sources.numel(), tnode.numel()
    ops.check_edges(sources, sources, n, n)
    rank = torch.zeros(P, dtype=torch.int64, device=dev)
    if not (Q and P):
        return rank
    qq, _ = ops.quantize_rows_i8(queries, index.normalize)
    kd = index.keys_q.double()
    ids = torch.arange(n, device=dev)
    tp = tptr.tolist()
    step = max(1, int(chunk_elems) // n)
    for a in range(0, Q, step):
        b = min(Q, a + step)
        if tp[b] == tp[a]:
            continue
        val = (qq[a:b].double() @ kd.t()).float() * index.kscale[None, :]
        elig = torch.ones(b - a, n, dtype=torch.bool, device=dev)
        elig[torch.arange(b - a, device=dev), sources[a:b]] = False
        if known is not None:
            rp, col = known._rowptr, known._col
            start = rp[sources[a:b]]
            cnt = rp[sources[a:b] + 1] - start
            seg = torch.repeat_interleave(torch.arange(b - a, device=dev), cnt)
            first = torch.cumsum(cnt, 0) - cnt
            at = torch.arange(seg.numel(), device=dev) - first[seg] + start[seg]
            elig[seg, col[at].long()] = False
        counts = (tptr[a + 1:b + 1] - tptr[a:b])
        tq = torch.repeat_interleave(torch.arange(b - a, device=dev), counts)
        for c in range(tp[a], tp[b], step):
            d = min(tp[b], c + step)
            ql, t = tq[c - tp[a]:d - tp[a]], tnode[c:d]
            ok = (t >= 0) & (t < n)
            tc = t.clamp(0, n - 1)
            ok &= elig[ql, tc]
            tv = val[ql, tc][:, None]
            rows_v = val[ql]
            ahead = ((rows_v > tv) | ((rows_v == tv) & (ids[None, :] < tc[:, None]))) & elig[ql]
            rank[c:d] = torch.where(ok, ahead.sum(1) + 1, torch.zeros_like(tc))
    return rank


@dataclass(frozen=True, eq=False)
class EmbeddingNeighbours:
    """An embedding retrieval stage, a ``prefilter`` of ``recommend_links`` / ``ranking.rank_links``: per source the ``m``
    nodes with the largest int8 inner product against its embedding, over all nodes (``embedding_candidates``).  ``keys``:
    None — the ``h`` given to the call is quantised per call — or a float32 [N, H] matrix, or a ready ``EmbeddingIndex`` (what a
    caller who serves many requests passes; its ``normalize`` must be this stage's).  The queries are ``h[sources]`` either
    way.  Checked on construction: ``1 <= m <= ops.mips_max_m()``, ``normalize`` a bool.  ``hops`` is not read by this stage."""
    m: int
    normalize: bool = False
    keys: Optional[object] = None

    def __post_init__(self):
        if isinstance(self.m, bool) or not isinstance(self.m, int):
            raise ValueError(f"m must be an int, got {self.m!r}")
        _check_m(self.m)
        if not isinstance(self.normalize, bool):
            raise ValueError(f"normalize must be a bool, got {self.normalize!r}")
        k = self.keys
        if isinstance(k, EmbeddingIndex):
            if k.normalize != self.normalize:
                raise ValueError(f"keys was indexed with normalize = {k.normalize}, the stage asks for {self.normalize}")
        elif k is not None and not (isinstance(k, Tensor) and k.dim() == 2 and k.dtype == torch.float32):
            raise ValueError("keys must be None, a float32 [N, H] matrix or an EmbeddingIndex")


class ShortListUnion:
    """A ``prefilter`` whose short list is, per source, the union (ascending, duplicate-free) of the short lists of its
    ``stages``: each a ``(kind, m[, decay])`` tuple (``prefilter_candidates``; the arity goes with ``hops``), a ``PathSums`` (the
    same stage for any ``m``; its ``decay`` goes with ``hops``), a ``RandomWalks`` (its ``length`` must equal ``hops``) or an
    ``EmbeddingNeighbours``.  What a mixed request needs: graph evidence where there
    is some, embeddings for the cold sources.  A source's list holds at most the sum of the stages' ``m``; ``k`` may be at most
    the largest ``m``.  There is no single retrieval order: ``ranking.rank_links`` reports ``retrieval_rank`` and ``m`` as None,
    and membership in the union is what ``coverage`` reads."""

    def __init__(self, *stages):
        if not stages:
            raise ValueError("ShortListUnion needs at least one stage")
        for st in stages:
            if not isinstance(st, (tuple, list, PathSums, RandomWalks, EmbeddingNeighbours)):
                raise ValueError(f"a stage must be a (kind, m[, decay]) tuple, a PathSums, a RandomWalks or an EmbeddingNeighbours, got {st!r}")
        self.stages = tuple(tuple(st) if isinstance(st, list) else st for st in stages)

    def __repr__(self):
        return f"ShortListUnion{self.stages!r}"


def _stage_m(stage) -> int:
    return stage.m if isinstance(stage, (PathSums, RandomWalks, EmbeddingNeighbours)) else stage[1]


def _prefilter_m(prefilter) -> Optional[int]:
    """The ``m`` a checked ``prefilter`` cuts at; None without one and for a union (no single cut)."""
    return None if prefilter is None or isinstance(prefilter, ShortListUnion) else _stage_m(prefilter)


def _refuse_cosine_of_int8(h, stage: EmbeddingNeighbours) -> None:
    """An ``ops.Int8Table`` serves a ``normalize=False`` stage as its own index; a cosine index is quantised from the unit-norm
    fp32 rows, which the table does not hold (TypeError; reads the types alone)."""
    if isinstance(h, ops.Int8Table) and stage.normalize:
        raise TypeError("an EmbeddingNeighbours stage with normalize=True and without keys= needs an fp32 (torch.float32) "
                        "embedding table, got an int8 table (Int8Table): its cosine index is quantised from the unit-norm fp32 "
                        "rows — pass keys=EmbeddingIndex(h_fp32, normalize=True)")


def _emb_pass(stage: EmbeddingNeighbours, h: Optional[Tensor], adj: SparseTensor, sources: Tensor, known: Optional[SparseTensor],
              targets: Optional[Tuple[Tensor, Tensor]] = None):
    """``_path_index_pass`` for an embedding stage: (``short``, ``rank``, ``count``) — the ``m`` nearest per source, the place of
    every target among ALL eligible nodes of its source (``embedding_retrieval_rank``), the length of every short list."""
    if h is None:
        raise ValueError("an EmbeddingNeighbours stage needs the node embeddings h")
    known = adj if known is None else known
    sources = _check_sources(adj, sources, known)
    n = adj.size(0)
    q8 = isinstance(h, ops.Int8Table)
    if not (q8 or isinstance(h, Tensor)) or h.dim() != 2 or h.shape[0] != n:
        raise ValueError(f"h must be the [{n}, H] node embeddings of adj")
    if stage.keys is None:
        ops.refuse_half_table(h, "an EmbeddingNeighbours stage without keys= (the int8 index is quantised from fp32 rows)")
        _refuse_cosine_of_int8(h, stage)
    if isinstance(stage.keys, EmbeddingIndex):
        index = stage.keys
    elif q8 and stage.keys is None:
        index = EmbeddingIndex.from_table(h)                 # (an int8 table IS the index of its rows: no second image)
    else:
        index = EmbeddingIndex((h if stage.keys is None else stage.keys).float(), stage.normalize)
    if index.n != n:
        raise ValueError(f"the stage's keys hold {index.n} nodes, adj {n}")
    ops.check_edges(sources, sources, n, n)                  # (before h is indexed)
    queries = h.float_rows(sources) if q8 else h.detach()[sources].float()
    ptr, edges, _ = embedding_candidates(index, queries, sources, stage.m, known)
    rank = embedding_retrieval_rank(index, queries, sources, known, *targets) if targets is not None else None
    return (ptr, edges), rank, ptr[1:] - ptr[:-1]


def _union_pass(union: ShortListUnion, h: Optional[Tensor], adj: SparseTensor, sources: Tensor, known: Optional[SparseTensor],
                hops: int) -> Tuple[Tensor, Tensor]:
    """The per-source union of the stages' short lists, formed with ``ops.csr_union`` on their (``ptr``, ids) pairs."""
    ptr = ids = None
    for st in union.stages:
        if isinstance(st, RandomWalks):
            p, e = _rw_pass(adj, sources, st, known)[0]
        elif isinstance(st, EmbeddingNeighbours):
            p, e = _emb_pass(st, h, adj, sources, known)[0]
        elif isinstance(st, PathSums):
            p, e = _path_index_pass(adj, sources, st.kind, st.m, known, hops, st.decay, None, keep=_keep_m_long)[0]
        else:
            p, e = _path_index_pass(adj, sources, st[0], st[1], known, hops, None if hops == 2 else st[2], None)[0]
        c = e[:, 1].to(torch.int32).contiguous()
        ptr, ids = (p.contiguous(), c) if ptr is None else ops.csr_union(ptr, ids, p.contiguous(), c)
    src = torch.repeat_interleave(sources, ptr[1:] - ptr[:-1], output_size=ids.numel())
    return ptr, torch.stack([src, ids.long()], 1)


def _check_prefilter(prefilter, k: int, hops: int = 2):
    """(kind, m) for ``hops=2``, (kind, m, decay) for ``hops=3``: the other arity is refused.  A ``RandomWalks`` (checked when
    it was made) passes as it is where it keeps at least ``k`` and walks ``hops`` steps, an ``EmbeddingNeighbours`` where it
    keeps at least ``k``; the stages of a ``ShortListUnion`` are checked one by one and the largest ``m`` must reach ``k``.  A
    ``PathSums`` passes where it keeps at least ``k`` and carries ``decay`` exactly under ``hops=3``; no 128 limit applies."""
    if isinstance(prefilter, PathSums):
        _check_path_sums_hops(prefilter, hops)
        if k > prefilter.m:
            raise ValueError(f"prefilter keeps m = {prefilter.m} candidates per source, fewer than k = {k}")
        return prefilter
    if isinstance(prefilter, EmbeddingNeighbours):
        if k > prefilter.m:
            raise ValueError(f"prefilter keeps m = {prefilter.m} candidates per source, fewer than k = {k}")
        return prefilter
    if isinstance(prefilter, ShortListUnion):
        stages = tuple(_check_prefilter(st, 1, hops) for st in prefilter.stages)
        top = max(_stage_m(st) for st in stages)
        if k > top:
            raise ValueError(f"prefilter keeps m = {top} candidates per source in its largest stage, fewer than k = {k}")
        return ShortListUnion(*stages)
    if isinstance(prefilter, RandomWalks):
        if k > prefilter.m:
            raise ValueError(f"prefilter keeps m = {prefilter.m} candidates per source, fewer than k = {k}")
        if hops != prefilter.length:
            raise ValueError(f"prefilter walks length = {prefilter.length} steps, hops = {hops}: the two must be equal")
        return prefilter
    form = "(kind, m)" if hops == 2 else "(kind, m, decay) under hops=3,"
    if not isinstance(prefilter, (tuple, list)) or len(prefilter) != hops or not isinstance(prefilter[0], str) \
            or isinstance(prefilter[1], bool) or not isinstance(prefilter[1], int):
        raise ValueError(f"prefilter must be None or {form} with kind one of {PATH_SUMS} and m an int, got {prefilter!r}")
    kind, m = _check_path_sum(prefilter[0]), _check_m(prefilter[1])
    if k > m:
        raise ValueError(f"prefilter keeps m = {m} candidates per source, fewer than k = {k}")
    return (kind, m) if hops == 2 else (kind, m, _check_decay(prefilter[2]))


def _candidates(adj: SparseTensor, adj2: Optional[SparseTensor], sources: Tensor, known: Optional[SparseTensor], hops: int,
                prefilter, targets: Optional[Tuple[Tensor, Tensor]] = None,
                h: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """The candidate list of a request: the short list where ``prefilter`` (checked) is given, else every candidate within
    ``hops`` hops.  A segment of the top-k takes fewer than 2^32 - 1 entries, and so does the flat list.  Third: with a short
    list and ``targets``, the retrieval rank of every target (``_path_index_pass``), else None — and None under a
    ``ShortListUnion``, which has no single retrieval order.  ``h``: the node embeddings, read by the embedding stages only."""
    if isinstance(prefilter, EmbeddingNeighbours):
        short, rank, _ = _emb_pass(prefilter, h, adj, sources, known, targets)
        return short[0], short[1], rank
    if isinstance(prefilter, ShortListUnion):
        return (*_union_pass(prefilter, h, adj, sources, known, hops), None)
    if isinstance(prefilter, RandomWalks):
        short, rank, _ = _rw_pass(adj, sources, prefilter, known, targets)
        return short[0], short[1], rank
    if isinstance(prefilter, PathSums):
        short, rank, _ = _path_index_pass(adj, sources, prefilter.kind, prefilter.m, known, hops, prefilter.decay, None, targets,
                                          keep=_keep_m_long)
        return short[0], short[1], rank
    if prefilter is not None:
        short, rank, _ = _path_index_pass(adj, sources, prefilter[0], prefilter[1], known, hops,
                                          None if hops == 2 else prefilter[2], None, targets)
        return short[0], short[1], rank
    if hops == 2:
        return (*two_hop_candidates(adj, adj2, sources, known), None)
    ptr, edges = three_hop_candidates(adj, sources, known)
    if edges.shape[0] >= (1 << 32) - 1:
        raise ValueError(f"{edges.shape[0]} candidates within three hops: the flat list must have fewer than 2^32 - 1 entries "
                         "(ask for fewer sources per call, or short-list with prefilter=(kind, m, decay))")
    return ptr, edges, None


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


def _check_request(predictor, adj2: Optional[SparseTensor], k: int, prefilter, hops):
    """The refusals of a model request, before anything touches the device: the checked (``hops``, ``prefilter``).  ``k``: what a
    short list must at least keep (checked by the caller)."""
    from .model import CNLinkPredictor3hopCNs
    if adj2 is None and isinstance(predictor, CNLinkPredictor3hopCNs):
        raise ValueError("cn6 needs adj2 = adj @ adj: the walk route has no 3-hop form")
    hops = _check_hops(hops)
    if prefilter is not None:
        prefilter = _check_prefilter(prefilter, k, hops)
    return hops, prefilter


def _check_table(predictor, h, prefilter) -> None:
    """The refusals of a bf16 / f16 embedding table (``pipeline.embedding_table``) in a model request, before anything touches
    the device (TypeError): cn6, and an ``EmbeddingNeighbours`` stage that would quantise its int8 index from ``h`` itself — pass
    ``keys=EmbeddingIndex(h_fp32)``; the queries ``h[sources]`` are widened exactly.  An ``ops.Int8Table`` is refused by cn6
    alike; a ``normalize=False`` stage without ``keys=`` takes the table itself as its index (``EmbeddingIndex.from_table``,
    queries ``table.float_rows(sources)``), a ``normalize=True`` one is refused.  Everything else passes the table on to the
    scoring loop."""
    from .model import CNLinkPredictor3hopCNs
    if not ops.is_compact_table(h):
        return
    if isinstance(predictor, CNLinkPredictor3hopCNs):
        ops.refuse_compact_table(h, "cn6 (cn_gather3)")
    stages = prefilter.stages if isinstance(prefilter, ShortListUnion) else (prefilter,)
    for st in stages:
        if isinstance(st, EmbeddingNeighbours) and st.keys is None:
            ops.refuse_half_table(h, "an EmbeddingNeighbours stage without keys= (the int8 index is quantised from fp32 rows)")
            _refuse_cosine_of_int8(h, st)


def _score_request(predictor, h: Tensor, adj: SparseTensor, adj2: Optional[SparseTensor], sources: Tensor, batch_size: int,
                   args, known: Optional[SparseTensor], run_ahead: int, prefilter, hops: int,
                   targets: Optional[Tuple[Tensor, Tensor]] = None):
    """Candidates, then ONE scoring call — what ``recommend_links`` selects from and ``ranking.rank_links`` ranks in:
    (``ptr``, ``edges``, ``scores``, the retrieval rank of ``targets`` under a short list or None).  ``hops`` and ``prefilter``
    come from ``_check_request``."""
    from .pipeline import score_edges, score_edges_walk
    ptr, edges, rank = _candidates(adj, adj2, sources, known, hops, prefilter, targets, h)
    if adj2 is None:
        scores = score_edges_walk(predictor, h, adj, edges, batch_size, args, run_ahead)
    else:
        scores = score_edges(predictor, h, adj, adj2, edges, batch_size, args, run_ahead)
    return ptr, edges, scores, rank


@torch.no_grad()
def recommend_links(predictor, h: Tensor, adj: SparseTensor, adj2: Optional[SparseTensor], sources: Tensor, k: int,
                    batch_size: int, args=None, known: Optional[SparseTensor] = None, run_ahead: int = 6,
                    prefilter: Optional[tuple] = None, hops: int = 2) -> Tuple[Tensor, Tensor]:
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
    is the unfiltered one.  ``prefilter=None``: every candidate is scored, as described above.

    ``hops=3``: the candidates are those within three hops (``three_hop_candidates``: every target with a non-empty cn1 or
    cn2, expanded from ``adj`` alone on either route) and the contract is the same sentence — the scores are exactly those of
    the one scoring call on the flat list; ValueError if that list has 2^32 - 1 entries or more.  Under a power law it is tens
    of times the 2-hop list, so the form to serve is ``hops=3`` with ``prefilter=(kind, m, decay)``: the short list is then
    taken over three hops by ``P₂ + decay · P₃`` (``prefilter_candidates(..., hops=3, decay=decay)``).  A 2-tuple with
    ``hops=3`` or a 3-tuple with ``hops=2`` is refused.  cn6 is served over these <= 3 hops; its own evidence reaches four.

    ``prefilter=PathSums(kind, m[, decay])``: the tuple form without its limit — the short list is
    ``prefilter_candidates_long(adj, sources, prefilter, known, hops)``, the tuple's list where ``m <=
    ops.segment_topk_max_k()`` and the ``m`` best by the same order beyond it; ``decay`` is required under ``hops=3`` and refused
    under ``hops=2``.  The contract is the same sentence.  ``k <= m``, and ``k`` itself stays within
    ``ops.segment_topk_max_k()``: the short list grows, the ranked answer does not.

    ``prefilter=RandomWalks(m, walks, length[, decay, seed])``: the short list is ``random_walk_short_list(adj, sources,
    prefilter, known)`` — the ``m`` most visited nodes of ``walks`` random walks per source, at a cost that does not grow with
    the neighbourhood — and the contract is the same sentence: the scores are exactly those the scoring loop returns for the
    flat retained list at this ``batch_size``.  ``k <= m``; ``hops`` must equal ``length`` (ValueError otherwise).  The list is
    a sample: a candidate no walk reached is not in it, however the model would have ranked it.

    ``prefilter=EmbeddingNeighbours(m[, normalize, keys])``: the short list is ``embedding_candidates`` over ``keys`` (default:
    this call's ``h``, quantised per call; a caller who serves many requests passes ``keys=EmbeddingIndex(...)``) with ``queries
    = h[sources]`` and ``known`` as given (default ``adj``) — the ``m`` nodes nearest to the source's embedding among ALL nodes,
    whatever their distance in the graph, so a source without neighbours gets ``k`` targets too.  The contract is the same
    sentence: the scores are exactly those the scoring loop returns for the flat retained list at this ``batch_size``.
    ``k <= m``; ``hops`` is not read by this stage.

    ``prefilter=ShortListUnion(stage, ...)``: the short list is the per-source union (ascending, duplicate-free) of the stages'
    short lists — tuples, ``RandomWalks`` and ``EmbeddingNeighbours``, each checked as above for this ``hops`` — and the
    contract is the same sentence again.  ``k`` may be at most the largest ``m`` of the stages."""
    if predictor.training:
        raise RuntimeError("recommend_links is the eval path; call predictor.eval() first")
    k = _check_k(k)
    hops, prefilter = _check_request(predictor, adj2, k, prefilter, hops)
    _check_table(predictor, h, prefilter)
    ptr, edges, scores, _ = _score_request(predictor, h, adj, adj2, sources, batch_size, args, known, run_ahead, prefilter, hops)
    return _select(scores, ptr, edges, k)


@torch.no_grad()
def recommend_links_heuristic(adj: SparseTensor, adj2: Optional[SparseTensor], sources: Tensor, k: int, batch_size: int,
                              kind: str, known: Optional[SparseTensor] = None, hops: int = 2) -> Tuple[Tensor, Tensor]:
    """``recommend_links`` with one training-free heuristic (``heuristics.score_edges_heuristic``) in place of a model.  A
    heuristic score depends on its candidate alone: the result does not change with ``batch_size`` or with the other sources.
    ``adj2=None`` serves the 1-hop kinds (cn, aa, ra, jaccard, pa), which never read A²: same candidates, same scores as with
    the product given.  The 2-hop kinds intersect with the rows of ``adj2`` and refuse None.  ``hops=3``: the candidates within
    three hops (``three_hop_candidates``); a 1-hop kind scores those beyond two hops 0."""
    from .heuristics import _check_kinds, score_edges_heuristic
    _check_kinds((kind,), adj2)
    k = _check_k(k)
    ptr, edges, _ = _candidates(adj, adj2, sources, known, _check_hops(hops), None)
    scores = score_edges_heuristic(adj, adj2, edges, batch_size, kind)
    return _select(scores, ptr, edges, k)
