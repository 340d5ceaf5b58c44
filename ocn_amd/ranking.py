"""Where held-out links land in the ranking that is served: ranks, then recall@K / NDCG@K / hit rate / MRR.

``recommend_links`` returns the best ``k <= 128`` targets of a source and drops the rest; ``evaluate.Evaluator`` implements the
reference's sampled-negative protocols.  Neither says whether a known-good link ``(s, t)`` is a candidate of ``s`` at all, whether
a short list kept it, or where it stands among the thousands of candidates of ``s``.  This module does, with the calls and the
order of ``recommend``:

* ``rank_links`` / ``rank_links_heuristic`` form the candidates and the scores exactly as ``recommend_links`` /
  ``recommend_links_heuristic`` do for the same arguments (one shared helper) and, instead of selecting the best ``k``, locate
  every true target in its source's segment: ``ops.segment_rank`` counts the entries that precede it in the total order of
  ``ops.segment_topk``.  So "rank <= k" and "``recommend_links(..., k)`` lists it at that place" are one statement;
* with a short list (``prefilter``) the same kernel ranks the targets by the short-list heuristic among ALL candidates, inside the
  retrieval pass — under ``hops=3`` chunk by chunk, before a chunk is reduced to its ``m`` best — so a miss is told apart: not a
  candidate, dropped by the short list, or ranked;
* an embedding short list (``recommend.EmbeddingNeighbours``) ranks the targets among ALL eligible nodes by an independent torch
  restatement of the int8 order; a ``recommend.ShortListUnion`` has no single order and reports membership only;
* ``rank_path_index`` is that retrieval stage alone, without a model: the cheap way to sweep ``kind``, ``decay`` and ``m``;
* ``ranking_metrics`` turns a result into the usual figures.

Ranks are unfiltered: the other true targets of a source are not removed from above a target.  One GPU.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import ops, recommend as R
from .sparse import SparseTensor

Truth = Union[SparseTensor, Tuple[Tensor, Tensor]]


@dataclass
class RankResult:
    """The ranks of the true targets of a request.  ``sources`` int64 [Q] as given (a repeated source is a segment of its own);
    ``tptr`` int64 [Q + 1] and ``target`` int64 [P]: the targets of source ``q`` are ``target[tptr[q]:tptr[q + 1]]``; ``n_cand``
    int64 [Q]: the lengths of the segments that were ranked; ``rank`` int64 [P]: 0 = not ranked, else the 1-based place among the
    scored candidates of its source; ``retrieval_rank`` int64 [P], None without a short list: the place by the short-list heuristic
    among ALL candidates within ``hops`` (0 = no candidate: beyond ``hops``, the source itself, or in ``known`` — or, under a
    random-walk short list, not visited by any walk); ``m``: the size of the short list or None.  ``rank > 0`` exactly when ``1 <= retrieval_rank <= m``."""
    sources: Tensor
    tptr: Tensor
    target: Tensor
    n_cand: Tensor
    rank: Tensor
    retrieval_rank: Optional[Tensor] = None
    m: Optional[int] = None

    def to(self, device) -> "RankResult":
        return replace(self, sources=self.sources.to(device), tptr=self.tptr.to(device), target=self.target.to(device),
                       n_cand=self.n_cand.to(device), rank=self.rank.to(device),
                       retrieval_rank=None if self.retrieval_rank is None else self.retrieval_rank.to(device))


def _truth_lists(adj: SparseTensor, sources: Tensor, truth: Truth) -> Tuple[Tensor, Tensor]:
    """(``tptr`` int64 [Q + 1], ``tnode`` int64 [P]) of ``sources``.  A matrix: row ``s`` of ``truth`` for every source, gathered
    on the device (the sources are bounds-checked first; the size ``P`` of the list costs one host sync).  A ready pair is
    checked — offsets from 0 to ``P``, ascending — with one host sync as well."""
    n, Q = adj.size(0), sources.numel()
    if isinstance(truth, SparseTensor):
        if tuple(truth.sparse_sizes()) != (n, n):
            raise ValueError(f"truth is {tuple(truth.sparse_sizes())}, expected the square size ({n}, {n}) of adj")
        ops.check_edges(sources, sources, n, n)
        rp, col = truth._rowptr, truth._col
        start = rp[sources]
        count = rp[sources + 1] - start
        tptr = torch.zeros(Q + 1, dtype=torch.int64, device=sources.device)
        torch.cumsum(count, 0, out=tptr[1:])
        P = int(tptr[-1].item())
        seg = torch.repeat_interleave(torch.arange(Q, device=sources.device), count, output_size=P)
        at = torch.arange(P, device=sources.device) - tptr[seg] + start[seg]
        return tptr, col[at].long()
    if not isinstance(truth, (tuple, list)) or len(truth) != 2 or not all(isinstance(t, Tensor) for t in truth):
        raise ValueError("truth must be a square SparseTensor of adj's size or a pair (tptr int64 [Q + 1], tnode int64 [P])")
    tptr, tnode = truth
    if tptr.dim() != 1 or tptr.dtype != torch.int64 or tnode.dim() != 1 or tnode.dtype != torch.int64:
        raise ValueError("truth: tptr and tnode must be 1-d int64 tensors")
    if tptr.numel() != Q + 1:
        raise ValueError(f"truth: tptr has {tptr.numel()} offsets, expected one per source and the total ({Q + 1})")
    if tptr.device != sources.device or tnode.device != sources.device:
        raise ValueError("truth: tptr and tnode must live on the device of sources")
    tptr, tnode = tptr.contiguous(), tnode.contiguous()
    ok = (tptr[0] == 0) & (tptr[-1] == tnode.numel()) & (tptr[1:] >= tptr[:-1]).all()
    if not bool(ok.item()):
        raise ValueError(f"truth: tptr must ascend from 0 to the {tnode.numel()} entries of tnode")
    return tptr, tnode


def _request(adj: SparseTensor, sources: Tensor, truth: Truth, known: Optional[SparseTensor]):
    sources = R._check_sources(adj, sources, adj if known is None else known)
    return sources, _truth_lists(adj, sources, truth)


@torch.no_grad()
def rank_links(predictor, h: Tensor, adj: SparseTensor, adj2: Optional[SparseTensor], sources: Tensor, truth: Truth,
               batch_size: int, args=None, known: Optional[SparseTensor] = None, run_ahead: int = 6,
               prefilter: Optional[tuple] = None, hops: int = 2) -> RankResult:
    """The place of every true target among the candidates ``recommend_links(predictor, h, adj, adj2, sources, k, batch_size,
    args, known, run_ahead, prefilter, hops)`` selects from: the same candidates, the same ONE scoring call, the same scores
    (see there for the contract: batch-coupled cn5 / cn7 scores, frozen column weights, the walk route of ``adj2=None``, cn6
    only with ``adj2``, eval mode only, ``known``, the arity of ``prefilter`` per ``hops``).  A target of rank ``r <= k`` is
    ``dst[q, r - 1]`` of that call; a rank is not bounded by the top-k limit.

    ``truth``: a square ``SparseTensor`` of ``adj``'s size — row ``s`` holds the targets that count as hits for ``s``, for
    instance ``SparseTensor.from_edge_index(test_edges, sparse_sizes=...).to_symmetric()`` — or a ready ragged pair (``tptr``
    int64 [Q + 1], ``tnode`` int64 [P]).  From a matrix the list is gathered for ``sources`` on the device, which costs one host
    sync (its size).  Targets that are no candidates (already in ``known``, the source itself, beyond ``hops``) get rank 0.

    ``prefilter``: the model ranks the short list only, and ``retrieval_rank`` tells where the heuristic put every target among
    all the candidates within ``hops`` — taken in the retrieval pass itself, chunk by chunk under ``hops=3``.

    ``prefilter=recommend.PathSums(kind, m[, decay])``: the tuple's stage for any ``m`` — the same ``retrieval_rank``, and
    ``rank > 0`` exactly when ``1 <= retrieval_rank <= m`` with that ``m``, which is the one reported.

    ``prefilter=recommend.RandomWalks(...)``: ``retrieval_rank`` is the place by the walks' ``val`` among all VISITED candidates
    of the source, before the cut to ``m`` — 0 means that no walk reached the target (or that it is no candidate at all).

    ``prefilter=recommend.EmbeddingNeighbours(...)``: ``retrieval_rank`` is the place of every target among ALL eligible nodes
    of its source — every node but the source and its row of ``known`` — in the stage's order, ``float32(dot) * kscale`` with
    ties to the lower id (``recommend.embedding_retrieval_rank``: an independent restatement in plain torch on the device —
    chunks of queries, a float64 matmul of the int8 matrices, a count of the keys that precede; the arithmetic is exact
    integers, so it is the kernel's order).  ``rank > 0`` exactly when ``1 <= retrieval_rank <= m``.  Evaluation only: the
    restatement forms [chunk, N] matrices.

    ``prefilter=recommend.ShortListUnion(...)``: a union has no single retrieval order — ``retrieval_rank`` and ``m`` are None,
    ``rank > 0`` exactly for the targets in the union, and that membership is what ``ranking_metrics`` reports as
    ``coverage`` (no ``retention``)."""
    if predictor.training:
        raise RuntimeError("rank_links is the eval path; call predictor.eval() first")
    hops, prefilter = R._check_request(predictor, adj2, 1, prefilter, hops)
    R._check_table(predictor, h, prefilter)
    sources, targets = _request(adj, sources, truth, known)
    ptr, edges, scores, rrank = R._score_request(predictor, h, adj, adj2, sources, batch_size, args, known, run_ahead, prefilter,
                                                 hops, targets if prefilter is not None else None)
    rank, _ = ops.segment_rank(scores, ptr, edges, *targets)
    return RankResult(sources, targets[0], targets[1], ptr[1:] - ptr[:-1], rank, rrank, R._prefilter_m(prefilter))


@torch.no_grad()
def rank_links_heuristic(adj: SparseTensor, adj2: Optional[SparseTensor], sources: Tensor, truth: Truth, batch_size: int,
                         kind: str, known: Optional[SparseTensor] = None, hops: int = 2) -> RankResult:
    """``rank_links`` with one training-free heuristic in place of a model: the candidates and scores of
    ``recommend_links_heuristic(adj, adj2, sources, k, batch_size, kind, known, hops)``."""
    from .heuristics import _check_kinds, score_edges_heuristic
    _check_kinds((kind,), adj2)
    hops = R._check_hops(hops)
    sources, targets = _request(adj, sources, truth, known)
    ptr, edges, _ = R._candidates(adj, adj2, sources, known, hops, None)
    scores = score_edges_heuristic(adj, adj2, edges, batch_size, kind)
    rank, _ = ops.segment_rank(scores, ptr, edges, *targets)
    return RankResult(sources, targets[0], targets[1], ptr[1:] - ptr[:-1], rank)


@torch.no_grad()
def rank_path_index(adj: SparseTensor, sources: Tensor, truth: Truth, kind: str, hops: int, decay: Optional[float] = None,
                    known: Optional[SparseTensor] = None, budget: Optional[int] = None) -> RankResult:
    """The retrieval stage on its own, no scoring pass: ``rank`` is the place of every target among all the candidates within
    ``hops`` by the path index of ``recommend.path_scored_candidates`` (``kind`` in ("cn", "aa", "ra"); ``decay`` and ``budget``
    belong to ``hops=3``) — what ``rank_links(..., prefilter=(kind, m[, decay]))`` returns as ``retrieval_rank``, for every
    ``m`` at once: a short list of ``m`` keeps exactly the targets with ``1 <= rank <= m``.  ``n_cand`` counts all candidates.
    Under ``hops=3`` the list is formed and ranked in chunks of at most ``budget`` candidates; the result does not depend on it."""
    kind, hops = R._check_path_sum(kind), R._check_hops(hops)
    if hops == 3:
        R._check_decay(decay)
        if budget is not None and int(budget) < 1:
            raise ValueError(f"budget must be a positive number of candidates, got {budget}")
    elif decay is not None or budget is not None:
        raise ValueError("decay and budget belong to hops=3")
    sources, targets = _request(adj, sources, truth, known)
    _, rank, count = R._path_index_pass(adj, sources, kind, None, known, hops, decay, budget, targets)
    return RankResult(sources, targets[0], targets[1], count, rank)


def _check_ks(ks) -> Tuple[int, ...]:
    if isinstance(ks, (str, bytes)) or not isinstance(ks, Sequence) or len(ks) == 0 or \
            any(isinstance(k, bool) or not isinstance(k, int) or k < 1 for k in ks):
        raise ValueError(f"ks must be a non-empty sequence of ints >= 1, got {ks!r}")
    return tuple(int(k) for k in ks)


def ranking_metrics(res: RankResult, ks: Sequence[int] = (10, 20, 50, 100)) -> dict:
    """The figures of a ``RankResult``, a dict of Python numbers.  Over the sources with at least one target (``n_eval`` of
    them; a source without targets enters no mean), per ``k`` in ``ks`` — any ``k >= 1``, the limit of the top-k kernel is no
    limit of a rank:

    * ``recall@k``: the mean over sources of hits / targets, a hit being a target with ``1 <= rank <= k``;
    * ``hit_rate@k``: the share of sources with at least one hit;
    * ``ndcg@k``: binary gains — DCG = the sum of ``1 / log2(1 + rank)`` over the hits, IDCG the same sum over the places
      ``1 .. min(k, targets)`` — the mean of DCG / IDCG;
    * ``pair_hits@k``: the share of (source, target) pairs that are hits;

    and once: ``mrr`` (the mean of 1 / best rank of a source, 0 where none of its targets is ranked), ``coverage`` (the share
    of pairs that are candidates at all: ``retrieval_rank > 0`` with a short list, else ``rank > 0``; under a random-walk short
    list, ``recommend.RandomWalks``, that reads "visited by a walk at all": a sampled stage misses candidates the exact
    expansions list), with a short list ``retention`` (the share of candidate pairs the short list kept) and ``m``; ``n_eval``, ``n_sources``, ``n_pairs``.  A share
    of nothing is 0.0.

    Plain torch on the host: ``tptr`` and the ranks are copied there once (a result on the CPU is read where it is), counts are
    exact integers, sums are float64 added target by target and source by source in index order — no atomics, the same bits
    wherever the result lives."""
    ks = _check_ks(ks)
    tptr, rank = res.tptr.cpu(), res.rank.cpu()
    if tptr.dim() != 1 or tptr.numel() < 1 or rank.dim() != 1 or tptr.dtype != torch.int64 or rank.dtype != torch.int64:
        raise ValueError("res: tptr int64 [Q + 1] and rank int64 [P] expected")
    Q, P = tptr.numel() - 1, rank.numel()
    n_t = tptr[1:] - tptr[:-1]
    if int(tptr[0]) != 0 or int(tptr[-1]) != P or bool((n_t < 0).any()):
        raise ValueError(f"res: tptr must ascend from 0 to the {P} entries of rank")
    seg = torch.repeat_interleave(torch.arange(Q), n_t, output_size=P)
    ev = n_t > 0
    n_eval = int(ev.sum())

    def mean(per_source: Tensor) -> float:                  # float64 [Q] -> the mean over the evaluated sources, in source order
        return float(per_source[ev].sum(dtype=torch.float64)) / n_eval if n_eval else 0.0

    out = {"n_sources": Q, "n_eval": n_eval, "n_pairs": P}
    gain = torch.where(rank > 0, 1.0 / torch.log2(1.0 + rank.clamp(min=1).double()), torch.zeros(P, dtype=torch.float64))
    kmax = int(min(max(ks), int(n_t.max()) if Q else 0))
    ideal = torch.zeros(kmax + 1, dtype=torch.float64)      # ideal[j] = the DCG of j hits in the places 1 .. j
    torch.cumsum(1.0 / torch.log2(1.0 + torch.arange(1, kmax + 1, dtype=torch.float64)), 0, out=ideal[1:])
    for k in ks:
        hit = (rank >= 1) & (rank <= k)
        hits = torch.zeros(Q, dtype=torch.int64).index_add_(0, seg, hit.long())
        dcg = torch.zeros(Q, dtype=torch.float64).index_add_(0, seg, torch.where(hit, gain, torch.zeros_like(gain)))
        idcg = ideal[n_t.clamp(max=k)]
        out[f"recall@{k}"] = mean(hits.double() / n_t.clamp(min=1).double())
        out[f"hit_rate@{k}"] = int((hits[ev] > 0).sum()) / n_eval if n_eval else 0.0
        out[f"ndcg@{k}"] = mean(dcg / torch.where(ev, idcg, torch.ones_like(idcg)))
        out[f"pair_hits@{k}"] = int(hit.sum()) / P if P else 0.0
    big = torch.iinfo(torch.int64).max
    best = torch.full((Q,), big, dtype=torch.int64).scatter_reduce_(0, seg, torch.where(rank > 0, rank, torch.full_like(rank, big)),
                                                                     "amin")
    out["mrr"] = mean(torch.where(best < big, 1.0 / best.double(), torch.zeros(Q, dtype=torch.float64)))
    ranked = int((rank > 0).sum())
    if res.retrieval_rank is None:
        out["coverage"] = ranked / P if P else 0.0
    else:
        cand = int((res.retrieval_rank.cpu() > 0).sum())
        out["coverage"] = cand / P if P else 0.0
        out["retention"] = ranked / cand if cand else 0.0
        out["m"] = res.m
    return out
