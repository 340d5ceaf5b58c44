"""Explaining a predicted link: which common neighbours carry the score of a pair.

Every predictor here (cn5, cn7, cn8) scores a pair (i, j) from two pooled vectors and the endpoints' own product,

    xcn1[e] = sum_k wa(e, k) h[k]       xcn2[e] = sum_k wb(e, k) h[k]       xij[e] = h[i] * h[j]

both sums running over the neighbours k of i that are common neighbours of the pair.  The model is additive over named nodes
right up to the MLP heads, so "you are recommended j because of k1, k2, k3" is a well-defined quantity: with
g1[e] = d score_e / d xcn1[e] and g2[e] = d score_e / d xcn2[e] from the heads' autograd path, member k accounts for

    wa(e, k) <h[k], g1[e]>   via xcn1       wb(e, k) <h[k], g2[e]>   via xcn2

— gradient x input on the pooled vectors.  ``ops.cn_attribution`` forms these for every flagged entry of the batch (the
sampled dense-dense product on the CN pattern: no [B, N] matrix, no nnz x H gather), ``ops.segment_topk`` picks the ``m``
strongest per pair.

    exp = explain_links(predictor, h, adj, adj2, edges, m=8)
    exp.nodes[e]        # the m common neighbours that count most for edges[e], best first (-1: fewer than m)
    exp.contrib[e]      # their shares {via xcn1, via xcn2}; exp.pooled[e] is what all members together account for

``explain_link_edges`` goes on from there, through the encoder: which MESSAGES of the graph made h[i], h[j] and the h[k] look the
way they do.  Put a mask M = 1 on every message of every conv layer (``model.message_masks``); the saliency of message v -> u in
layer l is d score_e / d M_l[u, v] at M = 1 — gradient x input again, the normalisation coefficients held fixed as PyG's
explainers hold them.  The gradient of a layer with respect to its messages is the sampled dense-dense product on the pattern
of A (``ops.sddmm_csr``); ``ops.segment_topk`` lists the strongest.

    ex = explain_link_edges(model, predictor, x, adj, adj2, edges, which, top=20)
    ex.entries[t]       # message col -> row as (row, col); ex.saliency[t] its total, ex.per_layer[t] its share per conv layer

cn6 (three tables and ``nip``), ``max`` aggregation, edge-sharded predictors, training mode, several GPUs, symmetrising the
messages (u, v) and (v, u), and explanations accumulated over batches are out of scope.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import ops

RANKS = ("signed", "magnitude")
COUNTERFACTUAL_CHUNK_BYTES = 1 << 30      # modified pooled rows of one heads call (the counterfactual is chunked beyond it)


@dataclass
class LinkExplanation:
    """What ``explain_links`` returns for a batch of B pairs.  ``score`` fp32 [B]; ``nodes`` int64 [B, m]: the listed common
    neighbours, best first, -1 where a pair has fewer than m; ``contrib`` fp32 [B, m, 2]: their shares {via xcn1, via xcn2},
    padding 0; ``kind`` uint8 [B, m]: the flag byte (1: cn1 entry, 2: cn2 entry, 3: both), padding 0; ``pooled`` fp32 [B, 2] =
    {<g1, xcn1>, <g2, xcn2>}: what all members together account for; ``pair`` fp32 [B] = <g3, xij>: the endpoints' own
    share; ``cnt1`` / ``cnt2``: the member counts; ``drop`` fp32 [B, m] (``counterfactual=True``, else None): the exact change
    of the score when the listed member is taken out, NaN on padding; ``flat`` (``return_flat=True``, else None):
    (off int64 [B + 1], attr fp32 [cap, 2], rank fp32 [cap]) — every position of the flag chain, ``rank`` = -inf on
    non-members.  A plain object: ``torch.save`` / ``torch.load`` keep it."""
    score: Tensor
    nodes: Tensor
    contrib: Tensor
    kind: Tensor
    pooled: Tensor
    pair: Tensor
    cnt1: Tensor
    cnt2: Optional[Tensor]
    drop: Optional[Tensor] = None
    flat: Optional[Tuple[Tensor, Tensor, Tensor]] = None
    # with ``return_flat``: (g1, g2, g3) and (xcn1, xcn2, xij) of the batch, for whoever checks the numbers above
    _grads: Optional[Tuple[Tensor, Tensor, Tensor]] = field(default=None, repr=False)
    _pooled_vectors: Optional[Tuple[Tensor, Tensor, Tensor]] = field(default=None, repr=False)


if hasattr(torch.serialization, "add_safe_globals"):        # (torch.load's weights_only unpickler names the classes it builds)
    torch.serialization.add_safe_globals([LinkExplanation])


_NO_H = object()


def _check_request(predictor, h, edges, m, rank, args, what: str = "explain_links", count: str = "m") -> int:
    """The refusals, all before any device work; returns ``m``.  ``h=_NO_H``: there is no embedding matrix to check yet
    (``explain_link_edges`` forms it)."""
    from .model import (CNLinkPredictor3hopCNs, CNLinkPredictorbaselearn, CNLinkPredictorbaselearnablation,
                        CNLinkPredictorOringin)
    if isinstance(predictor, CNLinkPredictor3hopCNs):
        raise NotImplementedError("cn6 pools with three column tables and nip: explaining it is not built")
    if not isinstance(predictor, (CNLinkPredictorOringin, CNLinkPredictorbaselearn, CNLinkPredictorbaselearnablation)):
        raise TypeError(f"{what} takes a cn5, cn7 or cn8 predictor, got {type(predictor).__name__}")
    if predictor.training:
        raise RuntimeError(f"{what} explains eval-mode scores; call predictor.eval() first")
    if predictor._sharded:
        raise RuntimeError("an edge-sharded predictor scores one rank's slice of a batch: explain on an unsharded one")
    if getattr(predictor, "_cn_cap", None) is not None:
        raise RuntimeError(f"{what} explains the exact pooling, this predictor pools a capped sample: set_cn_cap(None) first")
    if isinstance(m, bool) or not isinstance(m, int) or not 1 <= m <= ops.segment_topk_max_k():
        raise ValueError(f"{count} must be an int in 1..{ops.segment_topk_max_k()}, got {m!r}")
    if rank not in RANKS:
        raise ValueError(f"rank must be one of {RANKS}, got {rank!r}")
    if not isinstance(edges, Tensor) or edges.dim() != 2 or edges.shape[1] != 2 or edges.dtype != torch.int64:
        raise ValueError("edges must be an int64 [B, 2] tensor")
    if not 1 <= int(edges.shape[0]) <= ops.MAX_BATCH:
        raise ValueError(f"edges is ONE batch of 1 .. {ops.MAX_BATCH} candidates (the histogram field width), got {int(edges.shape[0])}")
    if h is not _NO_H:
        ops.refuse_compact_table(h, f"{what} (gradients through the pooled rows)")
    if h is not _NO_H and (not isinstance(h, Tensor) or h.dim() != 2 or h.dtype != torch.float32 or h.shape[1] not in ops.LN_WIDTHS):
        raise ValueError(f"h must be float32 [N, H] with H in {ops.LN_WIDTHS}")
    if predictor._weights_need_args and predictor._frozen is None and args is None:
        raise ValueError("cn7's column weights read args.sum: pass args (or install frozen column weights)")
    return m


def _entry_weights(kind: Tensor, w: Tensor, c: Tensor) -> Tuple[Tensor, Tensor]:
    """``entry_weights`` of the kernels (csrc/common.h) restated in torch: ``kind`` the flag bytes, ``w`` their columns' rows
    {w1, t, inv2, 0}, ``c`` the cn2 values (walk counts, or 1)."""
    is1, is2 = (kind & 1) != 0, (kind & 2) != 0
    zero = torch.zeros((), dtype=torch.float32, device=w.device)
    wa = torch.where(is1, w[..., 0], zero)
    wb = (torch.where(is2, c, zero) - torch.where(is1, w[..., 1], zero)) * w[..., 2]
    return wa, wb


def _counterfactual(predictor, h, w, st, pooled, pos, pad, nodes, kind) -> Tensor:
    """score(base) - score(member removed, column weights held fixed) for every listed member; NaN on padding."""
    xcn1, xcn2, xij = pooled
    B, m = nodes.shape
    H = h.shape[1]
    k = nodes.clamp(min=0)
    c = st.wc[pos].to(torch.float32) if st.wc is not None else torch.ones((), dtype=torch.float32, device=h.device).expand(B, m)
    wa, wb = _entry_weights(kind, w[k], c)
    wa, wb = torch.where(pad, torch.zeros_like(wa), wa), torch.where(pad, torch.zeros_like(wb), wb)
    drop = torch.empty(B, m, dtype=torch.float32, device=h.device)
    per = max(1, COUNTERFACTUAL_CHUNK_BYTES // (m * H * 4))           # candidates per heads call: their base rows ride with their modified rows
    for lo in range(0, B, per):
        hi = min(B, lo + per)
        n = hi - lo
        hk = h[k[lo:hi]]                                                 # [n, m, H]
        x1 = torch.cat([xcn1[lo:hi], (xcn1[lo:hi, None, :] - wa[lo:hi, :, None] * hk).reshape(n * m, H)])
        x2 = torch.cat([xcn2[lo:hi], (xcn2[lo:hi, None, :] - wb[lo:hi, :, None] * hk).reshape(n * m, H)])
        x3 = torch.cat([xij[lo:hi], xij[lo:hi, None, :].expand(n, m, H).reshape(n * m, H)])
        s = predictor._heads(h, x1.contiguous(), x2.contiguous(), x3.contiguous(), None).reshape(-1)
        drop[lo:hi] = s[:n, None] - s[n:].reshape(n, m)
    return torch.where(pad, torch.full_like(drop, float("nan")), drop)


def explain_links(predictor, h: Tensor, adj, adj2, edges: Tensor, m: int = 8, args=None, rank: str = "signed",
                  counterfactual: bool = False, return_flat: bool = False) -> LinkExplanation:
    """The ``m`` common neighbours that count most for every pair of ``edges`` (int64 [B, 2], the layout ``score_edges``
    takes), with their shares of the score: a ``LinkExplanation``.

    ``edges`` forms ONE batch, 1 <= B <= ``ops.MAX_BATCH``, and is explained as the batch a direct ``predictor(...)`` call on it
    would score.  ``adj2`` given: the pattern route (``adjoverlap`` handles); ``adj2=None``: the walk route (``get_cn1_cn2``) —
    the rule of ``freeze_columns``.  ``m`` in 1..``ops.segment_topk_max_k()``.  Predictors: cn5, cn7 (``args`` for its
    ``sum``), cn8, in eval mode, with or without ``set_frozen_columns``; cn6 raises NotImplementedError, training mode and an
    edge-sharded predictor RuntimeError, a bad ``m`` / ``rank`` / ``edges`` ValueError — all before any device work.

    What the numbers are: GRADIENT x INPUT ON THE POOLED VECTORS.  With g1[e] = d score_e / d xcn1[e], g2[e] likewise
    (autograd through the heads, which act row by row; no parameter's ``.grad`` is touched), member k of pair e has
    ``contrib = {wa <h[k], g1[e]>, wb <h[k], g2[e]>}`` (``ops.cn_attribution``), (wa, wb) being the weights the pooling gives
    that entry.  Summed over all members they are ``pooled[e]`` = {<g1, xcn1>, <g2, xcn2>}; ``pair[e]`` = <g3, xij> is the
    endpoints' own share.  This is exact for the part of the score that is linear in the pooled vectors and a linearisation
    beyond that (the heads' LayerNorm and ReLU).  For an unfrozen cn5 / cn7 the weights are those of THIS batch: as the scores
    do, they depend on who else is in it; with frozen column weights (or cn8) a pair's explanation is its own.

    ``rank``: "signed" lists the largest ``contrib.sum(-1)`` first (the strongest support), "magnitude" the largest absolute
    value (support and opposition alike); ties go to the lower node id.

    ``counterfactual=True`` adds ``drop[e, r]`` = score_e minus the score with listed member r taken out of both pooled
    vectors, the column weights held fixed — the exact effect of that one member, from one more heads call over B (1 + m)
    rows; a member with wa = wb = 0 has ``drop`` exactly 0.  ``return_flat=True`` adds ``flat`` = (off, attr, rank) over every
    position of the batch's flag chain."""
    from .utils import adjoverlap, fuse, get_cn1_cn2
    m = _check_request(predictor, h, edges, m, rank, args)
    e = edges.t().contiguous()
    adj.warm(walk=adj2 is None)
    if adj2 is not None:
        adj2.complete()
    handles = get_cn1_cn2(adj, e) if adj2 is None else (adjoverlap(adj, adj, e), adjoverlap(adj, adj2, e))
    with torch.no_grad():
        # always the flag chain: the one-pass states (cn8, frozen) keep no flags to attribute on
        st = fuse(*handles, e, None, adj=adj)
        w = predictor._weights(st, args)
        hc = h.contiguous()
        xcn1, xcn2, xij = st.gather(w, hc)
    with torch.enable_grad():
        x1, x2, x3 = (t.detach().clone().requires_grad_() for t in (xcn1, xcn2, xij))
        out = predictor._heads(hc, x1, x2, x3, None)
        if out.numel() != st.B:
            raise ValueError("explain_links explains a predictor with one output channel")
        g1, g2, g3 = torch.autograd.grad(out.sum(), (x1, x2, x3))
    with torch.no_grad():
        score = out.detach().reshape(-1)
        g1, g2, g3 = g1.contiguous(), g2.contiguous(), g3.contiguous()
        attr, rk = ops.cn_attribution(adj._rowptr, adj._col, st.src, st.off, st.flags, st.wc, w, hc, g1, g2, order=st.order)
        by = rk if rank == "signed" else torch.where(rk == float("-inf"), rk, rk.abs())
        val, pos = ops.segment_topk(by, st.off, m)
        pad = val == float("-inf")                                       # fewer than m members (or an empty row: pos = -1)
        pos = pos.clamp(min=0)
        local = pos - st.off[:-1, None]
        nodes = adj._col[(adj._rowptr[st.src][:, None] + local).clamp(min=0, max=max(adj._col.numel() - 1, 0))].to(torch.int64)
        nodes = torch.where(pad, torch.full_like(nodes, -1), nodes)
        contrib = torch.where(pad[..., None], torch.zeros((), device=attr.device), attr[pos])
        kind = torch.where(pad, torch.zeros((), dtype=torch.uint8, device=attr.device), st.flags[pos])
        pooled = torch.stack([(g1 * xcn1).sum(1), (g2 * xcn2).sum(1)], dim=1)
        pair = (g3 * xij).sum(1)
        drop = _counterfactual(predictor, hc, w, st, (xcn1, xcn2, xij), pos, pad, nodes, kind) if counterfactual else None
        st.check_status()
        return LinkExplanation(score=score, nodes=nodes, contrib=contrib, kind=kind, pooled=pooled, pair=pair,
                               cnt1=st.cnt1.clone(), cnt2=None if st.cnt2 is None else st.cnt2.clone(), drop=drop,
                               flat=(st.off, attr, rk) if return_flat else None,
                               _grads=(g1, g2, g3) if return_flat else None,
                               _pooled_vectors=(xcn1, xcn2, xij) if return_flat else None)


# ---- down to the edges: message saliency through the encoder ----------------------------------------------------------------------
@dataclass
class EdgeExplanation:
    """What ``explain_link_edges`` returns for one candidate.  ``score`` fp32 scalar: the autograd path's score of the pair;
    ``entries`` int64 [top, 2]: the listed messages as (row, col) of the adjacency — message col -> row — strongest first, -1
    where fewer than ``top`` messages have a non-zero saliency; ``saliency`` fp32 [top]: their totals over the conv layers,
    padding 0; ``per_layer`` fp32 [top, L]: the share of every conv layer (layer 0 first), padding 0; ``input_share`` fp32 [N] =
    <d score / d x[v], x[v]>: gradient x input on the encoder's input features (None for id inputs); ``flat``
    (``return_flat=True``, else None): fp32 [L, nnz], every message of every layer in the adjacency's CSR order.  A plain
    object: ``torch.save`` / ``torch.load`` keep it."""
    score: Tensor
    entries: Tensor
    saliency: Tensor
    per_layer: Tensor
    input_share: Optional[Tensor] = None
    flat: Optional[Tensor] = None


if hasattr(torch.serialization, "add_safe_globals"):
    torch.serialization.add_safe_globals([EdgeExplanation])


def _check_edge_request(model, predictor, edges, which, top, rank, args) -> int:
    """The refusals of ``explain_link_edges``, all before any device work; returns the number of conv layers."""
    _check_request(predictor, _NO_H, edges, top, rank, args, what="explain_link_edges", count="top")
    if model.training:
        raise RuntimeError("explain_link_edges explains eval-mode scores; call model.eval() first")
    if isinstance(which, bool) or not isinstance(which, int) or not 0 <= which < int(edges.shape[0]):
        raise ValueError(f"which must be the index of a candidate of edges, 0..{int(edges.shape[0]) - 1}, got {which!r}")
    convs = getattr(model, "convs", None)
    if convs is None or len(convs) == 0:
        raise ValueError("the encoder has no message-passing layer: there is no message to attribute to")
    if any(getattr(conv, "aggr", None) == "max" for conv in convs):
        raise ValueError("max aggregation has no per-message linearisation: explain_link_edges takes sum, mean and gcn layers")
    return len(convs)


def explain_link_edges(model, predictor, x: Tensor, adj, adj2, edges: Tensor, which: int, top: int = 20, args=None,
                       rank: str = "magnitude", return_flat: bool = False) -> EdgeExplanation:
    """The ``top`` messages of the graph that count most for the score of candidate ``edges[which]``, through the pooling AND
    the encoder ``model`` (a GCN / GCN2 / GCN3 of ``ocn_amd.model``): an ``EdgeExplanation``.

    ``edges`` (int64 [B, 2]) is ONE batch, 1 <= B <= ``ops.MAX_BATCH``, scored as a direct ``predictor(model(x, adj), ...)`` call
    would score it; the other candidates only supply the batch's column weights — with frozen column weights or cn8 they do not
    matter.  ``adj2=None`` selects the walk route.  ``top`` in 1..``ops.segment_topk_max_k()``.  cn6 raises NotImplementedError,
    training mode of either module and an edge-sharded predictor RuntimeError, a bad ``which`` / ``top`` / ``rank`` / ``edges``,
    a ``max`` layer and cn7 without ``args`` and without a frozen table ValueError — all before any device work.

    What the numbers are: GRADIENT x INPUT ON THE MESSAGES.  Every conv layer l gets a mask M_l = 1 on its nnz messages
    (``model.message_masks``: y[u] = post[u] sum_v M_l[u, v] c(u, v) x[v] + self term); the saliency of message v -> u in layer l
    is d score / d M_l[u, v] at M = 1, with the normalisation coefficients c held fixed (they do not see the mask).  It is
    exact for what is linear in the messages and a linearisation through LayerNorm / ReLU and the heads, as ``explain_links``
    documents for the heads.  The self term is no message and gets nothing.  The backward of the pooling is
    ``gather_backward`` on the batch's flag chain, not autograd: a frozen predictor works, and no parameter's ``.grad`` is
    touched anywhere.

    ``rank``: "magnitude" lists the largest ``|saliency|`` first, "signed" the largest signed value; ``saliency`` is the sum of
    the layers taken in layer order; ties go to the lower CSR position (``ops.segment_topk``'s order)."""
    from .model import message_masks
    from .utils import adjoverlap, fuse, get_cn1_cn2
    L = _check_edge_request(model, predictor, edges, which, top, rank, args)
    ops.refuse_compact_table(x, "explain_link_edges (gradients through the encoder and the pooled rows)")
    e = edges.t().contiguous()
    adj.warm(walk=adj2 is None)
    if adj2 is not None:
        adj2.complete()
    handles = get_cn1_cn2(adj, e) if adj2 is None else (adjoverlap(adj, adj, e), adjoverlap(adj, adj2, e))
    nnz = int(adj._col.numel())
    dev = adj._col.device
    floats = isinstance(x, Tensor) and x.is_floating_point()
    with torch.enable_grad():
        xl = x.detach().clone().requires_grad_() if floats else x
        masks = [torch.ones(nnz, dtype=torch.float32, device=dev, requires_grad=True) for _ in range(L)]
        with message_masks(adj, masks):
            h = model(xl, adj)
    hc = h.detach().contiguous()
    ops.refuse_compact_table(hc, "explain_link_edges (gradients through the encoder and the pooled rows)")
    if hc.dim() != 2 or hc.dtype != torch.float32 or hc.shape[1] not in ops.LN_WIDTHS:
        raise ValueError(f"the encoder's output must be float32 [N, H] with H in {ops.LN_WIDTHS}")
    with torch.no_grad():
        st = fuse(*handles, e, None, adj=adj)                               # always the flag chain, as in explain_links
        w = predictor._weights(st, args)
        xcn1, xcn2, xij = st.gather(w, hc)
    with torch.enable_grad():
        x1, x2, x3 = (t.detach().clone().requires_grad_() for t in (xcn1, xcn2, xij))
        out = predictor._heads(hc, x1, x2, x3, None)
        if out.numel() != st.B:
            raise ValueError("explain_link_edges explains a predictor with one output channel")
        g1, g2, g3 = torch.autograd.grad(out.reshape(-1)[which], (x1, x2, x3))     # zero outside row ``which``
    with torch.no_grad():
        dh = st.gather_backward(w, hc, g1, g2, g3)
        st.check_status()
    # the encoder backward: the L mask gradients and the input gradient, and no parameter's .grad
    grads = torch.autograd.grad(h, masks + ([xl] if floats else []), grad_outputs=dh.reshape(h.shape), allow_unused=True)
    with torch.no_grad():
        flat = torch.stack([torch.zeros(nnz, dtype=torch.float32, device=dev) if g is None else g for g in grads[:L]])
        total = flat[0].clone()
        for l in range(1, L):
            total += flat[l]
        live = torch.nonzero(total != 0).flatten()                          # ascending position
        val = total[live].contiguous()
        by = val.abs() if rank == "magnitude" else val
        seg = torch.tensor([0, int(live.numel())], dtype=torch.int64, device=dev)
        best, pos = ops.segment_topk(by, seg, top)
        pad = pos[0] < 0
        p = live[pos[0].clamp(min=0)] if live.numel() else torch.zeros(top, dtype=torch.int64, device=dev)
        row = torch.searchsorted(adj._rowptr, p, right=True) - 1
        col = adj._col[p.clamp(max=max(nnz - 1, 0))].to(torch.int64) if nnz else torch.zeros_like(p)
        entries = torch.where(pad[:, None], torch.full((), -1, dtype=torch.int64, device=dev), torch.stack([row, col], dim=1))
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        saliency = torch.where(pad, zero, total[p] if nnz else zero.expand(top))
        per_layer = torch.where(pad[:, None], zero, flat[:, p].t() if nnz else zero.expand(top, L)).contiguous()
        share = None
        if floats:
            gx = grads[L]
            share = torch.zeros(x.shape[0], dtype=torch.float32, device=dev) if gx is None else (gx * x).sum(1)
        return EdgeExplanation(score=out.detach().reshape(-1)[which].clone(), entries=entries, saliency=saliency, per_layer=per_layer,
                               input_share=share, flat=flat if return_flat else None)
