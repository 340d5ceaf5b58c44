"""Frozen column weights: batch-independent cn5 / cn7 scoring.

The column normalisation of cn5 and cn7 (``cn.sum(dim=0)``; for cn5 also the scale and the orthogonalised sums) couples the
candidates of a batch: the score of a pair depends on who else is asked about.  That is the reference's ``test()``; for
serving it is a defect.  The remedy is BatchNorm's in eval mode: take the statistics once, from a named reference batch, and
keep them.  The statistics are exactly the [N, 4] column-weight table {w1, t, inv2, 0} that ``ocn_cn_weights_cn5`` / ``_cn7``
write; with it installed (``predictor.set_frozen_columns``) every candidate is pooled "as if it stood beside that batch
without being counted in it", and nothing of a candidate depends on the rest of its batch.

    fc = freeze_columns(predictor, adj, adj2, split_edge["valid"]["edge"], args)
    predictor.set_frozen_columns(fc)
    dst, score = recommend_links(predictor, h, adj, adj2, sources, k, batch_size)     # any sources, any batch_size: same scores

The table is one batch's: statistics accumulated over several batches are out of scope (the packed histogram fields would
overflow, and rescaled non-integer sums would be a modelling decision).  cn8 needs none of this (it pools without column
weights), cn6 has two tables and ``nip`` and is not served here.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Optional

import torch
from torch import Tensor

from . import ops


@dataclass
class FrozenColumns:
    """The column weights of one reference batch and what was baked into them.  ``weights``: fp32 [n_cols, 4] on the device;
    ``kind``: "cn5" / "cn7"; ``valued``: taken on the walk route (cn2 carries walk counts) — such a table serves walk handles
    only, a pattern table pattern handles only; ``ref_size``: the candidates of the reference batch; ``innerprod`` (cn5), or
    ``sum_fill`` / ``polyfirst`` / ``polysecond`` (cn7): the predictor's values the table was formed with (None for the other
    kind).  A plain object: ``torch.save`` / ``torch.load`` keep it, no ``state_dict`` holds it."""
    weights: Tensor
    kind: str
    n_cols: int
    valued: bool
    ref_size: int
    innerprod: Optional[float] = None
    sum_fill: Optional[float] = None
    polyfirst: Optional[int] = None
    polysecond: Optional[int] = None

    def to(self, device) -> "FrozenColumns":
        return replace(self, weights=self.weights.to(device))


if hasattr(torch.serialization, "add_safe_globals"):        # (torch.load's weights_only unpickler names the classes it builds)
    torch.serialization.add_safe_globals([FrozenColumns])


def _kind_of(predictor) -> str:
    """"cn5" / "cn7" for the predictors that take a frozen table; the refusals for the others."""
    from .model import (CNLinkPredictor3hopCNs, CNLinkPredictorbaselearn, CNLinkPredictorbaselearnablation,
                        CNLinkPredictorOringin)
    if isinstance(predictor, CNLinkPredictorbaselearnablation):
        raise ValueError("cn8 pools without column weights: it is batch-independent as it is, there is nothing to freeze")
    if isinstance(predictor, CNLinkPredictor3hopCNs):
        raise NotImplementedError("cn6 normalises with two column tables and nip: freezing it is not built")
    if isinstance(predictor, CNLinkPredictorOringin):
        return "cn5"
    if isinstance(predictor, CNLinkPredictorbaselearn):
        return "cn7"
    raise TypeError(f"freeze_columns takes a cn5 or cn7 predictor, got {type(predictor).__name__}")


def baked_values(predictor, kind: str, args=None) -> dict:
    """What a table of ``kind`` bakes in, read from the predictor (and ``args``) now: the fields ``set_frozen_columns`` compares."""
    if kind == "cn5":
        return dict(innerprod=float(predictor.innerprod.detach().reshape(-1)[0].item()))
    out = dict(polyfirst=int(predictor.polyfirst), polysecond=int(predictor.polysecond))
    if args is not None:
        out["sum_fill"] = float(args.sum)
    return out


@torch.no_grad()
def freeze_columns(predictor, adj, adj2, ref_edges: Tensor, args=None) -> FrozenColumns:
    """The column weights ``predictor`` forms in eval mode for the ONE batch ``ref_edges`` (int64 [n, 2], the layout
    ``score_edges`` takes; 1 <= n < 2 ** ``ops.HIST_FIELD_BITS``), bit for bit: for cn5 with the stored ``innerprod`` (the
    order-exact column sums included when it is non-zero), for cn7 with ``args.sum`` and ``polyfirst`` / ``polysecond``.
    ``adj2`` given: the pattern route (``adjoverlap``); ``adj2=None``: the walk route (``get_cn1_cn2``), the table is then
    "valued".  No embeddings are needed.  The table is a clone: the weights entries write in place over the histogram scratch."""
    from .utils import adjoverlap, fuse, get_cn1_cn2
    kind = _kind_of(predictor)
    if predictor._sharded:
        raise RuntimeError("an edge-sharded predictor sums its histograms over the ranks: freeze on an unsharded one")
    if predictor.training:
        raise RuntimeError("freeze_columns takes the eval-mode weights; call predictor.eval() first")
    if not isinstance(ref_edges, Tensor) or ref_edges.dim() != 2 or ref_edges.shape[1] != 2 or ref_edges.dtype != torch.int64:
        raise ValueError("ref_edges must be an int64 [n, 2] tensor")
    n = int(ref_edges.shape[0])
    if not 1 <= n <= ops.MAX_BATCH:
        raise ValueError(f"the reference batch is ONE batch of 1 .. {ops.MAX_BATCH} candidates (the histogram field width), got {n}")
    if kind == "cn7" and args is None:
        raise ValueError("cn7's column weights read args.sum: pass args")
    e = ref_edges.t().contiguous()
    adj.warm(walk=adj2 is None)
    if adj2 is not None:
        adj2.complete()
    handles = get_cn1_cn2(adj, e) if adj2 is None else (adjoverlap(adj, adj, e), adjoverlap(adj, adj2, e))
    st = fuse(*handles, e, None, adj=adj)
    w = predictor._batch_weights(st, args).clone()
    st.check_status()
    return FrozenColumns(weights=w, kind=kind, n_cols=int(st.N), valued=bool(st.walk), ref_size=n,
                         **baked_values(predictor, kind, args))
