"""Training-free link heuristics on the intersection machinery: common-neighbour count, Adamic-Adar, resource allocation,
Jaccard and preferential attachment — the baselines of every table in the OCN / NCN line of papers — and their 2-hop
counterparts over N(i) ∩ pattern(adj2 row j) ("higher-order common neighbours" without a model).

Every score of a candidate (i, j) is a sum of a per-node weight over a set of common neighbours, so one HIP kernel
(``ops.cn_node_sums``: intersection and sum in one pass, no flags, no histogram) produces all of them from a [N, 4] node
table: a candidate's sum adds its members in ascending column order, one fp32 add each, starting from 0.  The table is
evaluated with torch on the CPU in fp32 — a device ``logf`` is not correctly rounded and the table must be reproducible
bit for bit (``model.chebyshev_diag`` takes the same route for the same reason) — and uploaded once per adjacency.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import ops
from .pipeline import RunAhead
from .sparse import SparseTensor
from .utils import PermIterator, _endpoints

KINDS = ("cn", "aa", "ra", "jaccard", "pa", "cn2", "aa2", "ra2")
TWO_HOP = ("cn2", "aa2", "ra2")


def node_table(adj: SparseTensor, node_weight: Optional[Tensor] = None) -> Tensor:
    """The [N, 4] fp32 node table {aa weight, ra weight, user0, user1} of ``adj`` on its device.  deg[k] = the stored length
    of row k; aa = 1 / log(deg) where deg >= 2, ra = 1 / deg where deg >= 1, else 0 — both formed on the CPU in fp32.
    ``node_weight`` ([N] or [N, 2] fp32) fills the user columns.  Without user columns the table is cached on the adjacency,
    as its bit rows are, behind an event that the streams of later readers wait for; with them it is built per call."""
    n = adj.size(1)
    if adj.size(0) != n:
        raise ValueError("link heuristics need a square adjacency")
    dev = adj.device()
    if not torch.device(dev).type == "cuda":
        raise ops._lib.OcnHipError("node_table: expected an adjacency on a CUDA/HIP device — ocn_amd has no CPU path")
    if node_weight is None:
        cached = getattr(adj, "_node_table", None)
        if cached is not None:
            adj._await("node_table")
            return cached
    deg = (adj._rowptr[1:] - adj._rowptr[:-1]).cpu()
    degf = deg.to(torch.float32)
    table = torch.zeros(n, 4, dtype=torch.float32)
    table[:, 0] = torch.where(deg >= 2, 1.0 / torch.log(degf), torch.zeros(()))
    table[:, 1] = torch.where(deg >= 1, 1.0 / degf, torch.zeros(()))
    if node_weight is not None:
        nw = node_weight.detach()
        if nw.dtype != torch.float32 or nw.dim() not in (1, 2) or nw.shape[0] != n or (nw.dim() == 2 and nw.shape[1] != 2):
            raise ValueError(f"node_weight must be float32 [{n}] or [{n}, 2], got {nw.dtype} {tuple(nw.shape)}")
        table[:, 2:2 + (1 if nw.dim() == 1 else 2)] = nw.cpu().reshape(n, -1)
        return table.to(dev)
    adj._node_table = table.to(dev)
    adj._published("node_table")
    return adj._node_table


def _sums(adj: SparseTensor, adj2: Optional[SparseTensor], edges: Tensor, w: Tensor, wsd: Optional[dict]):
    """One ``ops.cn_node_sums`` launch (behind the order launch of a large batch) for ``edges`` [2, B].  T1 = ``adj`` and
    T2 = ``adj2`` go as bit rows where the adjacency has them (``SparseTensor.bit_rows`` / ``.probed_bit_rows``), else as
    CSR; T1's row pointers always go along: the kernel reads the target's degree from them."""
    src, dst = _endpoints(edges, "edges")
    bm2 = csr2 = None
    if adj2 is not None:
        if adj2.sparse_sizes() != adj.sparse_sizes():
            raise ValueError("adj and adj2 differ in size")
        bm2 = adj2.probed_bit_rows(dst)
        csr2 = None if bm2 is not None else (adj2._rowptr, adj2._col)
    bm1 = adj.bit_rows()
    return ops.cn_node_sums(adj._rowptr, adj._col, (adj._rowptr, adj._col), csr2, src, dst, w, t1_bitmap=bm1, t2_bitmap=bm2,
                            order=ops.batch_order(src, adj.size(0), wsd), wsd=wsd, n_cols=adj.size(1))


def _check_kinds(kinds: Sequence[str], adj2) -> Tuple[str, ...]:
    kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
    for k in kinds:
        if k not in KINDS:
            raise ValueError(f"unknown heuristic {k!r}: one of {KINDS}")
        if k in TWO_HOP and adj2 is None:
            raise ValueError(f"heuristic {k!r} intersects with the rows of adj2, which is None")
    return kinds


def link_heuristics(adj: SparseTensor, adj2: Optional[SparseTensor], edges: Tensor, kinds: Sequence[str] = KINDS,
                    node_weight: Optional[Tensor] = None, wsd: Optional[dict] = None) -> Tensor:
    """Scores of the candidates ``edges`` ([2, B] int64, the layout of ``tar_ei``): fp32 [B, len(kinds)], a column per kind.

    cn / cn2: |N(i) ∩ N(j)| and |N(i) ∩ pattern(adj2 row j)| as fp32 (``adj2``: the project's A², diagonal included, or
    any other SparseTensor); aa, ra, aa2, ra2: the sums of 1 / log deg(k) and 1 / deg(k) over those sets, members added in
    ascending column order; jaccard = fl(cn) / fl(d_i + d_j - cn), one fp32 division of two exactly converted integers
    (0 where the union is empty); pa = fl(d_i) · fl(d_j).  One kernel launch (two with the processing order of a batch of
    ``ops.sort_edges_min_batch`` candidates or more); ``wsd``: a scratch dictionary reused from batch to batch."""
    kinds = _check_kinds(kinds, adj2)
    need2 = any(k in TWO_HOP for k in kinds)
    s1, s2, c1, c2, deg = _sums(adj, adj2 if need2 else None, edges, node_table(adj, node_weight), wsd)
    cols = []
    for k in kinds:
        if k in ("cn", "cn2"):
            cols.append((c1 if k == "cn" else c2).to(torch.float32))
        elif k in ("aa", "ra"):
            cols.append(s1[:, 0 if k == "aa" else 1])
        elif k in ("aa2", "ra2"):
            cols.append(s2[:, 0 if k == "aa2" else 1])
        elif k == "pa":
            cols.append(deg[:, 0] * deg[:, 1])
        else:
            # jaccard: the union's size as an integer.  The quotient of two integers below 2^24 is either an fp32 rounding
            # midpoint exactly or at least 2^-49 (relative) away from one, so the fp64 quotient rounded to fp32 IS the correctly
            # rounded fp32 division — whatever the device's own fp32 division rounds like
            union = deg[:, 0].to(torch.int64) + deg[:, 1].to(torch.int64) - c1
            q = (c1.to(torch.float64) / union.clamp(min=1).to(torch.float64)).to(torch.float32)
            cols.append(torch.where(union > 0, q, torch.zeros_like(q)))
    if not cols:
        return s1.new_zeros(s1.shape[0], 0)
    return torch.stack(cols, dim=1)


def weighted_cn(adj: SparseTensor, adj2: Optional[SparseTensor], edges: Tensor, node_weight: Tensor,
                wsd: Optional[dict] = None) -> Tuple[Tensor, Tensor]:
    """Σ of a node score over the common neighbours: (sum over N(i) ∩ N(j), sum over N(i) ∩ pattern(adj2 row j)), each
    [B, 2] for the user columns of ``node_weight`` ([N] fills the first one; without ``adj2`` the second sum is zero)."""
    if node_weight is None:
        raise ValueError("weighted_cn needs node_weight")
    s1, s2, _, _, _ = _sums(adj, adj2, edges, node_table(adj, node_weight), wsd)
    return s1[:, 2:].clone(), s2[:, 2:].clone()


@torch.no_grad()
def score_edges_heuristic(adj: SparseTensor, adj2: Optional[SparseTensor], edges: Tensor, batch_size: int, kind: str,
                          run_ahead: int = 6) -> Tensor:
    """One heuristic for ``edges`` [n, 2] (the layout of ``split_edge[...]['edge']``), batched like
    ``PermIterator(.., training=False)`` as ``pipeline.score_edges`` is; returns a [n] fp32 tensor on the device, which
    ``evaluate.Evaluator.eval`` takes as it is.  The split is bounds-checked once, the caches (bit rows, node table) are
    built before the loop, and the host stays at most ``run_ahead`` batches ahead of the GPU.  One stream; dealing the
    batches over several GPUs is not built for this loop."""
    (kind,) = _check_kinds((kind,), adj2)
    if edges.dim() != 2 or edges.shape[1] != 2:
        raise ValueError("edges must be [n, 2]")
    if edges.shape[0] == 0:
        return torch.zeros(0, dtype=torch.float32, device=edges.device)
    need2 = kind in TWO_HOP
    adj.warm(walk=False)
    node_table(adj)
    if need2:
        adj2.complete()
    wsd: dict = {}
    outs, window = [], RunAhead(run_ahead, edges.device)
    with ops.prevalidated(edges[:, 0], edges[:, 1], adj.size(0), adj.size(0)):
        for perm in PermIterator(edges.device, edges.shape[0], batch_size, training=False):
            window.wait()
            outs.append(link_heuristics(adj, adj2 if need2 else None, edges[perm].t(), (kind,), wsd=wsd)[:, 0])
            window.mark()
    return torch.cat(outs, dim=0)
