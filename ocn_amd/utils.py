"""Drop-in for the hot-path names of the reference's ``utils.py``.

``adjoverlap`` (utils.py:248-285), ``PermIterator`` (utils.py:8-36), ``sparse_tensor_multiply`` /
``block_matrix_multiply`` (utils.py:287-329) keep their signatures; ``get_cn1_cn2`` is the pygho
route of the ppa / citation2 drivers (NeighborOverlap_large_ppa.py:147-173).  ``adjoverlap`` and
``get_cn1_cn2`` return lazy :class:`CNBatch` handles instead of materialised [B, N] SparseTensors;
the predictors in ``ocn_amd.model`` recognise them and run the fused HIP path, ``.materialize()``
yields the explicit matrix for inspection and parity tests.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import ops
from .sparse import SparseTensor


class PermIterator:
    """Batch index iterator (utils.py:8-36): ``randperm`` + drop-last when training, ``arange`` +
    ragged tail kept in eval."""

    def __init__(self, device, size, bs, training=True) -> None:
        self.bs = bs
        self.training = training
        self.idx = torch.randperm(size, device=device) if training else torch.arange(size, device=device)

    def __len__(self):
        return (self.idx.shape[0] + (self.bs - 1) * (not self.training)) // self.bs

    def __iter__(self):
        self.ptr = 0
        return self

    def __next__(self):
        if self.ptr + self.bs * self.training > self.idx.shape[0]:
            raise StopIteration
        ret = self.idx[self.ptr:self.ptr + self.bs]
        self.ptr += self.bs
        return ret


def _check_batch(tarei: Tensor, name: str = "tarei") -> None:
    if tarei.dim() != 2 or tarei.shape[0] != 2:
        raise ValueError(f"{name} must be [2, B]")


def _endpoints(tarei: Tensor, name: str = "tarei") -> Tuple[Tensor, Tensor]:
    """(src, dst) of a candidate batch ``tarei`` [2, B], as the contiguous int64 vectors the kernels read."""
    _check_batch(tarei, name)
    return tarei[0].to(torch.int64).contiguous(), tarei[1].to(torch.int64).contiguous()


def _check_hop3(adj: SparseTensor, adj2: SparseTensor, tarei: Tensor) -> None:
    _check_batch(tarei)
    if adj.size(0) != adj.size(1):
        raise ValueError("the 3-hop common neighbours need a square adjacency")
    if tuple(adj2.sparse_sizes()) != tuple(adj.sparse_sizes()):
        raise ValueError("adjoverlap_3hop: adj2 must be adj @ adj, of adj's size")


def _a2_bit_rows(adj2: SparseTensor, dst: Tensor) -> Tensor:
    """Bit rows of A² for the A³-free cn3 pass: the ones this batch may probe (``SparseTensor.probed_bit_rows``, completing a
    small graph's product as the batch's flag pass does); else built from the CSR where they fit."""
    bits = adj2.probed_bit_rows(dst, row_lengths=True)
    if bits is None:
        bits = adj2.bit_rows()
    if bits is None:
        raise ValueError("the A³-free cn6 route needs dense bit rows of A², and this adj2 has none (it exceeds "
                         "ops.a1_bitmap_max_bytes and did not arrive with them); a materialised adj3 is still accepted")
    return bits


def _transposed(adj: SparseTensor, undirected: bool):
    """(rowptr, col) of Aᵀ and Σ_{k∈N(i)} |Aᵀ row k| per source i, the probe bound that sizes the work items of the cn3
    pass.  ``undirected``: A is symmetric — its own CSR and its cached ``neighbor_degree_sum``."""
    if undirected:
        return adj._rowptr, adj._col, adj.neighbor_degree_sum()
    at = adj.t()
    if getattr(adj, "_nds_t", None) is None:
        deg_t = at._rowptr[1:] - at._rowptr[:-1]
        adj._nds_t = torch.zeros(adj.size(0), dtype=torch.int64, device=deg_t.device).index_add_(
            0, adj._row64(), deg_t[adj._col.to(torch.int64)])
    return at._rowptr, at._col, adj._nds_t


def scratch_set_count() -> int:
    """Scratch sets a two-phase scoring loop rotates through (``predictor.begin``'s ``slot``, ``pipeline.GraphedPhases``)."""
    return max(2, int(ops.overlap_depth), int(ops.overlap_depth_small))


class _BatchState:
    """Every field the predictors and the scoring loops read of a batch state, with its "absent" value: a constructor
    assigns what its route produces, the rest reads as absent."""
    adj = ws = src = dst = order = cnt1 = cnt2 = None
    B = N = 0
    walk = False
    cls = pooled = None         # set by the predictor: class-major rows (ops.class_order; None = batch order), phase A's pools
    _cls_decided = False        # ... and whether it has decided that row order


class CNState(_BatchState):
    """Device state of one candidate batch after the intersection kernel: where each batch row
    starts (``off``), one flag byte per neighbour of the source node (bit 0: cn1 entry, bit 1: cn2
    entry), the walk counts of the valued route, the packed per-column histograms
    {n1, n2, n_union, walks}, and the integer CN counts."""
    t2 = None
    off = flags = wc = hist = status = scal = None
    rec = sched = None          # per-slot records and group costs the pattern route leaves for the pooling
    _hist_live = False          # the histogram is consumed (turned into weights in place) exactly once
    _sched_ready = False        # the pooling's visiting order was formed in phase A (prepare_schedule)
    sharded, shard_group = False, None

    def __init__(self, adj: SparseTensor, t1: Optional[SparseTensor], t2: Optional[SparseTensor],
                 tarei: Tensor, walk: bool = False, ws: Optional[dict] = None):
        self.src, self.dst = _endpoints(tarei)
        for t in (t1, t2):
            if t is not None and t.sparse_sizes() != adj.sparse_sizes():
                raise ValueError("adjoverlap: adjacency sizes differ")    # utils.py:164 assert
        if walk and adj.size(0) != adj.size(1):
            raise ValueError("get_cn1_cn2 needs a square adjacency")
        self.adj, self.walk, self.t2 = adj, walk, t2
        self.ws = ws                           # a predictor's scratch cache: this state is then transient
        self.B = self.src.numel()
        self.N = adj.size(1)
        ops.check_edges(self.src, self.dst, adj.size(0), adj.size(0) if walk else t1.size(0))
        # per-slot records the intersection pass leaves for the pooling (pattern route)
        self.rec = None if (walk or self.B == 0) else ops.buf(ws, "rec", (self.B, ops.REC_WORDS), torch.int64, self.src.device)
        # ... and what each group of ops.SCHED_GROUP slots will cost the pooling, for its longest-first schedule (+ room for the schedule)
        self.sched = (ops.buf(ws, "sched", ops.sched_words(self.B), torch.int32, self.src.device)
                      if (self.rec is not None and ops.heavy_first and self.B >= ops.sort_edges_min_batch) else None)
        # T2: the bit rows this batch may probe, the row pointers it has (rows on demand: none), the column ids unless deferred
        csr2 = bm2 = None
        if t2 is not None and not walk:
            bm2 = t2.probed_bit_rows(self.dst, row_lengths=True)
            csr2 = (t2.rowptr_formed(), t2._col if (t2.col_materialized() or bm2 is None) else None)
        # ... and whether T2 is certified as the complete A·A of this symmetric adjacency: stored candidates then read no T2
        certified = bool(csr2 is not None and ops.t2_cover and t2.covers(adj))
        (self.order, self.off, self.flags, self.wc, self.hist, self.cnt1, self.cnt2, self.status, self.scal) = ops.cn_flags(
            adj._rowptr, adj._col, None if walk else (t1._rowptr, t1._col), csr2, self.src, self.dst, self.N,
            adj.max_rowcount(), walk=walk, t2_bitmap=bm2, wsd=ws,
            nds=adj.neighbor_degree_sum() if (walk and ops.walk_two_sided) else None,
            t1_bitmap=None if walk else t1.bit_rows(), rec=self.rec, sched=self.sched, t2_certified=certified)
        self._hist_live = True

    @classmethod
    def from_materialized(cls, adj: SparseTensor, cn1: SparseTensor, cn2: SparseTensor, tarei: Tensor,
                          ws: Optional[dict] = None) -> "CNState":
        """Batch state from two explicit [B, N] matrices, as the reference's own ``adjoverlap`` / ``get_cn1_cn2`` return
        them (every row e a subset of N_adj(tarei[0][e]); cn1 values 1.0; cn2 values 1.0 or walk counts).  A format
        conversion in torch ops (searchsorted into the source rows), not a hot path: the handles of
        ``ocn_amd.utils.adjoverlap`` skip it."""
        st = cls.__new__(cls)
        st.adj, st.ws = adj, ws
        st.src, st.dst = _endpoints(tarei)
        st.B, st.N = st.src.numel(), adj.size(1)
        dev = st.src.device
        if tuple(cn1.sizes()) != (st.B, st.N) or tuple(cn2.sizes()) != (st.B, st.N):
            raise ValueError("cn1 / cn2 must be [B, N] with B = tar_ei.shape[1], N = adj.size(1)")
        ops.check_edges(st.src, st.dst, adj.size(0), adj.size(0))
        st.off = ops.edge_offsets(adj._rowptr, st.src)
        total = int(st.off[-1])
        st.flags = torch.zeros(max(total, 1), dtype=torch.uint8, device=dev)
        rows_sel = adj[st.src]                                    # row e = N(src[e]), columns ascending
        r_s, c_s, _ = rows_sel.coo()
        key_s = r_s * st.N + c_s                                  # ascending: position p of the flag buffer
        v2 = cn2.storage.value()
        st.walk = bool(v2 is not None and v2.numel() and bool((v2 != 1).any()))
        st.wc = torch.zeros(max(total, 1), dtype=torch.int32, device=dev) if st.walk else None
        for bit, m in ((1, cn1), (2, cn2)):
            r, c, v = m.coo()
            key = r * st.N + c
            pos = torch.searchsorted(key_s, key).clamp_(max=max(key_s.numel() - 1, 0))
            if key.numel() and not bool((key_s[pos] == key).all()):
                raise NotImplementedError("cn1 / cn2 entries outside the source rows of `adj` cannot be expressed as CN flags")
            if bit == 2 and v is not None:                        # explicit zeros (pygho Hadamard) are no entries
                keep = v != 0
                pos, v = pos[keep], v[keep]
            st.flags[pos] |= bit
            if bit == 2 and st.walk:
                st.wc[pos] = v.to(torch.int32)
        f = st.flags[:total].to(torch.int64)
        e_of = r_s
        st.cnt1 = torch.zeros(st.B, dtype=torch.int64, device=dev).index_add_(0, e_of, f & 1).to(torch.int32)
        st.cnt2 = torch.zeros(st.B, dtype=torch.int64, device=dev).index_add_(0, e_of, (f >> 1) & 1).to(torch.int32)
        z = torch.zeros(st.N, dtype=torch.int64, device=dev)
        n1 = z.clone().index_add_(0, c_s, f & 1)
        n2 = z.clone().index_add_(0, c_s, (f >> 1) & 1)
        nu = z.clone().index_add_(0, c_s, (f != 0).to(torch.int64))
        walks = z.clone().index_add_(0, c_s, st.wc[:total].to(torch.int64)) if st.walk else z
        st.hist = torch.stack([n1 | (n2 << ops.HIST_FIELD_BITS) | (nu << (2 * ops.HIST_FIELD_BITS)), walks], dim=1).contiguous()
        st.status = torch.zeros(4, dtype=torch.int32, device=dev)
        st.scal = torch.zeros(4, dtype=torch.int32, device=dev)
        st._hist_live = True
        return st

    @classmethod
    def hop3(cls, adj: SparseTensor, adj2: SparseTensor, tarei: Tensor, undirected: bool = True, off: Optional[Tensor] = None,
             order: Optional[Tensor] = None) -> "CNState":
        """The (A, A³) pass without a stored A³: the state ``CNState(adj, adj3, None, tarei)`` leaves for adj3 = the pattern
        of A·A·A, from ``adj`` and the bit rows of ``adj2 = adj @ adj`` (``ops.cn3_flags``).  ``off`` / ``order``: those of
        the batch's (A, A, A²) pass, which has then checked the edges; standing alone the state forms its own."""
        _check_hop3(adj, adj2, tarei)
        st = cls.__new__(cls)
        st.adj = adj
        st.src, st.dst = _endpoints(tarei)
        st.B, st.N = st.src.numel(), adj.size(1)
        if off is None:
            ops.check_edges(st.src, st.dst, adj.size(0), adj.size(0))
            off = ops.edge_offsets(adj._rowptr, st.src)
            order = ops.batch_order(st.src, adj.size(0))
        st.off, st.order = off, order
        bits = _a2_bit_rows(adj2, st.dst)
        rowptr_t, col_t, nds = _transposed(adj, undirected)
        st.flags, st.hist, st.cnt1, st.status = ops.cn3_flags(adj._rowptr, adj._col, rowptr_t, col_t, bits, st.src, st.dst, st.N,
                                                              off, order, adj.max_rowcount(), nds=nds)
        st.scal = torch.zeros(4, dtype=torch.int32, device=st.src.device)
        st._hist_live = True
        return st

    def mark_sharded(self, group) -> None:
        self.sharded, self.shard_group = True, group       # one rank's slice: histograms are summed over ``group``

    def check_status(self) -> None:
        """Raise for the error bits the intersection pass left for this batch (one host sync; ocn_hip.h: OCN_ST_*)."""
        bits = int(self.status[0].item())
        if bits:
            self.status[3:].zero_()
            raise RuntimeError(ops.status_message(bits))

    def hist_counts(self) -> Tensor:
        """int64 [N, 4] = {n1, n2, n_union, walk-count sum} per column."""
        assert self._hist_live, "histogram already consumed"
        return ops.hist_counts(self.hist)

    def weights_cn5(self, innerprod: Tensor) -> Tensor:
        assert self._hist_live, "histogram already consumed"
        self._hist_live = False
        s2, scal = None, self.scal                   # zeroed with the batch's other scratch (ops.cn_flags)
        if ops.colsum_wanted(innerprod):
            # innerprod != 0 (a trained checkpoint): S2 summed entry by entry in the reference's order
            run = lambda init: ops.cn_colsum_exact(self.adj._rowptr, self.adj._col, self.src, self.off, self.flags, None,
                                                   self.wc, self.hist, innerprod, scal, self.ws, s2_init=init)[0]
            if self.sharded:
                from .dist import ring_colsum          # an edge shard continues the chains of the ranks before it
                s2 = ring_colsum(run, self.hist.shape[0], self.hist.device, self.shard_group)
            else:
                s2 = run(None)
        return ops.cn_weights_cn5(self.hist, innerprod, valued=self.walk, wsd=self.ws, s2_exact=s2, scal=scal)

    def weights_cn7(self, sum_fill: float, diag1: Optional[Tensor] = None, diag2: Optional[Tensor] = None) -> Tensor:
        assert self._hist_live, "histogram already consumed"
        self._hist_live = False
        return ops.cn_weights_cn7(self.hist, sum_fill, diag1, diag2)

    def gather(self, weights: Tensor, h: Tensor, order: Optional[Tensor] = None, out_row: Optional[Tensor] = None,
               rowsum: Optional[Tensor] = None, cap=None, mult: Optional[Tensor] = None):
        """(xcn1, xcn2, x_i * x_j); ``order`` overrides the processing order, ``out_row`` sends batch row e
        to output row out_row[e] (class-major rows for the heads, ops.class_order); ``rowsum`` = A·h for the cn7 weights
        (ocn_hip.h, ocn_cn_gather: candidates whose whole source row is cn2 copy their xcn2 row).  ``cap`` = (rows, seed): the
        capped pooling in its place (``ops.cn_gather_cap``; ``rowsum`` is dropped, ``mult`` receives the multipliers)."""
        if cap is not None:
            return ops.cn_gather_cap(self.adj._rowptr, self.adj._col, self.src, self.dst, self.off, self.flags, self.wc, weights, h,
                                     cap[0], cap[1], order=self.order if order is None else order,
                                     max_row_len=self.adj.max_rowcount(), wsd=self.ws, out_row=out_row, cnt1=self.cnt1,
                                     cnt2=self.cnt2, rec=self.rec if order is None else None,
                                     sched=self.sched if order is None else None, sched_ready=self._sched_ready, mult=mult)
        return ops.cn_gather(self.adj._rowptr, self.adj._col, self.src, self.dst, self.off,
                             self.flags, self.wc, weights, h, order=self.order if order is None else order,
                             max_row_len=self.adj.max_rowcount(), wsd=self.ws, out_row=out_row,
                             cnt1=self.cnt1, cnt2=self.cnt2, rec=self.rec if order is None else None,
                             sched=self.sched if order is None else None,
                             rowsum=None if self.walk else rowsum, sched_ready=self._sched_ready)

    def prepare_schedule(self, H: int) -> None:
        """Phase A of a scoring loop: the pooling's visiting order needs the intersection pass only."""
        if self.sched is not None and self.rec is not None and ops.sched_groups(self.B, H):
            self._sched_ready = ops.gather_schedule(self.sched, self.B)

    def gather_backward(self, weights: Tensor, h: Tensor, g1: Tensor, g2: Tensor, g3: Tensor) -> Tensor:
        return ops.cn_gather_backward(self.adj._rowptr, self.adj._col, self.src, self.dst, self.off, self.flags,
                                      self.wc, weights, h, g1.contiguous(), g2.contiguous(), g3.contiguous(),
                                      order=self.order)

    def cn5_batch_innerprod(self) -> Tensor:
        """Σ (cn2 ⊙ ncn1) of this batch (model.py:2241-2244), from the integer column counts:
        every entry in both sets contributes 1/S1 of its column.  Pattern route only."""
        hc = self.hist_counts()
        if self.walk:
            # valued cn2: Σ over entries in both sets of walk count / S1[col] (host-side format code,
            # training only — the eval path never needs it)
            n1 = hc[:, 0]
            inv1 = torch.where(n1 >= 2, 1.0 / n1.clamp(min=1).to(torch.float32), torch.zeros((), device=n1.device))
            both = self.materialize(1)
            r, c, _ = both.coo()
            cn2 = self.materialize(2)
            key2 = cn2.coo()[0] * self.N + cn2.coo()[1]
            key1 = r * self.N + c
            idx = torch.searchsorted(key2, key1).clamp(max=max(key2.numel() - 1, 0))
            hit = (key2[idx] == key1) if key2.numel() else torch.zeros_like(key1, dtype=torch.bool)
            return (cn2.storage.value()[idx[hit]] * inv1[c[hit]]).sum()
        n1 = hc[:, 0]
        nb = n1 + hc[:, 1] - hc[:, 2]
        inv1 = torch.where(n1 >= 2, 1.0 / n1.clamp(min=1).to(torch.float32), torch.zeros((), device=n1.device))
        return (nb.to(torch.float32) * inv1).sum()

    def materialize(self, bit: int) -> SparseTensor:
        """[B, N] matrix of the entries whose flag has ``bit`` set; values 1.0, or the walk counts
        for bit 2 of the valued route (host-side format conversion for tests; not on the product
        path)."""
        row_sel = self.adj[self.src]
        r, c, _ = row_sel.coo()
        pos = torch.arange(r.numel(), device=r.device) - row_sel._rowptr[:-1][r] + self.off[:-1][r]
        keep = (self.flags[pos] & bit) != 0
        val = torch.ones(int(keep.sum()), device=r.device)
        if self.walk and bit == 2:
            val = self.wc[pos][keep].to(torch.float32)
        return SparseTensor(row=r[keep], col=c[keep], value=val, sparse_sizes=(self.B, self.N),
                            is_sorted=True, trust_data=True)


class CNBatch:
    """Lazy ``adjoverlap(adj1, adj2, tarei)``: rows N_adj1(tarei[0][e]) ∩ N_adj2(tarei[1][e]); or one
    half of ``get_cn1_cn2(adj, tedge)`` (``mode`` "walk1" / "walk2"); or ``adjoverlap_3hop(adj, adj2, tarei)`` (``mode``
    "hop3": rows N_adj(tarei[0][e]) ∩ N³(tarei[1][e]) from ``adj`` and ``adj2 = adj @ adj``)."""

    def __init__(self, adj1: SparseTensor, adj2: Optional[SparseTensor], tarei: Tensor, mode: str = "pattern",
                 undirected: bool = True):
        self.adj1, self.adj2, self.tarei, self.mode, self.undirected = adj1, adj2, tarei, mode, undirected
        self._state: Optional[CNState] = None
        self.fused: Optional["CNState3"] = None      # hop3: the batch state ``fuse3`` built with this handle (its status words)

    def sizes(self):
        return [self.tarei.shape[1], self.adj1.size(1)]

    def size(self, dim: int) -> int:
        return self.sizes()[dim]

    def device(self):
        return self.adj1.device()

    def _single(self) -> CNState:
        if self._state is None:
            if self.mode == "pattern":
                self._state = CNState(self.adj1, self.adj2, None, self.tarei)
            elif self.mode == "hop3":
                self._state = CNState.hop3(self.adj1, self.adj2, self.tarei, self.undirected)
            else:
                self._state = CNState(self.adj1, None, None, self.tarei, walk=True)
        return self._state

    def counts(self) -> Tensor:
        """Integer CN count per candidate edge (per-row count of non-zero entries)."""
        st = self._single()
        return st.cnt2 if self.mode == "walk2" else st.cnt1

    def materialize(self) -> SparseTensor:
        return self._single().materialize(2 if self.mode == "walk2" else 1)


class CNState3:
    """The 3-hop predictor's batch state: two intersection passes over the same candidates — (A, A, A²) and
    (A, A³) — sharing the row offsets (both walk the source rows of A).  ``adj3=None``: the second pass runs without a
    stored A³, from ``adj`` and the bit rows of ``adj2`` (``CNState.hop3``; ``undirected=False`` reads ``adj.t()`` for the
    rows of Aᵀ) and leaves the same state."""

    def __init__(self, adj: SparseTensor, adj2: SparseTensor, adj3: Optional[SparseTensor], tarei: Tensor,
                 undirected: bool = True):
        if adj3 is None:
            _check_hop3(adj, adj2, tarei)
        self.a = CNState(adj, adj, adj2, tarei)
        self.b = (CNState(adj, adj3, None, tarei) if adj3 is not None
                  else CNState.hop3(adj, adj2, tarei, undirected, off=self.a.off, order=self.a.order))
        self.adj, self.B, self.N = adj, self.a.B, self.a.N

    @property
    def cnt3(self) -> Tensor:
        return self.b.cnt1

    def weights(self, innerprod: Tensor, sharded: bool = False):
        """``sharded``: the histograms were summed over edge shards — the closed form over the global counts is
        used (the order-exact sums need every rank's entries in order; cn5 chains them through ocn_amd.dist.ring_colsum,
        the two-stage cn6 does not)."""
        assert self.a._hist_live and self.b._hist_live, "histograms already consumed"
        self.a._hist_live = self.b._hist_live = False
        exact = None if sharded else (self.adj._rowptr, self.adj._col, self.a.src, self.a.off, self.a.flags, self.b.flags)
        return ops.cn_weights_cn6(self.a.hist, self.b.hist, innerprod, exact=exact, scal=self.a.scal)

    def gather(self, wa: Tensor, wb: Tensor, nip: Tensor, h: Tensor):
        return ops.cn_gather3(self.adj._rowptr, self.adj._col, self.a.src, self.a.dst, self.a.off, self.a.flags,
                              self.b.flags, wa, wb, nip, h, order=self.a.order)

    def gather_backward(self, wa: Tensor, wb: Tensor, nip: Tensor, h: Tensor, g1, g2, g3, g4) -> Tensor:
        return ops.cn_gather3_backward(self.adj._rowptr, self.adj._col, self.a.src, self.a.dst, self.a.off, self.a.flags,
                                       self.b.flags, wa, wb, nip, h, g1.contiguous(), g2.contiguous(), g3.contiguous(),
                                       g4.contiguous(), order=self.a.order)


def _same_edges(a: Tensor, b: Tensor) -> bool:
    """The drivers hand the SAME tensor to both adjoverlap calls and to the predictor
    (NeighborOverlap_large.py:121-159): identity (or the same view of one storage) needs no device
    comparison, anything else costs a torch.equal (one host sync)."""
    if a is b or (a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()
                  and a.dtype == b.dtype and a.device == b.device):
        return True
    return torch.equal(a, b)


def _check_one_batch(cns, tar_ei: Tensor, one_adjacency: str, cn1_on_adj: bool = True) -> None:
    """``cns`` (cn1, cn2[, cn3]) and ``tar_ei`` describe ONE batch: source rows from one adjacency (else, and unless the caller's
    ``cn1_on_adj`` holds, NotImplementedError(``one_adjacency``)), the same shapes, the same edges."""
    first = cns[0]
    if not cn1_on_adj or any(c.adj1 is not first.adj1 for c in cns[1:]):
        raise NotImplementedError(one_adjacency)
    exc = why = None
    if tar_ei.shape != first.tarei.shape or any(c.tarei.shape != first.tarei.shape for c in cns[1:]):
        exc, why = ValueError, "describe different numbers of candidate edges"
    elif ops.validate_indices and not (all(_same_edges(first.tarei, c.tarei) for c in cns[1:]) and _same_edges(first.tarei, tar_ei)):
        exc, why = NotImplementedError, "must be built from the same candidate edges"
    if exc is not None:
        raise exc(", ".join(("cn1", "cn2", "cn3")[:len(cns)]) + " and tar_ei " + why)


def fuse3(cn1: "CNBatch", cn2: "CNBatch", cn3: "CNBatch", tar_ei: Tensor) -> CNState3:
    """(cn1, cn2, cn3) = adjoverlap(adj, adj | adj2 | adj3, e) of one candidate batch; cn3 may be
    ``adjoverlap_3hop(adj, adj2, e)`` instead, built on the SAME ``adj2`` object as cn2: no A³ is needed then."""
    for c in (cn1, cn2, cn3):
        if not isinstance(c, CNBatch) or (c.mode != "pattern" and not (c is cn3 and c.mode == "hop3")):
            raise NotImplementedError("cn6 takes the handles returned by ocn_amd.utils.adjoverlap (cn3: or adjoverlap_3hop)")
    _check_one_batch((cn1, cn2, cn3), tar_ei, "cn1/cn2/cn3 must come from adjoverlap(adj, adj|adj2|adj3, e) of one adjacency",
                     cn1_on_adj=cn1.adj2 is cn1.adj1)
    if cn3.mode == "hop3":
        if cn3.adj2 is not cn2.adj2:
            raise NotImplementedError("adjoverlap_3hop(adj, adj2, e) must be built on the adj2 object of cn2 = adjoverlap(adj, adj2, e)")
        st = CNState3(cn1.adj1, cn2.adj2, None, cn1.tarei, undirected=cn3.undirected)
        cn3.fused = st
        return st
    return CNState3(cn1.adj1, cn2.adj2, cn3.adj2, cn1.tarei)


def fuse(cn1, cn2, tar_ei: Tensor, ws: Optional[dict] = None, adj: Optional[SparseTensor] = None) -> CNState:
    """One intersection pass for the (cn1, cn2) pair every driver builds from the same candidate
    edges (NeighborOverlap_large.py:76-82,121-159; NeighborOverlap_large_ppa.py:98-133).  Explicit [B, N]
    SparseTensors (what the reference's own adjoverlap returns) are accepted too, given the adjacency the
    predictor was called with: they are converted to the flag form (CNState.from_materialized)."""
    if isinstance(cn1, CNBatch) != isinstance(cn2, CNBatch):
        cn1 = cn1.materialize() if isinstance(cn1, CNBatch) else cn1
        cn2 = cn2.materialize() if isinstance(cn2, CNBatch) else cn2
    if isinstance(cn1, SparseTensor) and isinstance(cn2, SparseTensor):
        if not isinstance(adj, SparseTensor):
            raise TypeError("explicit cn1 / cn2 matrices need the adjacency (the predictor's `adj` argument) to be rebuilt "
                            "as CN flags")
        return CNState.from_materialized(adj, cn1, cn2, tar_ei, ws=None)
    if not isinstance(cn1, CNBatch) or not isinstance(cn2, CNBatch):
        raise TypeError("ocn_amd predictors take the CNBatch handles returned by ocn_amd.utils.adjoverlap "
                        "/ get_cn1_cn2, or explicit [B, N] SparseTensors")
    _check_one_batch((cn1, cn2), tar_ei, "cn1 and cn2 must select their source rows from the same adjacency")
    if cn1.mode == "walk1" and cn2.mode == "walk2":
        return CNState(cn1.adj1, None, None, cn1.tarei, walk=True, ws=ws)
    if cn1.mode != "pattern" or cn2.mode != "pattern":
        raise NotImplementedError("mixing adjoverlap and get_cn1_cn2 handles in one predictor call")
    return CNState(cn1.adj1, cn1.adj2, cn2.adj2, cn1.tarei, ws=ws)


class CN8State(_BatchState):
    """A cn8 batch on the pattern route: cn8 pools without column weights, so the batch needs no flags, histogram or
    weights — only the operands of ``ops.cn8_pool`` (intersection and pooling in one pass).  ``pool(h)`` runs it and leaves
    the integer CN counts in ``cnt1`` / ``cnt2`` — too late for a class order: born "batch order, decided"."""
    t1 = t2 = None
    _cls_decided = True

    def __init__(self, adj: SparseTensor, t1: SparseTensor, t2: SparseTensor, tarei: Tensor, ws: Optional[dict] = None):
        self.src, self.dst = _endpoints(tarei)
        for t in (t1, t2):
            if t.sparse_sizes() != adj.sparse_sizes():
                raise ValueError("adjoverlap: adjacency sizes differ")    # utils.py:164 assert
        self.adj, self.t1, self.t2, self.ws = adj, t1, t2, ws
        self.B, self.N = self.src.numel(), adj.size(1)

    def pool(self, h: Tensor):
        """(xcn1, xcn2, x_i * x_j) of the batch; sets ``cnt1`` / ``cnt2``."""
        adj, t1, t2 = self.adj, self.t1, self.t2
        if h.dim() != 2 or h.shape[0] != self.N:
            raise ValueError("h must have one row per column of the adjacency")
        # T2: the bit rows this batch may probe (``SparseTensor.probed_bit_rows``), else its CSR; T1: bit rows where they fit
        # (small dense graphs), else its CSR
        bm2 = t2.probed_bit_rows(self.dst)
        csr2 = None if bm2 is not None else (t2._rowptr, t2._col)
        bm1 = t1.bit_rows()
        self.order = ops.batch_order(self.src, adj.size(0), self.ws)
        x1, x2, xij, self.cnt1, self.cnt2 = self._pool_op(adj._rowptr, adj._col, (t1._rowptr, t1._col), csr2, self.src, self.dst, h,
                                                          t1_bitmap=bm1, t2_bitmap=bm2, order=self.order, wsd=self.ws, n_cols=self.N)
        return x1, x2, xij

    def _pool_op(self, rowptr, col, csr1, csr2, src, dst, h, **kw):
        return ops.cn8_pool(rowptr, col, csr1, csr2, src, dst, h, **kw)


class FrozenState(CN8State):
    """A cn5 / cn7 batch on the pattern route whose column weights are FROZEN (``ocn_amd.frozen``): with the table fixed, a
    candidate's pooled vectors depend on the candidate alone, so the batch needs what a cn8 batch needs plus the table —
    ``pool(h)`` runs ``ops.cn_pool_frozen`` (intersection and weighted pooling in one pass)."""
    weights = None

    def __init__(self, adj: SparseTensor, t1: SparseTensor, t2: SparseTensor, tarei: Tensor, weights: Tensor,
                 ws: Optional[dict] = None):
        super().__init__(adj, t1, t2, tarei, ws=ws)
        if tuple(weights.shape) != (self.N, 4):
            raise ValueError(f"the frozen table has {weights.shape[0]} columns, the adjacency {self.N}")
        self.weights = weights

    def _pool_op(self, rowptr, col, csr1, csr2, src, dst, h, **kw):
        return ops.cn_pool_frozen(rowptr, col, csr1, csr2, src, dst, h, self.weights, **kw)


def fuse8(cn1, cn2, tar_ei: Tensor, ws: Optional[dict] = None, weights: Optional[Tensor] = None) -> Optional[CN8State]:
    """The cn8 batch of two pattern-mode ``adjoverlap`` handles (same adjacency, same candidate edges: the checks of
    ``fuse``), or None for anything else — walk handles and explicit matrices take the flag form (``fuse``).  ``weights``: a
    frozen column-weight table — the batch is then the ``FrozenState`` of a cn5 / cn7 predictor."""
    if not (isinstance(cn1, CNBatch) and isinstance(cn2, CNBatch) and cn1.mode == "pattern" and cn2.mode == "pattern"):
        return None
    _check_one_batch((cn1, cn2), tar_ei, "cn1 and cn2 must select their source rows from the same adjacency")
    if weights is not None:
        return FrozenState(cn1.adj1, cn1.adj2, cn2.adj2, cn1.tarei, weights, ws=ws)
    return CN8State(cn1.adj1, cn1.adj2, cn2.adj2, cn1.tarei, ws=ws)


def adjoverlap(adj1: SparseTensor, adj2: SparseTensor, tarei: Tensor, filled1: bool = False,
               calresadj: bool = False, cnsampledeg: int = -1, ressampledeg: int = -1) -> CNBatch:
    """utils.py:248-285.  ``calresadj`` / sampling belong to the cn2-cn4 predictors, which no
    reference driver can call."""
    if calresadj or cnsampledeg > 0 or ressampledeg > 0:
        raise NotImplementedError("calresadj / neighbour sampling are outside the cn5/cn7 path (a bounded pooling cost with "
                                  "other semantics than the reference's cnsampledeg: predictor.set_cn_cap)")
    return CNBatch(adj1, adj2, tarei)


def adjoverlap_3hop(adj: SparseTensor, adj2: SparseTensor, tarei: Tensor, undirected: bool = True) -> CNBatch:
    """The cn3 argument of cn6 without a stored A³: rows N(i) ∩ N³(j) for (i, j) = tarei[:, e], N³ the pattern of A·A·A —
    what ``adjoverlap(adj, adj3, tarei)`` yields for a materialised adj3 — from ``adj`` and ``adj2 = adj @ adj``.  Neighbour k of
    i is an entry exactly when row k of Aᵀ shares a column with row j of A² (``ops.cn3_flags``), so ``adj2`` must have dense
    bit rows: the ones a product arrives with, or built from its CSR where they fit ``ops.a1_bitmap_max_bytes``.
    ``undirected=True`` assumes a symmetric ``adj`` (as ``update.insert_edges`` does) and reads A's own CSR for the rows of
    Aᵀ; ``undirected=False`` reads ``adj.t()``.  The handle goes to the cn6 predictor beside
    ``adjoverlap(adj, adj, e)`` and ``adjoverlap(adj, adj2, e)`` of the same ``adj2`` object; standing alone it answers
    ``.counts()`` and ``.materialize()``."""
    _check_hop3(adj, adj2, tarei)
    return CNBatch(adj, adj2, tarei, "hop3", undirected=bool(undirected))


def get_cn1_cn2(adj: SparseTensor, tedge: Tensor) -> Tuple[CNBatch, CNBatch]:
    """NeighborOverlap_large_ppa.py:147-173 / NeighborOverlapCitation2.py:78-104:
    cn1 = Ei ⊙ Ej, cn2 = Ei ⊙ (Ej · A) with the number of 2-walks as values — no global A²."""
    return CNBatch(adj, None, tedge, "walk1"), CNBatch(adj, None, tedge, "walk2")


def block_matrix_multiply(spadj: SparseTensor, block_size: int, fold_quirk: bool = False) -> SparseTensor:
    """utils.py:287-323: A·A for the dense ddi graph by the reference's tile loop — (row block, column block) products of
    ``block_size`` on the integer matrix cores over A as a dense 0/1 matrix (ops.dense_block_adj2).  Values are not
    formed: ``adjoverlap`` discards them (utils.py:150-151).

    ``fold_quirk=False`` (default, what every parity claim uses): the offset-correct pattern of A².
    ``fold_quirk=True``: the reference as written — each block's ``SparseTensor.from_dense`` carries block-local
    indices and is added without the block's offset (utils.py:318-321), so all blocks fold onto the
    top-left ``block_size`` corner (the CPU restatement used by the tests has the same switch)."""
    n = spadj.size(0)
    if spadj.size(1) != n:
        raise ValueError("block_matrix_multiply needs a square adjacency")
    if n <= ops.dense_adj2_max_nodes and block_size > 0 and block_size % 32 == 0 and spadj._col.is_cuda:
        rowptr, col, bits = ops.dense_block_adj2(spadj._rowptr, spadj._col, n, int(block_size), fold=fold_quirk)
        out = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(n, n))
        if not fold_quirk:
            out._bitmap = bits                   # dense bit rows of A²: one probe per membership test in the intersection
            out._published("bitmap")
            out._square_of = spadj               # the offset-correct, complete A @ A of this very object (SparseTensor.covers)
        return out
    if fold_quirk:
        raise NotImplementedError("fold_quirk needs the dense block route (n <= ops.dense_adj2_max_nodes, block_size % 32 == 0)")
    return SparseTensor.from_torch_sparse_coo_tensor(
        spadj.to_torch_sparse_coo_tensor() @ spadj.to_torch_sparse_coo_tensor(), False)


def sparse_tensor_multiply(spadj: SparseTensor, block_size: int = 1024) -> SparseTensor:
    """utils.py:326-329.  Which reading of utils.py:318-321 the unchanged ddi command gets is a process-wide
    switch: ``ops.adj2_fold_quirk`` (environment ``OCN_ADJ2_FOLD_QUIRK=1``) selects the reference as written — every
    block folded onto the top-left corner; the default is the intended offset-correct A²."""
    return block_matrix_multiply(spadj, block_size, fold_quirk=bool(ops.adj2_fold_quirk))
