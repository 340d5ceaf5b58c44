"""Host-side wrappers of the C ABI: argument validation + raw-pointer calls.

torch is used for device memory and the current stream only.  Every function here requires
CUDA(HIP) tensors and raises if the library is missing — there is no CPU path.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._lib import check, ptr, stream_ptr

FLAGS_NOSYNC_LIMIT = 1 << 30     # bytes of flag buffer we are willing to over-allocate to avoid a host sync
validate_indices = True          # bounds-check candidate edges on the host side (one sync per batch)
stage_timer = None               # optional object with .mark(name): bench.py records HIP events between stages
LN_WIDTHS = (16, 32, 64, 128, 256, 512)   # row widths of the lane-group kernels (LayerNorm, pooling backward)
a1_bitmap_max_bytes = int(os.environ.get("OCN_A1_BITMAP_MAX_BYTES", 64 << 20))   # keep A itself as dense bit rows too when they fit this (ogbl-ddi: 2.3 MB): cn1 membership = one probe
a2_bitmap_max_bytes = 16 << 30   # keep A·B also as dense bit rows when n_rows * n_cols / 8 fits this budget
skip_zero_rows = True            # heads: skip the layers whose pooled input row is all zero (class-major rows)
skip_zero_min_share = 0.15       # ... and when fewer than this share of the head rows could be skipped (probed asynchronously)
skip_zero_backoff = 32           # batches evaluated plainly before the share is probed again
skip_zero_min_batch = 4096       # below this the extra small launches cost more than the skipped rows save
walk_two_sided = True            # walk route: sweep each candidate from its cheaper endpoint (needs nds of the adjacency)
walk_share_min = 2               # walk route, B <= 4096: candidates sharing a source are swept together from this group size on (0 = never)
sort_edges_min_batch = 4096      # batches at least this large are processed in src order (L2 reuse of shared rows)
heavy_first = os.environ.get("OCN_HEAVY_FIRST", "1") != "0"   # ... and the pooling (H = 256) visits its slot groups longest first (ocn_cn_flags' gcost -> ocn_gather_schedule)
t2_cover = os.environ.get("OCN_T2_COVER", "1") != "0"         # intersection pass: a T2 certified as the full A·A of a symmetric A is not read for candidates that are stored entries of A (ocn_cn_flags_cover; same bits)
sched_segment = int(os.environ.get("OCN_SCHED_SEG", 0))        # ... inside segments of this many groups of an XCD's eighth (0 = the whole eighth)
overlap_depth = int(os.environ.get("OCN_OVERLAP_DEPTH", 4))   # scratch sets of a predictor = the most batches a scoring loop keeps in flight (round 4: four, with the pooling in phase A)
overlap_depth_small = int(os.environ.get("OCN_OVERLAP_DEPTH_SMALL", 8))   # ... and for batches of at most overlap_small_batch candidates (the drivers' 2 048: latency chains, not bandwidth — citation2 shape 5.58 -> 5.83 M edges/s, ppa unchanged)
overlap_small_batch = 4096
overlap_deep_max_batch = int(os.environ.get("OCN_OVERLAP_DEEP_MAX_BATCH", 1 << 30))   # ... which it does for batches up to this size: every size by
                                 # default.  Two intersection passes beside one pooling + heads pay where phase A is the longer one: the drivers'
                                 # 2 048-candidate walk-route batches (citation2 shape 3.96 -> 4.81 M edges/s) and ANY trained cn5 model, whose
                                 # order-exact column sums sit in phase A (collab shape 104 -> 126 M); a fresh model's large batches lose < 1 %
# Sharded scoring loops: where a batch's histogram all-reduce starts.  None = by the loop: in phase B (on the caller's stream, the
# class ordering and the NEXT batch's phase A on the other stream fill the wait) when the loop overlaps two streams — started from
# the side stream the collective cost 25 % of the step in the one-rank rehearsal (105 M against 140 M edges/s) — and in phase A (a
# whole step ahead, hidden behind the next intersection pass in stream order) on one stream.  OCN_REDUCE_IN_FINISH=0|1 forces it.
shard_reduce_in_finish = {"0": False, "1": True}.get(os.environ.get("OCN_REDUCE_IN_FINISH", ""), None)
_overlap_active = False          # set by pipeline.overlapped_steps while it runs phase A on side streams
phase_a_extras = os.environ.get("OCN_PHASE_A_EXTRAS", "1") != "0"   # unsharded loops: class ordering + pooling schedule in phase A (else phase B)
# Unsharded loops: the POOLING runs in phase A too, so that phase B — the caller's stream — is the heads alone.  Round 3's split
# (side streams: prep + intersection + weights, 0.2 ms of kernels each; caller's stream: pooling + heads, 0.32 ms back to back) left
# the caller's stream the critical one; with the pooling moved and three side streams (overlap_depth 4) one box gives collab
# 150.6 -> 158.4 M edges/s, ddi 70.3 -> 99.5 M, ppa 5.08 -> 6.05 M, citation2 4.82 -> 5.58 M, a trained cn5 model unchanged; same bits.
phase_a_pool = os.environ.get("OCN_PHASE_A_POOL", "1") != "0"
# Scoring loops: phase A / phase B of a scratch set as captured HIP graphs (pipeline.GraphedPhases).  OFF by default: measured on one
# box, the host's enqueue time per step drops 0.26 -> 0.07 ms (ddi / ppa / citation2 shapes; collab 0.20 -> 0.08) and the
# throughput does not move (ddi 97.0 vs 97.8 M edges/s, ppa 5.5 - 6.0 vs 6.0, citation2 5.8 vs 5.6 - 5.8, collab 155.5 both): the
# steps are bound on the device, as round 3 found for the one-stream capture.  For a caller whose host has other work to do.
graph_loops = os.environ.get("OCN_GRAPH_LOOPS", "0") == "1"
graph_loops_min_batches_per_set = 6                                # ... from this many batches per scratch set on (two eager uses + one capture each)
overlap_min_batch = 2048         # ... from this many candidates per batch (Cora-sized batches: the two event hand-offs cost more than the overlap gives)
overlap_streams = os.environ.get("OCN_ONE_STREAM", "0") != "1"   # scoring loops: phase A of batch t + 1 on a second stream beside phase B of batch t (pipeline.overlapped_steps)
share_full_rows = True           # cn7 on a dense graph: candidates whose whole source row is cn2 copy (A h)[source] (ocn_cn_gather `rowsum`)
deterministic_backward = os.environ.get("OCN_ATOMIC_BACKWARD", "0") != "1"   # pooling backward node by node in a fixed order (ocn_cn_gather_backward_det); else fp32 atomics


def loop_depth(batch) -> int:
    """Batches a scoring loop keeps in flight (= streams it uses) for batches of this size (None: unknown -> two)."""
    if batch is None or batch > overlap_deep_max_batch:
        return 2
    return max(2, int(overlap_depth_small if batch <= overlap_small_batch else overlap_depth))


def _on_device(fn):
    """Launch on the device of the operands.  ``stream_ptr()`` is the current stream of the CURRENT
    device; tensors living on another device (a predictor on cuda:1 in a process whose current device is
    cuda:0) would otherwise be handed to a kernel enqueued on the wrong GPU.  Tensors on different
    devices are an error, as they are for torch's own operators."""
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kw):
        idx = -1
        for a in args:
            if isinstance(a, Tensor) and a.is_cuda:
                if idx < 0:
                    idx = a.device.index
                elif a.device.index != idx:
                    raise RuntimeError(f"{fn.__name__}: operands on different devices (cuda:{idx}, cuda:{a.device.index})")
        if idx >= 0 and idx != torch._C._cuda_getDevice():
            with torch.cuda.device(idx):
                return fn(*args, **kw)
        return fn(*args, **kw)
    return wrapper


def _mark(name: str, flops: float = 0.0) -> None:
    if stage_timer is not None:
        stage_timer.mark(name, flops)


def _req(t: Tensor, dtype, name: str, ndim: Optional[int] = None) -> Tensor:
    if not isinstance(t, Tensor) or not t.is_cuda:
        raise _lib.OcnHipError(f"{name}: expected a CUDA/HIP tensor — ocn_amd has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name}: expected {ndim}-d, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


# A half-precision embedding table (``pipeline.embedding_table``): dtype -> the `fmt` of ocn_cn_gather_h16.  Such a table serves the
# eval pooling of cn5 / cn7 / cn8 (``cn_gather``) and nothing else; every other consumer of a table refuses it (``refuse_half_table``).
HALF_TABLE_FMT = {torch.bfloat16: 0, torch.float16: 1}


def is_half_table(t) -> bool:
    return isinstance(t, Tensor) and t.dtype in HALF_TABLE_FMT


def refuse_half_table(t, what: str) -> None:
    """TypeError where ``t`` is a bf16 / f16 table and ``what`` is built for fp32 rows only.  Reads the dtype alone: callable
    before anything touches the device."""
    if is_half_table(t):
        raise TypeError(f"{what} needs an fp32 (torch.float32) embedding table, got {t.dtype}: a bf16 / f16 table serves the "
                        "eval-mode, no-grad pooling of cn5 / cn7 / cn8 only — pass table.float()")


class Int8Table:
    """An int8 embedding table (``pipeline.embedding_table(h, "int8")``): ``rows`` int8 [N, Hp], ``scale`` float32 [N] and
    ``width`` = H <= Hp — what ``quantize_rows_i8(h)`` returns, the image a ``recommend.EmbeddingIndex`` keeps, so one resident
    copy serves retrieval and scoring (``from_index`` / ``EmbeddingIndex.from_table`` share storage).  The table it stands for
    is ``float()`` = ``rows[:, :H].float() * scale[:, None]``, one fp32 multiply per element; the eval pooling of cn5 / cn7 / cn8
    (``cn_gather``, ``cn_gather_cap``: ocn_cn_gather_q8) gives bit for bit what the fp32 entries give for that matrix.  A plain
    object with as much of a tensor's surface as a scoring loop reads: ``torch.save`` stores it, ``to(device)`` moves it."""
    requires_grad = False

    def __init__(self, rows: Tensor, scale: Tensor, width: int):
        if not isinstance(rows, Tensor) or rows.dtype != torch.int8 or rows.dim() != 2 or not rows.is_contiguous():
            raise ValueError("rows must be a contiguous int8 [N, Hp] matrix")
        if not isinstance(scale, Tensor) or scale.dtype != torch.float32 or scale.dim() != 1 or not scale.is_contiguous() \
                or scale.numel() != rows.shape[0]:
            raise ValueError(f"scale must be a contiguous float32 [{rows.shape[0]}] vector: one scale per row")
        if scale.device != rows.device:
            raise ValueError(f"rows live on {rows.device}, scale on {scale.device}")
        if isinstance(width, bool) or not isinstance(width, int) or not 1 <= width <= rows.shape[1]:
            raise ValueError(f"width must be an int in 1..{rows.shape[1]} (the columns of rows), got {width!r}")
        self.rows, self.scale, self.width = rows, scale, width

    @classmethod
    def from_index(cls, index) -> "Int8Table":
        """The table an ``EmbeddingIndex`` holds, on the same storage.  A ``normalize=True`` index holds the image of the
        normalised rows, which is not the table: ValueError."""
        if index.normalize:
            raise ValueError("an index made with normalize=True holds the unit-norm rows, not the embedding table")
        return cls(index.keys_q, index.kscale, index.width)

    shape = property(lambda self: torch.Size((self.rows.shape[0], self.width)))
    device = property(lambda self: self.rows.device)
    dtype = property(lambda self: torch.int8)
    is_cuda = property(lambda self: self.rows.is_cuda)

    def dim(self) -> int:
        return 2

    def contiguous(self) -> "Int8Table":
        return self

    def detach(self) -> "Int8Table":
        return self

    def new_zeros(self, *size, dtype=torch.float32) -> Tensor:
        return self.scale.new_zeros(*size, dtype=dtype)

    def float(self) -> Tensor:
        """The fp32 [N, H] matrix this table stands for."""
        return self.rows[:, :self.width].float() * self.scale[:, None]

    def float_rows(self, ids: Tensor) -> Tensor:
        """``float()[ids]`` without forming the whole matrix."""
        return self.rows[ids, :self.width].float() * self.scale[ids][:, None]

    def to(self, device) -> "Int8Table":
        return Int8Table(self.rows.to(device), self.scale.to(device), self.width)


if hasattr(torch.serialization, "add_safe_globals"):        # (torch.load's weights_only unpickler names the classes it builds)
    torch.serialization.add_safe_globals([Int8Table])


def is_compact_table(t) -> bool:
    """A table the eval pooling of cn5 / cn7 / cn8 alone reads: bf16 / f16 rows, or an ``Int8Table``."""
    return is_half_table(t) or isinstance(t, Int8Table)


def refuse_compact_table(t, what: str) -> None:
    """``refuse_half_table``, and the same refusal of an ``Int8Table``.  Reads the type alone."""
    refuse_half_table(t, what)
    if isinstance(t, Int8Table):
        raise TypeError(f"{what} needs an fp32 (torch.float32) embedding table, got an int8 table (Int8Table): an int8 table "
                        "serves the eval-mode, no-grad pooling of cn5 / cn7 / cn8 only — pass table.float()")


ST_CAP, ST_SCAN = 1, 2           # include/ocn_hip.h: OCN_ST_CAP, OCN_ST_SCAN (bits of status[0] and of the sticky status[3])
REC_WORDS = 4                    # include/ocn_hip.h: OCN_REC_WORDS (int64 words of a slot record)
SCHED_GROUP, SCHED_EIGHTHS, SCHED_MAX_EIGHTH = 4, 8, 65535     # include/ocn_hip.h: OCN_SCHED_* (the pooling's schedule)
SCHED_H = 256                    # the width whose pooling workgroups are the schedule's groups


def sched_words(B: int) -> int:
    """int32 words of a batch's ``sched`` buffer: the group costs of the intersection pass, then room for the visiting order."""
    return 2 * ((B + SCHED_GROUP - 1) // SCHED_GROUP)


def sched_groups(B: int, H: int) -> int:
    """Schedule groups of ``B`` candidates pooled at width ``H`` where a visiting order exists and is followed, else 0."""
    n, rest = divmod(B, SCHED_GROUP * SCHED_EIGHTHS)      # whole groups, the same number in every XCD's eighth
    return n * SCHED_EIGHTHS if (H == SCHED_H and rest == 0 and 0 < n <= SCHED_MAX_EIGHTH) else 0


def _total(t: Tensor) -> int:
    """The grand total of a scan read on the host.  Negative = OCN_SCAN_POISON: the scan's workspace was not zero on entry
    (ocn_hip.h, ocn_scan_workspace_bytes) — a Python error here, where round 3 ended in a GPU trap."""
    v = int(t.item())
    if v < 0:
        raise _lib.OcnHipError("scan workspace was not zero on entry (two launches in flight on one workspace?)")
    return v


def _scan_total(ptrs: Tensor, n: int, total: Optional[int], name: str, what: str) -> int:
    """``ptrs`` is a scan over ``n`` segments — one entry each and the total, else ValueError(``what``).  Returns the total:
    ``total`` where the caller has read it already, else read here (one host sync for an output size)."""
    if _req(ptrs, torch.int64, name, 1).numel() != n + 1:
        raise ValueError(what)
    return _total(ptrs[-1]) if total is None else int(total)


def _fill_pairs(off: Tensor, Q: int, total: Optional[int], device) -> Tuple[int, Tensor]:
    """The total of the ``off`` scan of ``Q`` queries and the int64 [T, 2] pair list a fill pass writes."""
    T = _scan_total(off, Q, total, "off", "off: one entry per query and the total")
    return T, torch.empty(T, 2, dtype=torch.int64, device=device)


def status_message(bits: int) -> str:
    return "; ".join(m for b, m in ((ST_CAP, "CN flag buffer capacity exceeded"),
                                    (ST_SCAN, "a scan workspace was not zero on entry: the batch's offsets are void")) if bits & b)


def _ws(n: int, device, wsd=None) -> Tensor:
    """The zeroed workspace of a scan over ``n`` items (ocn_hip.h, ocn_scan_workspace_bytes: the library hands it back zero)."""
    return buf(wsd, "scan_ws", int(_lib.lib().ocn_scan_workspace_bytes(n)) // 8 + 1, torch.int64, device, zero_init=True)


def buf(ws, name: str, shape, dtype, device, zero: bool = False, zero_init: bool = False) -> Tensor:
    """Scratch tensor.  ``ws`` = None: a fresh allocation (states the caller keeps: tests, materialize).
    ``ws`` = a dict owned by a predictor: the buffer is cached by (name, shape, dtype) and reused by the
    next batch — stream order makes that safe, and a dozen allocator round trips per batch disappear
    from the host's critical path.  ``zero``: cleared on every call; ``zero_init``: cleared when it is
    allocated only (workspaces the library hands back zero: ocn_hip.h, ocn_scan_workspace_bytes)."""
    shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    if ws is None:
        return (torch.zeros if (zero or zero_init) else torch.empty)(shape, dtype=dtype, device=device)
    key = (name, shape, dtype, str(device))
    t = ws.get(key)
    if t is None:
        t = ws[key] = (torch.zeros if zero_init else torch.empty)(shape, dtype=dtype, device=device)
    if zero:
        t.zero_()
    return t


def zero_regions(tensors) -> None:
    """One launch that zeroes every tensor of the list (contiguous, 4-byte element multiples)."""
    ts = [t for t in tensors if t is not None and t.numel()]
    if not ts:
        return
    n = len(ts)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    nbytes = (ctypes.c_int64 * n)(*[t.numel() * t.element_size() for t in ts])
    idx = ts[0].device.index
    if idx != torch._C._cuda_getDevice():
        with torch.cuda.device(idx):
            return zero_regions(ts)
    check(_lib.lib().ocn_zero_regions(ptrs, nbytes, n, stream_ptr()), "ocn_zero_regions")


@_on_device
def edge_offsets(rowptr: Tensor, src: Tensor, wsd=None) -> Tensor:
    _req(rowptr, torch.int64, "rowptr", 1)
    _req(src, torch.int64, "src", 1)
    B = src.numel()
    off = buf(wsd, "off", B + 1, torch.int64, src.device)
    ws = _ws(B, src.device, wsd)
    check(_lib.lib().ocn_edge_offsets(ptr(rowptr), ptr(src), B, ptr(off), ptr(ws), stream_ptr()),
          "ocn_edge_offsets")
    return off


@_on_device
def scan_i32(cnt: Tensor) -> Tensor:
    _req(cnt, torch.int32, "cnt", 1)
    n = cnt.numel()
    out = torch.empty(n + 1, dtype=torch.int64, device=cnt.device)
    ws = _ws(n, cnt.device)
    check(_lib.lib().ocn_scan_i32(ptr(cnt), n, ptr(out), ptr(ws), stream_ptr()), "ocn_scan_i32")
    return out


@_on_device
def check_edges(src: Tensor, dst: Tensor, n_src: int, n_dst: int) -> None:
    """Reference behaviour for an out-of-range node id is an IndexError from index_select; a raw
    kernel would fault instead, so the ids are checked here (costs one host sync)."""
    if not validate_indices or src.numel() == 0:
        return
    if (int(n_src), int(n_dst)) in getattr(_checked, "scopes", ()):      # inside ``prevalidated`` for an adjacency of this size
        return
    _req(src, torch.int64, "src", 1); _req(dst, torch.int64, "dst", 1)
    bad = torch.zeros(1, dtype=torch.int32, device=src.device)
    check(_lib.lib().ocn_check_edges(ptr(src), ptr(dst), src.numel(), int(n_src), int(n_dst), ptr(bad), stream_ptr()),
          "ocn_check_edges")
    if int(bad.item()):
        raise IndexError("candidate edge endpoint out of range for the adjacency")


import threading  # noqa: E402
_checked = threading.local()      # .scopes: (n_src, n_dst) of the splits validated by the ``prevalidated`` scopes of THIS thread


class prevalidated:
    """``with ops.prevalidated(src_all, dst_all, n_src, n_dst):`` — bounds-check a whole split of candidate
    edges once (one host sync), then run the batches inside without the per-batch check.  This is what
    ``pipeline.score_edges`` / ``score_mrr_split`` do: the check is hoisted out of the batch loop, the
    exception for a bad id is the same IndexError, raised before the first batch.  The waiver is scoped: it
    holds for the calling thread only and only for adjacencies of the validated size — another thread, or a call on a
    graph of another size inside the scope, is checked as usual (``validate_indices`` itself is not touched)."""

    def __init__(self, src: Tensor, dst: Tensor, n_src: int, n_dst: int):
        check_edges(src.contiguous(), dst.contiguous(), n_src, n_dst)
        self._key = (int(n_src), int(n_dst))

    def __enter__(self):
        if not hasattr(_checked, "scopes"):
            _checked.scopes = []
        _checked.scopes.append(self._key)
        return self

    def __exit__(self, *exc):
        _checked.scopes.remove(self._key)
        return False


HIST_FIELD_BITS = 21             # hist word 0 packs n1 | n2 << 21 | n_union << 42
MAX_BATCH = (1 << HIST_FIELD_BITS) - 1


def hist_counts(hist: Tensor) -> Tensor:
    """Decode the packed histogram [N,2] int64 into int64 [N,4] = {n1, n2, n_union, walks}."""
    m = (1 << HIST_FIELD_BITS) - 1
    p = hist[:, 0]
    return torch.stack([p & m, (p >> HIST_FIELD_BITS) & m, (p >> (2 * HIST_FIELD_BITS)) & m, hist[:, 1]], dim=1)


def _batch_ids(src: Tensor, dst: Tensor, hist: bool = False) -> int:
    """B of a batch's int64 id vectors (the intersection family's operand checks start here); ``hist``: the packed histogram bounds B."""
    _req(src, torch.int64, "src", 1); _req(dst, torch.int64, "dst", 1)
    B = src.numel()
    if dst.numel() != B:
        raise ValueError("src/dst length mismatch")
    if hist and B > MAX_BATCH:
        raise ValueError(f"candidate batch of {B} edges exceeds the histogram field width ({MAX_BATCH})")
    return B


def _t_tail(rp, col, bm: Optional[Tensor], nm: str, n_cols: int, like: Optional[int]):
    """What both operand forms end with: the bit rows fit the matrix and the columns, and the row count is that of the pass's
    other matrix (``like``; ``dst`` indexes both).  Returns (rowptr, col, rows) as they go to the library."""
    if bm is not None:
        _req(bm, torch.int32, nm.lower() + "_bitmap", 2)
        if (rp is not None and bm.shape[0] != rp.numel() - 1) or bm.shape[1] * 32 < n_cols:
            raise ValueError(f"{nm.lower()}_bitmap does not match the {nm} adjacency")
    rows = rp.numel() - 1 if rp is not None else bm.shape[0]
    if like is not None and rows != like:
        raise ValueError(f"T1 has {like} rows, T2 {rows}")
    return rp, col, rows


def _t_pair_or_bits(t, bm: Optional[Tensor], nm: str, n_cols: int, like: Optional[int] = None, optional: bool = False):
    """A matrix of ocn_cn8_pool / ocn_cn_node_sums: ``t`` = its whole (rowptr, col) pair — half a pair counts as none — and / or
    its bit rows ``bm``; with ``optional`` it may be left out altogether (all None)."""
    rp, col = (None, None) if t is None else t
    if rp is None or col is None:
        if bm is None:
            if optional:
                return None, None, None
            raise ValueError(f"{nm}: needs its CSR arrays or its bit rows")
        rp = col = None
    else:
        _req(rp, torch.int64, "rowptr" + nm, 1); _req(col, torch.int32, "col" + nm, 1)
    return _t_tail(rp, col, bm, nm, n_cols, like)


def _t_of_flag_pass(t, bm, nm: str, n_cols: int, like=None, rowptr_optional: bool = False, col_deferred: bool = False):
    """A matrix of ocn_cn_flags: both CSR arrays, except that beside bit rows the row pointers may be absent with
    ``rowptr_optional`` and the column ids with ``col_deferred``."""
    rp, col = t
    if rp is not None or bm is None or not rowptr_optional:
        _req(rp, torch.int64, "rowptr" + nm, 1)
    if col is not None or bm is None or not col_deferred:
        _req(col, torch.int32, "col" + nm, 1)
    return _t_tail(rp, col, bm, nm, n_cols, like)


def _order_arg(order: Optional[Tensor], B: int) -> None:
    if order is not None and _req(order, torch.int64, "order", 1).numel() != B:
        raise ValueError("order: one entry per candidate")


def _nds_arg(nds: Optional[Tensor], n: int) -> Optional[Tensor]:
    if nds is not None and _req(nds, torch.int64, "nds", 1).numel() != n:
        raise ValueError("nds does not match the adjacency")
    return nds


def _flag_capacity(B: int, max_deg_a: int, off: Tensor) -> int:
    """Entries of a batch's flag buffer: B * (longest row) while over-allocating beats a host sync, else the total read from ``off``."""
    bound = B * max(int(max_deg_a), 0)
    return bound if bound <= FLAGS_NOSYNC_LIMIT else _total(off[-1])


def _cn_operands(rowptrA, colA, t1, t2, bm1, bm2, src, dst, order, B: int, n_cols: int):
    """The leading arguments of ocn_cn_flags[_rec], ocn_cn8_pool and ocn_cn_node_sums (``t1`` / ``t2``: the checked (rowptr, col))."""
    return (ptr(rowptrA), ptr(colA), ptr(t1[0]), ptr(t1[1]), ptr(t2[0]), ptr(t2[1]),
            ptr(bm1), bm1.shape[1] if bm1 is not None else 0, ptr(bm2), bm2.shape[1] if bm2 is not None else 0,
            ptr(src), ptr(dst), ptr(order), B, n_cols)


@_on_device
def cn_flags(rowptrA: Tensor, colA: Tensor, t1: Optional[Tuple[Tensor, Tensor]],
             t2: Optional[Tuple[Tensor, Tensor]], src: Tensor, dst: Tensor, n_cols: int, max_deg_a: int,
             walk: bool = False, t2_bitmap: Optional[Tensor] = None, wsd=None, nds: Optional[Tensor] = None,
             t1_bitmap: Optional[Tensor] = None, rec: Optional[Tensor] = None, sched: Optional[Tensor] = None,
             t2_certified: bool = False):
    """Intersection pass.  ``walk=False``: flags of N(src) against the rows of dst in t1 (and t2).
    ``walk=True``: the pygho route on A itself (t1/t2 ignored): cn1 flags + walk counts; with ``nds``
    (``neighbor_degree_sum`` of A) every batch row is swept from its cheaper endpoint.
    ``rec`` (int64 [B, REC_WORDS], pattern route): receives the per-slot records ``cn_gather`` reads instead of walking
    order -> src / dst / off / counts -> rowptr.
    ``t2_certified``: t2 is the complete pattern of A·A and A equals its transpose (``SparseTensor.covers``: the caller's
    word, not checked here) — with ``ops.t2_cover`` on, candidates that are stored entries of A then read no T2; same outputs.
    Returns (order|None, off, flags, wc|None, hist[N,2] int64 packed, cnt1, cnt2|None, status, scal) — ``scal``
    is the zeroed int32[4] statistics scratch the weights stage of the same batch uses."""
    dev = src.device
    _req(rowptrA, torch.int64, "rowptrA", 1); _req(colA, torch.int32, "colA", 1)
    has_t2 = not walk and t2 is not None
    if not walk:
        *csr1, rows = _t_of_flag_pass(t1, t1_bitmap, "T1", n_cols)
        if t2 is None and t2_bitmap is not None:
            raise ValueError("t2_bitmap does not match the T2 adjacency")
        # (T2's row pointers: a product with rows on demand has none, and past the small-graph histogram the kernel reads none)
        *csr2, _ = (None, None, None) if not has_t2 else _t_of_flag_pass(
            t2, t2_bitmap, "T2", n_cols, like=rows, col_deferred=True, rowptr_optional=t2[0] is None and n_cols > small_graph_cols())
    B = _batch_ids(src, dst, hist=True)
    _mark("begin")
    if walk and 0 < B <= int(_lib.lib().ocn_walk_prep_max_batch()) and walk_share_min > 0:
        return _cn_flags_walk_small(rowptrA, colA, src, dst, n_cols, max_deg_a, wsd, nds)
    # processing order: candidates with the same / nearby source node share most of the rows they
    # gather, so visiting them together turns HBM row fetches into L2 hits (outputs stay in batch order)
    want_order = B >= sort_edges_min_batch
    n_src = rowptrA.numel() - 1
    order = buf(wsd, "order", B, torch.int64, dev) if want_order else None
    ows = (buf(wsd, "order_ws", int(_lib.lib().ocn_order_workspace_bytes(n_src)) // 8 + 1, torch.int64, dev, zero_init=True)
           if want_order else None)
    off = buf(wsd, "off", B + 1, torch.int64, dev)
    sws = _ws(B, dev, wsd)
    hist = buf(wsd, "hist", (n_cols, 2), torch.int64, dev)
    cnt1 = buf(wsd, "cnt1", B, torch.int32, dev)
    cnt2 = buf(wsd, "cnt2", B, torch.int32, dev) if (walk or has_t2) else None
    status = buf(wsd, "status", 4, torch.int32, dev, zero_init=True)     # [0] error bits of this batch; [1], [2] walk-route work tickets; [3] sticky error bits
    scal = buf(wsd, "scal", 4, torch.int32, dev)         # the column statistics word of the weights stage
    # the flag offsets, the counting phase of the order and the batch's resets: ONE launch (ocn_batch_prep)
    zs = [t for t in [hist, status[:3], scal] + ([cnt1, cnt2] if walk else []) if t is not None and t.numel()]     # (status[3]: sticky)
    if sched is not None:             # group costs for the pooling's schedule (ocn_hip.h: ocn_cn_flags `gcost`): first half of `sched`
        if rec is None or walk or _req(sched, torch.int32, "sched", 1).numel() < sched_words(B):
            raise ValueError("sched: int32[sched_words(B)] beside the slot records of the pattern route")
    zp = (ctypes.c_void_p * len(zs))(*[t.data_ptr() for t in zs])
    zb = (ctypes.c_int64 * len(zs))(*[t.numel() * t.element_size() for t in zs])
    check(_lib.lib().ocn_batch_prep(ptr(rowptrA), ptr(src), B, ptr(off), ptr(sws), n_src, ptr(ows), zp, zb, len(zs),
                                    stream_ptr()), "ocn_batch_prep")
    rec_in = want_order and rec is not None and not walk      # the scatter that orders the batch starts the slot records too
    if rec_in:
        _req(dst, torch.int64, "dst", 1)
        if _req(rec, torch.int64, "rec").numel() < REC_WORDS * B:
            raise ValueError("rec: int64 [B, REC_WORDS]")
        check(_lib.lib().ocn_order_by_node_finish_rec(ptr(src), ptr(dst), ptr(rowptrA), ptr(off), B, n_src, ptr(order), ptr(rec),
                                                      ptr(ows), stream_ptr()), "ocn_order_by_node_finish_rec")
    elif want_order:
        check(_lib.lib().ocn_order_by_node_finish(ptr(src), B, n_src, ptr(order), ptr(ows), stream_ptr()),
              "ocn_order_by_node_finish")
    cap = _flag_capacity(B, max_deg_a, off)
    flags = buf(wsd, "flags", max(cap, 1), torch.uint8, dev)
    wc = buf(wsd, "wc", max(cap, 1), torch.int32, dev) if walk else None
    chunk_off = rev_off = None
    if walk:
        nds = _nds_arg(nds if walk_two_sided else None, n_src)
        chunk_off = buf(wsd, "chunk_off", B + 1, torch.int64, dev)
        cws = _ws(B, dev, wsd)
        check(_lib.lib().ocn_chunk_offsets(ptr(rowptrA), ptr(nds), ptr(src), ptr(order), B, ptr(chunk_off), ptr(cws),
                                           stream_ptr()), "ocn_chunk_offsets")
        if nds is not None:
            rev_off = buf(wsd, "rev_off", B + 1, torch.int64, dev)
            check(_lib.lib().ocn_walk_rev_offsets(ptr(rowptrA), ptr(nds), ptr(src), ptr(dst), ptr(order), B,
                                                  ptr(rev_off), ptr(cws), stream_ptr()), "ocn_walk_rev_offsets")
    _mark("cn_prep")
    if walk:
        check(_lib.lib().ocn_cn_walk_flags(ptr(rowptrA), ptr(colA), ptr(nds), ptr(src), ptr(dst), ptr(order), B,
                                           ptr(chunk_off), ptr(rev_off), ptr(off), int(max_deg_a), ptr(flags),
                                           ptr(wc), cap, ptr(hist), ptr(cnt1), ptr(cnt2), ptr(status),
                                           stream_ptr()), "ocn_cn_walk_flags")
    else:
        check(_lib.lib().ocn_cn_flags_cover(
            *_cn_operands(rowptrA, colA, csr1, csr2, t1_bitmap, t2_bitmap, src, dst, order, B, n_cols), ptr(off), ptr(flags), cap,
            ptr(hist), ptr(cnt1), ptr(cnt2), ptr(status), ptr(rec), ptr(sched), int(rec_in),
            int(bool(t2_certified) and has_t2 and t2_cover), stream_ptr()), "ocn_cn_flags")
    _mark("cn_flags")
    return order, off, flags, wc, hist, cnt1, cnt2, status, scal


def _cn_flags_walk_small(rowptrA, colA, src, dst, n_cols, max_deg_a, wsd, nds):
    """Walk route, small batch (the drivers' 2048): one prep launch (ocn_walk_prep), the per-candidate sweeps for
    candidates with a source of their own, the shared sweep for candidates that share one (ocn_cn_walk_group)."""
    dev, B = src.device, src.numel()
    l = _lib.lib()
    nds = _nds_arg(nds if walk_two_sided else None, rowptrA.numel() - 1)
    order = buf(wsd, "order", B, torch.int64, dev)
    off = buf(wsd, "off", B + 1, torch.int64, dev)
    chunk_off = buf(wsd, "chunk_off", B + 1, torch.int64, dev)
    rev_off = buf(wsd, "rev_off", B + 1, torch.int64, dev) if nds is not None else None
    g_head = buf(wsd, "g_head", B + 1, torch.int32, dev)
    g_item_off = buf(wsd, "g_item_off", B + 1, torch.int64, dev)
    g_active = buf(wsd, "g_active", B, torch.int32, dev)
    meta = buf(wsd, "walk_meta", 4, torch.int32, dev)
    hist = buf(wsd, "hist", (n_cols, 2), torch.int64, dev)
    cnt1 = buf(wsd, "cnt1", B, torch.int32, dev)
    cnt2 = buf(wsd, "cnt2", B, torch.int32, dev)
    status = buf(wsd, "status", 4, torch.int32, dev, zero_init=True)     # ([3]: the sticky error word, never cleared by the library)
    scal = buf(wsd, "scal", 4, torch.int32, dev)
    check(l.ocn_walk_prep(ptr(rowptrA), ptr(nds), ptr(src), ptr(dst), B, int(walk_share_min), ptr(order), ptr(off),
                          ptr(chunk_off), ptr(rev_off), ptr(g_head), ptr(g_item_off), ptr(g_active), ptr(meta), ptr(cnt1),
                          ptr(cnt2), ptr(status), ptr(scal), stream_ptr()), "ocn_walk_prep")
    zero_regions([hist])
    cap = _flag_capacity(B, max_deg_a, off)
    flags = buf(wsd, "flags", max(cap, 1), torch.uint8, dev)
    wc = buf(wsd, "wc", max(cap, 1), torch.int32, dev)
    _mark("cn_prep")
    check(l.ocn_cn_walk_flags(ptr(rowptrA), ptr(colA), ptr(nds), ptr(src), ptr(dst), ptr(order), B, ptr(chunk_off),
                              ptr(rev_off), ptr(off), int(max_deg_a), ptr(flags), ptr(wc), cap, ptr(hist), ptr(cnt1),
                              ptr(cnt2), ptr(status), stream_ptr()), "ocn_cn_walk_flags")
    check(l.ocn_cn_walk_group(ptr(rowptrA), ptr(colA), ptr(src), ptr(dst), ptr(order), B, ptr(g_head), ptr(g_item_off),
                              ptr(g_active), ptr(meta), ptr(off), ptr(flags), ptr(wc), cap, ptr(hist), ptr(cnt1), ptr(cnt2),
                              stream_ptr()), "ocn_cn_walk_group")
    _mark("cn_flags")
    return order, off, flags, wc, hist, cnt1, cnt2, status, scal


@_on_device
def cn3_flags(rowptrA: Tensor, colA: Tensor, rowptrT: Tensor, colT: Tensor, bits: Tensor, src: Tensor, dst: Tensor, n_cols: int,
              off: Tensor, order: Optional[Tensor], max_deg_a: int, wsd=None, nds: Optional[Tensor] = None,
              flags: Optional[Tensor] = None):
    """The (A, A³) pass of cn6 without a stored A³ (ocn_hip.h: ocn_cn3_flags): neighbour p of ``src[e]`` is a cn3 entry when
    its row of Aᵀ (``rowptrT`` / ``colT``; A's own arrays for a symmetric A) shares a column with bit row ``dst[e]`` of A²
    (``bits``, int32 [n, words]).  ``off`` / ``order``: the flag offsets and the processing order of the batch's (A, A, A²)
    pass (``cn_flags``), or ``edge_offsets`` / None.  ``nds`` (or None): Σ_{k∈N(i)} |Aᵀ row k| per source — the work items then
    sweep a bounded number of elements (``neighbor_degree_sum`` for a symmetric A).  ``flags`` (or None): a caller's uint8
    buffer, whose length is then the capacity; by default the capacity is the one ``cn_flags`` derives.
    Returns (flags, hist [n_cols, 2] int64 packed, cnt3 int32 [B], status int32 [4])."""
    dev = src.device
    _req(rowptrA, torch.int64, "rowptrA", 1); _req(colA, torch.int32, "colA", 1)
    _req(rowptrT, torch.int64, "rowptrT", 1); _req(colT, torch.int32, "colT", 1)
    B = _batch_ids(src, dst, hist=True)
    _req(bits, torch.int32, "bits", 2)
    n = rowptrA.numel() - 1
    if rowptrT.numel() != int(n_cols) + 1:
        raise ValueError("rowptrT: the transpose has one row per column of the adjacency")
    if bits.shape[0] != n or bits.shape[1] * 32 < n_cols:
        raise ValueError(f"bits ({tuple(bits.shape)}) does not match the adjacency: {n} bit rows of at least {n_cols} bits")
    if _req(off, torch.int64, "off", 1).numel() != B + 1:
        raise ValueError("off: int64 [B + 1]")
    _order_arg(order, B)
    _nds_arg(nds, n)
    _mark("begin")
    hist = buf(wsd, "hist3", (n_cols, 2), torch.int64, dev)
    cnt3 = buf(wsd, "cnt3", B, torch.int32, dev)
    status = buf(wsd, "status3", 4, torch.int32, dev, zero_init=True)      # ([3]: the sticky error word)
    zero_regions([hist, cnt3, status[:3]])
    chunk_off = buf(wsd, "chunk_off3", B + 1, torch.int64, dev)
    cws = _ws(B, dev, wsd)
    check(_lib.lib().ocn_chunk_offsets(ptr(rowptrA), ptr(nds), ptr(src), ptr(order), B, ptr(chunk_off), ptr(cws), stream_ptr()),
          "ocn_chunk_offsets")
    if flags is None:
        cap = _flag_capacity(B, max_deg_a, off)
        flags = buf(wsd, "flags3", max(cap, 1), torch.uint8, dev)
    else:
        cap = _req(flags, torch.uint8, "flags", 1).numel()
    _mark("cn3_prep")
    check(_lib.lib().ocn_cn3_flags(ptr(rowptrA), ptr(colA), ptr(rowptrT), ptr(colT), ptr(bits), bits.shape[1], ptr(src), ptr(dst),
                                   ptr(order), B, int(n_cols), ptr(off), ptr(flags), cap, ptr(hist), ptr(cnt3), ptr(status),
                                   ptr(nds), ptr(chunk_off), stream_ptr()), "ocn_cn3_flags")
    _mark("cn3_flags")
    return flags, hist, cnt3, status


@_on_device
def neighbor_degree_sum(rowptr: Tensor, col: Tensor) -> Tensor:
    """nds[v] = Σ_{u∈N(v)} deg(u) (int64): the elements a sweep of v's neighbour rows touches."""
    _req(rowptr, torch.int64, "rowptr", 1); _req(col, torch.int32, "col", 1)
    n = rowptr.numel() - 1
    out = torch.empty(n, dtype=torch.int64, device=rowptr.device)
    check(_lib.lib().ocn_neighbor_degree_sum(ptr(rowptr), ptr(col), n, ptr(out), stream_ptr()),
          "ocn_neighbor_degree_sum")
    return out


exact_colsum = True              # cn5 / cn6 with innerprod != 0: column sums in the reference's entry order (ocn_cn_colsum_exact)


def _ip_nonzero(innerprod: Tensor) -> bool:
    """Whether the ``innerprod`` buffer is non-zero, read back once per value: cached per live tensor object
    (weak reference) and version counter, so an eval loop pays one host sync in total, not one per batch — and a
    freed tensor's address being reused by another one cannot hit."""
    import weakref
    hit = _ip_cache.get("k")
    if hit is None or hit[0]() is not innerprod or hit[1] != innerprod.data_ptr() or hit[2] != innerprod._version:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("innerprod changed since the last eager call: run one eager batch before capturing")
        _ip_cache["k"] = (weakref.ref(innerprod), innerprod.data_ptr(), innerprod._version)
        _ip_cache["v"] = bool(innerprod.detach().reshape(-1)[0].item() != 0.0)
    return _ip_cache["v"]


_ip_cache: dict = {}


def colsum_wanted(innerprod: Tensor) -> bool:
    """cn5 / cn6: is the second column normalisation to be summed in the reference's entry order?  Only a
    non-zero ``innerprod`` makes the order matter (for 0 the closed form over the integer counts is exact)."""
    return exact_colsum and _ip_nonzero(innerprod)


@_on_device
def cn_colsum_exact(rowptrA, colA, src, off, flagsA, flagsB, wc, hist: Tensor, innerprod: Tensor, scal: Tensor, wsd=None,
                    s2_init: Optional[Tensor] = None):
    """Order-exact S2 (and S3 with ``flagsB``) of the batch; ocn_hip.h: ocn_cn_colsum_exact.  ``scal``: the
    batch's zeroed int32[4] statistics scratch (shared with the weights call).  Returns (s2, s3|None)."""
    _req(hist, torch.int64, "hist", 2)
    N, dev = hist.shape[0], hist.device
    cap = flagsA.numel()
    if cap >= (1 << 32) - 1:
        raise NotImplementedError("order-exact column sums address flag positions with 32 bits")
    ip = _req(innerprod.detach().reshape(1).to(torch.float32), torch.float32, "innerprod", 1)
    if s2_init is not None and _req(s2_init, torch.float32, "s2_init", 1).numel() != N:
        raise ValueError("s2_init must have one entry per column")
    s2 = buf(wsd, "s2_exact", N, torch.float32, dev)
    s3 = buf(wsd, "s3_exact", N, torch.float32, dev) if flagsB is not None else None
    ws = buf(wsd, "colsum_ws", int(_lib.lib().ocn_cn_colsum_workspace_bytes(N, cap)) // 8 + 1, torch.int64, dev)
    check(_lib.lib().ocn_cn_colsum_exact(ptr(rowptrA), ptr(colA), ptr(src), src.numel(), ptr(off), ptr(flagsA), ptr(flagsB),
                                         ptr(wc), cap, ptr(hist), N, ptr(ip), ptr(scal), ptr(s2_init), ptr(s2), ptr(s3),
                                         ptr(ws), stream_ptr()), "ocn_cn_colsum_exact")
    _mark("cn_colsum")
    return s2, s3


@_on_device
def cn_weights_cn5(hist: Tensor, innerprod: Tensor, valued: bool = False, wsd=None, s2_exact: Optional[Tensor] = None,
                   scal: Optional[Tensor] = None) -> Tensor:
    """In place: packed int64 [N,2] histogram -> float32 [N,4] weights {w1, t, inv2, 0} (same storage).
    ``s2_exact``: the column sums of ``cn_colsum_exact`` (then ``scal`` is the statistics scratch that call
    used); None: the closed form over the integer counts (exact for innerprod == 0)."""
    _req(hist, torch.int64, "hist", 2)
    ip = _req(innerprod.detach().reshape(1).to(torch.float32), torch.float32, "innerprod", 1)
    if scal is None:
        scal = buf(wsd, "scal", 4, torch.int32, hist.device, zero=True)
    if _ip_nonzero(innerprod) and s2_exact is None:     # the batch's scale statistic: only a non-zero innerprod reads it
        check(_lib.lib().ocn_cn5_column_stats(ptr(hist), hist.shape[0], ptr(scal), stream_ptr()), "ocn_cn5_column_stats")
    check(_lib.lib().ocn_cn_weights_cn5(ptr(hist), hist.shape[0], ptr(ip), ptr(scal), int(valued), ptr(s2_exact),
                                        stream_ptr()), "ocn_cn_weights_cn5")
    _mark("cn_weights")
    return hist.view(torch.float32)


@_on_device
def cn_weights_cn7(hist: Tensor, sum_fill: float, diag1: Optional[Tensor] = None, diag2: Optional[Tensor] = None) -> Tensor:
    """``diag1`` / ``diag2``: the Chebyshev diagonals of the cn1 / cn2 branch (float32 [N]; None = T0 = ones)."""
    _req(hist, torch.int64, "hist", 2)
    for d, nm in ((diag1, "diag1"), (diag2, "diag2")):
        if d is not None and _req(d, torch.float32, nm, 1).numel() != hist.shape[0]:
            raise ValueError(f"{nm}: one entry per column")
    check(_lib.lib().ocn_cn_weights_cn7(ptr(hist), hist.shape[0], float(sum_fill), ptr(diag1), ptr(diag2), stream_ptr()),
          "ocn_cn_weights_cn7")
    _mark("cn_weights")
    return hist.view(torch.float32)


@_on_device
def cn_gather(rowptrA, colA, src, dst, off, flags, wc: Optional[Tensor], weights: Tensor, h: Tensor,
              order: Optional[Tensor] = None, max_row_len: int = 0, wsd=None, out_row: Optional[Tensor] = None,
              cnt1: Optional[Tensor] = None, cnt2: Optional[Tensor] = None, rec: Optional[Tensor] = None,
              sched: Optional[Tensor] = None, rowsum: Optional[Tensor] = None, sched_ready: bool = False):
    """The pooling (ocn_hip.h: ocn_cn_gather).  ``h``: the fp32 embedding table — or a bf16 / f16 one (``pipeline.embedding_table``),
    which goes to ocn_cn_gather_h16: the same fp32 output buffer, the same schedule and slot records, no ``rowsum`` (it is
    dropped: the shortcut adds the same numbers in the same order), widths ``LN_WIDTHS`` only.  The three outputs are bit for
    bit those of the fp32 entry on ``h.float()``.  An ``Int8Table`` goes to ocn_cn_gather_q8 on the same terms."""
    if isinstance(h, Int8Table):
        return _cn_gather_q8(rowptrA, colA, src, dst, off, flags, wc, weights, h, 0, 0, order, max_row_len, wsd, out_row, cnt1,
                             cnt2, rec, sched, sched_ready, None)
    _req(weights, torch.float32, "weights", 2)
    half = is_half_table(h)
    _req(h, h.dtype if half else torch.float32, "h", 2)
    if weights.shape[0] != h.shape[0] or weights.shape[1] != 4:
        raise ValueError("weights must be [N,4] with N = h.shape[0]")
    B, H = src.numel(), h.shape[1]
    if half:
        if H not in LN_WIDTHS:
            raise NotImplementedError(f"the pooling of a {h.dtype} table supports hidden widths {LN_WIDTHS}, got {H}")
        if h.data_ptr() % 16:
            raise ValueError("h must be 16-byte aligned")
        rowsum = None
    out = buf(wsd, "pooled", (3, B, H), torch.float32, h.device)
    if rowsum is not None and (wc is not None or cnt2 is None or _req(rowsum, torch.float32, "rowsum", 2).shape != h.shape):
        raise ValueError("rowsum: [N, H] row sums of h, pattern route with per-row counts only")
    perm = None
    n_groups = sched_groups(B, H) if (sched is not None and rec is not None) else 0
    if n_groups:
        perm = sched[n_groups:]       # the intersection pass left the groups' costs in sched[:n_groups]; their visiting order follows
        if not sched_ready:           # (a scoring loop's phase A has run gather_schedule already)
            check(_lib.lib().ocn_gather_schedule(ptr(sched), n_groups, int(sched_segment), ptr(perm), stream_ptr()), "ocn_gather_schedule")
    _mark("cn_pre")                   # (stage timers: what sits between the intersection pass and the pooling on this stream)
    if half:
        check(_lib.lib().ocn_cn_gather_h16(ptr(rowptrA), ptr(colA), ptr(src), ptr(dst), ptr(order), B, ptr(off), ptr(flags),
                                           ptr(wc), ptr(weights), ptr(h), HALF_TABLE_FMT[h.dtype], H, int(max_row_len), ptr(out[0]),
                                           ptr(out[1]), ptr(out[2]), ptr(out_row), ptr(cnt1), ptr(cnt2), ptr(rec), ptr(perm),
                                           stream_ptr()), "ocn_cn_gather_h16")
        _mark("cn_gather")
        return out[0], out[1], out[2]
    check(_lib.lib().ocn_cn_gather(ptr(rowptrA), ptr(colA), ptr(src), ptr(dst), ptr(order), B, ptr(off), ptr(flags),
                                   ptr(wc), ptr(weights), ptr(h), H, int(max_row_len), ptr(out[0]), ptr(out[1]),
                                   ptr(out[2]), ptr(out_row), ptr(cnt1), ptr(cnt2), ptr(rec), ptr(perm), ptr(rowsum),
                                   stream_ptr()), "ocn_cn_gather")
    _mark("cn_gather")
    return out[0], out[1], out[2]


@_on_device
def cn_gather_cap(rowptrA, colA, src, dst, off, flags, wc: Optional[Tensor], weights: Tensor, h: Tensor, cap: int, seed: int = 0,
                  order: Optional[Tensor] = None, max_row_len: int = 0, wsd=None, out_row: Optional[Tensor] = None,
                  cnt1: Optional[Tensor] = None, cnt2: Optional[Tensor] = None, rec: Optional[Tensor] = None,
                  sched: Optional[Tensor] = None, sched_ready: bool = False, mult: Optional[Tensor] = None):
    """The capped pooling (ocn_hip.h: ocn_cn_gather_cap): ``cn_gather`` with at most ``cap`` embedding rows per candidate — a
    stratified sample of its common-neighbour entries, fixed by (``seed``, src, dst, the candidate's flags) and reweighted so
    that the pooled vectors are unbiased estimates of the exact ones.  A candidate with at most ``cap`` entries gets the bits
    of ``cn_gather``.  The same output buffer, schedule and slot records as ``cn_gather``; no ``rowsum``; fp32 tables of the
    widths ``LN_WIDTHS`` only.  ``mult`` (optional, int32, one word per flag position): receives every position's multiplier
    — the stratum size of a selected entry, 1 where the candidate is within the cap, 0 for every other position.  An
    ``Int8Table`` in place of ``h`` goes to ocn_cn_gather_q8: the same sample, bit for bit this call on ``h.float()``."""
    refuse_half_table(h, "the capped pooling (cn_gather_cap)")
    if isinstance(h, Int8Table):
        cap = int(cap)
        if not 1 <= cap < (1 << 31):
            raise ValueError("cap: at least one row per candidate (an int32)")
        return _cn_gather_q8(rowptrA, colA, src, dst, off, flags, wc, weights, h, cap, _seed(seed), order, max_row_len, wsd,
                             out_row, cnt1, cnt2, rec, sched, sched_ready, mult)
    _req(weights, torch.float32, "weights", 2)
    _req(h, torch.float32, "h", 2)
    if weights.shape[0] != h.shape[0] or weights.shape[1] != 4:
        raise ValueError("weights must be [N,4] with N = h.shape[0]")
    cap = int(cap)
    if not 1 <= cap < (1 << 31):
        raise ValueError("cap: at least one row per candidate (an int32)")
    seed = _seed(seed)
    B, H = src.numel(), h.shape[1]
    if H not in LN_WIDTHS:
        raise NotImplementedError(f"the capped pooling supports hidden widths {LN_WIDTHS}, got {H}")
    if mult is not None and (_req(mult, torch.int32, "mult", 1).numel() < flags.numel()):
        raise ValueError("mult: one int32 word per flag position")
    out = buf(wsd, "pooled", (3, B, H), torch.float32, h.device)
    perm = None
    n_groups = sched_groups(B, H) if (sched is not None and rec is not None) else 0
    if n_groups:
        perm = sched[n_groups:]       # (the groups' costs are those of the full sets: upper bounds here, which is fine for an order)
        if not sched_ready:
            check(_lib.lib().ocn_gather_schedule(ptr(sched), n_groups, int(sched_segment), ptr(perm), stream_ptr()), "ocn_gather_schedule")
    _mark("cn_pre")
    check(_lib.lib().ocn_cn_gather_cap(ptr(rowptrA), ptr(colA), ptr(src), ptr(dst), ptr(order), B, ptr(off), ptr(flags),
                                       ptr(wc), ptr(weights), ptr(h), H, int(max_row_len), ptr(out[0]), ptr(out[1]),
                                       ptr(out[2]), ptr(out_row), ptr(cnt1), ptr(cnt2), ptr(rec), ptr(perm), cap, seed, ptr(mult),
                                       stream_ptr()), "ocn_cn_gather_cap")
    _mark("cn_gather")
    return out[0], out[1], out[2]


def _cn_gather_q8(rowptrA, colA, src, dst, off, flags, wc, weights, table: Int8Table, cap: int, seed: int, order, max_row_len, wsd,
                  out_row, cnt1, cnt2, rec, sched, sched_ready, mult):
    """``cn_gather`` (``cap`` = 0) and ``cn_gather_cap`` (``cap`` >= 1) of an ``Int8Table``: ocn_cn_gather_q8."""
    _req(weights, torch.float32, "weights", 2)
    q, scale = _req(table.rows, torch.int8, "table.rows", 2), _req(table.scale, torch.float32, "table.scale", 1)
    N, H = table.shape
    if weights.shape[0] != N or weights.shape[1] != 4:
        raise ValueError("weights must be [N,4] with N = h.shape[0]")
    if H not in LN_WIDTHS:
        raise NotImplementedError(f"the pooling of an int8 table supports hidden widths {LN_WIDTHS}, got {H}")
    stride = q.shape[1]
    if stride % 16 or q.data_ptr() % 16:
        raise ValueError("an int8 table's rows must be 16-byte aligned and a multiple of 16 bytes long (quantize_rows_i8 pads)")
    B = src.numel()
    if mult is not None and (_req(mult, torch.int32, "mult", 1).numel() < flags.numel()):
        raise ValueError("mult: one int32 word per flag position")
    out = buf(wsd, "pooled", (3, B, H), torch.float32, q.device)
    perm = None
    n_groups = sched_groups(B, H) if (sched is not None and rec is not None) else 0
    if n_groups:
        perm = sched[n_groups:]
        if not sched_ready:
            check(_lib.lib().ocn_gather_schedule(ptr(sched), n_groups, int(sched_segment), ptr(perm), stream_ptr()), "ocn_gather_schedule")
    _mark("cn_pre")
    check(_lib.lib().ocn_cn_gather_q8(ptr(rowptrA), ptr(colA), ptr(src), ptr(dst), ptr(order), B, ptr(off), ptr(flags), ptr(wc),
                                      ptr(weights), ptr(q), stride, ptr(scale), H, int(max_row_len), ptr(out[0]), ptr(out[1]),
                                      ptr(out[2]), ptr(out_row), ptr(cnt1), ptr(cnt2), ptr(rec), ptr(perm), cap, seed, ptr(mult),
                                      stream_ptr()), "ocn_cn_gather_q8")
    _mark("cn_gather")
    return out[0], out[1], out[2]


_unit_w: dict = {}


def unit_weights(n: int, device) -> Tensor:
    """Column weights {1, 0, 1, 0} for every column (float32 [n, 4], cached per size and device): with them the pooling
    forms w1 = [cn1] and w2 = [cn2] * v — cn8's unnormalised pools — and its transpose the matching gradient."""
    key = (int(n), str(device))
    w = _unit_w.get(key)
    if w is None:
        if len(_unit_w) > 8:
            _unit_w.clear()
        w = _unit_w[key] = torch.tensor([1.0, 0.0, 1.0, 0.0], device=device).repeat(int(n), 1).contiguous()
    return w


@_on_device
def order_by_node(node: Tensor, n_nodes: int, wsd=None) -> Tensor:
    """A stable processing order of the batch rows by node id (ocn_hip.h: ocn_order_by_node) — the order ``cn_flags`` forms for
    itself through ocn_batch_prep / ocn_order_by_node_finish, for a pass that has no offsets to scan.  It uses the scratch names
    ``order`` / ``order_ws`` of ``cn_flags`` on purpose: a scratch set serves one batch state at a time (a predictor's slot runs
    either the flag pass or the one-pass cn8 pooling for a batch, never both), the shapes agree and the workspace is left zero."""
    _req(node, torch.int64, "node", 1)
    B = node.numel()
    order = buf(wsd, "order", B, torch.int64, node.device)
    ows = buf(wsd, "order_ws", int(_lib.lib().ocn_order_workspace_bytes(n_nodes)) // 8 + 1, torch.int64, node.device, zero_init=True)
    check(_lib.lib().ocn_order_by_node(ptr(node), B, int(n_nodes), ptr(order), ptr(ows), stream_ptr()), "ocn_order_by_node")
    return order


def batch_order(src: Tensor, n_nodes: int, wsd=None) -> Optional[Tensor]:
    """Outside ``cn_flags`` (which forms its own by this rule): by source from ``sort_edges_min_batch`` candidates on, else None."""
    return order_by_node(src, n_nodes, wsd) if src.numel() >= sort_edges_min_batch else None


# cn8 in eval on adjoverlap handles: ocn_cn8_pool when on, else flags -> unit weights -> the pooling of cn5 / cn7.  OFF by default:
# the one pass is built and tested bit-equal, but it gives up the chain's longest-first schedule and class-major head rows, and the
# default goes to it only on a measurement that shows its range below the chain's (tools/cn8bench.py).
cn8_fused_eval = os.environ.get("OCN_CN8_FUSED", "0") == "1"


@_on_device
def cn8_pool(rowptrA: Tensor, colA: Tensor, t1: Optional[Tuple[Optional[Tensor], Optional[Tensor]]],
             t2: Optional[Tuple[Optional[Tensor], Optional[Tensor]]], src: Tensor, dst: Tensor, h: Tensor,
             t1_bitmap: Optional[Tensor] = None, t2_bitmap: Optional[Tensor] = None, order: Optional[Tensor] = None, wsd=None,
             n_cols: Optional[int] = None):
    """cn8's intersection and pooling in one pass (ocn_hip.h: ocn_cn8_pool; pattern route).  ``t1`` / ``t2`` = (rowptr, col)
    of the matrices whose rows ``dst`` are intersected with N(src), and / or their dense bit rows; ``order``: an optional
    processing order (a permutation of the batch rows); ``n_cols``: the column count of A, T1 and T2 (default: the rows of
    ``h``, which it must equal — every column id indexes a row of h).  T1 and T2 must have the same number of rows, whichever
    form they come in: ``dst`` is bounds-checked against it.  Returns (xcn1, xcn2, xij [B, H], cnt1, cnt2 int32 [B])."""
    _req(rowptrA, torch.int64, "rowptrA", 1); _req(colA, torch.int32, "colA", 1)
    B = _batch_ids(src, dst)
    N, H = _req(h, torch.float32, "h", 2).shape
    if H not in LN_WIDTHS:
        raise NotImplementedError(f"cn8 pooling supports hidden widths {LN_WIDTHS}, got {H}")
    if n_cols is not None and int(n_cols) != N:
        raise ValueError(f"h has {N} rows, the adjacency {int(n_cols)} columns")
    *csr1, rows = _t_pair_or_bits(t1, t1_bitmap, "T1", N)
    *csr2, _ = _t_pair_or_bits(t2, t2_bitmap, "T2", N, like=rows)
    _order_arg(order, B)
    check_edges(src, dst, rowptrA.numel() - 1, rows)
    out = buf(wsd, "pooled", (3, B, H), torch.float32, h.device)
    cnt = buf(wsd, "cn8_cnt", (2, B), torch.int32, h.device)
    if B == 0:
        return out[0], out[1], out[2], cnt[0], cnt[1]
    _mark("cn_prep")
    check(_lib.lib().ocn_cn8_pool(*_cn_operands(rowptrA, colA, csr1, csr2, t1_bitmap, t2_bitmap, src, dst, order, B, N),
                                  ptr(h), H, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(cnt[0]), ptr(cnt[1]), stream_ptr()),
          "ocn_cn8_pool")
    _mark("cn8_pool")
    return out[0], out[1], out[2], cnt[0], cnt[1]


# A cn5 / cn7 predictor with frozen column weights (ocn_amd/frozen.py) in eval on adjoverlap handles: ocn_cn_pool_frozen when on,
# else the chain (flags -> the frozen table in place of the batch's weights -> the pooling).  OFF by default, by the rule of
# ``cn8_fused_eval``: the default goes to the one pass only on a measurement that shows its range below the chain's at the
# throughput shape (frozen column weights; tools/frozenbench.py).
frozen_fused_eval = os.environ.get("OCN_FROZEN_FUSED", "0") == "1"


@_on_device
def cn_pool_frozen(rowptrA: Tensor, colA: Tensor, t1: Optional[Tuple[Optional[Tensor], Optional[Tensor]]],
                   t2: Optional[Tuple[Optional[Tensor], Optional[Tensor]]], src: Tensor, dst: Tensor, h: Tensor, weights: Tensor,
                   t1_bitmap: Optional[Tensor] = None, t2_bitmap: Optional[Tensor] = None, order: Optional[Tensor] = None, wsd=None,
                   n_cols: Optional[int] = None):
    """Intersection and pooling with a frozen column-weight table in one pass (ocn_hip.h: ocn_cn_pool_frozen; pattern route).
    ``weights``: float32 [N, 4] = {w1, t, inv2, 0} per column, N = the rows of ``h``; everything else as for ``cn8_pool``.
    Bit for bit what ``cn_flags`` -> ``cn_gather(weights=weights)`` leave for every candidate, whatever else is in the batch.
    Returns (xcn1, xcn2, xij [B, H], cnt1, cnt2 int32 [B] — the member counts, whatever their weights)."""
    _req(rowptrA, torch.int64, "rowptrA", 1); _req(colA, torch.int32, "colA", 1)
    B = _batch_ids(src, dst)
    N, H = _req(h, torch.float32, "h", 2).shape
    if H not in LN_WIDTHS:
        raise NotImplementedError(f"frozen pooling supports hidden widths {LN_WIDTHS}, got {H}")
    if n_cols is not None and int(n_cols) != N:
        raise ValueError(f"h has {N} rows, the adjacency {int(n_cols)} columns")
    if tuple(_req(weights, torch.float32, "weights", 2).shape) != (N, 4):
        raise ValueError(f"weights must be [N, 4] with N = h.shape[0] = {N}, got {tuple(weights.shape)}")
    if weights.data_ptr() % 16:
        raise ValueError("weights must be 16-byte aligned")
    *csr1, rows = _t_pair_or_bits(t1, t1_bitmap, "T1", N)
    *csr2, _ = _t_pair_or_bits(t2, t2_bitmap, "T2", N, like=rows)
    _order_arg(order, B)
    check_edges(src, dst, rowptrA.numel() - 1, rows)
    out = buf(wsd, "pooled", (3, B, H), torch.float32, h.device)
    cnt = buf(wsd, "cn8_cnt", (2, B), torch.int32, h.device)
    if B == 0:
        return out[0], out[1], out[2], cnt[0], cnt[1]
    _mark("cn_prep")
    check(_lib.lib().ocn_cn_pool_frozen(*_cn_operands(rowptrA, colA, csr1, csr2, t1_bitmap, t2_bitmap, src, dst, order, B, N),
                                        ptr(weights), ptr(h), H, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(cnt[0]), ptr(cnt[1]),
                                        stream_ptr()), "ocn_cn_pool_frozen")
    _mark("cn_pool_frozen")
    return out[0], out[1], out[2], cnt[0], cnt[1]


@_on_device
def cn_attribution(rowptrA: Tensor, colA: Tensor, src: Tensor, off: Tensor, flags: Tensor, wc: Optional[Tensor], weights: Tensor,
                   h: Tensor, g1: Tensor, g2: Tensor, order: Optional[Tensor] = None, wsd=None) -> Tuple[Tensor, Tensor]:
    """The share of every common neighbour in <g1[e], xcn1[e]> and <g2[e], xcn2[e]> (ocn_hip.h: ocn_cn_attribution).  ``off``,
    ``flags``, ``wc`` (None on the pattern route) and ``order`` are a batch state's (``CNState``), ``weights`` the [N, 4] table
    that state is pooled with, ``g1`` / ``g2`` float32 [B, H] the gradients with respect to its pooled rows.  Returns
    (attr float32 [flags.numel(), 2], rank float32 [flags.numel()]): per flag position {via xcn1, via xcn2} and their sum, -inf
    on positions that are no member.  Only the positions below ``off[-1]`` are written."""
    _req(rowptrA, torch.int64, "rowptrA", 1); _req(colA, torch.int32, "colA", 1)
    B = _req(src, torch.int64, "src", 1).numel()
    if _req(off, torch.int64, "off", 1).numel() != B + 1:
        raise ValueError("off: [B + 1] offsets, one per candidate and the total")
    cap = _req(flags, torch.uint8, "flags", 1).numel()
    if wc is not None and _req(wc, torch.int32, "wc", 1).numel() < cap:
        raise ValueError("wc: one walk count per flag byte")
    N, H = _req(h, torch.float32, "h", 2).shape
    if H not in LN_WIDTHS:
        raise NotImplementedError(f"the attribution supports hidden widths {LN_WIDTHS}, got {H}")
    if tuple(_req(weights, torch.float32, "weights", 2).shape) != (N, 4):
        raise ValueError(f"weights must be [N, 4] with N = h.shape[0] = {N}, got {tuple(weights.shape)}")
    for name, g in (("g1", g1), ("g2", g2)):
        if tuple(_req(g, torch.float32, name, 2).shape) != (B, H):
            raise ValueError(f"{name} must be [B, H] = [{B}, {H}], got {tuple(g.shape)}")
    for name, t in (("weights", weights), ("h", h), ("g1", g1), ("g2", g2)):
        if t.data_ptr() % 16:
            raise ValueError(f"{name} must be 16-byte aligned")
    _order_arg(order, B)
    attr = buf(wsd, "attr", (cap, 2), torch.float32, h.device)
    rank = buf(wsd, "attr_rank", cap, torch.float32, h.device)
    check(_lib.lib().ocn_cn_attribution(ptr(rowptrA), ptr(colA), ptr(src), ptr(order), B, ptr(off), ptr(flags), ptr(wc), cap,
                                        ptr(weights), ptr(h), H, ptr(g1), ptr(g2), ptr(attr), ptr(rank), stream_ptr()),
          "ocn_cn_attribution")
    _mark("cn_attribution")
    return attr, rank


@_on_device
def cn_node_sums(rowptrA: Tensor, colA: Tensor, t1: Optional[Tuple[Optional[Tensor], Optional[Tensor]]],
                 t2: Optional[Tuple[Optional[Tensor], Optional[Tensor]]], src: Tensor, dst: Tensor, w: Tensor,
                 t1_bitmap: Optional[Tensor] = None, t2_bitmap: Optional[Tensor] = None, order: Optional[Tensor] = None, wsd=None,
                 n_cols: Optional[int] = None):
    """Sums of a node table over the common neighbours of a candidate batch, in one pass (ocn_hip.h: ocn_cn_node_sums) — what
    the link heuristics are made of (ocn_amd/heuristics.py).  ``t1`` / ``t2``, the bit rows, ``order`` and ``n_cols``: as for
    ``cn8_pool``, except that T2 may be left out altogether (``t2`` and ``t2_bitmap`` None: zero 2-hop outputs).  ``w``:
    float32 [N, 4], N = the column count of A, T1 and T2.  Returns (sum1, sum2 float32 [B, 4], cnt1, cnt2 int32 [B],
    deg float32 [B, 2] = {row length of src in A, of dst in T1}, or None where T1 has no CSR form)."""
    _req(rowptrA, torch.int64, "rowptrA", 1); _req(colA, torch.int32, "colA", 1)
    B = _batch_ids(src, dst)
    N = _req(w, torch.float32, "w", 2).shape[0]
    if w.shape[1] != 4:
        raise ValueError(f"w must be [N, 4], got {tuple(w.shape)}")
    if n_cols is not None and int(n_cols) != N:
        raise ValueError(f"w has {N} rows, the adjacency {int(n_cols)} columns")
    *csr1, rows = _t_pair_or_bits(t1, t1_bitmap, "T1", N)
    *csr2, _ = _t_pair_or_bits(t2, t2_bitmap, "T2", N, like=rows, optional=True)
    _order_arg(order, B)
    check_edges(src, dst, rowptrA.numel() - 1, rows)
    sums = buf(wsd, "heur_sums", (2, B, 4), torch.float32, w.device)
    cnt = buf(wsd, "heur_cnt", (2, B), torch.int32, w.device)
    deg = buf(wsd, "heur_deg", (B, 2), torch.float32, w.device) if csr1[0] is not None else None
    if B == 0:
        return sums[0], sums[1], cnt[0], cnt[1], deg
    check(_lib.lib().ocn_cn_node_sums(*_cn_operands(rowptrA, colA, csr1, csr2, t1_bitmap, t2_bitmap, src, dst, order, B, N),
                                      ptr(w), ptr(sums[0]), ptr(sums[1]), ptr(cnt[0]), ptr(cnt[1]), ptr(deg), stream_ptr()),
          "ocn_cn_node_sums")
    _mark("cn_node_sums")
    return sums[0], sums[1], cnt[0], cnt[1], deg


def row_diff_stage_cols() -> int:
    """Columns of an M row ``ocn_row_diff_*`` stages in LDS; longer rows are searched in memory."""
    return int(_lib.lib().ocn_row_diff_stage_cols())


def _row_diff_args(rowptrP: Tensor, colP: Tensor, rowptrM: Tensor, colM: Tensor, rows: Tensor) -> int:
    """The operand checks of both row-difference passes.  The columns of P and of M must be sorted and duplicate-free in every
    row, as every ``SparseTensor`` of the project stores them: the kernel does not sort again and this layer cannot see it."""
    _req(rowptrP, torch.int64, "rowptrP", 1); _req(colP, torch.int32, "colP", 1)
    _req(rowptrM, torch.int64, "rowptrM", 1); _req(colM, torch.int32, "colM", 1)
    _req(rows, torch.int64, "rows", 1)
    if rowptrP.numel() < 1 or rowptrP.numel() != rowptrM.numel():
        raise ValueError(f"P has {rowptrP.numel() - 1} rows, M {rowptrM.numel() - 1}")
    n = rowptrP.numel() - 1
    check_edges(rows, rows, n, n)
    return rows.numel()


@_on_device
def row_diff_count(rowptrP: Tensor, colP: Tensor, rowptrM: Tensor, colM: Tensor, rows: Tensor, drop_self: bool = True) -> Tensor:
    """count[q] = |P[s,:] \\ M[s,:]| for s = rows[q], without column s too under ``drop_self`` (ocn_hip.h: ocn_row_diff_count):
    int32 [Q].  ``scan_i32`` of it gives the offsets ``row_diff_fill`` writes at."""
    Q = _row_diff_args(rowptrP, colP, rowptrM, colM, rows)
    count = torch.empty(Q, dtype=torch.int32, device=rows.device)
    if Q:
        check(_lib.lib().ocn_row_diff_count(ptr(rowptrP), ptr(colP), ptr(rowptrM), ptr(colM), ptr(rows), Q, int(bool(drop_self)),
                                            ptr(count), stream_ptr()), "ocn_row_diff_count")
        _mark("row_diff_count")
    return count


@_on_device
def row_diff_fill(rowptrP: Tensor, colP: Tensor, rowptrM: Tensor, colM: Tensor, rows: Tensor, off: Tensor,
                  drop_self: bool = True, total: Optional[int] = None) -> Tensor:
    """The pairs (s, c) of every query's set, ascending in c, row-major in int64 [T, 2] from ``off[q]`` on (ocn_hip.h:
    ocn_row_diff_fill).  ``off``: ``scan_i32(row_diff_count(...))`` of the same operands; ``total`` = ``off[-1]`` where the
    caller has read it already (else it is read here: one host sync for the output size)."""
    Q = _row_diff_args(rowptrP, colP, rowptrM, colM, rows)
    T, edges = _fill_pairs(off, Q, total, rows.device)
    if Q and T:
        check(_lib.lib().ocn_row_diff_fill(ptr(rowptrP), ptr(colP), ptr(rowptrM), ptr(colM), ptr(rows), Q, int(bool(drop_self)),
                                           ptr(off), ptr(edges), stream_ptr()), "ocn_row_diff_fill")
        _mark("row_diff_fill")
    return edges


def two_hop_window_cols() -> int:
    """Columns of one LDS window of ``ocn_two_hop_diff_*``; a graph with more columns is swept in several."""
    return int(_lib.lib().ocn_two_hop_window_cols())


def _two_hop_args(rowptrA: Tensor, colA: Tensor, rowptrM: Tensor, colM: Tensor, rows: Tensor, window_cols: int,
                  window_limit=two_hop_window_cols) -> Tuple[int, int]:
    """The operand checks of the 2-hop passes: those of the row difference (A and M square and of one size, sorted
    duplicate-free columns, which this layer cannot see) and the window (``window_limit``: the entry's own).  Returns (Q, n)."""
    Q = _row_diff_args(rowptrA, colA, rowptrM, colM, rows)
    n = rowptrA.numel() - 1
    if not 0 < n < (1 << 31):
        raise ValueError(f"A has {n} rows: int32 columns serve 1 .. 2^31 - 1")
    window_cols = int(window_cols)
    if window_cols < 0 or window_cols % 64 or window_cols > window_limit():
        raise ValueError(f"window_cols must be 0 or a multiple of 64 up to {window_limit()}, got {window_cols}")
    return Q, n


@_on_device
def two_hop_diff_count(rowptrA: Tensor, colA: Tensor, rowptrM: Tensor, colM: Tensor, rows: Tensor, drop_self: bool = True,
                       window_cols: int = 0) -> Tensor:
    """count[q] = |(U_{m in A[s,:]} A[m,:]) \\ M[s,:]| for s = rows[q], without column s too under ``drop_self`` (ocn_hip.h:
    ocn_two_hop_diff_count): int32 [Q] — ``row_diff_count`` of the pattern of A·A without that product.  ``window_cols``:
    0, the library's window, except in tests of the sweep."""
    Q, n = _two_hop_args(rowptrA, colA, rowptrM, colM, rows, window_cols)
    count = torch.empty(Q, dtype=torch.int32, device=rows.device)
    if Q:
        check(_lib.lib().ocn_two_hop_diff_count(ptr(rowptrA), ptr(colA), ptr(rowptrM), ptr(colM), n, ptr(rows), Q,
                                                int(bool(drop_self)), int(window_cols), ptr(count), stream_ptr()),
              "ocn_two_hop_diff_count")
        _mark("two_hop_diff_count")
    return count


@_on_device
def two_hop_diff_fill(rowptrA: Tensor, colA: Tensor, rowptrM: Tensor, colM: Tensor, rows: Tensor, off: Tensor,
                      drop_self: bool = True, total: Optional[int] = None, window_cols: int = 0) -> Tensor:
    """The pairs (s, c) of every query's set, ascending in c, row-major in int64 [T, 2] from ``off[q]`` on (ocn_hip.h:
    ocn_two_hop_diff_fill).  ``off``, ``total``: as for ``row_diff_fill``."""
    Q, n = _two_hop_args(rowptrA, colA, rowptrM, colM, rows, window_cols)
    T, edges = _fill_pairs(off, Q, total, rows.device)
    if Q and T:
        check(_lib.lib().ocn_two_hop_diff_fill(ptr(rowptrA), ptr(colA), ptr(rowptrM), ptr(colM), n, ptr(rows), Q,
                                               int(bool(drop_self)), int(window_cols), ptr(off), ptr(edges), stream_ptr()),
              "ocn_two_hop_diff_fill")
        _mark("two_hop_diff_fill")
    return edges


def two_hop_sums_window_cols() -> int:
    """Columns of one LDS window of ``ocn_two_hop_sums_fill`` (a presence bit and an fp32 accumulator per column)."""
    return int(_lib.lib().ocn_two_hop_sums_window_cols())


@_on_device
def two_hop_sums_fill(rowptrA: Tensor, colA: Tensor, rowptrM: Tensor, colM: Tensor, rows: Tensor, off: Tensor,
                      w: Optional[Tensor] = None, wcol: int = 0, drop_self: bool = True, total: Optional[int] = None,
                      window_cols: int = 0) -> Tuple[Tensor, Tensor]:
    """The pairs of ``two_hop_diff_fill`` for the same operands and, beside each pair (s, c), the sum of ``w[m, wcol]`` over the
    m in row s of A whose row holds c, added in ascending m from 0.0f (ocn_hip.h: ocn_two_hop_sums_fill): (edges int64 [T, 2],
    val float32 [T]).  ``w``: a float32 [n, 4] node table (``heuristics.node_table``), ``wcol`` its column; None: every weight
    is 1, the sum counts the common neighbours.  ``off``: ``scan_i32(two_hop_diff_count(...))``, the one counting pass of both
    fills; ``total`` as for ``row_diff_fill``.  ``window_cols``: 0, the library's window, except in tests of the sweep."""
    Q, n = _two_hop_args(rowptrA, colA, rowptrM, colM, rows, window_cols, two_hop_sums_window_cols)
    if w is not None:
        if _req(w, torch.float32, "w", 2).shape != (n, 4):
            raise ValueError(f"w: expected the [{n}, 4] node table of A, got {tuple(w.shape)}")
        if w.device != rows.device:
            raise RuntimeError(f"two_hop_sums_fill: operands on different devices ({rows.device}, {w.device})")
        wcol = int(wcol)
        if not 0 <= wcol <= 3:
            raise ValueError(f"wcol must be a column 0..3 of the node table, got {wcol}")
    T, edges = _fill_pairs(off, Q, total, rows.device)
    val = torch.empty(T, dtype=torch.float32, device=rows.device)
    if Q and T:
        check(_lib.lib().ocn_two_hop_sums_fill(ptr(rowptrA), ptr(colA), ptr(rowptrM), ptr(colM), n, ptr(rows), Q,
                                               int(bool(drop_self)), int(window_cols), ptr(w), int(wcol) if w is not None else 0,
                                               ptr(off), ptr(edges), ptr(val), stream_ptr()), "ocn_two_hop_sums_fill")
        _mark("two_hop_sums_fill")
    return edges, val


prefilter_budget = 1 << 26       # candidates of one chunk of a 3-hop short list (recommend.prefilter_candidates): 1.3 GB at 20 B each


def frontier_window_cols() -> int:
    """Columns of one LDS window of ``ocn_frontier_count`` / ``ocn_frontier_sums_fill``."""
    return int(_lib.lib().ocn_frontier_window_cols())


def _frontier_list(lptr: Tensor, pairs: Tensor, val: Optional[Tensor], Q: int, n: int, name: str, device) -> Tensor:
    """The checks of one per-query list (the frontier or the seeds): ``lptr`` int64 [Q + 1], ``pairs`` int64 [T, 2] (the node
    is the second of a pair: the layout the fills write), ``val`` float32 [T] or None.  Node ids are range-checked through
    ``check_edges`` (waived inside ``prevalidated``, like every id check), and with them ``lptr[-1] <= T``.  That a query's
    nodes ascend is trusted, as for CSR columns.  Returns the pair tensor the entry is handed (never an empty one: the entry
    refuses NULL)."""
    if _req(lptr, torch.int64, f"ptr{name}", 1).numel() != Q + 1:
        raise ValueError(f"ptr{name}: one entry per query and the total")
    if _req(pairs, torch.int64, f"node{name}", 2).shape[1] != 2:
        raise ValueError(f"node{name}: expected the [T, 2] pair layout, got {tuple(pairs.shape)}")
    T = pairs.shape[0]
    if val is not None and _req(val, torch.float32, f"val{name}", 1).numel() != T:
        raise ValueError(f"val{name}: expected one value per pair of node{name} ({T}), got {val.numel()}")
    for t in (lptr, pairs, val):
        if t is not None and t.device != device:
            raise RuntimeError(f"frontier: operands on different devices ({device}, {t.device})")
    if validate_indices and (n, n) not in getattr(_checked, "scopes", ()):
        if T:
            nodes = pairs[:, 1].contiguous()
            check_edges(nodes, nodes, n, n)
        if Q and not 0 <= int(lptr[-1].item()) <= T:
            raise IndexError(f"ptr{name}: the total exceeds the {T} pairs of node{name}")
    return pairs if T else pairs.new_zeros(1, 2)


def _frontier_args(rowptrA, colA, rowptrM, colM, rows, window_cols, ptrF, nodeF, valF, ptrS, nodeS, valS):
    Q, n = _two_hop_args(rowptrA, colA, rowptrM, colM, rows, window_cols, frontier_window_cols)
    if (ptrS is None) != (nodeS is None):
        raise ValueError("seeds: ptrS and nodeS are given together or not at all")
    nodeF = _frontier_list(ptrF, nodeF, valF, Q, n, "F", rows.device)
    if ptrS is not None:
        nodeS = _frontier_list(ptrS, nodeS, valS, Q, n, "S", rows.device)
    if colM.numel() == 0:
        colM = colM.new_zeros(1)                                           # (an empty M: no row reads it, the entry still wants a pointer)
    return Q, n, colM, nodeF, nodeS


@_on_device
def frontier_count(rowptrA: Tensor, colA: Tensor, rowptrM: Tensor, colM: Tensor, rows: Tensor, ptrF: Tensor, nodeF: Tensor,
                   ptrS: Optional[Tensor] = None, nodeS: Optional[Tensor] = None, drop_self: bool = True,
                   window_cols: int = 0) -> Tensor:
    """count[q] = |(U_{c in F_q} A[c,:] U nodes(S_q)) \\ M[s,:]| for s = rows[q], without column s too under ``drop_self``
    (ocn_hip.h: ocn_frontier_count): int32 [Q].  ``ptrF`` int64 [Q + 1] and ``nodeF`` int64 [T, 2] are a per-query frontier list
    in the layout the fills write (the node is the second of a pair), ascending and duplicate-free per query; ``ptrS`` /
    ``nodeS``: the optional seed list, the same layout.  ``window_cols``: 0, the library's window, except in tests of the sweep."""
    Q, n, colM, nodeF, nodeS = _frontier_args(rowptrA, colA, rowptrM, colM, rows, window_cols, ptrF, nodeF, None, ptrS, nodeS, None)
    count = torch.empty(Q, dtype=torch.int32, device=rows.device)
    if Q:
        check(_lib.lib().ocn_frontier_count(ptr(rowptrA), ptr(colA), ptr(rowptrM), ptr(colM), n, ptr(rows), Q,
                                            int(bool(drop_self)), int(window_cols), ptr(ptrF), ptr(nodeF), ptr(ptrS), ptr(nodeS),
                                            ptr(count), stream_ptr()), "ocn_frontier_count")
        _mark("frontier_count")
    return count


@_on_device
def frontier_sums_fill(rowptrA: Tensor, colA: Tensor, rowptrM: Tensor, colM: Tensor, rows: Tensor, ptrF: Tensor, nodeF: Tensor,
                       valF: Optional[Tensor], ptrS: Optional[Tensor], nodeS: Optional[Tensor], valS: Optional[Tensor],
                       off: Tensor, drop_self: bool = True, total: Optional[int] = None, window_cols: int = 0,
                       values: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """The pairs (s, t) of every query's set, ascending in t, from ``off[q]`` on and, beside each, its ordered path sum
    (ocn_hip.h: ocn_frontier_sums_fill): (edges int64 [T, 2], val float32 [T]).  val = the seed value of t (``valS``, 0.0f where t
    is no seed) plus ``valF`` of every frontier node whose row holds t, one fp32 add each in ascending node id.  ``valF`` None:
    every weight is 1.  ``values=False``: the pairs alone, (edges, None); ``valF`` and ``valS`` are then not read.  ``off``:
    ``scan_i32(frontier_count(...))`` of the same operands; ``total`` as for ``row_diff_fill``.  The output is itself a list in
    the layout ``ptrF`` / ``nodeF`` / ``valF`` take: expansions chain without a conversion."""
    Q, n, colM, nodeF, nodeS = _frontier_args(rowptrA, colA, rowptrM, colM, rows, window_cols, ptrF, nodeF,
                                              valF if values else None, ptrS, nodeS, valS if values else None)
    if values and ptrS is not None and valS is None:
        raise ValueError("valS: seeds need their values where val is written")
    T, edges = _fill_pairs(off, Q, total, rows.device)
    val = torch.empty(T, dtype=torch.float32, device=rows.device) if values else None
    if Q and T:
        check(_lib.lib().ocn_frontier_sums_fill(ptr(rowptrA), ptr(colA), ptr(rowptrM), ptr(colM), n, ptr(rows), Q,
                                                int(bool(drop_self)), int(window_cols), ptr(ptrF), ptr(nodeF),
                                                ptr(valF if values else None), ptr(ptrS), ptr(nodeS),
                                                ptr(valS if values and ptrS is not None else None), ptr(off), ptr(edges), ptr(val),
                                                stream_ptr()), "ocn_frontier_sums_fill")
        _mark("frontier_sums_fill")
    return edges, val


def segment_topk_max_k() -> int:
    return int(_lib.lib().ocn_segment_topk_max_k())


@_on_device
def segment_topk(scores: Tensor, seg_ptr: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    """The ``k`` best entries of every segment ``scores[seg_ptr[q] : seg_ptr[q + 1]]``, best first (ocn_hip.h: ocn_segment_topk):
    (values float32 [Q, k], positions int64 [Q, k] into the flat vector; -inf and -1 where a segment has fewer than k).
    Order: higher score first, equal scores by position, +0.0 == -0.0, NaN after every number.  ``seg_ptr`` is trusted to be
    ascending offsets into ``scores`` with ``seg_ptr[-1] <= scores.numel()`` (checking it would cost a host sync)."""
    k = int(k)
    if not 1 <= k <= segment_topk_max_k():
        raise ValueError(f"k must be in 1..{segment_topk_max_k()}, got {k}")
    _req(scores, torch.float32, "scores", 1); _req(seg_ptr, torch.int64, "ptr", 1)
    if seg_ptr.numel() < 1:
        raise ValueError("ptr: [Q + 1] offsets")
    if scores.numel() >= (1 << 32) - 1:
        raise ValueError("scores: segments of 2^32 - 1 entries or more are not supported")
    Q = seg_ptr.numel() - 1
    val = torch.empty(Q, k, dtype=torch.float32, device=scores.device)
    pos = torch.empty(Q, k, dtype=torch.int64, device=scores.device)
    if Q:
        src = scores if scores.numel() else scores.new_empty(1)          # (no score to read: every segment is empty, the entry still wants a pointer)
        check(_lib.lib().ocn_segment_topk(ptr(src), ptr(seg_ptr), Q, k, ptr(val), ptr(pos), stream_ptr()), "ocn_segment_topk")
        _mark("segment_topk")
    return val, pos


@_on_device
def segment_rank(scores: Tensor, seg_ptr: Tensor, edges: Tensor, tptr: Tensor, tnode: Tensor) -> Tuple[Tensor, Tensor]:
    """Where given nodes stand in the order of ``segment_topk`` (ocn_hip.h: ocn_segment_rank): (rank int64 [P], pos int64 [P]).
    Segment ``q`` is ``scores[seg_ptr[q] : seg_ptr[q + 1]]`` with the ids ``edges[seg_ptr[q] : seg_ptr[q + 1], 1]``, ascending
    (the [T, 2] layout of the candidate builders); ``tnode[tptr[q] : tptr[q + 1]]`` are the nodes to rank in it — any order,
    repeats allowed, possibly none.  ``rank`` = 1 + the number of entries of the segment that come before the node's in that
    order, ``pos`` = its position in the flat vector; 0 and -1 where the node is no id of the segment (any int64 value).
    ``seg_ptr`` and ``tptr`` are trusted to be ascending offsets with ``seg_ptr[-1] <= scores.numel()`` and ``tptr[-1] ==
    tnode.numel()``, and the ids to ascend (checking would cost a host sync)."""
    _req(scores, torch.float32, "scores", 1); _req(seg_ptr, torch.int64, "ptr", 1)
    _req(tptr, torch.int64, "tptr", 1); _req(tnode, torch.int64, "tnode", 1)
    if _req(edges, torch.int64, "edges", 2).shape[1] != 2:
        raise ValueError(f"edges: expected the [T, 2] pair layout, got {tuple(edges.shape)}")
    if seg_ptr.numel() < 1:
        raise ValueError("ptr: [Q + 1] offsets")
    if tptr.numel() != seg_ptr.numel():
        raise ValueError(f"tptr: one target list per segment and the total ({seg_ptr.numel()} offsets), got {tptr.numel()}")
    if edges.shape[0] != scores.numel():
        raise ValueError(f"edges: one pair per score ({scores.numel()}), got {edges.shape[0]}")
    if scores.numel() >= (1 << 32) - 1:
        raise ValueError("scores: segments of 2^32 - 1 entries or more are not supported")
    Q, P = seg_ptr.numel() - 1, tnode.numel()
    if not (Q and P):                                                    # (targets without a segment are not found either)
        return (torch.zeros(P, dtype=torch.int64, device=scores.device), torch.full((P,), -1, dtype=torch.int64, device=scores.device))
    rank = torch.empty(P, dtype=torch.int64, device=scores.device)
    pos = torch.empty(P, dtype=torch.int64, device=scores.device)
    src = scores if scores.numel() else scores.new_empty(1)              # (no score to read: every segment is empty, the entry still wants
    ids = edges if scores.numel() else edges.new_zeros(1, 2)             #  its pointers)
    check(_lib.lib().ocn_segment_rank(ptr(src), ptr(seg_ptr), ptr(ids), Q, ptr(tptr), ptr(tnode), P, ptr(rank), ptr(pos),
                                      stream_ptr()), "ocn_segment_rank")
    _mark("segment_rank")
    return rank, pos


SEGMENT_KEEP_MAX_M = (1 << 31) - 1


@_on_device
def segment_keep_best(scores: Tensor, seg_ptr: Tensor, m: int, return_cut: bool = False):
    """The ``m`` best entries of every segment in the order of ``segment_topk``, as a set (ocn_hip.h: ocn_segment_keep_best):
    (``ptr_m`` int64 [Q + 1], ``keep_pos`` int64 [ptr_m[-1]][, ``cut`` int64 [Q]]).  ``keep_pos[ptr_m[q] : ptr_m[q + 1]]`` are the
    positions in the flat vector of the ``min(len_q, m)`` entries of segment ``q`` that ``segment_topk`` would list first,
    ASCENDING — no ranked order, no [Q, m] rectangle, and no limit of ``segment_topk_max_k()``: ``1 <= m <= 2^31 - 1``.
    ``return_cut``: the key of the worst kept entry of every segment (the bits of the kernel's uint64 — high word the score's
    monotone image, low word ~(position in the segment) — in an int64 tensor), 0 for an empty segment.  ``seg_ptr`` is trusted
    as ``segment_topk`` trusts it.  One host sync: the size of the kept list."""
    if isinstance(m, bool) or not isinstance(m, int) or not 1 <= m <= SEGMENT_KEEP_MAX_M:
        raise ValueError(f"m must be an int in 1..{SEGMENT_KEEP_MAX_M}, got {m!r}")
    _req(scores, torch.float32, "scores", 1); _req(seg_ptr, torch.int64, "ptr", 1)
    if seg_ptr.numel() < 1:
        raise ValueError("ptr: [Q + 1] offsets")
    if scores.numel() >= (1 << 32) - 1:
        raise ValueError("scores: segments of 2^32 - 1 entries or more are not supported")
    Q = seg_ptr.numel() - 1
    ptr_m = torch.zeros_like(seg_ptr)
    torch.cumsum((seg_ptr[1:] - seg_ptr[:-1]).clamp(max=m), 0, out=ptr_m[1:])
    total = int(ptr_m[-1].item()) if Q else 0
    keep = torch.empty(total, dtype=torch.int64, device=scores.device)
    cut = torch.zeros(Q, dtype=torch.int64, device=scores.device) if return_cut else None
    if Q and total:                                                      # (nothing kept: every segment is empty, every cut 0)
        check(_lib.lib().ocn_segment_keep_best(ptr(scores), ptr(seg_ptr), Q, m, ptr(ptr_m), ptr(keep), ptr(cut), stream_ptr()),
              "ocn_segment_keep_best")
        _mark("segment_keep_best")
    return (ptr_m, keep, cut) if return_cut else (ptr_m, keep)


@_on_device
def philox4x32(ctr: Tensor, key0: int, key1: int) -> Tensor:
    """Philox4x32-10 of every counter row (ocn_hip.h: ocn_philox4x32): ``ctr`` int32 [n, 4] holds the bit patterns of the four
    uint32 counter words, ``key0`` / ``key1`` are the key words (0 .. 2^32 - 1); returns the four output words, int32 [n, 4]
    bit patterns again.  The generator of the samplers below, exposed so that its stream of words can be pinned on its own."""
    _req(ctr, torch.int32, "ctr", 2)
    if ctr.shape[1] != 4:
        raise ValueError(f"ctr: expected [n, 4], got {tuple(ctr.shape)}")
    key0, key1 = int(key0), int(key1)
    if not (0 <= key0 < (1 << 32) and 0 <= key1 < (1 << 32)):
        raise ValueError("key words must be in 0 .. 2^32 - 1")
    out = torch.empty_like(ctr)
    if ctr.shape[0]:
        check(_lib.lib().ocn_philox4x32(ptr(ctr), key0, key1, ctr.shape[0], ptr(out), stream_ptr()), "ocn_philox4x32")
        _mark("philox4x32")
    return out


def sample_stage_cols() -> int:
    """Columns of a row ``ocn_sample_complement_rows`` stages in LDS; longer rows are searched in memory."""
    return int(_lib.lib().ocn_sample_stage_cols())


def _known_args(rowptrK: Tensor, colK: Tensor) -> int:
    """The operand checks of the samplers' ``known`` matrix: square (its size is its row count), 1 .. 2^31 - 1 rows.  Its columns
    must be sorted and duplicate-free in every row, as every ``SparseTensor`` of the project stores them."""
    _req(rowptrK, torch.int64, "rowptrK", 1); _req(colK, torch.int32, "colK", 1)
    n = rowptrK.numel() - 1
    if not 0 < n < (1 << 31):
        raise ValueError(f"known has {n} rows: int32 columns serve 1 .. 2^31 - 1")
    return n


def _seed(seed: int) -> int:
    seed = int(seed)
    if not 0 <= seed < (1 << 64):
        raise ValueError("seed must be in 0 .. 2^64 - 1")
    return seed


@_on_device
def complement_count(rowptrK: Tensor, colK: Tensor) -> Tensor:
    """count[s] = n - |known[s,:] U {s}| for every row of the square ``known`` (ocn_hip.h: ocn_complement_count): int32 [n].
    ``scan_i32`` of it gives the prefix ``sample_complement_pairs`` searches."""
    n = _known_args(rowptrK, colK)
    count = torch.empty(n, dtype=torch.int32, device=rowptrK.device)
    check(_lib.lib().ocn_complement_count(ptr(rowptrK), ptr(colK), n, ptr(count), stream_ptr()), "ocn_complement_count")
    _mark("complement_count")
    return count


@_on_device
def sample_complement_rows(rowptrK: Tensor, colK: Tensor, rows: Tensor, per: int, seed: int, first: int = 0) -> Tensor:
    """``per`` uniform draws, with replacement, from the columns outside ``known[s,:] U {s}`` for every s = rows[q] (ocn_hip.h:
    ocn_sample_complement_rows): int64 [Q, per], -1 where nothing is left outside.  Sample j of query q is fixed by
    (seed, first + q, j, known) alone."""
    n = _known_args(rowptrK, colK)
    _req(rows, torch.int64, "rows", 1)
    per, first = int(per), int(first)
    if not 1 <= per < (1 << 31):
        raise ValueError(f"per must be in 1 .. 2^31 - 1, got {per}")
    if first < 0:
        raise ValueError(f"first must not be negative, got {first}")
    seed = _seed(seed)
    check_edges(rows, rows, n, n)
    Q = rows.numel()
    out = torch.empty(Q, per, dtype=torch.int64, device=rows.device)
    if Q:
        check(_lib.lib().ocn_sample_complement_rows(ptr(rowptrK), ptr(colK), n, ptr(rows), Q, per, first, seed, ptr(out),
                                                    stream_ptr()), "ocn_sample_complement_rows")
        _mark("sample_complement_rows")
    return out


@_on_device
def sample_complement_pairs(rowptrK: Tensor, colK: Tensor, cptr: Tensor, num: int, seed: int, first: int = 0) -> Tensor:
    """``num`` uniform draws, with replacement, from the ordered pairs (s, c), c outside ``known[s,:] U {s}`` (ocn_hip.h:
    ocn_sample_complement_pairs): int64 [2, num], sources then targets.  ``cptr``: ``scan_i32(complement_count(...))`` of the
    same matrix; a total ``cptr[-1]`` of 0 is the caller's to refuse (the kernel then writes -1).  Sample t is fixed by
    (seed, first + t, known) alone."""
    n = _known_args(rowptrK, colK)
    if _req(cptr, torch.int64, "cptr", 1).numel() != n + 1:
        raise ValueError("cptr: one entry per row and the total")
    num, first = int(num), int(first)
    if num < 0 or first < 0:
        raise ValueError(f"num and first must not be negative, got {num}, {first}")
    seed = _seed(seed)
    out = torch.empty(2, num, dtype=torch.int64, device=rowptrK.device)
    if num:
        check(_lib.lib().ocn_sample_complement_pairs(ptr(rowptrK), ptr(colK), n, ptr(cptr), num, first, seed, ptr(out),
                                                     stream_ptr()), "ocn_sample_complement_pairs")
        _mark("sample_complement_pairs")
    return out


def sample_two_hop_window_cols() -> int:
    """Columns of one LDS window of ``ocn_sample_two_hop`` (the 2-hop bitmap less the thread prefixes the selection searches)."""
    return int(_lib.lib().ocn_sample_two_hop_window_cols())


@_on_device
def sample_two_hop(rowptrA: Tensor, colA: Tensor, rowptrM: Tensor, colM: Tensor, rows: Tensor, sptr: Tensor, seed: int,
                   sid: Optional[Tensor] = None, first: int = 0, drop_self: bool = True, total: Optional[int] = None,
                   want_count: bool = False, window_cols: int = 0):
    """Uniform draws, with replacement, from the set ``two_hop_diff_fill`` lists for s = rows[q] — without listing it (ocn_hip.h:
    ocn_sample_two_hop).  Query q owns the slots ``sptr[q] .. sptr[q + 1]`` of the result (``sptr``: int64 [Q + 1] ascending
    from 0, trusted; ``total`` = ``sptr[-1]`` where the caller knows it, else read here: one host sync): int64 [total], -1 in
    the slots of a query whose set is empty.  Slot i is fixed by (seed, first + q, i - sptr[q], A, M, s), or with ``sid`` (int64
    [total], non-negative sample ids) by (seed, sid[i], A, M, s) and ``first`` is ignored.  ``want_count``: returns (out, count)
    with count int32 [Q] = ``two_hop_diff_count`` of the same operands.  ``window_cols``: 0, the library's window, except in
    tests of the sweep."""
    Q, n = _two_hop_args(rowptrA, colA, rowptrM, colM, rows, window_cols, sample_two_hop_window_cols)
    T = _scan_total(sptr, Q, total, "sptr", "sptr: one entry per query and the total")
    first = int(first)
    if first < 0:
        raise ValueError(f"first must not be negative, got {first}")
    seed = _seed(seed)
    if sid is not None:
        if _req(sid, torch.int64, "sid", 1).numel() != T:
            raise ValueError(f"sid: one sample id per slot ({T}), got {sid.numel()}")
        if sid.device != rows.device:
            raise RuntimeError(f"sample_two_hop: operands on different devices ({rows.device}, {sid.device})")
    out = torch.empty(max(T, 1), dtype=torch.int64, device=rows.device)      # (a count-only call still hands the entry an address)
    count = torch.empty(Q, dtype=torch.int32, device=rows.device) if want_count else None
    if Q and (T or want_count):
        check(_lib.lib().ocn_sample_two_hop(ptr(rowptrA), ptr(colA), ptr(rowptrM), ptr(colM), n, ptr(rows), Q, int(bool(drop_self)),
                                            int(window_cols), ptr(sptr), ptr(sid), first, seed, ptr(count), ptr(out), stream_ptr()),
              "ocn_sample_two_hop")
        _mark("sample_two_hop")
    out = out[:T]
    return (out, count) if want_count else out


def rw_max_walks() -> int:
    """The largest ``walks`` of ``rw_visits_count`` / ``rw_visits_fill`` (ocn_hip.h: ocn_rw_max_walks): what the LDS of a CU
    holds at ``length=3``."""
    return int(_lib.lib().ocn_rw_max_walks())


def _rw_args(rowptrA: Tensor, colA: Tensor, rowptrM: Tensor, colM: Tensor, rows: Tensor, walks: int, length: int,
             seed: int) -> Tuple[int, int, int, int, int]:
    """The operand checks of both random-walk passes: those of the row difference (A and M of one size; M's columns sorted and
    duplicate-free, which this layer cannot see), ``walks`` in 1 .. ``rw_max_walks()``, ``length`` 2 or 3, the seed.
    Returns (Q, n, walks, length, seed)."""
    Q = _row_diff_args(rowptrA, colA, rowptrM, colM, rows)
    n = rowptrA.numel() - 1
    if not 0 < n < (1 << 31):
        raise ValueError(f"A has {n} rows: int32 columns serve 1 .. 2^31 - 1")
    if isinstance(walks, bool) or isinstance(length, bool):
        raise ValueError(f"walks and length must be ints, got {walks!r}, {length!r}")
    walks, length = int(walks), int(length)
    if not 1 <= walks <= rw_max_walks():
        raise ValueError(f"walks must be in 1..{rw_max_walks()}, got {walks}")
    if length not in (2, 3):
        raise ValueError(f"length must be 2 or 3, got {length}")
    return Q, n, walks, length, _seed(seed)


@_on_device
def rw_visits_count(rowptrA: Tensor, colA: Tensor, rowptrM: Tensor, colM: Tensor, rows: Tensor, walks: int, length: int,
                    seed: int) -> Tensor:
    """count[q] = the nodes that the second or third step of one of ``walks`` uniform walks of ``length`` steps from
    s = rows[q] reaches and that are neither s nor in row s of M (ocn_hip.h: ocn_rw_visits_count): int32 [Q].  ``scan_i32`` of
    it gives the offsets ``rw_visits_fill`` writes at.  A source's walks are fixed by (seed, s, A, walks, length)."""
    Q, n, walks, length, seed = _rw_args(rowptrA, colA, rowptrM, colM, rows, walks, length, seed)
    count = torch.empty(Q, dtype=torch.int32, device=rows.device)
    if Q:
        check(_lib.lib().ocn_rw_visits_count(ptr(rowptrA), ptr(colA), ptr(rowptrM), ptr(colM), n, ptr(rows), Q, walks, length, seed,
                                             ptr(count), stream_ptr()), "ocn_rw_visits_count")
        _mark("rw_visits_count")
    return count


@_on_device
def rw_visits_fill(rowptrA: Tensor, colA: Tensor, rowptrM: Tensor, colM: Tensor, rows: Tensor, walks: int, length: int,
                   seed: int, off: Tensor, decay: float = 0.0, total: Optional[int] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """The same walks again, written (ocn_hip.h: ocn_rw_visits_fill): (edges int64 [T, 2], val float32 [T], visits int32 [T, 2]).
    From ``off[q]`` on, in ascending node id: the pair (s, v), ``visits`` = (c2, c3) — the walks whose second / third step ends
    in v — and ``val = float32(c2) + float32(decay) * float32(c3)``, two roundings (``float32(c2)`` at ``length=2``, where
    ``decay`` must stay 0).  ``off``: ``scan_i32(rw_visits_count(...))`` of the same operands; ``total`` as for
    ``row_diff_fill``."""
    import math
    Q, n, walks, length, seed = _rw_args(rowptrA, colA, rowptrM, colM, rows, walks, length, seed)
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not math.isfinite(decay) or decay < 0:
        raise ValueError(f"decay must be a finite number >= 0, got {decay!r}")
    decay = float(torch.tensor(float(decay), dtype=torch.float32).item())          # (rounded to fp32 here, not by the ABI)
    if not math.isfinite(decay):
        raise ValueError("decay is not finite in float32")
    if length == 2 and decay != 0.0:
        raise ValueError("decay belongs to length=3")
    T, edges = _fill_pairs(off, Q, total, rows.device)
    val = torch.empty(T, dtype=torch.float32, device=rows.device)
    visits = torch.empty(T, 2, dtype=torch.int32, device=rows.device)
    if Q and T:
        check(_lib.lib().ocn_rw_visits_fill(ptr(rowptrA), ptr(colA), ptr(rowptrM), ptr(colM), n, ptr(rows), Q, walks, length, seed,
                                            ptr(off), decay, ptr(edges), ptr(val), ptr(visits), stream_ptr()), "ocn_rw_visits_fill")
        _mark("rw_visits_fill")
    return edges, val, visits


def mips_max_m() -> int:
    """The largest ``m`` of ``mips_topm_i8`` (ocn_hip.h: ocn_mips_max_m) — ``segment_topk_max_k()``."""
    return int(_lib.lib().ocn_mips_max_m())


def mips_h_align() -> int:
    """The width of ``mips_topm_i8`` operands is a multiple of this (ocn_hip.h: ocn_mips_h_align): the K step of the int8 MFMA
    pair.  ``quantize_rows_i8`` pads to it."""
    return int(_lib.lib().ocn_mips_h_align())


MIPS_H_MAX = 1024                # include/ocn_hip.h, ocn_mips_topm_i8: |dot| <= 1024 * 127^2 < 2^24 stays exact in fp32


def quantize_rows_i8(x: Tensor, normalize: bool = False) -> Tuple[Tensor, Tensor]:
    """Symmetric per-row int8 quantisation of an fp32 matrix ``x`` [R, H], in plain torch on ``x``'s device: (``q`` int8
    [R, Hp], ``scale`` float32 [R]) with ``q * scale[:, None]`` ~ ``x``.  ``normalize``: every row is divided by its L2 norm
    first (cosine retrieval; an all-zero row stays zero).  ``scale = amax(|row|) / 127`` (1 for an all-zero row), ``q =
    clamp(round(x / scale), -127, 127)`` — ``|x - q * scale| <= scale / 2`` up to the rounding of the division.  ``Hp`` is ``H``
    padded with zeros up to a multiple of ``mips_h_align()``: padding changes no dot product.  A non-finite ``x`` raises
    ValueError (one host sync)."""
    if not isinstance(x, Tensor) or x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError("x must be a float32 [R, H] matrix")
    R, H = x.shape
    if H < 1:
        raise ValueError("x must have at least one column")
    if R and not bool(torch.isfinite(x).all()):
        raise ValueError("x holds values that are not finite: they have no int8 image")
    if normalize:
        nrm = torch.linalg.vector_norm(x, dim=1, keepdim=True)
        x = x / torch.where(nrm > 0, nrm, torch.ones_like(nrm))
    amax = x.abs().amax(dim=1) if R else x.new_zeros(0)
    scale = torch.where(amax > 0, amax / 127.0, torch.ones_like(amax))
    q = torch.round(x / scale[:, None]).clamp_(-127, 127).to(torch.int8)
    align = mips_h_align()
    Hp = (H + align - 1) // align * align
    if Hp != H:
        q = torch.nn.functional.pad(q, (0, Hp - H))
    return q.contiguous(), scale.contiguous()


def _aligned16(t: Tensor) -> Tensor:
    """``t``, or a copy where its storage offset leaves it off a 16-byte boundary (the kernel reads 16 bytes at a time)."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


@_on_device
def mips_topm_i8(query_q: Tensor, keys_q: Tensor, kscale: Tensor, m: int, rows: Optional[Tensor] = None,
                 excl: Optional[Tuple[Tensor, Tensor]] = None, drop_self: bool = True, n_split: int = 0,
                 wsd=None) -> Tuple[Tensor, Tensor]:
    """For every query the ``m`` nodes with the largest ``float32(dot) * kscale[n]`` (ocn_hip.h: ocn_mips_topm_i8): (``val``
    float32 [Q, m], ``node`` int64 [Q, m]), best first, padded with -inf / -1.  ``query_q`` int8 [Q, H], ``keys_q`` int8
    [N, H], ``kscale`` float32 [N] — ``quantize_rows_i8`` makes them; ``dot`` is the exact int32 inner product, the multiply
    the only rounding.  ``rows`` int64 [Q]: the node id of every query; then ``drop_self`` excludes it and ``excl`` =
    (rowptr int64 [N + 1], col int32), a CSR with sorted duplicate-free columns, excludes the nodes of its row.  Without ``rows``
    every node is eligible.  Order: higher value first, +0.0 == -0.0, equal values to the lower node id.  ``n_split`` (0 = auto)
    slices the key range over workgroups; the result does not depend on it."""
    if isinstance(m, bool) or not isinstance(m, int) or not 1 <= m <= mips_max_m():
        raise ValueError(f"m must be in 1..{mips_max_m()}, got {m!r}")
    if isinstance(n_split, bool) or not isinstance(n_split, int) or n_split < 0:
        raise ValueError(f"n_split must be an int >= 0 (0 = automatic), got {n_split!r}")
    _req(query_q, torch.int8, "query_q", 2); _req(keys_q, torch.int8, "keys_q", 2); _req(kscale, torch.float32, "kscale", 1)
    Q, H = query_q.shape
    N = keys_q.shape[0]
    if keys_q.shape[1] != H:
        raise ValueError(f"query_q has {H} columns, keys_q {keys_q.shape[1]}")
    if H < 1 or H % mips_h_align() or H > MIPS_H_MAX:
        raise ValueError(f"the width must be a multiple of {mips_h_align()} up to {MIPS_H_MAX}, got {H} (quantize_rows_i8 pads)")
    if not 0 < N < (1 << 31):
        raise ValueError(f"keys_q has {N} rows: node ids serve 1 .. 2^31 - 1")
    if kscale.numel() != N:
        raise ValueError(f"kscale: one scale per key ({N}), got {kscale.numel()}")
    rp = col = None
    if rows is None:
        if excl is not None:
            raise ValueError("excl needs rows: the exclusion is the row of a query's node id")
    else:
        if _req(rows, torch.int64, "rows", 1).numel() != Q:
            raise ValueError(f"rows: one node id per query ({Q}), got {rows.numel()}")
        check_edges(rows, rows, N, N)
        if excl is not None:
            rp, col = excl
            _req(rp, torch.int64, "excl rowptr", 1); _req(col, torch.int32, "excl col", 1)
            if rp.numel() != N + 1:
                raise ValueError(f"excl has {rp.numel() - 1} rows, the keys {N}")
            if not col.numel():
                col = torch.zeros(1, dtype=torch.int32, device=col.device)
    dev = query_q.device
    for name, t in (("keys_q", keys_q), ("kscale", kscale), ("rows", rows), ("excl rowptr", rp), ("excl col", col)):
        if t is not None and t.device != dev:            # (rows is a keyword and excl a tuple: _on_device does not see them)
            raise RuntimeError(f"mips_topm_i8: {name} is on {t.device}, query_q on {dev}")
    val = torch.empty(Q, m, dtype=torch.float32, device=dev)
    node = torch.empty(Q, m, dtype=torch.int64, device=dev)
    if Q:
        nbytes = int(_lib.lib().ocn_mips_workspace_bytes(Q, N, m, n_split))
        if nbytes < 0:
            raise _lib.OcnHipError("ocn_mips_workspace_bytes refused its arguments")
        ws = buf(wsd, "mips_ws", (nbytes + 7) // 8, torch.int64, dev)
        qa, ka, sa = _aligned16(query_q), _aligned16(keys_q), _aligned16(kscale)
        check(_lib.lib().ocn_mips_topm_i8(ptr(qa), ptr(ka), ptr(sa), Q, N, H, ptr(rows), ptr(rp), ptr(col), 1 if drop_self else 0,
                                          m, n_split, ptr(val), ptr(node), ptr(ws), stream_ptr()), "ocn_mips_topm_i8")
        _mark("mips_topm_i8", 2.0 * Q * N * H)
    return val, node


CLASS_RANGES = 7                 # include/ocn_hip.h: OCN_CLASS_RANGES
R_CN1, R_BOTH, R_CN2_ONLY, R_ANY, R_NONE, R_CN1_ONLY, R_ALL = range(CLASS_RANGES)


@_on_device
def gather_schedule(sched: Tensor, B: int) -> bool:
    """The pooling's longest-first visiting order from the group costs the intersection pass left in ``sched[:n_groups]``
    (ocn_gather_schedule) into ``sched[n_groups:]``; False where the schedule does not apply (``sched_groups``)."""
    n_groups = sched_groups(B, SCHED_H) if sched is not None else 0
    if not n_groups:
        return False
    check(_lib.lib().ocn_gather_schedule(ptr(sched), n_groups, int(sched_segment), ptr(sched[n_groups:]), stream_ptr()), "ocn_gather_schedule")
    _mark("cn_sched")
    return True


@_on_device
def class_order(cnt1: Tensor, cnt2: Optional[Tensor], order: Optional[Tensor], wsd=None):
    """Class-major processing order for the heads (ocn_hip.h: ocn_class_order).
    Returns (order2 [B] slot -> batch row, inv [B] batch row -> slot, ranges int64 [7, 2] on the device)."""
    _req(cnt1, torch.int32, "cnt1", 1)
    B = cnt1.numel()
    dev = cnt1.device
    order2 = buf(wsd, "cls_order", B, torch.int64, dev)
    inv = buf(wsd, "cls_inv", B, torch.int64, dev)
    ranges = buf(wsd, "cls_ranges", (CLASS_RANGES, 2), torch.int64, dev)
    prefix = buf(wsd, "cls_prefix", B + 1, torch.int64, dev)
    ws = _ws(B, dev, wsd)
    check(_lib.lib().ocn_class_order(ptr(cnt1), ptr(cnt2), ptr(order), B, ptr(order2), ptr(inv), ptr(ranges),
                                     ptr(prefix), ptr(ws), stream_ptr()), "ocn_class_order")
    _mark("cn_class")
    return order2, inv, ranges


@_on_device
def cn_weights_cn6(histA: Tensor, histB: Tensor, innerprod: Tensor, exact=None, scal: Optional[Tensor] = None):
    """In place: histA -> float32 [N,4] {inv1, t, inv2, 0}, histB -> {1/S3, 0, 0, 0}; returns them and the
    device scalar nip (ocn_hip.h: ocn_cn_weights_cn6).  ``exact`` = (rowptrA, colA, src, off, flagsA, flagsB):
    order-exact S2 / S3 for a non-zero ``innerprod``, as for cn5."""
    _req(histA, torch.int64, "histA", 2); _req(histB, torch.int64, "histB", 2)
    if histA.shape != histB.shape:
        raise ValueError("histA / histB shape mismatch")
    ip = _req(innerprod.detach().reshape(1).to(torch.float32), torch.float32, "innerprod", 1)
    if scal is None:
        scal = torch.zeros(4, dtype=torch.int32, device=histA.device)
    nip = torch.empty(1, dtype=torch.float32, device=histA.device)
    s2 = s3 = None
    if exact is not None and colsum_wanted(innerprod):
        rowptrA, colA, src, off, flagsA, flagsB = exact
        s2, s3 = cn_colsum_exact(rowptrA, colA, src, off, flagsA, flagsB, None, histA, innerprod, scal)
    elif _ip_nonzero(innerprod):
        check(_lib.lib().ocn_cn5_column_stats(ptr(histA), histA.shape[0], ptr(scal), stream_ptr()), "ocn_cn5_column_stats")
    check(_lib.lib().ocn_cn_weights_cn6(ptr(histA), ptr(histB), histA.shape[0], ptr(ip), ptr(scal), ptr(nip),
                                        ptr(s2), ptr(s3), stream_ptr()), "ocn_cn_weights_cn6")
    _mark("cn_weights")
    return histA.view(torch.float32).view(-1, 4), histB.view(torch.float32).view(-1, 4), nip


@_on_device
def cn_gather3(rowptrA, colA, src, dst, off, flagsA, flagsB, wA: Tensor, wB: Tensor, nip: Tensor, h: Tensor,
               order: Optional[Tensor] = None):
    """(xcn1, xcn2, xcn3, x_i * x_j) of the 3-hop predictor.  fp32 rows only: a bf16 / f16 table raises TypeError."""
    refuse_compact_table(h, "cn6 (cn_gather3)")
    _req(wA, torch.float32, "weightsA", 2); _req(wB, torch.float32, "weightsB", 2)
    _req(h, torch.float32, "h", 2)
    if wA.shape != (h.shape[0], 4) or wB.shape != (h.shape[0], 4):
        raise ValueError("weights must be [N,4] with N = h.shape[0]")
    B, H = src.numel(), h.shape[1]
    if H not in LN_WIDTHS:
        raise NotImplementedError(f"cn6 pooling supports hidden widths {LN_WIDTHS}, got {H}")
    out = torch.empty(4, B, H, dtype=torch.float32, device=h.device)
    check(_lib.lib().ocn_cn_gather3(ptr(rowptrA), ptr(colA), ptr(src), ptr(dst), ptr(order), B, ptr(off), ptr(flagsA),
                                    ptr(flagsB), ptr(wA), ptr(wB), ptr(nip), ptr(h), H, ptr(out[0]), ptr(out[1]),
                                    ptr(out[2]), ptr(out[3]), stream_ptr()), "ocn_cn_gather3")
    _mark("cn_gather")
    return out[0], out[1], out[2], out[3]


@_on_device
def cn_gather3_backward(rowptrA, colA, src, dst, off, flagsA, flagsB, wA: Tensor, wB: Tensor, nip: Tensor, h: Tensor,
                        g1: Tensor, g2: Tensor, g3: Tensor, g4: Tensor, order: Optional[Tensor] = None) -> Tensor:
    """Gradient of cn6's (xcn1, xcn2, xcn3, xij) with respect to h (ocn_hip.h: ocn_cn_gather3_backward; fp32 atomics)."""
    B, H = src.numel(), h.shape[1]
    for t, nm in ((g1, "g1"), (g2, "g2"), (g3, "g3"), (g4, "g4")):
        if _req(t, torch.float32, nm, 2).shape != (B, H):
            raise ValueError(f"{nm}: expected [{B}, {H}]")
    if H not in LN_WIDTHS:
        raise NotImplementedError(f"cn6 pooling backward supports hidden widths {LN_WIDTHS}, got {H}")
    dh = torch.zeros_like(h)
    check(_lib.lib().ocn_cn_gather3_backward(ptr(rowptrA), ptr(colA), ptr(src), ptr(dst), ptr(order), B, ptr(off), ptr(flagsA),
                                             ptr(flagsB), ptr(wA), ptr(wB), ptr(nip), ptr(h), H, ptr(g1), ptr(g2), ptr(g3), ptr(g4),
                                             ptr(dh), stream_ptr()), "ocn_cn_gather3_backward")
    return dh


@_on_device
def cn_gather_backward(rowptrA, colA, src, dst, off, flags, wc, weights: Tensor, h: Tensor, g1: Tensor, g2: Tensor,
                       g3: Tensor, order: Optional[Tensor] = None) -> Tensor:
    """Gradient of (xcn1, xcn2, xij) with respect to h: node by node in a fixed order (``deterministic_backward``, the
    default), or with fp32 atomics (``OCN_ATOMIC_BACKWARD=1``)."""
    B, H = src.numel(), h.shape[1]
    for t, nm in ((g1, "g1"), (g2, "g2"), (g3, "g3")):
        if _req(t, torch.float32, nm, 2).shape != (B, H):
            raise ValueError(f"{nm}: expected [{B}, {H}]")
    if H not in LN_WIDTHS:
        raise NotImplementedError(f"pooling backward supports hidden widths {LN_WIDTHS}, got {H}")
    dh = torch.zeros_like(h)
    if deterministic_backward:
        l = _lib.lib()
        cap, N = flags.numel(), h.shape[0]
        ws = torch.empty(int(l.ocn_cn_gather_backward_det_workspace_bytes(N, B, cap)), dtype=torch.uint8, device=h.device)
        check(l.ocn_cn_gather_backward_det(ptr(rowptrA), ptr(colA), ptr(src), ptr(dst), B, ptr(off), ptr(flags), ptr(wc), cap,
                                           ptr(weights), ptr(h), N, H, ptr(g1), ptr(g2), ptr(g3), ptr(dh), ptr(ws),
                                           stream_ptr()), "ocn_cn_gather_backward_det")
        return dh
    check(_lib.lib().ocn_cn_gather_backward(ptr(rowptrA), ptr(colA), ptr(src), ptr(dst), ptr(order), B, ptr(off),
                                            ptr(flags), ptr(wc), ptr(weights), ptr(h), H, ptr(g1), ptr(g2), ptr(g3),
                                            ptr(dh), stream_ptr()), "ocn_cn_gather_backward")
    return dh


@_on_device
def cn_gather_backward_lists(rowptrA, colA, src, dst, off, flags, N: int):
    """The per-node key lists of the deterministic pooling backward (ocn_hip.h: ocn_cn_gather_backward_det_lists), for
    inspection: (col_off int64 [N + 1], keys int32 [col_off[N]]).  One host sync (the list total)."""
    l = _lib.lib()
    B, cap = src.numel(), flags.numel()
    ws = torch.empty(int(l.ocn_cn_gather_backward_det_workspace_bytes(N, B, cap)), dtype=torch.uint8, device=src.device)
    check(l.ocn_cn_gather_backward_det_lists(ptr(rowptrA), ptr(colA), ptr(src), ptr(dst), B, ptr(off), ptr(flags), cap, N, ptr(ws),
                                             stream_ptr()), "ocn_cn_gather_backward_det_lists")
    col_off = ws[: (N + 1) * 8].view(torch.int64)
    k0 = int(l.ocn_cn_gather_backward_det_keys_offset(N))
    return col_off, ws[k0: k0 + 4 * _total(col_off[N])].view(torch.int32)


SPMM_MODES = {"sum": 0, "add": 0, "mean": 1, "max": 2}


@_on_device
def spmm_csr(rowptr: Tensor, col: Tensor, x: Tensor, pre: Optional[Tensor] = None,
             post: Optional[Tensor] = None, mode: str = "sum", edge_scale: bool = False,
             self_mode: int = 0, val: Optional[Tensor] = None) -> Tensor:
    _req(rowptr, torch.int64, "rowptr", 1); _req(col, torch.int32, "col", 1)
    _req(x, torch.float32, "x", 2)
    n = rowptr.numel() - 1
    if pre is not None and (_req(pre, torch.float32, "pre", 1).numel() != x.shape[0]):
        raise ValueError("pre must have one entry per row of x")
    if pre is not None and edge_scale and n > x.shape[0]:      # pre lives in the column space; edge_scale reads pre[r] too
        raise ValueError("edge_scale reads pre[r] of every output row: the operator has more rows than pre has entries")
    if post is not None and (_req(post, torch.float32, "post", 1).numel() != n):
        raise ValueError("post must have one entry per output row")
    if self_mode and x.shape[0] != n:
        raise ValueError("self term needs a square operator")
    if val is not None and _req(val, torch.float32, "val", 1).numel() != col.numel():
        raise ValueError("val must have one entry per stored column")
    y = torch.empty(n, x.shape[1], dtype=torch.float32, device=x.device)
    check(_lib.lib().ocn_spmm_csr(ptr(rowptr), ptr(col), ptr(val), n, ptr(x), x.shape[1], ptr(pre), ptr(post),
                                  SPMM_MODES[mode], int(edge_scale), int(self_mode), ptr(y), stream_ptr()),
          "ocn_spmm_csr")
    return y


@_on_device
def spmm_csr_rows(rowptr: Tensor, col: Tensor, x: Tensor, rows: Tensor, pre: Optional[Tensor] = None,
                  post: Optional[Tensor] = None, mode: str = "sum", edge_scale: bool = False,
                  self_mode: int = 0, val: Optional[Tensor] = None) -> Tensor:
    """``spmm_csr(...)[rows]`` without forming the other rows (ocn_hip.h: ocn_spmm_csr_rows): a compact ``[len(rows), F]``
    matrix, bit for bit the listed rows of the full product — both entries run one kernel body.  ``rows``: int64, ascending,
    duplicate-free, each in ``[0, n)``; ``pre`` / ``post`` stay indexed by global ids.  The result is a new tensor: the launch
    never writes into ``x``."""
    _req(rowptr, torch.int64, "rowptr", 1); _req(col, torch.int32, "col", 1)
    _req(x, torch.float32, "x", 2); _req(rows, torch.int64, "rows", 1)
    n = rowptr.numel() - 1
    if x.shape[1] not in LN_WIDTHS:
        raise ValueError(f"spmm_csr_rows: unsupported width {x.shape[1]}")
    if pre is not None and (_req(pre, torch.float32, "pre", 1).numel() != x.shape[0]):
        raise ValueError("pre must have one entry per row of x")
    if pre is not None and edge_scale and n > x.shape[0]:      # pre lives in the column space; edge_scale reads pre[r] too
        raise ValueError("edge_scale reads pre[r] of every output row: the operator has more rows than pre has entries")
    if post is not None and (_req(post, torch.float32, "post", 1).numel() != n):
        raise ValueError("post must have one entry per output row")
    if self_mode and x.shape[0] != n:
        raise ValueError("self term needs a square operator")
    if val is not None and _req(val, torch.float32, "val", 1).numel() != col.numel():
        raise ValueError("val must have one entry per stored column")
    y = torch.empty(rows.numel(), x.shape[1], dtype=torch.float32, device=x.device)
    if rows.numel():
        if not col.numel():                               # no entries: no column array to point at; nothing reads the stand-in
            col = torch.zeros(1, dtype=torch.int32, device=x.device)
        check(_lib.lib().ocn_spmm_csr_rows(ptr(rowptr), ptr(col), ptr(val), n, ptr(x), x.shape[1], ptr(pre), ptr(post),
                                           SPMM_MODES[mode], int(edge_scale), int(self_mode), ptr(rows), rows.numel(), ptr(y),
                                           stream_ptr()), "ocn_spmm_csr_rows")
    return y


@_on_device
def sddmm_csr(rowptr: Tensor, col: Tensor, g: Tensor, x: Tensor, pre: Optional[Tensor] = None,
              post: Optional[Tensor] = None, mode: str = "sum", edge_scale: bool = False,
              self_mode: int = 0, val: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """The sampled dense-dense product on the pattern of the operator (ocn_hip.h: ocn_sddmm_csr): float32 [nnz],
    ``out[p] = c * <g[r], x[k]>`` for entry p = (r, k), c the coefficient ``spmm_csr`` with the same keywords gives that entry
    — the gradient of ``spmm_csr``'s result with respect to a mask on its messages, for an upstream gradient ``g``.  ``g``
    [n_rows, F], ``x`` [n_cols, F], F in ``LN_WIDTHS``; the other operands are ``spmm_csr``'s.  ``mode`` "max" and "mean" with
    ``pre`` / ``post`` / ``self_mode`` are refused.  ``out``: a float32 vector of at least nnz entries to write into (the rest
    is left alone); the result is its first nnz entries.  Column ids are trusted, as ``spmm_csr`` trusts them."""
    _req(rowptr, torch.int64, "rowptr", 1); _req(col, torch.int32, "col", 1)
    _req(g, torch.float32, "g", 2); _req(x, torch.float32, "x", 2)
    n, nnz = rowptr.numel() - 1, col.numel()
    if n < 0:
        raise ValueError("rowptr: [n_rows + 1] offsets")
    if g.shape[0] != n or g.shape[1] != x.shape[1]:
        raise ValueError("g must be [n_rows, F] with the width of x")
    if x.shape[1] not in LN_WIDTHS:
        raise ValueError(f"sddmm_csr: unsupported width {x.shape[1]}")
    if mode not in SPMM_MODES or SPMM_MODES[mode] == 2:
        raise ValueError(f"sddmm_csr: mode must be sum or mean, got {mode!r} (max has no per-message linearisation)")
    if SPMM_MODES[mode] == 1 and (pre is not None or post is not None or self_mode):
        raise ValueError("sddmm_csr: mean takes no pre / post / self term")
    if self_mode not in (0, 1, 2):
        raise ValueError(f"self_mode must be 0, 1 or 2, got {self_mode!r}")
    if pre is not None and (_req(pre, torch.float32, "pre", 1).numel() != x.shape[0]):
        raise ValueError("pre must have one entry per row of x")
    if pre is not None and edge_scale and n > x.shape[0]:      # pre lives in the column space; edge_scale reads pre[r] too
        raise ValueError("edge_scale reads pre[r] of every output row: the operator has more rows than pre has entries")
    if post is not None and (_req(post, torch.float32, "post", 1).numel() != n):
        raise ValueError("post must have one entry per output row")
    if self_mode and x.shape[0] != n:
        raise ValueError("self term needs a square operator")
    if val is not None and _req(val, torch.float32, "val", 1).numel() != nnz:
        raise ValueError("val must have one entry per stored column")
    if out is None:
        out = torch.empty(nnz, dtype=torch.float32, device=x.device)
    elif _req(out, torch.float32, "out", 1).numel() < nnz:
        raise ValueError("out must hold one entry per stored column")
    if n and nnz:
        check(_lib.lib().ocn_sddmm_csr(ptr(rowptr), ptr(col), ptr(val), n, ptr(g), ptr(x), x.shape[1], ptr(pre), ptr(post),
                                       SPMM_MODES[mode], int(edge_scale), int(self_mode), ptr(out), stream_ptr()),
              "ocn_sddmm_csr")
        _mark("sddmm_csr", 2.0 * nnz * x.shape[1])
    return out[:nnz]


@_on_device
def spmm_max_arg(rowptr: Tensor, col: Tensor, x: Tensor, val: Optional[Tensor] = None,
                 n_cols: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """(y, arg): y = the max aggregation of ``spmm_csr(mode="max")`` (valued: max_k val_ik * x_k), arg [n, F] int32 = the
    column id of each winner (first maximum in row order; -1 in an empty row) — what ``spmm_max_backward`` reads.
    ``n_cols``: the operator's column count; x must have that many rows (every column id indexes a row of x)."""
    _req(rowptr, torch.int64, "rowptr", 1); _req(col, torch.int32, "col", 1)
    _req(x, torch.float32, "x", 2)
    if n_cols is not None and x.shape[0] != n_cols:
        raise ValueError(f"x has {x.shape[0]} rows, the operator {n_cols} columns")
    n = rowptr.numel() - 1
    if val is not None and _req(val, torch.float32, "val", 1).numel() != col.numel():
        raise ValueError("val must have one entry per stored column")
    if col.numel() == 0:                                  # no entries: every row is empty
        return (torch.zeros(n, x.shape[1], dtype=torch.float32, device=x.device),
                torch.full((n, x.shape[1]), -1, dtype=torch.int32, device=x.device))
    y = torch.empty(n, x.shape[1], dtype=torch.float32, device=x.device)
    arg = torch.empty(n, x.shape[1], dtype=torch.int32, device=x.device)
    check(_lib.lib().ocn_spmm_csr_max_arg(ptr(rowptr), ptr(col), ptr(val), n, ptr(x), x.shape[1], ptr(y), ptr(arg),
                                          stream_ptr()), "ocn_spmm_csr_max_arg")
    return y, arg


@_on_device
def spmm_max_backward(rowptrT: Tensor, colT: Tensor, arg: Tensor, g: Tensor, val: Optional[Tensor] = None,
                      n_cols: Optional[int] = None) -> Tensor:
    """gx = the input gradient of ``spmm_max_arg``: gx[k] = Σ_{i: arg[i] == k} val_ik * g[i], over the CSR of Aᵀ
    (rowptrT, colT, its values ``val``), in Aᵀ's row order (deterministic).  ``n_cols``: Aᵀ's column count (= A's rows);
    arg and g must have that many rows (every column id of Aᵀ indexes a row of both)."""
    _req(rowptrT, torch.int64, "rowptrT", 1); _req(colT, torch.int32, "colT", 1)
    _req(arg, torch.int32, "arg", 2); _req(g, torch.float32, "g", 2)
    if arg.shape != g.shape:
        raise ValueError("arg and g must have the same shape")
    if n_cols is not None and arg.shape[0] != n_cols:
        raise ValueError(f"arg / g have {arg.shape[0]} rows, the transposed operator {n_cols} columns")
    if val is not None and _req(val, torch.float32, "val", 1).numel() != colT.numel():
        raise ValueError("val must have one entry per stored column")
    n = rowptrT.numel() - 1
    if colT.numel() == 0:
        return torch.zeros(n, g.shape[1], dtype=torch.float32, device=g.device)
    gx = torch.empty(n, g.shape[1], dtype=torch.float32, device=g.device)
    check(_lib.lib().ocn_spmm_max_backward(ptr(rowptrT), ptr(colT), ptr(val), n, ptr(arg), ptr(g), g.shape[1], ptr(gx),
                                           stream_ptr()), "ocn_spmm_max_backward")
    return gx


@_on_device
def deg_rsqrt(rowptr: Tensor, add: float = 1.0, val: Optional[Tensor] = None) -> Tensor:
    _req(rowptr, torch.int64, "rowptr", 1)
    n = rowptr.numel() - 1
    out = torch.empty(n, dtype=torch.float32, device=rowptr.device)
    check(_lib.lib().ocn_deg_rsqrt(ptr(rowptr), ptr(val), n, float(add), ptr(out), stream_ptr()), "ocn_deg_rsqrt")
    return out


@_on_device
def bitrows_from_csr(rowptr: Tensor, col: Tensor, n_cols: int) -> Tensor:
    """ocn_hip.h: ocn_bitrows_from_csr — the pattern as dense bit rows, int32 [n_rows, ceil(n_cols / 32)]."""
    _req(rowptr, torch.int64, "rowptr", 1); _req(col, torch.int32, "col", 1)
    n = rowptr.numel() - 1
    bits = torch.zeros(n, (int(n_cols) + 31) // 32, dtype=torch.int32, device=rowptr.device)
    check(_lib.lib().ocn_bitrows_from_csr(ptr(rowptr), ptr(col), n, ptr(bits), bits.shape[1], stream_ptr()), "ocn_bitrows_from_csr")
    return bits


def _csr_setop_args(rowptrA: Tensor, colA: Tensor, rowptrB: Tensor, colB: Tensor):
    """The operand checks of both passes of the union and of the difference.  Columns sorted and duplicate-free in every row,
    as every ``SparseTensor`` of the project stores them.  An empty column array has no address: the library gets a one-element
    stand-in it never reads."""
    _req(rowptrA, torch.int64, "rowptrA", 1); _req(colA, torch.int32, "colA", 1)
    _req(rowptrB, torch.int64, "rowptrB", 1); _req(colB, torch.int32, "colB", 1)
    if rowptrA.numel() < 1 or rowptrA.numel() != rowptrB.numel():
        raise ValueError(f"A has {rowptrA.numel() - 1} rows, B {rowptrB.numel() - 1}")
    if not colA.numel():
        colA = torch.zeros(1, dtype=torch.int32, device=colA.device)
    if not colB.numel():
        colB = torch.zeros(1, dtype=torch.int32, device=colB.device)
    return rowptrA.numel() - 1, colA, colB


def _csr_setop_count(entry: str, rowptrA: Tensor, colA: Tensor, rowptrB: Tensor, colB: Tensor) -> Tensor:
    n, colA, colB = _csr_setop_args(rowptrA, colA, rowptrB, colB)
    count = torch.empty(n, dtype=torch.int32, device=rowptrA.device)
    if n:
        check(getattr(_lib.lib(), entry)(ptr(rowptrA), ptr(colA), ptr(rowptrB), ptr(colB), n, ptr(count), stream_ptr()), entry)
    return count


def _csr_setop_fill(entry: str, rowptrA: Tensor, colA: Tensor, rowptrB: Tensor, colB: Tensor, rowptrC: Tensor,
                    total: Optional[int]) -> Tensor:
    n, colA, colB = _csr_setop_args(rowptrA, colA, rowptrB, colB)
    T = _scan_total(rowptrC, n, total, "rowptrC", "rowptrC: one entry per row and the total")
    colC = torch.empty(max(T, 1), dtype=torch.int32, device=rowptrA.device)
    if n and T:
        check(getattr(_lib.lib(), entry)(ptr(rowptrA), ptr(colA), ptr(rowptrB), ptr(colB), n, ptr(rowptrC), ptr(colC),
                                         stream_ptr()), entry)
    return colC[:T]


@_on_device
def csr_union_count(rowptrA: Tensor, colA: Tensor, rowptrB: Tensor, colB: Tensor) -> Tensor:
    """count[r] = |A[r,:] U B[r,:]| (ocn_hip.h: ocn_csr_union_count): int32 [n_rows]; ``scan_i32`` of it gives the row pointers
    ``csr_union_fill`` writes at."""
    return _csr_setop_count("ocn_csr_union_count", rowptrA, colA, rowptrB, colB)


@_on_device
def csr_union_fill(rowptrA: Tensor, colA: Tensor, rowptrB: Tensor, colB: Tensor, rowptrC: Tensor, total: Optional[int] = None) -> Tensor:
    """The columns of every row's union, ascending, int32 [rowptrC[-1]] (ocn_hip.h: ocn_csr_union_fill).  ``rowptrC``:
    ``scan_i32(csr_union_count(...))`` of the same operands; ``total`` = ``rowptrC[-1]`` where the caller has read it already."""
    return _csr_setop_fill("ocn_csr_union_fill", rowptrA, colA, rowptrB, colB, rowptrC, total)


def csr_union(rowptrA: Tensor, colA: Tensor, rowptrB: Tensor, colB: Tensor) -> Tuple[Tensor, Tensor]:
    """(rowptrC, colC) of the row-wise union: count -> scan -> fill, one host read for the output size."""
    rowptrC = scan_i32(csr_union_count(rowptrA, colA, rowptrB, colB))
    return rowptrC, csr_union_fill(rowptrA, colA, rowptrB, colB, rowptrC)


@_on_device
def csr_minus_count(rowptrA: Tensor, colA: Tensor, rowptrB: Tensor, colB: Tensor) -> Tensor:
    """count[r] = |A[r,:] \\ B[r,:]| (ocn_hip.h: ocn_csr_minus_count): int32 [n_rows]; ``scan_i32`` of it gives the row pointers
    ``csr_minus_fill`` writes at."""
    return _csr_setop_count("ocn_csr_minus_count", rowptrA, colA, rowptrB, colB)


@_on_device
def csr_minus_fill(rowptrA: Tensor, colA: Tensor, rowptrB: Tensor, colB: Tensor, rowptrC: Tensor, total: Optional[int] = None) -> Tensor:
    """The columns of every row's difference, ascending, int32 [rowptrC[-1]] (ocn_hip.h: ocn_csr_minus_fill).  ``rowptrC``:
    ``scan_i32(csr_minus_count(...))`` of the same operands; ``total`` = ``rowptrC[-1]`` where the caller has read it already."""
    return _csr_setop_fill("ocn_csr_minus_fill", rowptrA, colA, rowptrB, colB, rowptrC, total)


def csr_minus(rowptrA: Tensor, colA: Tensor, rowptrB: Tensor, colB: Tensor) -> Tuple[Tensor, Tensor]:
    """(rowptrC, colC) of the row-wise difference A \\ B: count -> scan -> fill, one host read for the output size."""
    rowptrC = scan_i32(csr_minus_count(rowptrA, colA, rowptrB, colB))
    return rowptrC, csr_minus_fill(rowptrA, colA, rowptrB, colB, rowptrC)


def _bitrows_update(fn: str, what: str, operands, bits: Tensor) -> Tensor:
    """The body of ``bitrows_insert`` / ``bitrows_remove`` = ``fn``: ``operands`` = (rowptr, col, name suffix) of the square
    matrices the entry ``ocn_<fn>`` takes, in its order and with D last; ``what`` names them in the shape error.  Returns the
    bits changed per row, int32 [n].  A matrix without entries has no column array to point at (A' after every entry has
    left): the library gets a stand-in nothing reads."""
    for rp, c, sfx in operands:
        _req(rp, torch.int64, "rowptr" + sfx, 1); _req(c, torch.int32, "col" + sfx, 1)
    _req(bits, torch.int32, "bits", 2)
    n = operands[0][0].numel() - 1
    if any(rp.numel() != n + 1 for rp, _, _ in operands) or bits.shape[0] != n or bits.shape[1] * 32 < n:
        raise ValueError(f"{fn}: {what}, D and the bit rows must all be n x n")
    changed = torch.zeros(n, dtype=torch.int32, device=bits.device)
    nnzD = operands[-1][1].numel()
    if n and nnzD:
        l = _lib.lib()
        cols = [c if c.numel() else torch.zeros(1, dtype=torch.int32, device=bits.device) for _, c, _ in operands]
        csr = [p for (rp, _, _), c in zip(operands, cols) for p in (ptr(rp), ptr(c))]
        ws = torch.empty(int(getattr(l, f"ocn_{fn}_workspace_bytes")(nnzD)), dtype=torch.uint8, device=bits.device)
        check(getattr(l, f"ocn_{fn}")(*csr, n, nnzD, ptr(bits), bits.shape[1], ptr(changed), ptr(ws), stream_ptr()), f"ocn_{fn}")
    return changed


@_on_device
def bitrows_insert(rowptrA: Tensor, colA: Tensor, rowptrT: Tensor, colT: Tensor, rowptrD: Tensor, colD: Tensor, bits: Tensor) -> Tensor:
    """ocn_hip.h: ocn_bitrows_insert — ``bits`` (the bit rows of A·A, int32 [n, words]) become those of A'·A' IN PLACE, for
    A' = (rowptrA, colA) = A U D, its transpose (rowptrT, colT) and the new entries D.  Returns ``added`` int32 [n]: the bits
    turned on per row."""
    return _bitrows_update("bitrows_insert", "A', its transpose",
                           [(rowptrA, colA, "A"), (rowptrT, colT, "T"), (rowptrD, colD, "D")], bits)


@_on_device
def bitrows_remove(rowptrA0: Tensor, colA0: Tensor, rowptrT0: Tensor, colT0: Tensor, rowptrA: Tensor, colA: Tensor,
                   rowptrT: Tensor, colT: Tensor, rowptrD: Tensor, colD: Tensor, bits: Tensor) -> Tensor:
    """ocn_hip.h: ocn_bitrows_remove — ``bits`` (the bit rows of A·A, int32 [n, words]) become those of A'·A' IN PLACE, for
    the old A = (rowptrA0, colA0) and its transpose (rowptrT0, colT0), A' = (rowptrA, colA) = A \\ D and its transpose
    (rowptrT, colT), and the removed entries D.  Returns ``removed`` int32 [n]: the bits turned off per row."""
    return _bitrows_update("bitrows_remove", "A, A', their transposes",
                           [(rowptrA0, colA0, "A0"), (rowptrT0, colT0, "T0"), (rowptrA, colA, "A"), (rowptrT, colT, "T"),
                            (rowptrD, colD, "D")], bits)


# EncoderState.refresh (ocn_amd/update.py) walks the full encoder instead of the listed rows once the listed rows hold more than
# this share of the adjacency entries the full walk reads (sum over the layers of the entries in the layer's rows, against
# layers x nnz).  Measured on one MI355X ("Refreshing h"): the row walk was level with the full pass at a
# share of 0.41 (collab shape, 3 layers, 1 000 edges) and slower at 0.59 (citation2 shape, 5 layers, ONE edge) and 0.60 (collab,
# 1 layer, 100 000 edges); nothing was measured in between.  0.4 = the largest share at which it did not lose, rounded down.
refresh_full_share = 0.4


@_on_device
def rows_neighbourhood(rowptrT: Tensor, colT: Tensor, rows: Tensor, bits: Tensor) -> Tensor:
    """ocn_hip.h: ocn_rows_neighbourhood — ORs into ``bits`` (ONE bit row, int32 [ceil(n / 32)], the caller's, never cleared
    here) the bit of every id in ``rows`` (int64) and of every column of those rows of (rowptrT, colT): the CSR whose row k
    lists the rows that read column k, the adjacency itself where it is symmetric.  Returns ``bits``."""
    _req(rowptrT, torch.int64, "rowptrT", 1); _req(colT, torch.int32, "colT", 1)
    _req(rows, torch.int64, "rows", 1); _req(bits, torch.int32, "bits", 1)
    n = rowptrT.numel() - 1
    if n < 0 or bits.numel() != (n + 31) // 32:
        raise ValueError(f"rows_neighbourhood: {bits.numel()} words of bits for {n} rows")
    if n and rows.numel():
        l = _lib.lib()
        if not colT.numel():
            colT = torch.zeros(1, dtype=torch.int32, device=bits.device)
        ws = torch.empty(int(l.ocn_rows_neighbourhood_workspace_bytes(rows.numel())), dtype=torch.uint8, device=bits.device)
        check(l.ocn_rows_neighbourhood(ptr(rowptrT), ptr(colT), n, ptr(rows), rows.numel(), ptr(bits), ptr(ws), stream_ptr()),
              "ocn_rows_neighbourhood")
    return bits


@_on_device
def bits_to_list(bits: Tensor, n_bits: int) -> Tensor:
    """The ids of the set bits of ONE bit row (int32 [ceil(n_bits / 32)]), ascending, int64 (ocn_hip.h: ocn_bitlist_count ->
    scan -> ocn_bitlist_fill).  One host read for the output size."""
    _req(bits, torch.int32, "bits", 1)
    n_bits = int(n_bits)
    if n_bits < 0 or bits.numel() != (n_bits + 31) // 32:
        raise ValueError(f"bits_to_list: {bits.numel()} words for {n_bits} bits")
    if not n_bits:
        return torch.empty(0, dtype=torch.int64, device=bits.device)
    l = _lib.lib()
    cnt = torch.empty(bits.numel(), dtype=torch.int32, device=bits.device)
    check(l.ocn_bitlist_count(ptr(bits), n_bits, ptr(cnt), stream_ptr()), "ocn_bitlist_count")
    off = scan_i32(cnt)
    total = _total(off[-1])
    out = torch.empty(max(total, 1), dtype=torch.int64, device=bits.device)
    if total:
        check(l.ocn_bitlist_fill(ptr(bits), n_bits, ptr(off), ptr(out), stream_ptr()), "ocn_bitlist_fill")
    return out[:total]


@_on_device
def bitrows_to_cols(bits: Tensor, n_cols: int, rowptr: Tensor) -> Tensor:
    """The column ids of dense bit rows, ascending per row, at the row pointers of their counts (ocn_hip.h: ocn_bitrows_fill).
    One host read for the output size."""
    _req(bits, torch.int32, "bits", 2)
    n = bits.shape[0]
    nnz = _scan_total(rowptr, n, None, "rowptr", "rowptr: one entry per bit row and the total")
    col = torch.empty(max(nnz, 1), dtype=torch.int32, device=bits.device)
    if nnz:
        check(_lib.lib().ocn_bitrows_fill(ptr(bits), bits.shape[1], n, int(n_cols), ptr(rowptr), ptr(col), stream_ptr()), "ocn_bitrows_fill")
    return col[:nnz]


@_on_device
def spgemm_pattern(rowptrA, colA, rowptrB, colB, n_cols_b: int, defer_fill: bool = False, want_bitmap: bool = True):
    """CSR pattern of A·B (columns ascending) and, when it fits ``a2_bitmap_max_bytes`` (and ``want_bitmap``), the same
    rows as dense bit rows.  One host sync for the output size — with ``defer_fill`` and bit rows, not before somebody calls
    the returned thunk: ``(rowptrC, fill, bitmap)`` where ``fill()`` -> colC runs the second pass (the counting pass, the scan
    of the row lengths and the bit rows are done)."""
    _req(rowptrA, torch.int64, "rowptrA", 1); _req(colA, torch.int32, "colA", 1)
    _req(rowptrB, torch.int64, "rowptrB", 1); _req(colB, torch.int32, "colB", 1)
    l = _lib.lib()
    if n_cols_b > l.ocn_spgemm_max_cols():
        raise NotImplementedError(f"A·B pattern with {n_cols_b} columns exceeds the LDS bitmap "
                                  f"({l.ocn_spgemm_max_cols()}); the reference does not form A² at "
                                  "that size either (it uses the per-batch walk-count route)")
    n = rowptrA.numel() - 1
    dev = colA.device
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    words = (n_cols_b + 31) // 32
    bitmap = None
    if want_bitmap and n * words * 4 <= a2_bitmap_max_bytes and n > 0:
        bitmap = torch.empty(n, words, dtype=torch.int32, device=dev)       # every row is written in full
    check(l.ocn_spgemm_pattern_count(ptr(rowptrA), ptr(colA), n, ptr(rowptrB), ptr(colB), n_cols_b,
                                     ptr(cnt), ptr(bitmap), words, stream_ptr()), "ocn_spgemm_pattern_count")
    rowptrC = scan_i32(cnt)

    def fill() -> Tensor:
        nnz = _total(rowptrC[-1])
        colC = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)[:nnz]
        if nnz:
            with torch.cuda.device(dev):
                check(l.ocn_spgemm_pattern_fill(ptr(rowptrA), ptr(colA), n, ptr(rowptrB), ptr(colB), n_cols_b,
                                                ptr(rowptrC), ptr(colC), stream_ptr()), "ocn_spgemm_pattern_fill")
        return colC
    if defer_fill and bitmap is not None:
        return rowptrC, fill, bitmap
    return rowptrC, fill(), bitmap


def small_graph_cols() -> int:
    """ocn_hip.h: ocn_cn_flags_small_graph_cols — up to this many columns the intersection pass reads T2's row lengths beside its
    bit rows (so a product whose rows are built on demand is not for such graphs)."""
    return int(_lib.lib().ocn_cn_flags_small_graph_cols())


lazy_product_rows = os.environ.get("OCN_LAZY_PRODUCT", "1") != "0"     # a product formed under autograd builds its bit rows on demand (sparse._lazy_product)


def spgemm_max_cols() -> int:
    return int(_lib.lib().ocn_spgemm_max_cols())


@_on_device
def spgemm_bit_rows(rowptrA, colA, rowptrB, colB, n_cols_b: int, rows: Tensor, done: Tensor, bitmap: Tensor) -> None:
    """ocn_hip.h: ocn_spgemm_bit_rows — the dense bit rows ``rows`` (int64 ids) of A·B that ``done`` (int32 per row) does not
    mark yet, into ``bitmap`` [n_rows, words]; on the current stream."""
    _req(rowptrA, torch.int64, "rowptrA", 1); _req(colA, torch.int32, "colA", 1)
    _req(rowptrB, torch.int64, "rowptrB", 1); _req(colB, torch.int32, "colB", 1)
    _req(rows, torch.int64, "rows", 1); _req(done, torch.int32, "done", 1); _req(bitmap, torch.int32, "bitmap", 2)
    n = rowptrA.numel() - 1
    if done.numel() != n or bitmap.shape[0] != n or bitmap.shape[1] * 32 < n_cols_b:
        raise ValueError("spgemm_bit_rows: done / bitmap do not match the product")
    _mark("begin")
    check(_lib.lib().ocn_spgemm_bit_rows(ptr(rowptrA), ptr(colA), n, ptr(rowptrB), ptr(colB), n_cols_b, ptr(rows), rows.numel(),
                                         ptr(done), ptr(bitmap), bitmap.shape[1], stream_ptr()), "ocn_spgemm_bit_rows")
    _mark("adj2_rows")


dense_adj2_max_nodes = 32768      # block route: A as a dense int8 matrix (n^2 bytes, twice) up to this many nodes
# utils.sparse_tensor_multiply (the drivers' --adj2byblock call, NeighborOverlap_large.py:116): False = the intended A²,
# True = the reference as written (utils.py:318-321, SURVEY Q7: block-local indices, all blocks folded onto one corner)
adj2_fold_quirk = os.environ.get("OCN_ADJ2_FOLD_QUIRK", "0") == "1"


@_on_device
def dense_block_adj2(rowptr: Tensor, col: Tensor, n: int, block_size: int, fold: bool = False):
    """Pattern of A·A by the reference's block loop on the integer matrix cores (ocn_hip.h: ocn_dense_block_mm_bits).
    Returns (rowptrC, colC, bit rows [n, words] int32)."""
    _req(rowptr, torch.int64, "rowptr", 1); _req(col, torch.int32, "col", 1)
    if block_size <= 0 or block_size % 32:
        raise ValueError("block_size must be a positive multiple of 32 for the dense block route")
    l = _lib.lib()
    dev = col.device
    ld = (n + 63) // 64 * 64
    dense = torch.zeros(ld, ld, dtype=torch.int8, device=dev)
    denseT = torch.zeros(ld, ld, dtype=torch.int8, device=dev)
    check(l.ocn_dense_from_csr(ptr(rowptr), ptr(col), n, ld, ptr(dense), ptr(denseT), stream_ptr()), "ocn_dense_from_csr")
    words = (n + 31) // 32
    bits = torch.zeros(n, words, dtype=torch.int32, device=dev)
    for r0 in range(0, n, block_size):                   # the tile loop of utils.py:305-321
        for c0 in range(0, n, block_size):
            check(l.ocn_dense_block_mm_bits(ptr(dense), ptr(denseT), ld, n, r0, min(r0 + block_size, n), c0, min(c0 + block_size, n),
                                            int(fold), ptr(bits), words, stream_ptr()), "ocn_dense_block_mm_bits")
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    check(l.ocn_bitrows_count(ptr(bits), words, n, n, ptr(cnt), stream_ptr()), "ocn_bitrows_count")
    rowptrC = scan_i32(cnt)
    nnz = _total(rowptrC[-1])
    colC = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)[:nnz]
    if nnz:
        check(l.ocn_bitrows_fill(ptr(bits), words, n, n, ptr(rowptrC), ptr(colC), stream_ptr()), "ocn_bitrows_fill")
    return rowptrC, colC, bits


@_on_device
def rows_ln_relu(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, relu: bool, inplace: bool = False) -> Tensor:
    """LayerNorm over the last dim of a [rows, H] fp32 matrix, optionally followed by ReLU."""
    _req(x, torch.float32, "x", 2)
    _req(gamma, torch.float32, "gamma", 1); _req(beta, torch.float32, "beta", 1)
    rows, H = x.shape
    if gamma.numel() != H or beta.numel() != H or H not in LN_WIDTHS:
        raise ValueError("rows_ln_relu: unsupported width")
    y = x if inplace else torch.empty_like(x)
    check(_lib.lib().ocn_rows_ln_relu(ptr(x), ptr(gamma), ptr(beta), float(eps), int(relu), rows, H, ptr(y),
                                      stream_ptr()), "ocn_rows_ln_relu")
    return y


@_on_device
def ln_drop_relu_forward(x: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], eps: float, p: float, seed: int, relu: bool):
    """y = relu?(dropout_p(LN?(x))) in one launch (ocn_hip.h: ocn_ln_drop_relu_forward); returns (y, stats | None)."""
    _req(x, torch.float32, "x", 2)
    rows, H = x.shape
    if H not in LN_WIDTHS:
        raise ValueError("ln_drop_relu: unsupported width")
    if gamma is not None and (_req(gamma, torch.float32, "gamma", 1).numel() != H or _req(beta, torch.float32, "beta", 1).numel() != H):
        raise ValueError("ln_drop_relu: gamma / beta width")
    y = torch.empty_like(x)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device) if gamma is not None else None
    check(_lib.lib().ocn_ln_drop_relu_forward(ptr(x), ptr(gamma), ptr(beta), float(eps), float(p), int(seed), int(relu), rows, H, ptr(y),
                                              ptr(stats), stream_ptr()), "ocn_ln_drop_relu_forward")
    return y, stats


@_on_device
def ln_drop_relu_backward(g: Tensor, x: Tensor, y: Tensor, stats: Optional[Tensor], gamma: Optional[Tensor], p: float, seed: int,
                          relu: bool):
    """(dx, dgamma | None, dbeta | None) of ``ln_drop_relu_forward`` (deterministic: ocn_hip.h)."""
    g = _req(g.contiguous(), torch.float32, "g", 2)
    rows, H = g.shape
    dx = torch.empty_like(g)
    dg = db = ws = None
    if gamma is not None:
        dg, db = torch.empty_like(gamma), torch.empty_like(gamma)
        ws = torch.empty(int(_lib.lib().ocn_ln_drop_relu_workspace_bytes(H)), dtype=torch.uint8, device=g.device)
    check(_lib.lib().ocn_ln_drop_relu_backward(ptr(g), ptr(x), ptr(y), ptr(stats), ptr(gamma), float(p), int(seed), int(relu), rows, H,
                                               ptr(dx), ptr(dg), ptr(db), ptr(ws), stream_ptr()), "ocn_ln_drop_relu_backward")
    return dx, dg, db


@_on_device
def dropout_keep_mask(seed: int, p: float, n: int, device) -> Tensor:
    out = torch.empty(n, dtype=torch.uint8, device=device)
    with torch.cuda.device(out.device):
        check(_lib.lib().ocn_dropout_keep_mask(int(seed), float(p), n, ptr(out), stream_ptr()), "ocn_dropout_keep_mask")
    return out


@_on_device
def combine3(coef: Tensor, x1: Tensor, x2: Tensor, x3: Tensor) -> Tensor:
    """coef[0]*x1 + coef[1]*x2 + coef[2]*x3 with the coefficients read on the device."""
    _req(coef, torch.float32, "coef", 1)
    for t, nm in ((x1, "x1"), (x2, "x2"), (x3, "x3")):
        _req(t, torch.float32, nm)
    if coef.numel() != 3 or x1.shape != x2.shape or x1.shape != x3.shape or x1.numel() % 4:
        raise ValueError("combine3: shape mismatch")
    out = torch.empty_like(x1)
    check(_lib.lib().ocn_combine3(ptr(coef), ptr(x1), ptr(x2), ptr(x3), x1.numel(), ptr(out), stream_ptr()),
          "ocn_combine3")
    return out


@_on_device
def mix3_backward(coef: Tensor, g: Tensor, x1: Tensor, x2: Tensor, x3: Tensor):
    """(d1, d2, d3, dcoef) of z = coef[0] x1 + coef[1] x2 + coef[2] x3 (ocn_hip.h: ocn_mix3_backward)."""
    g = _req(g.contiguous(), torch.float32, "g")
    for t, nm in ((x1, "x1"), (x2, "x2"), (x3, "x3")):
        if _req(t, torch.float32, nm).shape != g.shape:
            raise ValueError("mix3_backward: shape mismatch")
    n = g.numel()
    if n % 4:
        raise ValueError("mix3_backward: n must be a multiple of 4")
    l = _lib.lib()
    d1, d2, d3 = torch.empty_like(g), torch.empty_like(g), torch.empty_like(g)
    dcoef = torch.empty(3, dtype=torch.float32, device=g.device)
    ws = torch.empty(int(l.ocn_mix3_workspace_bytes()), dtype=torch.uint8, device=g.device)
    check(l.ocn_mix3_backward(ptr(coef), ptr(g), ptr(x1), ptr(x2), ptr(x3), n, ptr(d1), ptr(d2), ptr(d3), ptr(dcoef), ptr(ws),
                              stream_ptr()), "ocn_mix3_backward")
    return d1, d2, d3, dcoef


@_on_device
def fill_rows(dst: Tensor, vec: Tensor, row_range: Tensor) -> None:
    """dst[rows of the device-side range] = vec (dst may be a column slice of a wider buffer)."""
    _req_strided(dst, "dst")
    _req(vec, torch.float32, "vec")
    _req(row_range, torch.int64, "row_range", 1)
    if vec.numel() != dst.shape[1]:
        raise ValueError("fill_rows: width mismatch")
    check(_lib.lib().ocn_fill_rows(ptr(dst), dst.stride(0), dst.shape[1], ptr(vec), ptr(row_range), dst.shape[0],
                                   stream_ptr()), "ocn_fill_rows")
    _mark("mlp_glue")


LINEAR_WIDTHS = (32, 64, 128, 256)
fast_linear = True               # route eligible nn.Linear layers of the heads through ocn_linear_bf16x6
_panels: dict = {}


@_on_device
def linear_panel(weight: Tensor) -> Tensor:
    """Pre-split, fragment-ordered bf16 panel of an nn.Linear weight.  Cached per live tensor object
    (weak reference) and rebuilt when the weight is modified in place (``_version``), re-pointed
    (``data_ptr``) or reshaped — a freed weight's address being reused by another module must not
    hit."""
    import weakref
    key = id(weight)
    hit = _panels.get(key)
    if (hit is not None and hit[0]() is weight and hit[1] == weight.data_ptr() and hit[2] == weight._version
            and hit[3] == tuple(weight.shape)):
        return hit[4]
    w = _req(weight.detach(), torch.float32, "weight", 2)
    N, K = w.shape
    panel = torch.empty(int(_lib.lib().ocn_linear_panel_bytes(N, K)), dtype=torch.uint8, device=w.device)
    check(_lib.lib().ocn_linear_split_weight(ptr(w), N, K, ptr(panel), stream_ptr()), "ocn_linear_split_weight")
    if len(_panels) > 512:
        for k in [k for k, v in _panels.items() if v[0]() is None]:
            del _panels[k]
    _panels[key] = (weakref.ref(weight), weight.data_ptr(), weight._version, (N, K), panel)
    return panel


@_on_device
def heads_panel(weight: Tensor):
    """The f16 hi/lo panel of a weight [N, K] for ocn_heads_fused (ocn_hip.h: ocn_heads_split_weight) and the inverse of
    the power of two it was scaled by (max |scale * W| in [2^13, 2^14): f16 has a 5-bit exponent).  Not cached here
    (the heads pack caches it); one host sync for the maximum."""
    import math
    w = _req(weight.detach(), torch.float32, "weight", 2)
    N, K = w.shape
    m = float(w.abs().max().item()) if w.numel() else 0.0
    if not math.isfinite(m):
        raise ValueError("heads_panel: non-finite weight")
    sw = 13 - math.frexp(m)[1] + 1 if m > 0.0 else 0          # frexp: m = f * 2^e, f in [0.5, 1)  ->  floor(log2 m) = e - 1
    sw = max(-100, min(100, sw))
    panel = torch.empty(int(_lib.lib().ocn_heads_panel_bytes(N, K)), dtype=torch.uint8, device=w.device)
    check(_lib.lib().ocn_heads_split_weight(ptr(w), N, K, float(2.0 ** sw), ptr(panel), stream_ptr()), "ocn_heads_split_weight")
    return panel, float(2.0 ** -sw)


HEADS_WIDTHS = (128, 256)
train_linear = True              # autograd on: the heads' Linear layers (forward and input gradient) on the MFMA kernel
train_tails = os.environ.get("OCN_TRAIN_TAILS", "1") != "0"      # ... and their LayerNorm -> Dropout -> ReLU tails as one launch each way (ocn_ln_drop_relu_*)
fused_heads = True               # cn5 / cn7 eval: the whole MLP head as one launch (ocn_heads_fused)
fused_heads_min_width = 128      # narrower heads (ppa / citation2 / ddi: H = 32..64) have a k-loop of 2-4 steps: the fused
                                 # kernel's per-tile epilogues dominate and the grouped launches are faster (ddi: 18 vs 31 us)


def heads_small_batch(max_rows: int = -1) -> int:
    """ocn_hip.h: ocn_heads_small_batch — batches up to ``max_rows`` candidates take the latency form of the fused head (same
    bits); returns the previous bound, a negative argument only queries."""
    return int(_lib.lib().ocn_heads_small_batch(int(max_rows)))


def flags_pair_min_batch(min_rows: int = -1) -> int:
    """ocn_hip.h: ocn_cn_flags_pair_min_batch — on larger graphs, batches of at least ``min_rows`` candidates run the
    intersection pass with two slots per wave (same bits); returns the previous bound, a negative argument only queries."""
    return int(_lib.lib().ocn_cn_flags_pair_min_batch(int(min_rows)))


def gather_pair_min_batch(min_rows: int = -1) -> int:
    """ocn_hip.h: ocn_cn_gather_pair_min_batch — record-fed H = 256 batches of at least ``min_rows`` candidates are pooled with
    two slots per wave (same bits); returns the previous bound, a negative argument only queries."""
    return int(_lib.lib().ocn_cn_gather_pair_min_batch(int(min_rows)))


@_on_device
def heads_fused(x1: Tensor, x2: Tensor, xij: Tensor, pack: dict, ranges: Optional[Tensor], y_row_map: Optional[Tensor],
                b_on_union: bool, scratch: Tensor, dump: Optional[Tensor] = None) -> Optional[Tensor]:
    """ocn_hip.h: ocn_heads_fused.  ``pack``: panels / vectors prepared by ``model._CNPredictorBase._fused_pack``.
    Returns the [B, 1] scores (or None in constants mode, where ``dump`` receives what a skipped branch contributes;
    scoring mode reads it back as ``pack["cpark"]``)."""
    for t, nm in ((x1, "xcn1"), (x2, "xcn2"), (xij, "xij")):
        _req(t, torch.float32, nm, 2)
    B, H = xij.shape
    if x1.shape != (B, H) or x2.shape != (B, H) or H not in HEADS_WIDTHS:
        raise ValueError("heads_fused: shape mismatch")
    a = _lib.OcnHeadsArgs()
    a.x[0], a.x[1], a.x[2] = x1.data_ptr(), x2.data_ptr(), xij.data_ptr()
    a.ldx, a.B, a.H = H, B, H
    for i in range(3):
        a.p_first[i] = pack["first"][i].data_ptr()
        a.p_out[i] = pack["out"][i].data_ptr()
    a.p_mid[0], a.p_mid[1] = pack["mid"][0].data_ptr(), pack["mid"][1].data_ptr()
    a.vec = pack["vec"].data_ptr()
    a.ranges = 0 if ranges is None else _req(ranges, torch.int64, "ranges").data_ptr()
    a.y_row_map = 0 if y_row_map is None else _req(y_row_map, torch.int64, "y_row_map", 1).data_ptr()
    y = None
    nconst = int(_lib.lib().ocn_heads_const_bytes(H)) // 4
    if dump is None:
        y = torch.empty((B, 1), dtype=torch.float32, device=xij.device)
        a.y = y.data_ptr()
        if _req(pack["cpark"], torch.float32, "cpark", 1).numel() != nconst:
            raise ValueError("heads_fused: constants buffer of the wrong size")
        a.cpark = pack["cpark"].data_ptr()
    else:
        if B != 1 or _req(dump, torch.float32, "dump", 1).numel() != nconst:
            raise ValueError("heads_fused: constants mode takes one row and ocn_heads_const_bytes(H) bytes")
        a.dump = dump.data_ptr()
    if scratch.numel() * scratch.element_size() < int(_lib.lib().ocn_heads_scratch_bytes(H)):
        raise ValueError("heads_fused: scratch too small")
    a.scratch = scratch.data_ptr()
    a.eps, a.ln, a.b_on_union = float(pack["eps"]), int(pack["ln"]), int(bool(b_on_union))
    _mark("mlp_glue")
    check(_lib.lib().ocn_heads_fused(ctypes.byref(a), stream_ptr()), "ocn_heads_fused")
    _mark("linear", pack["flops_per_row"] * B)
    return y


def linear_ok(x: Tensor, weight: Tensor) -> bool:
    return (fast_linear and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous()
            and weight.shape[0] in LINEAR_WIDTHS and weight.shape[1] % 16 == 0 and weight.shape[1] == x.shape[1])


@_on_device
def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, ln=None, relu: bool = False,
           dot=None, y_row_map: Optional[Tensor] = None) -> Tensor:
    """epilogue(x @ weight.T + bias): optional LayerNorm ``ln=(gamma, beta, eps)``, ReLU, and a
    trailing Linear(N -> 1) ``dot=(w[1,N], b[1] | None)`` (then the result is [M, 1]; with
    ``y_row_map`` row r of x lands in row y_row_map[r] of it)."""
    _req(x, torch.float32, "x", 2)
    M, K = x.shape
    N = weight.shape[0]
    if y_row_map is not None:
        if dot is None:
            raise ValueError("y_row_map needs the dot epilogue")
        y = torch.empty((M, 1), dtype=torch.float32, device=x.device)
        linear_grouped([dict(x=x, weight=weight, bias=bias, ln=ln, relu=relu, dot=(dot[0].reshape(1, -1), dot[1]), y=y,
                             y_row_map=y_row_map)], K, N)
        return y
    panel = linear_panel(weight)
    _mark("mlp_glue")
    y = torch.empty((M, 1) if dot is not None else (M, N), dtype=torch.float32, device=x.device)
    g = b = None
    eps = 0.0
    if ln is not None:
        g, b, eps = ln
    dw = db = None
    if dot is not None:
        dw, db = dot
        dw = dw.reshape(-1)
    check(_lib.lib().ocn_linear_bf16x6(ptr(x), M, K, ptr(panel), N, ptr(bias), ptr(g), ptr(b), float(eps),
                                       int(relu), ptr(dw), ptr(db), ptr(y), stream_ptr()), "ocn_linear_bf16x6")
    _mark("linear", 2.0 * M * K * N)
    return y


def linear_ok_t(gy: Tensor, weight: Tensor) -> bool:
    """``linear_t`` takes these shapes (the product gy @ weight as a Linear whose weight is weight^T)."""
    return (fast_linear and gy.is_cuda and gy.dim() == 2 and gy.dtype == torch.float32
            and weight.shape[1] in LINEAR_WIDTHS and weight.shape[0] % 16 == 0 and weight.shape[0] == gy.shape[1])


@_on_device
def linear_t(gy: Tensor, weight: Tensor) -> Tensor:
    """gy @ weight ([M, N] x [N, K] -> [M, K]) on the bf16x6 MFMA kernel: the input gradient of y = x @ weight^T.
    The transposed panel is built per call (the weight changes with every optimiser step)."""
    gy = _req(gy.contiguous(), torch.float32, "gy", 2)
    wt = _req(weight.detach().t().contiguous(), torch.float32, "weight^T", 2)          # [K, N]: K outputs, N inputs
    K, N = wt.shape
    M = gy.shape[0]
    panel = torch.empty(int(_lib.lib().ocn_linear_panel_bytes(K, N)), dtype=torch.uint8, device=wt.device)
    check(_lib.lib().ocn_linear_split_weight(ptr(wt), K, N, ptr(panel), stream_ptr()), "ocn_linear_split_weight")
    y = torch.empty((M, K), dtype=torch.float32, device=gy.device)
    check(_lib.lib().ocn_linear_bf16x6(ptr(gy), M, N, ptr(panel), K, None, None, None, 0.0, 0, None, None, ptr(y),
                                       stream_ptr()), "ocn_linear_bf16x6")
    return y


@_on_device
def wgrad(gy: Tensor, x: Tensor, with_bias: bool = True):
    """Weight / bias gradient of ``y = x @ W^T + b``: ``(gy^T @ x, gy.sum(0))`` — ``ocn_wgrad`` (bf16x6 on the matrix
    cores, split over the batch, partial results added in slice order: deterministic).  gy [B, N], x [B, K] fp32 with
    unit column stride (row strides free)."""
    if gy.dim() == 2 and gy.stride(1) != 1:
        gy = gy.contiguous()
    if x.dim() == 2 and x.stride(1) != 1:
        x = x.contiguous()
    _req_strided(gy, "gy")
    _req_strided(x, "x")
    B, N = gy.shape
    K = x.shape[1]
    if x.shape[0] != B:
        raise ValueError(f"wgrad: {tuple(gy.shape)} against {tuple(x.shape)}")
    l = _lib.lib()
    ws = torch.empty(int(l.ocn_wgrad_workspace_bytes(B, N, K)), dtype=torch.uint8, device=gy.device)
    gw = torch.empty((N, K), dtype=torch.float32, device=gy.device)
    gb = torch.empty((N,), dtype=torch.float32, device=gy.device) if with_bias else None
    ldy = gy.stride(0) if B > 1 else max(N, gy.stride(0))
    ldx = x.stride(0) if B > 1 else max(K, x.stride(0))
    check(l.ocn_wgrad(ptr(gy), ldy, ptr(x), ldx, B, N, K, ptr(gw), ptr(gb) if with_bias else None, ptr(ws), stream_ptr()),
          "ocn_wgrad")
    return gw, gb


@_on_device
def coo_to_csr(row: Tensor, col: Tensor, n_rows: int, n_cols: int, symmetrize: bool = False, dedupe: bool = False,
               check_range: bool = True):
    """(rowptr int64[n_rows + 1], col int32[nnz']) of the pattern with entries (row[q], col[q]) — plus the transposed
    entries when ``symmetrize`` — columns ascending per row, duplicates removed when ``dedupe`` (``ocn_coo_to_csr``:
    counting pass, chained scan, fill, per-row sorts; no sort over the edge list).  ONE device -> host read (entries
    written and the range status)."""
    row = _req(row.contiguous(), torch.int64, "row", 1)
    col = _req(col.contiguous(), torch.int64, "col", 1)
    nnz = row.numel()
    if col.numel() != nnz:
        raise ValueError("coo_to_csr: row and col differ in length")
    l = _lib.lib()
    dev = row.device
    ws = torch.empty(int(l.ocn_coo_to_csr_workspace_bytes(nnz, n_rows, int(symmetrize), int(dedupe))), dtype=torch.uint8, device=dev)
    rowptr = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
    out = torch.empty(nnz * (2 if symmetrize else 1), dtype=torch.int32, device=dev)
    res = torch.empty(2, dtype=torch.int64, device=dev)
    check(l.ocn_coo_to_csr(ptr(row), ptr(col), nnz, n_rows, n_cols, int(symmetrize), int(dedupe), ptr(rowptr), ptr(out),
                           ptr(ws), ptr(res), stream_ptr()), "ocn_coo_to_csr")
    n_out, bad = (int(v) for v in res.tolist())
    if bad:          # (the status is on the host anyway: out-of-range entries are never dropped silently; `check_range` kept for callers)
        raise IndexError("SparseTensor: index out of range for sparse_sizes")
    if n_out < 0:
        raise _lib.OcnHipError("ocn_coo_to_csr: scan state was not zero")
    return rowptr, out[:n_out]


def linear_grouped(groups, K: int, N: int) -> None:
    """Up to five Linear layers of the same (K, N) in one launch.  Each group is a dict:
    x [M, >=K] (row stride may exceed K), weight [N, K], y (preallocated, row stride >= N, or [M, 1] with
    ``dot``), optional bias, ln=(gamma, beta, eps), relu, scale (device float[1]), addend [M, >=N] (or one
    row [1, N] with ``add_bcast``), dot=(w[1, N], b[1]), row_range (device int64[2]: only rows
    [begin, end) of the buffers), y_row_map (device int64[M]: destination row of the dot output).
    ``dot`` with an addend and ``y_row_map`` without ``dot`` are refused, as ocn_linear_grouped refuses them."""
    if not 1 <= len(groups) <= 5:
        raise ValueError("1..5 groups")
    idx = groups[0]["x"].device.index
    if idx is not None and idx != torch._C._cuda_getDevice():
        with torch.cuda.device(idx):
            return linear_grouped(groups, K, N)
    arr = (_lib.OcnLinearGroup * len(groups))()
    keep = []
    for a, g in zip(arr, groups):
        x, w, y = g["x"], g["weight"], g["y"]
        _req_strided(x, "x"); _req_strided(y, "y")
        if x.shape[1] != K or tuple(w.shape) != (N, K) or x.shape[0] != y.shape[0]:
            raise ValueError("linear_grouped: shape mismatch")
        ln = g.get("ln")
        dot = g.get("dot")
        add = g.get("addend")
        if add is not None and dot is not None:
            raise ValueError("linear_grouped: the dot epilogue takes no addend")
        if g.get("y_row_map") is not None and dot is None:
            raise ValueError("linear_grouped: y_row_map needs the dot epilogue")
        if add is not None:
            _req_strided(add, "addend")
            if g.get("add_bcast") and add.shape != (1, N):
                raise ValueError("add_bcast: addend must be [1, N]")
        panel = linear_panel(w)
        keep.append(panel)
        a.X, a.ldX, a.M, a.Wp = x.data_ptr(), x.stride(0), x.shape[0], panel.data_ptr()
        a.bias = 0 if g.get("bias") is None else g["bias"].data_ptr()
        a.gamma, a.beta, a.eps = (0, 0, 0.0) if ln is None else (ln[0].data_ptr(), ln[1].data_ptr(), float(ln[2]))
        a.relu = int(bool(g.get("relu")))
        a.scale = 0 if g.get("scale") is None else g["scale"].data_ptr()
        if add is not None:
            a.addend, a.ldAdd = add.data_ptr(), add.stride(0)
            a.add_bcast = int(bool(g.get("add_bcast")))
        rr, rm = g.get("row_range"), g.get("y_row_map")
        if rr is not None:
            _req(rr, torch.int64, "row_range", 1)
            a.row_range = rr.data_ptr()
        if rm is not None:
            _req(rm, torch.int64, "y_row_map", 1)
            a.y_row_map = rm.data_ptr()
        if dot is not None:
            a.dotw = dot[0].data_ptr()
            a.dotb = 0 if dot[1] is None else dot[1].data_ptr()
            a.ldY = 1
        else:
            a.ldY = y.stride(0)
        a.Y = y.data_ptr()
    _mark("mlp_glue")
    check(_lib.lib().ocn_linear_grouped(ctypes.cast(arr, ctypes.c_void_p), len(groups), K, N, stream_ptr()),
          "ocn_linear_grouped")
    _mark("linear", sum(2.0 * g["x"].shape[0] * K * N for g in groups))


def _req_strided(t: Tensor, name: str) -> None:
    """2-d fp32 device tensor whose rows are contiguous (row stride may exceed the width)."""
    if not (isinstance(t, Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1):
        raise ValueError(f"{name}: expected a 2-d fp32 device tensor with contiguous rows")
