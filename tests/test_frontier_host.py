"""Frontier expansion and 3-hop recommendation (``ocn_frontier_count`` / ``ocn_frontier_sums_fill``, ``hops=3`` in
ocn_amd/recommend.py) without a GPU: the entries' declarations and argument checks, and the refusals of the Python layers —
every one of them before the device."""
import math
import os
import re
from ctypes import c_void_p

import pytest
import torch

from ocn_amd import _lib

P = c_void_p(4096)             # a non-NULL address that is never read: every call below returns before its first HIP call
Z = c_void_p(0)
NAMES = ("ocn_frontier_window_cols", "ocn_frontier_count", "ocn_frontier_sums_fill")


def test_frontier_entries_are_additions_to_abi_9(hiplib):
    header = open(os.path.join(_lib.INCLUDE, "ocn_hip.h")).read()
    later = header[header.index("Later additions to 9"):header.index("#define OCN_ABI_VERSION")]
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(hiplib, name)
        assert re.search(r"\b" + name + r"\s*\(", header), name              # declared ...
        assert name in later, name                                             # ... and listed among the additions to 9
    assert "#define OCN_ABI_VERSION 9" in header
    assert hiplib.ocn_abi_version() == _lib.ABI_VERSION == 9
    window = hiplib.ocn_frontier_window_cols()
    assert window >= 64 and window % 64 == 0
    lds = 160 * 1024 - 2048 - 4 * 256 * 4                                      # without the four waves' claim tables
    assert window * 33 // 8 <= lds < (window + 64) * 33 // 8                   # a bit and an fp32 per column
    assert os.path.exists(os.path.join(_lib.CSRC, "frontier.hip"))


def _count(lib, **kw):
    a = dict(rpA=P, cA=P, rpM=P, cM=P, n=100, rows=P, Q=4, drop=1, window=0, pF=P, nF=P, pS=P, nS=P, count=P)
    a.update(kw)
    return lib.ocn_frontier_count(a["rpA"], a["cA"], a["rpM"], a["cM"], a["n"], a["rows"], a["Q"], a["drop"], a["window"],
                                  a["pF"], a["nF"], a["pS"], a["nS"], a["count"], Z)


def _fill(lib, **kw):
    a = dict(rpA=P, cA=P, rpM=P, cM=P, n=100, rows=P, Q=4, drop=1, window=0, pF=P, nF=P, vF=P, pS=P, nS=P, vS=P, off=P, edges=P,
             val=P)
    a.update(kw)
    return lib.ocn_frontier_sums_fill(a["rpA"], a["cA"], a["rpM"], a["cM"], a["n"], a["rows"], a["Q"], a["drop"], a["window"],
                                      a["pF"], a["nF"], a["vF"], a["pS"], a["nS"], a["vS"], a["off"], a["edges"], a["val"], Z)


def test_frontier_entries_reject_bad_arguments_before_any_hip_call(hiplib):
    # every call is empty (Q == 0) or wrong: none reaches a HIP call, so none needs a GPU
    for call, needed in ((_count, ("rpA", "cA", "rpM", "cM", "rows", "pF", "nF", "count")),
                         (_fill, ("rpA", "cA", "rpM", "cM", "rows", "pF", "nF", "off", "edges"))):
        for name in needed:
            assert call(hiplib, **{name: Z}) == -1, name
            assert call(hiplib, Q=0, **{name: Z}) == -1, name
        assert call(hiplib, Q=-1) == -1
        for n in (0, -5, 1 << 31, 1 << 40):
            assert call(hiplib, n=n) == -1 and call(hiplib, Q=0, n=n) == -1, n
        window = hiplib.ocn_frontier_window_cols()
        for w in (-64, -1, 1, 63, 65, 100, window - 1, window + 64, 2 * window, hiplib.ocn_two_hop_sums_window_cols()):
            assert call(hiplib, window=w) == -1 and call(hiplib, Q=0, window=w) == -1, w
        assert call(hiplib, pS=Z) == -1 and call(hiplib, nS=Z) == -1 and call(hiplib, Q=0, pS=Z) == -1      # half a seed list
        # a valid empty call launches nothing
        assert call(hiplib, Q=0) == 0 and call(hiplib, Q=0, n=(1 << 31) - 1) == 0
        assert call(hiplib, Q=0, window=64) == 0 and call(hiplib, Q=0, window=window) == 0
        assert call(hiplib, Q=0, pS=Z, nS=Z) == 0                              # no seeds
    assert _fill(hiplib, vS=Z) == -1 and _fill(hiplib, Q=0, vS=Z) == -1        # seeds without values where val is written
    assert _fill(hiplib, Q=0, vS=Z, val=Z) == 0 and _fill(hiplib, Q=0, vS=Z, pS=Z, nS=Z) == 0
    assert _fill(hiplib, Q=0, vF=Z) == 0 and _fill(hiplib, Q=0, val=Z, vF=Z) == 0     # unit weights; the pairs alone


def _req_anywhere(t, dtype, name, ndim=None):
    """``ops._req`` without its device check, so that the checks behind it can be reached on the CPU."""
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name}: expected {ndim}-d, got shape {tuple(t.shape)}")
    return t


class _NoFrontier:
    """The library with the frontier launches taken out: a wrapper that reached one would fail the test, not touch a device."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name in NAMES[1:]:
            raise AssertionError("the wrapper reached the library")
        return getattr(self._real, name)


def test_frontier_wrappers_check_operands_before_the_library(hiplib, monkeypatch):
    from ocn_amd import ops
    rp3, rp2, col = torch.tensor([0, 1, 2, 2]), torch.tensor([0, 1, 2]), torch.tensor([1, 0], dtype=torch.int32)
    rows, off = torch.tensor([0, 1]), torch.tensor([0, 1, 2])
    pF, nF, vF = torch.tensor([0, 1, 2]), torch.tensor([[0, 1], [1, 0]]), torch.tensor([1.0, 2.0])
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.frontier_count(rp3, col, rp3, col, rows, pF, nF)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.frontier_sums_fill(rp3, col, rp3, col, rows, pF, nF, vF, None, None, None, off)
    monkeypatch.setattr(ops, "_req", _req_anywhere)
    monkeypatch.setattr(ops, "validate_indices", False)
    monkeypatch.setattr(_lib, "lib", lambda real=_lib.lib: _NoFrontier(real()))
    W = ops.frontier_window_cols()

    def both(match, exc=ValueError, **kw):
        a = dict(rpA=rp3, cA=col, rpM=rp3, cM=col, rows=rows, pF=pF, nF=nF, vF=vF, pS=None, nS=None, vS=None, off=off, window=0)
        a.update(kw)
        with pytest.raises(exc, match=match):
            ops.frontier_count(a["rpA"], a["cA"], a["rpM"], a["cM"], a["rows"], a["pF"], a["nF"], a["pS"], a["nS"], window_cols=a["window"])
        with pytest.raises(exc, match=match):
            ops.frontier_sums_fill(a["rpA"], a["cA"], a["rpM"], a["cM"], a["rows"], a["pF"], a["nF"], a["vF"], a["pS"], a["nS"], a["vS"],
                                   a["off"], total=2, window_cols=a["window"])

    both("P has 3 rows, M 2", rpM=rp2)
    for bad in (-64, 32, 100, W + 64, ops.two_hop_window_cols()):
        both(f"multiple of 64 up to {W}", window=bad)
    both("ptrF: one entry per query and the total", pF=torch.tensor([0, 2]))
    both(r"nodeF: expected the \[T, 2\] pair layout", nF=torch.zeros(2, 3, dtype=torch.int64))
    both("nodeF: expected 2-d", nF=torch.tensor([1, 0]))
    both("nodeF: expected torch.int64", TypeError, nF=nF.int())
    both("ptrF: expected torch.int64", TypeError, pF=pF.int())
    both("rows: expected torch.int64", TypeError, rows=rows.int())
    both("colP: expected torch.int32", TypeError, cA=col.long())
    both("given together or not at all", pS=pF)
    both("given together or not at all", nS=nF)
    both("ptrS: one entry per query and the total", pS=torch.tensor([0, 2]), nS=nF, vS=vF)
    with pytest.raises(ValueError, match="valF: expected one value per pair"):
        ops.frontier_sums_fill(rp3, col, rp3, col, rows, pF, nF, torch.zeros(3), None, None, None, off, total=2)
    with pytest.raises(TypeError, match="valF: expected torch.float32"):
        ops.frontier_sums_fill(rp3, col, rp3, col, rows, pF, nF, vF.double(), None, None, None, off, total=2)
    with pytest.raises(ValueError, match="valS: seeds need their values"):
        ops.frontier_sums_fill(rp3, col, rp3, col, rows, pF, nF, vF, pF, nF, None, off, total=2)
    with pytest.raises(ValueError, match="off: one entry per query and the total"):
        ops.frontier_sums_fill(rp3, col, rp3, col, rows, pF, nF, vF, None, None, None, torch.tensor([0, 1]), total=1)


def _tiny():
    from ocn_amd.sparse import SparseTensor
    return SparseTensor.from_edge_index(torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), sparse_sizes=(4, 4))


def test_three_hop_arguments_are_refused_before_the_device(hiplib):
    from ocn_amd import ops, recommend as R
    from ocn_amd.model import predictor_dict
    adj = _tiny()                                                           # on the CPU: reaching a device operand raises OcnHipError
    src = torch.tensor([0, 2])
    pred = predictor_dict["cn5"](8, 8, 1, 3, 0.0).eval()
    h = torch.randn(4, 8)
    top = ops.segment_topk_max_k()
    assert ops.prefilter_budget == 1 << 26
    for hops in (1, 4, 0, -3, 2.5, "3", None, True):
        with pytest.raises(ValueError, match="hops must be 2 or 3"):
            R.recommend_links(pred, h, adj, None, src, 3, 64, hops=hops)
        with pytest.raises(ValueError, match="hops must be 2 or 3"):
            R.recommend_links_heuristic(adj, None, src, 3, 64, "ra", hops=hops)
        with pytest.raises(ValueError, match="hops must be 2 or 3"):
            R.path_scored_candidates(adj, src, "cn", hops, 0.5)
        with pytest.raises(ValueError, match="hops must be 2 or 3"):
            R.prefilter_candidates(adj, src, "cn", 5, hops=hops, decay=0.5)
    for adj2 in (None, adj):
        # the arity goes with the hops
        for bad in (("ra", 10), ["cn", 5], ("ra", 10, 0.5, 1), "ra", 10):
            with pytest.raises(ValueError, match=r"prefilter must be None or \(kind, m, decay\)"):
                R.recommend_links(pred, h, adj, adj2, src, 3, 64, prefilter=bad, hops=3)
        for bad in (("ra", 10, 0.5), ("ra", 10, 0)):
            with pytest.raises(ValueError, match=r"prefilter must be None or \(kind, m\)"):
                R.recommend_links(pred, h, adj, adj2, src, 3, 64, prefilter=bad)
            with pytest.raises(ValueError, match=r"prefilter must be None or \(kind, m\)"):
                R.recommend_links(pred, h, adj, adj2, src, 3, 64, prefilter=bad, hops=2)
        for decay in (-0.5, -1, math.nan, math.inf, -math.inf, "0.5", None, True):
            with pytest.raises(ValueError, match="decay must be a finite number >= 0"):
                R.recommend_links(pred, h, adj, adj2, src, 3, 64, prefilter=("ra", 10, decay), hops=3)
        with pytest.raises(ValueError, match="fewer than k = 6"):
            R.recommend_links(pred, h, adj, adj2, src, 6, 64, prefilter=("ra", 5, 0.5), hops=3)
        with pytest.raises(ValueError, match=f"m must be in 1..{top}"):
            R.recommend_links(pred, h, adj, adj2, src, 3, 64, prefilter=("ra", top + 1, 0.5), hops=3)
        with pytest.raises(ValueError, match=f"m must be in 1..{top}"):
            R.recommend_links(pred, h, adj, adj2, src, 1, 64, prefilter=("cn", 0, 0.5), hops=3)
        with pytest.raises(ValueError, match=r"no path sum.*'cn', 'aa', 'ra'"):
            R.recommend_links(pred, h, adj, adj2, src, 3, 64, prefilter=("jaccard", 10, 0.5), hops=3)
        with pytest.raises(ValueError, match=f"k must be in 1..{top}"):
            R.recommend_links(pred, h, adj, adj2, src, top + 1, 64, hops=3)
    for decay in (-0.5, math.nan, math.inf, None, "1"):
        with pytest.raises(ValueError, match="decay must be a finite number >= 0"):
            R.path_scored_candidates(adj, src, "cn", 3, decay)
        with pytest.raises(ValueError, match="decay must be a finite number >= 0"):
            R.path_scored_candidates(adj, src, "cn", 2, decay)
        with pytest.raises(ValueError, match="decay must be a finite number >= 0"):
            R.prefilter_candidates(adj, src, "ra", 5, hops=3, decay=decay)
    with pytest.raises(TypeError):
        R.path_scored_candidates(adj, src, "cn", 3)                          # decay has no default
    with pytest.raises(ValueError, match="decay and budget belong to hops=3"):
        R.prefilter_candidates(adj, src, "ra", 5, decay=0.5)
    with pytest.raises(ValueError, match="decay and budget belong to hops=3"):
        R.prefilter_candidates(adj, src, "ra", 5, budget=100)
    for budget in (0, -1):
        with pytest.raises(ValueError, match="budget must be a positive number"):
            R.prefilter_candidates(adj, src, "ra", 5, hops=3, decay=0.5, budget=budget)
    with pytest.raises(ValueError, match="no path sum"):
        R.path_scored_candidates(adj, src, "pa", 3, 0.5)
    with pytest.raises(ValueError, match="m must be in 1"):
        R.prefilter_candidates(adj, src, "ra", top + 1, hops=3, decay=0.5)
    with pytest.raises(ValueError, match="sources must be a 1-d int64"):
        R.three_hop_candidates(adj, src.int())
    with pytest.raises(ValueError, match="sources must be a 1-d int64"):
        R.path_scored_candidates(adj, src[None], "cn", 3, 0.5)
    other = type(adj).from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(5, 5))
    with pytest.raises(ValueError, match="known is"):
        R.three_hop_candidates(adj, src, known=other)
    with pytest.raises(RuntimeError, match="eval path"):
        R.recommend_links(pred.train(), h, adj, None, src, 3, 64, hops=3)
    pred.eval()
    cn6 = predictor_dict["cn6"](8, 8, 1, 3, 0.0).eval()
    with pytest.raises(ValueError, match="cn6 needs adj2"):
        R.recommend_links(cn6, h, adj, None, src, 3, 64, prefilter=("ra", 5, 0.5), hops=3)
    # valid arguments get as far as the first device operand: there is no CPU path
    for call in (lambda: R.three_hop_candidates(adj, src),
                 lambda: R.path_scored_candidates(adj, src, "ra", 3, 0.5),
                 lambda: R.path_scored_candidates(adj, src, "cn", 3, 0),
                 lambda: R.path_scored_candidates(adj, src, "cn", 2, 0.5),
                 lambda: R.prefilter_candidates(adj, src, "ra", 5, hops=3, decay=0.5, budget=1000),
                 lambda: R.recommend_links(pred, h, adj, None, src, 3, 64, hops=3),
                 lambda: R.recommend_links(pred, h, adj, adj, src, 3, 64, prefilter=("ra", 3, 0.5), hops=3),
                 lambda: R.recommend_links(pred, h, adj, None, src, 3, 64, prefilter=["cn", top, 1], hops=3),
                 lambda: R.recommend_links_heuristic(adj, None, src, 3, 64, "ra", hops=3)):
        with pytest.raises(_lib.OcnHipError, match="no CPU path"):
            call()


def test_budget_chunks_are_consecutive_and_within_the_budget():
    from ocn_amd.recommend import _budget_chunks
    count = torch.tensor([3, 4, 0, 5, 20, 1, 1, 9, 0], dtype=torch.int32)
    chunks = list(_budget_chunks(count, 10))
    assert chunks == [(0, 3, 7), (3, 4, 5), (4, 5, 20), (5, 7, 2), (7, 9, 9)]          # (20 alone: a source above the budget)
    assert [a for a, _, _ in chunks[1:]] == [b for _, b, _ in chunks[:-1]] and chunks[0][0] == 0 and chunks[-1][1] == 9
    assert all(t <= 10 or b - a == 1 for a, b, t in chunks) and sum(t for _, _, t in chunks) == int(count.sum())
    assert list(_budget_chunks(count, 1000)) == [(0, 9, 43)]
    assert list(_budget_chunks(count[:0], 10)) == []
    assert list(_budget_chunks(torch.tensor([50]), 10)) == [(0, 1, 50)]
