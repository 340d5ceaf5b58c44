"""Two-stage link recommendation (``ocn_two_hop_sums_fill``, ``recommend_links(prefilter=...)`` in ocn_amd/recommend.py)
without a GPU: the entry's declaration and argument checks, and the refusals of the Python layers."""
import os
import re
from ctypes import c_void_p

import pytest
import torch

from ocn_amd import _lib

P = c_void_p(4096)             # a non-NULL address that is never read: every call below returns before its first HIP call
Z = c_void_p(0)


def test_two_hop_sums_entries_are_additions_to_abi_9(hiplib):
    header = open(os.path.join(_lib.INCLUDE, "ocn_hip.h")).read()
    later = header[header.index("Later additions to 9"):header.index("#define OCN_ABI_VERSION")]
    for name in ("ocn_two_hop_sums_window_cols", "ocn_two_hop_sums_fill"):
        assert name in _lib.SIGNATURES and hasattr(hiplib, name)
        assert re.search(r"\b" + name + r"\s*\(", header), name              # declared ...
        assert name in later, name                                             # ... and listed among the additions to 9
    assert "#define OCN_ABI_VERSION 9" in header
    assert hiplib.ocn_abi_version() == _lib.ABI_VERSION == 9
    window = hiplib.ocn_two_hop_sums_window_cols()
    assert window >= 64 and window % 64 == 0
    assert window * 33 // 8 <= 160 * 1024 - 2048 < (window + 64) * 33 // 8   # a bit and an fp32 per column in the bitmap kernel's LDS
    assert window < hiplib.ocn_two_hop_window_cols()


def _sums(lib, **kw):
    a = dict(rpA=P, cA=P, rpM=P, cM=P, n=100, rows=P, Q=4, drop=1, window=0, w=P, wcol=0, off=P, edges=P, val=P)
    a.update(kw)
    return lib.ocn_two_hop_sums_fill(a["rpA"], a["cA"], a["rpM"], a["cM"], a["n"], a["rows"], a["Q"], a["drop"], a["window"],
                                     a["w"], a["wcol"], a["off"], a["edges"], a["val"], Z)


def test_two_hop_sums_fill_rejects_bad_arguments_before_any_hip_call(hiplib):
    # every call is empty (Q == 0) or wrong: none reaches a HIP call, so none needs a GPU
    for name in ("rpA", "cA", "rpM", "cM", "rows", "off", "edges", "val"):
        assert _sums(hiplib, **{name: Z}) == -1, name
        assert _sums(hiplib, Q=0, **{name: Z}) == -1, name
    assert _sums(hiplib, Q=-1) == -1
    for n in (0, -5, 1 << 31, 1 << 40):
        assert _sums(hiplib, n=n) == -1 and _sums(hiplib, Q=0, n=n) == -1, n
    window = hiplib.ocn_two_hop_sums_window_cols()
    for w in (-64, -1, 1, 63, 65, 100, window - 1, window + 64, 2 * window, hiplib.ocn_two_hop_window_cols()):
        assert _sums(hiplib, window=w) == -1 and _sums(hiplib, Q=0, window=w) == -1, w
    for wcol in (-1, 4, 100):
        assert _sums(hiplib, wcol=wcol) == -1 and _sums(hiplib, Q=0, wcol=wcol) == -1, wcol
    # a valid empty call launches nothing
    assert _sums(hiplib, Q=0) == 0 and _sums(hiplib, Q=0, n=(1 << 31) - 1) == 0
    assert _sums(hiplib, Q=0, window=64) == 0 and _sums(hiplib, Q=0, window=window) == 0
    for wcol in (0, 1, 2, 3):
        assert _sums(hiplib, Q=0, wcol=wcol) == 0
    for wcol in (-1, 0, 4, 1 << 20):                                        # without a table the column is ignored
        assert _sums(hiplib, Q=0, w=Z, wcol=wcol) == 0, wcol


def _req_anywhere(t, dtype, name, ndim=None):
    """``ops._req`` without its device check, so that the checks behind it can be reached on the CPU."""
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name}: expected {ndim}-d, got shape {tuple(t.shape)}")
    return t


def test_two_hop_sums_wrapper_checks_operands_before_the_library(hiplib, monkeypatch):
    from ocn_amd import ops
    rp3, rp2, col = torch.tensor([0, 1, 2, 2]), torch.tensor([0, 1, 2]), torch.tensor([1, 0], dtype=torch.int32)
    rows, off = torch.tensor([0, 1]), torch.tensor([0, 1, 2])
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.two_hop_sums_fill(rp3, col, rp3, col, rows, off)
    monkeypatch.setattr(ops, "_req", _req_anywhere)
    monkeypatch.setattr(ops, "validate_indices", False)
    monkeypatch.setattr(_lib, "lib", lambda real=_lib.lib: _NoFill(real()))
    w = torch.zeros(3, 4)
    with pytest.raises(ValueError, match="P has 3 rows, M 2"):
        ops.two_hop_sums_fill(rp3, col, rp2, col, rows, off)
    with pytest.raises(ValueError, match="off: one entry per query and the total"):
        ops.two_hop_sums_fill(rp3, col, rp3, col, rows, torch.tensor([0, 1]), total=1)
    for bad in (-64, 32, 100, ops.two_hop_sums_window_cols() + 64, ops.two_hop_window_cols()):
        with pytest.raises(ValueError, match=f"multiple of 64 up to {ops.two_hop_sums_window_cols()}"):
            ops.two_hop_sums_fill(rp3, col, rp3, col, rows, off, window_cols=bad, total=2)
    for bad in (torch.zeros(3, 3), torch.zeros(4, 4), torch.zeros(2, 4)):
        with pytest.raises(ValueError, match=r"w: expected the \[3, 4\] node table"):
            ops.two_hop_sums_fill(rp3, col, rp3, col, rows, off, bad, total=2)
    with pytest.raises(ValueError, match="w: expected 2-d"):
        ops.two_hop_sums_fill(rp3, col, rp3, col, rows, off, torch.zeros(12), total=2)
    with pytest.raises(TypeError, match="w: expected torch.float32"):
        ops.two_hop_sums_fill(rp3, col, rp3, col, rows, off, w.double(), total=2)
    with pytest.raises(TypeError, match="colP: expected torch.int32"):
        ops.two_hop_sums_fill(rp3, col.long(), rp3, col, rows, off, w, total=2)
    with pytest.raises(TypeError, match="rows: expected torch.int64"):
        ops.two_hop_sums_fill(rp3, col, rp3, col, rows.int(), off, w, total=2)
    with pytest.raises(TypeError, match="off: expected torch.int64"):
        ops.two_hop_sums_fill(rp3, col, rp3, col, rows, off.int(), w, total=2)
    for bad in (-1, 4):
        with pytest.raises(ValueError, match="wcol must be a column 0..3"):
            ops.two_hop_sums_fill(rp3, col, rp3, col, rows, off, w, bad, total=2)


class _NoFill:
    """The library with the fill entry taken out: a wrapper that reached it would fail the test, not touch a device."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name == "ocn_two_hop_sums_fill":
            raise AssertionError("the wrapper reached the library")
        return getattr(self._real, name)


def _tiny():
    from ocn_amd.sparse import SparseTensor
    return SparseTensor.from_edge_index(torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), sparse_sizes=(4, 4))


def test_prefilter_arguments_are_refused_before_the_device(hiplib):
    from ocn_amd import ops, recommend as R
    from ocn_amd.model import predictor_dict
    adj = _tiny()                                                           # on the CPU: reaching a device operand raises OcnHipError
    src = torch.tensor([0, 2])
    pred = predictor_dict["cn5"](8, 8, 1, 3, 0.0).eval()
    h = torch.randn(4, 8)
    top = ops.segment_topk_max_k()
    assert top == 128
    for adj2 in (None, adj):
        with pytest.raises(ValueError, match="fewer than k = 6"):
            R.recommend_links(pred, h, adj, adj2, src, 6, 64, prefilter=("ra", 5))
        with pytest.raises(ValueError, match=f"m must be in 1..{top}"):
            R.recommend_links(pred, h, adj, adj2, src, 3, 64, prefilter=("ra", top + 1))
        with pytest.raises(ValueError, match=f"m must be in 1..{top}"):
            R.recommend_links(pred, h, adj, adj2, src, 1, 64, prefilter=("cn", 0))
        for kind in ("jaccard", "pa", "cn2", "katz"):
            with pytest.raises(ValueError, match=r"no path sum.*'cn', 'aa', 'ra'"):
                R.recommend_links(pred, h, adj, adj2, src, 3, 64, prefilter=(kind, 10))
        for bad in ("ra", ("ra",), ("ra", 10, 1), (10, "ra"), ("ra", 10.0), ("ra", "10"), ("ra", True), 10, {"ra": 10}):
            with pytest.raises(ValueError, match=r"prefilter must be None or \(kind, m\)"):
                R.recommend_links(pred, h, adj, adj2, src, 3, 64, prefilter=bad)
    with pytest.raises(RuntimeError, match="eval path"):
        R.recommend_links(pred.train(), h, adj, None, src, 3, 64, prefilter=("ra", 10))
    pred.eval()
    with pytest.raises(ValueError, match="no path sum"):
        R.two_hop_scored_candidates(adj, src, "jaccard")
    with pytest.raises(ValueError, match="no path sum"):
        R.prefilter_candidates(adj, src, "pa", 5)
    with pytest.raises(ValueError, match="m must be in 1"):
        R.prefilter_candidates(adj, src, "ra", 0)
    with pytest.raises(ValueError, match="sources must be a 1-d int64"):
        R.two_hop_scored_candidates(adj, src.int(), "cn")
    other = type(adj).from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(5, 5))
    with pytest.raises(ValueError, match="known is"):
        R.two_hop_scored_candidates(adj, src, "cn", known=other)
    # valid arguments get as far as the first device operand: there is no CPU path
    for call in (lambda: R.two_hop_scored_candidates(adj, src, "cn"),
                 lambda: R.prefilter_candidates(adj, src, "ra", 5),
                 lambda: R.recommend_links(pred, h, adj, None, src, 3, 64, prefilter=("ra", 3)),
                 lambda: R.recommend_links(pred, h, adj, None, src, 3, 64, prefilter=["cn", top])):
        with pytest.raises(_lib.OcnHipError, match="no CPU path"):
            call()
